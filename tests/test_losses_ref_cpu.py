"""CPU checks behind tests/test_losses_f64_gpu.py (no GPU, no HIP library):

1. tests/losses_ref.py agrees with oracle/jp_oracle.py evaluated in float64 to 1e-12 -- the referee states the project's operations;
2. every input condition of the GPU file holds on the float64 reference alone: mask caps, both residual signs and clamped pixels in
   every scale case, exact-zero stencils in the flat rectangle, the min-reprojection margins and shares;
3. every case built for a launch path lies on it, by the grid expressions as they stand in the kernel sources;
4. the bars of the GPU file follow from the fp32 oracle's own error against the float64 reference (losses_cases.BARS).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import jp_oracle as J
from tests import losses_cases as C
from tests import losses_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


# ------------------------------------------------------------------------------------------- 1. restatement == oracle in float64
@pytest.mark.parametrize("name", list(C.SMOOTH_CASES))
def test_smooth_matches_oracle_f64(name):
    ref = C.smooth_reference(name)
    loss, grad = C.smooth_oracle(name, F64)
    assert _rel(ref["loss"], loss) <= 1e-12
    assert C.err_max(ref["grad"], grad) <= 1e-12


@pytest.mark.parametrize("name", [n for n, c in C.SCALE_CASES.items() if c[6] != "empty"])
def test_scale_matches_oracle_f64(name):
    ref = C.scale_reference(name)
    loss, grad = C.scale_oracle(name, F64)
    assert _rel(ref["loss"], loss) <= 1e-12
    assert C.err_max(ref["grad"], grad) <= 1e-12


def test_scale_empty_case_is_nan_with_zero_gradient():
    ref = C.scale_reference("64x96->64x96 empty")
    loss, _ = C.scale_oracle("64x96->64x96 empty", F64)
    assert ref["nvalid"] == 0 and bool(torch.isnan(ref["loss"])) and bool(torch.isnan(loss))
    assert float(ref["grad"].abs().max()) == 0.0


@pytest.mark.parametrize("shape,region,wk,with_sdf", [c for c in C.LAYOUT_CASES if c[0] != "513x512"])
def test_layout_matches_oracle_f64(shape, region, wk, with_sdf):
    ref = C.layout_reference(shape, region, wk, with_sdf)
    loss, grad = C.layout_oracle(shape, region, wk, with_sdf, F64)
    assert _rel(ref["loss"], loss) <= 1e-12
    assert C.err_max(ref["grad"], grad) <= 1e-12


@pytest.mark.parametrize("name", C.SDF_CASES)
def test_signed_distance_matches_oracle(name):
    m = C.sdf_inputs(name)
    ref = R.signed_distance(m)
    oh = torch.cat([1 - m, m], 1).numpy()
    got = torch.from_numpy(J.compute_sdf(oh)[:, 1])
    assert float((ref.sdf - got).abs().max()) <= 1e-12
    some = m[:, 0].amax((1, 2)) > 0.5                                     # an image without foreground is all zero
    assert bool((ref.sign[some][m[some, 0] < 0.5] == 1).all()) and bool((ref.sign[m[:, 0] > 0.5] <= 0).all())
    if name == "130x300":
        assert int(m[1].sum()) == 1 and int(m[2].sum()) == 0 and bool((m[3] == 1).all())
        assert float(ref.sdf[2].abs().max()) == 0.0
        assert int(ref.d2[3, 4, 3]) == 5 * 5 + 3 * 3                     # the phantom site (-1, 0)
        assert int(ref.d2[1, 0, 0]) == 129 ** 2 + 299 ** 2
    if name == "257x258":
        assert float(ref.sdf.max()) > 60.0


def test_l1_and_sums():
    ref, o = C.l1_reference(), C.l1_reference(torch.float32)
    assert _rel(o["loss"], ref["loss"]) <= 1e-6
    lo, hi = C.L1_EQUAL
    assert float(ref["da"][lo:hi].abs().max()) == 0.0 and float(ref["db"][lo:hi].abs().max()) == 0.0
    x = torch.tensor([1e8, 1.0, -1e8, 1e-8], dtype=torch.float32)
    assert R.exact_sum(x) == float(np.float32(1.0)) + float(np.float32(1e-8))


# ------------------------------------------------------------------------------------------- 2. input conditions
@pytest.mark.parametrize("name", list(C.SMOOTH_CASES))
def test_smooth_conditions(name):
    ref = C.smooth_reference(name)
    masked = 1 - float(ref["keep"].double().mean())
    print(f"smooth {name}: {ref['ambiguous']} ambiguous stencils, {ref['zeros']} exactly zero, masked share {masked:.5f}")
    assert masked <= C.MASK_CAP
    B, h, w = C.SMOOTH_CASES[name]
    if name != "2x3x3":        # its rectangle is a single pixel
        assert ref["zeros"] > 0
    disp, img = C.smooth_inputs(name)
    assert img.shape == (B, 3, h, w)


@pytest.mark.parametrize("name", list(C.SCALE_CASES))
def test_scale_conditions(name):
    ref = C.scale_reference(name)
    masked = 1 - float(ref["keep"].double().mean())
    print(f"scale {name}: valid {ref['nvalid']}, pred<gt {ref['below']:.3f}, pred>gt {ref['above']:.3f}, clamped {ref['clamped']:.3f}, "
          f"ambiguous label px {ref['ambiguous']:.5f}, masked disparity px {masked:.5f}, reached {float(ref['reached'].double().mean()):.4f}")
    assert masked <= C.MASK_CAP
    if C.SCALE_CASES[name][6] == "empty":
        assert ref["nvalid"] == 0
        return
    assert ref["below"] >= 0.1 and ref["above"] >= 0.1 and ref["clamped"] >= 0.01
    assert float(ref["grad"][~ref["reached"]].abs().max() if bool((~ref["reached"]).any()) else 0.0) == 0.0
    if name == "728x724->90x110":
        assert float((~ref["reached"]).double().mean()) > 0.9


@pytest.mark.parametrize("ncand,noise", list(C.MINREPROJ_SEEDS))
def test_minreproj_conditions(ncand, noise):
    ref = C.minreproj_reference(ncand, noise)
    share = torch.bincount(ref.argmin, minlength=ncand).double() / ref.argmin.numel()
    print(f"minreproj {ncand} candidates, noise {noise}: smallest margin {float(ref.margin.min()):.3e}, shares {share.tolist()}")
    assert float(ref.margin.min()) > C.MINREPROJ_MARGIN
    assert float(share.min()) >= C.MINREPROJ_WIN
    c, nz, partner = C.minreproj_inputs(ncand, noise, C.MINREPROJ_SEEDS[(ncand, noise)])
    lo, hi = C.MINREPROJ_TIE01
    assert torch.equal(c[0][lo:hi], c[1][lo:hi]) and bool((ref.argmin[lo:hi] == 0).all())       # bit-equal: the first wins
    if ncand == 4:
        lo, hi = C.MINREPROJ_TIE23
        assert torch.equal(c[2][lo:hi], c[3][lo:hi]) and bool((ref.argmin[lo:hi] == 2).all())
    assert C.find_minreproj_seed(ncand, noise) == C.MINREPROJ_SEEDS[(ncand, noise)]              # the first admissible seed


def test_the_checks_would_notice_a_dropped_element_or_gate():
    """What a subtly wrong kernel would change, stated on the references: each is far outside the bar that guards it."""
    for rows, cols in C.ROW_SUM_CASES:                            # one element left out of a row sum
        x = C.row_sum_inputs(rows, cols)
        for r in range(rows):
            assert float(x[r, -1].abs()) > 100 * C.double_sum_bound(cols, float(x[r].double().abs().sum()))
    for key in C.MINREPROJ_SEEDS:                                 # the last pixel left out of the sum of minima
        ref = C.minreproj_reference(*key)
        c, nz, _ = C.minreproj_inputs(*key, C.MINREPROJ_SEEDS[key])
        last = min(float(t[-1]) for t in c)
        assert last - 1e-4 > 100 * (C.double_sum_bound(C.MINREPROJ_N, ref.sum_abs) + ref.fma_slack)
    for name, case in C.SCALE_CASES.items():                      # the clamp passing a gradient above 80
        if case[6] == "empty":
            continue
        disp, label, crop = C.scale_inputs(name)
        d = disp.double().requires_grad_(True)
        depth = 1 / (1 / C.MAX_DEPTH + (1 / C.MIN_DEPTH - 1 / C.MAX_DEPTH) * d)
        pr = F.interpolate(depth, label.shape[2:], mode="bilinear", align_corners=False)
        ref = C.scale_reference(name)
        v, lab = pr.detach() > 80, label.double()
        v = v & (lab > 0)
        if crop is not None:
            inside = torch.zeros_like(v)
            inside[:, :, crop[0]:crop[1], crop[2]:crop[3]] = True
            v = v & inside
        (C.SCALE_WEIGHT * C.GOUT * (pr / lab.clamp(min=1e-30))[v].sum() / ref["nvalid"]).backward()      # what the gate holds back
        assert float(d.grad.abs().max() / ref["grad"].abs().max()) > 10 * C.BARS["scale_grad"], name


# ------------------------------------------------------------------------------------------- 3. launch paths
def test_grid_expressions_stand_in_the_sources():
    text = {}
    for kernel, (path, expr, per_wg, cap) in C.GRIDS.items():
        if path not in text:
            with open(os.path.join(ROOT, path)) as f:
                text[path] = f.read()
            assert C.TPB_LINE in text[path], path
        assert expr in text[path], f"{kernel}: the launch grid in {path} changed; update losses_cases.GRIDS and its cases"


@pytest.mark.parametrize("case", list(C.PATHS))
def test_cases_take_their_paths(case):
    for kernel, n, path in C.PATHS[case]:
        _, _, per_wg, cap = C.GRIDS[kernel]
        if path.startswith("strided"):
            assert n > C.stride_threshold(kernel) and n % C.stride_threshold(kernel) != 0, (case, kernel)      # strides, with a tail
        else:
            assert C.workgroups(kernel, n) > 1 and (cap is None or n <= C.stride_threshold(kernel)), (case, kernel)
        assert path.endswith("aligned") or n % per_wg != 0, (case, kernel)                      # a ragged last workgroup


# ------------------------------------------------------------------------------------------- 4. bars from the fp32 oracle's error
def _oracle_errors():
    e = {k: 0.0 for k in C.ORACLE_ERR}
    per_case = []

    def up(k, v, case):
        e[k] = max(e[k], v)
        per_case.append((k, case, v))

    for name in C.SMOOTH_CASES:
        ref = C.smooth_reference(name)
        loss, grad = C.smooth_oracle(name)
        up("smooth_loss", C.err_rel(loss, ref["loss"]), name)
        up("smooth_grad", C.err_max_kept(grad, ref["grad"], ref["keep"]), name)
    for name, case in C.SCALE_CASES.items():
        if case[6] == "empty":
            continue
        ref = C.scale_reference(name)
        loss, grad = C.scale_oracle(name)
        up("scale_loss", C.err_rel(loss, ref["loss"]), name)
        up("scale_grad", C.err_max_kept(grad, ref["grad"], ref["keep"]), name)
    for case in C.LAYOUT_CASES:
        ref = C.layout_reference(*case)
        loss, grad = C.layout_oracle(*case)
        up("layout_loss", C.err_rel(loss, ref["loss"]), case)
        up("layout_grad", C.err_max(grad, ref["grad"]), case)
    ref, o = C.l1_reference(), C.l1_reference(torch.float32)
    up("l1_loss", C.err_rel(o["loss"], ref["loss"]), "l1")
    up("l1_grad", max(C.err_max(o["da"], ref["da"]), C.err_max(o["db"], ref["db"])), "l1")
    return e, per_case


def test_bars_follow_from_the_oracle_error():
    measured, per_case = _oracle_errors()
    for k, case, v in per_case:
        print(f"{k:12s} {str(case):44s} fp32 oracle error {v:.3e}")
    for k, v in measured.items():
        print(f"{k:12s} fp32 oracle error {v:.3e}  recorded {C.ORACLE_ERR[k]:.2e}  bar {C.BARS[k]:.0e}")
    for k, v in measured.items():
        # the recorded figures reproduce (25 % of room for another CPU's vector width and libm)
        assert v <= 1.25 * C.ORACLE_ERR[k], k
    for k, bar in C.BARS.items():
        if k in C.BAR_NOTES:
            continue                                   # derived next to the bar in losses_cases.py
        assert bar == pytest.approx(C.round_up_1sig(8 * C.ORACLE_ERR[k]), rel=1e-9), k
    for k, bar in C.BARS.items():
        assert bar <= C.FORMER_BARS[k], k              # never looser than tests/test_kernels_gpu.py
