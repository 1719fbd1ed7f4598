"""CPU checks behind tests/test_photometric_f64_gpu.py (no GPU, no HIP library):

1. tests/photometric_ref.py, evaluated in float32, agrees with oracle/jp_oracle.py (+ grid_sample) to 1e-6 -- the float64 referee
   states the same operation as the project's oracle;
2. every input condition of the GPU file holds on the float64 reference alone, for every one of its cases and committed seeds;
3. the bars of the GPU file follow from the fp32 oracle's own error against the float64 reference (photometric_cases.BARS).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import jp_oracle as J
from tests import photometric_cases as C
from tests import photometric_ref as R


# ------------------------------------------------------------------------------------------- 1. restatement == oracle in fp32
@pytest.mark.parametrize("B,H,W,hs,ws", [(2, 24, 40, 6, 10), (3, 17, 33, 17, 33)])
def test_restatement_matches_oracle_fp32(B, H, W, hs, ws):
    g = torch.Generator().manual_seed(H)
    K, invK = C.intrinsics(B, H, W)
    aa = (torch.rand(B, 3, generator=g) - 0.5) * 0.06
    tr = (torch.rand(B, 3, generator=g) - 0.5) * 0.2
    disp = torch.rand(B, 1, hs, ws, generator=g) * 0.045 + 0.005
    col = torch.rand(B, 3, H, W, generator=g)
    tgt = torch.rand(B, 3, H, W, generator=g)
    for invert in (False, True):
        T, P = R.pose(aa, tr, K, invert)
        TJ = J.transformation_from_parameters(aa.view(B, 1, 3), tr.view(B, 1, 3), invert)
        assert C.err_abs(T, TJ) <= 1e-6
        w = R.warp(disp, invK, P, col, H, W, C.MIN_DEPTH, C.MAX_DEPTH)
        _, depth = J.disp_to_depth(F.interpolate(disp, [H, W], mode="bilinear", align_corners=False), C.MIN_DEPTH, C.MAX_DEPTH)
        grid = J.project(J.backproject(depth, invK), K, TJ, H, W)
        pj = F.grid_sample(col, grid, mode="bilinear", padding_mode="border", align_corners=False)
        assert C.err_abs(w.pred, pj) <= 1e-6
        # the coordinates the restatement reports are grid_sample's un-normalised ones
        assert C.err_abs(w.ix, ((grid[..., 0] + 1) * W - 1) / 2) <= 1e-6 * W
        assert C.err_abs(w.iy, ((grid[..., 1] + 1) * H - 1) / 2) <= 1e-6 * H
        rl, pre = R.reprojection(w.pred, tgt)
        assert C.err_abs(rl, J.reprojection_loss(pj, tgt)) <= 1e-6
        assert C.err_abs(pre.clamp(0, 1), J.ssim(pj, tgt)) <= 1e-6


def test_min_reprojection_matches_oracle_fp32():
    inp = C.composite_inputs(C.COMP_SEED)
    r32, o = C.composite_reference(inp, torch.float32), C.composite_oracle_fp32(inp)
    for s in range(len(C.COMP_SCALES)):
        assert torch.equal(r32["argmin"][s], o["argmin"][s])
        assert abs(float(r32["loss"][s]) - float(o["loss"][s])) <= 1e-6


# ------------------------------------------------------------------------------------------- 2. input conditions
@functools.lru_cache(maxsize=None)
def _warp_case(shape, regime, frame=0):
    inp = C.warp_inputs(shape, regime, C.WARP_SEEDS[(shape, regime)], frame)
    return inp, C.warp_reference(inp)


@pytest.mark.parametrize("shape,regime", C.WARP_CASES)
def test_warp_conditions(shape, regime):
    inp, ref = _warp_case(shape, regime)
    assert C.warp_conditions(regime, ref, inp["H"], inp["W"]) == []
    assert C.find_warp_seed(shape, regime) == C.WARP_SEEDS[(shape, regime)]       # the committed seed is the first admissible one


def test_two_frame_conditions():
    for frame in (0, 1):
        inp, ref = _warp_case(*C.TWO_FRAME_CASE, frame)
        assert C.warp_conditions(C.TWO_FRAME_CASE[1], ref, inp["H"], inp["W"]) == []


@functools.lru_cache(maxsize=None)
def _ssim_case(H, W):
    x, y, idx, eq = C.ssim_inputs(H, W)
    xr, lr, pre = C.ssim_reference(x, y)
    masked, exact0, eqin = C.ssim_masks(pre, eq)
    return x, y, idx, eq, xr, lr, pre, masked, exact0, eqin


@pytest.mark.parametrize("H,W", C.SSIM_SHAPES)
def test_ssim_conditions(H, W):
    x, y, idx, eq, xr, lr, pre, masked, exact0, eqin = _ssim_case(H, W)
    assert float(masked.double().mean()) <= C.MASK_CAP
    assert torch.equal(x[eq.unsqueeze(1).expand_as(x)], y[eq.unsqueeze(1).expand_as(x)])        # pred == target bit for bit
    assert bool(eqin.any()) and bool((x == 1.0).all(1).any())                                  # the rectangles exist
    # the windows inside the pred == target rectangle sit exactly on the clamp, and the reference gradient under them is 0
    assert float(pre.abs().amax(1)[exact0].max()) <= 1e-12
    idm, runs = C.ssim_weights(idx, masked)
    for cand, wgt, keep in runs:
        assert bool((wgt > 0).any()) and bool(keep.any())                                      # every candidate wins somewhere
        g = C.ssim_grad(xr, lr, wgt)
        assert float(g[eqin.unsqueeze(1).expand_as(g)].abs().max()) <= 1e-10 * float(g.abs().max())


def test_composite_conditions():
    assert C.composite_conditions(C.composite_reference(C.composite_inputs(C.COMP_SEED))) == []
    assert C.find_composite_seed() == C.COMP_SEED


def test_pose_inputs():
    aa, tr, K, dP = C.pose_inputs()
    got = aa.double().norm(dim=1)
    assert float(got[0]) == 0.0
    for a, want in zip(got[1:], C.POSE_ANGLES[1:]):
        assert abs(float(a) - want) <= 1e-6 * want
    for invert in (False, True):                 # the reference is finite in every regime, and its axis-angle gradient at 0 is 0
        T, P, da, dt = C.pose_reference(aa, tr, K, dP, invert)
        assert all(bool(torch.isfinite(t).all()) for t in (T, P, da, dt))
        assert float(da[0].abs().max()) == 0.0 and float(da[1:].abs().amin(1).min()) > 0.0


# ------------------------------------------------------------------------------------------- 3. bars from the fp32 oracle's error
def _oracle_errors():
    """largest error of the fp32 CPU oracle against the float64 reference per asserted quantity: same inputs, masks and metrics as
    the GPU tests"""
    e = {k: 0.0 for k in C.ORACLE_ERR}

    def up(k, v):
        e[k] = max(e[k], v)

    aa, tr, K, dP = C.pose_inputs()
    for invert in (False, True):
        T, P, da, dt = C.pose_reference(aa, tr, K, dP, invert)
        TJ = J.transformation_from_parameters(aa.view(-1, 1, 3), tr.view(-1, 1, 3), invert)
        up("pose_T", C.err_abs(TJ, T))
        up("pose_P", C.err_max(torch.matmul(K, TJ)[:, :3], P))
        _, _, da32, dt32 = C.pose_reference(aa, tr, K, dP, invert, torch.float32)
        up("pose_grad", max(C.err_max(da32, da), C.err_max(dt32, dt)))
    for shape, regime in C.WARP_CASES:
        inp, ref = _warp_case(shape, regime)
        o = C.warp_oracle_fp32(inp, ref["mask"])
        keep = ~ref["mask"].unsqueeze(1)
        up("warp_pred", C.err_abs(o["pred"], ref["pred"], keep.expand_as(ref["pred"])))
        up("warp_ddisp_up", C.err_rms(o["ddisp_up"], ref["ddisp_up"], keep))
        up("warp_dP", C.err_max(o["dP"], ref["dP"]))
    two = [_warp_case(*C.TWO_FRAME_CASE, f) for f in (0, 1)]
    os_ = [C.warp_oracle_fp32(inp, ref["mask"]) for inp, ref in two]
    keep = ~(two[0][1]["mask"] | two[1][1]["mask"]).unsqueeze(1)
    up("warp_ddisp_up", C.err_rms(os_[0]["ddisp_up"] + os_[1]["ddisp_up"], two[0][1]["ddisp_up"] + two[1][1]["ddisp_up"], keep))
    for H, W in C.SSIM_SHAPES:
        x, y, idx, eq, xr, lr, pre, masked, exact0, eqin = _ssim_case(H, W)
        x32 = x.clone().requires_grad_(True)
        l32 = J.reprojection_loss(x32, y)
        up("ssim_fwd", C.err_abs(l32.squeeze(1), lr.squeeze(1), ~masked))
        for cand, wgt, keep in C.ssim_weights(idx, masked)[1]:
            gr = C.ssim_grad(xr, lr, wgt)
            up("ssim_bwd", C.err_rms(C.ssim_grad(x32, l32, wgt.float()), gr, keep.unsqueeze(1).expand_as(gr)))
    inp = C.composite_inputs(C.COMP_SEED)
    ref, o = C.composite_reference(inp), C.composite_oracle_fp32(inp)
    for s in range(len(C.COMP_SCALES)):
        up("comp_loss", C.err_max(o["loss"][s], ref["loss"][s]))
        up("comp_ddisp", C.err_max(o["ddisp"][s], ref["ddisp"][s]))
    for j in range(2):
        up("comp_daa", C.err_max(o["daa"][j], ref["daa"][j]))
        up("comp_dtr", C.err_max(o["dtr"][j], ref["dtr"][j]))
    return e


def test_bars_follow_from_the_oracle_error():
    measured = _oracle_errors()
    for k, v in measured.items():
        print(f"{k:14s} fp32 oracle error {v:.3e}  recorded {C.ORACLE_ERR[k]:.2e}  bar {C.BARS[k]:.0e}")
    for k, v in measured.items():
        # the recorded figures reproduce (25 % of room for another CPU's vector width and libm)
        assert v <= 1.25 * C.ORACLE_ERR[k], k
    for k, bar in C.BARS.items():
        rule = C.round_up_1sig(8 * C.ORACLE_ERR[k])
        if k in C.BAR_EXCEPTIONS:
            assert bar <= rule, k                      # an exception may only be tighter than the rule
        else:
            assert bar == pytest.approx(rule, rel=1e-9), k
    for k in ("warp_ddisp_up", "warp_dP", "ssim_bwd", "comp_ddisp", "comp_daa", "comp_dtr", "pose_grad"):
        assert C.BARS[k] <= 2e-2 / 20, k               # every gradient: at least 20 x tighter than the old 2e-2
