"""The loss kernels (jperceiver_amd/csrc/losses.hip) and the min-reprojection reduction of photometric.hip per element against FLOAT64
references (tests/losses_ref.py under autograd on the CPU), at the smallest shapes that put each kernel on the path the training step
runs: several workgroups with a ragged last one, and a capped grid whose threads stride with a ragged tail (tests/losses_cases.py
holds the thresholds next to the launch expressions; tests/test_losses_ref_cpu.py checks them, and every condition below, without a
GPU).  Everything runs through ops_loss (smooth_loss, scale_loss, layout_loss, signed_distance, l1_loss) or _lib.call (jp_row_sum,
jp_minreproj_fwd); every loss slot has the upstream gradient 0.7; one case per backward kernel also adds onto a seeded buffer.

The operations are piecewise (the sign of a stencil or a residual, the depth clamp).  The elements whose branch fp32 rounding could
decide are taken out by the float64 reference alone, before a kernel runs:

  smoothness     a stencil of the normalised disparity with 0 < |s| < 1e-6 is ambiguous (an exact 0 is not: the flat rectangle is 0
                 in any precision and sgn(0) = 0 decides its gradient); the pixels it reads are left out of the gradient comparison
  scale loss     a valid label pixel with |pred - gt| < 1e-4 gt, or pred within 1e-3 of 80 or 1e-6 of 1e-3, is ambiguous; the
                 disparity pixels it interpolates from are left out.  Disparity pixels no valid label pixel reads must be exactly 0
  min-reproj.    nothing can be masked: each committed seed keeps every argmin margin above 1e-6 outside the deliberate ties

At most 0.5 % of a case may be masked.  Masked shares of the committed cases: smoothness 1x513x515 7.6e-6 (the two pixels of one
stencil), every other smoothness case 0; scale loss 352x312->131x380 3.6e-5 of the disparity pixels, every other scale case 0.

Bars.  For every asserted quantity the error of the project's fp32 CPU oracle (oracle/jp_oracle.py, float32) against the float64
reference was measured on the same cases, masks and metric; the bar is 8 x the largest such error over the cases, rounded up to one
significant digit.  No hardware-intrinsic allowance is added.

  quantity         metric                  fp32 oracle   bar      held to before (test_kernels_gpu.py)
  smoothness loss  |err| / |ref|           6.39e-8       6e-7     2e-4
  smoothness grad  max |err| / max |ref|   3.05e-7       3e-6     5e-4
  scale loss       |err| / |ref|           4.50e-7       4e-6     2e-4
  scale grad       max |err| / max |ref|   4.79e-5       4e-4     1e-3
  layout loss      |err| / |ref|           1.03e-7       9e-7     2e-4
  layout grad      max |err| / max |ref|   4.38e-7       4e-6     5e-4
  L1 loss          |err| / |ref|           5.04e-8       5e-7     1e-4
  L1 grad          max |err| / max |ref|   8.02e-9       7e-8     1e-4

  derived, not measured:
  signed distance  round(sdf^2) equals the integer squared distance; sign and boundary zeros exact; |sdf| within 1 fp32 ulp of sqrt
  row sum          |err| <= n 2^-53 sum |x| against the exactly rounded sum (any order of a double summation; the output is a double)
  min-reproj. sum  the same bound, plus sum |fma(noise, 1e-5f, c) - (c + fl(noise 1e-5f))| over the winners: a compiler may contract
                   the documented c + noise * 1e-5f into one rounding.  min_index is compared exactly.

Every test prints its figures before it asserts them (pytest -s).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops_loss                                            # noqa: E402
from jperceiver_amd._lib import call                                           # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                            # noqa: E402
from tests import losses_cases as C                                            # noqa: E402
from tests import losses_ref as R                                              # noqa: E402

DEV = "cuda"
BARS = C.BARS


def _check(figures):
    """figures: [(label, error, bar key)...] -- print all, then assert all"""
    for label, err, key in figures:
        print(f"  {label:34s} {err:.3e}   bar {BARS[key]:.0e}")
    bad = [f"{label}: {err:.3e} > {BARS[key]:.0e}" for label, err, key in figures if not err <= BARS[key]]
    assert not bad, "; ".join(bad)


def _run(record, leaves, seeded=None):
    """record(lv) the op under `recording`, set the slot's upstream gradient, run backward.  seeded: {leaf index: buffer} placed into
    the leaf's gradient before backward (add mode).  -> loss value (1,) on the CPU"""
    lv = ops_loss.LossVec(["s"], DEV)
    tape = Tape()
    with recording(tape):
        record(lv)
    lv.grads.fill_(C.GOUT)
    for i, buf in (seeded or {}).items():
        leaves[i].g = buf.to(DEV).clone()
    tape.backward()
    return lv.vals.cpu()


# ------------------------------------------------------------------------------------------- smoothness
@pytest.mark.parametrize("name,add", [(n, False) for n in C.SMOOTH_CASES] + [(C.SMOOTH_ADD_CASE, True)])
def test_smooth_loss_f64(name, add):
    disp, img = C.smooth_inputs(name)
    ref = C.smooth_reference(name)
    dv, imgd = Var(disp.to(DEV), True), img.to(DEV)
    seed = C.seeded_like(ref["grad"], 11) if add else None
    val = _run(lambda lv: ops_loss.smooth_loss(lv, "s", dv, imgd, C.SMOOTH_WEIGHT), [dv], {0: seed} if add else None)
    want = ref["grad"] + seed.double() if add else ref["grad"]
    got = dv.g.cpu()
    print(f"  ambiguous stencils {ref['ambiguous']}, exactly zero {ref['zeros']}, masked share {1 - float(ref['keep'].double().mean()):.2e}")
    assert bool(torch.isfinite(got).all())
    _check([("loss", C.err_rel(val, ref["loss"]), "smooth_loss"),
            ("ddisp / max" + (" (add mode)" if add else ""),
             float((got.double() - want).abs()[ref["keep"]].max() / ref["grad"].abs().max()), "smooth_grad")])


# ------------------------------------------------------------------------------------------- scale loss
@pytest.mark.parametrize("name,add", [(n, False) for n in C.SCALE_CASES] + [(C.SCALE_ADD_CASE, True)])
def test_scale_loss_f64(name, add):
    disp, label, crop = C.scale_inputs(name)
    ref = C.scale_reference(name)
    dv, labd = Var(disp.to(DEV), True), label.to(DEV)
    seed = C.seeded_like(ref["grad"], 12) if add else None
    val = _run(lambda lv: ops_loss.scale_loss(lv, "s", dv, labd, C.SCALE_WEIGHT, C.MIN_DEPTH, C.MAX_DEPTH, crop), [dv],
               {0: seed} if add else None)
    got = dv.g.cpu()
    print(f"  valid {ref['nvalid']}, pred < gt {ref['below']:.3f}, clamped at 80 {ref['clamped']:.3f}, masked share "
          f"{1 - float(ref['keep'].double().mean()):.2e}, disparity pixels read {float(ref['reached'].double().mean()):.4f}")
    assert bool(torch.isfinite(got).all())
    if ref["nvalid"] == 0:                       # no valid pixel: the loss is 0 / 0 as the oracle's mean of nothing, the gradient exactly 0
        assert bool(torch.isnan(val).all()) and float(got.abs().max()) == 0.0
        return
    unread = ~ref["reached"]
    if not add and bool(unread.any()):
        assert float(got[unread].abs().max()) == 0.0, "a disparity pixel that no valid label pixel reads got a gradient"
    want = ref["grad"] + seed.double() if add else ref["grad"]
    _check([("loss", C.err_rel(val, ref["loss"]), "scale_loss"),
            ("ddisp / max" + (" (add mode)" if add else ""),
             float((got.double() - want).abs()[ref["keep"]].max() / ref["grad"].abs().max()), "scale_grad")])


# ------------------------------------------------------------------------------------------- layout loss
@pytest.mark.parametrize("shape,region,wk,with_sdf,add", [c + (False,) for c in C.LAYOUT_CASES] + [C.LAYOUT_ADD_CASE + (True,)])
def test_layout_loss_f64(shape, region, wk, with_sdf, add):
    logits, label, sdf = C.layout_inputs(shape)
    ref = C.layout_reference(shape, region, wk, with_sdf)
    lw, cew, l2w = C.LAYOUT_WEIGHTS[wk]
    zv, labd = Var(logits.to(DEV), True), label.to(DEV)
    sdfd = sdf.float().to(DEV) if with_sdf else None
    seed = C.seeded_like(ref["grad"], 13) if add else None
    val = _run(lambda lv: ops_loss.layout_loss(lv, "s", zv, labd, sdfd, C.LAYOUT_W0, C.LAYOUT_W1, lw, cew, l2w, region), [zv],
               {0: seed} if add else None)
    want = ref["grad"] + seed.double() if add else ref["grad"]
    got = zv.g.cpu()
    assert bool(torch.isfinite(got).all())
    _check([("loss", C.err_rel(val, ref["loss"]), "layout_loss"),
            ("dlogits / max" + (" (add mode)" if add else ""), float((got.double() - want).abs().max() / ref["grad"].abs().max()),
             "layout_grad")])


# ------------------------------------------------------------------------------------------- signed distance
@pytest.mark.parametrize("name", C.SDF_CASES)
def test_signed_distance_exact(name):
    m = C.sdf_inputs(name)
    ref = R.signed_distance(m)
    got = ops_loss.signed_distance(m.to(DEV)).cpu()
    assert bool(torch.isfinite(got).all())
    d2 = torch.round(got.double() ** 2).long()
    want = ref.d2 * ref.sign.abs()                               # the boundary zeros and the empty image are 0
    rt = want.double().sqrt().float()                            # the correctly rounded fp32 root
    ulp = (torch.nextafter(rt, torch.full_like(rt, float("inf"))) - rt).double()
    off = ((got.abs().double() - rt.double()).abs() / ulp).max()
    print(f"  largest distance {float(ref.sdf.abs().max()):.2f}, wrong squared distances {int((d2 != want).sum())}, "
          f"wrong signs {int((torch.sign(got).long() != ref.sign).sum())}, |sdf| off the rounded root by {float(off):.2f} ulp")
    assert torch.equal(d2, want)
    assert torch.equal(torch.sign(got).long(), ref.sign)
    assert float(off) <= 1.0


# ------------------------------------------------------------------------------------------- L1
@pytest.mark.parametrize("run", C.L1_RUNS)
def test_l1_loss_f64(run):
    a, b = C.l1_inputs()
    ref = C.l1_reference()
    av, bv = Var(a.to(DEV), run != "db"), Var(b.to(DEV), run != "da")
    seeded = {0: C.seeded_like(ref["da"], 14), 1: C.seeded_like(ref["db"], 15)} if run == "add" else None
    val = _run(lambda lv: ops_loss.l1_loss(lv, "s", av, bv), [av, bv], seeded)
    figs = [("loss", C.err_rel(val, ref["loss"]), "l1_loss")]
    lo, hi = C.L1_EQUAL
    for i, (v, key) in enumerate(((av, "da"), (bv, "db"))):
        if not v.rg:
            assert v.g is None
            continue
        got = v.g.cpu()
        if run == "add":
            # fp32 cannot hold seed + gradient more finely than an ulp of the seed, so the sum is compared to the fp32 sum of the seed and
            # the reference gradient rounded to fp32 (the kernel's constant is within the bar of it, as the other runs assert)
            want = (seeded[i] + ref[key].float()).double()
            figs.append((f"{key} / max (add mode)", float((got.double() - want).abs().max() / ref[key].abs().max()), "l1_grad"))
        else:
            assert float(got[lo:hi].abs().max()) == 0.0, "a == b must give exactly 0"
            figs.append((f"{key} / max", C.err_max(got, ref[key]), "l1_grad"))
    _check(figs)


# ------------------------------------------------------------------------------------------- row sum
@pytest.mark.parametrize("rows,cols", C.ROW_SUM_CASES)
def test_row_sum_f64(rows, cols):
    x = C.row_sum_inputs(rows, cols)
    out = torch.full((rows,), float("nan"), device=DEV, dtype=torch.float64)
    call("jp_row_sum", x.to(DEV), out, rows, cols)
    out = out.cpu()
    for r in range(rows):
        err, bound = abs(float(out[r]) - R.exact_sum(x[r])), C.double_sum_bound(cols, float(x[r].double().abs().sum()))
        print(f"  row {r}: |err| {err:.3e}   bound {bound:.3e}")
    for r in range(rows):
        assert abs(float(out[r]) - R.exact_sum(x[r])) <= C.double_sum_bound(cols, float(x[r].double().abs().sum()))


# ------------------------------------------------------------------------------------------- min-reprojection
@pytest.mark.parametrize("ncand,noise", list(C.MINREPROJ_SEEDS))
def test_minreproj_f64(ncand, noise):
    c, nz, _ = C.minreproj_inputs(ncand, noise, C.MINREPROJ_SEEDS[(ncand, noise)])
    ref = C.minreproj_reference(ncand, noise)
    n = C.MINREPROJ_N
    cd = [t.to(DEV) for t in c] + [None] * (4 - ncand)           # c3, then c2, absent: NULL
    nd = [t.to(DEV) for t in nz] + [None] * (2 - len(nz))
    idx = torch.full((n,), -1, device=DEV, dtype=torch.int64)
    acc = torch.full((1,), float("nan"), device=DEV, dtype=torch.float64)
    call("jp_minreproj_fwd", cd[0], cd[1], cd[2], cd[3], nd[0], nd[1], idx, acc, n)
    idx, got = idx.cpu(), float(acc.cpu())
    err, bound = abs(got - ref.total), C.double_sum_bound(n, ref.sum_abs) + ref.fma_slack
    print(f"  wrong argmin {int((idx != ref.argmin).sum())} of {n}, smallest margin {float(ref.margin.min()):.2e}, sum |err| {err:.3e}   "
          f"bound {bound:.3e} (of which a fused multiply-add may take {ref.fma_slack:.3e})")
    assert torch.equal(idx, ref.argmin)
    assert err <= bound
