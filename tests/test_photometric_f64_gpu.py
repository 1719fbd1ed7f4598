"""The view-synthesis + photometric loss kernels (jperceiver_amd/csrc/photometric.hip) per element against a FLOAT64 reference
(tests/photometric_ref.py under autograd on the CPU): the pose, the CGT warp forward / backward, SSIM+L1 forward / backward and the
min-reprojection composite of ops_loss.

The operations are piecewise (floor and border clip of the sampling coordinate, the SSIM clamp).  As kink_act does for activations,
the elements whose branch the fp32 rounding could decide are taken out -- but here the decision comes from the float64 reference
alone, before a kernel runs (tests/photometric_cases.py; tests/test_photometric_ref_cpu.py checks the same conditions without a GPU):

  lattice mask   pixels whose float64 ix (iy) lies within 3e-3 of an integer in [0, W-1] ([0, H-1]), the two clip borders included,
                 are left out of per-pixel comparisons, and the upstream gradient is zeroed there on both sides, so that they
                 contribute to no aggregated output either.  At most 2 % of a case.
  clamp mask     windows whose float64 pre-clamp SSIM value lies within 1e-5 of 0 or 1 weigh 0 on both sides (their min_index is
                 set to a value that matches no candidate).  At most 2 %.  The windows inside the pred == target rectangle are
                 exactly 0 and are NOT masked: their derivative is 0 on either side of the gate, and the device gradient is asserted
                 to be 0 (under the same bar) on the pixels at least 2 inside that rectangle.
  composite      nothing can be masked per pixel, so the committed seed keeps every coordinate 1e-3 from a lattice line, every argmin
                 margin above 1e-5, every SSIM value 1e-5 from the clamp, and lets each of the four candidates win >= 2 %.

Bars.  For every asserted quantity the error of the project's fp32 CPU oracle against the float64 reference was measured on the same
inputs, masks and metric; the bar is 8 x the largest such error over the cases, rounded up to one significant digit.

  quantity        metric                  fp32 oracle   bar      note
  pose T          max |err|               1.88e-7       2e-6
  pose P          max |err| / max |ref|   1.72e-7       2e-6
  pose gradients  max |err| / max |ref|   1.47e-5       3e-7     tighter than the rule: jp_pose_bwd runs in double, it owes only the
                                                                 rounding of its fp32 outputs (5 x 2^-24)
  warp pred       max |err|               6.76e-5       6e-4
  warp ddisp_up   max |err| / rms(ref)    2.56e-4       1e-3     tighter than the rule (3e-3): 20 x under the former 2e-2
  warp dP         max |err| / max |ref|   9.74e-6       8e-5
  ssim+l1 fwd     max |err|               2.48e-5       2e-4
  ssim+l1 bwd     max |err| / rms(ref)    6.23e-4       1e-3     tighter than the rule (5e-3), for the same reason; the oracle's own
                                                                 error here is variance cancellation in the flat and saturated
                                                                 rectangles (E[x^2] - mu^2 against C2 = 9e-4)
  composite loss  |err| / |ref|           1.36e-7       2e-6
  composite ddisp max |err| / max |ref|   4.62e-5       4e-4
  composite d_aa  max |err| / max |ref|   5.96e-6       5e-5
  composite d_tr  max |err| / max |ref|   4.25e-6       4e-5

Every test prints its figures before it asserts them (pytest -s).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops_loss                                            # noqa: E402
from jperceiver_amd._lib import call                                           # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                            # noqa: E402
from tests import photometric_cases as C                                       # noqa: E402

DEV = "cuda"
BARS = C.BARS


def _check(figures):
    """figures: [(label, error, bar key)...] -- print all, then assert all"""
    for label, err, key in figures:
        print(f"  {label:34s} {err:.3e}   bar {BARS[key]:.0e}")
    bad = [f"{label}: {err:.3e} > {BARS[key]:.0e}" for label, err, key in figures if not err <= BARS[key]]
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------- (a) pose alone
@pytest.mark.parametrize("invert", [False, True])
def test_pose_f64(invert):
    aa, tr, K, dP = C.pose_inputs()
    B = aa.shape[0]
    Tr, Pr, dar, dtr = C.pose_reference(aa, tr, K, dP, invert)
    aad, trd, Kd = aa.to(DEV), tr.to(DEV), K.to(DEV)
    T, P = torch.empty(B, 4, 4, device=DEV), torch.empty(B, 3, 4, device=DEV)
    call("jp_pose_fwd", aad, trd, Kd, T, P, B, int(invert))
    da, dt = torch.full((B, 3), float("nan"), device=DEV), torch.full((B, 3), float("nan"), device=DEV)
    call("jp_pose_bwd", dP.to(DEV), aad, trd, Kd, da, dt, B, int(invert), 0)
    da, dt = da.cpu(), dt.cpu()
    assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(dt).all())
    assert float(da[0].abs().max()) == 0.0                                     # |axisangle| = 0: the explicit branch
    figs = [("cam_T_cam", C.err_abs(T.cpu(), Tr), "pose_T"), ("P", C.err_max(P.cpu(), Pr), "pose_P")]
    for b, th in enumerate(C.POSE_ANGLES):       # every regime against the launch's largest gradient, and a row of its own
        figs.append((f"d_axisangle |aa|={th:g}", float((da[b].double() - dar[b]).abs().max() / dar.abs().max()), "pose_grad"))
        figs.append((f"d_translation |aa|={th:g}", float((dt[b].double() - dtr[b]).abs().max() / dtr.abs().max()), "pose_grad"))
    _check(figs)


# ------------------------------------------------------------------------------------------- (b) warp forward and backward
@functools.lru_cache(maxsize=None)
def _warp_case(shape, regime, frame=0):
    inp = C.warp_inputs(shape, regime, C.WARP_SEEDS[(shape, regime)], frame)
    ref = C.warp_reference(inp)
    assert C.warp_conditions(regime, ref, inp["H"], inp["W"]) == []
    return inp, ref


def _warp_device(inp, go, dup, accumulate):
    """-> pred, dP (fresh double buffer); dup is written (accumulate 0) or added to (1)"""
    B, H, W, hs, ws = (inp[k] for k in ("B", "H", "W", "hs", "ws"))
    d, iK, P, col = (inp[k].to(DEV).contiguous() for k in ("disp", "invK", "P", "color"))
    pred = torch.full((B, 3, H, W), float("nan"), device=DEV)
    call("jp_cgt_warp_fwd", d, hs, ws, iK, P, col, pred, B, H, W, C.MIN_DEPTH, C.MAX_DEPTH)
    dP = torch.zeros(B, 12, device=DEV, dtype=torch.float64)
    call("jp_cgt_warp_bwd", go.to(DEV).contiguous(), d, hs, ws, iK, P, col, dup, dP, B, H, W, C.MIN_DEPTH, C.MAX_DEPTH, accumulate)
    return pred.cpu(), dP.cpu()


@pytest.mark.parametrize("shape,regime", C.WARP_CASES)
def test_warp_f64(shape, regime):
    inp, ref = _warp_case(shape, regime)
    dup = torch.full((inp["B"], 1, inp["H"], inp["W"]), float("nan"), device=DEV)
    pred, dP = _warp_device(inp, ref["go"], dup, 0)
    keep = ~ref["mask"].unsqueeze(1)
    print(f"  lattice mask {float(ref['mask'].double().mean()):.4f}")
    _check([("pred", C.err_abs(pred, ref["pred"], keep.expand_as(pred)), "warp_pred"),
            ("ddisp_up / rms", C.err_rms(dup.cpu(), ref["ddisp_up"], keep), "warp_ddisp_up"),
            ("dP / max", C.err_max(dP, ref["dP"]), "warp_dP")])


def test_warp_two_frames_accumulate_f64():
    """two source frames into ONE ddisp_up: written by the first (accumulate 0), added to by the second (accumulate 1)"""
    (i0, r0), (i1, r1) = (_warp_case(*C.TWO_FRAME_CASE, f) for f in (0, 1))
    dup = torch.full((i0["B"], 1, i0["H"], i0["W"]), float("nan"), device=DEV)
    _, dP0 = _warp_device(i0, r0["go"], dup, 0)
    _, dP1 = _warp_device(i1, r1["go"], dup, 1)
    keep = ~(r0["mask"] | r1["mask"]).unsqueeze(1)
    _check([("ddisp_up(0 + 1) / rms", C.err_rms(dup.cpu(), r0["ddisp_up"] + r1["ddisp_up"], keep), "warp_ddisp_up"),
            ("dP frame 0 / max", C.err_max(dP0, r0["dP"]), "warp_dP"), ("dP frame 1 / max", C.err_max(dP1, r1["dP"]), "warp_dP")])


# ------------------------------------------------------------------------------------------- (c) SSIM + L1
@pytest.mark.parametrize("H,W", C.SSIM_SHAPES)
def test_ssim_l1_f64(H, W):
    x, y, idx, eq = C.ssim_inputs(H, W)
    B = x.shape[0]
    xr, lr, pre = C.ssim_reference(x, y)
    masked, exact0, eqin = C.ssim_masks(pre, eq)
    assert float(masked.double().mean()) <= C.MASK_CAP
    idm, runs = C.ssim_weights(idx, masked)
    xd, yd, idd = x.to(DEV), y.to(DEV), idm.to(DEV)
    out = ops_loss.ssim_l1(xd, yd)
    figs = [("fwd", C.err_abs(out.cpu().squeeze(1), lr.squeeze(1), ~masked), "ssim_fwd")]
    gout = torch.tensor([C.SSIM_GOUT], device=DEV)
    for cand, wgt, keep in runs:
        gr = C.ssim_grad(xr, lr, wgt)
        rms = float(gr.pow(2).mean().sqrt())
        dp = torch.full((B, 3, H, W), float("nan"), device=DEV)
        # a NULL min_index weighs every window (the candidate number is then not read)
        call("jp_ssim_l1_bwd", xd, yd, idd if cand is not None else None, cand if cand is not None else 2, gout, C.SSIM_GSCALE, dp,
             B, H, W)
        dp = dp.cpu()
        assert bool(torch.isfinite(dp).all())
        tag = f"cand {cand}" if cand is not None else "NULL index"
        figs.append((f"bwd {tag} / rms", C.err_rms(dp, gr, keep.unsqueeze(1).expand_as(gr)), "ssim_bwd"))
        figs.append((f"bwd {tag} pred==target / rms", float(dp[eqin.unsqueeze(1).expand_as(dp)].abs().max()) / rms, "ssim_bwd"))
    _check(figs)


# ------------------------------------------------------------------------------------------- (d) the composite
def test_min_reprojection_composite_f64():
    inp = C.composite_inputs(C.COMP_SEED)
    ref = C.composite_reference(inp)
    assert C.composite_conditions(ref) == []
    B, H, W, nS = C.COMP_B, C.COMP_H, C.COMP_W, len(C.COMP_SCALES)
    Kd, iKd, target = inp["K"].to(DEV), inp["invK"].to(DEV), inp["target"].to(DEV)
    colors = [c.to(DEV) for c in inp["colors"]]
    avs = [Var(a.to(DEV), True) for a in inp["aas"]]
    tvs = [Var(t.to(DEV), True) for t in inp["trs"]]
    dvs = [Var(d.to(DEV), True) for d in inp["disps"]]
    slots = [("min_reconstruct_loss", s) for s in range(nS)]
    lv = ops_loss.LossVec(slots, DEV)
    lv.grads.copy_(torch.tensor(C.COMP_GOUT))
    id_losses = [ops_loss.ssim_l1(c, target) for c in colors]
    tape = Tape()
    idxs = []
    with recording(tape):
        poses = [ops_loss.pose(a, t, Kd, inv) for a, t, inv in zip(avs, tvs, C.COMP_INVERT)]       # shared by all three scales
        for s in range(nS):
            _, idx = ops_loss.min_reprojection_loss(lv, slots[s], dvs[s], poses, colors, target, iKd, id_losses,
                                                    [n.to(DEV) for n in inp["noises"][s]], H, W, C.MIN_DEPTH, C.MAX_DEPTH, nS)
            idxs.append(idx)
    tape.backward()
    for s in range(nS):
        share = torch.bincount(ref["argmin"][s].flatten(), minlength=4).tolist()
        print(f"  scale {s}: candidate wins {share}, smallest margin {float(ref['margin'][s].min()):.2e}")
        assert torch.equal(idxs[s].cpu(), ref["argmin"][s]), f"argmin of scale {s}"
    figs = []
    for s in range(nS):
        figs.append((f"loss scale {s}", C.err_max(lv.vals[s:s + 1].cpu(), ref["loss"][s].view(1)), "comp_loss"))
        figs.append((f"ddisp scale {s} / max", C.err_max(dvs[s].g.cpu(), ref["ddisp"][s]), "comp_ddisp"))
    for j in range(2):
        figs.append((f"d_axisangle pose {j} / max", C.err_max(avs[j].g.cpu(), ref["daa"][j]), "comp_daa"))
        figs.append((f"d_translation pose {j} / max", C.err_max(tvs[j].g.cpu(), ref["dtr"][j]), "comp_dtr"))
    _check(figs)
