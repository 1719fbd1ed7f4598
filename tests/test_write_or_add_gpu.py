"""Write-or-add and NaN-poisoned buffers on every gradient path (collected after every other file of the suite).

Two contracts of the library that the per-kernel files never vary:

  * "write or add": every entry point with an `accumulate` / `acc*` flag (and every op that goes through `Var.add_grad`) must ADD to a
    gradient buffer that a second consumer already wrote and WRITE into a fresh one.  Each case runs forward + backward twice on the
    same inputs: pass 1 with the input gradients absent (acc = 0) and the parameter gradients pre-filled with a seeded random tensor R,
    pass 2 with every input gradient pre-filled with its own R and the parameter gradients with another R'.  R has the rms of the
    gradient it is added to (0.25 <= rms(R) / rms(grad) <= 4 is asserted), so a dropped or doubled add is an error of about 1 x the
    gradient -- thousands of times the bar.
  * independence from uninitialised memory: both passes run inside `poisoned()`, which fills every floating-point device tensor that
    `torch.empty` / `torch.empty_like` return with NaN (outputs, gradient buffers, split-K / pack / statistics scratch, the magnitude
    scratch): a tile tail left unwritten, pack padding that is read, scratch expected to be zero or a fold over more partials than were
    written all surface as NaN.  `torch.zeros` is untouched (the magnitude slots are zeroed by contract).

References: float64 conv / pad / interpolate autograd on the CPU (kink_act convention of tests/test_kernels_gpu.py) for every case of at
most 1e9 multiply-adds.  Above that pass 2 is compared with R + pass 1 on the device in float64 (and nothing may be NaN / Inf): all
bench shapes (their ATen comparison is in tests/test_bench_shapes_gpu.py), and also the larger CONV_CASES / fused-upsample
cases (theirs is in tests/test_kernels_gpu.py) -- of the table below conv (4, 129, 64, 96, 64, ...) at 1.8e9 and
conv (3, 160, 32, 64, 128, ...) at 1.1e9 multiply-adds, and the fused cases except the first and (2, 32, 64, 32, 128, 72).  Every
case prints the mode it used ("[mode] ...").  Bars: close() of tests/test_kernels_gpu.py with the sibling test's rtol for the
same quantity.  The kernel tags of pass 2 must equal those of pass 1 (same instantiation with and without accumulation).

Branch of jp_conv2d_dgrad[_src3] -> case of the sweep that is asserted (by profile tag, in both passes) to take it:

  DgradEpi (generic engine on the pack)        conv  (2, 64, 24, 40, 128, 1, 2, 0, 0, 0, False)             DgradBT<1>, DgradEpi
  DgradS2PointEpi (1x1 stride 2)               bench "downsample 64->128 1x1 stride 2 @256^2"
  DgradS2Epi (parity-class stride 2)           conv  (2, 64, 32, 48, 128, 3, 2, 1, 0, 0, False)
  class-uniform jp_igemm_p9s2d_kernel          bench "ResNet layer2.0 / layer3.0 / layer4.0 ... stride 2"
  jp_p9sm_launch, one slice (SmDgradEpi)       bench "pose encoder layer2 128->128 3x3 @24x80, N = 16"
  jp_p9sm_launch + slice_reduce (SmSliceEpi)   bench "pose encoder layer4 512->512 3x3 @6x20, N = 16"
  ... sm.splits > 1 with reflect               bench "layout encoder conv2 128->128 3x3 reflect @16^2", conv (3, 160, 32, 64, 128, ...)
  split-K scratch fold (DgradBT, WgradEpiWS)   conv  (2, 64, 24, 40, 128, 3, 2, 1, 0, 0, False), bench "CCT 128->256 3x3 @8x8"
  ... with reflect + border pass               conv  (2, 129, 10, 14, 96, 3, 1, 1, 1, 2, True)
  AtomicEpi behind the memset                  test_dgrad_without_split_scratch (split_ws = NULL through the C ABI; zero pad and reflect)
  short-row-tail launch, reflect, Cin = 129    conv  (4, 129, 64, 96, 64, 3, 1, 1, 1, 2, True): P9 on 128 rows + DgradBT<3, true>, DgradEpi
  short-row-tail launch, reflect, Cin = 513    extra (2, 513, 32, 96, 32, 3, 1, 1, 1, 2, True): P9 on 512 rows + DgradBT<3, true>, DgradEpi
  row-tile kernel (jp_igemm_r3_kernel)         fused (1, 64, 128, 128, 128, 136) (the _src3 variant); single-source entry point:
                                               test_row_tile_dgrad_single_source_in_child (JP_P9SM=0 in a child process -- no shape of the
                                               sweep reaches that branch at the default settings, the small-map kernel comes first)
  P9 patch kernel main pass + border pass      bench "merge 256->256 3x3 reflect @256^2 / @128^2"
  jp_c16_dgrad (no engine launch)              small-channel (2, 16, 16, 64, 128, 1, 0, False) and the other 16 -> 16 cases
  up-head kernel (no engine launch)            disparity head: all five cases
  border_pass through scratch                  every reflect case above (DgradBorderB<3>, WgradEpiWS)
  border_pass, read-modify-write epilogue      conv  (2, 32, 16, 24, 16, 3, 1, 1, 1, 0, True), test_dgrad_without_split_scratch[reflect]
  per-source dgrad (_src3)                     the three iconv bench shapes; fused (3, 128, 128, 64, 64, 160) (DgradUPB + DgradUPBorderB)

Pass 2 must launch exactly the kernels pass 1 launched (asserted for every case).
"""
import contextlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops, ops_loss, _lib                                   # noqa: E402
from jperceiver_amd._lib import call                                             # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                              # noqa: E402
from oracle import jp_oracle as J                                                # noqa: E402
from tests.test_kernels_gpu import (kink_act, CONV_CASES, FUSED_UPSAMPLE_CASES, DISPARITY_HEAD_CASES,       # noqa: E402
                                    SMALL_CHANNEL_CASES, BN_EPILOGUE_CASES, _geom, _masks)
from tests.test_bench_shapes_gpu import BENCH_CONV, ICONV_BENCH_CASES, kernel_tags, _expect     # noqa: E402

DEV = "cuda"
CPU_REF_MACS = 1e9          # no CPU reference above this many multiply-adds (the suite has no time to spare)
OBSERVED = {}               # family -> largest error / bar seen (printed per test: the measured basis for a later tightening)


# ------------------------------------------------------------------------------------------- helpers
@contextlib.contextmanager
def poisoned():
    """Every floating-point device tensor out of torch.empty / torch.empty_like is NaN for the duration (filled on the current
    stream).  ops.py / ops_loss.py allocate through these two only (ops._new, torch.empty_like, torch.empty); the per-stream magnitude
    scratch is cached, so the cache is dropped first and re-allocated inside."""
    orig_empty, orig_like = torch.empty, torch.empty_like

    def fill(t):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    def empty(*a, **k):
        return fill(orig_empty(*a, **k))

    def empty_like(*a, **k):
        return fill(orig_like(*a, **k))

    ops.amax_pool_reset()
    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = orig_empty, orig_like
        ops.amax_pool_reset()


def rand(*shape, seed, scale=1.0):
    """seeded normal tensor (a device generator: the bench-shape tensors would take seconds each on the host)"""
    g = torch.Generator(device=DEV).manual_seed(1000003 * seed + sum(shape))
    return torch.randn(*shape, generator=g, device=DEV) * scale


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def like_grad(ref, seed):
    """R: seeded, of the gradient's own rms"""
    return rand(*ref.shape, seed=seed, scale=max(rms(ref), 1e-30))


def check_ratio(R, grad, what):
    q = rms(R) / max(rms(grad), 1e-300)
    assert 0.25 <= q <= 4, f"{what}: rms(R) / rms(grad) = {q:.3g}: the test would be blind"


def check(got, ref, rtol, fam, msg, atol=1e-5, bar=None):
    """close() of tests/test_kernels_gpu.py (same bar: (atol + rtol) x max(1, max|ref|)), evaluated in float64 where the tensors live;
    `bar`: an absolute bar given by the caller instead."""
    assert bool(torch.isfinite(got).all()), f"{msg}: NaN / Inf in the result"
    ref = ref.to(got.device)
    err = float((got.double() - ref.double()).abs().max())
    scale = max(1.0, float(ref.abs().max()))
    if bar is None:
        bar = atol * scale + rtol * scale
    OBSERVED[fam] = max(OBSERVED.get(fam, 0.0), err / bar)
    print(f"[{fam}] {msg}: max abs err {err:.3e}, bar {bar:.3e} (err / bar {err / bar:.3f}; family max so far {OBSERVED[fam]:.3f})")
    assert err <= bar, f"{msg} max abs err {err:.3e} (scale {scale:.3e}, bar {bar:.3e})"


# ------------------------------------------------------------------------------------------- conv sweep
def _single(case, **kw):
    N, Cin, H, W, Cout, K, s, p, pm, act, bias = case
    return dict(srcs=[((N, Cin, H, W), 0)], Cout=Cout, K=K, s=s, p=p, pm=pm, act=act, bias=bias, wscale=(Cin * K * K) ** -0.5,
                rg=True, **kw)


def _fused(N, H, W, Cr, Cx, Cout, wscale=0.05, **kw):
    return dict(srcs=[((N, Cr, H, W), 0), ((N, Cx, H // 2, W // 2), 1), ((N, 1, H, W), 0)], Cout=Cout, K=3, s=1, p=1, pm=1, act=2,
                bias=True, wscale=wscale, rg=True, **kw)


def _no_engine(names, what):
    assert not names, f"{what}: expected the direct kernels (no implicit-GEMM launch), got {names}"


def _tags(want):
    return lambda names, what: _expect(names, want, what)


def _raw(want):
    """tags given as they are printed (no split-twin translation)"""
    def f(names, what):
        for w in want:
            assert any(w in n for n in names), f"{what}: expected a launch of {w!r}, the library launched {sorted(set(names))}"
    return f


def _all(*fs):
    def f(names, what):
        for g in fs:
            g(names, what)
    return f


# branch assertions on imported cases (see the table in the module docstring)
_P9_128 = "jp_igemm_p9_kernel<2, 2, false, true, DgradEpi, 9, 1>"
CONV_TAGS = {
    (2, 64, 24, 40, 128, 1, 2, 0, 0, 0, False): _raw(["DgradBT<1>, DgradEpi"]),
    (2, 64, 24, 40, 128, 3, 2, 1, 0, 0, False): _raw(["DgradBT<3>, WgradEpiWS"]),
    (2, 64, 32, 48, 128, 3, 2, 1, 0, 0, False): _raw(["DgradS2Epi"]),
    (2, 129, 10, 14, 96, 3, 1, 1, 1, 2, True): _raw(["DgradBT<3>, WgradEpiWS", "DgradBorderB<3>, WgradEpiWS"]),
    (4, 129, 64, 96, 64, 3, 1, 1, 1, 2, True): _all(_tags([_P9_128]), _raw(["DgradBT<3, true>, DgradEpi", "DgradBorderB<3>"])),
    (2, 32, 16, 24, 16, 3, 1, 1, 1, 0, True): _raw(["DgradBorderB<3>, DgradBorderEpi"]),
    (3, 160, 32, 64, 128, 3, 1, 1, 1, 2, True): _all(_tags(["SM<2, 2, false, true, SmSliceEpi, 9>"]), _raw(["DgradBorderB<3>"])),
}
FUSED_TAGS = {
    (1, 64, 128, 128, 128, 136): _raw(["jp_igemm_r3_kernel", "DgradBT<3, true>, DgradEpi", "DgradBorderB<3>"]),
    (3, 128, 128, 64, 64, 160): _raw(["DgradUPB, DgradEpi", "DgradUPBorderB", "DgradBorderB<3>"]),
}
# a case added because no imported one reaches the branch: the 513-channel bank's short row tail with reflect in the single-source
# entry point (P9 main pass on 512 rows, a 1-row launch of the generic engine, border pass)
EXTRA_CONV = [
    ((2, 513, 32, 96, 32, 3, 1, 1, 1, 2, True), _raw(["DgradEpi, 9, 1>", "DgradBT<3, true>, DgradEpi", "DgradBorderB<3>"])),
]

BENCH_EXTRA_TAGS = {        # branch evidence beyond what BENCH_CONV lists (epilogue names as printed)
    "downsample 64->128 1x1 stride 2 @256^2": _raw(["DgradS2PointEpi"]),
    "CCT 128->256 3x3 @8x8 (a quarter of a 4x32 tile: stays on the generic engine)": _raw(["WgradEpiWS"]),
}
# a key that no longer matches its table (a case edited, a label reworded) would drop the assertion silently
assert set(CONV_TAGS) <= set(CONV_CASES) and set(FUSED_TAGS) <= set(FUSED_UPSAMPLE_CASES)
assert set(BENCH_EXTRA_TAGS) <= {c[0] for c in BENCH_CONV}
ICONV_BWD = ["jp_igemm_p9_kernel<2, 2, false, true, DgradEpi, 9, 1>", "DgradBorderB<3>", "jp_wgrad_w9_kernel<2, 2, 1, true>", "WgradAP, WgradBP"]


def _build_sweep():
    sweep = []
    for c in CONV_CASES:
        sweep.append(("conv", str(c), _single(c, bwd_tags=CONV_TAGS.get(c))))
    for c, t in EXTRA_CONV:
        sweep.append(("conv", "extra " + str(c), _single(c, bwd_tags=t)))
    for c in FUSED_UPSAMPLE_CASES:
        sweep.append(("fused", str(c), _fused(*c, bwd_tags=FUSED_TAGS.get(c))))
    for c in DISPARITY_HEAD_CASES:
        N, C, h, w = c
        sweep.append(("disp_head", str(c), dict(srcs=[((N, C, h, w), 1)], Cout=1, K=3, s=1, p=1, pm=1, act=3, bias=True, wscale=0.1, rg=True,
                                                bwd_tags=_no_engine)))
    for c in SMALL_CHANNEL_CASES:
        N, Ci, Co, H, W, up, act, bias = c
        direct = _no_engine if (Ci == 16 and Co == 16) else None
        sweep.append(("small_ch", str(c), dict(srcs=[((N, Ci, H >> up, W >> up), up)], Cout=Co, K=3, s=1, p=1, pm=0, act=act, bias=bias,
                                               wscale=0.1, rg=True, fwd_tags=direct, bwd_tags=direct)))
    for label, c, kf, kd, kw in BENCH_CONV:
        bwd = _tags(kd + kw)
        if label in BENCH_EXTRA_TAGS:
            bwd = _all(bwd, BENCH_EXTRA_TAGS[label])
        sweep.append(("bench", label, dict(_single(c, fwd_tags=_tags(kf), bwd_tags=bwd), rg=c[1] > 6, device_only=True)))
    for c in ICONV_BENCH_CASES:
        N, H, W, Cr, Cx, Co = c
        bw = list(ICONV_BWD)
        if H >= 128:      # (at 64^2 the half-resolution dgrad of the upsampled segment takes the tap-major path instead)
            bw += ["jp_igemm_p9sd_kernel<DgradEpi>" if os.environ.get("JP_P9SD", "1") != "0" else "DgradUPB", "DgradUPBorderB"]
        sweep.append(("iconv_bench", str(c), _fused(*c, wscale=(9 * (Cr + Cx + 1)) ** -0.5, device_only=True,
                                                    fwd_tags=_tags(["jp_igemm_p9u_kernel<FwdEpi>"]), bwd_tags=_tags(bw))))
    return sweep


SWEEP = _build_sweep()

# rtol (forward, input gradients, weight / bias gradients): what the sibling test of the family uses for the same quantity
RTOL = {"conv": (1e-4, 1e-4, 2e-4), "fused": (1e-4, 2e-4, 2e-4), "disp_head": (1e-4, 2e-4, 2e-4), "small_ch": (1e-4, 2e-4, 2e-4),
        "bench": (2e-4, 2e-4, 2e-4), "iconv_bench": (2e-4, 2e-4, 2e-4)}


def _macs(d):
    N, _, h, w = d["srcs"][0][0]
    H, W = h << d["srcs"][0][1], w << d["srcs"][0][1]
    Cin = sum(s[0][1] for s in d["srcs"])
    OH, OW = (H + 2 * d["p"] - d["K"]) // d["s"] + 1, (W + 2 * d["p"] - d["K"]) // d["s"] + 1
    return float(N) * OH * OW * d["Cout"] * Cin * d["K"] ** 2


def _act_bwd(gy, y, act):
    if act == 1:
        return gy * (y > 0)
    if act == 2:
        return gy * torch.where(y > 0, 1.0, 0.01)
    if act == 3:
        return gy * y * (1 - y)
    return gy


def _reference(d, xs, w, b, y_dev, gy):
    L = [t.detach().double().cpu().requires_grad_(True) for t in xs]
    wr = w.detach().double().cpu().requires_grad_(True)
    br = b.detach().double().cpu().requires_grad_(True) if b is not None else None
    cat = torch.cat([F.interpolate(t, scale_factor=2, mode="nearest") if u else t for t, (_, u) in zip(L, d["srcs"])], 1)
    p = d["p"]
    xi = F.pad(cat, (p, p, p, p), mode="reflect") if d["pm"] == 1 else cat
    yr = kink_act(F.conv2d(xi, wr, br, d["s"], 0 if d["pm"] == 1 else p), y_dev, d["act"])
    yr.backward(gy.double().cpu())
    return yr.detach(), [t.grad for t in L], wr.grad, (br.grad if br is not None else None)


def _conv_pass(d, xs, w, b, gy_of, gx, pre_bwd):
    """forward + backward under poisoning; gy_of(y) -> the upstream gradient; gx: pre-filled input gradients (None: absent); pre_bwd(y) -> (R_w, R_b) placed in the
    parameter gradients between forward and backward."""
    with poisoned():
        vs = [Var(t, d["rg"], None if gx is None else gx[i].clone()) for i, t in enumerate(xs)]
        wv = Var(w, True, None)
        bv = Var(b, True, None) if b is not None else None
        tape = Tape()
        with recording(tape), kernel_tags() as kf:
            y = ops.conv2d(None, wv, bv, d["s"], d["p"], d["pm"], d["act"], srcs=[(v, u) for v, (_, u) in zip(vs, d["srcs"])])
        Rw, Rb = pre_bwd(y.t)
        wv.g = Rw.clone()
        if bv is not None:
            bv.g = Rb.clone()
        y.g = gy_of(y.t).clone()
        was = ops._WG_ON
        ops._WG_ON = False
        try:
            with kernel_tags() as kb:
                tape.backward()
        finally:
            ops._WG_ON = was
    torch.cuda.synchronize()
    return dict(y=y.t, dx=[v.g for v in vs], dw=wv.g, db=(bv.g if bv is not None else None), Rw=Rw, Rb=Rb, kf=kf.names, kb=kb.names)


@pytest.mark.parametrize("fam,label,d", SWEEP, ids=[f"{f}-{l}" for f, l, _ in SWEEP])
def test_conv_write_or_add_poisoned(fam, label, d):
    rt_f, rt_x, rt_w = RTOL[fam]
    xs = [rand(*shp, seed=11 + i) for i, (shp, _) in enumerate(d["srcs"])]
    Cin = sum(s[0][1] for s in d["srcs"])
    w = rand(d["Cout"], Cin, d["K"], d["K"], seed=21, scale=d["wscale"])
    b = rand(d["Cout"], seed=22) if d["bias"] else None
    use_ref = not d.get("device_only") and _macs(d) <= CPU_REF_MACS
    ref = {}
    gyh = {}

    def gy_of(y):
        if "gy" not in gyh:
            gyh["gy"] = rand(*y.shape, seed=23)
        return gyh["gy"]

    def pre1(y):
        gy = gy_of(y)
        if use_ref:
            ref["y"], ref["dx"], ref["dw"], ref["db"] = _reference(d, xs, w, b, y, gy)
            sw, sb = rms(ref["dw"]), (rms(ref["db"]) if b is not None else 0.0)
        else:
            # no reference: the sums behind dw / db have N * OH * OW independent terms x * dy' resp. dy' (dy' = dy through the activation)
            dyp = _act_bwd(gy, y, d["act"])
            n = y.shape[0] * y.shape[2] * y.shape[3]
            xr = (sum(float(t.double().pow(2).sum()) for t in xs) / sum(t.numel() for t in xs)) ** 0.5
            sb = n ** 0.5 * rms(dyp)
            sw = sb * xr
        return rand(*w.shape, seed=31, scale=sw), (rand(*b.shape, seed=32, scale=sb) if b is not None else None)

    def run(gx, pre):
        return _conv_pass(d, xs, w, b, gy_of, gx, pre)

    p1 = run(None, pre1)
    what = f"{fam} {label}"
    print(f"[mode] {what}: {'float64 CPU reference' if use_ref else 'device-side, pass 2 vs R + pass 1'} ({_macs(d):.2e} multiply-adds)")
    print(f"[tags] {what}: forward {sorted(set(p1['kf']))} backward {sorted(p1['kb'])}")
    for k, names in (("fwd_tags", p1["kf"]), ("bwd_tags", p1["kb"])):
        if d.get(k) is not None:
            d[k](names, what + " pass 1 " + k)
    dw1 = p1["dw"].double() - p1["Rw"].double()
    db1 = p1["db"].double() - p1["Rb"].double() if b is not None else None
    for nm, t in [("y", p1["y"]), ("dw - R", dw1), ("db - R", db1)] + [(f"dx{i}", g) for i, g in enumerate(p1["dx"])]:
        if t is not None:
            assert bool(torch.isfinite(t).all()), f"{what} pass 1: NaN / Inf in {nm}"
    check_ratio(p1["Rw"], ref["dw"] if use_ref else dw1, what + " R_w")
    if b is not None:
        check_ratio(p1["Rb"], ref["db"] if use_ref else db1, what + " R_b")
    if use_ref:
        check(p1["y"], ref["y"], rt_f, fam, what + " pass 1 fwd")
        for i, g in enumerate(p1["dx"]):
            check(g, ref["dx"][i], rt_x, fam, what + f" pass 1 dx{i}")
        check(p1["dw"], ref["dw"] + p1["Rw"].double().cpu(), rt_w, fam, what + " pass 1 R + dw")
        if b is not None:
            check(p1["db"], ref["db"] + p1["Rb"].double().cpu(), rt_w, fam, what + " pass 1 R + db")
    # ---- pass 2: every gradient buffer already holds something
    gx = None
    if d["rg"]:
        gx = [like_grad(ref["dx"][i] if use_ref else p1["dx"][i], 41 + i) for i in range(len(xs))]
        for i, r in enumerate(gx):
            check_ratio(r, ref["dx"][i] if use_ref else p1["dx"][i], what + f" R_x{i}")
    Rw2 = like_grad(ref["dw"] if use_ref else dw1, 51)
    Rb2 = like_grad(ref["db"] if use_ref else db1, 52) if b is not None else None
    p2 = run(gx, lambda y: (Rw2, Rb2))
    assert sorted(p2["kf"]) == sorted(p1["kf"]) and sorted(p2["kb"]) == sorted(p1["kb"]), \
        f"{what}: the accumulate pass took other kernels: {sorted(set(p2['kf'] + p2['kb']))} vs {sorted(set(p1['kf'] + p1['kb']))}"
    for k, names in (("fwd_tags", p2["kf"]), ("bwd_tags", p2["kb"])):
        if d.get(k) is not None:
            d[k](names, what + " pass 2 " + k)
    assert torch.equal(p2["y"], p1["y"]), f"{what}: the forward output differs between the two passes"
    if d["rg"]:
        for i, g in enumerate(p2["dx"]):
            base = ref["dx"][i].to(DEV) if use_ref else p1["dx"][i].double()
            check(g, gx[i].double() + base, rt_x, fam, what + f" pass 2 R + dx{i}")
    check(p2["dw"], Rw2.double() + (ref["dw"].to(DEV) if use_ref else dw1), rt_w, fam, what + " pass 2 R' + dw")
    if b is not None:
        check(p2["db"], Rb2.double() + (ref["db"].to(DEV) if use_ref else db1), rt_w, fam, what + " pass 2 R' + db")


ROW_TILE_CASE = (1, 64, 6, 256, 32, 3, 1, 1, 1, 2, True)      # W % 256 == 0, 64 rows, K small enough for one slice, H % 8 != 0 (no P9)


def test_row_tile_dgrad_single_source_in_child():
    """The row-tile branch of the single-source jp_conv2d_dgrad: at the default settings the small-map patch kernel (JP_P9SM, default 2)
    takes every shape that would reach it, so the sweep hits jp_igemm_r3_kernel through jp_conv2d_dgrad_src3 only.  The switch is read
    once per process: a child with JP_P9SM=0 runs the two-pass case and asserts the row-tile kernel + border pass by tag."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import tests.test_write_or_add_gpu as t\n"
            "d = t._single(t.ROW_TILE_CASE, bwd_tags=t._raw(['jp_igemm_r3_kernel', 'DgradEpi', 'DgradBorderB<3>']))\n"
            "t.test_conv_write_or_add_poisoned('conv', 'row tile ' + str(t.ROW_TILE_CASE), d)\n"
            "print('CHILD OK')\n") % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, JP_P9SM="0"), cwd=root)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------- direct C-ABI cases
def _f64_conv(x, w, b, s, p, pm, gy):
    xr, wr = x.detach().double().cpu().requires_grad_(True), w.detach().double().cpu().requires_grad_(True)
    xi = F.pad(xr, (p, p, p, p), mode="reflect") if pm == 1 else xr
    yr = F.conv2d(xi, wr, b.detach().double().cpu() if b is not None else None, s, 0 if pm == 1 else p)
    if gy is not None:
        yr.backward(gy.double().cpu())
    return yr.detach(), xr.grad, wr.grad


def _amax_ws():
    return torch.empty(int(_lib.lib().fn["jp_conv2d_amax_ws_floats"]()), device=DEV)


def _fn(name, *a):
    return int(_lib.lib().fn[name](*a))


@pytest.mark.parametrize("case", [(4, 512, 6, 20, 512, 3, 1, 1, 0),         # pose encoder layer4 @6x20 (4 images: 1.1e9 multiply-adds on the CPU)
                                  (8, 128, 16, 16, 128, 3, 1, 1, 1)],       # layout encoder conv2, reflect (W < 32)
                         ids=["pose-512-6x20", "reflect-128-16x16"])
def test_dgrad_without_split_scratch(case):
    """jp_conv2d_dgrad with split_ws = NULL on shapes whose jp_conv2d_dgrad_split_floats() > 0: what an external caller of the drop-in
    boundary gets (the K slices meet in atomics behind `if (!accumulate) memset`), accumulate 0 and 1, against float64."""
    N, Cin, H, W, Cout, K, s, p, pm = case
    assert _fn("jp_conv2d_dgrad_split_floats", N, Cin, H, W, Cout, K, s, p) > 0
    OH, OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    w = rand(Cout, Cin, K, K, seed=2, scale=(Cin * K * K) ** -0.5)
    dy = rand(N, Cout, OH, OW, seed=3)
    _, dxr, _ = _f64_conv(rand(N, Cin, H, W, seed=1), w, None, s, p, pm, dy)
    R = like_grad(dxr, 4)
    check_ratio(R, dxr, "R")
    nwd = _fn("jp_conv2d_ws_floats", Cin, Cout, K, 1)
    tags = []
    for acc in (0, 1):
        with poisoned(), kernel_tags() as kt:
            dx = R.clone() if acc else torch.empty(N, Cin, H, W, device=DEV)
            call("jp_conv2d_dgrad", dy, w, dx, N, Cin, H, W, Cout, K, s, p, pm, acc, torch.empty(nwd, device=DEV), 0, None, None, None,
                 None, _amax_ws())
        print("split_ws = NULL tags:", kt.names)
        assert not any("SliceEpi" in n or "WgradEpiWS" in n for n in kt.names), kt.names      # nothing may go through the absent scratch
        check(dx, dxr + (R.double().cpu() if acc else 0), 1e-4, "abi", f"dgrad split_ws=NULL accumulate={acc}")
        tags.append(sorted(kt.names))
    assert tags[0] == tags[1]
    assert any("AtomicEpi" in n for n in tags[0]), tags[0]


@pytest.mark.parametrize("case", [(2, 96, 20, 28, 160, 3, 1, 1, 1), (2, 64, 24, 40, 128, 3, 2, 1, 0), (1, 128, 16, 16, 256, 1, 1, 0, 0)],
                         ids=["reflect", "stride2", "1x1"])
def test_conv_without_pack_scratch(case):
    """jp_conv2d_fwd / jp_conv2d_dgrad with ws = NULL, ws_state = 0 on Cout >= 16 layers: the generic unpacked engine."""
    N, Cin, H, W, Cout, K, s, p, pm = case
    x, w, b = rand(N, Cin, H, W, seed=1), rand(Cout, Cin, K, K, seed=2, scale=(Cin * K * K) ** -0.5), rand(Cout, seed=3)
    OH, OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    dy = rand(N, Cout, OH, OW, seed=4)
    yr, dxr, _ = _f64_conv(x, w, b, s, p, pm, dy)
    with poisoned():
        y = torch.empty(N, Cout, OH, OW, device=DEV)
        call("jp_conv2d_fwd", x, w, b, y, N, Cin, H, W, Cout, K, s, p, pm, 0, None, 0, None, None, None, None, _amax_ws(), None, None)
    check(y, yr, 1e-4, "abi", "fwd ws=NULL")
    R = like_grad(dxr, 5)
    check_ratio(R, dxr, "R")
    for acc in (0, 1):
        with poisoned(), kernel_tags() as kt:
            dx = R.clone() if acc else torch.empty(N, Cin, H, W, device=DEV)
            call("jp_conv2d_dgrad", dy, w, dx, N, Cin, H, W, Cout, K, s, p, pm, acc, None, 0, None, None, None, None, _amax_ws())
        assert any("DgradA<" in n for n in kt.names), kt.names
        check(dx, dxr + (R.double().cpu() if acc else 0), 1e-4, "abi", f"dgrad ws=NULL accumulate={acc}")


# (N, Cin, H, W, Cout, K, stride, pad, pad_mode), tag of the family as printed (either arithmetic twin)
WGRAD_FAMILIES = [
    ("W9S wide", (2, 128, 32, 64, 128, 3, 1, 1, 1), ["jp_wgrad_w9_kernel<2, 2, 1, true>"]),
    ("W9S narrow", (4, 128, 32, 64, 64, 3, 1, 1, 0), ["jp_wgrad_w9_kernel<1, 2, 2, false>"]),
    ("W1S", (2, 128, 32, 64, 256, 1, 1, 0, 0), ["jp_wgrad_w1_kernel"]),
    ("W9S2", (2, 128, 32, 64, 256, 3, 2, 1, 0), None),
    ("W7", (2, 6, 64, 128, 64, 7, 2, 3, 0), ["jp_wgrad_w7_kernel<6>"]),
    ("table + tail", (2, 193, 16, 32, 128, 3, 1, 1, 1), ["jp_wgrad_w9_kernel<2, 2, 1, true>"]),
    ("table only", (1, 150, 9, 11, 80, 3, 1, 1, 0), None),
    ("c16", (2, 16, 64, 128, 16, 3, 1, 1, 0), None),
]


@pytest.mark.parametrize("label,case,tags", WGRAD_FAMILIES, ids=[c[0] for c in WGRAD_FAMILIES])
@pytest.mark.parametrize("with_ws", [True, False], ids=["ws", "no-ws"])
def test_wgrad_overwrites_poisoned_dw(label, case, tags, with_ws):
    """jp_conv2d_wgrad with accumulate = 0 into a NaN-filled dw (the `if (!accumulate) memset` and whatever each path does after it),
    with the queried scratch and with ws = NULL, ws_floats = 0 (optional by the header); accumulate = 1 on top of R as well."""
    N, Cin, H, W, Cout, K, s, p, pm = case
    x = rand(N, Cin, H, W, seed=1)
    OH, OW = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    dy = rand(N, Cout, OH, OW, seed=2)
    _, _, dwr = _f64_conv(x, rand(Cout, Cin, K, K, seed=3), None, s, p, pm, dy)
    nws = _fn("jp_conv2d_wgrad_ws_floats", N, Cin, H, W, Cout, K, s, p) if with_ws else 0
    R = like_grad(dwr, 4)
    check_ratio(R, dwr, "R")
    for acc in (0, 1):
        with poisoned(), kernel_tags() as kt:
            dw = R.clone() if acc else torch.empty(Cout, Cin, K, K, device=DEV)
            call("jp_conv2d_wgrad", x, dy, dw, N, Cin, H, W, Cout, K, s, p, pm, acc, torch.empty(nws, device=DEV) if nws else None, nws,
                 None, None, _amax_ws())
        print(f"wgrad {label} ws={nws} tags:", kt.names)
        if tags is not None and with_ws:
            _expect(kt.names, tags, f"wgrad {label}")
        if label == "W9S2" and with_ws:
            assert any("jp_wgrad_w9s2_kernel" in n for n in kt.names) or os.environ.get("JP_W9S2", "1") == "0", kt.names
        if label == "c16":
            _no_engine(kt.names, "c16 wgrad")
        check(dw, dwr + (R.double().cpu() if acc else 0), 2e-4, "abi", f"wgrad {label} ws={'yes' if nws else 'NULL'} accumulate={acc}")


@pytest.mark.parametrize("with_ws", [True, False], ids=["ws", "no-ws"])
def test_wgrad_src3_parity_class_overwrites_poisoned_dw(with_ws):
    """jp_conv2d_wgrad_src3 on cat(r, up(x), d) with accumulate = 0 into NaN: W4S parity-class kernels on the upsampled segment, the
    single-source paths on the others, the table pass for the disparity channel; with ws = NULL, ws_floats = 0 (the header does not
    require scratch) the generic engine on the virtual concat."""
    N, H, W, Cr, Cx, Cout = 2, 32, 64, 32, 128, 72
    r, xh, dd = rand(N, Cr, H, W, seed=1), rand(N, Cx, H // 2, W // 2, seed=2), rand(N, 1, H, W, seed=3)
    dy = rand(N, Cout, H, W, seed=4)
    cat = torch.cat((r, F.interpolate(xh, scale_factor=2, mode="nearest"), dd), 1)
    _, _, dwr = _f64_conv(cat, rand(Cout, Cr + Cx + 1, 3, 3, seed=5), None, 1, 1, 1, dy)
    nws = _fn("jp_conv2d_wgrad_src3_ws_floats", Cr, 0, Cx, 1, 1, 0, N, H, W, Cout, 3, 1, 1, 1)
    assert nws > 0
    if not with_ws:
        nws = 0
    R = like_grad(dwr, 6)
    check_ratio(R, dwr, "R")
    for acc in (0, 1):
        with poisoned(), kernel_tags() as kt:
            dw = R.clone() if acc else torch.empty(Cout, Cr + Cx + 1, 3, 3, device=DEV)
            call("jp_conv2d_wgrad_src3", r, Cr, 0, xh, Cx, 1, dd, 1, 0, dy, dw, N, H, W, Cout, 3, 1, 1, 1, acc,
                 torch.empty(nws, device=DEV) if nws else None, nws, None, None, None, None, _amax_ws())
        print(f"wgrad_src3 ws={nws} tags:", kt.names)
        if with_ws:
            _expect(kt.names, ["WgradAP, WgradBP"], "src3 wgrad, upsampled segment")
        else:
            assert kt.names and not any("WgradEpiWS" in n or "w4s" in n for n in kt.names), kt.names     # nothing through the absent scratch
        check(dw, dwr + (R.double().cpu() if acc else 0), 2e-4, "abi", f"wgrad_src3 ws={'yes' if nws else 'NULL'} accumulate={acc}")


@pytest.mark.parametrize("accs,null", [((1, 0, 0), None), ((0, 1, 0), None), ((0, 0, 1), None), ((1, 1, 1), 0), ((0, 1, 0), 2)],
                         ids=["acc100", "acc010", "acc001", "dx0-null", "dx2-null"])
def test_dgrad_src3_mixed_flags(accs, null):
    """jp_conv2d_dgrad_src3: one flag per source -- mixed patterns, and one dx* = NULL (that source needs no gradient)."""
    N, H, W, Cr, Cx, Cout = 3, 128, 128, 32, 32, 32        # (the smallest map the per-source path takes)
    cs, us = (Cr, Cx, 1), (0, 1, 0)
    assert _fn("jp_conv2d_dgrad_src3_ok", Cr, 0, Cx, 1, 1, 0, N, H, W, Cout, 3, 1, 1, 1)
    w = rand(Cout, Cr + Cx + 1, 3, 3, seed=2, scale=0.05)
    dy = rand(N, Cout, H, W, seed=3)
    # float64 reference of the gradient w.r.t. the virtual concat, routed to the sources (the upsampled one sums its 2x2 blocks)
    cat = torch.zeros(N, Cr + Cx + 1, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.pad(cat, (1, 1, 1, 1), mode="reflect"), w.double().cpu()).backward(dy.double().cpu())
    g = cat.grad
    refs = [g[:, :Cr], F.avg_pool2d(g[:, Cr:Cr + Cx], 2) * 4, g[:, Cr + Cx:]]
    Rs = [like_grad(refs[i], 10 + i) for i in range(3)]
    nwd = _fn("jp_conv2d_ws_floats", Cr + Cx + 1, Cout, 3, 1)
    nsd = _fn("jp_conv2d_dgrad_src3_split_floats", Cr, 0, Cx, 1, 1, 0, N, H, W)
    with poisoned():
        dx = [None if i == null else (Rs[i].clone() if accs[i] else torch.empty_like(Rs[i])) for i in range(3)]
        args = []
        for i in range(3):
            args += [dx[i], cs[i], us[i], accs[i]]
        call("jp_conv2d_dgrad_src3", dy, w, *args, N, H, W, Cout, 3, 1, 1, 1, torch.empty(nwd, device=DEV), 0,
             torch.empty(nsd, device=DEV) if nsd else None, None, None, None, _amax_ws())
    for i in range(3):
        if i != null:
            check_ratio(Rs[i], refs[i], f"R{i}")
            check(dx[i], refs[i] + (Rs[i].double().cpu() if accs[i] else 0), 2e-4, "abi", f"dgrad_src3 acc={accs} null={null} dx{i}")


# ------------------------------------------------------------------------------------------- the rest of the accumulate family
# Each entry: f(pre) -> {name: (got, float64 reference WITHOUT the pre-filled part, rtol, atol)}.  pre = None: input gradients absent
# (parameter-like buffers, which the library always adds to, start at zero); pre = {name: R}: every buffer starts at its R.
def _g(pre, k, like=None):
    if pre is None:
        return None if like is None else torch.zeros_like(like)
    return pre[k].clone()


def _o_upsample(pre):
    x, gy = rand(2, 6, 5, 7, seed=1), rand(2, 6, 10, 14, seed=2)
    xv = Var(x, True, _g(pre, "dx"))
    tape = Tape()
    with recording(tape):
        y = ops.upsample2x(xv)
    y.g = gy.clone()
    tape.backward()
    return {"dx": (xv.g, F.avg_pool2d(gy.double(), 2) * 4, 1e-4, 1e-5)}


def _o_copy_channels(pre):
    ts = [rand(2, c, 6, 8, seed=i) for i, c in enumerate((3, 6, 4))]
    gy = rand(2, 13, 6, 8, seed=9)
    vs = [Var(t, True, _g(pre, f"d{i}")) for i, t in enumerate(ts)]
    tape = Tape()
    with recording(tape):
        y = ops.cat_channels(vs)
    y.g = gy.clone()
    tape.backward()
    offs = (0, 3, 9, 13)
    return {f"d{i}": (vs[i].g, gy[:, offs[i]:offs[i + 1]].double(), 1e-4, 1e-5) for i in range(3)}


def _o_bilinear(pre):
    x, gy = rand(2, 3, 8, 12, seed=1), rand(2, 3, 37, 50, seed=2)
    xv = Var(x, True, _g(pre, "dx"))
    tape = Tape()
    with recording(tape):
        y = ops.bilinear_resize(xv, 37, 50)
    y.g = gy.clone()
    tape.backward()
    xr = x.double().cpu().requires_grad_(True)
    F.interpolate(xr, [37, 50], mode="bilinear", align_corners=False).backward(gy.double().cpu())
    return {"dx": (xv.g, xr.grad, 1e-4, 1e-5)}


def _o_channel_sum(pre):
    N, C, HW = 3, 5, 37 * 13
    x = rand(N, C, HW, seed=1)
    out = {}
    for ws in (True, False):
        o = _g(pre, "out") if pre is not None else torch.empty(C, device=DEV)
        n = _fn("jp_channel_sum_ws_floats", N, C, HW)
        call("jp_channel_sum", x, o, N, C, HW, 0 if pre is None else 1, torch.empty(n, device=DEV) if (ws and n) else None)
        out["out" if ws else "out_nows"] = (o, x.double().sum(dim=(0, 2)), 1e-5, 1e-5)
    if pre is not None:
        out["out_nows"] = (out["out_nows"][0] - pre["out"] + pre["out_nows"], *out["out_nows"][1:])
    return out


def _o_colsum(pre):
    M, N = 10, 36
    x = rand(M, N, seed=1)
    o = _g(pre, "out") if pre is not None else torch.empty(N, device=DEV)
    call("jp_colsum", x, o, M, N, 0 if pre is None else 1)
    return {"out": (o, x.double().sum(0), 1e-5, 1e-5)}


def _o_act_bwd_bias(pre):
    N, C, H, W = 3, 5, 37, 13
    dy, y = rand(N, C, H, W, seed=3), rand(N, C, H, W, seed=4)
    db = _g(pre, "db", torch.empty(C, device=DEV))
    dx = torch.empty_like(dy)
    n = _fn("jp_act_bwd_bias_ws_floats", N, C, H * W)
    call("jp_act_bwd_bias", dy, y, dx, db, N, C, H * W, 2, None, torch.empty(n, device=DEV))
    ref = dy.double() * torch.where(y > 0, 1.0, 0.01).double()
    assert bool(torch.isfinite(dx).all())
    return {"db": (db, ref.sum(dim=(0, 2, 3)), 1e-5, 1e-5)}


def _o_smooth(pre):
    B, h, w, f = 2, 16, 24, 2
    g = torch.Generator().manual_seed(2)
    disp = torch.rand(B, 1, h, w, generator=g) * 0.6 + 0.1
    img = torch.rand(B, 3, h * f, w * f, generator=g)
    img_ds = ops.area_downsample(img.to(DEV), f)
    dr = disp.double().requires_grad_(True)
    dn = dr / (dr.mean(2, True).mean(3, True) + 1e-7)
    (J.smooth_loss(dn, img_ds.double().cpu()) * 0.25).backward()
    lv = ops_loss.LossVec(["s"], DEV)
    dv = Var(disp.to(DEV), True, _g(pre, "ddisp"))
    tape = Tape()
    with recording(tape):
        ops_loss.smooth_loss(lv, "s", dv, img_ds, 0.25)
    call("jp_fill", lv.grads, 1, 1.0)
    tape.backward()
    return {"ddisp": (dv.g, dr.grad, 5e-4, 1e-6)}


def _o_scale_loss(pre):
    B, hs, ws, FH, FW = 2, 16, 16, 37, 124
    g = torch.Generator().manual_seed(4)
    disp = torch.rand(B, 1, hs, ws, generator=g) * 0.3 + 0.01
    label = torch.rand(B, 1, FH, FW, generator=g) * 30
    label[label < 12] = 0
    dr = disp.double().requires_grad_(True)
    _, depth = J.disp_to_depth(dr, 0.1, 100.0)
    (J.scale_loss(J.default_opt(type="static"), depth, label.double()) * 0.05).backward()
    lv = ops_loss.LossVec(["s"], DEV)
    dv = Var(disp.to(DEV), True, _g(pre, "ddisp"))
    tape = Tape()
    with recording(tape):
        ops_loss.scale_loss(lv, "s", dv, label.to(DEV), 0.05, 0.1, 100.0, None)
    call("jp_fill", lv.grads, 1, 1.0)
    tape.backward()
    return {"ddisp": (dv.g, dr.grad, 1e-3, 1e-6)}


def _o_layout_loss(pre):
    from jperceiver_amd import synthetic as syn
    n = 48
    lab = torch.from_numpy(_masks(n))
    logits = torch.from_numpy((syn.hash_uniform(7, "logits", (5, 2, n, n)) - 0.5) * 4)
    lw, cew, l2w = 20.0, 1.0, 20.0
    lr = logits.double().requires_grad_(True)
    gt = lab.long().squeeze(1)
    (lw * J.iou_loss(lr, gt) + cew * F.cross_entropy(lr, gt, weight=torch.tensor([1.0, 5.0], dtype=torch.float64))
     + l2w * J.bd_loss(lr, gt)).backward()
    lv = ops_loss.LossVec(["t"], DEV)
    zv = Var(logits.to(DEV), True, _g(pre, "dlogits"))
    labd = lab.to(DEV)
    tape = Tape()
    with recording(tape):
        ops_loss.layout_loss(lv, "t", zv, labd, ops_loss.signed_distance(labd), 1.0, 5.0, lw, cew, l2w)
    call("jp_fill", lv.grads, 1, 1.0)
    tape.backward()
    return {"dlogits": (zv.g, lr.grad, 5e-4, 1e-7)}


def _o_linear_act(pre):
    x, w, b = rand(2, 5, 36, seed=1), rand(36, 36, seed=2, scale=0.2), rand(36, seed=3)
    gy = rand(2, 5, 36, seed=4)
    xv, wv, bv = Var(x, True, _g(pre, "dx")), Var(w, True, _g(pre, "dw", w)), Var(b, True, _g(pre, "db", b))
    tape = Tape()
    with recording(tape):
        y = ops.linear_act(xv, wv, bv, ops.ACT_RELU)
    y.g = gy.clone()
    tape.backward()
    L = [t.double().cpu().requires_grad_(True) for t in (x, w, b)]
    kink_act(F.linear(*L), y.t, 1).backward(gy.double().cpu())
    return {k: (v.g, t.grad, 2e-4, 1e-5) for k, v, t in zip(("dx", "dw", "db"), (xv, wv, bv), L)}


def _o_split_rows(pre):
    x = rand(6, 4, 5, seed=1)
    gs = [rand(2, 4, 5, seed=2), None, rand(2, 4, 5, seed=3)]
    xv = Var(x, True, _g(pre, "dx"))
    tape = Tape()
    with recording(tape):
        parts = ops.split_rows(xv, 2)
    for p_, g_ in zip(parts, gs):
        p_.g = None if g_ is None else g_.clone()
    tape.backward()
    return {"dx": (xv.g, torch.cat([gs[0], torch.zeros_like(gs[0]), gs[2]]).double(), 1e-6, 1e-6)}


def _o_batchnorm(pre):
    N, C, H, W = 3, 48, 14, 18
    x, r = rand(N, C, H, W, seed=1) * 2 + 0.5, rand(N, C, H, W, seed=4)
    g, b = rand(C, seed=2) * 0.2 + 1, rand(C, seed=3) * 0.1
    gy = rand(N, C, H, W, seed=5)
    xv, rv = Var(x, True, _g(pre, "dx")), Var(r, True, _g(pre, "dres"))
    gv, bv = Var(g, True, _g(pre, "dgamma", g)), Var(b, True, _g(pre, "dbeta", b))
    tape = Tape()
    with recording(tape):
        y = ops.batchnorm_train(xv, gv, bv, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), rv, True, 0.1, 1e-5, 1)
    y.g = gy.clone()
    tape.backward()
    if pre is not None:
        assert xv.gamax is None and rv.gamax is None
    L = [t.double().cpu().requires_grad_(True) for t in (x, r, g, b)]
    pre_act = F.batch_norm(L[0], None, None, L[2], L[3], True, 0.1, 1e-5) + L[1]
    kink_act(pre_act, y.t, 1).backward(gy.double().cpu())
    return {k: (v.g, t.grad, 3e-4 if k != "dres" else 1e-4, 1e-5) for k, v, t in zip(("dx", "dres", "dgamma", "dbeta"), (xv, rv, gv, bv), L)}


def _o_maxpool_addend(pre):
    x = torch.round(rand(2, 32, 20, 28, seed=1) * 4) / 4
    gy, add = rand(2, 32, 20, 28, seed=2), rand(2, 32, 20, 28, seed=3)
    xv = Var(x, True, _g(pre, "dx"))
    tape = Tape()
    with recording(tape):
        y = ops.maxpool(xv, 5, 1, 2, bwd_addend=lambda: add)
    y.g = gy.clone()
    tape.backward()
    if pre is not None:
        assert xv.gamax is None
    xr = x.double().cpu().requires_grad_(True)
    F.max_pool2d(xr, 5, 1, 2).backward(gy.double().cpu())
    return {"dx": (xv.g, xr.grad + add.double().cpu(), 1e-6, 1e-5)}


def _o_add(pre):
    a, b = rand(2, 3, 5, 7, seed=1), rand(2, 3, 5, 7, seed=2)
    gy = rand(2, 3, 5, 7, seed=3)
    av, bv = Var(a, True, _g(pre, "da")), Var(b, True, _g(pre, "db"))
    tape = Tape()
    with recording(tape):
        y = ops.add(av, bv)
    y.g, y.gamax = gy.clone(), torch.zeros(1, device=DEV)
    tape.backward()
    if pre is not None:
        assert av.gamax is None and bv.gamax is None
    return {"da": (av.g, gy.double(), 1e-6, 1e-6), "db": (bv.g, gy.double(), 1e-6, 1e-6)}


def _o_mul_mask(pre):
    x, gy = rand(2, 6, 5, 7, seed=1), rand(2, 6, 5, 7, seed=2)
    m = (rand(2, 6, 5, 7, seed=4) > 0).float()
    xv = Var(x, True, _g(pre, "dx"))
    xv.gamax = torch.zeros(1, device=DEV) if pre is not None else None
    tape = Tape()
    with recording(tape):
        y = ops.mul_mask(xv, m, 2.0)
    y.g = gy.clone()
    tape.backward()
    if pre is not None:
        assert xv.gamax is None
    return {"dx": (xv.g, gy.double() * m.double() * 2.0, 1e-6, 1e-6)}


def _o_act(pre):
    x, gy = rand(2, 6, 5, 7, seed=1), rand(2, 6, 5, 7, seed=2)
    xv = Var(x, True, _g(pre, "dx"))
    xv.gamax = torch.zeros(1, device=DEV) if pre is not None else None
    tape = Tape()
    with recording(tape):
        y = ops.act(xv, ops.ACT_LEAKY)
    y.g = gy.clone()
    tape.backward()
    if pre is not None:
        assert xv.gamax is None
    return {"dx": (xv.g, gy.double() * torch.where(x > 0, 1.0, 0.01).double(), 1e-6, 1e-6)}


def _o_cgt_warp_pose(pre):
    """jp_cgt_warp_bwd (ddisp_up written or added), jp_bilinear_bwd, jp_pose_bwd (axis-angle / translation gradients written or added).
    The oracle's gradients are piecewise (border clipping, floor): 2e-2 of the gradient's maximum as in test_cgt_warp_and_pose -- a
    dropped add (about 1 x rms) is only some ten bars away from that, so the sharp check for these outputs is the device-side one in
    test_other_write_or_add (pass 2 vs R + pass 1 at 16 ulp)."""
    B, H, W, hs, ws = 2, 32, 48, 16, 24
    K, invK, aa, tr = _geom(B, H, W)
    g = torch.Generator().manual_seed(3)
    disp = torch.rand(B, 1, hs, ws, generator=g) * 0.5 + 0.2
    col = torch.rand(B, 3, H, W, generator=g)
    go = torch.randn(B, 3, H, W, generator=g)
    L = [t.clone().requires_grad_(True) for t in (disp, aa, tr)]
    T = J.transformation_from_parameters(L[1].view(B, 1, 3), L[2].view(B, 1, 3), False)
    d_up = F.interpolate(L[0], [H, W], mode="bilinear", align_corners=False)
    d_up.retain_grad()
    _, depth = J.disp_to_depth(d_up, 0.1, 100.0)
    pr = F.grid_sample(col, J.project(J.backproject(depth, invK), K, T, H, W), mode="bilinear", padding_mode="border", align_corners=False)
    (pr * go).sum().backward()
    av, tv = Var(aa.to(DEV), True, _g(pre, "daa")), Var(tr.to(DEV), True, _g(pre, "dtr"))
    Kd, iKd, cd, dd = K.to(DEV), invK.to(DEV), col.to(DEV), disp.to(DEV)
    tape = Tape()
    with recording(tape):
        pp = ops_loss.pose(av, tv, Kd, False)
    dup = _g(pre, "dup") if pre is not None else torch.empty(B, 1, H, W, device=DEV)
    call("jp_cgt_warp_bwd", go.to(DEV), dd, hs, ws, iKd, pp.P, cd, dup, pp.dP, B, H, W, 0.1, 100.0, 0 if pre is None else 1)
    tape.backward()
    # absolute bars (5th entry): err <= 2e-2 x max |gradient-only reference|, what test_cgt_warp_and_pose asserts
    big = lambda t: 2e-2 * float(t.abs().max())                                        # noqa: E731
    return {"dup": (dup, d_up.grad, None, None, big(d_up.grad)), "daa": (av.g, L[1].grad, None, None, big(L[1].grad)),
            "dtr": (tv.g, L[2].grad, None, None, big(L[2].grad))}


OTHER = {"jp_upsample2x_bwd": _o_upsample, "jp_copy_channels": _o_copy_channels, "jp_bilinear_bwd": _o_bilinear,
         "jp_channel_sum": _o_channel_sum, "jp_colsum": _o_colsum, "jp_act_bwd_bias": _o_act_bwd_bias, "jp_smooth_bwd": _o_smooth,
         "jp_scale_loss_bwd": _o_scale_loss, "jp_layout_loss_bwd": _o_layout_loss, "jp_cgt_warp_bwd+jp_pose_bwd": _o_cgt_warp_pose,
         "linear_act": _o_linear_act, "split_rows": _o_split_rows, "batchnorm_bwd": _o_batchnorm, "maxpool_bwd_addend": _o_maxpool_addend,
         "add": _o_add, "mul_mask": _o_mul_mask, "act": _o_act}


ULP = 2.0 ** -23


@pytest.mark.parametrize("name", list(OTHER))
def test_other_write_or_add(name):
    """Entries (got, reference, rtol, atol[, absolute bar]).  Pass 2 is compared twice: with R + the float64 reference at the sibling
    test's bar, and with R + pass 1 on the device.  The latter differs from correct code by the fp32 rounding of where R enters the
    sum only: for entries with a close() bar that bar is the ceiling; for entries whose reference bar is the loose absolute one
    (piecewise oracle gradients) it is 16 ulp of max |R + pass 1| -- the kernels add R to the finished fp32 value (one rounding, <= 1
    ulp of the result), the double-precision pose accumulator is summed in another order run to run (<= 1 ulp after the conversion)."""
    f = OTHER[name]
    with poisoned():
        r1 = f(None)
    torch.cuda.synchronize()
    pre = {}
    for i, (k, (got, ref, rtol, atol, *bar)) in enumerate(r1.items()):
        check(got, ref, rtol, "other", f"{name} fresh {k}", atol=atol, bar=bar[0] if bar else None)
        pre[k] = like_grad(ref, 70 + i)
        check_ratio(pre[k], ref, f"{name} R[{k}]")
    with poisoned():
        r2 = f(pre)
    torch.cuda.synchronize()
    for k, (got, ref, rtol, atol, *bar) in r2.items():
        check(got, ref.to(DEV).double() + pre[k].double(), rtol, "other", f"{name} accumulate {k}", atol=atol, bar=bar[0] if bar else None)
        want = r1[k][0].double() + pre[k].double()
        if bar:
            check(got, want, None, "other_device", f"{name} accumulate vs R + fresh {k}", bar=16 * ULP * float(want.abs().max()))
        else:
            check(got, want, rtol, "other_device", f"{name} accumulate vs R + fresh {k}", atol=atol)


# ------------------------------------------------------------------------------------------- BatchNorm statistics from the conv epilogue
# both sides of every condition launch_p9s evaluates when it sizes the partials (JP_P9_TILE at its default): 64-row banks take 16-row
# tiles when H % 16 == 0 and that leaves >= 256 workgroups, 8-row tiles otherwise; 128-row banks 8-row tiles when H % 8 == 0 and
# >= 256 workgroups, 4-row tiles otherwise
BN_EXTRA = [(8, 64, 72, 128, True),       # 64 rows, H % 16 != 0 (H % 8 == 0): 8-row tiles
            (7, 64, 128, 128, True),      # 64 rows, H % 16 == 0 but 7 * 8 * 4 = 224 < 256 workgroups: 8-row tiles
            (8, 128, 128, 64, True),      # 128 rows, H % 8 == 0 and 8 * 16 * 2 = 256 workgroups: 8-row tiles
            (8, 128, 132, 64, True)]      # 128 rows, H % 8 != 0 (H % 4 == 0): 4-row tiles


@pytest.mark.parametrize("N,C,H,W,expect", BN_EPILOGUE_CASES + BN_EXTRA)
def test_batchnorm_statistics_from_the_conv_epilogue_poisoned(N, C, H, W, expect):
    """test_batchnorm_statistics_from_the_conv_epilogue with every scratch (the statistics partials included) NaN before the call: a
    fold over more partials than the epilogue wrote, or a partial left unwritten, is a NaN in the normalised output."""
    assert os.environ.get("JP_P9_TILE") is None
    x = Var(rand(N, C, H, W, seed=11) * 1.7 + 0.2, True)
    w = Var(rand(C, C, 3, 3, seed=12) * (9 * C) ** -0.5, True, torch.zeros(C, C, 3, 3, device=DEV))
    gamma, beta = rand(C, seed=13) * 0.2 + 1.0, rand(C, seed=14) * 0.1
    outs = []
    for fused in (True, False):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        with poisoned(), recording(Tape()):
            y = ops.conv2d(x, w, None, 1, 1, ops.PAD_ZERO, ops.ACT_NONE, bn_stats=fused)
            if fused:
                assert (y.bnst is not None) == (expect and ops.split_scheme() in (2, 3)), (y.bnst is not None, expect)
                if y.bnst is not None:
                    st_ws, parts = y.bnst
                    have = _fn("jp_conv2d_fwd_bn_stats_floats", N, H, W, C)
                    assert st_ws.numel() == have and parts * 2 * C <= have, (parts, C, have)
                    print(f"bn_stats {N}x{C}x{H}x{W}: {parts} partials per channel, {parts * 2 * C} of {have} floats")
            else:
                assert y.bnst is None
            z = ops.batchnorm_train(y, Var(gamma.clone(), True, torch.zeros(C, device=DEV)), Var(beta.clone(), True, torch.zeros(C, device=DEV)),
                                    rm, rv, relu=True)
        outs.append((y.t.clone(), z.t.clone(), rm.clone(), rv.clone()))
    (y1, z1, rm1, rv1), (y0, z0, rm0, rv0) = outs
    assert torch.equal(y1, y0)
    check(z1, z0, 2e-5, "bn", "normalised output, fused statistics vs the pass over y", atol=2e-5)
    check(rm1, rm0, 1e-5, "bn", "running mean", atol=1e-6)
    check(rv1, rv0, 1e-5, "bn", "running var", atol=1e-6)
    yd = y0.double().cpu()
    ref = F.relu(F.batch_norm(yd, None, None, gamma.double().cpu(), beta.double().cpu(), True, 0.1, 1e-5))
    check(z1, ref, 1e-4, "bn", "vs float64 batch norm", atol=1e-4)
    m64, v64 = yd.mean(dim=(0, 2, 3)), yd.var(dim=(0, 2, 3), unbiased=True)
    check(rm1, 0.1 * m64, 1e-5, "bn", "running mean vs float64", atol=1e-6)
    check(rv1, 0.9 + 0.1 * v64, 1e-5, "bn", "running var vs float64", atol=1e-6)
