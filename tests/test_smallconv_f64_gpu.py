"""The direct small-channel convolutions -- conv_small.hip (the Cout <= 4 kernels and the upsample-aware disparity head
sigmoid(Conv3x3_reflect(up2x(x)))) and conv_c16.hip (the 16 -> 16 BEV decoder layers) -- per element against FLOAT64 references
(tests/smallconv_ref.py on the CPU), at the smallest shapes that reach every launch path: channel counts that are no multiple of 4 or 8,
the three forward kernels of the head and its three weight-gradient tiers, the chunked and the tiled weight gradient of conv_small with
several segments and half-resolution offsets, 48 KiB of LDS weights, and a c16 weight gradient whose workgroups take a second tile
(tests/smallconv_cases.py holds the cases and mirrors the launch expressions; tests/test_smallconv_ref_cpu.py checks every path claim,
the reference itself, the term sums, the gate shares and the bars without a GPU).

Metric.  Every figure is max over the tensor of |got - ref64| / S, S = sum_k |a_k| |b_k| of that element's own terms (+ |bias| for the
forward; sum |g| for the bias gradient; S / 4 for the sigmoid outputs, compared with sigmoid(pre64)).  The backward reference is the
float64 convolution backward of g = dy y64 (1 - y64) for the sigmoid heads and of dy gate for ReLU / leaky ReLU, where the gate is
pre64 > 0 except where |pre64| < (forward bar) S: there the device decides (y > 0).  At most 0.5 % of a case may be decided by the
device (C2: 9.1e-5, C3: 3.4e-5 of the elements, from the reference alone), and no unambiguous gate may differ.

Every case runs forward and backward through ops.conv2d(..., srcs=...) under the library's profile tags: the disparity-head and c16
cases must launch no implicit-GEMM kernel at all; the conv_small cases none in the forward and, in the backward, only the input gradient
(the library has no direct dgrad for them: jp_conv2d_dgrad's exact-fp32 engine runs it, and it is held to the same bar).  The
weight-gradient tiers run through jp_conv2d_wgrad_src3 with the arguments ops.py passes: scratch of exactly the size
jp_conv2d_wgrad_src3_ws_floats returns, filled with NaN (fixed-order fold; two runs must be bit-identical), for the head also exactly
the 16 N hw floats of the gathered planes (atomics behind the gather), and no scratch (atomics); dw is pre-filled with a seeded tensor
and accumulate = 1, so the fold's += is checked too.

Measured bars.  For every quantity and family the error of two fp32 CPU evaluations was measured on the same cases, gates and metric:
ATen float32 (F.conv2d under autograd on the built input, one thread) and one sequential fp32 fmaf chain per element (smallconv_ref.chain32).  The
bar is 8 x the larger figure over the family's cases, rounded up to one significant digit; nothing is added for the hardware.  The
last column is what the kernels reached on an MI355X, copied from this file's printed output: measured on the device, for the reader
only -- no bar was derived from it.

  family quantity   ATen fp32   fp32 chain   bar     held to before (test_kernels_gpu.py, of max |ref|)   MI355X (measured on the device)
  up     fwd        1.48e-7     1.57e-7      2e-6    1.1e-4                                                8.95e-8
  up     dx         3.13e-7     9.51e-7      8e-6    2.1e-4                                                4.62e-7
  up     dw         2.73e-7     7.21e-7      6e-6    2.1e-4                                                5.29e-7
  up     db         3.53e-8     1.48e-7      2e-6    2.1e-4                                                1.40e-7
  small  fwd        2.55e-7     2.25e-7      3e-6    1.1e-4                                                3.20e-7
  small  dx         2.50e-7     2.48e-7      2e-6    1.1e-4                                                2.33e-7
  small  dw         2.64e-7     2.64e-7      3e-6    2.1e-4                                                8.47e-8
  small  db         3.78e-8     3.78e-8      4e-7    2.1e-4                                                3.99e-9
  c16    fwd        8.82e-7     1.27e-6      2e-5    1.1e-4                                                1.27e-6
  c16    dx         4.23e-7     4.18e-7      4e-6    2.1e-4                                                4.27e-7
  c16    dw         1.97e-7     1.97e-7      2e-6    2.1e-4                                                3.36e-8
  c16    db         8.39e-8     8.39e-8      7e-7    2.1e-4                                                5.09e-9

(The c16 forward figures come from C3, whose channel 1 is scaled by 2^10: one channel carries S.  The weight-gradient tiers are held to
the dw bar of their family; their largest figure on the device: 8.97e-8 (U2 without the partial-sum scratch).)

Every test prints its figures before it asserts them (pytest -s).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                                                 # noqa: E402
from jperceiver_amd import _lib                                                # noqa: E402
from jperceiver_amd._lib import call                                           # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                            # noqa: E402
from tests import smallconv_cases as C                                         # noqa: E402
from tests import smallconv_ref as R                                           # noqa: E402
from tests.test_bench_shapes_gpu import kernel_tags                            # noqa: E402

DEV = "cuda"
NAN = float("nan")


def _check(family, figures):
    """figures: [(label, error, quantity)...] -- print all, then assert all"""
    for label, err, q in figures:
        print(f"  {label:28s} {err:.3e}   bar {C.BARS[(family, q)]:.0e}")
    bad = [f"{label}: {err:.3e} > {C.BARS[(family, q)]:.0e}" for label, err, q in figures if not err <= C.BARS[(family, q)]]
    assert not bad, "; ".join(bad)


def _describe(case):
    if C.up_head(case):
        N, Cc, h, wd = case.N, case.srcs[0][0], case.H // 2, case.W // 2
        f, w = C.up_fwd(N, Cc, h, wd), C.up_wgrad(N, Cc, h, wd)
        return (f"{f['kernel']}, {f['wgs']} workgroups per image ({f['last']} live in the last), dgrad tail {Cc % 4}, weight gradient "
                f"{w['blocks']} blocks (tail {w['block_tail']}) x {w['nb']} bands of {w['band']} (last {w['last_band']})")
    if C.c16_ok(case):
        w = C.c16_wgrad(case)
        return f"c16: {w['ntiles']} tiles on {w['grid']} workgroups ({w['second_tile']} take a second tile)"
    w = C.small_wgrad(case)
    return f"conv_small: {'tiled' if w['tiled'] else 'chunked'} weight gradient, grid {w['grid']}, chunk {w['chunk']}, {w['lds']} bytes of LDS weights"


# --------------------------------------------------------------------------------------------------- through ops.conv2d
@pytest.mark.parametrize("name", list(C.CASES))
def test_direct_conv_f64(name):
    case, inp = C.CASES[name], C.inputs(name)
    print(f"  {name}: {_describe(case)}")
    xvs = [Var(x.to(DEV), True) for x in inp.xs]
    wv = Var(inp.w.to(DEV), True, torch.zeros_like(inp.w, device=DEV))
    bv = Var(inp.b.to(DEV), True, torch.zeros_like(inp.b, device=DEV)) if case.bias else None
    tape = Tape()
    with recording(tape), kernel_tags() as kf:
        y = ops.conv2d(None, wv, bv, 1, 1, int(case.reflect), case.act, srcs=[(v, up) for v, (_, up) in zip(xvs, case.srcs)])
    yt = y.t.cpu()
    y.g = inp.dy.to(DEV).clone()
    was = ops._WG_ON
    ops._WG_ON = False
    try:
        with kernel_tags() as kb:
            tape.backward()
    finally:
        ops._WG_ON = was
    torch.cuda.synchronize()
    if C.route(case) == "small":
        assert not kf.names, f"expected the direct forward kernel, the library launched {kf.names}"
        assert all("Dgrad" in n for n in kb.names), f"only the input gradient may run on the engine, the library launched {kb.names}"
    else:
        assert not kf.names and not kb.names, f"expected direct kernels only, the library launched {kf.names + kb.names}"
    got = dict(y=yt, dxs=[v.g.cpu() for v in xvs], dw=wv.g.cpu(), db=bv.g.cpu() if case.bias else None)
    for k, v in got.items():
        for t in (v if isinstance(v, list) else [v]):
            assert t is None or bool(torch.isfinite(t).all()), f"{k} is not finite"
    figs, up = C.evaluate(name, got)
    share = up.amb / yt.numel()
    print(f"  ambiguous gates {share:.2e} of the elements (cap {C.AMBIGUOUS_CAP}), unambiguous gates that differ: {up.wrong}")
    assert share <= C.AMBIGUOUS_CAP
    assert up.wrong == 0, "the device's gate differs from the reference's on an unambiguous element"
    _check(case.family, [(f"{name} {q}", e, q) for q, e in figs.items()])


# --------------------------------------------------------------------------------------------------- weight-gradient tiers, C ABI
@pytest.mark.parametrize("name", C.TIER_CASES)
def test_wgrad_scratch_tiers_f64(name):
    case, inp = C.CASES[name], C.inputs(name)
    want, S = C.tier_reference(name)
    s3 = []
    for i in range(3):
        s3 += [inp.xs[i].to(DEV), case.srcs[i][0], case.srcs[i][1]] if i < len(case.srcs) else [None, 0, 0]
    dims = (case.N, case.H, case.W, case.Cout, 3, 1, 1, int(case.reflect))
    full = int(_lib.lib().fn["jp_conv2d_wgrad_src3_ws_floats"](s3[1], s3[2], s3[4], s3[5], s3[7], s3[8], *dims))
    assert full == C.wgrad_ws_floats(case) > 0
    tiers = [("full scratch", full), ("full scratch again", full)]
    if C.up_head(case):
        tiers.append(("gathered planes only", C.up_wgrad(case.N, case.srcs[0][0], case.H // 2, case.W // 2)["d_floats"]))
    tiers.append(("no scratch", 0))
    dy, seed = inp.dy.to(DEV), C.dw_seed(name).to(DEV)
    runs = {}
    for label, n in tiers:
        dw = seed.clone()
        ws = torch.full((n,), NAN, device=DEV) if n else None
        call("jp_conv2d_wgrad_src3", *s3, dy, dw, *dims, 1, ws, n, None, None, None, None, ops._amax_ws(dy.device, None))
        torch.cuda.synchronize()
        runs[label] = dw.cpu()
    figs = [(f"{name} dw, {label}", R.worst(v, want, S), "dw") for label, v in runs.items()]
    for label, v in runs.items():
        assert bool(torch.isfinite(v).all()), f"{label}: dw is not finite"
    assert torch.equal(runs["full scratch"], runs["full scratch again"]), "the fixed-order fold must be bit-reproducible"
    _check(case.family, figs)
