"""The BatchNorm kernels and the per-channel sum (jperceiver_amd/csrc/bn.hip) per element against FLOAT64 references (tests/bn_ref.py on
the CPU), at the smallest shapes that put each kernel on the paths the training step runs: planes split into several chunks with a
ragged last one, float4 and scalar statistics, the fold of the partial sums, apply kernels whose threads stride, fp32 runs that fold
into the double in mid-loop, per-group statistics, and the fused stem tail's bands, tiles and pooled chunks (tests/bn_cases.py mirrors
chunking() and the launch expressions; tests/test_bn_ref_cpu.py checks every path claim, and every condition below, without a GPU).

The kernels are called through the C ABI (_lib.call), so that save_mean, save_invstd, the argmax bytes and the workspace are visible;
the workspace has exactly the size the query functions return and is filled with NaN first, so a partial sum that is read but never
written turns the statistics NaN.  The `groups` cases go through ops.batchnorm_train / ops.bn_relu_maxpool_train.  With a ReLU and no
residual the backward gets y = NULL (the gate is recomputed from x, as ops.batchnorm_train does); with a residual it gets y.

Ambiguous decisions.  A ReLU gate is ambiguous where the float64 pre-activation has |pre| < 2^-20 (|x sc| + |sh| + |residual|): a few
fp32 roundings of the terms fmaf combines.  There the reference backward takes the device's decision (y > 0); everywhere else the
device's gate must equal the reference's.  A pooled window is ambiguous where its two largest distinct candidates differ by less than
that allowance (the largest among its candidates); there the device's argmax byte is taken if it names a candidate that close to the
maximum, and everywhere else the byte must equal the reference's.  Exact ties are not ambiguous: zeros after the ReLU take the first
maximum in window order.  At most 0.5 % of a case may be decided by the device; the committed cases have no ambiguous window and no
ambiguous gate at all except (8, 128, 64, 64) relu 9.5e-7 / relu+res 1.4e-6, (16, 128, 96, 96) relu 4.2e-7 and (16, 128, 93, 89)
relu 3.5e-7 of their elements (computed by tests/test_bn_ref_cpu.py, from the reference alone).

Measured bars.  For every asserted quantity of the ordinary, fold, groups and fused-stem cases the error of an fp32 CPU evaluation
(ATen's native_batch_norm -- what F.batch_norm runs -- F.relu, F.max_pool2d under autograd, float32) against the float64 reference
was measured on the same cases, gates and metric; the bar is 8 x the largest such error over the cases, rounded up to one
significant digit.  No hardware allowance is added.  (fp32 figures: x86-64 CPU; tests/test_bn_ref_cpu.py recomputes them.)

  quantity       metric                                          fp32 evaluation   bar      held to before (test_kernels_gpu.py)
  y, pooled y    max |err| / max |ref|                           1.16e-7           1e-6     1.1e-4
  dx             max |err| / max |ref|                           2.24e-7           2e-6     3.1e-4
  dres           max |err| / max |ref|                           0                 0        1.1e-4
  dgamma         per channel |err| / max(|ref|, sum|terms| u)    1.54e-4           2e-3     -- (3.1e-4 of the largest channel)
  dbeta          per channel |err| / max(|ref|, sum|terms| u)    1.24e-4           1e-3     -- (3.1e-4 of the largest channel)
  dgamma / max   max |err| / max |ref| over the channels         2.24e-6           2e-5     3.1e-4
  dbeta / max    max |err| / max |ref| over the channels         9.20e-5           3.1e-4   3.1e-4   (the rule gives 8e-4: capped)
  running_mean   max |err| / max |ref|                           1.65e-7           2e-6     1.1e-4
  running_var    max |err| / max |ref|                           1.51e-7           2e-6     1.1e-4
  save_mean      max |err| / max |ref|                           5.83e-8           5e-7     not visible
  save_invstd    max |err| / max |ref|                           9.06e-8           8e-7     not visible

(2, 3, 1, 1), two elements per channel, is a special-statistics case by its size: its channel 0 holds 1.066 and 0.984, E[x^2] / var =
628, and dx there is the residue of terms 1e5 times larger.  The fp32 evaluation is 4.7e-4 off in its dx and the one-pass variance
2.8e-5 in invstd; either figure would loosen every other case's bar a thousandfold.  Its save_mean, running_mean, dbeta and dres stay
under the measured bars; save_invstd, y, dx, dgamma and running_var (with the unbiased factor 2) are held to the derived bounds below
with R = 1 (a thread sees one element), and take no part in the measured figures.

The per-channel figures of ATen are large because it sums a channel's terms in fp32 and some channels cancel to 1e-3 of their terms;
the kernels fold fp32 runs of 32 terms in double and stay far below (printed by every test).

Derived bounds, not measured (the derivations stand in tests/bn_cases.py: var_bound, special_bounds, channel_sum_bound,
eval_reference).  With u = 2^-24 and fp32 runs of R = 32 terms:

  variance       |var_dev - var_64| <= (3 R + 1) u E[x^2] (+ n 2^-53 E[x^2] of double arithmetic): the kernel forms E[x^2] - mean^2
                 from fp32 squares.  var_dev is recovered from save_invstd as invstd^-2 - eps, which has 3 u (var + eps) of its own.
                 For the channel 1000 + 0.5 randn this is 5.8 against a variance of 0.25: no digit of the variance is promised
                 there, and the oracle's two-pass variance is tighter.  y, dx, dgamma and the running statistics of the offset,
                 constant and zero channels are held to the bound propagated through invstd (relative 0.5 bound / (var + eps) + 4 u)
                 and the mean (R u E|x| + u |mean|); the ordinary channel of the same tensor is held to the measured bars, so an
                 ill-conditioned channel does not disturb its neighbours.
  x = 0.5        everything is exact: variance 0, save_mean 0.5, save_invstd == fl32(1 / sqrt(eps)), and y equals the documented
                 fmaf(x, sc, fmaf(-mean, sc, beta)) bit for bit.  That is NOT beta bit for bit: fmaf(-0.5, sc, beta) rounds
                 beta - 158 gamma to a float with an ulp of 1.5e-5, so y = beta + (that rounding error), within u (|mean sc| + 2 |beta|)
                 of beta.  The all-zero channel does give y == beta bit for bit.
  x = 3.3f       the fp32 run sums of 3.3f round, so mean and E[x^2] carry errors and the variance is not 0: the derived bounds.
  channel sum    |err| <= 33 u sum|x| + u |out0 + sum| + S u (sum|partial| + |out0|) per channel (+ n 2^-53 sum|x| for the float64
                 sum it is compared with); with the scratch the result is bit-reproducible: two runs must be equal.
  eval mode      |err| <= 8 u (|x sc| + |rm sc| + |beta| + |residual|) per element.

Every test prints its figures before it asserts them (pytest -s).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                                                 # noqa: E402
from jperceiver_amd import _lib                                                # noqa: E402
from jperceiver_amd._lib import call                                           # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                            # noqa: E402
from tests import bn_cases as C                                                # noqa: E402

DEV = "cuda"
BARS = C.BARS
NAN = float("nan")


def _check(figures):
    """figures: [(label, error, bar key)...] -- print all, then assert all"""
    for label, err, key in figures:
        print(f"  {label:34s} {err:.3e}   bar {BARS[key]:.0e}")
    bad = [f"{label}: {err:.3e} > {BARS[key]:.0e}" for label, err, key in figures if not err <= BARS[key]]
    assert not bad, "; ".join(bad)


def _finite(got):
    for k, v in got.items():
        if v is not None and v.is_floating_point():
            assert bool(torch.isfinite(v).all()), f"{k} is not finite"


def _poison(n, dtype=torch.float32):
    return torch.full((n,), NAN, device=DEV, dtype=dtype)


def _ws(query, *dims):
    """a workspace of exactly the size the library asks for, every double NaN"""
    n = int(_lib.lib().fn[query](*dims))
    return _poison(n, torch.float64)


def _dev(t):
    return None if t is None else t.to(DEV)


def _train_abi(inp, relu, nup, seeds=None):
    """jp_bn_train_fwd + jp_bn_train_bwd on one group -> the dict bn_cases.train_figures takes (CPU tensors)"""
    N, Cc, H, W = inp.x.shape
    HW = H * W
    x, gamma, beta, dy, res = (_dev(t) for t in (inp.x, inp.gamma, inp.beta, inp.dy, inp.residual))
    rm, rv = inp.rm.to(DEV).clone(), inp.rv.to(DEV).clone()
    y, sm, si = _poison(N * Cc * HW).view(N, Cc, H, W), _poison(Cc), _poison(Cc)
    call("jp_bn_train_fwd", x, gamma, beta, res, y, rm, rv, sm, si, _ws("jp_bn_ws_doubles", N, Cc, HW), N, Cc, HW, C.MOMENTUM, C.EPS,
         int(relu), nup, None, None, 0)
    dx = _poison(N * Cc * HW).view(N, Cc, H, W)
    dres = _poison(N * Cc * HW).view(N, Cc, H, W) if res is not None else None
    dg = seeds[0].to(DEV).clone() if seeds else _poison(Cc)
    db = seeds[1].to(DEV).clone() if seeds else _poison(Cc)
    # ReLU without a residual: y = NULL, the kernels recompute the gate from x
    call("jp_bn_train_bwd", dy, x, y if (relu and res is not None) else None, gamma, beta, sm, si, dx, dres, dg, db,
         _ws("jp_bn_ws_doubles", N, Cc, HW), N, Cc, HW, int(relu), 1 if seeds else 0, None)
    torch.cuda.synchronize()
    return dict(y=y.cpu(), save_mean=sm.cpu().view(1, Cc), save_invstd=si.cpu().view(1, Cc), rm=rm.cpu(), rv=rv.cpu(), dx=dx.cpu(),
                dres=dres.cpu() if dres is not None else None, dgamma=dg.cpu(), dbeta=db.cpu())


def _report_gates(ref, wrong):
    print(f"  ambiguous gates {ref.amb_share:.2e} of the elements (cap {C.MASK_CAP}), unambiguous gates that differ: {wrong}")
    assert ref.amb_share <= C.MASK_CAP
    assert wrong == 0, "the device's ReLU gate differs from the reference's on an unambiguous element"


# ------------------------------------------------------------------------------------------- train: chunks, paths, strides
def _sid(shape):
    return "x".join(str(v) for v in shape)


@pytest.mark.parametrize("shape,mode,nup", [(s, m, n) for s in C.TRAIN_CASES for m in C.MODES for n in (1, 2)],
                         ids=[f"{_sid(s)}-{m}-{n}" for s in C.TRAIN_CASES for m in C.MODES for n in (1, 2)])
def test_batchnorm_train_f64(shape, mode, nup):
    relu, res = C.MODES[mode]
    ref = C.train_reference(shape, mode)
    got = _train_abi(ref.inp, relu, nup)
    L = C.launch(shape[0], shape[1], shape[2] * shape[3])
    print(f"  {L.CH} chunks of {L.chunk} ({L.short} short), {L.stats} statistics, {L.apply} apply{' striding' if L.strides else ''}")
    _finite(got)
    figs, wrong = C.train_figures(ref, got, nup)
    _report_gates(ref, wrong)
    _check(figs)
    if C.two_per_channel(ref):       # a special-statistics case by its size (bn_cases.VARIANCE_FREE): the derived bounds for the rest
        bwd, _ = C.train_backward(ref, got["y"])
        bad = [b for c in range(shape[1]) for b in C.hold(C.derived_figures(ref, got, nup, bwd, c, run=1))]
        assert not bad, "; ".join(bad)


def test_batchnorm_train_accumulates_parameter_gradients():
    shape, mode = C.ACC_CASE
    ref = C.train_reference(shape, mode)
    bwd, _ = C.train_backward(ref, ref.y)
    seeds = (C.acc_seed(bwd.dgamma, 21), C.acc_seed(bwd.dbeta, 22))
    got = _train_abi(ref.inp, True, 1, seeds)
    _finite(got)
    figs, wrong = C.train_figures(ref, got, 1, seeds)
    _report_gates(ref, wrong)
    _check(figs)


@pytest.mark.parametrize("shape", list(C.FOLD_CASES), ids=_sid)
def test_batchnorm_train_fp32_runs_fold_in_mid_loop(shape):
    ref = C.train_reference(shape, "relu")
    got = _train_abi(ref.inp, True, 1)
    L = C.launch(shape[0], shape[1], shape[2] * shape[3])
    print(f"  {L.iters} {L.stats} iterations per thread: the fold after {C.FOLD4 if L.stats == 'float4' else C.FOLD1} fires before the end")
    _finite(got)
    figs, wrong = C.train_figures(ref, got, 1)
    _report_gates(ref, wrong)
    _check(figs)


# ------------------------------------------------------------------------------------------- groups, through ops
def _ops_leaves(inp):
    xv = Var(inp.x.to(DEV), True)
    gv = Var(inp.gamma.to(DEV), True, torch.zeros_like(inp.gamma, device=DEV))
    bv = Var(inp.beta.to(DEV), True, torch.zeros_like(inp.beta, device=DEV))
    return xv, gv, bv, inp.rm.to(DEV).clone(), inp.rv.to(DEV).clone()


@pytest.mark.parametrize("name,mode,nup", [(n, m, u) for n in C.GROUP_CASES for m, u in C.GROUP_RUNS])
def test_batchnorm_train_groups_f64(name, mode, nup):
    shape, groups = C.GROUP_CASES[name]
    relu, res = C.MODES[mode]
    ref = C.train_reference(shape, mode, groups)
    inp = ref.inp
    xv, gv, bv, rm, rv = _ops_leaves(inp)
    rvv = Var(inp.residual.to(DEV), True) if res else None
    tape = Tape()
    with recording(tape):
        y = ops.batchnorm_train(xv, gv, bv, rm, rv, rvv, relu, C.MOMENTUM, C.EPS, nup, groups)
    y.g = inp.dy.to(DEV).clone()
    yt = y.t.cpu()
    tape.backward()
    torch.cuda.synchronize()
    got = dict(y=yt, rm=rm.cpu(), rv=rv.cpu(), dx=xv.g.cpu(), dres=rvv.g.cpu() if res else None, dgamma=gv.g.cpu(), dbeta=bv.g.cpu())
    _finite(got)
    # the saved statistics stay inside the op: the reference's stand in, so that the shared figure list applies
    got["save_mean"], got["save_invstd"] = ref.mean.float(), ref.invstd.float()
    figs, wrong = C.train_figures(ref, got, nup)
    _report_gates(ref, wrong)
    _check([f for f in figs if not f[2].startswith("save_")])


# ------------------------------------------------------------------------------------------- fused stem tail
def _pool_abi(inp, nup, seeds=None):
    N, Cc, H, W = inp.x.shape
    OH, OW = H // 2, W // 2
    x, gamma, beta, dpool = (_dev(t) for t in (inp.x, inp.gamma, inp.beta, inp.dy))
    rm, rv = inp.rm.to(DEV).clone(), inp.rv.to(DEV).clone()
    pooled, sm, si = _poison(N * Cc * OH * OW).view(N, Cc, OH, OW), _poison(Cc), _poison(Cc)
    idx = torch.full((N, Cc, OH, OW), 255, device=DEV, dtype=torch.uint8)
    call("jp_bn_relu_pool_fwd", x, gamma, beta, pooled, idx, rm, rv, sm, si, _ws("jp_bn_ws_doubles", N, Cc, H * W), N, Cc, H, W,
         C.MOMENTUM, C.EPS, nup, None)
    dx = _poison(N * Cc * H * W).view(N, Cc, H, W)
    dg = seeds[0].to(DEV).clone() if seeds else _poison(Cc)
    db = seeds[1].to(DEV).clone() if seeds else _poison(Cc)
    call("jp_bn_relu_pool_bwd", dpool, idx, x, gamma, beta, sm, si, dx, dg, db, _ws("jp_bn_relu_pool_bwd_ws_doubles", N, Cc, H, W),
         N, Cc, H, W, 1 if seeds else 0)
    torch.cuda.synchronize()
    return dict(y=pooled.cpu(), idx=idx.cpu(), save_mean=sm.cpu().view(1, Cc), save_invstd=si.cpu().view(1, Cc), rm=rm.cpu(),
                rv=rv.cpu(), dx=dx.cpu(), dgamma=dg.cpu(), dbeta=db.cpu())


def _pool_check(ref, got, nup, seeds=None):
    _finite(got)
    figs, wrong_idx, wrong_gate = C.pool_figures(ref, got, nup, seeds)
    print(f"  ambiguous windows {ref.win_share:.2e}, ambiguous gates {ref.amb_share:.2e} (cap {C.MASK_CAP}); argmax bytes that differ "
          f"{wrong_idx}, gates that differ {wrong_gate}")
    assert ref.win_share <= C.MASK_CAP and ref.amb_share <= C.MASK_CAP
    assert wrong_idx == 0, "an argmax byte differs from the first maximum of the reference on an unambiguous window"
    assert wrong_gate == 0
    return figs


@pytest.mark.parametrize("name", [n for n, c in C.POOL_CASES.items() if c[3] == "abi"])
def test_bn_relu_pool_f64(name):
    shape, groups, nup, _ = C.POOL_CASES[name]
    ref = C.pool_reference(name)
    L = C.pool_launch(*shape)
    print(f"  pooled {L.OH}x{L.OW}: {L.bands} bands of {L.RB} rows ({L.band_short} short), {L.tile_rows}x{L.tile_cols} tiles, statistics "
          f"in {L.stats.CH} chunks, pooled reduce in {L.pooled.CH} chunks of {L.pooled.chunk} ({L.pooled.short} short)")
    _check(_pool_check(ref, _pool_abi(ref.inp, nup), nup))


def test_bn_relu_pool_accumulates_parameter_gradients():
    name = C.POOL_ACC_CASE
    ref = C.pool_reference(name)
    bwd, _, _ = C.pool_backward(ref, ref.pooled.float(), ref.idx)
    seeds = (C.acc_seed(bwd.dgamma, 23), C.acc_seed(bwd.dbeta, 24))
    _check(_pool_check(ref, _pool_abi(ref.inp, 1, seeds), 1, seeds))


def test_bn_relu_pool_groups_f64():
    """the pose-stem configuration through ops.bn_relu_maxpool_train: two groups, two running-stat updates each, in order"""
    name = "4x16x64x128 g2"
    shape, groups, nup, _ = C.POOL_CASES[name]
    ref = C.pool_reference(name)
    inp = ref.inp
    xv, gv, bv, rm, rv = _ops_leaves(inp)
    seen = {}
    real = ops.call

    def spy(fn, *a):                       # the argmax bytes stay inside the op: take them as the forward call leaves them
        real(fn, *a)
        if fn == "jp_bn_relu_pool_fwd":
            seen.setdefault("idx", []).append(a[4])
    tape = Tape()
    ops.call = spy
    try:
        with recording(tape):
            y = ops.bn_relu_maxpool_train(xv, gv, bv, rm, rv, C.MOMENTUM, C.EPS, nup, groups)
    finally:
        ops.call = real
    y.g = inp.dy.to(DEV).clone()
    yt = y.t.cpu()
    tape.backward()
    torch.cuda.synchronize()
    assert len(seen["idx"]) == groups
    got = dict(y=yt, idx=torch.cat([t.cpu() for t in seen["idx"]], 0), rm=rm.cpu(), rv=rv.cpu(), dx=xv.g.cpu(), dgamma=gv.g.cpu(),
               dbeta=bv.g.cpu())
    figs = _pool_check(ref, dict(got, save_mean=ref.mean.float(), save_invstd=ref.invstd.float()), nup)
    _check([f for f in figs if not f[2].startswith("save_")])


# ------------------------------------------------------------------------------------------- special statistics
@pytest.mark.parametrize("name", list(C.SPECIAL_TENSORS))
def test_batchnorm_special_statistics(name):
    ref = C.special_reference(name)
    inp = ref.inp
    got = _train_abi(inp, False, 1)
    _finite(got)
    is_max = float(torch.tensor(1.0 / math.sqrt(C.EPS32), dtype=torch.float32))            # fl32(1 / sqrt(eps))
    figs, bad = [], []
    for c, kind in enumerate(C.SPECIAL_TENSORS[name]):
        print(f" channel {c}: {kind}")
        mean, var, invstd = (float(t[0, c]) for t in (ref.mean, ref.var, ref.invstd))
        sm, si = float(got["save_mean"][0, c]), float(got["save_invstd"][0, c])
        y, dx, x = got["y"][:, c], got["dx"][:, c], inp.x[:, c]
        if kind == "plain":                # the neighbour of the ill-conditioned channels: the measured bars
            figs += [(f"[{c}] y / max", C.err_max(y, ref.y[:, c]), "y"), (f"[{c}] dx / max", C.err_max(dx, ref.bwd.dx[:, c]), "dx"),
                     (f"[{c}] save_mean", abs(sm - mean) / abs(mean), "save_mean"),
                     (f"[{c}] save_invstd", abs(si - invstd) / invstd, "save_invstd"),
                     (f"[{c}] running_mean", abs(float(got["rm"][c]) - float(ref.rm[1][c])) / max(abs(float(inp.rm[c])), abs(mean)),
                      "running_mean"),
                     (f"[{c}] running_var", abs(float(got["rv"][c]) - float(ref.rv[1][c])) / float(ref.rv[1][c]), "running_var"),
                     (f"[{c}] dgamma", abs(float(got["dgamma"][c]) - float(ref.bwd.dgamma[c]))
                      / max(abs(float(ref.bwd.dgamma[c])), float(ref.bwd.abs_dgamma[c]) * C.U), "dgamma")]
            continue
        bad += C.hold(C.derived_figures(ref, got, 1, ref.bwd, c))
        if kind in ("const", "const-", "zero"):          # exact: every sum of the kernel is exact in fp32 and in double
            v = C.SPECIAL_VALUES[kind]
            off_beta = float((y.double() - float(inp.beta[c])).abs().max())
            print(f"  exact: save_mean {sm!r}, save_invstd {si!r} (fl32(1/sqrt(eps)) = {is_max!r}), max |y - beta| {off_beta:.3e}")
            assert sm == v and si == is_max, "a constant channel whose squares are exact must have variance exactly 0"
            sc = (got["save_invstd"][0, c].double() * inp.gamma[c].double()).float()
            sh = C.fmaf32(-got["save_mean"][0, c], sc, inp.beta[c])
            assert torch.equal(y, C.fmaf32(x, sc, sh)), "y is not fmaf(x, sc, fmaf(-mean, sc, beta)) bit for bit"
            assert off_beta <= C.U * (abs(v * float(sc)) + 2 * abs(float(inp.beta[c])))
            if kind == "zero":
                assert bool((y == inp.beta[c]).all()), "an all-zero channel must give beta bit for bit"
    figs.append(("dbeta per channel (all channels)", C.err_channels(got["dbeta"], ref.bwd.dbeta, ref.bwd.dbeta, ref.bwd.abs_dbeta), "dbeta"))
    for label, err, key in figs:
        print(f"  {label:44s} {err:.3e}   bar {BARS[key]:.0e}")
        if not err <= BARS[key]:
            bad.append(f"{label}: {err:.3e} > {BARS[key]:.0e}")
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------- channel sum
@pytest.mark.parametrize("shape", C.CHANNEL_SUM_CASES, ids=_sid)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_channel_sum_f64(shape, accumulate):
    N, Cc, H, W = shape
    x, out0 = C.channel_sum_inputs(shape)
    want, bound = C.channel_sum_bound(x, out0 if accumulate else None)
    xd = x.to(DEV)
    start = out0.to(DEV) if accumulate else _poison(Cc)
    runs = {}
    for label, scratch in (("scratch", True), ("scratch again", True), ("atomics", False)):
        out = start.clone()
        ws = _poison(int(_lib.lib().fn["jp_channel_sum_ws_floats"](N, Cc, H * W))) if scratch else None
        call("jp_channel_sum", xd, out, N, Cc, H * W, accumulate, ws)
        runs[label] = out.cpu()
    worst = {k: float(((v.double() - want).abs() / bound).max()) for k, v in runs.items()}
    print(f"  {C.chunking(N, Cc, H * W)[0]} chunks, S = {N * C.chunking(N, Cc, H * W)[0]}; largest |err| / bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; smallest bound / |sum| {float((bound / want.abs()).min()):.2e}")
    for k, v in runs.items():
        assert bool(torch.isfinite(v).all()), k
    assert torch.equal(runs["scratch"], runs["scratch again"]), "the scratch route must be bit-reproducible"
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------- eval mode
@pytest.mark.parametrize("shape", C.EVAL_CASES, ids=_sid)
@pytest.mark.parametrize("relu,res", [(False, False), (True, True), (True, False)])
def test_batchnorm_eval_f64(shape, relu, res):
    N, Cc, H, W = shape
    inp = C.eval_inputs(shape)
    want, bound = C.eval_reference(inp, relu, res)
    y = _poison(N * Cc * H * W).view(N, Cc, H, W)
    call("jp_bn_eval_fwd", _dev(inp.x), _dev(inp.gamma), _dev(inp.beta), _dev(inp.rm), _dev(inp.rv), _dev(inp.residual) if res else None,
         y, N, Cc, H * W, C.EPS, int(relu))
    y = y.cpu()
    worst = float(((y.double() - want).abs() / bound).max())
    print(f"  largest |err| / bound {worst:.3f}; y / max {C.err_max(y, want):.3e}; running_var[0] = {float(inp.rv[0])}")
    assert bool(torch.isfinite(y).all())
    assert worst <= 1.0
