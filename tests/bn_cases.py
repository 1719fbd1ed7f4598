"""Cases, seeded inputs, launch mirrors, ambiguity masks, error metrics, derived bounds and bars shared by tests/test_bn_ref_cpu.py (which
checks every condition on the float64 reference without a GPU) and tests/test_bn_f64_gpu.py (which runs the kernels of
jperceiver_amd/csrc/bn.hip).  Everything here is CPU-only torch; nothing imports the HIP library."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests import bn_ref as R
from tests.photometric_cases import err_max, round_up_1sig          # noqa: F401  (the suite's metrics and rounding rule)

F64 = torch.float64
U = 2.0 ** -24                # unit roundoff of fp32
MASK_CAP = 0.005              # at most this share of a case's elements / windows may take the device's decision
AMBIGUOUS = 2.0 ** -20        # |pre| below this times the magnitudes fmaf combines: a few fp32 roundings could decide the sign
EPS, MOMENTUM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))          # the eps the kernels see

# ------------------------------------------------------------------------------------------- launch mirrors
# The constants of bn.hip that decide which path a shape takes, as they stand in the source (tests/test_bn_ref_cpu.py finds every
# string verbatim, so a changed constant fails there), next to their Python mirrors.
BN_HIP = "jperceiver_amd/csrc/bn.hip"
TPB = 256
SOURCE_LINES = {
    "tpb": "constexpr int TPB = 256;",
    "chunking": ("void chunking(int N, int C, int HW, int* CH, int* chunk) {\n"
                 "    int ch = std::max(1, 2048 / std::max(1, N * C));\n"
                 "    ch = std::min(ch, std::max(1, HW / 2048));\n"
                 "    *chunk = (HW + ch - 1) / ch;\n"
                 "    *CH = (HW + *chunk - 1) / *chunk;\n"
                 "}"),
    "stats_path": "if (((HW | chunk) & 3) == 0) {",
    "apply_path": "if ((HW & 3) == 0) {",
    "gx": "const int gx = std::min(jp_cdiv(HW, 4 * TPB), 64);",
    "pool_tile": "constexpr int SP_TW = 64, SP_TH = 16;",
    "pool_band": "const int RB = OH >= 128 ? 32 : 8",
    "fold4": "if (++run == 8) { s += fs; q += fq; fs = fq = 0.f; run = 0; }",
    "fold1": "if (++run == 32) { s += fs; q += fq; fs = fq = 0.f; run = 0; }",
    "fold_sum": "if (++run == 32) { s += fs; fs = 0.f; run = 0; }",
}
FOLD4, FOLD1 = 8, 32          # iterations of a thread between two folds of its fp32 run into the double: float4 path, scalar path
RUN = 32                      # ... which is 32 fp32 terms either way
GX_CAP = 64
SP_TW, SP_TH = 64, 16


def chunking(N, C, HW):
    """-> (CH, chunk): chunks per plane and elements per chunk"""
    ch = max(1, 2048 // max(1, N * C))
    ch = min(ch, max(1, HW // 2048))
    chunk = (HW + ch - 1) // ch
    return (HW + chunk - 1) // chunk, chunk


def launch(N, C, HW):
    """what bn_stats / bn_bwd_reduce and the apply kernels do with an (N, C, HW) tensor"""
    CH, chunk = chunking(N, C, HW)
    float4 = ((HW | chunk) & 3) == 0
    per_thread = -(-((chunk // 4) if float4 else chunk) // TPB)          # loop iterations of thread 0 in a full chunk
    apply4 = HW % 4 == 0
    units = HW // 4 if apply4 else HW
    gx = min(-(-HW // (4 * TPB)), GX_CAP)
    return SimpleNamespace(CH=CH, chunk=chunk, S=N * CH, stats="float4" if float4 else "scalar", short=CH * chunk - HW,
                           iters=per_thread, folds=per_thread > (FOLD4 if float4 else FOLD1), apply="float4" if apply4 else "scalar",
                           gx=gx, strides=units > gx * TPB)


def bn_ws_doubles(N, C, HW):
    return 2 * C * N * chunking(N, C, HW)[0]


def pool_bwd_ws_doubles(N, C, H, W):
    return bn_ws_doubles(N, C, (H // 2) * (W // 2)) + C


def channel_sum_ws_floats(N, C, HW):
    return C * N * chunking(N, C, HW)[0]


def pool_launch(N, C, H, W):
    OH, OW = H // 2, W // 2
    RB = 32 if OH >= 128 else 8
    return SimpleNamespace(OH=OH, OW=OW, RB=RB, bands=-(-OH // RB), band_short=-(-OH // RB) * RB - OH,
                           tile_rows=-(-OH // SP_TH), tile_row_short=-(-OH // SP_TH) * SP_TH - OH,
                           tile_cols=-(-OW // SP_TW), tile_col_short=-(-OW // SP_TW) * SP_TW - OW,
                           stats=launch(N, C, H * W), pooled=launch(N, C, OH * OW))


# ------------------------------------------------------------------------------------------- cases
# (N, C, H, W) -> what the case exists for, as launch() must report it (tests/test_bn_ref_cpu.py asserts every entry)
TRAIN_CASES = {
    (2, 3, 1, 1): dict(CH=1, chunk=1, stats="scalar", apply="scalar", count=2),              # unbiased factor 2
    (2, 3, 1, 3): dict(CH=1, chunk=3, stats="scalar", apply="scalar", count=6),              # HW < 4
    (3, 5, 7, 9): dict(CH=1, chunk=63, stats="scalar", apply="scalar"),
    (2, 3, 8, 1026): dict(CH=4, chunk=2052, stats="float4", short=0, apply="float4"),
    (2, 3, 4, 2564): dict(CH=5, chunk=2052, stats="float4", short=4, apply="float4"),        # ragged last chunk
    (2, 3, 8, 1025): dict(CH=4, chunk=2050, stats="scalar", short=0, apply="float4"),        # HW % 4 == 0, chunk % 4 != 0
    (1, 2, 1, 6151): dict(CH=3, chunk=2051, stats="scalar", short=2, apply="scalar", strides=True),   # odd plane base offsets; the
    # scalar apply path strides as soon as HW > 256 gx (gx counts 1024 elements per workgroup, a scalar workgroup covers 256)
    (1, 2, 4, 16385): dict(CH=32, chunk=2049, stats="scalar", short=28, apply="float4", strides=True),
    (8, 128, 64, 64): dict(CH=2, chunk=2048, stats="float4", short=0, apply="float4"),       # ch limited by N * C
}
FOLD_CASES = {
    (16, 128, 96, 96): dict(CH=1, chunk=9216, stats="float4", iters=9, folds=True),          # the run == 8 fold fires mid-loop
    (16, 128, 93, 89): dict(CH=1, chunk=8277, stats="scalar", iters=33, folds=True, strides=True),   # the run == 32 fold fires mid-loop
}
MODES = {"plain": (False, False), "relu": (True, False), "relu+res": (True, True)}          # name -> (relu, residual)
ACC_CASE = ((2, 3, 4, 2564), "relu")                  # run with acc_param_grads = 1 onto seeded dgamma / dbeta as well

# fused stem tail: name -> (shape, groups, n_updates, route)
POOL_CASES = {
    "2x3x4x4": ((2, 3, 4, 4), 1, 1, "abi"),            # smallest legal map, one partial tile
    "2x4x260x64": ((2, 4, 260, 64), 1, 1, "abi"),      # RB 32, 5 bands (ragged), 9 tile rows (ragged), half a tile wide, pooled reduce in 2 chunks
    "1x2x4x6152": ((1, 2, 4, 6152), 1, 2, "abi"),      # pooled plane in 3 ragged chunks, 49 tile columns (last 4 wide), the `right` edge
    "4x16x64x128 g2": ((4, 16, 64, 128), 2, 2, "ops"),  # the pose-stem configuration
}
POOL_ACC_CASE = "2x4x260x64"
GROUP_CASES = {"6x5x7x9 g3": ((6, 5, 7, 9), 3), "4x3x8x1026 g2": ((4, 3, 8, 1026), 2)}
GROUP_RUNS = (("relu", 2), ("relu+res", 1))           # (mode, n_updates) of every groups case
SPECIAL_SHAPE = (2, 4, 8, 1026)
CHANNEL_SUM_CASES = ((2, 3, 8, 1026), (1, 2, 1, 6151), (3, 5, 7, 9), (16, 128, 93, 89))
EVAL_CASES = ((3, 5, 7, 9), (1, 2, 4, 16385))


# ------------------------------------------------------------------------------------------- bars
# Largest error of an fp32 CPU evaluation (ATen's native_batch_norm -- what F.batch_norm runs -- F.relu and F.max_pool2d under autograd,
# float32, as tests/test_kernels_gpu.py uses) against tests/bn_ref.py in float64, over every ordinary, fold, fused-stem and groups
# case: same inputs, gates and metric as the GPU assertions (tests/test_bn_ref_cpu.py recomputes them).
#   y, dx, dres, save_mean, save_invstd, running_mean, running_var:  max |err| / max |ref| over the tensor
#   dgamma, dbeta:  per channel, |err| / max(|ref|, sum |terms| 2^-24); the largest channel
#   dgamma_max, dbeta_max:  max |err| / max |ref| over the channels (the metric of tests/test_kernels_gpu.py)
# Measured with torch 2 on an x86-64 CPU; the case that gave the figure stands behind it.
ORACLE_ERR = {
    "y": 1.161e-07,              # pool 2x4x260x64
    "dx": 2.240e-07,             # pool 2x4x260x64
    "dres": 0.0,                 # dy times the gate: exact in any precision
    "dgamma": 1.542e-04,         # (1, 2, 1, 6151) relu: a channel whose sum cancels to 1e-3 of its terms, summed in fp32 by ATen
    "dbeta": 1.238e-04,          # (2, 3, 8, 1026) relu+res: likewise
    "running_mean": 1.647e-07,   # (2, 3, 8, 1025), two updates
    "running_var": 1.512e-07,    # (8, 128, 64, 64), two updates
    "save_mean": 5.825e-08,      # (16, 128, 96, 96)
    "save_invstd": 9.063e-08,    # (16, 128, 96, 96)
    "dgamma_max": 2.240e-06,     # pool 1x2x4x6152
    "dbeta_max": 9.200e-05,      # (1, 2, 4, 16385) relu: 65 540 terms per channel summed in fp32
}
# What tests/test_kernels_gpu.py holds the same quantity to (rtol + atol of `close`, relative to max(1, max |ref|)); save_mean and
# save_invstd were not visible there.  The per-channel metric is new.
FORMER_BARS = {"y": 1.1e-4, "dx": 3.1e-4, "dres": 1.1e-4, "dgamma": None, "dbeta": None, "running_mean": 1.1e-4, "running_var": 1.1e-4,
               "save_mean": None, "save_invstd": None, "dgamma_max": 3.1e-4, "dbeta_max": 3.1e-4}
# The case with TWO elements per channel, (2, 3, 1, 1), is a special-statistics case by its size: its channel 0 holds 1.066 and 0.984,
# E[x^2] / var = 628, and dx is (dy0 - dy1) / 2 * eps / (var + eps) times the scale -- the residue of terms 1e5 times larger.  The
# one-pass variance of the kernels is 2.8e-5 off there in invstd, the two-pass fp32 evaluation 4.7e-4 off in dx; measured over all
# cases either would loosen every other case's bar a thousandfold.  Its variance-dependent quantities are held to the DERIVED bounds
# (derived_figures) and take no part in the measured figures; the others (VARIANCE_FREE) stay under the measured bars.
VARIANCE_FREE = ("save_mean", "running_mean", "dbeta", "dbeta_max", "dres")
BAR_NOTES = {
    "dres": "the fp32 evaluation is exact, so the bar is 0: the device must be exact too",
    "dgamma_max": "this file's addition to the per-channel metric: the rule, capped by what tests/test_kernels_gpu.py held",
    "dbeta_max": "as dgamma_max: the rule gives 8e-4 (ATen sums 65 540 terms in fp32), the former bar 3.1e-4 holds instead",
}


def bar_rule(v, former=None):
    """8 x the fp32 evaluation's error rounded up to one significant digit (the rule of tests/photometric_cases.py), and never looser
    than what the quantity was held to before; no hardware allowance is added"""
    bar = round_up_1sig(8 * v) if v > 0 else 0.0
    return bar if former is None else min(bar, former)


BARS = {k: bar_rule(v, FORMER_BARS[k]) for k, v in ORACLE_ERR.items()}


def err_channels(got, want, grad, abs_terms):
    """per channel |got - want| / max(|grad|, sum |terms| 2^-24): the largest channel (one wrong channel cannot hide behind a large
    one).  want: the gradient, or seed + gradient in accumulate mode; the scale is always the gradient's own.  A channel without a
    single open gate has no terms: its gradient is exactly 0 and any other value is an infinite error"""
    e = (got.detach().double() - want).abs()
    return float((e / torch.maximum(grad.abs(), abs_terms * U).clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------- inputs
def _gen(seed, shape):
    return torch.Generator().manual_seed(7000 + 131 * seed + sum(s * p for s, p in zip(shape, (1, 3, 5, 7))) % 1009)


def params(C, g):
    """gamma about 1 with spread 0.2, gamma[0] = -0.7 (max and affine do not commute), gamma[1] = 0 (sc == 0: the gate depends on beta
    alone); beta small; running statistics at non-trivial values"""
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    gamma[0] = -0.7
    if C > 1:
        gamma[1] = 0.0
    beta = 0.1 * torch.randn(C, generator=g)
    rm = 0.3 * torch.randn(C, generator=g)
    rv = 0.5 + torch.rand(C, generator=g)
    return gamma, beta, rm, rv


def train_inputs(shape, res=False, seed=0, groups=1):
    """-> SimpleNamespace(x, gamma, beta, rm, rv, dy, residual) of float32 tensors.  groups > 1: group g's data is x * (1 + g) + 3 g, so
    a statistic taken over the wrong slice is far off"""
    N, C, H, W = shape
    g = _gen(seed, shape)
    x = torch.randn(N, C, H, W, generator=g) * 2 + 0.5
    gamma, beta, rm, rv = params(C, g)
    dy = torch.randn(N, C, H, W, generator=g)
    residual = torch.randn(N, C, H, W, generator=g) if res else None
    Ng = N // groups
    for k in range(1, groups):
        x[k * Ng:(k + 1) * Ng] = x[k * Ng:(k + 1) * Ng] * (1 + k) + 3 * k
    return SimpleNamespace(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, dy=dy, residual=residual)


def pool_inputs(name, seed=0):
    shape, groups, nup, route = POOL_CASES[name]
    N, C, H, W = shape
    g = _gen(seed + 50, shape)
    x = torch.randn(N, C, H, W, generator=g) * 2 + 0.3
    gamma, beta, rm, rv = params(C, g)
    dpool = torch.randn(N, C, H // 2, W // 2, generator=g)
    Ng = N // groups
    for k in range(1, groups):
        x[k * Ng:(k + 1) * Ng] = x[k * Ng:(k + 1) * Ng] * (1 + k) + 3 * k
    return SimpleNamespace(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, dy=dpool, residual=None)


def acc_seed(ref_grad, seed):
    """the buffer the accumulate-mode runs add onto: -(0.25 .. 0.75) of the gradient per channel (a dropped add, or one applied twice,
    moves the result by that share; the sum stays below the gradient, so its own fp32 rounding stays below the gradient's)"""
    g = torch.Generator().manual_seed(seed)
    return (-ref_grad.double() * (0.25 + 0.5 * torch.rand(ref_grad.shape, generator=g, dtype=F64))).float()


# ------------------------------------------------------------------------------------------- references
def _d(t):
    return None if t is None else t.double()


def _cat(ts):
    return ts[0] if len(ts) == 1 else torch.cat(ts, 0)


def _train_ref(inp, relu, groups=1):
    """float64 forward of one (grouped) train call -> per group BnFwd, running statistics after 1 and 2 updates per group (in order),
    ambiguity mask of the ReLU gate"""
    outs, rm, rv = {}, {}, {}
    for nup in (1, 2):
        o, rm[nup], rv[nup] = R.grouped_fwd(R.bn_train_fwd, groups, _d(inp.x), _d(inp.gamma), _d(inp.beta), _d(inp.rm), _d(inp.rv),
                                            _d(inp.residual), relu=relu, eps=EPS32, momentum=MOMENTUM, n_updates=nup)
        outs = outs or o                       # y and the batch statistics do not depend on n_updates
    pre = _cat([o.pre for o in outs])
    terms = _cat([o.terms for o in outs])
    amb = (pre.abs() < AMBIGUOUS * terms) if relu else torch.zeros_like(pre, dtype=torch.bool)
    return SimpleNamespace(inp=inp, relu=relu, groups=groups, fwd=outs, y=_cat([o.y for o in outs]), pre=pre, amb=amb,
                           mean=torch.stack([o.mean for o in outs], 0), var=torch.stack([o.var for o in outs], 0),
                           invstd=torch.stack([o.invstd for o in outs], 0), rm=rm, rv=rv,
                           amb_share=float(amb.double().mean()))


@functools.lru_cache(maxsize=6)
def train_reference(shape, mode, groups=1):
    relu, res = MODES[mode]
    return _train_ref(train_inputs(shape, res, groups=groups), relu, groups)


def train_backward(ref, y_got):
    """the reference backward of a train case with the DEVICE's ReLU decision (y_got > 0) on the ambiguous elements.
    -> BnBwd summed over the groups (dx / dres concatenated), number of unambiguous elements whose gate differs"""
    inp = ref.inp
    gate, wrong = None, 0
    if ref.relu:
        dev = y_got > 0
        own = ref.pre > 0
        wrong = int(((dev != own) & ~ref.amb).sum())
        gate = torch.where(ref.amb, dev, own)
    Ng = inp.x.shape[0] // ref.groups
    parts = []
    for k in range(ref.groups):
        sl = slice(k * Ng, (k + 1) * Ng)
        parts.append(R.bn_train_bwd(_d(inp.dy[sl]), _d(inp.x[sl]), ref.mean[k], ref.invstd[k], _d(inp.gamma),
                                    gate[sl] if gate is not None else None))
    ref.gate = gate                      # (the derived bounds need the gate that was used)
    return _sum_bwd(parts), wrong


def two_per_channel(ref):
    return ref.inp.x.numel() // ref.inp.x.shape[1] // ref.groups == 2


def _sum_bwd(parts):
    return R.BnBwd(_cat([p.dx for p in parts]), _cat([p.dres for p in parts]), sum(p.dgamma for p in parts),
                   sum(p.dbeta for p in parts), sum(p.abs_dgamma for p in parts), sum(p.abs_dbeta for p in parts))


def train_figures(ref, got, nup, seeds=None):
    """got: dict of float32 CPU tensors y, save_mean (G, C), save_invstd (G, C), rm, rv, dx, dres (or None), dgamma, dbeta.
    seeds: (dgamma seed, dbeta seed) of an accumulate-mode run.  -> [(label, error, bar key)...], wrong gates"""
    bwd, wrong = train_backward(ref, got["y"])
    want_dg, want_db = bwd.dgamma, bwd.dbeta
    if seeds is not None:
        want_dg, want_db = want_dg + seeds[0].double(), want_db + seeds[1].double()
    tag = " (add mode)" if seeds is not None else ""
    figs = [("y / max", err_max(got["y"], ref.y), "y"),
            ("dx / max", err_max(got["dx"], bwd.dx), "dx")] + _shared_figures(ref, got, nup, bwd, want_dg, want_db, tag)
    if got.get("dres") is not None:
        figs.append(("dres / max", err_max(got["dres"], bwd.dres), "dres"))
    if two_per_channel(ref):             # the rest is held to the derived bounds: derived_figures
        figs = [f for f in figs if f[2] in VARIANCE_FREE]
    return figs, wrong


def _shared_figures(ref, got, nup, bwd, want_dg, want_db, tag):
    return [("save_mean / max", err_max(got["save_mean"], ref.mean), "save_mean"),
            ("save_invstd / max", err_max(got["save_invstd"], ref.invstd), "save_invstd"),
            ("running_mean / max", err_max(got["rm"], ref.rm[nup]), "running_mean"),
            ("running_var / max", err_max(got["rv"], ref.rv[nup]), "running_var"),
            ("dgamma per channel" + tag, err_channels(got["dgamma"], want_dg, bwd.dgamma, bwd.abs_dgamma), "dgamma"),
            ("dbeta per channel" + tag, err_channels(got["dbeta"], want_db, bwd.dbeta, bwd.abs_dbeta), "dbeta"),
            ("dgamma / max" + tag, float((got["dgamma"].double() - want_dg).abs().max() / bwd.dgamma.abs().max()), "dgamma_max"),
            ("dbeta / max" + tag, float((got["dbeta"].double() - want_db).abs().max() / bwd.dbeta.abs().max()), "dbeta_max")]


def train_oracle(ref, nup):
    """the fp32 CPU evaluation of a (grouped) train case: ATen's native_batch_norm (what F.batch_norm calls), + residual, F.relu, under
    autograd -> the dict train_figures takes"""
    inp = ref.inp
    x, gamma, beta = (t.clone().requires_grad_(True) for t in (inp.x, inp.gamma, inp.beta))
    r = inp.residual.clone().requires_grad_(True) if inp.residual is not None else None
    rm, rv = inp.rm.clone(), inp.rv.clone()
    Ng = x.shape[0] // ref.groups
    ys, sm, si = [], [], []
    for k in range(ref.groups):
        for _ in range(nup):
            out, m, i = torch.native_batch_norm(x[k * Ng:(k + 1) * Ng], gamma, beta, rm, rv, True, MOMENTUM, EPS)
        ys.append(out)
        sm.append(m.detach())
        si.append(i.detach())
    y = torch.cat(ys, 0)
    if r is not None:
        y = y + r
    if ref.relu:
        y = F.relu(y)
    y.backward(inp.dy)
    return dict(y=y.detach(), save_mean=torch.stack(sm, 0), save_invstd=torch.stack(si, 0), rm=rm, rv=rv, dx=x.grad,
                dres=r.grad if r is not None else None, dgamma=gamma.grad, dbeta=beta.grad)


# ------------------------------------------------------------------------------------------- fused stem tail
@functools.lru_cache(maxsize=None)
def pool_reference(name):
    """float64 forward of a fused-stem case.  A window is ambiguous where its two largest DISTINCT candidates differ by less than the
    allowance (the largest AMBIGUOUS * terms among its candidates).  Exact ties are not ambiguous: zeros after the ReLU take the
    first-maximum rule.  A candidate whose own gate is ambiguous counts with its signed pre-activation, so that it is distinct from
    the exact zeros next to it."""
    shape, groups, nup_case, route = POOL_CASES[name]
    inp = pool_inputs(name)
    ref = _train_ref(inp, True, groups)
    allow = AMBIGUOUS * _cat([o.terms for o in ref.fwd])
    cand = R.pool_candidates(torch.where(ref.amb, ref.pre, ref.y))
    pooled, idx = R.first_max(R.pool_candidates(ref.y))
    al = R.pool_candidates(allow).clamp(min=0).amax(0)                 # -inf (outside the map) -> 0
    top = cand.amax(0)
    second = torch.where(cand < top, cand, torch.full_like(cand, float("-inf"))).amax(0)
    ref.amb_win = (top - second) < al
    ref.pooled, ref.idx, ref.cand, ref.win_allow = pooled, idx, cand, al
    ref.win_share = float(ref.amb_win.double().mean())
    return ref


def byte_from_flat(flat, H, W):
    """F.max_pool2d(return_indices=True) flat input positions -> the argmax byte ky * 3 + kx of MaxPool2d(3, 2, 1)"""
    OH, OW = flat.shape[2:]
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    iy, ix = flat // W, flat % W
    return ((iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))).to(torch.uint8)


def pool_backward(ref, pooled_got, idx_got):
    """the reference backward with the device's argmax byte on the ambiguous windows and its ReLU decision (pooled > 0) on ambiguous
    argmax elements.  -> BnBwd, wrong argmax bytes (unambiguous windows that differ + ambiguous windows whose pick is not within the
    allowance of the maximum), wrong gates"""
    inp = ref.inp
    N, C, H, W = inp.x.shape
    picked = ref.cand.gather(0, idx_got.long().clamp(max=8).unsqueeze(0))[0]
    take = ref.amb_win & (idx_got <= 8) & (picked >= ref.cand.amax(0) - ref.win_allow)
    wrong_idx = int(((idx_got != ref.idx) & ~ref.amb_win).sum()) + int((ref.amb_win & ~take).sum())
    idx = torch.where(take, idx_got, ref.idx)
    pos = (R.argmax_position(idx, H, W) + (torch.arange(N * C).view(N, C, 1, 1) * (H * W))).reshape(-1)
    gate = (ref.pre > 0).reshape(-1).clone()
    dev_open = (pooled_got > 0).reshape(-1)
    amb_at = ref.amb.reshape(-1)[pos]
    wrong_gate = int(((dev_open != gate[pos]) & ~amb_at).sum())
    gate[pos[amb_at]] = dev_open[amb_at]
    gate = gate.view(N, C, H, W)
    Ng = N // ref.groups
    parts = []
    for g in range(ref.groups):
        sl = slice(g * Ng, (g + 1) * Ng)
        parts.append(R.bn_relu_pool_bwd(_d(inp.dy[sl]), idx[sl], _d(inp.x[sl]), ref.mean[g], ref.invstd[g], _d(inp.gamma), gate[sl]))
    return _sum_bwd(parts), wrong_idx, wrong_gate


def pool_figures(ref, got, nup, seeds=None):
    """got: pooled, idx (uint8), save_mean, save_invstd, rm, rv, dx, dgamma, dbeta -> figures, wrong argmax bytes, wrong gates"""
    bwd, wrong_idx, wrong_gate = pool_backward(ref, got["y"], got["idx"])
    want_dg, want_db = bwd.dgamma, bwd.dbeta
    if seeds is not None:
        want_dg, want_db = want_dg + seeds[0].double(), want_db + seeds[1].double()
    tag = " (add mode)" if seeds is not None else ""
    figs = [("pooled / max", err_max(got["y"], ref.pooled), "y"),
            ("dx / max", err_max(got["dx"], bwd.dx), "dx")] + _shared_figures(ref, got, nup, bwd, want_dg, want_db, tag)
    return figs, wrong_idx, wrong_gate


def pool_oracle(ref, nup):
    """the fp32 CPU evaluation of a fused-stem case: native_batch_norm, F.relu, F.max_pool2d(3, 2, 1) under autograd"""
    inp = ref.inp
    N, C, H, W = inp.x.shape
    x, gamma, beta = (t.clone().requires_grad_(True) for t in (inp.x, inp.gamma, inp.beta))
    rm, rv = inp.rm.clone(), inp.rv.clone()
    Ng = N // ref.groups
    ys, sm, si = [], [], []
    for k in range(ref.groups):
        for _ in range(nup):
            out, m, i = torch.native_batch_norm(x[k * Ng:(k + 1) * Ng], gamma, beta, rm, rv, True, MOMENTUM, EPS)
        ys.append(out)
        sm.append(m.detach())
        si.append(i.detach())
    y, flat = F.max_pool2d(F.relu(torch.cat(ys, 0)), 3, 2, 1, return_indices=True)
    y.backward(inp.dy)
    return dict(y=y.detach(), idx=byte_from_flat(flat, H, W), save_mean=torch.stack(sm, 0), save_invstd=torch.stack(si, 0), rm=rm, rv=rv,
                dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)


# ------------------------------------------------------------------------------------------- special statistics (derived bounds)
# Two tensors of SPECIAL_SHAPE; channel kinds in order.  offset: 1000 + 0.5 randn (mean / std = 2000); const: 0.5 (0.25 is exact in fp32
# and in double: the device variance must be exactly 0); inexact: 3.3f; zero; plain: randn * 2 + 0.5.
SPECIAL_TENSORS = {"A": ("offset", "const", "inexact", "plain"), "B": ("zero", "plain", "offset-", "const-")}
SPECIAL_VALUES = {"const": 0.5, "const-": -2.0, "inexact": 3.3, "zero": 0.0}


def special_inputs(name, seed=0):
    """no ReLU, no residual; gamma about 1 (gamma[0] = -0.7 kept, no zero scale: y of a constant channel has to come out of the
    arithmetic, not of sc == 0)"""
    N, C, H, W = SPECIAL_SHAPE
    g = _gen(seed + 90 + len(name) + ord(name[0]), SPECIAL_SHAPE)
    x = torch.empty(N, C, H, W)
    for c, kind in enumerate(SPECIAL_TENSORS[name]):
        if kind in SPECIAL_VALUES:
            x[:, c] = SPECIAL_VALUES[kind]
        elif kind.startswith("offset"):
            x[:, c] = (1000.0 if kind == "offset" else -1000.0) + 0.5 * torch.randn(N, H, W, generator=g)
        else:
            x[:, c] = torch.randn(N, H, W, generator=g) * 2 + 0.5
    gamma, beta, rm, rv = params(C, g)
    gamma[1] = 1.1
    dy = torch.randn(N, C, H, W, generator=g)
    return SimpleNamespace(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, dy=dy, residual=None)


@functools.lru_cache(maxsize=None)
def special_reference(name):
    ref = _train_ref(special_inputs(name), False)
    ref.bwd, _ = train_backward(ref, None)
    return ref


def hold(figures):
    """figures of derived_figures: print all -> the list of those over their bound"""
    for label, err, bound in figures:
        print(f"  {label:44s} {err:.3e}   bound {bound:.3e}")
    return [f"{label}: {err:.3e} > {bound:.3e}" for label, err, bound in figures if not err <= bound]


def var_bound(x_c, run=RUN):
    """|var_device - var_float64| of one channel (x_c: its elements, float64; run: fp32 terms a thread adds before it folds).

    The kernel forms var = E[x^2] - mean^2 from sums that each thread runs in fp32 over R = 32 terms before it folds them into a
    double (everything after that -- the block sum, the fold over the partials, the division and the subtraction -- is double, and
    adds about n 2^-53 E[x^2]).  With u = 2^-24:
      * each square is rounded once:                                   u     sum x^2
      * a run of R fp32 additions: (R - 1) roundings of a partial sum
        that is at most the run's sum of magnitudes:                   R u   sum x^2   and   R u sum |x|
      * the error of the mean, R u E|x|, enters var as 2 |mean| times
        itself, and |mean| E|x| <= E[x^2]:                             2 R u E[x^2]
    together (3 R + 1) u E[x^2].  Relative to the variance this is (3 R + 1) u (1 + mean^2 / var): a channel whose mean is 2000
    standard deviations gets no correct digit, which is the limit of the one-pass formula and not of this implementation.  (A thread
    that sees a single element adds nothing in fp32; R = 1 is granted there.)"""
    ex2 = float((x_c * x_c).mean())
    return (3 * run + 1) * U * ex2 + x_c.numel() * 2.0 ** -53 * ex2


def special_bounds(ref, c, run=RUN, bwd=None, gate=None):
    """per-element bounds on y and dx of channel c of a one-group case, propagated from var_bound through invstd.  bwd: the reference
    backward (default: ref.bwd); gate: the ReLU gate it used (dy below is dy times the gate).

    rho = 0.5 var_bound / (var + eps) + 4 u     relative error of invstd (first order in the variance error; its own rounding to
                                                 float and that of sc = invstd gamma are in the 4 u)
    dm  = R u E|x| + u |mean|                    error of the mean: the fp32 runs, and its rounding to float
    y  = fmaf(x, sc, fmaf(-mean, sc, beta)) (+ residual; the ReLU is 1-Lipschitz):
         |err| <= rho |pre - beta - residual| + (1 + rho) |sc| dm + 4 u (|x sc| + |mean sc| + |beta| + |residual|)
    dx = sc (dy - k1 - xhat k2), xhat = (x - mean) invstd, k1 = E[dy], k2 = E[dy xhat]:
         ex  = rho |xhat| + (1 + rho) invstd dm                        error of xhat (largest over the channel: exm)
         dk1 = R u E|dy|,   dk2 = E|dy| exm + R u E|dy xhat|           errors of the two means
         |err| <= rho |dx| + (1 + rho) |sc| (dk1 + ex |k2| + (|xhat| + ex) dk2) + 8 u |sc| (|dy| + |k1| + |xhat k2|)"""
    inp = ref.inp
    bwd = bwd if bwd is not None else ref.bwd
    x, dy = inp.x[:, c].double(), inp.dy[:, c].double()
    if gate is not None:
        dy = dy * gate[:, c].double()
    r = inp.residual[:, c].double() if inp.residual is not None else torch.zeros_like(x)
    mean, var, invstd = float(ref.mean[0, c]), float(ref.var[0, c]), float(ref.invstd[0, c])
    gamma, beta = float(inp.gamma[c]), float(inp.beta[c])
    sc = abs(invstd * gamma)
    vb = var_bound(x, run)
    rho = 0.5 * vb / (var + EPS32) + 4 * U
    dm = run * U * float(x.abs().mean()) + U * abs(mean)
    y_bound = (rho * (ref.pre[:, c] - beta - r).abs() + (1 + rho) * sc * dm
               + 4 * U * ((x * sc).abs() + abs(mean) * sc + abs(beta) + r.abs()))
    xhat = (x - mean) * invstd
    k1, k2 = float(dy.mean()), float((dy * xhat).mean())
    ex = rho * xhat.abs() + (1 + rho) * invstd * dm
    dk1 = run * U * float(dy.abs().mean())
    dk2 = float(dy.abs().mean()) * float(ex.max()) + run * U * float((dy * xhat).abs().mean())
    dx_bound = (rho * bwd.dx[:, c].abs() + (1 + rho) * sc * (dk1 + ex * abs(k2) + (xhat.abs() + ex) * dk2)
                + 8 * U * sc * (dy.abs() + abs(k1) + (xhat * k2).abs()))
    return SimpleNamespace(var_bound=vb, rho=rho, dm=dm, dk2=dk2, y_bound=y_bound, dx_bound=dx_bound)


def derived_figures(ref, got, nup, bwd, c, run=RUN):
    """channel c of a one-group case against the derived bounds -> [(label, error, bound)...].  var_dev is recovered from save_invstd
    as invstd^-2 - eps, which has 3 u (var + eps) of rounding of its own."""
    inp = ref.inp
    n = inp.x.numel() // inp.x.shape[1]
    b = special_bounds(ref, c, run, bwd, getattr(ref, "gate", None))
    mean, var = float(ref.mean[0, c]), float(ref.var[0, c])
    sm, si = float(got["save_mean"][0, c]), float(got["save_invstd"][0, c])
    tiny = 1e-300

    def worst(g, r, bound):
        return float(((g.double() - r).abs() / bound.clamp(min=tiny)).max())

    return [(f"[{c}] |var_dev - var_64|", abs(si ** -2.0 - EPS32 - var), b.var_bound + 3 * U * (var + EPS32)),
            (f"[{c}] |save_mean - mean_64|", abs(sm - mean), b.dm),
            (f"[{c}] max |y - y_64| / bound", worst(got["y"][:, c], ref.y[:, c], b.y_bound), 1.0),
            (f"[{c}] max |dx - dx_64| / bound", worst(got["dx"][:, c], bwd.dx[:, c], b.dx_bound), 1.0),
            (f"[{c}] |dgamma - dgamma_64|", abs(float(got["dgamma"][c]) - float(bwd.dgamma[c])), n * b.dk2 + U * abs(float(bwd.dgamma[c]))),
            (f"[{c}] |running_mean - ref|", abs(float(got["rm"][c]) - float(ref.rm[nup][c])),
             nup * (MOMENTUM * b.dm + 4 * U * (abs(float(inp.rm[c])) + MOMENTUM * abs(mean)))),
            (f"[{c}] |running_var - ref|", abs(float(got["rv"][c]) - float(ref.rv[nup][c])),
             nup * (MOMENTUM * b.var_bound * unbiased_factor(n) + 4 * U * (abs(float(inp.rv[c])) + MOMENTUM * var * unbiased_factor(n))))]


def fmaf32(a, b, c):
    """fmaf on fp32 values held in float64 tensors: the product of two 24-bit significands and the sum with a third value whose exponent
    is within 2^5 of it are exact in double, so one rounding to float32 is the fused result"""
    return (a.double() * b.double() + c.double()).float()


# ------------------------------------------------------------------------------------------- channel sum
def channel_sum_inputs(shape, seed=0):
    g = _gen(seed + 70, shape)
    N, C, H, W = shape
    x = torch.randn(N, C, H, W, generator=g) * 2 + 0.5
    out0 = torch.randn(C, generator=g) * 50
    return x, out0


def channel_sum_bound(x, out0):
    """per channel |error| of jp_channel_sum against the float64 sum (itself within n 2^-53 sum |x| of the exact one, which is added).

    Each workgroup's threads add runs of 32 terms in fp32 -- 31 roundings of a partial sum of at most the run's sum |x| -- fold the
    runs in double and round the workgroup's sum to float once: at most 32 u sum |x| over the channel (33 u is granted).  The S
    partials then meet in fp32, in a fixed order behind the scratch or in atomics in any order: S additions, each rounding a value
    of at most |out0| + sum |partial|.  The last addition's rounding is u |result|:
        (33 u) sum |x|  +  u |out0 + sum|  +  S u (sum |partial| + |out0|)            (out0 = 0 without `accumulate`)"""
    N, C, H, W = x.shape
    CH, chunk = chunking(N, C, H * W)
    xd = x.double().reshape(N, C, H * W)
    sum_abs = xd.abs().sum((0, 2))
    parts = torch.stack([xd[:, :, k * chunk:(k + 1) * chunk].sum(2) for k in range(CH)], 2)          # (N, C, CH)
    part_abs = parts.abs().sum((0, 2))
    total = xd.sum((0, 2))
    o = out0.double().abs() if out0 is not None else torch.zeros(C, dtype=F64)
    want = total + (out0.double() if out0 is not None else 0)
    S = N * CH
    return want, 33 * U * sum_abs + U * want.abs() + S * U * (part_abs + o) + N * H * W * 2.0 ** -53 * sum_abs


# ------------------------------------------------------------------------------------------- eval mode
def eval_inputs(shape, seed=0):
    """running statistics positive and seeded; channel 0 has running_var = 0 (invstd = 1 / sqrt(eps))"""
    inp = train_inputs(shape, True, seed + 30)
    inp.rv[0] = 0.0
    return inp


def eval_reference(inp, relu, res):
    """-> y, bound per element.  The kernel evaluates sc = gamma / sqrtf(rv + eps) (three roundings), sh = fmaf(-rm, sc, beta) (one),
    fmaf(x, sc, sh) (one) and the residual add (one): no term passes through more than six roundings, so
    |err| <= 8 u (|x sc| + |rm sc| + |beta| + |residual|)"""
    x, gamma, beta, rm, rv = (_d(t) for t in (inp.x, inp.gamma, inp.beta, inp.rm, inp.rv))
    r = _d(inp.residual) if res else None
    y = R.bn_eval_fwd(x, gamma, beta, rm, rv, r, relu, EPS32)
    sc = (gamma / torch.sqrt(rv + EPS32)).view(1, -1, 1, 1)
    mag = (x * sc).abs() + (rm.view(1, -1, 1, 1) * sc).abs() + beta.abs().view(1, -1, 1, 1) + (r.abs() if res else 0)
    return y, 8 * U * mag


def unbiased_factor(count):
    return count / (count - 1) if count > 1 else 1.0


assert math.isclose(U, 5.960464477539063e-08)
