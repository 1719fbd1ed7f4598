"""Cases, seeded inputs, launch mirrors, ambiguity masks, error metrics, derived bounds and bars shared by tests/test_dense_ref_cpu.py
(which checks every condition on the float64 reference without a GPU) and tests/test_dense_f64_gpu.py (which runs the kernels of
jperceiver_amd/csrc/small.hip and the three kernels of pointwise.hip that only the BEV-layout head uses).  Everything here is CPU-only
torch; nothing imports the HIP library or the oracle."""
import contextlib
import functools
import math
import zlib
from types import SimpleNamespace

import torch

from tests import dense_ref as R

F64 = torch.float64
U = 2.0 ** -24                # unit roundoff of fp32
MASK_CAP = 0.005              # at most this share of a case's gates / columns may take the device's decision
NAN = float("nan")
SENTINEL = 12345.6787109375   # what the padding columns of C hold (exact in fp32)

# ------------------------------------------------------------------------------------------- launch mirrors
# The constants of small.hip / pointwise.hip that decide which path a shape takes, as they stand in the source
# (tests/test_dense_ref_cpu.py finds every string verbatim, so a changed constant fails there), next to their Python mirrors.
SMALL_HIP = "jperceiver_amd/csrc/small.hip"
POINTWISE_HIP = "jperceiver_amd/csrc/pointwise.hip"
TS = 16                       # GEMM tile: TS x TS outputs per workgroup, TS values of k per trip
CS_COLS, CS_LANES = 64, 16    # colsum_kernel: 64 columns x 16 row lanes per workgroup
WG_SMALL, WG = 64, 256        # workgroup sizes of the index kernels
BIAS_BLOCK_CAP = 65535        # jp_bias_act_rows launches at most this many workgroups of 256; beyond, threads stride
TPB, POINTWISE_BLOCK_CAP = 256, 1 << 20
SOURCE_LINES = {
    SMALL_HIP: {          # key -> (line, how often it stands in the file)
        "ts": ("constexpr int TS = 16;", 1),
        "gemm_grid": ("dim3 grid(jp_cdiv(N, TS), jp_cdiv(M, TS), batch);", 1),
        "gemm_k": ("for (int k0 = 0; k0 < K; k0 += TS) {", 1),
        "gemm_fma": ("for (int k = 0; k < TS; ++k) acc = fmaf(As[ty][k], Bs[k][tx], acc);", 1),
        "gemm_epilogue": ("*c = alpha * acc + (beta != 0.f ? beta * *c : 0.f);", 1),
        "colsum_part": ("__shared__ float part[16][65];", 1),
        "colsum_lanes": ("const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;", 1),
        "colsum_loop": ("for (int r = ty; r < M; r += 16) s += x[(size_t)r * N + c];", 1),
        "colsum_fold": ("for (int k = 1; k < 16; ++k) s += part[k][tx];", 1),
        "colsum_launch": ("hipLaunchKernelGGL(colsum_kernel, dim3(jp_cdiv(N, 64)), dim3(1024), 0, st, x, out, M, N, accumulate);", 1),
        "colmax_launch": ("hipLaunchKernelGGL(colmax_kernel, dim3(jp_cdiv(B * Cn, 64)), dim3(64), 0, st, E, val, arg, B, R, Cn);", 1),
        "colmax_bwd_launch": ("dim3(jp_cdiv((long)B * R * Cn, 256)), dim3(256)", 1),
        "gather_launch": ("dim3(jp_cdiv((long)B * C * Nn, 256)), dim3(256)", 2),
        "mean_launch": ("dim3(jp_cdiv(BC, 64)), dim3(64)", 1),
        "total_256_launch": ("dim3(jp_cdiv(total, 256)), dim3(256)", 3),          # spatial_mean_bwd, bcast_matmul fwd, its bwd_v
        "bwd_a_launch": ("dim3(jp_cdiv(total, 64)), dim3(64)", 1),
        "bias_launch": ("dim3((int)std::min<long>((total + 255) / 256, 65535)), dim3(256)", 1),
        "bias_loop": ("for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)", 1),
    },
    POINTWISE_HIP: {
        "tpb": ("constexpr int TPB = 256;", 1),
        "blocks_for": ("inline int blocks_for(long n) { return (int)std::min<long>((n + TPB - 1) / TPB, 1 << 20); }", 1),
        "softmax_max": ("const float ea = __expf(a - m), eb = __expf(b - m);", 1),
    },
}


def round_up_1sig(v):
    """v rounded up to one significant digit (the rule of tests/photometric_cases.py, restated: importing that module would import
    the oracle, which the GPU file must not depend on)"""
    e = math.floor(math.log10(v))
    m = math.ceil(v / 10 ** e - 1e-9)
    return float(f"{m}e{e}") if m < 10 else float(f"1e{e + 1}")


def cdiv(a, b):
    return -(-a // b)


def gemm_launch(M, N, K):
    """what gemm_sb_kernel does with an M x N x K product: tiles along the rows (blockIdx.y), the columns (blockIdx.x), trips of the
    k0 loop, and how many rows / columns / k of the last tile or trip lie outside the extents"""
    return SimpleNamespace(row_tiles=cdiv(M, TS), col_tiles=cdiv(N, TS), k_trips=cdiv(K, TS), row_short=cdiv(M, TS) * TS - M,
                           col_short=cdiv(N, TS) * TS - N, k_short=cdiv(K, TS) * TS - K)


def colsum_launch(M, N):
    """workgroups, columns of the last one that lie outside N, trips of row lane 0 through `for (r = ty; r < M; r += 16)`, and how
    many of the 16 row lanes take one trip fewer than lane 0"""
    trips = cdiv(M, CS_LANES)
    return SimpleNamespace(blocks=cdiv(N, CS_COLS), col_short=cdiv(N, CS_COLS) * CS_COLS - N, trips=trips,
                           lanes_short=trips * CS_LANES - M)


def index_launch(total, wg):
    """a one-thread-per-element kernel: workgroups and idle threads of the last one"""
    return SimpleNamespace(blocks=cdiv(total, wg), idle=cdiv(total, wg) * wg - total)


def bias_launch(total):
    blocks = min(cdiv(total, WG), BIAS_BLOCK_CAP)
    return SimpleNamespace(blocks=blocks, strides=total > blocks * WG, tail=total - blocks * WG)


# ------------------------------------------------------------------------------------------- inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(str(name).encode()) % (2 ** 31))


def randn(name, *shape, scale=1.0):
    return torch.randn(*shape, generator=_gen(name)) * scale


def acc_seed(grad, name):
    """the buffer an add-mode run adds onto: -(0.25 .. 0.75) of the gradient per element (a dropped add, or one applied twice, moves
    the result by that share; the sum stays below the gradient, so its own fp32 rounding stays below the gradient's)"""
    return (-grad.double() * (0.25 + 0.5 * torch.rand(grad.shape, generator=_gen(name), dtype=F64))).float()


def err_terms(got, want, mag):
    """per element |got - want| / sum |terms|: the largest (an element without terms is exactly 0; anything else there is infinite)"""
    e = (got.detach().double() - want).abs()
    return float((e / mag.clamp(min=1e-300)).max()) if e.numel() else 0.0


def bits(t):
    """fp32 tensor -> its bit patterns (NaN compares equal to the same NaN)"""
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------- GEMM
# gemm_sb_kernel: every thread owns one C element.  acc = fmaf(a, b, acc) over K terms (the zero padding of the last trip adds
# nothing): K roundings, each of a partial sum of at most sum |a b|.  alpha * acc rounds once, beta * c rounds once (u |beta c|), their
# sum rounds once:  |err| <= (K + 3) u (|alpha| sum |a b| + |beta c|)  to first order.
def gemm_bound(K):
    return (K + 3) * U


def _g(M, N, K, **kw):
    d = dict(M=M, N=N, K=K, batch=1, tA=0, tB=0, alpha=1.0, beta=0.0, pad=(0, 0, 0), shareA=False, claim={})
    d.update(kw)
    return d


# name -> case; `claim`: what gemm_launch must report (tests/test_dense_ref_cpu.py asserts every entry)
GEMM_CASES = {
    "forward form": _g(33, 17, 19, tB=1, claim=dict(row_tiles=3, col_tiles=2, k_trips=2, row_short=15, col_short=15, k_short=13)),
    "weight-gradient form": _g(17, 19, 33, tA=1, beta=1.0, claim=dict(row_tiles=2, col_tiles=2, k_trips=3, k_short=15)),
    "input-gradient form, write": _g(33, 19, 17, claim=dict(row_tiles=3, col_tiles=2, k_trips=2, k_short=15)),      # beta 0 onto NaN
    "input-gradient form, add": _g(33, 19, 17, beta=1.0, claim=dict(row_tiles=3, col_tiles=2, k_trips=2)),
    "both transposes": _g(33, 17, 19, tA=1, tB=1, claim=dict(row_tiles=3, col_tiles=2, k_trips=2)),
    "exact K chunk": _g(5, 7, 16, claim=dict(k_trips=1, k_short=0)),
    "K chunk plus one": _g(5, 7, 17, claim=dict(k_trips=2, k_short=15)),
    "minimal": _g(1, 1, 1, claim=dict(row_tiles=1, col_tiles=1, k_trips=1, row_short=15, col_short=15, k_short=15)),
    "scaled": _g(33, 17, 19, tB=1, alpha=-0.5, beta=0.25, claim=dict(row_tiles=3)),
    "batched": _g(37, 37, 5, batch=3, tA=1, claim=dict(row_tiles=3, col_tiles=3, k_trips=1, row_short=11, k_short=11)),
    "batched adjoint dk": _g(5, 37, 37, batch=3, tB=1, beta=1.0, claim=dict(row_tiles=1, col_tiles=3, k_trips=3, k_short=11)),
    "batched adjoint dq": _g(5, 37, 37, batch=3, beta=1.0, claim=dict(row_tiles=1, col_tiles=3, k_trips=3, k_short=11)),
    "shared operand": _g(9, 21, 18, batch=3, shareA=True, claim=dict(col_tiles=2, k_trips=2)),
    "padded leading dimensions": _g(33, 17, 19, pad=(3, 5, 2), beta=1.0, claim=dict(row_tiles=3, col_tiles=2, k_trips=2)),
    # the step's own shapes (B = 8: M = B * 128 rows of 64 features; k, q (8, 16, 64))
    "step linear forward": _g(1024, 64, 64, tB=1, claim=dict(row_tiles=64, col_tiles=4, k_trips=4, row_short=0, k_short=0)),
    "step linear dW": _g(64, 64, 1024, tA=1, beta=1.0, claim=dict(k_trips=64)),
    "step linear dx": _g(1024, 64, 64, claim=dict(row_tiles=64)),
    "step energy": _g(64, 64, 16, batch=8, tA=1, claim=dict(row_tiles=4, col_tiles=4, k_trips=1, k_short=0)),
    "step energy dk": _g(16, 64, 64, batch=8, tB=1, beta=1.0, claim=dict(row_tiles=1, k_trips=4)),
    "step energy dq": _g(16, 64, 64, batch=8, beta=1.0, claim=dict(row_tiles=1, k_trips=4)),
}
GEMM_BETA1 = tuple(n for n, c in GEMM_CASES.items() if c["beta"] == 1.0)


def gemm_args(c):
    """-> (lda, ldb, ldc, sA, sB, sC, rows of A, rows of B): A is stored (K x M) when transposed, else (M x K); B (N x K) when
    transposed, else (K x N); the leading dimensions are the stored row lengths plus the case's padding"""
    M, N, K = c["M"], c["N"], c["K"]
    rowsA, lda = (K, M) if c["tA"] else (M, K)
    rowsB, ldb = (N, K) if c["tB"] else (K, N)
    lda, ldb, ldc = lda + c["pad"][0], ldb + c["pad"][1], N + c["pad"][2]
    return lda, ldb, ldc, (0 if c["shareA"] else rowsA * lda), rowsB * ldb, M * ldc, rowsA, rowsB


@functools.lru_cache(maxsize=None)
def gemm_case(name):
    """-> SimpleNamespace(A, B, C flat fp32 buffers, abi: the argument tuple after the three pointers, ref: the float64 result (flat),
    mag, ic: flat indices of the written elements, padmask: flat mask of C's padding columns).  The padding of A and B is NaN (a kernel
    that reads it shows), that of C the sentinel; beta == 0 cases start from a NaN-filled C"""
    c = GEMM_CASES[name]
    M, N, K, batch = c["M"], c["N"], c["K"], c["batch"]
    lda, ldb, ldc, sA, sB, sC, rowsA, rowsB = gemm_args(c)
    g = _gen("gemm " + name)

    def operand(nb, rows, ld, cols):
        t = torch.full((nb, rows, ld), NAN)
        t[:, :, :cols] = torch.randn(nb, rows, cols, generator=g)
        return t.reshape(-1)

    A = operand(1 if c["shareA"] else batch, rowsA, lda, lda - c["pad"][0])
    B = operand(batch, rowsB, ldb, ldb - c["pad"][1])
    C = torch.full((batch, M, ldc), SENTINEL)
    C[:, :, :N] = torch.randn(batch, M, N, generator=g) * 3 if c["beta"] != 0 else NAN
    padmask = torch.zeros(batch, M, ldc, dtype=torch.bool)
    padmask[:, :, N:] = True
    C = C.reshape(-1)
    abi = (M, N, K, lda, ldb, ldc, sA, sB, sC, batch, c["tA"], c["tB"], c["alpha"], c["beta"])
    ref, mag = R.gemm(A, B, C, *abi)
    return SimpleNamespace(case=c, A=A, B=B, C=C, abi=abi, ref=ref, mag=mag, ic=R.gemm_c_index(M, N, ldc, sC, batch),
                           padmask=padmask.reshape(-1))


def gemm_figure(g, got):
    return err_terms(got[g.ic], g.ref[g.ic], g.mag)


def gemm_fp32(g):
    """ATen's fp32 baddbmm on the same operands -> flat C"""
    c = g.case
    a, b = R.gemm_operands(g.A, g.B, *g.abi[:5], *g.abi[6:8], *g.abi[9:12])
    old = g.C[g.ic]
    if c["beta"] == 0:
        old = torch.zeros_like(old)
    out = g.C.clone()
    out[g.ic] = torch.baddbmm(old, a.contiguous(), b.contiguous(), beta=c["beta"], alpha=c["alpha"])
    return out


# ------------------------------------------------------------------------------------------- bias + activation
# bias_act_rows_kernel: y + bias rounds once; ReLU keeps it; the leaky slope multiplies once more (act 2: 2 u); the sigmoid is held
# to an absolute bar.  fp32 addition is correctly rounded, so the sign of fl(y + b) is that of y + b: no gate of this kernel alone is
# ambiguous.
BIAS_CASES = {            # name -> (M, N, act, bias)
    "33x17 act0": (33, 17, 0, True), "33x17 act1": (33, 17, 1, True), "33x17 act2": (33, 17, 2, True), "33x17 act3": (33, 17, 3, True),
    "33x17 no bias": (33, 17, 1, False),
    "loss-vector form": (21, 1, 0, True),
    "step 1024x64": (1024, 64, 1, True),
}
BIAS_BIG_TOTAL = BIAS_BLOCK_CAP * WG + 77          # one case just above the block cap: threads stride over a ragged tail


def bias_bound(act):
    return (2 if act == R.ACT_LEAKY else 1) * U


def _small_factor(n):
    return next((d for d in range(2, 2000) if n % d == 0), 1)


BIAS_BIG_N = _small_factor(BIAS_BIG_TOTAL)         # the row length of the big case: its smallest factor (1 if it has none below 2000)


@functools.lru_cache(maxsize=None)
def bias_case(name):
    M, N, act, has_bias = BIAS_CASES[name]
    y = randn("bias y " + name, M, N)
    b = randn("bias b " + name, N) if has_bias else None
    want, pre, mag = R.bias_act_rows(y, b, act)
    return SimpleNamespace(M=M, N=N, act=act, y=y, bias=b, want=want, pre=pre, mag=mag)


def bias_big_case():
    """(not cached: 16.8 M elements).  The reference is one float64 add"""
    N = BIAS_BIG_N
    M = BIAS_BIG_TOTAL // N
    y = randn("bias big", M, N)
    b = randn("bias big b", N)
    return SimpleNamespace(M=M, N=N, act=0, y=y, bias=b, want=y.double() + b.double(), mag=y.double().abs() + b.double().abs())


def bias_fp32(c):
    pre = c.y + (c.bias if c.bias is not None else 0)
    return {0: lambda t: t, 1: torch.relu, 2: lambda t: torch.nn.functional.leaky_relu(t, 0.01), 3: torch.sigmoid}[c.act](pre)


# ------------------------------------------------------------------------------------------- column sum
# colsum_kernel: row lane ty adds rows ty, ty + 16, ... serially, starting from 0: at most ceil(M / 16) - 1 roundings; lane 0 then
# adds the 15 other lanes' partials (15 roundings) and, in add mode, the old value (1 rounding).  Every rounding is of a partial sum
# of at most sum |terms|:  |err| <= (ceil(M / 16) + 16) u sum |terms|   (the issue's figure; the count above is one below it).
COLSUM_CASES = {          # (M, N) -> what colsum_launch must report
    (1, 1): dict(blocks=1, trips=1, col_short=63, lanes_short=15),
    (15, 64): dict(blocks=1, trips=1, col_short=0, lanes_short=1),
    (16, 65): dict(blocks=2, trips=1, col_short=63, lanes_short=0),
    (17, 63): dict(blocks=1, trips=2, col_short=1, lanes_short=15),       # the second trip of the row loop: lane 0 alone
    (100, 130): dict(blocks=3, trips=7, col_short=62, lanes_short=12),
    (22, 1): dict(blocks=1, trips=2, col_short=63),                       # N = 1: the loss-vector sum
    (1024, 64): dict(blocks=1, trips=64, lanes_short=0),                  # the step's bias gradient: M = B * 128
}


def colsum_bound(M):
    return (cdiv(M, CS_LANES) + 16) * U


@functools.lru_cache(maxsize=None)
def colsum_case(shape):
    M, N = shape
    x = randn(f"colsum {shape}", M, N)
    out0 = randn(f"colsum seed {shape}", N, scale=5.0)
    return SimpleNamespace(x=x, out0=out0, write=R.colsum(x), add=R.colsum(x, out0))


# ------------------------------------------------------------------------------------------- column max
COLMAX_SHAPES = {         # (B, R, Cn) -> workgroups of 64 / idle threads of colmax, workgroups of 256 / idle threads of colmax_bwd
    (1, 1, 1): dict(fwd=(1, 63), bwd=(1, 255)),
    (2, 37, 65): dict(fwd=(3, 62), bwd=(19, 54)),
    (3, 64, 64): dict(fwd=(3, 0), bwd=(48, 0)),
    (8, 64, 64): dict(fwd=(8, 0), bwd=(128, 0)),                          # the step's energy
}
COLMAX_DATA = ("normal", "ties", "constant column", "-inf column", "+inf", "nan row 0", "nan middle", "nan last")


def colmax_input(shape, kind):
    """the energies are given directly, so every decision is exact and needs no mask"""
    B, Rr, Cn = shape
    E = randn(f"colmax {shape} {kind}", B, Rr, Cn)
    if kind == "ties":
        E = torch.round(E * 2) / 2                       # multiples of 0.5: many exact ties; the first index must win
    elif kind == "constant column":
        E[:, :, 0] = 0.75
        E[:, :, Cn // 2] = -2.0
    elif kind == "-inf column":
        E[:, :, Cn // 2] = float("-inf")
    elif kind == "+inf":
        E[:, Rr // 2, :] = float("inf")
        E[:, Rr - 1, 0] = float("inf")                   # a second +inf further down column 0: the first wins
    elif kind.startswith("nan"):
        row = {"nan row 0": 0, "nan middle": Rr // 2, "nan last": Rr - 1}[kind]
        E[:, row, :] = NAN
    return E


def colmax_nan_row(shape, kind):
    return {"nan row 0": 0, "nan middle": shape[1] // 2, "nan last": shape[1] - 1}[kind]


# ------------------------------------------------------------------------------------------- gather
# gather_cols_bwd_kernel: one thread per dV element adds the dT[j] with arg[j] == i serially from 0: hits - 1 roundings of partial
# sums of at most sum |terms|:  |err| <= hits u sum |terms|; an element that no index names is exactly 0.
GATHER_SHAPES = {         # (B, C, Nn) -> workgroups of 256, idle threads
    (3, 5, 37): (3, 213),
    (2, 3, 300): (8, 248),
    (8, 128, 64): (256, 0),                                               # the step's feature selection
}
GATHER_INDEX = ("repeats", "all equal", "permutation")
ROT_N = 256               # net.rot270 on a (2, 1, 256, 256) label: C = 1, Nn = 65536


def gather_index(shape, kind):
    """(B, Nn) int64, a different row per batch"""
    B, _, Nn = shape
    g = _gen(f"gather idx {shape} {kind}")
    if kind == "repeats":
        return torch.randint(0, Nn, (B, Nn), generator=g)
    if kind == "all equal":
        return (torch.arange(B).view(B, 1) * 7 % Nn).expand(B, Nn).contiguous()
    return torch.stack([torch.randperm(Nn, generator=g) for _ in range(B)])


# ------------------------------------------------------------------------------------------- spatial mean
# spatial_mean_kernel: a serial sum of HW terms from 0 (HW - 1 roundings), times scale, divided by HW (one rounding each; both exact
# at HW = 1 with scale a power of two): (HW + 1) u sum |terms| to first order, HW u at HW = 1.  The issue holds it to HW u, the
# stricter figure; that is what is asserted.  spatial_mean_bwd_kernel: dout * scale / HW, two roundings: 2 u |value|.
MEAN_CASES = {            # (BC, HW) -> workgroups of 64 of the forward, workgroups of 256 of the adjoint
    (1, 1): (1, 1), (65, 7): (2, 2), (48, 120): (1, 23), (96, 120): (2, 45),          # (96, 120): the pose decoder at B = 8, 2 x 6 frames
}
MEAN_SCALE = 0.01          # what the pose decoder passes ...
MEAN_SCALE32 = float(torch.tensor(MEAN_SCALE, dtype=torch.float32))          # ... and what the kernels see of it: the references use this one


def mean_bound(HW):
    return HW * U


MEAN_BWD_BOUND = 2 * U


# ------------------------------------------------------------------------------------------- per-channel n x n product
# bcast_matmul_fwd_kernel: s += a[k] * v[k] over n terms (fused or not: every product's rounding is u of that product, every
# addition's u of a partial sum; n u sum |terms| covers both).  bwd_v: n terms.  bwd_a: C n terms.
BCAST_CASES = {           # (B, C, n) -> workgroups of 256 of fwd / bwd_v, workgroups of 64 of bwd_a
    (1, 1, 1): (1, 1), (2, 3, 5): (1, 1), (1, 2, 17): (3, 5), (2, 20, 6): (6, 2), (8, 128, 8): (256, 8),
}


# ------------------------------------------------------------------------------------------- channel-broadcast product, softmax
# mul_bcast_c_kernel is one fp32 product: bit-equal to the fp32 product.  mul_bcast_c_bwd_s_kernel: g += dout * a over C terms: C u.
MUL_CASES = {(1, 1, 1): 1, (3, 5, 37): 3, (2, 3, 300): 8, (8, 128, 64): 256}          # (B, C, HW) -> workgroups of the forward
SOFTMAX_CASES = ((1, 1), (3, 37), (2, 300), (2, 4096))
SOFTMAX_DIFFS = (0.0, 1e-3, -1e-3, 20.0, -20.0, 90.0, -90.0, 200.0, -200.0)
SOFTMAX_SUM_BOUND = 2 * U


def softmax_input(shape):
    """(N, 2, HW) finite logits; the listed differences x1 - x0 stand in every case (around offsets up to +-100, so that a kernel
    without the max subtraction overflows); the (1, 1) case takes them one per repeat"""
    N, HW = shape
    x = randn(f"softmax {shape}", N, 2, HW, scale=3.0)
    flat = x.permute(0, 2, 1).reshape(-1, 2)
    if flat.shape[0] >= len(SOFTMAX_DIFFS):
        for i, d in enumerate(SOFTMAX_DIFFS):
            base = (-100.0, 0.0, 100.0)[i % 3]
            flat[i, 0], flat[i, 1] = base, base + d
        x = flat.reshape(N, HW, 2).permute(0, 2, 1).contiguous()
    return x


def softmax_single_inputs():
    return [torch.tensor([[[100.0], [100.0 + d]]]) for d in SOFTMAX_DIFFS]


# ------------------------------------------------------------------------------------------- ambiguous decisions
def gate_allowance(K, terms):
    """a ReLU gate whose float64 pre-activation lies within this of zero takes the device's decision"""
    return (K + 2) * U * terms


def replay_gate(pre, amb, dev):
    """-> (the gate to use, number of unambiguous gates where the device differs)"""
    own = pre > 0
    return torch.where(amb, dev, own), int(((dev != own) & ~amb).sum())


def column_ambiguity(E, terms, K):
    """E, terms (B, R, Cn) float64 -> SimpleNamespace(idx: first maximum, second: the runner-up's row, amb (B, Cn): the two largest
    energies lie within the larger of their two allowances (K + 2) u sum |terms| of each other, gap, allow)"""
    B, Rr, Cn = E.shape
    val, idx = R.colmax(E)
    if Rr == 1:
        z = torch.zeros(B, Cn, dtype=torch.bool)
        return SimpleNamespace(idx=idx, second=idx, amb=z, gap=torch.full((B, Cn), float("inf"), dtype=F64), allow=torch.zeros(B, Cn, dtype=F64))
    rest = E.scatter(1, idx.unsqueeze(1), float("-inf"))
    val2, idx2 = R.colmax(rest)
    allow = (K + 2) * U * torch.maximum(R.select_rows(terms, idx), R.select_rows(terms, idx2))
    gap = val - val2
    return SimpleNamespace(idx=idx, second=idx2, amb=gap <= allow, gap=gap, allow=allow)


def replay_index(amb, dev):
    """-> (the index to use, number of columns where the device's index is wrong: an unambiguous column that differs, or an ambiguous
    one whose index names neither of the two largest)"""
    ok = torch.where(amb.amb, (dev == amb.idx) | (dev == amb.second), dev == amb.idx)
    return torch.where(ok, dev, amb.idx), int((~ok).sum())


AMBIGUITY_SHAPES = ((8, 16, 64), (2, 16, 64), (2, 16, 1024))          # standard-normal k, q: the shares are recorded by the CPU test


def energy_ambiguity(k, q):
    k, q = k.double(), q.double()
    return column_ambiguity(R.energy(k, q), R.energy_terms(k, q), k.shape[1])


# ------------------------------------------------------------------------------------------- chain 1: the CVP MLP
MLP_SHAPE = (2, 128, 8, 8)           # TransformModule._fwd at occ_map_size // 32 = 8: M = 256 rows of 64 features, ReLU twice
MLP_KEYS = ("y", "dx", "dw1", "db1", "dw2", "db2")
MLP_LEAVES = ("x", "w1", "b1", "w2", "b2")


@functools.lru_cache(maxsize=None)
def mlp_reference():
    B, C, H, W = MLP_SHAPE
    F_ = H * W
    inp = SimpleNamespace(x=randn("mlp x", B, C, H, W), w1=randn("mlp w1", F_, F_, scale=0.15), b1=randn("mlp b1", F_, scale=0.1),
                          w2=randn("mlp w2", F_, F_, scale=0.15), b2=randn("mlp b2", F_, scale=0.1), dy=randn("mlp dy", B, C, H, W))
    x, w1, b1, w2, b2 = (getattr(inp, n).double() for n in MLP_LEAVES)
    y, pre, h = R.mlp_chain(x, w1, b1, w2, b2)
    terms = [R.linear_terms(x.reshape(B, C, F_), w1, b1), R.linear_terms(h, w2, b2)]
    amb = [p.abs() <= gate_allowance(F_, t) for p, t in zip(pre, terms)]
    share = [float(a.double().mean()) for a in amb]
    return SimpleNamespace(inp=inp, pre=pre, amb=amb, share=share)


def _grads(out, dy, leaves):
    out.backward(dy)
    return [t.grad for t in leaves]


def mlp_evaluate(ref, gates, dtype=F64):
    """the chain under autograd with the given gates, in float64 (the reference) or float32 (ATen's linear: the fp32 evaluation)
    -> dict over MLP_KEYS"""
    inp = ref.inp
    L = [getattr(inp, n).to(dtype).clone().requires_grad_(True) for n in MLP_LEAVES]
    if dtype == F64:
        y = R.mlp_chain(*L, gates=gates)[0]
    else:
        B, C, H, W = inp.x.shape
        h = torch.nn.functional.linear(L[0].reshape(B, C, H * W), L[1], L[2])
        h = torch.where(gates[0], h, torch.zeros((), dtype=dtype))
        y = torch.nn.functional.linear(h, L[3], L[4])
        y = torch.where(gates[1], y, torch.zeros((), dtype=dtype)).reshape(B, C, H, W)
    g = _grads(y, inp.dy.to(dtype), L)
    return dict(zip(MLP_KEYS, [y.detach()] + g))


def mlp_replay(ref, dev_gates):
    """-> (the float64 result with the device's decision on the ambiguous gates, wrong gates per layer, the gates used)"""
    gates, wrong = zip(*[replay_gate(p, a, d) for p, a, d in zip(ref.pre, ref.amb, dev_gates)])
    return mlp_evaluate(ref, list(gates)), list(wrong), list(gates)


# ------------------------------------------------------------------------------------------- chain 2: the CCT algebra
CCT_DIMS = (2, 16, 128, 8)           # B, C // 8, C, n: k, q (2, 16, 64), v (2, 128, 64), residual and depth values (2, 128, 8, 8)
CCT_LEAVES = ("k", "q", "v", "res", "kd", "qd", "vd")
CCT_KEYS = ("out", "S", "attn", "dk", "dq", "dv", "dres", "dkd", "dqd", "dvd")


@functools.lru_cache(maxsize=None)
def cct_reference():
    B, Ck, C, n = CCT_DIMS
    N = n * n
    inp = SimpleNamespace(k=randn("cct k", B, Ck, N), q=randn("cct q", B, Ck, N), v=randn("cct v", B, C, N),
                          res=randn("cct res", B, C, n, n), kd=randn("cct kd", B, Ck, N), qd=randn("cct qd", B, Ck, N),
                          vd=randn("cct vd", B, C, n, n), go=randn("cct go", B, C, n, n))
    amb = [energy_ambiguity(inp.k, inp.q), energy_ambiguity(inp.kd, inp.qd)]
    return SimpleNamespace(inp=inp, amb=amb, share=[float(a.amb.double().mean()) for a in amb])


def cct_evaluate(ref, idx, dtype=F64):
    """the chain under autograd with the given indices, in float64 (the reference) or float32 (ATen's bmm / matmul) -> dict over
    CCT_KEYS"""
    inp = ref.inp
    B, Ck, C, n = CCT_DIMS
    L = [getattr(inp, nm).to(dtype).clone().requires_grad_(True) for nm in CCT_LEAVES]
    if dtype == F64:
        out, (E, Ed), _ = R.cct_chain(*L, idx=idx)
    else:
        k, q, v, res, kd, qd, vd = L
        E, Ed = torch.bmm(k.permute(0, 2, 1), q), torch.bmm(kd.permute(0, 2, 1), qd)
    S, attn = R.select_rows(E, idx[0]), R.select_rows(Ed, idx[1])
    if dtype != F64:
        T = torch.gather(v, 2, idx[0].view(B, 1, -1).expand(-1, C, -1)).view(B, C, n, n)
        out = res + T * S.view(B, 1, n, n) + attn.view(B, 1, n, n) @ vd
    g = _grads(out, inp.go.to(dtype), L)
    return dict(zip(CCT_KEYS, [out.detach(), S.detach(), attn.detach()] + g))


def cct_replay(ref, dev_idx):
    idx, wrong = zip(*[replay_index(a, d) for a, d in zip(ref.amb, dev_idx)])
    return cct_evaluate(ref, list(idx)), list(wrong), list(idx)


def chain_seeds(prefix, want, leaves):
    """the seeded gradients of an add run: one per leaf, from the reference gradient"""
    return {n: acc_seed(want["d" + n], f"{prefix} seed {n}") for n in leaves}


def chain_figures(prefix, got, want, seeds=None):
    """per tensor max |err| / max |ref|; in an add run the gradient is compared with seed + gradient at the gradient's own scale
    -> [(label, error, bar key)...]"""
    figs = []
    for key, w in want.items():
        target = w
        if seeds is not None and key[0] == "d" and key[1:] in seeds:
            target = w + seeds[key[1:]].double()
        figs.append((f"{prefix}.{key}" + (" (add run)" if target is not w else ""),
                     float((got[key].detach().double() - target).abs().max() / w.abs().max()), f"{prefix}.{key}"))
    return figs


@contextlib.contextmanager
def one_thread():
    """the fp32 figures are taken with one thread, so that ATen's blocking does not depend on the machine's core count"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------- bars
# Largest error of an fp32 CPU evaluation (ATen: baddbmm, sum, mean, index_add_, matmul, sigmoid, softmax, linear / bmm under autograd
# with the replayed decisions) against tests/dense_ref.py in float64, over every case of the family: same inputs and metric as the
# GPU assertions (tests/test_dense_ref_cpu.py recomputes them: fp32_figures there).
#   sums and products: per element |err| / sum |terms|, the largest;  sigmoid, softmax: max |err|;  chains: max |err| / max |ref|
# Measured with torch 2 on an x86-64 CPU, one thread.
ORACLE_ERR = {
    "gemm": 2.971e-07,               # step linear forward (1024, 64, 64)
    "bias_act": 5.960e-08,           # step 1024x64: half an ulp, the one rounding of the add
    "sigmoid": 6.915e-08,            # 33x17 act3
    "colsum": 8.623e-08,             # (17, 63)
    "gather_bwd": 1.419e-07,         # (8, 128, 64), every index equal: 64 hits
    "spatial_mean": 1.039e-07,       # (65, 7)
    "spatial_mean_bwd": 9.138e-08,   # (96, 120)
    "bcast_fwd": 1.837e-07,          # (8, 128, 8)
    "bcast_bwd_a": 1.235e-07,        # (2, 3, 5)
    "bcast_bwd_v": 1.817e-07,        # (8, 128, 8)
    "mul_bwd_s": 1.144e-07,          # (2, 3, 300)
    "softmax": 8.649e-08,            # (2, 4096)
    "mlp.y": 2.161e-07, "mlp.dx": 2.765e-07, "mlp.dw1": 3.194e-07, "mlp.db1": 1.241e-07, "mlp.dw2": 2.766e-07, "mlp.db2": 1.476e-07,
    "cct.out": 1.421e-07, "cct.S": 1.240e-07, "cct.attn": 1.378e-07, "cct.dk": 1.550e-07, "cct.dq": 1.205e-07, "cct.dv": 1.032e-07,
    "cct.dres": 2.917e-08,           # the add run: seed + go rounds once; the fresh run is exact
    "cct.dkd": 1.545e-07, "cct.dqd": 1.396e-07, "cct.dvd": 1.347e-07,
}
# What tests/test_kernels_gpu.py::test_linear_and_cct_algebra holds the same quantity to (rtol + atol of `close`, relative to
# max(1, max |ref|)); S and attn were not compared there, and the kernel-level families had no test of their own.
FORMER_BARS = {k: None for k in ORACLE_ERR}
FORMER_BARS.update({"mlp.y": 1.1e-4, "cct.out": 1.1e-4})
FORMER_BARS.update({k: 2.1e-4 for k in ORACLE_ERR if k.startswith(("mlp.d", "cct.d"))})


def bar_rule(v, former=None):
    """8 x the fp32 evaluation's error rounded up to one significant digit (the rule of tests/photometric_cases.py), and never looser
    than what the quantity was held to before; no hardware allowance is added"""
    bar = round_up_1sig(8 * v) if v > 0 else 0.0
    return bar if former is None else min(bar, former)


BARS = {k: bar_rule(v, FORMER_BARS[k]) for k, v in ORACLE_ERR.items()}


def sum_bar(family, derived):
    """a sum's bar: the smaller of its derived first-order bound and the family's measured bar"""
    return min(derived, BARS[family])
