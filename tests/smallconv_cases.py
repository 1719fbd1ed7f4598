"""Cases, launch mirrors and bars of the direct small-channel convolution tests (tests/test_smallconv_f64_gpu.py on the device,
tests/test_smallconv_ref_cpu.py without one).

The mirrors restate, in plain Python, the launch expressions of jperceiver_amd/csrc/conv_common.h (up_head, small_head),
conv_small.hip (jp_up_head_fwd, jp_up_head_wgrad[_ws_floats], small_wgrad_grid, the `tiled` condition) and conv_c16.hip (jp_c16_ok,
jp_c16_wgrad), so that the CPU test can state which kernel, tier, band count and tile count every case takes.

Inputs are seeded randn; weights are scaled by (9 Cin)^-0.5; in the `scaled` cases input channel 1 is multiplied by 2^10 and channel 2
by 2^-10, so that a kernel that is right against the tensor's maximum but loose per element shows.  In the scaled SIGMOID case (U2) the
weights of those two channels carry the inverse factor: with the plain weights the pre-activation is N(0, 280^2), the sigmoid
saturates, fl32(1 - y) is 0 where y64 (1 - y64) is 1e-120, and every fp32 evaluation -- both yardsticks included -- is 100 % of S off
in dx (measured: 1.0 of S for ATen and for the chain, which would put the family's dx bar at 8).  With the inverse factor every product
keeps its size, the head works where the model's does, and the range still shows where it can: dw of channel 1 is 2^20 times dw of
channel 2, dx the other way round.  The leaky case C3 has no such problem and keeps the plain weights.
"""
import functools
import math

import torch

from tests import smallconv_ref as R
from tests.smallconv_ref import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID, Case

TPB = 256


def cdiv(a, b):
    return (a + b - 1) // b


# --------------------------------------------------------------------------------------------------- cases
def _up(name, N, C, h, wd, scaled=False):
    """disparity head: Cout = 1, one source stored at (h, wd), reflection, bias, sigmoid; the output is 2h x 2wd"""
    return Case(name, "up", N, ((C, 1),), 2 * h, 2 * wd, 1, True, True, ACT_SIGMOID, scaled)


CASES = {c.name: c for c in [
    _up("U1", 1, 8, 2, 2),
    _up("U2", 2, 13, 5, 6, scaled=True),
    _up("U3", 3, 10, 9, 20),
    _up("U4", 1, 9, 3, 4),
    _up("U5", 1, 11, 129, 256),
    _up("U6", 2, 12, 66, 128),
    _up("U7", 1, 768, 2, 4),
    _up("U8a", 1, 769, 2, 4),                   # the two that up_head() rejects: conv_small with an upsampled segment
    _up("U8b", 2, 7, 5, 6),
    Case("S1", "small", 2, ((6, 0),), 67, 70, 2, True, True, ACT_NONE, False),
    Case("S2", "small", 1, ((341, 0),), 6, 6, 4, False, True, ACT_NONE, False),
    Case("S3", "small", 2, ((3, 0),), 1, 9, 2, False, False, ACT_NONE, False),
    Case("S4r", "small", 1, ((3, 0), (4, 1), (1, 0)), 96, 96, 2, True, True, ACT_NONE, False),
    Case("S4z", "small", 1, ((3, 0), (4, 1), (1, 0)), 96, 96, 2, False, True, ACT_NONE, False),
    Case("S5", "small", 2, ((5, 1),), 20, 28, 3, True, False, ACT_NONE, False),
    Case("C1", "c16", 1, ((16, 0),), 64, 64, 16, False, False, ACT_NONE, False),
    Case("C2", "c16", 9, ((16, 1),), 64, 256, 16, False, True, ACT_RELU, False),
    Case("C3", "c16", 3, ((16, 0),), 96, 128, 16, False, True, ACT_LEAKY, True),
]}
FAMILIES = ("up", "small", "c16")
TIER_CASES = ("U2", "U6", "S1", "S4r", "S4z", "C2")       # weight-gradient tiers through the C ABI
GATHER_CASES = ("U1", "U2", "S4r", "S4z")                 # the reference against the independent gather evaluation

# Measured bars: 8 x the larger error of the two fp32 yardsticks (smallconv_ref.aten32, chain32) over the family's cases, rounded up to
# one significant digit; the yardstick figures stand in YARDSTICKS as (aten32, chain32) and tests/test_smallconv_ref_cpu.py recomputes
# them (ATen on one thread, so that the figures do not depend on the machine's core count; its weight and bias gradients are then
# sequential sums and some figures coincide with the chain's).  Every figure is max |x - ref64| / S over the tensor (S / 4 for the
# sigmoid outputs).  Nothing here was read off the device.
YARDSTICKS = {
    ("up", "fwd"): (1.484e-07, 1.565e-07), ("up", "dx"): (3.134e-07, 9.512e-07),
    ("up", "dw"): (2.732e-07, 7.210e-07), ("up", "db"): (3.534e-08, 1.483e-07),
    ("small", "fwd"): (2.554e-07, 2.249e-07), ("small", "dx"): (2.499e-07, 2.481e-07),
    ("small", "dw"): (2.641e-07, 2.641e-07), ("small", "db"): (3.777e-08, 3.777e-08),
    ("c16", "fwd"): (8.822e-07, 1.266e-06), ("c16", "dx"): (4.233e-07, 4.183e-07),
    ("c16", "dw"): (1.973e-07, 1.973e-07), ("c16", "db"): (8.389e-08, 8.389e-08),
}
MARGIN = 8


def round_up_1(v):
    """v rounded up to one significant digit"""
    e = math.floor(math.log10(v))
    m = math.ceil(v / 10 ** e - 1e-9)
    return m * 10 ** e


def bar_of(aten, chain):
    return round_up_1(MARGIN * max(aten, chain))


BARS = {k: bar_of(*v) for k, v in YARDSTICKS.items()}
AMBIGUOUS_CAP = 0.005             # at most 0.5 % of a case's ReLU gates may be left to the evaluation under test


# --------------------------------------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def inputs(name):
    case = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    xs = [torch.randn(case.N, C, case.H >> up, case.W >> up, generator=g) for C, up in case.srcs]
    if case.scaled:
        xs[0][:, 1] *= 2.0 ** 10
        xs[0][:, 2] *= 2.0 ** -10
    Ci = R.cin(case)
    w = torch.randn(case.Cout, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5
    if case.scaled and case.act == ACT_SIGMOID:       # (see the head of this file: the sigmoid must stay in its working range)
        w[:, 1] *= 2.0 ** -10
        w[:, 2] *= 2.0 ** 10
    b = torch.randn(case.Cout, generator=g) if case.bias else None
    dy = torch.randn(case.N, case.Cout, case.H, case.W, generator=g)
    return R.Inputs(xs, w, b, dy)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 forward of a case, computed once and shared (nobody writes into it)"""
    return R.forward(inputs(name), CASES[name])


def evaluate(name, got):
    case = CASES[name]
    return R.evaluate(inputs(name), case, reference(name), got, BARS[(case.family, "fwd")])


def dw_seed(name):
    case = CASES[name]
    g = torch.Generator().manual_seed(77 + sorted(CASES).index(name))
    return torch.randn(case.Cout, R.cin(case), 3, 3, generator=g) * 0.5


@functools.lru_cache(maxsize=None)
def tier_reference(name):
    """weight gradient of dy taken as the pre-activation gradient, added to dw_seed: what jp_conv2d_wgrad_src3 leaves with
    accumulate = 1 -> (float64 result, term sum with the seed as one more term)"""
    case, inp = CASES[name], inputs(name)
    bwd = R.backward(inp, case, inp.dy.double(), want_dx=False)
    seed = dw_seed(name).double()
    return bwd.dw + seed, bwd.S_dw + seed.abs()


# --------------------------------------------------------------------------------------------------- mirrors: conv_common.h
def up_head(case):
    (c0, up0), rest = case.srcs[0], case.srcs[1:]
    return (case.Cout == 1 and not rest and bool(up0) and 8 <= c0 <= 768 and case.reflect and case.H % 2 == 0 and case.W % 2 == 0
            and case.H >= 4 and case.W >= 4)


def small_head(case):
    return case.Cout <= 4 and case.Cout * R.cin(case) * 9 * 4 <= 48 * 1024


def c16_ok(case):
    return (len(case.srcs) == 1 and case.srcs[0][0] == 16 and case.Cout == 16 and not case.reflect and case.H % 32 == 0
            and case.W % 64 == 0 and case.H >= 64)


def route(case):
    """the first test of jp_conv2d_fwd_src3 / wgrad_impl that takes the case"""
    if up_head(case):
        return "up_head"
    fwd_first = "small" if small_head(case) else ("c16" if c16_ok(case) else "igemm")
    return fwd_first


# --------------------------------------------------------------------------------------------------- mirrors: conv_small.hip
def up_fwd(N, C, h, wd):
    """jp_up_head_fwd -> dict(kernel, workgroups per image, live lanes of the last workgroup, channel ranges of the four wave groups)"""
    if wd % 4 == 0:
        pairs = h * (wd // 2)
        if N * pairs <= 8 * 2048:
            cq = cdiv(C, 4)
            groups = [(min(C, g * cq), min(C, g * cq + cq)) for g in range(4)]
            return dict(kernel="up_head_fwd2s_kernel<4>", wgs=cdiv(pairs, 64), last=pairs - (cdiv(pairs, 64) - 1) * 64, groups=groups,
                        lds=16 * C * 4)
        return dict(kernel="up_head_fwd2_kernel", wgs=cdiv(pairs, TPB), last=pairs - (cdiv(pairs, TPB) - 1) * TPB, groups=None,
                    lds=16 * C * 4)
    return dict(kernel="up_head_fwd_kernel", wgs=cdiv(h * wd, TPB), last=h * wd - (cdiv(h * wd, TPB) - 1) * TPB, groups=None,
                lds=16 * C * 4)


def up_wgrad(N, C, h, wd):
    """the band arithmetic of jp_up_head_wgrad and the three scratch sizes that select its tiers"""
    hw = h * wd
    bands = max(1, min(hw // (TPB * 16), 16))
    band = cdiv(cdiv(hw, bands), TPB) * TPB
    nb = cdiv(hw, band)
    return dict(band=band, nb=nb, last_band=hw - (nb - 1) * band, blocks=cdiv(C, 8), block_tail=C % 8, d_floats=16 * N * hw,
                ws_floats=16 * N * hw + 16 * C * nb * N, folded=nb * N)


def small_wgrad(case):
    """jp_conv_small_wgrad: tiled condition, small_wgrad_grid and the partial-sum scratch"""
    N, H, W, Ci = case.N, case.H, case.W, R.cin(case)
    tiled = len(case.srcs) == 1 and not case.srcs[0][1] and H >= 2 and W >= 2
    if tiled:
        grid, chunk = (cdiv(H, 64), Ci, N), 0
    else:
        chunks = max(1, 2048 // max(1, Ci * N))
        chunks = min(chunks, max(1, H * W // 4096))
        chunk = cdiv(cdiv(H * W, chunks), TPB) * TPB
        grid = (cdiv(H * W, chunk), Ci, N)
    return dict(tiled=tiled, grid=grid, chunk=chunk, ws_floats=grid[0] * grid[2] * Ci * min(max(case.Cout, 1), 4) * 9,
                lds=case.Cout * Ci * 9 * 4)


# --------------------------------------------------------------------------------------------------- mirrors: conv_c16.hip
def c16_wgrad(case):
    ntiles = case.N * (case.H // 4) * (case.W // 64)
    grid = min(ntiles, 512)
    return dict(ntiles=ntiles, grid=grid, second_tile=max(0, ntiles - grid), tiles_per_image=(case.H // 4) * (case.W // 64),
                ws_floats=grid * case.Cout * 16 * 9)


def wgrad_ws_floats(case):
    """jp_conv2d_wgrad_src3_ws_floats for the cases of this file"""
    if c16_ok(case):
        return c16_wgrad(case)["ws_floats"]
    if up_head(case):
        return up_wgrad(case.N, case.srcs[0][0], case.H // 2, case.W // 2)["ws_floats"]
    assert small_head(case)
    return small_wgrad(case)["ws_floats"]
