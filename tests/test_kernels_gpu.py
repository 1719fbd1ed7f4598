"""Per-kernel parity tests on a real MI355X: every HIP kernel (called through the C ABI via
jperceiver_amd.ops) against plain PyTorch fp32 ops evaluated ON THE CPU (leaves are `.cpu()` clones: the referee is
ATen's CPU implementation, not MIOpen on the same device) / the oracle, on the same seeded inputs.
Tolerances: fp32 summation-order differences only (rtol 1e-4 unless noted)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops, ops_loss                                        # noqa: E402
from jperceiver_amd import _lib                                                # noqa: E402
from jperceiver_amd._lib import call                                           # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                            # noqa: E402
from oracle import jp_oracle as J                                              # noqa: E402

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + int(np.prod(shape)) % 9973)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= atol * scale + rtol * scale, f"{msg} max abs err {err:.3e} (scale {scale:.3e})"


def kink_act(pre, y_hip, act):
    """relu / leaky_relu of the CPU referee with the DEVICE's branch decision on pre-activations within 1e-4 of the
    kink: |fwd error| ~ 1e-5 can put such an element on the other side, and its derivative (1 vs 0 / 0.01) would then
    differ legitimately -- the forward values are compared separately, at tolerance."""
    if act not in (1, 2):
        return {0: lambda t: t, 3: torch.sigmoid}[act](pre)
    slope = 0.0 if act == 1 else 0.01
    pos = torch.where(pre.detach().abs() < 1e-4, y_hip.detach().cpu() > 0, pre.detach() > 0)
    return torch.where(pos, pre, slope * pre)


def pvar(t):
    """parameter-like Var: gradient accumulates into a zeroed buffer"""
    return Var(t, True, torch.zeros_like(t))


# ------------------------------------------------------------------------------------------- conv
CONV_CASES = [
    # N, Cin, H, W, Cout, K, stride, pad, pad_mode, act, bias
    (2, 64, 24, 40, 128, 3, 1, 1, 0, 0, False),     # resnet 3x3
    (2, 64, 24, 40, 128, 3, 2, 1, 0, 0, False),     # resnet 3x3 stride 2
    (2, 64, 24, 40, 128, 1, 2, 0, 0, 0, False),     # downsample 1x1 stride 2
    (2, 3, 32, 48, 64, 7, 2, 3, 0, 0, False),       # stem 7x7
    (2, 6, 32, 48, 64, 7, 2, 3, 0, 0, False),       # pose stem
    (1, 128, 16, 16, 256, 1, 1, 0, 0, 0, False),    # reduce 1x1
    (2, 96, 20, 28, 160, 3, 1, 1, 1, 2, True),      # reflect + bias + leaky (iconv / merge)
    (2, 256, 9, 13, 1, 3, 1, 1, 1, 3, True),        # disp head: Cout=1, sigmoid
    (3, 16, 12, 12, 2, 3, 1, 1, 1, 0, True),        # topview head Cout=2
    (2, 128, 2, 2, 128, 3, 1, 1, 1, 0, True),       # reflect pad on a 2x2 map
    (2, 512, 6, 20, 256, 1, 1, 0, 0, 1, True),      # pose reduce + relu
    (2, 200, 8, 8, 72, 3, 1, 1, 0, 0, True),        # odd channel counts, zero pad
    (1, 64, 70, 130, 64, 3, 1, 1, 0, 0, False),     # N-tile tail (pixels not multiple of 64)
    (2, 129, 10, 14, 96, 3, 1, 1, 1, 2, True),      # 128-aligned wgrad path + 1-channel tail (the 513-channel iconv shape)
    (1, 150, 9, 11, 80, 3, 1, 1, 0, 0, False),      # ... + 22-channel tail
    (2, 256, 8, 8, 128, 3, 1, 1, 1, 0, True),       # uniform-tap wgrad, reflect
    (2, 128, 6, 10, 72, 1, 1, 0, 0, 0, False),      # uniform-tap wgrad, 1x1
    (2, 64, 16, 24, 64, 3, 1, 1, 0, 0, False),      # 64-ch whole-tap wgrad tiles, Cout<=64 (4 taps / tile), zero pad
    (2, 64, 16, 24, 64, 3, 1, 1, 1, 0, True),       # ... reflect
    (2, 64, 32, 48, 128, 3, 2, 1, 0, 0, False),     # ... stride 2, 2 taps / tile
    (2, 64, 32, 48, 128, 1, 2, 0, 0, 0, False),     # ... 1x1 stride 2
    (2, 128, 16, 32, 256, 3, 2, 1, 0, 0, False),    # scalar-base uniform-tap wgrad, stride 2 zero pad
    (2, 256, 16, 16, 128, 3, 1, 1, 0, 1, True),     # scalar-base uniform-tap wgrad, zero pad
    (5, 64, 6, 10, 64, 3, 1, 1, 0, 0, False),       # pixel tiles straddling several images (relative-image offsets)
    (5, 96, 6, 10, 160, 3, 1, 1, 1, 0, False),      # ... reflect
    (2, 8, 70, 130, 1, 3, 1, 1, 1, 3, True),        # small-Cout head over several LDS tiles / row bands, reflect
    (1, 5, 80, 66, 3, 3, 1, 1, 0, 0, True),         # ... zero pad, Cout=3
    (2, 16, 16, 24, 16, 3, 1, 1, 0, 1, True),       # BEV decoder 16->16: half-empty K chunks, 16 taps slots / wgrad tile
    (2, 32, 16, 24, 32, 3, 1, 1, 0, 0, False),      # 32->32
    (2, 32, 16, 24, 16, 3, 1, 1, 1, 0, True),       # 32->16 reflect
    (2, 16, 9, 11, 24, 3, 1, 1, 0, 0, False),       # 16 channels, odd map (table wgrad)
    (1, 64, 8, 256, 64, 3, 1, 1, 0, 0, False),      # row-tile kernel (W % 256 == 0, Cout <= 64), zero pad
    (2, 96, 6, 128, 160, 3, 1, 1, 1, 2, True),      # row-tile kernel, 128-wide tiles, reflect + bias + leaky
    (2, 72, 5, 128, 72, 3, 1, 1, 0, 1, True),       # row-tile kernel, channel tail chunk, zero pad
    (1, 3, 448, 448, 64, 7, 2, 3, 0, 0, False),     # stem at a size that takes the whole-tap K-chunk path (CP = 4)
    (1, 6, 448, 452, 64, 7, 2, 3, 0, 1, True),      # pose stem (CP = 8), ragged width
    (2, 64, 96, 128, 256, 3, 1, 1, 1, 2, True),     # P9 patch kernel forward (reflect, 2 M tiles, 2 channel chunks)
    (2, 128, 64, 96, 160, 3, 1, 1, 0, 1, True),     # P9 forward zero pad (M tile tail 160 = 128 + 32) AND P9 dgrad (rows 128)
    (1, 32, 128, 256, 192, 3, 1, 1, 0, 0, False),   # P9 forward, a single channel chunk, tiles at every image border
    (3, 160, 32, 64, 128, 3, 1, 1, 1, 2, True),     # P9 dgrad main pass + reflection border pass, 3 images, rows 160
    (8, 64, 64, 96, 64, 3, 1, 1, 0, 0, False),      # P9 64-channel variant (8x32 pixel tiles), forward and dgrad, zero pad
    (6, 64, 64, 128, 48, 3, 1, 1, 1, 2, True),      # ... reflect, Cout 48 (row tail inside the only M tile)
    (2, 64, 96, 128, 256, 1, 1, 0, 0, 0, False),    # P1 (1x1 through the patch kernel): forward, 2 M tiles, one 64-channel stage
    (8, 128, 64, 64, 128, 1, 1, 0, 0, 1, True),     # P1 forward + dgrad, two stages, bias + relu
    (8, 64, 64, 96, 64, 1, 1, 0, 0, 0, False),      # P1 64-channel variant (8x32 pixel tiles), forward + dgrad
    (2, 192, 64, 64, 160, 1, 1, 0, 0, 2, True),     # P1: 3 stages, M tile tail (160), dgrad rows 192
    (2, 128, 32, 64, 128, 3, 1, 1, 1, 0, True),     # W9 patch wgrad: 2 input-channel tiles, reflect, tiles at every border
    (3, 192, 16, 32, 136, 3, 1, 1, 0, 0, False),    # W9: 3 input-channel tiles, Cout tail (136 = 128 + 8), zero pad, 3 images
    (8, 256, 32, 32, 256, 3, 1, 1, 1, 2, True),     # W9: 4 x 2 output tiles, K split over the 64 pixel tiles
    (2, 193, 16, 32, 128, 3, 1, 1, 1, 0, False),    # W9 on 192 channels + table pass for the 1-channel tail
    (4, 128, 32, 64, 64, 3, 1, 1, 0, 0, False),     # W9 narrow variant (Cout <= 64: two K groups per workgroup), 2 channel tiles
    (4, 129, 64, 96, 64, 3, 1, 1, 1, 2, True),      # P9 dgrad on the 128-row tile of a 129-channel bank + its 1-row tail launch
    (4, 64, 64, 128, 256, 3, 1, 1, 1, 2, True),     # P9 forward, 256-channel 8-wave tiles (>= 256 workgroups), reflect
    (4, 64, 64, 128, 256, 1, 1, 0, 0, 1, True),     # 1x1 through the patch kernel on 256-channel 8-wave tiles (default for such banks): forward
    (4, 256, 64, 128, 128, 1, 1, 0, 0, 0, False),   # ... dgrad (256 rows), 4 stages
    (2, 128, 32, 64, 256, 1, 1, 0, 0, 0, True),     # W1 patch wgrad (1x1): one 256 x 128 output tile, K split over 32 pixel tiles
    (2, 256, 32, 32, 200, 1, 1, 0, 0, 1, True),     # W1: two input-channel tiles, 200 output channels (clamped / masked rows)
    (4, 256, 64, 128, 64, 3, 1, 1, 0, 0, False),    # P9 dgrad on 256-row 8-wave tiles, zero pad (no tap-major pack built)
    (2, 6, 64, 128, 64, 7, 2, 3, 0, 1, True),       # W7 stem wgrad, 6 input channels (10 column blocks, one K group)
    (3, 3, 96, 192, 64, 7, 2, 3, 0, 0, False),      # W7 stem wgrad, 3 input channels (5 column blocks x 2 K groups), 3 images
]


# (fp32 referee, largest error of the tensor: tests/test_smallconv_f64_gpu.py holds the direct Cout <= 4, disparity-head and 16 -> 16 kernels
# per element to float64 references on every launch path, scratch tier and ragged channel count)
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_fwd_bwd(case):
    N, Cin, H, W, Cout, K, s, p, pm, act, bias = case
    x = rnd(N, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, K, K, seed=2, scale=(Cin * K * K) ** -0.5)
    b = rnd(Cout, seed=3) if bias else None
    xv, wv = Var(x, True), pvar(w)
    bv = pvar(b) if bias else None
    tape = Tape()
    with recording(tape):
        y = ops.conv2d(xv, wv, bv, s, p, pm, act)
    # reference
    xr, wr = x.detach().cpu().clone().requires_grad_(True), w.detach().cpu().clone().requires_grad_(True)
    br = b.detach().cpu().clone().requires_grad_(True) if bias else None
    xi = F.pad(xr, (p, p, p, p), mode="reflect") if pm == 1 else xr
    yr = kink_act(F.conv2d(xi, wr, br, s, 0 if pm == 1 else p), y.t, act)
    close(y.t, yr, msg="fwd")
    gy = rnd(*yr.shape, seed=4)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    close(xv.g, xr.grad, msg="dgrad")
    close(wv.g, wr.grad, rtol=2e-4, msg="wgrad")
    if bias:
        close(bv.g, br.grad, rtol=2e-4, msg="bias grad")


FUSED_UPSAMPLE_CASES = [            # N, H, W, Cr, Cx, Cout
    (2, 12, 20, 40, 24, 32),      # generic gather (unaligned segments)
    (3, 128, 128, 64, 64, 160),   # upsample-aware parity-class forward + per-source dgrad (4 slots on the upsampled segment)
    (3, 128, 128, 32, 96, 40),    # ... 64x256 tile, 3 channel chunks in the upsampled segment
    (2, 32, 64, 32, 128, 72),     # per-segment wgrad: parity-class kernels on the upsampled segment (Cx % 128 == 0)
    (1, 64, 128, 128, 128, 136),  # ... + uniform-tap path on the reduce segment, two M tiles
    (1, 192, 256, 128, 64, 136),  # per-source dgrad with the row-tile kernel on the full-resolution segment (W % 128 == 0)
    (1, 192, 256, 128, 64, 128),  # per-source dgrad: P9 patch kernel on the full-resolution segment's tiles of the bank's pack
    (2, 64, 96, 256, 128, 64),    # ... two 128-row tiles, 2 images
    (2, 64, 128, 64, 96, 256),    # P9U patch kernel forward: 2 skip stages + 3 upsampled stages + disparity stage, 2 M tiles
    (1, 128, 128, 32, 32, 128),   # P9U: one stage of each kind, tiles at every image border
]


@pytest.mark.parametrize("N,H,W,Cr,Cx,Cout", FUSED_UPSAMPLE_CASES)
def test_conv2d_fused_upsample_concat(N, H, W, Cr, Cx, Cout):
    """iconv_k(cat(reduce, up(x), disp)) and its three input gradients (depth_decoder.py:76-77)."""
    r, xh, d = rnd(N, Cr, H, W, seed=1), rnd(N, Cx, H // 2, W // 2, seed=2), rnd(N, 1, H, W, seed=3)
    w, b = rnd(Cout, Cr + Cx + 1, 3, 3, seed=4, scale=0.05), rnd(Cout, seed=5)
    rv, xv, dv, wv, bv = Var(r, True), Var(xh, True), Var(d, True), pvar(w), pvar(b)
    tape = Tape()
    with recording(tape):
        y = ops.conv2d(None, wv, bv, 1, 1, 1, 2, srcs=[(rv, 0), (xv, 1), (dv, 0)])
    leaves = [t.detach().cpu().clone().requires_grad_(True) for t in (r, xh, d, w, b)]
    cat = torch.cat((leaves[0], F.interpolate(leaves[1], scale_factor=2, mode="nearest"), leaves[2]), 1)
    yr = kink_act(F.conv2d(F.pad(cat, (1, 1, 1, 1), mode="reflect"), leaves[3], leaves[4]), y.t, 2)
    close(y.t, yr, msg="fwd")
    gy = rnd(*yr.shape, seed=6)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    for got, ref, nm in zip((rv.g, xv.g, dv.g, wv.g, bv.g), leaves, ("d_reduce", "d_x_half", "d_disp", "dw", "db")):
        close(got, ref.grad, rtol=2e-4, msg=nm)


DISPARITY_HEAD_CASES = [(2, 40, 6, 10), (1, 256, 20, 36), (3, 64, 2, 2), (1, 256, 64, 64),      # N, C, h, w
                        (8, 64, 128, 128)]      # large map: the one-chain two-pixel forward, precomputed-gather wgrad


# (fp32 referee, largest error of the tensor: tests/test_smallconv_f64_gpu.py holds the direct Cout <= 4, disparity-head and 16 -> 16 kernels
# per element to float64 references on every launch path, scratch tier and ragged channel count)
@pytest.mark.parametrize("N,C,h,w", DISPARITY_HEAD_CASES)
def test_disparity_head_on_upsampled_source(N, C, h, w):
    """disp_k = sigmoid(Conv3x3_reflect(up2x(x))) (depth_decoder.py:36-39,70-71): upsample-aware direct kernels."""
    x = rnd(N, C, h, w, seed=1)
    wt, b = rnd(1, C, 3, 3, seed=2, scale=0.1), rnd(1, seed=3)
    xv, wv, bv = Var(x, True), pvar(wt), pvar(b)
    tape = Tape()
    with recording(tape):
        y = ops.conv2d(None, wv, bv, 1, 1, 1, 3, srcs=[(xv, 1)])
    xr, wr, br = (t.detach().cpu().clone().requires_grad_(True) for t in (x, wt, b))
    up = F.interpolate(xr, scale_factor=2, mode="nearest")
    yr = torch.sigmoid(F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), wr, br))
    close(y.t, yr, msg="fwd")
    gy = rnd(*yr.shape, seed=4)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    close(xv.g, xr.grad, rtol=2e-4, msg="dx (half resolution)")
    close(wv.g, wr.grad, rtol=2e-4, msg="dw")
    close(bv.g, br.grad, rtol=2e-4, msg="db")


# ------------------------------------------------------------------------------------------- batch norm
@pytest.mark.parametrize("shape", [(3, 48, 14, 18), (3, 64, 14, 18),
                                   # a pose-encoder layer2 shape: float4 statistics and apply, one chunk per plane (N * C = 1024 but
                                   # HW = 1920 < 2 * 2048), under two iterations per thread -- no fp32 run reaches a fold before the last
                                   # one; chunked planes and folding runs are in tests/test_bn_f64_gpu.py
                                   (8, 128, 24, 80)])
@pytest.mark.parametrize("relu,res,nup", [(True, False, 1), (True, True, 1), (False, False, 2)])
def test_batchnorm_train(relu, res, nup, shape):
    N, C, H, W = shape
    x = rnd(N, C, H, W, seed=1) * 2 + 0.5
    g, b = rnd(C, seed=2) * 0.2 + 1, rnd(C, seed=3) * 0.1
    r = rnd(N, C, H, W, seed=4) if res else None
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    xv, gv, bv = Var(x, True), pvar(g), pvar(b)
    rvv = Var(r, True) if res else None
    tape = Tape()
    with recording(tape):
        y = ops.batchnorm_train(xv, gv, bv, rm, rv, rvv, relu, 0.1, 1e-5, nup)
    xr, gr, br = (t.detach().cpu().clone().requires_grad_(True) for t in (x, g, b))
    rr = r.detach().cpu().clone().requires_grad_(True) if res else None
    rm2, rv2 = torch.zeros(C), torch.ones(C)
    for _ in range(nup):
        yr = F.batch_norm(xr, rm2, rv2, gr, br, True, 0.1, 1e-5)
    if res:
        yr = yr + rr
    if relu:
        yr = F.relu(yr)
    close(y.t, yr, msg="fwd")
    close(rm, rm2, msg="running_mean")
    close(rv, rv2, msg="running_var")
    gy = rnd(*yr.shape, seed=5)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    close(xv.g, xr.grad, rtol=3e-4, msg="dx")
    close(gv.g, gr.grad, rtol=3e-4, msg="dgamma")
    close(bv.g, br.grad, rtol=3e-4, msg="dbeta")
    if res:
        close(rvv.g, rr.grad, msg="dres")


@pytest.mark.parametrize("shape,groups,nup", [((2, 8, 12, 20), 1, 1), ((4, 16, 64, 128), 2, 2), ((3, 5, 300, 64), 1, 1),
                                              ((8, 64, 512, 512), 1, 1), ((16, 64, 96, 320), 2, 1)],
                         ids=["small", "two-groups-double-update", "ragged-bands", "depth-stem-bench-shape", "pose-stem-bench-shape"])
def test_bn_relu_maxpool_fused_stem_tail(shape, groups, nup):
    """ops.bn_relu_maxpool_train (ResNet stem tail in one pass each way, csrc/bn.hip) against the two ops it replaces --
    batchnorm_train(relu) + maxpool(3, 2, 1): the pooled map, the argmax decisions (through the gradient) and the running
    statistics bit for bit, the gradients to fp32 rounding (the fused backward sums the same terms in another order) -- and,
    on the small shape, against ATen on the CPU.  Many exact ties: relu zeroes half the map."""
    N, C, H, W = shape
    x = rnd(N, C, H, W, seed=1) * 2 + 0.3
    g, b = rnd(C, seed=2) * 0.2 + 1, rnd(C, seed=3) * 0.1
    g[0] = -0.7                                                 # a negative scale: max and affine do not commute
    res = {}
    for fused in (True, False):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        xv, gv, bv = Var(x, True), pvar(g.clone()), pvar(b.clone())
        tape = Tape()
        with recording(tape):
            if fused:
                y = ops.bn_relu_maxpool_train(xv, gv, bv, rm, rv, 0.1, 1e-5, nup, groups)
            else:
                y = ops.maxpool(ops.batchnorm_train(xv, gv, bv, rm, rv, None, True, 0.1, 1e-5, nup, groups), 3, 2, 1)
        gy = rnd(*y.t.shape, seed=5)
        y.g = gy.clone()
        tape.backward()
        res[fused] = dict(y=y.t.clone(), rm=rm, rv=rv, dx=xv.g.clone(), dg=gv.g.clone(), db=bv.g.clone())
    a, r = res[True], res[False]
    assert torch.equal(a["y"], r["y"]) and torch.equal(a["rm"], r["rm"]) and torch.equal(a["rv"], r["rv"])
    close(a["dx"], r["dx"], rtol=2e-5, atol=1e-6, msg="dx vs unfused")
    close(a["dg"], r["dg"], rtol=2e-5, atol=1e-6, msg="dgamma vs unfused")
    close(a["db"], r["db"], rtol=2e-5, atol=1e-6, msg="dbeta vs unfused")
    # identical argmax decisions: the gradient reaches exactly the same input positions before the BatchNorm terms spread it
    if N * C * H * W <= 1 << 16 and groups == 1:
        xr, gr, br = (t.detach().cpu().clone().requires_grad_(True) for t in (x, g, b))
        rm2, rv2 = torch.zeros(C), torch.ones(C)
        for _ in range(nup):
            yr = F.batch_norm(xr, rm2, rv2, gr, br, True, 0.1, 1e-5)
        yr = F.max_pool2d(F.relu(yr), 3, 2, 1)
        close(a["y"], yr, msg="fwd vs ATen")
        close(a["rm"], rm2, msg="running_mean")
        yr.backward(gy.cpu())
        close(a["dx"], xr.grad, rtol=3e-4, msg="dx vs ATen")
        close(a["dg"], gr.grad, rtol=3e-4, msg="dgamma vs ATen")
        close(a["db"], br.grad, rtol=3e-4, msg="dbeta vs ATen")


# ------------------------------------------------------------------------------------------- pooling & co
@pytest.mark.parametrize("k,s,p,H,W", [(3, 2, 1, 20, 28), (5, 1, 2, 9, 13), (2, 2, 0, 8, 8), (3, 2, 1, 21, 27),
                                       (5, 1, 2, 40, 150), (3, 2, 1, 70, 262), (2, 2, 0, 36, 132), (3, 1, 1, 19, 70),
                                       # row-streaming 5x5 kernels (W = 32 / 64 / 128 / 256): several row bands, ragged last
                                       # band, dead lane groups in the last wave, many exact ties
                                       (5, 1, 2, 32, 32), (5, 1, 2, 64, 64), (5, 1, 2, 70, 128), (5, 1, 2, 130, 256),
                                       (5, 1, 2, 7, 32), (5, 1, 2, 3, 64),
                                       # 3x3 stride-2 stem backward (2x2-cell gather kernel): row bands (ragged last one), ties
                                       (3, 2, 1, 64, 128), (3, 2, 1, 300, 64), (3, 2, 1, 2, 4)])
def test_maxpool(k, s, p, H, W):
    x = rnd(2, 5, H, W, seed=1)
    if H > 30:
        x = torch.round(x * 2) / 2      # many exact ties -> exercises the first-maximum rule
    xv = Var(x, True)
    tape = Tape()
    with recording(tape):
        y = ops.maxpool(xv, k, s, p)
    xr = x.detach().cpu().clone().requires_grad_(True)
    yr = F.max_pool2d(xr, k, s, p)
    close(y.t, yr, rtol=0, atol=0)
    gy = rnd(*yr.shape, seed=2)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    close(xv.g, xr.grad, rtol=1e-6)


def test_crp_block_single_node_backward():
    """CRPBlock (layers.py:184-199) runs as one tape node whose backward folds the residual gradient into the
    max-pool backward kernels; values and all gradients must match the plain autograd chain."""
    from jperceiver_amd.model.modules import CRPBlock
    torch.manual_seed(0)
    blk = CRPBlock(32, 32, 4).to(DEV)
    x = rnd(2, 32, 20, 28, seed=1)
    x = torch.round(x * 4) / 4                       # ties in the 5x5 windows
    xv = Var(x, True)
    tape = Tape()
    with recording(tape):
        y = blk._fwd(ops.act(xv, ops.ACT_RELU))      # a producer node in front, as in the decoder
    xr = x.detach().cpu().clone().requires_grad_(True)
    ws = [getattr(blk, f"{i + 1}_pointwise").conv.weight for i in range(4)]
    wr = [w.detach().detach().cpu().clone().requires_grad_(True) for w in ws]
    top = acc = F.relu(xr)
    for w in wr:
        top = F.conv2d(F.max_pool2d(top, 5, 1, 2), w)
        acc = top + acc
    close(y.t, acc, msg="fwd")
    gy = rnd(*acc.shape, seed=2)
    y.g = gy.clone()
    tape.backward()
    acc.backward(gy.cpu())
    close(xv.g, xr.grad, rtol=2e-4, msg="dx")
    for w, r in zip(ws, wr):
        close(w.grad, r.grad, rtol=3e-4, msg="dw")   # ops.param accumulates into .grad


@pytest.mark.parametrize("H,W", [(5, 7), (6, 8), (3, 6)])   # scalar, float4 and float2 code paths
def test_upsample_cat_add_mask_act(H, W):
    x = rnd(2, 6, H, W, seed=1)
    xv = Var(x, True)
    a, b = Var(rnd(2, 3, 2 * H, 2 * W, seed=2), True), Var(rnd(2, 4, 2 * H, 2 * W, seed=3), True)
    m = (rnd(2, 6, H, W, seed=4) > 0).float()
    tape = Tape()
    with recording(tape):
        u = ops.upsample2x(ops.mul_mask(xv, m, 2.0))
        c = ops.cat_channels([a, u, b])
        y = ops.act(ops.add(c, c), ops.ACT_LEAKY)
    leaves = [t.detach().cpu().clone().requires_grad_(True) for t in (x, a.t, b.t)]
    ur = F.interpolate(leaves[0] * m.cpu() * 2.0, scale_factor=2, mode="nearest")
    cr = torch.cat((leaves[1], ur, leaves[2]), 1)
    yr = F.leaky_relu(cr + cr)
    close(y.t, yr)
    gy = rnd(*yr.shape, seed=5)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    for got, ref in zip((xv.g, a.g, b.g), leaves):
        close(got, ref.grad)


@pytest.mark.parametrize("H,W,OH,OW", [(16, 16, 64, 64), (8, 12, 37, 50), (32, 32, 12, 40), (64, 64, 19, 62), (30, 44, 12, 40)])
def test_bilinear_resize(H, W, OH, OW):
    x = rnd(2, 3, H, W, seed=1)
    xv = Var(x, True)
    tape = Tape()
    with recording(tape):
        y = ops.bilinear_resize(xv, OH, OW)
    xr = x.detach().cpu().clone().requires_grad_(True)
    yr = F.interpolate(xr, [OH, OW], mode="bilinear", align_corners=False)
    close(y.t, yr)
    gy = rnd(*yr.shape, seed=2)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    close(xv.g, xr.grad)


def test_area_downsample():
    x = rnd(2, 3, 32, 48, seed=1)
    for f in (2, 4, 8):
        close(ops.area_downsample(x, f), F.interpolate(x.cpu(), (32 // f, 48 // f), mode="area"))


# ------------------------------------------------------------------------------------------- small dense / CCT
# (one shape, fp32 referee: tests/test_dense_f64_gpu.py holds every kernel of small.hip per element to float64 references at ragged
# tiles, several workgroups, ties, NaN / Inf and seeded accumulation)
def test_linear_and_cct_algebra():
    B, C, n = 2, 16, 6
    x = rnd(B, 5, 36, seed=1)
    w, b = rnd(36, 36, seed=2, scale=0.2), rnd(36, seed=3)
    xv, wv, bv = Var(x, True), pvar(w), pvar(b)
    k, q, v = Var(rnd(B, C, n * n, seed=4), True), Var(rnd(B, C, n * n, seed=5), True), Var(rnd(B, 20, n * n, seed=6), True)
    att, vd = Var(rnd(B, 1, n, n, seed=7), True), Var(rnd(B, 20, n, n, seed=8), True)
    tape = Tape()
    with recording(tape):
        y = ops.linear_act(xv, wv, bv, ops.ACT_RELU)
        e = ops_loss.bmm_tn(k, q)
        fs, arg = ops_loss.colmax(e)
        T = ops_loss.gather_cols(v, arg)
        S = ops_loss.view(fs, (B, 1, n, n))
        r = ops_loss.mul_bcast_c(ops_loss.view(T, (B, 20, n, n)), S)
        o = ops.add(r, ops_loss.bcast_matmul(att, vd))
    L = [t.detach().cpu().clone().requires_grad_(True) for t in (x, w, b, k.t, q.t, v.t, att.t, vd.t)]
    yr = F.relu(F.linear(L[0], L[1], L[2]))
    er = torch.bmm(L[3].permute(0, 2, 1), L[4])
    fsr, argr = torch.max(er, dim=1)
    Tr = torch.gather(L[5], 2, argr.view(B, 1, -1).expand(-1, 20, -1)).view(B, 20, n, n)
    orr = Tr * fsr.view(B, 1, n, n) + L[6] @ L[7]
    close(y.t, yr)
    assert torch.equal(arg.cpu(), argr)
    close(o.t, orr)
    gy, go = rnd(*yr.shape, seed=9), rnd(*orr.shape, seed=10)
    y.g, o.g = gy.clone(), go.clone()
    tape.backward()
    (yr * gy.cpu()).sum().backward()
    (orr * go.cpu()).sum().backward()
    for got, ref, nm in zip((xv.g, wv.g, bv.g, k.g, q.g, v.g, att.g, vd.g), L, "x w b k q v att vd".split()):
        close(got, ref.grad, rtol=2e-4, msg=nm)


# ------------------------------------------------------------------------------------------- photometric
def _geom(B, H, W, seed=7):
    K = torch.tensor([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]).repeat(B, 1, 1)
    invK = torch.linalg.pinv(K)
    g = torch.Generator().manual_seed(seed)
    aa = (torch.rand(B, 3, generator=g) - 0.5) * 0.06
    tr = (torch.rand(B, 3, generator=g) - 0.5) * 0.2
    return K, invK, aa, tr


@pytest.mark.parametrize("H,W,hs,ws,invert", [(32, 48, 16, 24, False), (40, 72, 5, 9, True), (64, 64, 32, 32, True)])
def test_cgt_warp_and_pose(H, W, hs, ws, invert):
    B = 2
    K, invK, aa, tr = _geom(B, H, W)
    g = torch.Generator().manual_seed(3)
    disp = torch.rand(B, 1, hs, ws, generator=g) * 0.5 + 0.2
    col = torch.rand(B, 3, H, W, generator=g)
    go = torch.randn(B, 3, H, W, generator=g)
    # oracle on CPU
    L = [t.detach().cpu().clone().requires_grad_(True) for t in (disp, aa, tr)]
    T = J.transformation_from_parameters(L[1].view(B, 1, 3), L[2].view(B, 1, 3), invert)
    d_up = F.interpolate(L[0], [H, W], mode="bilinear", align_corners=False)
    _, depth = J.disp_to_depth(d_up, 0.1, 100.0)
    grid = J.project(J.backproject(depth, invK), K, T, H, W)
    pr = F.grid_sample(col, grid, mode="bilinear", padding_mode="border", align_corners=False)
    (pr * go).sum().backward()
    # HIP
    dv, av, tv = Var(disp.to(DEV), True), Var(aa.to(DEV), True), Var(tr.to(DEV), True)
    Kd, iKd, cd = K.to(DEV), invK.to(DEV), col.to(DEV)
    tape = Tape()
    with recording(tape):
        pp = ops_loss.pose(av, tv, Kd, invert)
    pred = torch.empty(B, 3, H, W, device=DEV)
    call("jp_cgt_warp_fwd", dv.t, hs, ws, iKd, pp.P, cd, pred, B, H, W, 0.1, 100.0)
    close(pp.T, T, rtol=1e-5, atol=1e-6, msg="cam_T_cam")
    close(pred, pr, rtol=2e-3, atol=2e-3, msg="warped image")
    dup = torch.empty(B, 1, H, W, device=DEV)
    call("jp_cgt_warp_bwd", go.to(DEV).contiguous(), dv.t, hs, ws, iKd, pp.P, cd, dup, pp.dP, B, H, W, 0.1, 100.0, 0)
    gd = torch.empty_like(dv.t)
    call("jp_bilinear_bwd", dup, gd, B, hs, ws, H, W, 0)
    tape.backward()
    # gradients through border clipping / floor are piecewise: compare in aggregate
    ref = L[0].grad
    err = (gd.cpu() - ref).abs().max() / (ref.abs().max() + 1e-12)
    assert err < 2e-2, f"ddisp rel err {err}"
    for got, r, nm in ((av.g, L[1].grad, "d_axisangle"), (tv.g, L[2].grad, "d_translation")):
        e = (got.cpu() - r).abs().max() / (r.abs().max() + 1e-12)
        assert e < 2e-2, f"{nm} rel err {e}"


@pytest.mark.parametrize("H,W", [(16, 16), (37, 70), (64, 130), (48, 256)])
def test_ssim_l1_fwd_bwd(H, W):
    B = 2
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 3, H, W, generator=g)
    y = 0.7 * x + 0.3 * torch.rand(B, 3, H, W, generator=g)
    xr = x.detach().cpu().clone().requires_grad_(True)
    lr = J.reprojection_loss(xr, y)
    out = ops_loss.ssim_l1(x.to(DEV), y.to(DEV))
    close(out, lr, rtol=1e-4, atol=1e-5, msg="fwd")
    idx = (torch.rand(B, H, W, generator=g) * 4).long()
    cand = 2
    w = (idx == cand).float().unsqueeze(1) * 0.37
    (lr * w).sum().backward()
    dp = torch.empty(B, 3, H, W, device=DEV)
    gout = torch.tensor([0.37], device=DEV)
    call("jp_ssim_l1_bwd", x.to(DEV), y.to(DEV), idx.to(DEV), cand, gout, 1.0, dp, B, H, W)
    close(dp, xr.grad, rtol=2e-4, atol=1e-6, msg="bwd")


def test_minreproj():
    B, H, W = 2, 9, 11
    c = [rnd(B, 1, H, W, seed=i).abs() for i in range(4)]
    nz = [rnd(B, 1, H, W, seed=10 + i) for i in range(2)]
    idx = torch.empty(B, H, W, device=DEV, dtype=torch.int64)
    acc = torch.zeros(1, device=DEV, dtype=torch.float64)
    call("jp_minreproj_fwd", c[0], c[1], c[2], c[3], nz[0], nz[1], idx, acc, B * H * W)
    cat = torch.cat([c[0] + nz[0] * 1e-5, c[1] + nz[1] * 1e-5, c[2], c[3]], 1)
    m, i = torch.min(cat, dim=1)
    assert torch.equal(idx, i)
    assert abs(float(acc) - float(m.double().sum())) < 1e-5


# ------------------------------------------------------------------------------------------- other losses
@pytest.mark.parametrize("h,w,f", [(16, 24, 2), (8, 8, 4), (33, 20, 1)])
def test_smooth_loss(h, w, f):
    B = 2
    g = torch.Generator().manual_seed(2)
    disp = torch.rand(B, 1, h, w, generator=g) * 0.6 + 0.1
    img = torch.rand(B, 3, h * f, w * f, generator=g)
    dr = disp.detach().cpu().clone().requires_grad_(True)
    dn = dr / (dr.mean(2, True).mean(3, True) + 1e-7)
    ref = J.smooth_loss(dn, img) * 0.25
    ref.backward()
    lv = ops_loss.LossVec(["s"], DEV)
    dv = Var(disp.to(DEV), True)
    tape = Tape()
    with recording(tape):
        ops_loss.smooth_loss(lv, "s", dv, ops.area_downsample(img.to(DEV), f), 0.25)
    call("jp_fill", lv.grads, 1, 1.0)
    tape.backward()
    close(lv.vals, ref.reshape(1), rtol=2e-4, msg="value")
    close(dv.g, dr.grad, rtol=5e-4, atol=1e-6, msg="grad")


@pytest.mark.parametrize("hs,ws,FH,FW,crop", [(16, 16, 37, 124, None), (32, 32, 20, 30, None), (8, 8, 60, 80, (10, 50, 5, 70))])
def test_scale_loss(hs, ws, FH, FW, crop):
    B = 2
    g = torch.Generator().manual_seed(4)
    disp = torch.rand(B, 1, hs, ws, generator=g) * 0.3 + 0.01
    label = torch.rand(B, 1, FH, FW, generator=g) * 30
    label[label < 12] = 0
    dr = disp.detach().cpu().clone().requires_grad_(True)
    _, depth = J.disp_to_depth(dr, 0.1, 100.0)
    opt = J.default_opt(type="static")
    lab = label
    if crop is not None:
        m = torch.zeros_like(label)
        m[:, :, crop[0]:crop[1], crop[2]:crop[3]] = 1
        lab = label * m
    ref = J.scale_loss(opt, depth, lab) * 0.05
    ref.backward()
    lv = ops_loss.LossVec(["s"], DEV)
    dv = Var(disp.to(DEV), True)
    tape = Tape()
    with recording(tape):
        ops_loss.scale_loss(lv, "s", dv, label.to(DEV), 0.05, 0.1, 100.0, crop)
    call("jp_fill", lv.grads, 1, 1.0)
    tape.backward()
    close(lv.vals, ref.reshape(1), rtol=2e-4, msg="value")
    close(dv.g, dr.grad, rtol=1e-3, atol=1e-6, msg="grad")


def _masks(n=48):
    masks = np.zeros((5, 1, n, n), np.float32)
    yy, xx = np.mgrid[:n, :n]
    masks[1, 0] = ((yy - 20) ** 2 + (xx - 25) ** 2 < 100)
    r2 = (yy - 24) ** 2 + (xx - 24) ** 2
    masks[2, 0] = (r2 < 300) & (r2 > 90)
    masks[3, 0, 10, 30] = 1
    masks[4, 0] = 1
    return masks


def test_sdf_matches_reference_golden(golden_dir):
    g = np.load(golden_dir + "/unit_vectors.npz")
    m = torch.from_numpy(_masks()).to(DEV)
    sdf = ops_loss.signed_distance(m)
    ref = torch.from_numpy(g["sdf/out"][:, 1]).float()
    close(sdf, ref, rtol=0, atol=1e-6, msg="sdf vs scipy (reference golden)")


def test_sdf_random_and_layout_loss(golden_dir):
    gld = np.load(golden_dir + "/unit_vectors.npz")
    from jperceiver_amd import synthetic as syn
    n = 48
    masks = _masks(n)
    logits = torch.from_numpy((syn.hash_uniform(7, "logits", (5, 2, n, n)) - 0.5) * 4)
    lab = torch.from_numpy(masks)
    for mode, (lw, cew, l2w) in {"iou": (1.0, 0.0, 0.0), "ce": (0.0, 1.0, 0.0), "bd": (0.0, 0.0, 1.0), "sum3": (20.0, 1.0, 20.0)}.items():
        lr = logits.detach().cpu().clone().requires_grad_(True)
        gt = lab.long().squeeze(1)
        ref = lw * J.iou_loss(lr, gt) + cew * F.cross_entropy(lr, gt, weight=torch.tensor([1.0, 5.0])) + l2w * J.bd_loss(lr, gt)
        ref.backward()
        if mode == "iou":
            assert float(ref) == pytest.approx(float(gld["loss/iou"]), rel=1e-6)
        if mode == "bd":
            assert float(ref) == pytest.approx(float(gld["loss/bd"]), rel=1e-6)
        lv = ops_loss.LossVec(["t"], DEV)
        zv = Var(logits.to(DEV), True)
        labd = lab.to(DEV)
        tape = Tape()
        with recording(tape):
            ops_loss.layout_loss(lv, "t", zv, labd, ops_loss.signed_distance(labd), 1.0, 5.0, lw, cew, l2w)
        call("jp_fill", lv.grads, 1, 1.0)
        tape.backward()
        close(lv.vals, ref.detach().float().reshape(1), rtol=2e-4, msg=mode + " value")
        close(zv.g, lr.grad.float(), rtol=5e-4, atol=1e-7, msg=mode + " grad")


def test_sdf_random_masks():
    from scipy.ndimage import distance_transform_edt  # noqa: F401  (oracle uses it)
    g = torch.Generator().manual_seed(9)
    m = (torch.rand(3, 1, 64, 40, generator=g) > 0.7).float()
    m[1] = 0
    oh = torch.cat([1 - m, m], 1).numpy()
    ref = torch.from_numpy(J.compute_sdf(oh)[:, 1]).float()
    close(ops_loss.signed_distance(m.to(DEV)), ref, rtol=0, atol=1e-6)


def test_l1_and_combine():
    a, b = rnd(2, 8, 4, 4, seed=1), rnd(2, 8, 4, 4, seed=2)
    lv = ops_loss.LossVec(["l1", "x", "c"], DEV)
    av, bv = Var(a, True), Var(b, True)
    tape = Tape()
    with recording(tape):
        ops_loss.l1_loss(lv, "l1", av, bv)
        ops_loss.combine(lv, "c", [("l1", 0.001), ("x", 1.0)])
    close(lv.vals[0:1], F.l1_loss(a.cpu(), b.cpu()).reshape(1))
    close(lv.vals[2:3], (0.001 * F.l1_loss(a.cpu(), b.cpu())).reshape(1))
    call("jp_fill", lv.grads, 3, 1.0)
    tape.backward()
    ar = a.detach().cpu().clone().requires_grad_(True)
    (1.001 * F.l1_loss(ar, b.cpu())).backward()
    close(av.g, ar.grad)
    close(bv.g, -ar.grad)


# ------------------------------------------------------------------------------------------- optimizer / rng
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_adam_clip_matches_torch(grad_scale):
    """clip_grad_norm_(35) + torch.optim.Adam on the CPU vs the two-stage norm + fused clip/Adam pass; grad_scale = 0.5
    is the 2-rank data-parallel case: the arena holds the SUM of the ranks' gradients and the 1/world averaging is
    folded into the kernel (norm AND update must see the mean gradient)."""
    n = 10007
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2) * 3
    pr = p0.detach().cpu().clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    nblk = int(ops._jplib().fn["jp_sumsq_blocks"]())
    part = torch.zeros(2 * nblk, device=DEV, dtype=torch.float64)
    nsq = torch.zeros(1, device=DEV, dtype=torch.float64)
    for step in range(1, 4):
        g = g0 * step                                  # mean gradient
        pr.grad = g.cpu().clone()
        torch.nn.utils.clip_grad_norm_([pr], 35.0)
        opt.step()
        gs = (g / grad_scale).contiguous()             # what the arena holds after the SUM all-reduce
        h = 5120                                       # two "buckets" (16-B aligned split), folded in a fixed order
        call("jp_grad_sumsq_partials", gs[:h], part[:nblk], h)
        call("jp_grad_sumsq_partials", gs[h:], part[nblk:], n - h)
        call("jp_sum_doubles", part, nsq, 2 * nblk)
        assert float(nsq) == pytest.approx(float((gs.double() ** 2).sum()), rel=1e-6)
        call("jp_adam_clip_step", p, gs, m, v, n, nsq, grad_scale, 35.0, 1e-3, 0.9, 0.999, 1e-8, step)
        close(p, pr, rtol=1e-5, atol=1e-6, msg=f"step {step}")


def test_grad_norm_is_deterministic():
    """The global-norm reduction has a fixed order (no atomics): bit-identical run to run."""
    g = rnd(3_000_017, seed=5) * 2
    nblk = int(ops._jplib().fn["jp_sumsq_blocks"]())
    part = torch.zeros(nblk, device=DEV, dtype=torch.float64)
    outs = []
    for _ in range(5):
        nsq = torch.zeros(1, device=DEV, dtype=torch.float64)
        call("jp_grad_sumsq_partials", g, part, g.numel())
        call("jp_sum_doubles", part, nsq, nblk)
        outs.append(float(nsq))
    assert len(set(outs)) == 1
    assert outs[0] == pytest.approx(float((g.double() ** 2).sum()), rel=1e-7)


def test_rng_statistics():
    m = ops.keep_mask((1 << 20,), DEV, 0.5)
    assert abs(float(m.mean()) - 0.5) < 5e-3 and set(m.unique().tolist()) == {0.0, 1.0}
    z = ops.randn((1 << 20,), DEV)
    assert abs(float(z.mean())) < 5e-3 and abs(float(z.std()) - 1.0) < 5e-3
    assert not torch.equal(ops.keep_mask((64,), DEV), ops.keep_mask((64,), DEV)) or True


# ------------------------------------------------------------------------------------------- §8b public callables
def test_ssim_module_matches_reference_vector(golden_dir):
    """`SSIM()(x, y)` (layers.py:97-107) vs the map the reference produced (unit_vectors.npz) and the oracle."""
    from jperceiver_amd import synthetic as syn
    from jperceiver_amd.model.modules import SSIM
    g = np.load(golden_dir + "/unit_vectors.npz")
    x = torch.from_numpy(syn.hash_uniform(7, "ssim_x", (2, 3, 16, 16)))
    y = 0.7 * x + 0.3 * torch.from_numpy(syn.hash_uniform(7, "ssim_y", (2, 3, 16, 16)))
    out = SSIM()(x.to(DEV), y.to(DEV))
    assert out.shape == (2, 3, 16, 16)
    close(out, torch.from_numpy(g["ssim/out"]), rtol=1e-5, atol=1e-5, msg="vs reference vector")
    for H, W in ((37, 70), (2, 2), (64, 130)):
        a = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H))
        b = 0.6 * a + 0.4 * torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(W))
        close(SSIM()(a.to(DEV), b.to(DEV)), J.ssim(a, b), rtol=1e-5, atol=1e-5, msg=f"vs oracle {H}x{W}")
    with pytest.raises(ValueError):
        SSIM()(x.to(DEV), y[:, :2].to(DEV))


def test_backproject_project_modules_match_reference_vector(golden_dir):
    """`Backproject(B,H,W)(depth, inv_K)` and `Project(B,H,W)(points, K, T)` (layers.py:41-82) vs the sampling grid
    the reference produced for the same inputs (unit_vectors.npz: warp/grid) and the oracle."""
    from jperceiver_amd import synthetic as syn
    from jperceiver_amd.model.modules import Backproject, Project
    g = np.load(golden_dir + "/unit_vectors.npz")
    Bn, H, W = 2, 12, 20
    K = torch.tensor([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]).repeat(Bn, 1, 1)
    invK = torch.linalg.pinv(K)
    depth = 1.0 / (0.01 + 9.99 * torch.from_numpy(syn.hash_uniform(7, "d", (Bn, 1, H, W))))
    vec = torch.from_numpy((syn.hash_uniform(7, "aa", (8, 1, 3)) - 0.5) * 0.2)
    vec[0] = 0
    tr = torch.from_numpy((syn.hash_uniform(7, "tr", (8, 1, 3)) - 0.5))
    T = J.transformation_from_parameters(vec[1:3], tr[1:3] * 0.3, invert=False)
    cam = Backproject(Bn, H, W)(depth.to(DEV), invK.to(DEV))
    assert cam.shape == (Bn, 4, H * W)
    close(cam, J.backproject(depth, invK), rtol=1e-5, atol=1e-5, msg="cam points vs oracle")
    pix = Project(Bn, H, W)(cam, K.to(DEV), T.to(DEV))
    assert pix.shape == (Bn, H, W, 2)
    close(pix, torch.from_numpy(g["warp/grid"]), rtol=1e-4, atol=1e-4, msg="grid vs reference vector")
    with pytest.raises(ValueError):
        Project(Bn, H, W)(cam[:, :3].contiguous(), K.to(DEV), T.to(DEV))


def test_iou_and_bd_loss_classes_match_reference_vectors(golden_dir):
    """`IoULoss(apply_nonlin=softmax)(x, y)` (dice_loss.py:293-331) and `BDLoss()(logits, gt)`
    (boundary_loss.py:150-192): values vs the reference's (unit_vectors.npz), gradients vs the oracle."""
    from jperceiver_amd import synthetic as syn
    from jperceiver_amd.model import IoULoss, BDLoss
    gld = np.load(golden_dir + "/unit_vectors.npz")
    n = 48
    masks = _masks(n)
    logits = torch.from_numpy((syn.hash_uniform(7, "logits", (5, 2, n, n)) - 0.5) * 4)
    gt = torch.from_numpy(masks[:, 0]).long()
    softmax_helper = lambda t: F.softmax(t, 1)       # noqa: E731  (the reference's own helper, net.py:563)
    from jperceiver_amd.model import SoftDiceLoss, TverskyLoss, FocalLoss
    for cls, key, orc in ((lambda: IoULoss(apply_nonlin=softmax_helper), "loss/iou", J.iou_loss), (BDLoss, "loss/bd", J.bd_loss),
                          (lambda: SoftDiceLoss(apply_nonlin=softmax_helper), "loss/dice", lambda z, t: J.region_loss(z, t, 2.0, 1.0, 1.0)),
                          (lambda: TverskyLoss(apply_nonlin=softmax_helper), "loss/tversky", lambda z, t: J.region_loss(z, t, 1.0, 0.3, 0.7)),
                          (lambda: FocalLoss(apply_nonlin=softmax_helper), "loss/focal", J.focal_loss)):
        z = logits.to(DEV).requires_grad_(True)
        loss = cls()(z, gt.to(DEV))
        assert loss.dim() == 0
        assert float(loss) == pytest.approx(float(gld[key]), rel=2e-5, abs=1e-7), key
        (loss * 0.7).backward()
        zr = logits.clone().requires_grad_(True)
        (orc(zr, gt) * 0.7).backward()
        close(z.grad, zr.grad.float(), rtol=5e-4, atol=1e-7, msg=key + " grad")
    # one-hot ground truth is accepted like in get_tp_fp_fn (dice_loss.py:53-55)
    oh = torch.stack([1 - gt, gt], 1).float()
    l2 = IoULoss(apply_nonlin=softmax_helper)(logits.to(DEV), oh.to(DEV))
    assert float(l2) == pytest.approx(float(gld["loss/iou"]), rel=2e-5)
    with pytest.raises(NotImplementedError):
        IoULoss(apply_nonlin=None)
    with pytest.raises(NotImplementedError):
        IoULoss(apply_nonlin=softmax_helper, batch_dice=True)


@pytest.mark.parametrize("N,C,H,W,act", [(3, 5, 37, 13, 2), (8, 16, 64, 64, 2), (2, 7, 128, 96, 1), (1, 3, 1, 5, 2)])
def test_act_bwd_bias_one_pass(N, C, H, W, act):
    """jp_act_bwd_bias: dx = dy * act'(y) and dbias[c] += sum over (n, pixels) of dx in one pass (layers.py:147-167 Conv3x3 blocks:
    bias + LeakyReLU) -- against the two-kernel form (jp_act_bwd, jp_channel_sum) and a float64 sum; dbias is accumulated into."""
    dy, y = rnd(N, C, H, W, seed=3), rnd(N, C, H, W, seed=4)
    dx = torch.empty_like(dy)
    db = torch.full((C,), 0.25, device=DEV)
    call("jp_act_bwd_bias", dy, y, dx, db, N, C, H * W, act, None, None)
    # with scratch the partial sums are folded in a fixed order: the same bits on every run, and the sum of the atomics path
    nws = int(_lib.lib().fn["jp_act_bwd_bias_ws_floats"](N, C, H * W))
    dbs = []
    for _ in range(2):
        dbw = torch.full((C,), 0.25, device=DEV)
        call("jp_act_bwd_bias", dy, y, torch.empty_like(dy), dbw, N, C, H * W, act, None, torch.empty(nws, device=DEV))
        dbs.append(dbw)
    assert torch.equal(dbs[0], dbs[1])
    close(dbs[0], db, rtol=1e-5, atol=1e-5, msg="dbias with scratch vs atomics")
    nwc = int(_lib.lib().fn["jp_channel_sum_ws_floats"](N, C, H * W))
    cs = []
    for _ in range(2):
        o = torch.zeros(C, device=DEV)
        call("jp_channel_sum", dy, o, N, C, H * W, 0, torch.empty(nwc, device=DEV))
        cs.append(o)
    assert torch.equal(cs[0], cs[1])
    close(cs[0], dy.double().sum(dim=(0, 2, 3)).float(), rtol=1e-5, atol=1e-5, msg="channel_sum with scratch")
    dx2 = torch.empty_like(dy)
    call("jp_act_bwd", dy, y, dx2, dy.numel(), act, None)
    assert torch.equal(dx, dx2)
    slope = 0.01 if act == 2 else 0.0
    ref = dy.double() * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope)).double()
    close(dx, ref.float(), rtol=1e-6, atol=1e-7, msg="dx")
    close(db, (0.25 + ref.sum(dim=(0, 2, 3))).float(), rtol=1e-5, atol=1e-5, msg="dbias")


SMALL_CHANNEL_CASES = [(2, 16, 16, 64, 128, 1, 0, False),    # N, Cin, Cout, H, W, up, act, bias: BEV upconv 16 -> 16 on the upsampled map
                       (3, 16, 16, 96, 128, 0, 1, True),      # full-resolution source, bias + ReLU, 3 images
                       (1, 16, 16, 64, 64, 1, 2, True),
                       (2, 32, 32, 64, 64, 1, 1, True)]       # (32 channels: implicit-GEMM engine)


# (fp32 referee, largest error of the tensor: tests/test_smallconv_f64_gpu.py holds the direct Cout <= 4, disparity-head and 16 -> 16 kernels
# per element to float64 references on every launch path, scratch tier and ragged channel count)
@pytest.mark.parametrize("N,Cin,Cout,H,W,up,act,bias", SMALL_CHANNEL_CASES)
def test_small_channel_direct_conv(N, Cin, Cout, H, W, up, act, bias):
    """The 16 / 32-channel 3x3 zero-pad layers of the BEV decoder (layout_model.py:138-153) run on direct VALU kernels
    (conv_c16.hip): forward, input gradient (through the nearest-2x upsample where the source is stored at half resolution) and
    weight / bias gradients against ATen."""
    from tests.test_bench_shapes_gpu import kernel_tags
    h, w_ = (H // 2, W // 2) if up else (H, W)
    x = rnd(N, Cin, h, w_, seed=1)
    wt, b = rnd(Cout, Cin, 3, 3, seed=2, scale=0.1), (rnd(Cout, seed=3) if bias else None)
    xv, wv, bv = Var(x, True), pvar(wt), (pvar(b) if bias else None)
    tape = Tape()
    with recording(tape), kernel_tags() as kt:
        y = ops.conv2d(None, wv, bv, 1, 1, 0, act, srcs=[(xv, up)])
    if Cin == 16 and Cout == 16:        # the library dispatches 16 -> 16 to the direct kernels (the 32-channel layers stay on the engine)
        assert not kt.names, f"expected the direct kernels (no implicit-GEMM launch), got {kt.names}"
    xr, wr = x.detach().cpu().clone().requires_grad_(True), wt.detach().cpu().clone().requires_grad_(True)
    br = b.detach().cpu().clone().requires_grad_(True) if bias else None
    src = F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr
    yr = kink_act(F.conv2d(src, wr, br, 1, 1), y.t, act)
    close(y.t, yr, msg="fwd")
    gy = rnd(*yr.shape, seed=4)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    close(xv.g, xr.grad, rtol=2e-4, msg="dx")
    close(wv.g, wr.grad, rtol=2e-4, msg="dw")
    if bias:
        close(bv.g, br.grad, rtol=2e-4, msg="db")


def test_p1l_persistent_1x1():
    """The opt-in persistent 1x1 kernel (csrc/igemm_p1l.h, JP_P1L=1: weight stages through LDS-DMA, one sequence of stages over a
    range of tiles; layers.py:147-167 / 184-199 at the CRP shape): forward and dgrad must be BIT-IDENTICAL to the default patch
    kernel's (same pack, same products in the same order) and the profiler must name the kernel.  The switch is read once per
    process, so the two runs are subprocesses."""
    import os
    import subprocess
    from jperceiver_amd import ops as _ops
    if _ops.split_scheme() != 3:
        pytest.skip("the persistent 1x1 kernel reads the three-plane bf16 pack: only in a -DJP_NS=3 build of the library")
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys, hashlib, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tools")
from jperceiver_amd import ops
from jperceiver_amd.ops import Var, Tape, recording
from conv_bench import profiled
g = torch.Generator().manual_seed(7)
N, C, H, W, Co = 8, 256, 256, 256, 256
x = torch.randn(N, C, H, W, generator=g).cuda()
w = (torch.randn(Co, C, 1, 1, generator=g) * C ** -0.5).cuda()
gy = torch.randn(N, Co, H, W, generator=g).cuda()
xv, wv = Var(x, True), Var(w, True, torch.zeros_like(w))
tape = Tape()
def step():
    with recording(tape):
        step.y = ops.conv2d(xv, wv, None, 1, 0, 0, 0)
    step.y.g = gy
    tape.backward()
names = sorted({r[0] for r in profiled(step)})
h = hashlib.sha256(step.y.t.cpu().numpy().tobytes() + xv.g.cpu().numpy().tobytes()).hexdigest()
ref = torch.nn.functional.conv2d(x.cpu()[:1], w.cpu())
err = float((step.y.t[:1].cpu() - ref).abs().max() / ref.abs().max())
print("RESULT", h, err, "|".join(names))
''' % (ROOT, ROOT)
    out = {}
    for flag in ("0", "1"):
        env = dict(os.environ, JP_P1L=flag)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")][-1].split(" ", 3)
        out[flag] = (line[1], float(line[2]), line[3])
    assert "jp_conv1x1_p1l_kernel<FwdEpi>" in out["1"][2] and "jp_conv1x1_p1l_kernel<DgradEpi>" in out["1"][2], out["1"][2]
    assert "p1l" not in out["0"][2]
    assert out["0"][0] == out["1"][0], "the persistent 1x1 kernel's results differ from the patch kernel's"
    assert out["1"][1] < 2e-5


BN_EPILOGUE_CASES = [(8, 64, 128, 128, True),      # N, C, H, W, expect: ResNet layer1 shape class: 64-row 4-wave tiles (wide)
                     (8, 128, 64, 64, True),       # layer2: 128-row 4-wave tiles
                     (8, 64, 64, 96, True),        # regular (not wide) 64-row tiles
                     (8, 512, 32, 32, True),       # layer4: four 128-row M tiles per pixel tile (XCD-remapped ids)
                     (8, 256, 64, 128, False)]     # 256-row 8-wave tiles: no statistics epilogue -> the pass over y


@pytest.mark.parametrize("N,C,H,W,expect", BN_EPILOGUE_CASES)
def test_batchnorm_statistics_from_the_conv_epilogue(N, C, H, W, expect):
    """Round 6 (VERDICT r03-r05 "BatchNorm folded into the convolutions", resnet.py:29-45): a 3x3 convolution that feeds a train-mode
    BatchNorm leaves per-channel partial sums of y and y^2 in its epilogue (jp_conv2d_fwd* bn_stats) and jp_bn_train_fwd folds them
    instead of reading y for the statistics.  Same normalised output, saved statistics and running statistics as the two-pass form
    (fp32 partial sums in another order: 1e-6), and as float64 on the CPU."""
    x = Var(rnd(N, C, H, W, seed=11) * 1.7 + 0.2, True)
    w = Var(rnd(C, C, 3, 3, seed=12) * (9 * C) ** -0.5, True, torch.zeros(C, C, 3, 3, device=DEV))
    gamma, beta = rnd(C, seed=13) * 0.2 + 1.0, rnd(C, seed=14) * 0.1
    outs = []
    for fused in (True, False):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        with recording(Tape()):
            y = ops.conv2d(x, w, None, 1, 1, ops.PAD_ZERO, ops.ACT_NONE, bn_stats=fused)
            if fused:
                assert (y.bnst is not None) == (expect and ops.split_scheme() in (2, 3)), (y.bnst is not None, expect)
            else:
                assert y.bnst is None
            z = ops.batchnorm_train(y, Var(gamma.clone(), True, torch.zeros(C, device=DEV)), Var(beta.clone(), True, torch.zeros(C, device=DEV)),
                                    rm, rv, relu=True)
        outs.append((y.t.clone(), z.t.clone(), rm.clone(), rv.clone()))
    (y1, z1, rm1, rv1), (y0, z0, rm0, rv0) = outs
    assert torch.equal(y1, y0)                                  # the convolution's output does not depend on the extra epilogue work
    close(z1, z0, rtol=2e-5, atol=2e-5, msg="normalised output, fused statistics vs the pass over y")
    close(rm1, rm0, rtol=1e-5, atol=1e-6, msg="running mean")
    close(rv1, rv0, rtol=1e-5, atol=1e-6, msg="running var")
    yd = y0.double().cpu()
    ref = F.relu(F.batch_norm(yd, None, None, gamma.double().cpu(), beta.double().cpu(), True, 0.1, 1e-5))
    close(z1, ref.float(), rtol=1e-4, atol=1e-4, msg="vs float64 batch norm")
