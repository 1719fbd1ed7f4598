"""Parity at the EXACT shapes bench.py's step issues (B = 8, 1024^2, BASELINE.json configs[1]) -- VERDICT r02 "weak" item 1.

Every tile / split decision of the conv engine depends on N*H*W (8-wave P9 tiles "when the launch keeps >= 256
workgroups", W9 tiles_per_split, the split-K cost model, small-grid splits), so the kernel unit cases of
tests/test_kernels_gpu.py (<= 8x256x32x32) do not take the dispatch plans the benchmark times.  Here:

  * the by-time top conv instantiations of profiles/r0*_kernel_stats_bench_b8_1024.md run at the (N, C, H, W) the step
    issues them with, against ATen evaluated ON THE CPU (rtol 2e-4 of the tensor's max), and the test asserts through the
    library's own profile tags (jp_profile_*) that the intended kernel instantiation is the one that ran;
  * HBM-bound kernels (BatchNorm 8x64x512^2, 5x5 max-pool 8x256x256^2) at their largest bench shape;
  * configs[2] / configs[3] per-GPU batches (12 and 24 images at 1024^2) run one full step each and are held to a
    size-independent property instead of the oracle: a batch made of k copies of a 4-image batch has the same BatchNorm
    statistics, the same per-item outputs, the same mean losses and the same gradients as the 4-image batch itself --
    while N = 12 / 24 takes different tile / split-K plans than N = 4.  (configs[1]'s own B = 8 step is checked against the
    oracle in tests/test_config_steps_gpu.py::test_config_step[cfg1_full_B8_1024].)
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops, _lib                                            # noqa: E402
from jperceiver_amd import synthetic as syn                                     # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                             # noqa: E402
from tests.test_kernels_gpu import rnd, close, kink_act, pvar                   # noqa: E402


class kernel_tags:
    """with kernel_tags() as kt: ...  -> kt.names = rocprofv3-style names of the igemm kernels launched inside."""

    def __enter__(self):
        L = _lib.lib()
        if L.fn["jp_profile_begin"](256) != 0:
            raise RuntimeError(L.last_error())
        self.names = []
        return self

    def __exit__(self, *exc):
        import bench
        L = _lib.lib()
        torch.cuda.synchronize()
        n = L.fn["jp_profile_end"]()
        buf, fl, ms = ctypes.create_string_buffer(512), ctypes.c_double(), ctypes.c_float()
        for i in range(n):
            rc = L.fn["jp_profile_get"](i, ctypes.cast(buf, ctypes.c_void_p), 512, ctypes.cast(ctypes.pointer(fl), ctypes.c_void_p),
                                        ctypes.cast(ctypes.pointer(ms), ctypes.c_void_p))
            assert rc == 0, L.last_error()
            self.names.append(bench._kernel_name(buf.value.decode()))
        return False


def _split_name(w):
    """Names of the split-bf16 twins the library launches for the same tiles unless JP_P9S / JP_W9S / JP_P9US = 0:
    jp_igemm_p9_kernel<WM, WN, REFLECT, REV, Epi, TAPS, CPB> -> jp_igemm_p9s_kernel<WM, WN, 2, REFLECT, REV, Epi, TAPS, KGS>
    (igemm_p9s.h), the wide W9 -> jp_wgrad_w9s_kernel<TR, REFLECT> (igemm_w9s.h), P9U -> P9US2 (igemm_p9us2.h)."""
    import os
    import re
    mw = re.fullmatch(r"jp_wgrad_w9_kernel<2, 2, 1, (\w+)>", w)
    if mw is not None and os.environ.get("JP_W9S", "1") != "0":
        # NCB = 2 (128 x 64-channel tiles, 2-row pixel tiles) or, round 4, 1 (256 x 32 channels, 4-row pixel tiles unless JP_W9S_TR1=2)
        return (f"jp_wgrad_w9s_kernel<2, {mw.group(1)}, 1, ", f"jp_wgrad_w9s_kernel<4, {mw.group(1)}, 1, 1>")
    mn = re.fullmatch(r"jp_wgrad_w9_kernel<1, 2, 2, (\w+)>", w)
    if mn is not None and os.environ.get("JP_W9S", "1") != "0":
        return f"jp_wgrad_w9s_kernel<4, {mn.group(1)}, 2, 2>"         # narrow twin: two K groups per workgroup
    if w == "jp_wgrad_w1_kernel" and os.environ.get("JP_W9S", "1") != "0":
        return "jp_wgrad_w1s_kernel"
    if w.startswith("SM<"):                                          # small-map split-bf16 patch kernel (conv_p9sm.hip); JP_P9SM=0 / JP_P9S=0: generic engine
        on = os.environ.get("JP_P9S", "1") != "0" and os.environ.get("JP_P9SM", "1") != "0"
        return "jp_igemm_p9sm_kernel<" + w[3:].rstrip(">") if on else "jp_igemm_kernel"
    if w.startswith("STEM<"):                                        # 7x7 stem forward: P7S (igemm_p7s.h) or the generic engine's FwdBC
        on = os.environ.get("JP_P9S2", "1") != "0" and os.environ.get("JP_P9S", "1") != "0"
        return f"jp_igemm_p7s_kernel<{w[5]}" if on else ("FwdBC<7, 4>" if w[5] == "3" else "FwdBC<7, 8>")
    if w.startswith("W9S2<"):                                        # stride-2 3x3 weight gradient: igemm_w9s2.h (round 4) or the generic engine
        on = os.environ.get("JP_W9S2", "1") != "0" and os.environ.get("JP_W9S", "1") != "0"
        return f"jp_wgrad_w9s2_kernel<{w[5]}>" if on else "jp_igemm_kernel"
    if w == "S2F":                                                   # stride-2 forward: patch kernel (igemm_p9s2f.h) or the generic engine
        on = os.environ.get("JP_P9S2", "1") != "0" and os.environ.get("JP_P9S", "1") != "0"
        return "jp_igemm_p9s2f_kernel" if on else "jp_igemm_kernel"
    if w == "DgradS2B" and os.environ.get("JP_P9S2", "1") != "0" and os.environ.get("JP_P9S", "1") != "0":
        return "jp_igemm_p9s2d_kernel"                                # class-uniform stride-2 dgrad (igemm_p9s2d.h)
    if w == "WgradAP, WgradBP" and os.environ.get("JP_W9S", "1") != "0":
        return "jp_wgrad_w4s_kernel<2>"                               # parity-class wgrad of the upsampled segment (igemm_w4s.h)
    if w == "jp_igemm_p9u_kernel<FwdEpi>" and os.environ.get("JP_P9US", "1") != "0":
        return "jp_igemm_p9us2_kernel<FwdEpi>"             # igemm_p9us2.h (round 5: the re-laid instruction stream)
    m = re.fullmatch(r"jp_igemm_p9_kernel<(\d), (\d), (\w+), (\w+), (\w+), (\d), \d>", w)
    if m is None or os.environ.get("JP_P9S", "1") == "0":
        return w
    taps = m.group(6)
    if taps == "1" and m.group(1) == "4" and os.environ.get("JP_P1L", "0") == "1":
        # opt-in (round 5): the persistent 1x1 kernel (igemm_p1l.h) where every CU gets >= 8 tiles, the patch kernel elsewhere
        return (f"jp_conv1x1_p1l_kernel<{m.group(5)}>", f"jp_igemm_p9s_kernel<4, 2, 2, false, false, {m.group(5)}, 1, 2>")
    tile = int(os.environ.get("JP_P9_TILE", "3"))
    if taps == "9" and ((m.group(1) == "4" and tile >= 1) or (m.group(1) == "2" and tile >= 2) or (m.group(1) == "1" and tile >= 3)):
        # round 4: 8x32-pixel "wide" tiles where H % 8 == 0 and they still give >= 256 workgroups, the 4x32 ones elsewhere
        return (f"jp_igemm_p9s_wide_kernel<{m.group(1)}, {m.group(2)}, {m.group(3)}, {m.group(4)}, {m.group(5)}, 9, 1>",
                f"jp_igemm_p9s_kernel<{m.group(1)}, {m.group(2)}, 2, {m.group(3)}, {m.group(4)}, {m.group(5)}, 9, 1>")
    return f"jp_igemm_p9s_kernel<{m.group(1)}, {m.group(2)}, 2, {m.group(3)}, {m.group(4)}, {m.group(5)}, {taps}, {1 if taps == '9' else 2}>"


def _expect(names, wanted, what):
    for w in map(_split_name, wanted):
        alts = w if isinstance(w, tuple) else (w,)
        assert any(a in n for a in alts for n in names), f"{what}: expected a launch of {alts!r}, the library launched {sorted(set(names))}"


# (label, (N, Cin, H, W, Cout, K, stride, pad, pad_mode, act, bias), expected kernels fwd / dgrad / wgrad)
BENCH_CONV = [
    ("merge 256->256 3x3 reflect @256^2 (decoder merge1 / iconv skip segment)",
     (8, 256, 256, 256, 256, 3, 1, 1, 1, 2, True),
     ["jp_igemm_p9_kernel<4, 2, true, false, FwdEpi, 9, 1>"],
     ["jp_igemm_p9_kernel<4, 2, false, true, DgradEpi, 9, 1>"],
     ["jp_wgrad_w9_kernel<2, 2, 1, true>"]),
    ("merge 256->256 3x3 reflect @128^2", (8, 256, 128, 128, 256, 3, 1, 1, 1, 2, True),
     ["jp_igemm_p9_kernel<4, 2, true, false, FwdEpi, 9, 1>"],
     ["jp_igemm_p9_kernel<4, 2, false, true, DgradEpi, 9, 1>"],
     ["jp_wgrad_w9_kernel<2, 2, 1, true>"]),
    ("CRP / reduce 256->256 1x1 @256^2", (8, 256, 256, 256, 256, 1, 1, 0, 0, 0, False),
     ["jp_igemm_p9_kernel<4, 2, false, false, FwdEpi, 1, 2>"],
     ["jp_igemm_p9_kernel<4, 2, false, false, DgradEpi, 1, 2>"],
     ["jp_wgrad_w1_kernel"]),
    ("reduce1 64->256 1x1 @256^2", (8, 64, 256, 256, 256, 1, 1, 0, 0, 0, False), ["jp_igemm"], ["jp_igemm"], ["jp_"]),
    ("ResNet layer1 64->64 3x3 zero pad @256^2", (8, 64, 256, 256, 64, 3, 1, 1, 0, 0, False),
     ["jp_igemm_p9_kernel<1, 4, false, false, FwdEpi, 9, 1>"],
     ["jp_igemm_p9_kernel<1, 4, false, true, DgradEpi, 9, 1>"],
     ["jp_wgrad_w9_kernel<1, 2, 2, false>"]),
    ("ResNet layer2 128->128 3x3 @128^2", (8, 128, 128, 128, 128, 3, 1, 1, 0, 0, False),
     ["jp_igemm_p9_kernel<2, 2, false, false, FwdEpi, 9, 1>"],
     ["jp_igemm_p9_kernel<2, 2, false, true, DgradEpi, 9, 1>"],
     ["jp_wgrad_w9_kernel<2, 2, 1, false>"]),
    ("ResNet layer3 256->256 3x3 @64^2", (8, 256, 64, 64, 256, 3, 1, 1, 0, 0, False),
     ["jp_igemm_p9"], ["jp_igemm_p9"], ["jp_wgrad_w9_kernel<2, 2, 1, false>"]),
    ("ResNet layer4 512->512 3x3 @32^2", (8, 512, 32, 32, 512, 3, 1, 1, 0, 0, False),
     ["jp_igemm_p9_kernel<2, 2, false, false, FwdEpi, 9, 1>"],
     ["jp_igemm_p9_kernel<2, 2, false, true, DgradEpi, 9, 1>"],
     ["jp_wgrad_w9_kernel<2, 2, 1, false>"]),
    ("ResNet layer2.0 64->128 3x3 stride 2 @256^2", (8, 64, 256, 256, 128, 3, 2, 1, 0, 0, False),
     ["S2F"], ["DgradS2B"], ["W9S2<2>"]),
    ("ResNet layer3.0 128->256 3x3 stride 2 @128^2", (8, 128, 128, 128, 256, 3, 2, 1, 0, 0, False),
     ["S2F"], ["DgradS2B"], ["W9S2<1>"]),
    ("ResNet layer4.0 256->512 3x3 stride 2 @64^2", (8, 256, 64, 64, 512, 3, 2, 1, 0, 0, False),
     ["jp_igemm"], ["jp_igemm"], ["W9S2<1>"]),
    ("downsample 64->128 1x1 stride 2 @256^2", (8, 64, 256, 256, 128, 1, 2, 0, 0, 0, False), ["jp_igemm"], ["jp_igemm"], ["jp_igemm"]),
    ("stem 3->64 7x7 stride 2 @1024^2", (8, 3, 1024, 1024, 64, 7, 2, 3, 0, 0, False),
     ["STEM<3>"], [], ["jp_wgrad_w7_kernel<3>"]),
    ("pose stem 6->64 7x7 stride 2 @192x640 (both pairs stacked: N = 16)", (16, 6, 192, 640, 64, 7, 2, 3, 0, 0, False),
     ["STEM<6>"], [], ["jp_wgrad_w7_kernel<6>"]),
    ("pose encoder layer1 64->64 3x3 @48x160, N = 16", (16, 64, 48, 160, 64, 3, 1, 1, 0, 0, False), ["jp_igemm"], ["jp_igemm"], ["jp_"]),
    # small maps (conv_p9sm.hip, round 4): partial tiles masked, reduction split over grid.z when the tile grid is small
    ("pose encoder layer2 128->128 3x3 @24x80, N = 16 (W % 32 != 0: masked tiles)", (16, 128, 24, 80, 128, 3, 1, 1, 0, 0, False),
     ["SM<2, 2, false, false, SmFwdEpi, 9>"], ["SM<2, 2, false, true, SmDgradEpi, 9>"], ["jp_"]),
    ("pose encoder layer3 256->256 3x3 @12x40, N = 16", (16, 256, 12, 40, 256, 3, 1, 1, 0, 0, False),
     ["SM<2, 2, false, false, Sm"], ["SM<2, 2, false, true, Sm"], ["jp_"]),
    ("pose encoder layer4 512->512 3x3 @6x20, N = 16 (small grid: split K, H % 4 != 0)", (16, 512, 6, 20, 512, 3, 1, 1, 0, 0, False),
     ["SM<2, 2, false, false, SmSliceEpi, 9>"], ["SM<2, 2, false, true, SmSliceEpi, 9>"], ["jp_"]),
    ("pose decoder squeeze 512->256 1x1 @6x20, N = 16", (16, 512, 6, 20, 256, 1, 1, 0, 0, 1, True),
     ["SM<2, 2, false, false, SmSliceEpi, 1>"], ["SM<2, 2, false, false, SmSliceEpi, 1>"], ["jp_"]),
    ("BEV decoder 128->64 3x3 @64^2", (8, 128, 64, 64, 64, 3, 1, 1, 0, 0, True), ["jp_igemm"], ["jp_igemm"], ["jp_"]),
    ("layout encoder conv1 512->128 3x3 reflect @32^2 (64 tiles: split K)", (8, 512, 32, 32, 128, 3, 1, 1, 1, 0, True),
     ["SM<2, 2, true, false, SmSliceEpi, 9>"], ["jp_igemm_p9"], ["jp_"]),
    ("layout encoder conv2 128->128 3x3 reflect @16^2 (W < 32)", (8, 128, 16, 16, 128, 3, 1, 1, 1, 0, True),
     ["SM<2, 2, true, false, SmSliceEpi, 9>"], ["SM<2, 2, false, true, SmSliceEpi, 9>"], ["jp_"]),
    ("CCT 128->256 3x3 @8x8 (a quarter of a 4x32 tile: stays on the generic engine)", (8, 128, 8, 8, 256, 3, 1, 1, 0, 0, True),
     ["jp_igemm_kernel"], ["jp_igemm_kernel"], ["jp_"]),
    ("BEV 256->64 3x3 @32^2 (64-row tiles, 8x32 pixels)", (8, 256, 32, 32, 64, 3, 1, 1, 0, 1, True),
     ["SM<1, 4, false, false, SmSliceEpi, 9>"], ["SM<2, 2, false, true, Sm"], ["jp_"]),
    ("CCT value conv 256->256 1x1 @32^2", (8, 256, 32, 32, 256, 1, 1, 0, 0, 0, True), ["SM<2, 2, false, false, Sm"], ["SM<2, 2, false, "], ["jp_"]),
    ("odd map 64->96 3x3 reflect @13x37, N = 3 (every edge partial; accumulate into dx)", (3, 64, 13, 37, 96, 3, 1, 1, 1, 2, True),
     ["SM<2, 2, true, false, Sm"], ["SM<1, 4, false, true, Sm"], ["jp_"]),
]


@pytest.mark.parametrize("label,case,k_fwd,k_dgrad,k_wgrad", BENCH_CONV, ids=[c[0] for c in BENCH_CONV])
def test_conv_at_bench_shape(label, case, k_fwd, k_dgrad, k_wgrad):
    N, Cin, H, W, Cout, K, s, p, pm, act, bias = case
    x = rnd(N, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, K, K, seed=2, scale=(Cin * K * K) ** -0.5)
    b = rnd(Cout, seed=3) if bias else None
    needs_dx = Cin > 6                                   # the stems read images: no input gradient in the step
    xv, wv = Var(x, needs_dx), pvar(w)
    bv = pvar(b) if bias else None
    tape = Tape()
    with recording(tape), kernel_tags() as kt:
        y = ops.conv2d(xv, wv, bv, s, p, pm, act)
    _expect(kt.names, k_fwd, label + " forward")
    xr = x.detach().cpu().clone().requires_grad_(needs_dx)
    wr = w.detach().cpu().clone().requires_grad_(True)
    br = b.detach().cpu().clone().requires_grad_(True) if bias else None
    xi = F.pad(xr, (p, p, p, p), mode="reflect") if pm == 1 else xr
    yr = kink_act(F.conv2d(xi, wr, br, s, 0 if pm == 1 else p), y.t, act)
    close(y.t, yr, rtol=2e-4, msg="fwd")
    gy = rnd(*yr.shape, seed=4)
    y.g = gy.clone()
    yr.backward(gy.cpu())
    R = None
    if "accumulate into dx" in label:
        # a second consumer's gradient already sits in dx: seeded, of the gradient's own size (a dropped or doubled add shifts every
        # element by about its own magnitude)
        R = rnd(*x.shape, seed=5) * float(xr.grad.pow(2).mean().sqrt())
        xv.g = R.clone()
    was = ops._WG_ON
    ops._WG_ON = False
    try:
        with kernel_tags() as kt:
            tape.backward()
    finally:
        ops._WG_ON = was
    _expect(kt.names, k_dgrad + k_wgrad, label + " backward")
    if needs_dx:
        close(xv.g, xr.grad if R is None else xr.grad + R.cpu(), rtol=2e-4, msg="dgrad")
    close(wv.g, wr.grad, rtol=2e-4, msg="wgrad")
    if bias:
        close(bv.g, br.grad, rtol=2e-4, msg="bias grad")


ICONV_BENCH_CASES = [(8, 256, 256, 256, 256, 256),     # N, H, W, Cr, Cx, Cout -- iconv1: cat(reduce1, up(x2), disp2) @256^2
                     (8, 128, 128, 256, 256, 256),     # iconv2 @128^2
                     (8, 64, 64, 256, 256, 256)]       # iconv3 @64^2


@pytest.mark.parametrize("N,H,W,Cr,Cx,Cout", ICONV_BENCH_CASES)
def test_iconv_at_bench_shape(N, H, W, Cr, Cx, Cout):
    """iconv_k(cat(reduce_k, up2x(x_{k+1}), disp_{k+1})) -> 256, reflect + leaky (depth_decoder.py:76-77), the three largest
    convolutions of the step: P9U forward, per-source dgrad (P9 on the skip segment, parity-class on the upsampled one),
    per-source wgrad."""
    r, xh, d = rnd(N, Cr, H, W, seed=1), rnd(N, Cx, H // 2, W // 2, seed=2), rnd(N, 1, H, W, seed=3)
    w, b = rnd(Cout, Cr + Cx + 1, 3, 3, seed=4, scale=(9 * (Cr + Cx + 1)) ** -0.5), rnd(Cout, seed=5)
    rv, xv, dv, wv, bv = Var(r, True), Var(xh, True), Var(d, True), pvar(w), pvar(b)
    tape = Tape()
    with recording(tape), kernel_tags() as kt:
        y = ops.conv2d(None, wv, bv, 1, 1, 1, 2, srcs=[(rv, 0), (xv, 1), (dv, 0)])
    _expect(kt.names, ["jp_igemm_p9u_kernel<FwdEpi>"], "iconv forward")
    leaves = [t.detach().cpu().clone().requires_grad_(True) for t in (r, xh, d, w, b)]
    cat = torch.cat((leaves[0], F.interpolate(leaves[1], scale_factor=2, mode="nearest"), leaves[2]), 1)
    yr = kink_act(F.conv2d(F.pad(cat, (1, 1, 1, 1), mode="reflect"), leaves[3], leaves[4]), y.t, 2)
    del cat
    close(y.t, yr, rtol=2e-4, msg="fwd")
    gy = rnd(*yr.shape, seed=6)
    y.g = gy.clone()
    was = ops._WG_ON
    ops._WG_ON = False
    try:
        with kernel_tags() as kt:
            tape.backward()
    finally:
        ops._WG_ON = was
    # skip segment: P9 dgrad on the 128-row tiles of the 513-row bank's pack + reflection border pass; upsampled segment:
    # parity-class dgrad at half resolution (+ its edge pass); wgrad per source (W9 on the skip segment, parity-class
    # kernels on the upsampled one, table pass for the disparity channel)
    _expect(kt.names, ["jp_igemm_p9_kernel<2, 2, false, true, DgradEpi, 9, 1>", "DgradBorderB<3>",
                       "jp_wgrad_w9_kernel<2, 2, 1, true>", "WgradAP, WgradBP"], "iconv backward")
    if H >= 128:      # at 64^2 the half-resolution (32^2) dgrad of the upsampled segment takes the tap-major path instead
        import os
        _expect(kt.names, ["jp_igemm_p9sd_kernel<DgradEpi>" if os.environ.get("JP_P9SD", "1") != "0" else "DgradUPB", "DgradUPBorderB"],
                "iconv backward, upsampled segment")
    yr.backward(gy.cpu())
    for got, ref, nm in zip((rv.g, xv.g, dv.g, wv.g, bv.g), leaves, ("d_reduce", "d_x_half", "d_disp", "dw", "db")):
        close(got, ref.grad, rtol=2e-4, msg=nm)


def test_batchnorm_at_bench_shape():
    """bn1 of both ResNet stems at the bench shape (8 x 64 x 512^2: the largest BatchNorm of the step), train mode + ReLU."""
    N, C, H, W = 8, 64, 512, 512
    x = rnd(N, C, H, W, seed=1) * 2 + 0.5
    g, b = rnd(C, seed=2) * 0.2 + 1, rnd(C, seed=3) * 0.1
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    xv, gv, bv = Var(x, True), pvar(g), pvar(b)
    tape = Tape()
    with recording(tape):
        y = ops.batchnorm_train(xv, gv, bv, rm, rv, None, True, 0.1, 1e-5, 1)
    xr, gr, br = (t.detach().cpu().clone().requires_grad_(True) for t in (x, g, b))
    rm2, rv2 = torch.zeros(C), torch.ones(C)
    yr = F.relu(F.batch_norm(xr, rm2, rv2, gr, br, True, 0.1, 1e-5))
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


def test_crp_at_bench_shape():
    """One CRP stage at the stage-1 decoder shape (8 x 256 x 256^2): 5x5 max-pool (row-streaming kernel) -> 1x1 -> add,
    forward and backward with the first-maximum tie rule (layers.py:184-199)."""
    N, C, H, W = 8, 256, 256, 256
    x = torch.round(rnd(N, C, H, W, seed=1) * 4) / 4            # many exact ties
    xv = Var(x, True)
    tape = Tape()
    with recording(tape):
        y = ops.maxpool(xv, 5, 1, 2)
    xr = x.detach().cpu().clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 5, 1, 2)
    close(y.t, yr, rtol=0, atol=0)
    gy = rnd(*yr.shape, seed=2)
    y.g = gy.clone()
    tape.backward()
    yr.backward(gy.cpu())
    close(xv.g, xr.grad, rtol=1e-6)


# ------------------------------------------------------------------------------------------- configs[2] / [3] batches
def _tiled_step(k, base_B=4, HW=1024, loss_sum=3, ty="static", split="odometry"):
    from jperceiver_amd.model import MONO
    from jperceiver_amd.apis import build_optimizer, change_input_variable
    from oracle import jp_oracle as J            # only default_opt (the option dict); nothing of the oracle is evaluated here
    FR = [0, -1, 1]
    B = base_B * k
    opt = J.default_opt(frame_ids=FR, imgs_per_gpu=B, height=HW, width=HW, occ_map_size=HW // 4, type=ty, split=split,
                        loss_sum=loss_sum)
    model = MONO.module_dict["Baseline"](opt)
    model.load_state_dict(syn.synth_state_dict(model.state_dict(), seed=0), strict=True)
    model = model.cuda().train()
    inp = syn.make_batch(base_B, HW, HW, FR, HW // 4, (375, 1242), split, seed=31)
    masks = syn.make_dropout_masks(base_B, HW, HW, seed=31)
    noise = syn.make_automask_noise(base_B, HW, HW, 4, 2, seed=31)
    rep = lambda t: torch.cat([t] * k, 0) if k > 1 else t                      # noqa: E731
    d = change_input_variable({kk: rep(v) for kk, v in inp.items()}, opt=model.opt)
    d[("dropout_mask", 0)], d[("dropout_mask", 1)] = rep(masks[0]).cuda(), rep(masks[1]).cuda()
    for s, per in enumerate(noise):
        for j, nz in enumerate(per):
            d[("automask_noise", s, j)] = rep(nz).cuda()
    optim = build_optimizer(model, dict(type="Adam", lr=1e-4, weight_decay=0))
    optim.zero_grad()
    out, losses = model(d)
    total = losses.total()
    total.backward()
    torch.cuda.synchronize()
    res = dict(losses={kk: float(v) for kk, v in losses.items()}, total=float(total),
               grads={n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()},
               disp=[out[("disp", 0, s)].detach().cpu() for s in range(4)],
               topview=out["topview"].detach().cpu(), pose=out[("cam_T_cam", 0, -1)].detach().cpu(),
               min_index=[out[("min_index", s)].detach().cpu() for s in range(4)])
    del model, optim, out, losses, total, d
    torch.cuda.empty_cache()
    return res


@pytest.fixture(scope="module")
def base_step():
    return {}


@pytest.mark.parametrize("k,loss_sum,ty,split", [(3, 1, "static", "odometry"),           # configs[2]: 12 images / GPU, loss_sum 1
                                                 (6, 0, "static_eigen", "eigen")])       # configs[3]: 24 images / GPU, eigen split
def test_config_batch_tiling_invariance(k, loss_sum, ty, split, base_step):
    key = (loss_sum, ty, split)
    if key not in base_step:
        base_step[key] = _tiled_step(1, loss_sum=loss_sum, ty=ty, split=split)
    a, b = base_step[key], _tiled_step(k, loss_sum=loss_sum, ty=ty, split=split)
    B0 = 4
    assert np.isfinite(b["total"])
    assert set(a["losses"]) == set(b["losses"])
    for kk in a["losses"]:
        x, y = b["losses"][kk], a["losses"][kk]
        assert abs(x - y) <= 1e-3 * max(abs(y), 1e-4), (kk, x, y)
    for s in range(4):
        for c in range(k):
            got = b["disp"][s][c * B0:(c + 1) * B0]
            assert float((got - a["disp"][s]).abs().max() / a["disp"][s].abs().max()) < 1e-3, ("disp", s, c)
            agree = float((b["min_index"][s][c * B0:(c + 1) * B0] == a["min_index"][s]).float().mean())
            assert agree > 0.998, ("min_index", s, c, agree)
    for c in range(k):
        assert float((b["topview"][c * B0:(c + 1) * B0] - a["topview"]).abs().max() / a["topview"].abs().max()) < 1e-3
        np.testing.assert_allclose(b["pose"][c * B0:(c + 1) * B0].numpy(), a["pose"].numpy(), atol=1e-4)
    bad = []
    for n, ga in a["grads"].items():
        gb = b["grads"][n]
        rn = float(ga.norm())
        err = float((gb - ga).norm())
        # discrete selections (automask arg-min, CCT arg-max) are free-running on both sides: same band as the oracle tests
        tol = 8e-2 if ga.numel() == 1 else 4e-2 if ("query_conv" in n or "key_conv" in n) else 2e-2
        if err > tol * rn + 2e-5 * abs(a["total"]):
            bad.append((n, err, rn))
    assert not bad, f"{len(bad)} gradients differ between the 4-image batch and its {k}-fold tiling: {bad[:6]}"
