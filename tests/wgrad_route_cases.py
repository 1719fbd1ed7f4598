"""Which kernel jp_conv2d_wgrad_src3 runs: one case per route of csrc/conv_wgrad.hip's wgrad_route ("Which kernel the
weight gradient runs"), at the smallest shape that reaches it.  tests/test_wgrad_routes_gpu.py launches them; tools/wgrad_query_ab.py
puts their source lists to the scratch-size queries of two libraries.

A case: (label, sources [(channels, upsampled)...], Cout, N, H, W, K, stride, pad, pad mode, expected launches, fold).

Expected launches: the profiled launches of the call in order, each a tuple of substrings that its kernel name (as bench.py prints it)
must contain.  The generic engine's name carries its tile (WM, WN), its two loaders and its epilogue: WgradEpiWS = split-K partial tiles
stored to scratch and folded in a fixed order, WgradEpiT / WgradEpi = added into dw by the epilogue's atomics.  () = a direct kernel
of conv_small.hip / conv_c16.hip, which the profiler does not tag: no tagged launch at all.

Fold: what sums the scratch into dw after the launches, one entry of FOLD_KERNELS per pass, comma-separated in launch order
(reduce4<8> from 64 slices on, wide from 32 splits of at most 2^16 outputs on; atomic = no fold kernel).  The fold kernels carry no
library tag: the test reads the names of the kernels the device ran from torch.profiler and holds their sequence to fold_kernels().
The direct kernels' cases name, in the same column, a substring of the kernel that must have run.  BITWISE marks the cases every
partial sum of which goes through scratch and a fixed-order fold: two builds of the library that differ in host code only must agree
on their dw byte for byte (tools/wgrad_dw_ab.py); the others meet in atomics and are held to the tolerance only.

Not reachable from here: the exact-fp32 twins (jp_wgrad_w9_kernel, jp_wgrad_w1_kernel, and the generic engine in place of W9S2 / W4S)
are chosen by JP_W9S=0 / JP_W9S2=0, read once per process: tools/conv_bench.py A/B runs cover them.  The channel-major multi-source arm
(several sources or an upsampled one, fewer than 32 channels): every such case of test_kernels_gpu.SMALL_CHANNEL_CASES is 16 -> 16 on
a map the direct 16 -> 16 kernels take, so the case here is the two-source 8 + 8 layer of tests/conv_route_cases.py instead.  The
multi-source table arm is FUSED_UPSAMPLE_CASES[0].
"""
R, Z = 1, 0         # reflect / zero padding


def _g(wm, wn, a, b, e):
    """generic engine, interleaved gather (IL = true): jp_igemm_kernel<WM, WN, 32, A, B, E, false, true>"""
    return (f"jp_igemm_kernel<{wm}, {wn}, 32, {a}, {b}, {e}, false, true>",)


def _w9s(tr, pm, kg, ncb):
    return (f"jp_wgrad_w9s_kernel<{tr}, {'true' if pm == R else 'false'}, {kg}, {ncb}>",)


def _refl(pm):
    return "true" if pm == R else "false"


_TABLE_WS = _g(4, 1, "WgradA", "WgradBT1<3>", "WgradEpiWS")         # 1-channel table pass of a > 64-row bank, through scratch
ICONV = [(64, 0), (128, 1), (1, 0)]

CASES = [
    # ---- slice kernels: partial sums per K slice in scratch, wgrad_reduce4_kernel folds them
    ("W1S, 16 pixel tiles (the floor), 4 slices", [(128, 0)], 192, 2, 16, 64, 1, 1, 0, Z, [("jp_wgrad_w1s_kernel",)], "reduce4<1>"),
    ("W1S, 64 slices", [(128, 0)], 192, 2, 64, 256, 1, 1, 0, Z, [("jp_wgrad_w1s_kernel",)], "reduce4<8>"),
    ("W7, 3 channels", [(3, 0)], 64, 1, 64, 128, 7, 2, 3, Z, [("jp_wgrad_w7_kernel<3>",)], "w7_reduce<3>"),
    ("W7, 6 channels", [(6, 0)], 64, 1, 64, 128, 7, 2, 3, Z, [("jp_wgrad_w7_kernel<6>",)], "w7_reduce<6>"),
    ("W9S2, KG = 2", [(32, 0)], 128, 1, 16, 128, 3, 2, 1, Z, [("jp_wgrad_w9s2_kernel<2>",)], "reduce4<1>"),
    ("W9S2, KG = 1", [(32, 0)], 256, 1, 16, 128, 3, 2, 1, Z, [("jp_wgrad_w9s2_kernel<1>",)], "reduce4<1>"),
] + [
    (f"W9S narrow, Cout = {co}, {'reflect' if pm == R else 'zero'}", [(64, 0)], co, 1, 16, 64, 3, 1, 1, pm, [_w9s(4, pm, 2, 2)], "reduce4<1>")
    for co in (64, 48) for pm in (R, Z)
] + [
    (f"W9S 128 x 64, {'reflect' if pm == R else 'zero'}", [(64, 0)], 128, 1, 8, 64, 3, 1, 1, pm, [_w9s(2, pm, 1, 2)], "reduce4<1>")
    for pm in (R, Z)
] + [
    ("W9S narrow, 32 splits of two slices each: 64 slices", [(64, 0)], 64, 1, 64, 128, 3, 1, 1, Z, [_w9s(4, Z, 2, 2)], "reduce4<8>"),
    ("W9S 256 x 32, 4-row tiles", [(64, 0)], 256, 1, 16, 64, 3, 1, 1, R, [_w9s(4, R, 1, 1)], "reduce4<1>"),
    ("W9S 256 x 32, 2-row fallback (H % 4 != 0)", [(64, 0)], 256, 1, 6, 96, 3, 1, 1, R, [_w9s(2, R, 1, 1)], "reduce4<1>"),
    ("W9S + table tail", [(129, 0)], 128, 1, 8, 64, 3, 1, 1, R, [_w9s(2, R, 1, 2), _TABLE_WS], "reduce4<1>, reduce"),
] + [
    # ---- generic engine, single source
    (f"uniform-tap, scalar-base, {'reflect' if pm == R else 'zero'}", [(128, 0)], 72, 1, 8, 24, 3, 1, 1, pm,
     [_g(2, 2, "WgradAS", f"WgradBUS<3, {_refl(pm)}>", "WgradEpiT")], "atomic")
    for pm in (R, Z)
] + [
    ("uniform-tap, scalar-base, two images: split K through scratch", [(128, 0)], 72, 2, 8, 24, 3, 1, 1, R,
     [_g(2, 2, "WgradAS", "WgradBUS<3, true>", "WgradEpiWS")], "reduce"),
    ("uniform-tap, per-element loaders (Cout % 8 != 0)", [(128, 0)], 68, 1, 8, 24, 3, 1, 1, R,
     [_g(2, 2, "WgradA", "WgradBU<3>", "WgradEpiT")], "atomic"),
    ("uniform-tap + table tail", [(129, 0)], 72, 1, 8, 24, 3, 1, 1, R,
     [_g(2, 2, "WgradAS", "WgradBUS<3, true>", "WgradEpiT"), _g(4, 1, "WgradA", "WgradBT1<3>", "WgradEpiT")], "atomic, atomic"),
] + [
    (f"BMS {ci} -> {co}, {'reflect' if pm == R else 'zero'}", [(ci, 0)], co, 1, 8, 24, 3, 1, 1, pm,
     [_g(wm, wn, "WgradAS", f"WgradBMS<3, {_refl(pm)}, {tpt}, {ci}>", "WgradEpiT")], "atomic")
    for ci, co, wm, wn, tpt in ((32, 32, 1, 4, 8), (64, 64, 1, 4, 4), (64, 72, 2, 2, 2), (16, 24, 1, 4, 16)) for pm in (R, Z)
] + [
    ("BMS 16 -> 24 at 64 x 64: 32 splits of 24 x 144 outputs", [(16, 0)], 24, 1, 64, 64, 3, 1, 1, Z,
     [_g(1, 4, "WgradAS", "WgradBMS<3, false, 16, 16>", "WgradEpiWS")], "wide"),
    ("single-source table", [(40, 0)], 24, 1, 8, 24, 3, 1, 1, R, [_g(1, 4, "WgradA", "WgradBT1<3>", "WgradEpiT")], "atomic"),
    ("single-source table at 64 x 64: 32 splits of 24 x 360 outputs through scratch, never the wide fold", [(40, 0)], 24, 1, 64, 64,
     3, 1, 1, R, [_g(1, 4, "WgradA", "WgradBT1<3>", "WgradEpiWS")], "reduce"),
    # ---- several sources
    ("multi-source table (FUSED_UPSAMPLE_CASES[0])", [(40, 0), (24, 1), (1, 0)], 32, 2, 12, 20, 3, 1, 1, R,
     [_g(1, 4, "WgradA", "WgradBT<3>", "WgradEpiT")], "atomic"),
    ("channel-major, two sources of 8 channels", [(8, 0), (8, 1)], 8, 1, 8, 8, 3, 1, 1, R,
     [_g(1, 4, "WgradA", "WgradB<3>", "WgradEpi")], "atomic"),
    # ---- per-segment calls: W9S / BMS on the skip segment's own columns, the parity-class kernels on the upsampled segment, the
    # sub-range table on the disparity channel
    ("segments at 32 x 64: W4S", ICONV, 128, 1, 32, 64, 3, 1, 1, R, [_w9s(2, R, 1, 2), ("jp_wgrad_w4s_kernel<2>",), _TABLE_WS],
     "reduce4<1>, parity, reduce"),
    ("segments at 8 x 64: two pixel tiles, below W4S's floor of 8", ICONV, 128, 1, 8, 64, 3, 1, 1, R,
     [_w9s(2, R, 1, 2), _g(2, 2, "WgradAP", "WgradBP", "WgradEpiWS"), _TABLE_WS], "reduce4<1>, parity, reduce"),
    ("segments at 6 x 64: odd half-resolution height, generic parity kernels", ICONV, 128, 1, 6, 64, 3, 1, 1, R,
     [_g(2, 2, "WgradAS", "WgradBMS<3, true, 2, 64>", "WgradEpiWS"), _g(2, 2, "WgradAP", "WgradBP", "WgradEpiWS"), _TABLE_WS],
     "reduce, parity, reduce"),
]

# the direct kernels of conv_small.hip / conv_c16.hip (their float64 tests: tests/test_smallconv_f64_gpu.py): the route only
DIRECT_CASES = [
    ("up-head", [(8, 1)], 1, 1, 4, 4, 3, 1, 1, R, [], "up_head_wgrad"),
    ("c16", [(16, 0)], 16, 1, 64, 64, 3, 1, 1, Z, [], "c16_wgrad_kernel"),
    ("small-head", [(16, 0)], 1, 1, 8, 8, 3, 1, 1, R, [], "conv_small_wgrad"),
]

# every partial sum through scratch and a fixed-order fold: byte-identical dw between two builds of the library
BITWISE = {c[0] for c in CASES if "atomic" not in c[11]}

# fold column entry -> the kernel's name as the device profiler prints it (a substring); atomic: no fold kernel
FOLD_KERNELS = {"reduce4<1>": "wgrad_reduce4_kernel<1>", "reduce4<8>": "wgrad_reduce4_kernel<8>", "reduce": "wgrad_reduce_kernel",
                "wide": "wgrad_reduce_wide_kernel", "parity": "wgrad_fold_parity_kernel", "w7_reduce<3>": "w7_reduce_kernel<3>",
                "w7_reduce<6>": "w7_reduce_kernel<6>", "atomic": None}
# every fold kernel of conv_wgrad.hip / igemm_w7.h, by the name before its template arguments
FOLD_FAMILY = ("wgrad_reduce4_kernel", "wgrad_reduce_kernel", "wgrad_reduce_wide_kernel", "wgrad_fold_parity_kernel", "w7_reduce_kernel")


def fold_kernels(case):
    """the fold kernels the case must run, in launch order"""
    return [FOLD_KERNELS[f] for f in case[11].split(", ") if FOLD_KERNELS[f]]


def query_floats(fn, case):
    """scratch floats the library asks for the case: the single-source query for one full-resolution source, the src3 query otherwise
    (fn: name -> callable, e.g. _lib.lib().fn)"""
    _, srcs, Cout, N, H, W, K, s, p, pm = case[:10]
    if len(srcs) == 1 and not srcs[0][1]:
        return int(fn["jp_conv2d_wgrad_ws_floats"](N, srcs[0][0], H, W, Cout, K, s, p))
    flat = [a for cu in srcs for a in cu]
    return int(fn["jp_conv2d_wgrad_src3_ws_floats"](*(flat + [0] * (6 - len(flat))), N, H, W, Cout, K, s, p, pm))
