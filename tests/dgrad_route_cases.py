"""Which kernel jp_conv2d_dgrad / jp_conv2d_dgrad_src3 runs: one case per route of csrc/conv_dgrad.hip's dgrad_route and
dgrad_src3_route ("Which kernel the input gradient runs"), at the smallest shape that reaches it.
tests/test_dgrad_routes_gpu.py launches them; tools/dgrad_ab.py puts them to two builds of the library.

A case: (label, sources [(channels, upsampled)...], Cout, N, H, W, K, stride, pad, pad mode, ws, split_ws, expected launches, folds,
amax).  One full-resolution source = jp_conv2d_dgrad, anything else = jp_conv2d_dgrad_src3.  ws / split_ws: whether the call gets the
pack scratch (jp_conv2d_ws_floats) and the split scratch (the entry point's *_split_floats query; a case that asks for it must be
given a non-zero figure).

Expected launches: the profiled launches of the call in order, each a tuple of substrings that its kernel name (as bench.py prints
it) must contain.  The generic engine's name carries its two loaders and its epilogue: WgradEpiWS = K slices stored to scratch and
folded in a fixed order, AtomicEpi = K slices added into dx by atomics, DgradBorderEpi / DgradEdgeEpi = the read-modify-write epilogue
of the reflection border / upsample edge pass (atomics where its K loop is split).  The direct kernels of conv_c16.hip / conv_small.hip
carry no tag.

Folds: the fold kernels the device must run, in order (FOLD_FAMILY; their names come from torch.profiler).  amax: the call reports
max |dx| (of the first source) into its amax_dx slot and sets the done flag; the P9 / P1 patch kernels' epilogues do, the other
kernels do not, a row tail keeps the slot from being offered, and a border pass through the read-modify-write epilogue withdraws the
report.  (A reflection layer's slot is an upper bound in general, the main pass's value of a border pixel being in it as well as the
folded one; at the shapes here the largest element is not such a pixel and the slot is held to equality.)

The launch, fold and amax columns were filled from a run against the library of the commit before the routes became one function.
ATOMIC: the cases some partial sum of which meets in atomics; the others must replay byte for byte from their own pack
(ws_state = 1) and between two builds that differ in host code only (tools/dgrad_ab.py).

Not reachable from here: the exact-fp32 twins (JP_P9S=0), the generic forms behind JP_P9S2D / JP_P1S2 / JP_P9SD / JP_P9SM = 0, and
the row-tile kernel without a row tail in the single-source entry point (JP_P9SM takes every such shape at the default setting;
tests/test_write_or_add_gpu.py runs it in a child process): the switches are read once per process.
"""
R, Z = 1, 0         # reflect / zero padding


def _g(a, b, e):
    """generic engine: jp_igemm_kernel<WM, WN, 32, A, B, E, ...>"""
    return ("jp_igemm_kernel<", f", {a}, {b}, {e}")


def _p9(wm, wn, taps=9, rev="true"):
    """P9S patch kernel, narrow or wide tiles: ...<WM, WN, [2,] false, REV, DgradEpi, TAPS, KGS>"""
    return ("jp_igemm_p9s_", f"kernel<{wm}, {wn}, ", f"false, {rev}, DgradEpi, {taps}, ")


def _sm(wm, wn, epi, taps=9, rev="true"):
    return (f"jp_igemm_p9sm_kernel<{wm}, {wn}, false, {rev}, {epi}, {taps}>",)


_BORDER_WS = _g("PackA", "DgradBorderB<3>", "WgradEpiWS")
_BORDER_RMW = _g("PackA", "DgradBorderB<3>", "DgradBorderEpi")
_EDGE_WS = _g("PackA", "DgradUPBorderB", "WgradEpiWS")
_EDGE_RMW = _g("PackA", "DgradUPBorderB", "DgradEdgeEpi")
ICONV = [(64, 0), (128, 1), (1, 0)]
ICONV128 = [(128, 0), (128, 1), (1, 0)]

CASES = [
    # ---- jp_conv2d_dgrad
    ("C16", [(16, 0)], 16, 1, 64, 64, 3, 1, 1, Z, True, False, [], "", False),
    ("P9S2D <1, 4>", [(64, 0)], 16, 1, 128, 384, 3, 2, 1, Z, True, False, [("jp_igemm_p9s2d_kernel<1, 4, 2, DgradEpi>",)], "", False),
    ("P9S2D <2, 2>", [(128, 0)], 16, 1, 64, 384, 3, 2, 1, Z, True, False, [("jp_igemm_p9s2d_kernel<2, 2, 2, DgradEpi>",)], "", False),
    ("P1S2", [(512, 0)], 64, 1, 64, 384, 1, 2, 0, Z, True, False,
     [("jp_igemm_p9s_kernel<2, 2, 2, false, false, DgradS2PointEpi, 1, 2>",)], "", False),
    ("S2_PARITY", [(16, 0)], 16, 1, 32, 32, 3, 2, 1, Z, True, False, [_g("PackAS2", "DgradS2B", "DgradS2Epi")], "", False),
    ("P9SM, one split, zero pad", [(64, 0)], 32, 1, 8, 24, 3, 1, 1, Z, True, False, [_sm(1, 4, "SmDgradEpi")], "", False),
    ("P9SM, one split, reflect: border pass in two atomic slices", [(64, 0)], 32, 1, 8, 24, 3, 1, 1, R, True, False,
     [_sm(1, 4, "SmDgradEpi"), _BORDER_RMW], "", False),
    ("P9SM, two splits, reflect: border pass through scratch", [(64, 0)], 64, 1, 8, 24, 3, 1, 1, R, True, True,
     [_sm(1, 4, "SmSliceEpi"), _BORDER_WS], "slice_reduce, border_add", False),
    ("SPLIT_ATOMIC, reflect: the same call without split_ws, border pass read-modify-write", [(64, 0)], 64, 1, 8, 24, 3, 1, 1, R,
     True, False, [_g("PackA", "DgradBT<3>", "AtomicEpi"), _BORDER_RMW], "", False),
    ("SPLIT_SCRATCH", [(64, 0)], 64, 1, 12, 40, 3, 2, 1, Z, True, True, [_g("PackA", "DgradBT<3>", "WgradEpiWS")],
     "slice_reduce", False),
    ("SPLIT_ATOMIC", [(64, 0)], 64, 1, 12, 40, 3, 2, 1, Z, True, False, [_g("PackA", "DgradBT<3>", "AtomicEpi")], "", False),
    ("P1", [(256, 0)], 64, 1, 64, 512, 1, 1, 0, Z, True, False, [_p9(4, 2, taps=1, rev="false")], "", True),
    ("P9, zero pad: no tap-major pack", [(128, 0)], 32, 1, 64, 384, 3, 1, 1, Z, True, False, [_p9(2, 2)], "", True),
    ("P9, reflect: border pass through scratch", [(128, 0)], 64, 1, 64, 384, 3, 1, 1, R, True, True, [_p9(2, 2), _BORDER_WS],
     "border_add", True),
    ("P9, reflect, without split_ws: border pass read-modify-write", [(128, 0)], 64, 1, 64, 384, 3, 1, 1, R, True, False,
     [_p9(2, 2), _BORDER_RMW], "", False),
    ("P9 + tail, reflect", [(129, 0)], 32, 1, 64, 384, 3, 1, 1, R, True, True,
     [_p9(2, 2), _g("PackA", "DgradBT<3, true>", "DgradEpi"), _BORDER_RMW], "", False),
    ("ROW_TILE + tail", [(129, 0)], 32, 1, 8, 128, 3, 1, 1, Z, True, False,
     [("jp_igemm_r3_kernel<2, 2, ", "PackA, FwdBR3<false, true, 128>, DgradEpi"), _g("PackA", "DgradBT<3, true>", "DgradEpi")], "", False),
    ("TAP, stride 1, + tail", [(129, 0)], 24, 1, 8, 24, 3, 1, 1, Z, True, False,
     [_g("PackA", "DgradBT<3, true>", "DgradEpi"), _g("PackA", "DgradBT<3, true>", "DgradEpi")], "", False),
    ("TAP, 7x7 stride 2", [(3, 0)], 64, 1, 128, 384, 7, 2, 3, Z, True, False, [_g("PackA", "DgradBT<7>", "DgradEpi")], "", False),
    ("CHANNEL_MAJOR, Cout < 16", [(16, 0)], 8, 1, 8, 8, 3, 1, 1, Z, True, False, [_g("DgradA<3>", "DgradB<3>", "DgradEpi")], "", False),
    ("CHANNEL_MAJOR, no pack scratch", [(128, 0)], 32, 1, 64, 384, 3, 1, 1, R, False, False,
     [_g("DgradA<3>", "DgradB<3>", "DgradEpi")], "", False),
    # ---- jp_conv2d_dgrad_src3
    ("segments: TAP, generic upsampled arm, SMALL; edge pass through scratch", ICONV, 128, 1, 128, 384, 3, 1, 1, R, True, True,
     [_g("PackA", "DgradBT<3, true>", "DgradEpi"), _BORDER_WS, _g("PackA", "DgradUPB", "DgradEpi"), _EDGE_WS, _BORDER_WS],
     "border_add, edge_add, border_add", False),
    ("segments: the same without split_ws", ICONV, 128, 1, 128, 384, 3, 1, 1, R, True, False,
     [_g("PackA", "DgradBT<3, true>", "DgradEpi"), _BORDER_RMW, _g("PackA", "DgradUPB", "DgradEpi"), _EDGE_RMW, _BORDER_RMW], "", False),
    ("segments: P9SD at two images", ICONV, 128, 2, 128, 384, 3, 1, 1, R, True, True,
     [_g("PackA", "DgradBT<3, true>", "DgradEpi"), _BORDER_WS, ("jp_igemm_p9sd_kernel<DgradEpi>",), _EDGE_WS, _BORDER_WS],
     "border_add, edge_add, border_add", False),
    ("segments: ROW_TILE on the skip segment (W % 256 == 0)", ICONV, 128, 1, 192, 256, 3, 1, 1, R, True, True,
     [("jp_igemm_r3_kernel<1, 4, ", "PackA, FwdBR3<false, true, 256>, DgradEpi"), _BORDER_WS, _g("PackA", "DgradUPB", "DgradEpi"),
      _EDGE_WS, _BORDER_WS], "border_add, edge_add, border_add", False),
    ("segments: P9 on a 128-channel skip segment at offset 0", ICONV128, 128, 1, 128, 384, 3, 1, 1, R, True, True,
     [_p9(2, 2), _BORDER_WS, _g("PackA", "DgradUPB", "DgradEpi"), _EDGE_WS, _BORDER_WS], "border_add, edge_add, border_add", True),
    ("up-head", [(8, 1)], 1, 1, 4, 4, 3, 1, 1, R, False, False, [], "", False),
]

# some partial sum meets in atomics: held to the tolerance only, listed (not held) by tools/dgrad_ab.py
ATOMIC = {c[0] for c in CASES if "AtomicEpi" in str(c[12])} | {
    "P9SM, one split, reflect: border pass in two atomic slices", "P9, reflect, without split_ws: border pass read-modify-write",
    "P9 + tail, reflect", "segments: the same without split_ws"}

# fold column entry -> the kernel's name as the device profiler prints it
FOLD_KERNELS = {"slice_reduce": "slice_reduce_nchw_kernel", "border_add": "border_add_kernel", "edge_add": "edge_add_kernel"}
FOLD_FAMILY = tuple(FOLD_KERNELS.values())


def fold_kernels(case):
    return [FOLD_KERNELS[f] for f in case[13].split(", ") if f]


def single(case):
    """the case goes to jp_conv2d_dgrad (one full-resolution source) rather than jp_conv2d_dgrad_src3"""
    return len(case[1]) == 1 and not case[1][0][1]


def cu6(srcs):
    flat = [a for cu in srcs for a in cu]
    return flat + [0] * (6 - len(flat))


def scratch_floats(fn, case):
    """(floats of the pack scratch, floats of split_ws) the library's queries ask for the case (fn: name -> callable)"""
    _, srcs, Cout, N, H, W, K, s, p, pm = case[:10]
    Cin = sum(c for c, _ in srcs)
    pack = int(fn["jp_conv2d_ws_floats"](Cin, Cout, K, 1))
    if single(case):
        return pack, int(fn["jp_conv2d_dgrad_split_floats"](N, Cin, H, W, Cout, K, s, p))
    return pack, int(fn["jp_conv2d_dgrad_src3_split_floats"](*cu6(srcs), N, H, W))
