"""Which route ops.conv2d takes for the weight gradient and the input gradient of a layer: the cases of tests/test_conv_routes_cpu.py
(ops._wgrad_route / ops._dgrad_route on the library's host-side queries) and tests/test_conv_routes_gpu.py (the launches at ops.call).

A case: (sources [(channels, upsampled)...], Cout, N, H, W, K, stride, pad, pad mode, wgrad kind, the query that sizes the wgrad
scratch, dgrad kind).  "one" = jp_conv2d_wgrad_ws_floats (the layer as ONE full-resolution source), "src3" =
jp_conv2d_wgrad_src3_ws_floats on the sources as they are.  The sizes themselves are the library's answers, never constants here: a
kernel change that resizes a scratch must not break a route test.

The expectations were transcribed from the branch chains conv2d's backward had before the routes became functions, evaluated against
the default (two-split) build:

  weight gradient   1. one upsampled source and jp_conv2d_up_head_ok        direct, "src3"      (disparity head)
                    2. several sources and the "src3" query > 0             direct, "src3"      (per-segment kernels)
                    3. several sources or an upsampled one, Cin >= 32       concat, "one"
                    4. one full-resolution source                           direct, "one"
                    5. otherwise (few channels)                             direct, "src3"
  input gradient    1. one full-resolution source                           single
                    2. jp_conv2d_dgrad_src3_ok                              src3
                    3. otherwise                                            concat
"""
from jperceiver_amd import _lib

R, Z = 1, 0         # reflect / zero padding

ROUTE_CASES = [
    ([(64, 0)], 64, 1, 16, 32, 3, 1, 1, R, "direct", "one", "single"),
    ([(256, 0)], 256, 1, 8, 32, 1, 1, 0, Z, "direct", "one", "single"),
    ([(3, 0)], 64, 1, 32, 64, 7, 2, 3, Z, "direct", "one", "single"),
    ([(16, 0)], 1, 1, 8, 8, 3, 1, 1, R, "direct", "one", "single"),
    ([(8, 1)], 1, 1, 4, 4, 3, 1, 1, R, "direct", "src3", "src3"),                           # step 1: the up-head kernels
    ([(8, 1)], 1, 1, 4, 4, 3, 1, 1, Z, "direct", "src3", "concat"),                         # ... zero padding: no up-head (step 5)
    ([(64, 0), (128, 1), (1, 0)], 128, 1, 4, 64, 3, 1, 1, R, "direct", "src3", "concat"),   # step 2; dgrad below the half-resolution
    ([(64, 0), (128, 1), (1, 0)], 128, 1, 192, 256, 3, 1, 1, R, "direct", "src3", "src3"),  # pixel floor of the per-source kernels, and at it
    ([(64, 0), (128, 1), (1, 0)], 64, 1, 4, 64, 3, 1, 1, R, "concat", "one", "concat"),     # step 3: no per-segment kernels for Cout = 64
    ([(64, 0), (64, 1)], 128, 1, 192, 256, 3, 1, 1, R, "concat", "one", "src3"),
    ([(128, 0), (128, 0)], 128, 1, 8, 32, 3, 1, 1, Z, "concat", "one", "concat"),
    ([(64, 1)], 32, 1, 8, 64, 3, 1, 1, Z, "concat", "one", "concat"),
    ([(16, 1)], 16, 1, 64, 64, 3, 1, 1, Z, "direct", "src3", "concat"),                     # step 5: the 16 -> 16 kernel's partial sums
    ([(16, 1)], 16, 1, 32, 64, 3, 1, 1, Z, "direct", "src3", "concat"),                     # ... a map small enough to need none
    ([(8, 0), (8, 1)], 8, 1, 8, 8, 3, 1, 1, R, "direct", "src3", "concat"),
    ([(64, 0), (128, 1), (1, 0)], 2, 1, 4, 64, 3, 1, 1, R, "direct", "src3", "concat"),     # step 2 on the small-head kernels
    TRAP := ([(64, 1)], 2, 1, 8, 8, 3, 1, 1, Z, "concat", "one", "concat"),                 # step 3 although the "src3" query is positive
]

# The cases the GPU test launches.  Shapes that the sweeps of the suite already run (tests/test_kernels_gpu.py CONV_CASES,
# DISPARITY_HEAD_CASES, FUSED_UPSAMPLE_CASES, SMALL_CHANNEL_CASES; tests/test_write_or_add_gpu.py runs all of them forward and backward):
# together they reach each of the five weight-gradient steps and the three input-gradient routes.  The CPU test holds them to the
# routes written here, like the cases above.
GPU_ROUTE_CASES = [
    ([(64, 0)], 64, 2, 16, 24, 3, 1, 1, R, "direct", "one", "single"),                      # step 4
    ([(40, 1)], 1, 2, 12, 20, 3, 1, 1, R, "direct", "src3", "src3"),                        # step 1
    ([(32, 0), (128, 1), (1, 0)], 72, 2, 32, 64, 3, 1, 1, R, "direct", "src3", "concat"),   # step 2
    ([(40, 0), (24, 1), (1, 0)], 32, 2, 12, 20, 3, 1, 1, R, "concat", "one", "concat"),     # step 3, three sources
    ([(32, 1)], 32, 2, 64, 64, 3, 1, 1, Z, "concat", "one", "concat"),                      # step 3, one upsampled source
    ([(16, 1)], 16, 2, 64, 128, 3, 1, 1, Z, "direct", "src3", "concat"),                    # step 5
]


def cu6(srcs):
    """(c0, up0, c1, up1, c2, up2) of a source list"""
    flat = [a for cu in srcs for a in cu]
    return tuple(flat + [0] * (6 - len(flat)))


def geom(case):
    """the record conv2d builds for the case's layer"""
    from jperceiver_amd import ops
    srcs, Cout, N, H, W, K, s, p, pm = case[:9]
    fill = (0,) * (3 - len(srcs))
    return ops._ConvGeom(tuple(c for c, _ in srcs) + fill, tuple(u for _, u in srcs) + fill, len(srcs), N, H, W,
                         sum(c for c, _ in srcs), Cout, K, s, p, pm, (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1)


def query(name, *ints):
    return int(_lib.lib().fn[name](*ints))


def wgrad_floats(case):
    """what the query the case names returns for it"""
    srcs, Cout, N, H, W, K, s, p, pm, _, which, _ = case
    if which == "one":
        return query("jp_conv2d_wgrad_ws_floats", N, sum(c for c, _ in srcs), H, W, Cout, K, s, p)
    return query("jp_conv2d_wgrad_src3_ws_floats", *cu6(srcs), N, H, W, Cout, K, s, p, pm)


def dgrad_floats(case):
    """(packed-weight floats, split-K floats) of the case's input-gradient route"""
    srcs, Cout, N, H, W, K, s, p, pm, _, _, kind = case
    Cin = sum(c for c, _ in srcs)
    pack = query("jp_conv2d_ws_floats", Cin, Cout, K, 1) if Cout >= 16 else 0
    if kind == "src3":
        return pack, query("jp_conv2d_dgrad_src3_split_floats", *cu6(srcs), N, H, W)
    return pack, query("jp_conv2d_dgrad_split_floats", N, Cin, H, W, Cout, K, s, p)
