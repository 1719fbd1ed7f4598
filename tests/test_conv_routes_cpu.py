"""ops._wgrad_route / ops._dgrad_route on the cases of tests/conv_route_cases.py, without a GPU: the route functions take the layer's
geometry and ask the library's host-side queries only (the library loads without a device, tests/test_abi.py), so which shape takes
which route is pinned where every pull request runs.  Kinds are asserted as written in the table; sizes as "what the named query
returns for these arguments"."""
import pytest

from jperceiver_amd import ops
from tests import conv_route_cases as C

pytestmark = pytest.mark.skipif(C.query("jp_split_scheme") != 2, reason="the table was derived against the two-split build")

ALL = C.ROUTE_CASES + C.GPU_ROUTE_CASES


def _id(case):
    srcs, Cout, N, H, W, K, s, p, pm = case[:9]
    return "+".join(f"{c}{'u' if u else ''}" for c, u in srcs) + f"-{Cout}-{N}x{H}x{W}-k{K}s{s}p{p}{'RZ'[pm == C.Z]}"


@pytest.mark.parametrize("case", ALL, ids=[_id(c) for c in ALL])
def test_routes_of_the_table(case):
    g = C.geom(case)
    assert ops._wgrad_route(g) == (case[9], C.wgrad_floats(case))
    assert ops._dgrad_route(g) == (case[11], *C.dgrad_floats(case))


def test_table_reaches_every_branch():
    """each of the five weight-gradient steps and the three input-gradient routes, in the table and in the GPU subset"""
    def step(case):
        srcs, kind, which = case[0], case[9], case[10]
        if kind == "concat":
            return 3
        if which == "one":
            return 4
        if len(srcs) > 1:
            return 2 if C.wgrad_floats(case) > 0 else 5
        Cout, N, H, W, K, s, p, pm = case[1:9]
        return 1 if C.query("jp_conv2d_up_head_ok", *srcs[0], 0, 0, Cout, K, s, p, pm, H, W) else 5

    for table in (C.ROUTE_CASES, C.GPU_ROUTE_CASES):
        assert {step(c) for c in table} == {1, 2, 3, 4, 5}
        assert {c[11] for c in table} == {"single", "src3", "concat"}


def test_one_upsampled_source_is_not_asked_the_segment_question():
    """Steps 1, 2 and 5 are not "direct wherever the src3 query is positive": for one upsampled 64-channel source it is positive, and
    the layer still takes the concat route, because step 2 asks only for several sources."""
    srcs, Cout, N, H, W, K, s, p, pm = C.TRAP[:9]
    assert C.query("jp_conv2d_wgrad_src3_ws_floats", *C.cu6(srcs), N, H, W, Cout, K, s, p, pm) > 0
    assert ops._wgrad_route(C.geom(C.TRAP))[0] == "concat"


@pytest.mark.parametrize("c0", [8, 768])
def test_up_head_scratch_is_never_empty(c0):
    """conv2d allocates the route's scratch only when the query is positive; over the up-head predicate's channel range it is"""
    assert C.query("jp_conv2d_up_head_ok", c0, 1, 0, 0, 1, 3, 1, 1, C.R, 4, 4)
    assert C.query("jp_conv2d_wgrad_src3_ws_floats", c0, 1, 0, 0, 0, 0, 1, 4, 4, 1, 3, 1, 1, C.R) > 0


def test_geometry_record():
    g = C.geom(([(64, 0), (128, 1), (1, 0)], 128, 2, 4, 64, 3, 1, 1, C.R))
    assert g.cu == (64, 0, 128, 1, 1, 0) and g.big and not g.single and (g.OH, g.OW) == (4, 64)
    assert g.sig == ((64, 128, 1), (0, 1, 0), 2, 4, 64, 1, 1, C.R)
    c = g.concat()
    assert c.cu == (193, 0, 0, 0, 0, 0) and c.single and c[3:] == g[3:]
    assert not C.geom(([(16, 1)], 16, 1, 8, 8, 3, 1, 1, C.Z)).single and not C.geom(([(16, 0)], 64, 1, 8, 8, 3, 1, 1, C.Z)).big
