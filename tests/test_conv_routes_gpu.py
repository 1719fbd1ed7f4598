"""The launches of ops.conv2d's backward, recorded at ops.call, for one layer per weight-gradient step and input-gradient route of
tests/conv_route_cases.py: which entry points run, in which order, on which source geometry and with how much scratch.  No numerics
here -- tests/test_kernels_gpu.py and tests/test_write_or_add_gpu.py check these very shapes against references."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                                                   # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                              # noqa: E402
from tests import conv_route_cases as C                                          # noqa: E402

DEV = "cuda"
MOVES = ("jp_upsample2x_fwd", "jp_copy_channels", "jp_upsample2x_bwd")
WATCHED = MOVES + ("jp_conv2d_fwd_src3", "jp_conv2d_wgrad_src3", "jp_conv2d_dgrad", "jp_conv2d_dgrad_src3")
# the last source of the three-source concat case needs no gradient: its slice of the concat's gradient is routed nowhere
NEEDS_GRAD = {3: (True, True, False)}


def _id(case):
    return f"wgrad-{case[9]}-{case[10]}-dgrad-{case[11]}-" + "+".join(f"{c}{'u' if u else ''}" for c, u in case[0])


@pytest.mark.parametrize("k", range(len(C.GPU_ROUTE_CASES)), ids=[_id(c) for c in C.GPU_ROUTE_CASES])
def test_backward_launch_pattern(k, monkeypatch):
    case = C.GPU_ROUTE_CASES[k]
    srcs, Cout, N, H, W, K, s, p, pm, wkind, _, dkind = case
    if ops.split_scheme() != 2:
        pytest.skip("the routes of the table were derived against the two-split build")
    Cin = sum(c for c, _ in srcs)
    g = torch.Generator(device=DEV).manual_seed(k)
    rg = NEEDS_GRAD.get(k, (True,) * len(srcs))
    vs = [Var(torch.randn(N, c, H >> u, W >> u, generator=g, device=DEV), rg[i]) for i, (c, u) in enumerate(srcs)]
    w = Var(torch.randn(Cout, Cin, K, K, generator=g, device=DEV) * (Cin * K * K) ** -0.5, True, torch.zeros(Cout, Cin, K, K, device=DEV))
    b = Var(torch.randn(Cout, generator=g, device=DEV), True, torch.zeros(Cout, device=DEV))
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda n, *a: (calls.append((n, a)) if n in WATCHED else None, real(n, *a))[1])
    tape = Tape()
    with recording(tape):
        y = ops.conv2d(None, w, b, s, p, pm, ops.ACT_NONE, srcs=[(v, u) for v, (_, u) in zip(vs, srcs)])
    assert [n for n, _ in calls] == ["jp_conv2d_fwd_src3"]          # nothing is materialised for the forward
    del calls[:]
    y.g = torch.randn(y.t.shape, generator=g, device=DEV)
    tape.backward()
    torch.cuda.synchronize()
    names = [n for n, _ in calls]
    print(names)

    # ---- weight gradient: first in the backward
    gather = ["jp_upsample2x_fwd" if u else "jp_copy_channels" for _, u in srcs] if wkind == "concat" else []
    assert names[:len(gather) + 1] == gather + ["jp_conv2d_wgrad_src3"]
    a = calls[len(gather)][1]
    assert (a[1], a[2], a[4], a[5], a[7], a[8]) == ((Cin, 0, 0, 0, 0, 0) if wkind == "concat" else C.cu6(srcs))
    assert a[21] == C.wgrad_floats(case) and (a[20] is not None) == (a[21] > 0)
    if wkind == "concat":
        assert a[3] is None and a[6] is None and tuple(a[0].shape) == (N, Cin, H, W)
        for (n, m), v in zip(calls, vs):                           # each source once, in source order
            assert m[0] is v.t and m[1] is a[0]

    # ---- input gradient
    rest = calls[len(gather) + 1:]
    scatter = [("jp_upsample2x_bwd" if u else "jp_copy_channels") for (_, u), need in zip(srcs, rg) if need]
    want = {"single": ["jp_conv2d_dgrad"], "src3": ["jp_conv2d_dgrad_src3"], "concat": ["jp_conv2d_dgrad"] + scatter}[dkind]
    assert [n for n, _ in rest] == want
    d = rest[0][1]
    if dkind == "single":       # (dx, accumulate, amax_dx_done: into the fresh gradient buffer, magnitude wanted)
        assert d[2] is vs[0].g and d[12] == 0 and d[18] is not None
    elif dkind == "concat":     # into a buffer of the virtual concat: written, not added to, and no magnitude slot
        assert tuple(d[2].shape) == (N, Cin, H, W) and d[12] == 0 and d[17] is None and d[18] is None
        for (n, m), v in zip(rest[1:], [v for v, need in zip(vs, rg) if need]):
            assert m[0] is d[2] and m[1] is v.g
    else:
        assert (d[3], d[4], d[7], d[8], d[11], d[12]) == C.cu6(srcs)
        assert [d[2] is not None, d[6] is not None, d[10] is not None] == [i < len(srcs) and rg[i] for i in range(3)]
    for v, need in zip(vs, rg):
        assert (v.g is not None) == need
