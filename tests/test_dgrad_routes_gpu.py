"""jp_conv2d_dgrad / jp_conv2d_dgrad_src3 at one shape per kernel route (tests/dgrad_route_cases.py).  Per case: the profiled
launches are the route's, in order; the fold kernels the device ran (untagged: their names come from torch.profiler) are the route's;
dx written over a NaN-filled buffer, from a NaN-filled pack scratch and split scratch, matches a float64 CPU gradient (autograd
through F.conv2d over an explicit reflect pad, nearest upsample and concat), and so does dx added (accumulate = 1) onto a seed of the
gradient's own RMS; a second call that replays the pack the first one left (ws_state = 1) gives the same bytes, where no partial sum
meets in atomics; and the call reports max |dx| exactly where the case's column says so, and not at all elsewhere.  Tolerance: `close`
of tests/test_kernels_gpu.py at rtol 2e-4, as tests/test_bench_shapes_gpu.py holds dgrad to.  The test asks nothing of the host
code's shape: it passes unedited against the library of the commit before the routes became one function (JP_LIB_PATH)."""
import ctypes
import functools
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops, _lib                                            # noqa: E402
from tests import dgrad_route_cases as C                                        # noqa: E402
from tests.test_bench_shapes_gpu import kernel_tags                             # noqa: E402
from tests.test_kernels_gpu import rnd, close                                   # noqa: E402
from tests.test_wgrad_routes_gpu import device_kernels                          # noqa: E402


def _operands(case):
    _, srcs, Cout, N, H, W, K, s, p, pm = case[:10]
    Cin = sum(c for c, _ in srcs)
    w = rnd(Cout, Cin, K, K, seed=2, scale=(Cin * K * K) ** -0.5)
    dy = rnd(N, Cout, (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1, seed=7)
    return w, dy


@functools.lru_cache(maxsize=None)
def _reference(k):
    """float64 dx per source of CASES[k] on the CPU, from the operands the test uploads (k: the first case of that geometry)"""
    case = C.CASES[k]
    _, srcs, Cout, N, H, W, K, s, p, pm = case[:10]
    w, dy = _operands(case)
    xs = [torch.zeros(N, c, H >> u, W >> u, dtype=torch.float64, requires_grad=True) for c, u in srcs]
    x = torch.cat([F.interpolate(t, scale_factor=2, mode="nearest") if u else t for t, (_, u) in zip(xs, srcs)], 1)
    if pm == C.R and p:
        x, p = F.pad(x, (p, p, p, p), mode="reflect"), 0
    F.conv2d(x, w.double().cpu(), None, s, p).backward(dy.double().cpu())
    return [t.grad for t in xs]


def run_case(case, w, dy, dxs, accumulate, ws, ws_state):
    """one call with the scratch the library's queries ask for -> (tagged kernel names, names of all kernels the device ran, done
    flag, amax slot).  ws: the pack scratch (None: the case runs without); split_ws is NaN-filled where the case gets one."""
    _, srcs, Cout, N, H, W, K, s, p, pm = case[:10]
    L = _lib.lib()
    nsp = C.scratch_floats(L.fn, case)[1]
    assert not case[11] or nsp > 0, f"{case[0]}: the case wants split_ws and the query asks for none"
    sp = torch.full((nsp,), float("nan"), device=dy.device) if case[11] else None
    amax_ws = torch.empty(int(L.fn["jp_conv2d_amax_ws_floats"]()), device=dy.device)
    slot, done = torch.zeros(int(L.fn["jp_amax_slot_floats"]()), device=dy.device), ctypes.c_int(-1)
    with device_kernels() as dk, kernel_tags() as kt:
        if C.single(case):
            _lib.call("jp_conv2d_dgrad", dy, w, dxs[0], N, srcs[0][0], H, W, Cout, K, s, p, pm, accumulate, ws, ws_state, sp, None, slot,
                      ctypes.addressof(done), amax_ws)
        else:
            args = []
            for i in range(3):
                args += [dxs[i], srcs[i][0], srcs[i][1], accumulate] if i < len(srcs) else [None, 0, 0, 0]
            _lib.call("jp_conv2d_dgrad_src3", dy, w, *args, N, H, W, Cout, K, s, p, pm, ws, ws_state, sp, None, slot,
                      ctypes.addressof(done), amax_ws)
    return kt.names, dk.names, done.value, float(slot.max())


def pack_scratch(case, dev):
    return torch.full((C.scratch_floats(_lib.lib().fn, case)[0],), float("nan"), device=dev) if case[10] else None


def _check_route(ran, case, dx0, what):
    names, device, done, slot = ran
    want, folds = case[12], C.fold_kernels(case)
    got = [n for n in device if any(re.search(rf"\b{f}\b", n) for f in C.FOLD_FAMILY)]
    mx = float(dx0.abs().max())
    print("ROUTE", what, "| tags", names, "| folds", got, "| done", done, "slot", slot, "max|dx|", mx)
    assert len(names) == len(want) and all(all(s in n for s in w) for n, w in zip(names, want)), \
        f"{what}: expected the launches {want}, the library made {names}"
    assert len(got) == len(folds) and all(f in n for n, f in zip(got, folds)), \
        f"{what}: expected the fold kernels {folds}, the device ran {got} (of {device})"
    assert done == (1 if case[14] else 0), f"{what}: amax_dx done flag {done}"
    if case[14]:
        assert slot == mx, f"{what}: the amax_dx slot holds {slot}, max |dx| is {mx}"


@pytest.mark.parametrize("k", range(len(C.CASES)), ids=[c[0] for c in C.CASES])
def test_dgrad_route(k):
    if ops.split_scheme() != 2:
        pytest.skip("the routes of the table were derived against the two-split build")
    case = C.CASES[k]
    label, srcs, N, H, W = case[0], case[1], case[3], case[4], case[5]
    w, dy = _operands(case)
    refs = _reference(next(i for i, c in enumerate(C.CASES) if c[1:10] == case[1:10]))
    ws = pack_scratch(case, dy.device)
    dxs = [torch.full((N, c, H >> u, W >> u), float("nan"), device=dy.device) for c, u in srcs]       # accumulate = 0 must overwrite it
    _check_route(run_case(case, w, dy, dxs, 0, ws, 0), case, dxs[0], label)
    for i, (dx, ref) in enumerate(zip(dxs, refs)):
        print(f"dx{i} max abs err", float((dx.double().cpu() - ref).abs().max()), "scale", float(ref.abs().max()))
        close(dx, ref, rtol=2e-4, msg=f"dx{i}")
    if label not in C.ATOMIC:
        # the pack the first call left, replayed
        again = [torch.full_like(dx, float("nan")) for dx in dxs]
        _check_route(run_case(case, w, dy, again, 0, ws, 1 if ws is not None else 0), case, again[0], label + " (replay)")
        for i, (a, dx) in enumerate(zip(again, dxs)):
            assert torch.equal(a, dx), f"{label}: dx{i} replayed from the pack differs from the first call's"
    # a gradient already there, of the gradient's own size: a dropped or doubled add shifts every element by about its own magnitude
    seeds = [rnd(*ref.shape, seed=5 + i) * float(ref.pow(2).mean().sqrt()) for i, ref in enumerate(refs)]
    dxs = [sd.clone() for sd in seeds]
    _check_route(run_case(case, w, dy, dxs, 1, pack_scratch(case, dy.device), 0), case, dxs[0], label + " (accumulate)")
    for i, (dx, ref, sd) in enumerate(zip(dxs, refs, seeds)):
        close(dx, ref + sd.double().cpu(), rtol=2e-4, msg=f"dx{i}, accumulated")
