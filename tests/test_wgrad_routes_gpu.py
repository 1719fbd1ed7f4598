"""jp_conv2d_wgrad_src3 at one shape per kernel route (tests/wgrad_route_cases.py): the profiled launches must be the route's, in
order, the fold kernels that sum the scratch into dw must be the route's (untagged: their names come from torch.profiler's record of
what the device ran), and dw must match a float64 CPU convolution gradient -- written with the scratch the library's query asks for
over a NaN-filled dw, and added (accumulate = 1) onto a non-zero dw.  Tolerance: `close` of tests/test_kernels_gpu.py at rtol 2e-4, as
every weight-gradient comparison of that file.  The test asks nothing of the host code's shape: it passes unedited against the library
of the commit before the routes became one function (JP_LIB_PATH)."""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops, _lib                                            # noqa: E402
from tests import wgrad_route_cases as C                                        # noqa: E402
from tests.test_bench_shapes_gpu import kernel_tags                             # noqa: E402
from tests.test_kernels_gpu import rnd, close                                   # noqa: E402


def _operands(case):
    _, srcs, Cout, N, H, W, K, s, p, pm = case[:10]
    xs = [rnd(N, c, H >> u, W >> u, seed=11 + i) for i, (c, u) in enumerate(srcs)]
    dy = rnd(N, Cout, (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1, seed=7)
    return xs, dy


@functools.lru_cache(maxsize=None)
def _reference(k):
    """float64 dw of CASES[k] on the CPU, from the operands the test uploads"""
    case = C.CASES[k]
    _, srcs, Cout, N, H, W, K, s, p, pm = case[:10]
    xs, dy = _operands(case)
    x = torch.cat([F.interpolate(t, scale_factor=2, mode="nearest") if u else t for t, (_, u) in zip(xs, srcs)], 1).double().cpu()
    if pm == C.R and p:
        x, p = F.pad(x, (p, p, p, p), mode="reflect"), 0
    return torch.nn.grad.conv2d_weight(x, (Cout, x.shape[1], K, K), dy.double().cpu(), stride=s, padding=p)


class device_kernels:
    """with device_kernels() as dk: ...  -> dk.names = names of the kernels the device ran inside, in the order they started"""

    def __enter__(self):
        self.prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA])
        self.prof.__enter__()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.prof.__exit__(*exc)
        ev = [e for e in self.prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        self.names = [e.name for e in sorted(ev, key=lambda e: e.time_range.start)]
        return False


def _wgrad(case, xs, dy, dw, accumulate):
    """one call as ops.conv2d's backward makes it, with the scratch the query asks for; -> (tagged kernel names, names of all the
    kernels the device ran)"""
    _, srcs, Cout, N, H, W, K, s, p, pm = case[:10]
    L = _lib.lib()
    nws = C.query_floats(L.fn, case)
    ws = torch.empty(nws, device=dy.device) if nws else None
    amax_ws = torch.empty(int(L.fn["jp_conv2d_amax_ws_floats"]()), device=dy.device)
    src = []
    for i in range(3):
        src += [xs[i], srcs[i][0], srcs[i][1]] if i < len(srcs) else [None, 0, 0]
    with device_kernels() as dk, kernel_tags() as kt:
        _lib.call("jp_conv2d_wgrad_src3", *src, dy, dw, N, H, W, Cout, K, s, p, pm, accumulate, ws, nws, None, None, None, None, amax_ws)
    return kt.names, dk.names


def _check_launches(ran, case, what):
    names, device = ran
    want, folds = case[10], C.fold_kernels(case)
    print(what, names, device)
    assert len(names) == len(want) and all(all(s in n for s in w) for n, w in zip(names, want)), \
        f"{what}: expected the launches {want}, the library made {names}"
    got = [n for n in device if any(re.search(rf"\b{f}\b", n) for f in C.FOLD_FAMILY)]
    assert len(got) == len(folds) and all(f in n for n, f in zip(got, folds)), \
        f"{what}: expected the fold kernels {folds}, the device ran {got} (of {device})"


def _two_split():
    if ops.split_scheme() != 2:
        pytest.skip("the routes of the table were derived against the two-split build")


@pytest.mark.parametrize("k", range(len(C.CASES)), ids=[c[0] for c in C.CASES])
def test_wgrad_route(k):
    _two_split()
    case = C.CASES[k]
    label, srcs, Cout = case[:3]
    K = case[6]
    xs, dy = _operands(case)
    ref = _reference(k)
    dw = torch.full((Cout, sum(c for c, _ in srcs), K, K), float("nan"), device=dy.device)      # accumulate = 0 must overwrite it
    _check_launches(_wgrad(case, xs, dy, dw, 0), case, label)
    print("max abs err", float((dw.double().cpu() - ref).abs().max()), "scale", float(ref.abs().max()))
    close(dw, ref, rtol=2e-4, msg="dw")
    # a gradient already there, of the gradient's own size: a dropped or doubled add shifts every element by about its own magnitude
    seed = rnd(*dw.shape, seed=5) * float(ref.pow(2).mean().sqrt())
    dw = seed.clone()
    _check_launches(_wgrad(case, xs, dy, dw, 1), case, label + " (accumulate)")
    close(dw, ref + seed.double().cpu(), rtol=2e-4, msg="dw, accumulated")


@pytest.mark.parametrize("k", range(len(C.DIRECT_CASES)), ids=[c[0] for c in C.DIRECT_CASES])
def test_direct_kernel_route(k):
    _two_split()
    case = C.DIRECT_CASES[k]
    xs, dy = _operands(case)
    dw = torch.full((case[2], sum(c for c, _ in case[1]), case[6], case[6]), float("nan"), device=dy.device)
    names, device = _wgrad(case, xs, dy, dw, 0)
    print(case[0], names, device)
    assert not names, f"{case[0]}: expected the direct kernels (no implicit-GEMM launch), got {names}"
    assert any(case[11] in n for n in device), f"{case[0]}: expected a {case[11]} kernel, the device ran {device}"
    assert not any(f in n for n in device for f in C.FOLD_FAMILY + ("jp_igemm", "jp_wgrad")), f"{case[0]}: the device ran {device}"
    assert bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0, f"{case[0]}: dw was not written"
