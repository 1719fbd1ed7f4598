"""The three kernels of csrc/depthbev.hip through ops.call (and `DepthBev` on top of them), against the float64 numpy restatement in
tests/depthbev_ref.py.  Every comparison is np.array_equal: the header pins the lift's arithmetic operation by operation, each
rounded once, and integer add / min / max do not depend on any order.  Every case runs with both forms of the lift kernel
(JP_DEPTH_BEV_RUNS = 0: per-lane atomics, 1: wave-level run aggregation; the library reads the switch at every call).

Shapes are the smallest at which the kernels can still go wrong: 24 x 200 images (the width is no multiple of the 64 lanes, runs
of equal cells cross wave and row boundaries) of two cameras with different intrinsics and planes, occ 16 and 32; a 1 x 1 image;
64 x 256 pixels in ONE cell; cells alternating lane by lane; NaN inside runs; runs of exactly 64 and of 65 lanes, on and off a
wave boundary.  Every output is a slice out of the middle of a larger buffer of canary values that must survive, and starts out
poisoned (0x7f bytes) where the kernel has to overwrite it."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                                     # noqa: E402
from jperceiver_amd.apis import DepthBev, agreement_scores         # noqa: E402
from tests import depthbev_ref as R                                # noqa: E402

DEV = "cuda"
PAD = 4096
CANARY = {torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5, torch.float32: 12345.0}
POISON = {torch.int32: 0x7F7F7F7F, torch.uint8: 0x7F, torch.float32: 3.3961775e38}      # 0x7f in every byte
RANGE = dict(off=0.27, min_range=1.0, max_range=40.0, h_min=-1.0, h_max=3.0, obst_h=0.3)


@pytest.fixture(params=["0", "1"], ids=["lanes", "runs"])
def form(request, monkeypatch):
    monkeypatch.setenv("JP_DEPTH_BEV_RUNS", request.param)
    return request.param


def _guarded(n, dtype, init=None):
    """-> (whole buffer, the n elements in its middle): canaries on both sides, the middle poisoned or holding `init`"""
    buf = torch.full((n + 2 * PAD,), CANARY[dtype], dtype=dtype, device=DEV)
    mid = buf[PAD:PAD + n]
    if init is None:
        mid.fill_(POISON[dtype])
    else:
        mid.copy_(torch.as_tensor(init, dtype=dtype).reshape(-1))
    return buf, mid


def _canaries_alive(buf, n):
    c = CANARY[buf.dtype]
    return bool((buf[:PAD] == c).all()) and bool((buf[PAD + n:] == c).all())


def _lift(depth, cam, occ, accumulate=False, times=1, init=None, **kw):
    """depth (B,H,W) float32, cam (B,8) float64 (numpy) -> (kernel grid, reference grid) as (B,4,occ,occ) numpy"""
    B, H, W = depth.shape
    a = {**RANGE, **kw}
    n = B * 4 * occ * occ
    buf, grid = _guarded(n, torch.int32, init)
    d, c = torch.from_numpy(depth).to(DEV), torch.from_numpy(cam).to(DEV)
    for _ in range(times):
        ops.call("jp_depth_bev_lift", d, c, grid, B, H, W, occ, 40.0 / occ, a["off"], a["min_range"], a["max_range"], a["h_min"],
                 a["h_max"], a["obst_h"], 1 if accumulate else 0)
    torch.cuda.synchronize()
    assert _canaries_alive(buf, n)
    want = R.empty_grid(B, occ) if init is None else np.array(init, dtype=np.int32).reshape(B, 4, occ, occ)
    for _ in range(times):
        R.lift(want, depth, cam, occ, 40.0 / occ, accumulate=accumulate, **a)
    return grid.cpu().numpy().reshape(B, 4, occ, occ), want


def _keys(depth, cam, occ, **kw):
    a = {**RANGE, **kw}
    a.pop("obst_h")
    return R.keys(depth, cam, occ, 40.0 / occ, **a)


def _longest_run(keys):
    """longest run of equal accepted keys among consecutive pixels in memory order"""
    k = keys.reshape(-1)
    best = cur = 0
    for i in range(k.size):
        cur = 0 if k[i] < 0 else (cur + 1 if i > 0 and k[i] == k[i - 1] else 1)
        best = max(best, cur)
    return best


def _cams():
    """two cameras: a level one and one pitched 6 degrees down, with other intrinsics"""
    a = math.radians(6.0)
    return np.array([[100.3, 98.7, 99.5, 4.25, 0.0, 1.0, 0.0, 1.73],
                     [71.0, 64.0, 103.0, 2.0, 0.01, math.cos(a), math.sin(a), 1.6]], dtype=np.float64)


def _scene(H=24, W=200, seed=0):
    """(2,H,W) float32: camera 0 sees its ground plane with two boxes on it and sky; camera 1 ground + noise, NaN / Inf / 0 / negative
    sprinkled in"""
    rng = np.random.default_rng(seed)
    cams = _cams()
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for fx, fy, cx, cy, nx, ny, nz, h in cams:
        den = nx * (u - cx) / fx + ny * (v - cy) / fy + nz
        with np.errstate(all="ignore"):
            out.append(np.where(den > 1e-3, h / np.where(den > 1e-3, den, 1.0), np.inf))
    d0, d1 = out
    d0[6:20, 30:70] = np.minimum(d0[6:20, 30:70], 12.5)
    d0[3:22, 120:131] = np.minimum(d0[3:22, 120:131], 7.0)
    d1 = d1 * rng.uniform(0.9, 1.1, size=d1.shape)
    bad = rng.random(d1.shape)
    d1[bad < 0.02] = np.nan
    d1[(bad >= 0.02) & (bad < 0.03)] = np.inf
    d1[(bad >= 0.03) & (bad < 0.04)] = 0.0
    d1[(bad >= 0.04) & (bad < 0.05)] = -3.0
    return np.stack([d0, d1]).astype(np.float32), cams


@pytest.mark.parametrize("occ", [16, 32])
def test_two_cameras_24x200(form, occ):
    depth, cams = _scene()
    got, want = _lift(depth, cams, occ)
    assert np.array_equal(got, want)
    assert got[0, 0].sum() > 1000 and got[1, 0].sum() > 1000 and got[0, 1].sum() > 0 and not np.array_equal(got[0], got[1])
    keys = _keys(depth, cams, occ).reshape(-1)
    last, first = keys[63:-1:64], keys[64::64]                             # the two sides of every wave boundary
    assert _longest_run(keys) > 16 and ((last == first) & (last >= 0)).sum() > 20      # runs go on across wave boundaries
    # the camera rows matter: swapped, the grids differ
    swapped, _ = _lift(depth, cams[::-1].copy(), occ)
    assert not np.array_equal(swapped, got)
    # other ranges and another offset
    got2, want2 = _lift(depth, cams, occ, off=1.9, max_range=15.0, h_max=1.0, obst_h=0.1, min_range=3.0)
    assert np.array_equal(got2, want2) and 0 < got2[:, 0].sum() < got[:, 0].sum()


def test_one_pixel(form):
    cam = np.array([[64.0, 64.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.73]])
    got, want = _lift(np.full((1, 1, 1), 10.0, dtype=np.float32), cam, 16)
    assert np.array_equal(got, want)
    assert got[0, :, 11, 8].tolist() == [1, 1, 1730, 1730] and got[0, 0].sum() == 1
    got, want = _lift(np.full((1, 1, 1), np.nan, dtype=np.float32), cam, 16)
    assert np.array_equal(got, want) and np.array_equal(got, R.empty_grid(1, 16))


def test_every_pixel_in_one_cell(form):
    cam = np.array([[1e5, 1e5, -1000.0, 32.0, 0.0, 1.0, 0.0, 1.0]])
    rng = np.random.default_rng(1)
    depth = rng.uniform(10.0, 10.5, size=(1, 64, 256)).astype(np.float32)
    got, want = _lift(depth, cam, 16)
    assert np.array_equal(got, want)
    assert got[0, 0].sum() == got[0, 0].max() == 16384 and got[0, 1].max() == 16384
    assert got[0, 2].min() < got[0, 3].max()


def test_cells_alternating_lane_by_lane(form):
    cam = np.array([[1e5, 1e5, -1000.0, 12.0, 0.0, 1.0, 0.0, 1.0]] * 2)
    depth = np.empty((2, 24, 200), dtype=np.float32)
    depth[:, :, 0::2], depth[:, :, 1::2] = 10.0, 20.0
    depth[1] += 5.0
    keys = _keys(depth, cam, 16)
    assert _longest_run(keys) == 1 and (keys >= 0).all()
    got, want = _lift(depth, cam, 16)
    assert np.array_equal(got, want)
    assert sorted(got[0, 0][got[0, 0] > 0].tolist()) == [2400, 2400]


def test_rejected_pixels_inside_runs(form):
    cam = np.array([[1e5, 1e5, -1000.0, 12.0, 0.0, 1.0, 0.0, 1.0]])
    rng = np.random.default_rng(2)
    depth = rng.uniform(10.0, 10.5, size=(1, 24, 200)).astype(np.float32)
    hole = rng.random(depth.shape) < 0.1
    hole[0, 0, [0, 1, 63, 64, 65, 127, 199]] = True                         # at a wave's first and last lanes, at a row's end
    depth[hole] = np.nan
    got, want = _lift(depth, cam, 16)
    assert np.array_equal(got, want)
    assert got[0, 0].sum() == got[0, 0].max() == int((~hole).sum())
    assert 1 < _longest_run(_keys(depth, cam, 16)) < 64


@pytest.mark.parametrize("lead", [0, 7, 63])
def test_runs_of_64_and_65(form, lead):
    # one image row in memory order: `lead` rejected pixels, 64 pixels over one cell, 65 over the next, the rest over a third
    cam = np.array([[1e5, 1e5, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0]])
    W = 256
    depth = np.full((1, 1, W), 30.0, dtype=np.float32)
    depth[0, 0, :lead] = np.nan
    depth[0, 0, lead:lead + 64] = 10.0
    depth[0, 0, lead + 64:lead + 129] = 20.0
    depth[0, 0, lead + 129:] += np.linspace(0.0, 0.5, W - lead - 129, dtype=np.float32)
    got, want = _lift(depth, cam, 16)
    assert np.array_equal(got, want)
    assert sorted(got[0, 0][got[0, 0] > 0].tolist()) == sorted([64, 65, W - lead - 129])


def test_accumulate_overwrite_and_repeatability(form):
    depth, cams = _scene(seed=3)
    once, want1 = _lift(depth, cams, 16)
    assert np.array_equal(once, want1)
    # accumulate onto an empty grid twice: 2 n, 2 n_obst, the same extremes
    twice, want2 = _lift(depth, cams, 16, accumulate=True, times=2, init=R.empty_grid(2, 16))
    assert np.array_equal(twice, want2)
    assert np.array_equal(twice[:, :2], 2 * once[:, :2]) and np.array_equal(twice[:, 2:], once[:, 2:])
    # ... and onto what another scene left
    other, _ = _lift(_scene(seed=4)[0], cams, 16)
    both, wantb = _lift(depth, cams, 16, accumulate=True, init=other)
    assert np.array_equal(both, wantb) and np.array_equal(both[:, 0], once[:, 0] + other[:, 0])
    assert np.array_equal(both[:, 2], np.minimum(once[:, 2], other[:, 2])) and np.array_equal(both[:, 3], np.maximum(once[:, 3], other[:, 3]))
    # accumulate = 0 twice equals once, from a poisoned buffer and from a used one; two runs give the same bits
    again, _ = _lift(depth, cams, 16, times=2)
    used, _ = _lift(depth, cams, 16, init=other)
    assert np.array_equal(again, once) and np.array_equal(used, once)


def test_both_forms_give_the_same_grid(monkeypatch):
    depth, cams = _scene(seed=5)
    grids = []
    for f in ("0", "1"):
        monkeypatch.setenv("JP_DEPTH_BEV_RUNS", f)
        grids.append(_lift(depth, cams, 32)[0])
    assert np.array_equal(grids[0], grids[1])


@pytest.mark.parametrize("cells", [1, 63, 32 * 32 + 5])
def test_classes_and_height(cells):
    rng = np.random.default_rng(20 + cells)
    B = 2
    n = rng.integers(0, 6, size=(B, cells)).astype(np.int32)
    no = (rng.random((B, cells)) * (n + 1)).astype(np.int32).clip(0, n)
    hmax = rng.integers(-1000, 3001, size=(B, cells)).astype(np.int32)
    hmax[n == 0] = R.INT_MIN
    hmin = np.where(n == 0, R.INT_MAX, hmax - rng.integers(0, 500, size=(B, cells))).astype(np.int32)
    grid = np.stack([n, no, hmin, hmax], 1)
    for mp, op in ((1, 2), (2, 1), (0, 0), (3, 3)):
        wcls, wh = R.classes(grid.reshape(B, 4, 1, cells), mp, op)
        for want_h in (False, True):
            cbuf, cls = _guarded(B * cells, torch.uint8)
            hbuf, hgt = _guarded(B * cells, torch.float32)
            ops.call("jp_depth_bev_classes", torch.from_numpy(grid).to(DEV), cls, hgt if want_h else None, B, cells, mp, op)
            torch.cuda.synchronize()
            assert _canaries_alive(cbuf, B * cells) and _canaries_alive(hbuf, B * cells)
            assert np.array_equal(cls.cpu().numpy(), wcls.reshape(-1)), (mp, op)
            if want_h:
                got = hgt.cpu().numpy()
                assert np.array_equal(np.isnan(got), wcls.reshape(-1) == 255)
                assert np.array_equal(got, wh.reshape(-1), equal_nan=True)
            else:
                assert bool((hgt == POISON[torch.float32]).all())            # not asked for: not written
    assert set(np.unique(R.classes(grid.reshape(B, 4, 1, cells))[0]).tolist()) <= {1, 2, 255}


@pytest.mark.parametrize("cells", [1, 63, 1024, 64 * 64 + 5])
def test_agreement_counts(cells):
    rng = np.random.default_rng(30 + cells)
    B = 3
    lifted = rng.choice(np.array([0, 1, 2, 3, 255], dtype=np.uint8), size=(B, cells), p=[0.05, 0.4, 0.3, 0.05, 0.2])
    layout = rng.choice(np.array([0, 1, 2, 3, 255], dtype=np.uint8), size=(B, cells), p=[0.4, 0.3, 0.2, 0.05, 0.05])
    buf, out = _guarded(B * 6, torch.int32)
    for _ in range(2):                                                       # overwritten, not accumulated
        ops.call("jp_bev_agree", torch.from_numpy(lifted).to(DEV), torch.from_numpy(layout).to(DEV), out, B, cells)
    torch.cuda.synchronize()
    assert _canaries_alive(buf, B * 6)
    want = R.agree(lifted, layout)
    assert np.array_equal(out.cpu().numpy().reshape(B, 2, 3), want)
    if cells >= 1024:
        assert (want > 0).all() and want.sum() < B * cells


def test_depth_bev_object(form):
    depth, cams = _scene(seed=6)
    H, W = depth.shape[1:]
    K = np.zeros((2, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cams[:, 0], cams[:, 1], cams[:, 2], cams[:, 3], 1.0
    db = DepthBev(2, 16, K, (H, W), plane=cams[:, 4:], min_points=2)
    assert np.array_equal(db.cam.cpu().numpy(), cams)
    assert np.array_equal(db.grid.cpu().numpy(), R.empty_grid(2, 16)) and bool((db.cls == 255).all()) and int(db.agree.abs().sum()) == 0
    d = torch.from_numpy(depth).to(DEV)
    with pytest.raises(ValueError, match="depth must be"):
        db.lift(d[:, :, :-1])
    with pytest.raises(TypeError, match="float32"):
        db.lift(d.double())
    with pytest.raises(ValueError, match="layout must be"):
        db.agreement(torch.zeros((2, 16, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError, match="uint8"):
        db.agreement(torch.zeros((2, 16, 16), dtype=torch.int32, device=DEV))
    assert db.lift(d.unsqueeze(1)) is db
    want = R.lift(R.empty_grid(2, 16), depth, cams, 16, 2.5, **RANGE)
    assert np.array_equal(db.grid.cpu().numpy(), want)
    wcls, wh = R.classes(want, 2, 2)
    assert np.array_equal(db.classes().cpu().numpy(), wcls) and db.classes() is db.cls
    assert np.array_equal(db.height().cpu().numpy(), wh, equal_nan=True)
    layout = torch.from_numpy(np.random.default_rng(7).integers(0, 3, size=(2, 16, 16), dtype=np.uint8)).to(DEV)
    counts = db.agreement(layout)
    wantc = R.agree(wcls, layout.cpu().numpy())
    assert counts is db.agree and np.array_equal(counts.cpu().numpy(), wantc) and wantc.sum() > 0
    s = agreement_scores(counts, cells=256)
    assert s["observed"].shape == (2,) and np.array_equal(s["observed"], wantc.sum((1, 2)) / 256.0)
    db.lift(d, accumulate=True)
    assert np.array_equal(db.grid[:, 0].cpu().numpy(), 2 * want[:, 0])
    db.reset()
    assert np.array_equal(db.grid.cpu().numpy(), R.empty_grid(2, 16)) and bool((db.cls == 255).all())
    # K given for camera frames twice as wide and four times as high as the depth maps is scaled down to them
    K2 = K.copy()
    K2[:, 0] *= 2.0
    K2[:, 1] *= 4.0
    db2 = DepthBev(2, 16, K2, (4 * H, 2 * W), depth_hw=(H, W), plane=cams[:, 4:])
    assert np.array_equal(db2.lift(d).grid.cpu().numpy(), want)
