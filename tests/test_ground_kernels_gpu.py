"""jp_ground_fit (csrc/ground.hip) through ops.call, and `DepthBev(ground=...)` on top of it, against the numpy restatement in
tests/ground_ref.py.  `mom` compares with np.array_equal (integers), `cam` and `stat` bit for bit (array_equal, NaN-aware): the
header pins the arithmetic operation by operation, each rounded once, and integer sums do not depend on any order.

Shapes are the smallest at which the kernels can still go wrong: 48 x 200 and 7 x 70 images of two cameras with different
intrinsics and priors -- W is no multiple of the 64 lanes, waves straddle image rows, the last workgroup is partly empty -- with
parts = 1, 3 and 64 workgroups per camera (64 is more than 7 x 70 has work for: empty workgroups have to store zeros), 1, 2 and 4
rounds, with and without a layout, with a prior and tracking.  part, mom and stat sit in the middle of a larger buffer of canary
values that must survive and start out as garbage bytes: the call needs nothing zeroed."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                                     # noqa: E402
from jperceiver_amd.apis import DepthBev                           # noqa: E402
from tests import depthbev_ref as R                                # noqa: E402
from tests import ground_ref as G                                  # noqa: E402

DEV = "cuda"
PAD = 512
OCC = 16
ARGS = dict(occ=OCC, res_f=40.0 / OCC, off=0.27, min_range=1.0, max_range=40.0, band=0.3)
SOLVE = dict(min_points=50, min_spread=0.5, max_tilt_deg=10.0, h_lo=0.5, h_hi=4.0)
SHAPES = {"48x200": (48, 200), "7x70": (7, 70)}


def _normal(pitch_deg, roll_deg):
    n = np.array([math.tan(math.radians(roll_deg)), 1.0, math.tan(math.radians(pitch_deg))])
    return n / np.linalg.norm(n)


def _cams(H, W):
    """two cameras with different intrinsics; the plane columns hold what a tracking call starts from"""
    f = 64.0 if W >= 200 else 20.0
    return np.array([[f, f, 0.5 * W, H / 3.0, 0.0, 1.0, 0.0, 1.5],
                     [1.1 * f + 0.3, 0.9 * f, 0.5 * W + 3.25, H / 3.0 - 0.5, 0.0, 1.0, 0.0, 1.7]], dtype=np.float64)


def _planes():
    return [(*_normal(2.0, 1.0), 1.65), (*_normal(-1.5, -1.0), 1.6)]


def _scene(H, W, seed=0, poison=False, planes=None, box=True, cams=None):
    """(2, H, W) float32: every camera sees its own tilted plane, camera 1 under 0.5 % of noise, camera 0 exactly but for a box 9 m
    ahead that hides the far ground (all of it stands higher above the plane than the band: it must add nothing)"""
    rng = np.random.default_rng(seed)
    cams = _cams(H, W) if cams is None else cams
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for (fx, fy, cx, cy, *_), (nx, ny, nz, h) in zip(cams, planes or _planes()):
        den = nx * (u - cx) / fx + ny * (v - cy) / fy + nz
        with np.errstate(all="ignore"):
            out.append(np.where(den > 1e-3, h / np.where(den > 1e-3, den, 1.0), np.inf))
    d0, d1 = out
    if box:
        rows = max(H // 2 - 2, 1)
        d0[:rows, W // 5:W // 3] = np.minimum(d0[:rows, W // 5:W // 3], 9.0)
    d1 = d1 * rng.uniform(0.995, 1.005, size=d1.shape)
    if poison:
        for d in (d0, d1):
            bad = rng.random(d.shape)
            d[bad < 0.03] = np.nan
            d[(bad >= 0.03) & (bad < 0.05)] = np.inf
            d[(bad >= 0.05) & (bad < 0.07)] = -np.inf
            d[(bad >= 0.07) & (bad < 0.09)] = 0.0
            d[(bad >= 0.09) & (bad < 0.11)] = -3.0
    return np.stack([d0, d1]).astype(np.float32), cams


def _layout(seed=1):
    """(2, OCC, OCC) uint8: mostly road, some background and car cells, one stray value"""
    rng = np.random.default_rng(seed)
    lay = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=(2, OCC, OCC), p=[0.2, 0.7, 0.1])
    lay[0, 3, 3] = 7
    return lay


def _priors():
    return np.array([[0.0, 1.0, 0.0, 1.5], [0.01, math.sqrt(1.0 - 2e-4), 0.01, 1.75]], dtype=np.float64)


def _garbage(n, dtype, seed):
    """-> (whole buffer, the n elements in its middle): canary bytes on both sides, garbage bytes in the middle"""
    size = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((n + 2 * PAD) * size,), 0xA5, dtype=torch.uint8)
    g = torch.Generator().manual_seed(seed)
    raw[PAD * size:(PAD + n) * size] = torch.randint(0, 256, (n * size,), dtype=torch.uint8, generator=g)
    buf = raw.to(DEV).view(dtype)
    return buf, buf[PAD:PAD + n]


def _canaries_alive(buf, n):
    raw = buf.view(torch.uint8)
    size = buf.element_size()
    return bool((raw[:PAD * size] == 0xA5).all()) and bool((raw[(PAD + n) * size:] == 0xA5).all())


def _fit(depth, cams, layout, prior, parts, rounds, **kw):
    """-> (cam (B,8), mom (B,10), stat (B,3)) numpy, as the kernels leave them"""
    B, H, W = depth.shape
    a = {**ARGS, **SOLVE, **kw}
    pbuf, part = _garbage(B * parts * 10, torch.int64, 1)
    mbuf, mom = _garbage(B * 10, torch.int64, 2)
    sbuf, stat = _garbage(B * 3, torch.float64, 3)
    d, cam = torch.from_numpy(depth).to(DEV), torch.from_numpy(cams).to(DEV)
    lay = None if layout is None else torch.from_numpy(layout).to(DEV)
    pri = None if prior is None else torch.from_numpy(prior).to(DEV)
    ops.call("jp_ground_fit", d, lay, pri, cam, part, mom, stat, B, H, W, a["occ"], a["res_f"], a["off"], a["min_range"], a["max_range"],
             a["band"], rounds, parts, a["min_points"], a["min_spread"], a["max_tilt_deg"], a["h_lo"], a["h_hi"])
    torch.cuda.synchronize()
    assert _canaries_alive(pbuf, B * parts * 10) and _canaries_alive(mbuf, B * 10) and _canaries_alive(sbuf, B * 3)
    if pri is not None:
        assert np.array_equal(pri.cpu().numpy(), prior)                # only read
    # what the last round's workgroups left in `part` adds up to mom, and every row was written (garbage would not add up)
    assert np.array_equal(part.cpu().numpy().reshape(B, parts, 10).sum(1), mom.cpu().numpy().reshape(B, 10))
    return cam.cpu().numpy(), mom.cpu().numpy().reshape(B, 10), stat.cpu().numpy().reshape(B, 3)


def _want(depth, cams, layout, prior, rounds, **kw):
    return G.fit(depth, layout, prior, cams, rounds=rounds, **{**ARGS, **SOLVE, **kw})


def _same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2], equal_nan=True))


@pytest.mark.parametrize("with_prior", [True, False], ids=["prior", "tracking"])
@pytest.mark.parametrize("with_layout", [False, True], ids=["free", "layout"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parts_and_rounds(shape, with_layout, with_prior):
    H, W = SHAPES[shape]
    depth, cams = _scene(H, W)
    layout = _layout() if with_layout else None
    prior = _priors() if with_prior else None
    seen = []
    for rounds in (1, 2, 4):
        want = _want(depth, cams, layout, prior, rounds)
        print(f"{shape} layout {with_layout} prior {with_prior} rounds {rounds}: status {want[2][:, 0].tolist()} n {want[1][:, 0].tolist()} "
              f"plane {want[0][:, 4:].round(5).tolist()}")
        for parts in (1, 3, 64):
            got = _fit(depth, cams, layout, prior, parts, rounds)
            assert _same(got, want), (rounds, parts)
            assert np.array_equal(got[0][:, :4], cams[:, :4])           # the intrinsics are only read
        seen.append(want)
    assert all(w[1][:, 0].min() > 0 for w in seen)                      # every camera had inliers in every configuration
    if shape == "48x200" and not with_layout:
        w = seen[1]
        assert (w[2][:, 0] == 0).all() and np.abs(w[0][0, 4:] - np.array(_planes()[0])).max() < 1e-3     # camera 0: an exact plane
        assert not np.array_equal(seen[0][0][:, 4:], seen[1][0][:, 4:])                                  # a second round moves the plane


@pytest.mark.parametrize("shape", list(SHAPES))
def test_poisoned_depth(shape):
    H, W = SHAPES[shape]
    depth, cams = _scene(H, W, seed=4, poison=True)
    assert np.isnan(depth).sum() > 0 and np.isinf(depth).sum() > 0 and (depth <= 0).sum() > 0
    for layout in (None, _layout(2)):
        want = _want(depth, cams, layout, _priors(), 2)
        for parts in (3, 64):
            assert _same(_fit(depth, cams, layout, _priors(), parts, 2), want), parts
        assert want[1][:, 0].min() > 0
    # nothing but poison: ten zeros per camera, status 1, the prior is what the call leaves
    for bad in (np.nan, np.inf, -np.inf, 0.0, -5.0):
        got = _fit(np.full((2, H, W), bad, dtype=np.float32), cams, None, _priors(), 3, 1)
        assert not got[1].any() and got[2][:, :2].tolist() == [[1.0, 0.0]] * 2 and np.isnan(got[2][:, 2]).all()
        assert np.array_equal(got[0][:, 4:], _priors())


def test_image_wider_than_one_column_chunk():
    # 1100 columns: more than the 4 x 256 a workgroup covers at a time -- the kernel's column loop runs twice, the second time mostly
    # past the end of the row -- and 5 rows: with parts = 64 most workgroups have no row at all
    H, W = 5, 1100
    cams = np.array([[400.0, 20.0, 550.0, 1.0, 0.0, 1.0, 0.0, 1.5], [380.0, 21.0, 540.5, 0.75, 0.0, 1.0, 0.0, 1.7]])
    depth, _ = _scene(H, W, seed=9, planes=[(*_normal(1.0, 0.5), 1.55), (*_normal(-1.0, 0.5), 1.65)], box=False, cams=cams)
    for layout in (None, _layout(6)):
        want = _want(depth, cams, layout, None, 2)
        print(f"5x1100 layout {layout is not None}: status {want[2][:, 0].tolist()} n {want[1][:, 0].tolist()}")
        for parts in (1, 3, 64):
            assert _same(_fit(depth, cams, layout, None, parts, 2), want), parts
        cut = depth.copy()
        cut[:, :, 1024:] = 0.0                                          # the columns of the second chunk do count
        assert (_want(cut, cams, layout, None, 2)[1][:, 0] < want[1][:, 0]).all()


def test_every_rejection_leaves_the_plane():
    H, W = SHAPES["48x200"]
    cams = _cams(H, W)
    level = _priors()
    level[1] = [0.0, 1.0, 0.0, 1.7]
    # status 1: a plane pitched 10 degrees has no inlier against a level prior.  status 2: one image row has no spread along z.
    steep, _ = _scene(H, W, planes=[(*_normal(10.0, 0.0), 1.5), (*_normal(10.0, 0.0), 1.7)], box=False)
    flat, _ = _scene(H, W, planes=[(0.0, 1.0, 0.0, 1.5), (0.0, 1.0, 0.0, 1.7)], box=False)
    row = np.zeros_like(flat)
    row[:, 24] = flat[:, 24]
    good, _ = _scene(H, W)
    cases = [("too few points", steep, {}, [1, 1]),
             ("ill-conditioned", row, {}, [2, 2]),
             ("height out of bounds", good, dict(h_hi=1.62), [3, 0]),          # camera 0's plane is 1.65 m up, camera 1's 1.6
             ("tilt out of bounds", good, dict(max_tilt_deg=2.0), [3, 0])]      # camera 0 is tilted 2.24 degrees, camera 1 1.80
    for what, depth, kw, status in cases:
        for prior in (level, None):
            start = cams.copy()
            if prior is not None:
                start[:, 4:] = [[0.3, 0.8, 0.1, 2.5], [0.2, 0.9, -0.1, 3.0]]  # not read, and overwritten with the prior or the fit
            want = _want(depth, start, None, prior, 2, **kw)
            got = _fit(depth, start, None, prior, 3, 2, **kw)
            print(f"{what}, prior {prior is not None}: status {got[2][:, 0].tolist()} n {got[2][:, 1].tolist()}")
            assert _same(got, want), what
            assert got[2][:, 0].tolist() == status, what
            for b in (0, 1):
                if status[b] != 0:
                    assert np.array_equal(got[0][b, 4:], level[b] if prior is not None else cams[b, 4:]), (what, b)
                    assert np.isnan(got[2][b, 2])
                else:
                    assert not np.array_equal(got[0][b, 4:], start[b, 4:]) and got[2][b, 2] >= 0.0


def test_two_runs_give_the_same_bits():
    H, W = SHAPES["48x200"]
    depth, cams = _scene(H, W, seed=7, poison=True)
    a = _fit(depth, cams, _layout(3), _priors(), 64, 2)
    b = _fit(depth, cams, _layout(3), _priors(), 64, 2)
    assert _same(a, b) and a[1][:, 0].min() > 0
    # tracking: a second call starts where the first ended -- two calls of one round equal one call of two rounds
    one = _fit(depth, cams, None, None, 3, 1)
    two = _fit(depth, one[0], None, None, 3, 1)
    assert _same(two, _fit(depth, cams, None, None, 3, 2))


def test_lift_after_fit_uses_the_fitted_plane():
    H, W = SHAPES["48x200"]
    depth, cams = _scene(H, W, seed=8)
    K = np.zeros((2, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cams[:, 0], cams[:, 1], cams[:, 2], cams[:, 3], 1.0
    layout = _layout(5)
    d, lay = torch.from_numpy(depth).to(DEV), torch.from_numpy(layout).to(DEV)
    lift = dict(off=0.27, min_range=1.0, max_range=40.0, h_min=-1.0, h_max=3.0, obst_h=0.3)
    for track in (False, True):
        g = dict(rounds=2, parts=3, min_points=50, track=track)
        db = DepthBev(2, OCC, K, (H, W), plane=cams[:, 4:], ground=g)
        assert np.array_equal(db.plane0.cpu().numpy(), cams[:, 4:]) and db.plane0.dtype == torch.float64
        assert db.ground()["status"].tolist() == [-1, -1]
        with pytest.raises(ValueError, match="use_layout"):
            db.fit_ground(d)
        with pytest.raises(ValueError, match="layout must be"):
            db.fit_ground(d, lay[:, :8])
        with pytest.raises(TypeError, match="uint8"):
            db.fit_ground(d, lay.int())
        with pytest.raises(ValueError, match="depth must be"):
            db.fit_ground(d[:, :, :-1], lay)
        assert db.fit_ground(d.unsqueeze(1), lay) is db
        want = _want(depth, cams, layout, None if track else cams[:, 4:].copy(), 2)
        assert np.array_equal(db.cam.cpu().numpy(), want[0]) and np.array_equal(db.mom.cpu().numpy(), want[1])
        assert np.array_equal(db.stat.cpu().numpy(), want[2], equal_nan=True) and (want[2][:, 0] == 0).all()
        db.lift(d)
        grid = R.lift(R.empty_grid(2, OCC), depth, want[0], OCC, 40.0 / OCC, **lift)
        assert np.array_equal(db.grid.cpu().numpy(), grid)
        assert not np.array_equal(grid, R.lift(R.empty_grid(2, OCC), depth, cams, OCC, 40.0 / OCC, **lift))      # the plane matters
        got = db.ground()
        assert np.array_equal(got["plane"], want[0][:, 4:]) and np.array_equal(got["height"], want[0][:, 7])
        assert got["status"].tolist() == [0, 0] and got["n"].tolist() == want[1][:, 0].tolist() and np.array_equal(got["rms"], want[2][:, 2])
        assert np.array_equal(got["height_ratio"], want[0][:, 7] / cams[:, 7])
        assert np.allclose(got["pitch_deg"], [2.0, -1.5], atol=0.1) and np.allclose(got["roll_deg"], [1.0, -1.0], atol=0.1)
        # a second call: from plane0 again, or from where the first ended
        db.fit_ground(d, lay)
        again = want if not track else _want(depth, want[0], layout, None, 2)
        assert np.array_equal(db.cam.cpu().numpy(), again[0]) and np.array_equal(db.mom.cpu().numpy(), again[1])
        db.reset()
        assert np.array_equal(db.cam.cpu().numpy(), cams) and db.ground()["status"].tolist() == [-1, -1]
    # without the layout gate no layout is needed; without `ground` there is no fit and nothing is allocated for one
    db = DepthBev(2, OCC, K, (H, W), plane=cams[:, 4:], ground=dict(use_layout=False, parts=3, min_points=50))
    db.fit_ground(d)
    assert np.array_equal(db.cam.cpu().numpy(), _want(depth, cams, None, cams[:, 4:].copy(), 2)[0])
    plain = DepthBev(2, OCC, K, (H, W), plane=cams[:, 4:])
    assert plain.ground_kw is None and not hasattr(plain, "part") and not hasattr(plain, "mom")
    with pytest.raises(RuntimeError, match="ground=True"):
        plain.fit_ground(d)
