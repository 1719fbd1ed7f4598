"""The three kernels of csrc/bevmap.hip through ops.call, against the float64 numpy restatement in tests/bevmap_ref.py, which works
on the WHOLE map (a window of jp_bev_fuse that missed a cell would show).  Every comparison is torch.equal with no cell excluded:
the header pins the arithmetic operation by operation, each rounded once, and integer votes do not depend on any order.

Shapes are the smallest at which the kernels can still go wrong: occ 16 and 20 (res_f = 2.5 and 2 m), a map of 48 x 40 cells (a
row / column swap shows) with world (0, 0) off its centre, two cameras with different poses in every call, map cells as large as
the frame's (`eq`), half as large (`fine`) and 1.2 x as large (`coarse`: cell centres fall exactly on frame-cell boundaries), and
seeded random layouts.  Every output is a slice out of the middle of a larger buffer of canary values that must survive."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                                     # noqa: E402
from tests import bevmap_ref as R                                  # noqa: E402

DEV = "cuda"
MH, MW = 48, 40
ORG = (30.0, 18.0)
PAD = 4096
CANARY = {torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5}
GRID = [(16, "eq"), (16, "fine"), (16, "coarse"), (20, "eq"), (20, "fine"), (20, "coarse")]


def _res(occ, mode):
    res_f = 40.0 / occ
    return res_f, {"eq": res_f, "fine": res_f / 2, "coarse": 1.2 * res_f}[mode]


def _guarded(n, dtype, init=None):
    """-> (whole buffer, the n elements in its middle): canaries on both sides"""
    buf = torch.full((n + 2 * PAD,), CANARY[dtype], dtype=dtype, device=DEV)
    mid = buf[PAD:PAD + n]
    if init is None:
        mid.zero_()
    else:
        mid.copy_(torch.as_tensor(init, dtype=dtype).reshape(-1))
    return buf, mid


def _canaries_alive(buf, n):
    c = CANARY[buf.dtype]
    return bool((buf[:PAD] == c).all()) and bool((buf[PAD + n:] == c).all())


def _layouts(B, N, occ, seed):
    return np.random.default_rng(seed).integers(0, 3, size=(B, N, occ, occ), dtype=np.uint8)


def _fuse(layouts, poses, occ, mode, off=0.27, max_range=40.0, init=None, times=1, org=ORG):
    """layouts (B,N,occ,occ) uint8, poses (B,N,12|16) float64 (numpy) -> (kernel counts, reference counts) as (B,3,MH,MW) numpy"""
    B, N = layouts.shape[:2]
    res_f, res = _res(occ, mode)
    n = B * 3 * MH * MW
    buf, counts = _guarded(n, torch.int32, init)
    lay = torch.from_numpy(layouts).to(DEV)
    P = torch.from_numpy(np.ascontiguousarray(poses)).to(DEV)
    for _ in range(times):
        ops.call("jp_bev_fuse", lay, P, poses.shape[-1], N, counts, B, occ, res_f, off, max_range, MH, MW, res, org[0], org[1])
    torch.cuda.synchronize()
    assert _canaries_alive(buf, n)
    want = np.zeros((B, 3, MH, MW), dtype=np.int32) if init is None else np.array(init, dtype=np.int32).reshape(B, 3, MH, MW)
    for _ in range(times):
        R.fuse(want, layouts, poses, occ, res_f, off, max_range, res, org[0], org[1])
    return counts.cpu().numpy().reshape(B, 3, MH, MW), want


def _shift(a, b, res):
    T = np.identity(4)
    T[0, 3], T[2, 3] = a * res, b * res
    return T


def _pair(T0, T1):
    return np.stack([T0, T1]).reshape(2, 1, 16)


@pytest.mark.parametrize("occ,mode", GRID)
def test_identity(occ, mode):
    lay = _layouts(2, 1, occ, 1)
    res = _res(occ, mode)[1]
    got, want = _fuse(lay, _pair(np.identity(4), _shift(3, -2, res)), occ, mode, off=0.0)
    assert np.array_equal(got, want)
    assert got[:, 0].max() == 1 and got[0, 0].sum() > 0 and not np.array_equal(got[0], got[1])
    if mode == "eq":            # the hand-computed placement of tests/test_bevmap_abi_cpu.py: the layout as it is, far edge up
        r0, c0 = int(ORG[0]) - occ, int(ORG[1]) - occ // 2
        assert np.array_equal(got[0, 0, r0:r0 + occ, c0:c0 + occ], np.ones((occ, occ), dtype=np.int32))
        assert got[0, 0].sum() == occ * occ
        assert np.array_equal(got[0, 1, r0:r0 + occ, c0:c0 + occ], (lay[0, 0] == 1).astype(np.int32))
        assert np.array_equal(got[0, 2, r0:r0 + occ, c0:c0 + occ], (lay[0, 0] == 2).astype(np.int32))


@pytest.mark.parametrize("occ,mode", GRID)
def test_whole_cell_translations_on_and_off_every_edge(occ, mode):
    lay = _layouts(2, 1, occ, 2)
    res = _res(occ, mode)[1]
    far = 3 * max(MH, MW)
    #        inside    partly off: left, right, top, bottom          wholly off: left, right, top, bottom
    shifts = [(2, 5), (-14, 0), (19, 1), (0, 25), (1, -24), (-far, 0), (far, 0), (0, far), (0, -far), (-far, far)]
    seen = 0
    for a, b in shifts:
        got, want = _fuse(lay, _pair(_shift(a, b, res), _shift(-a, b + 1, res)), occ, mode)
        assert np.array_equal(got, want), (a, b)
        if abs(a) == far or abs(b) == far:
            assert got.sum() == 0, (a, b)
        seen += int(got[:, 0].sum())
    assert seen > 0


@pytest.mark.parametrize("occ,mode", GRID)
def test_exact_quarter_and_half_turns(occ, mode):
    lay = _layouts(2, 1, occ, 3)
    res = _res(occ, mode)[1]
    for deg, other in ((90, 270), (180, 90), (270, 180)):
        got, want = _fuse(lay, _pair(R.yaw_pose(deg), R.yaw_pose(other, 2 * res, -3 * res)), occ, mode, off=0.0)
        assert np.array_equal(got, want), deg
        assert got[0, 0].sum() > 0
        if mode == "eq" and deg == 90:      # forward = to the right on the map: the layout turned clockwise, beside the origin column
            r0, c0 = int(ORG[0]) - occ // 2, int(ORG[1])
            assert np.array_equal(got[0, 1, r0:r0 + occ, c0:c0 + occ], (np.rot90(lay[0, 0], -1) == 1).astype(np.int32))


@pytest.mark.parametrize("occ,mode", GRID)
def test_general_poses(occ, mode):
    rng = np.random.default_rng(100 + occ)
    res = _res(occ, mode)[1]
    lay = _layouts(2, 8, occ, 4)
    # yaw anywhere, pitch and roll <= 0.1 rad; translation up to the map size for one camera, near the map for the other
    poses = np.stack([np.stack([R.general_pose(rng, max(MH, MW) * res) for _ in range(8)]),
                      np.stack([R.general_pose(rng, 8 * res) for _ in range(8)])]).reshape(2, 8, 16)
    hits = 0
    for k in range(8):
        got, want = _fuse(lay[:, k:k + 1], poses[:, k:k + 1], occ, mode, org=(29.5, 18.25))
        assert np.array_equal(got, want), k
        hits += int(got[:, 0].sum())
    assert hits > 0


@pytest.mark.parametrize("occ,mode", GRID)
def test_offsets_and_max_range(occ, mode):
    rng = np.random.default_rng(7)
    lay = _layouts(2, 1, occ, 5)
    poses = np.stack([R.general_pose(rng, 5.0), np.identity(4)]).reshape(2, 1, 16)
    results = []
    for off in (0.0, 0.27, 1.9):
        got, want = _fuse(lay, poses, occ, mode, off=off)
        assert np.array_equal(got, want), off
        results.append(got)
    assert not np.array_equal(results[0], results[2])
    got, want = _fuse(lay, poses, occ, mode, max_range=15.0)
    assert np.array_equal(got, want)
    assert 0 < got[:, 0].sum() < results[1][:, 0].sum()


@pytest.mark.parametrize("occ,mode", GRID)
def test_counts_accumulate_and_batches_equal_single_frames(occ, mode):
    rng = np.random.default_rng(11)
    lay = _layouts(2, 7, occ, 6)
    poses = np.stack([R.general_pose(rng, 10.0) for _ in range(14)]).reshape(2, 7, 16)
    # the same frame three times: three times the counts
    once, want1 = _fuse(lay[:, :1], poses[:, :1], occ, mode)
    thrice, want3 = _fuse(lay[:, :1], poses[:, :1], occ, mode, times=3)
    assert np.array_equal(once, want1) and np.array_equal(thrice, want3) and np.array_equal(thrice, 3 * once)
    assert once[:, 0].sum() > 0
    # N = 7 in one call (atomics) = seven single-frame calls (one owner per cell), on top of counts that are already there
    init = rng.integers(0, 5, size=(2, 3, MH, MW)).astype(np.int32)
    batch, want = _fuse(lay, poses, occ, mode, init=init)
    assert np.array_equal(batch, want)
    single = init
    for k in range(7):
        single, _ = _fuse(np.ascontiguousarray(lay[:, k:k + 1]), np.ascontiguousarray(poses[:, k:k + 1]), occ, mode, init=single)
    assert np.array_equal(batch, single)
    assert batch[:, 0].max() > init[:, 0].max()
    # rows 0..2 of the poses (pose_stride 12) give what the 4 x 4 gives (pose_stride 16)
    rows, _ = _fuse(lay, np.ascontiguousarray(poses[:, :, :12]), occ, mode, init=init)
    assert np.array_equal(rows, batch)


@pytest.mark.parametrize("occ,mode", GRID)
def test_degenerate_poses_contribute_nothing(occ, mode):
    rng = np.random.default_rng(13)
    lay = _layouts(2, 1, occ, 8)
    init = rng.integers(0, 5, size=(2, 3, MH, MW)).astype(np.int32)
    good = np.identity(4)
    flat = np.identity(4)
    flat[0, 0] = 1e-7                                       # det = 1e-7 < 1e-6
    zero = np.zeros((4, 4))
    nan_t = np.identity(4)
    nan_t[0, 3] = np.nan                                    # a finite det, but nowhere to put the window
    inf_t = np.identity(4)
    inf_t[2, 3] = -np.inf
    huge = _shift(1e300, -1e300, 1.0)
    for name, bad in (("det", flat), ("zero", zero), ("nan", np.full((4, 4), np.nan)), ("nan_t", nan_t), ("inf_t", inf_t), ("huge", huge)):
        for cam in (0, 1):
            poses = _pair(bad, good) if cam == 0 else _pair(good, bad)
            got, want = _fuse(lay, poses, occ, mode, init=init)
            assert np.array_equal(got, want), name
            assert np.array_equal(got[cam], init[cam]), name                 # untouched
            assert got[1 - cam, 0].sum() > init[1 - cam, 0].sum(), name      # the other camera of the same call is fused
    # ... and with N > 1 (the atomic kernel): the bad frames of a batch are skipped, the good ones counted
    poses = np.stack([flat, good, np.full((4, 4), np.nan), good, nan_t, good]).reshape(2, 3, 16)
    got, want = _fuse(_layouts(2, 3, occ, 9), poses, occ, mode, init=init)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("cells", [1, 63, MH * MW])
def test_map_classes(cells):
    rng = np.random.default_rng(17 + cells)
    B = 2
    seen = rng.integers(0, 9, size=(B, cells)).astype(np.int32)
    car = (rng.random((B, cells)) * (seen + 1)).astype(np.int32).clip(0, seen)
    road = (rng.random((B, cells)) * (seen - car + 1)).astype(np.int32).clip(0, seen - car)
    counts = np.stack([seen, road, car], 1)                              # (B,3,cells): seen = 0 and exact ties are frequent
    if cells >= 8:
        counts[0, :, :8] = [[0, 4, 4, 4, 4, 3, 8, 8], [0, 2, 1, 0, 1, 3, 3, 4], [0, 0, 0, 2, 1, 0, 1, 4]]
    for min_seen, rf, cf in ((1.0, 0.5, 0.5), (4.0, 0.5, 0.5), (1.0, 0.75, 0.25), (0.0, 1.0, 1.0)):
        wcls, wrgb = R.classes(counts.reshape(B, 3, 1, cells), min_seen, rf, cf)
        for want_rgb in (False, True):
            cbuf, cls = _guarded(B * cells, torch.uint8)
            rbuf, rgb = _guarded(B * cells * 3, torch.uint8)
            ops.call("jp_bev_map_classes", torch.from_numpy(counts).to(DEV), cls, rgb if want_rgb else None, B, cells, min_seen, rf, cf)
            torch.cuda.synchronize()
            assert _canaries_alive(cbuf, B * cells) and _canaries_alive(rbuf, B * cells * 3)
            assert np.array_equal(cls.cpu().numpy(), wcls.reshape(-1)), (min_seen, rf, cf)
            if want_rgb:
                assert np.array_equal(rgb.cpu().numpy(), wrgb.reshape(-1))
            else:
                assert bool((rgb == 0).all())                            # not asked for: not written
    if cells >= 8:
        wcls, _ = R.classes(counts.reshape(B, 3, 1, cells), 1.0, 0.5, 0.5)
        assert wcls[0, 0, :8].tolist() == [255, 1, 0, 2, 1, 1, 1, 2]


@pytest.mark.parametrize("mode", ["eq", "fine"])
def test_map_mark(mode):
    res = _res(16, mode)[1]
    B, cap, n = 2, 9, 7
    rng = np.random.default_rng(23)
    traj = np.zeros((B, cap, 12))
    traj[:, :, [0, 5, 10]] = 1.0
    traj[:, :, 3] = rng.uniform(-20, 20, size=(B, cap))
    traj[:, :, 11] = rng.uniform(-15, 30, size=(B, cap))
    traj[0, 1, [3, 11]] = traj[0, 0, [3, 11]]               # a repeated row
    traj[0, 2, 3] = 1e6                                     # off the map: right, above, not finite
    traj[1, 0, 11] = 1e6
    traj[1, 1, 3] = np.nan
    traj[1, 2, 11] = np.inf
    traj[1, 3, [3, 11]] = [-ORG[1] * res, ORG[0] * res - 1e-9]          # the map's first cell
    traj[1, 4, [3, 11]] = [(MW - ORG[1]) * res, 0.0]                    # one column past its last
    traj[:, n:, [3, 11]] = 0.0                              # rows past n are not drawn: they would mark the origin cell
    img = rng.integers(0, 256, size=(B, MH, MW, 3)).astype(np.uint8)
    buf, rgb = _guarded(img.size, torch.uint8, img)
    color = (250, 128, 7)
    ops.call("jp_bev_map_mark", rgb, B, MH, MW, torch.from_numpy(traj).to(DEV), n, cap, res, ORG[0], ORG[1],
             color[0] | color[1] << 8 | color[2] << 16)
    torch.cuda.synchronize()
    assert _canaries_alive(buf, img.size)
    want = R.mark(img.copy(), traj, n, res, ORG[0], ORG[1], color)
    got = rgb.cpu().numpy().reshape(img.shape)
    assert np.array_equal(got, want)
    changed = (got != img).any(-1)
    assert 0 < changed[0].sum() <= n - 2 and 0 < changed[1].sum() <= n - 4
    assert changed[1, 0, 0] and not changed[0, int(ORG[0]), int(ORG[1])]
