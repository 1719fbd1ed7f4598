"""LiDAR depth ground truth on the device (csrc/lidar.hip, core/evaluation.py::lidar_depth_maps).

Expected values come from the reference's own generate_depth_map (tests/golden/lidar_depth_{a,b}.npz, written by
tools/make_lidar_golden.py on synthetic calibration files and scans) and, where no golden exists (the large map, and an item pushed
through a map of another size), from `restate` below: a numpy restatement -- per-pixel minimum, the rule for the pixel pairs
(r, W-1) / (r+1, 0) that share the reference's duplicate key, the clamp of negatives -- that is itself pinned to the goldens first.

Where the bounds come from:
* pixel set: the fixtures guarantee (cond_half_dist >= 1e-9) that no last-bit difference of a 4-term float64 dot product moves a
  point to another pixel, so the set of nonzero pixels must be identical.
* values: |d - d_ref| <= 16 * 2^-53 * max_i sum_j |P[2,j] v_ij| over the points that land in the image: the worst-case difference of
  two evaluation orders (with or without fused multiply-adds) of a 4-term float64 dot product is 4 units of that sum's last place;
  the bound leaves a factor of 4.  With vel_depth the value is a float32 coordinate widened to float64: exact.
* the two goldens differ in size and a call has one size, so the ragged call runs both scans through EACH size: the item whose size
  matches is compared with the reference's map, the other with the restatement.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd._lib import call, lib                                       # noqa: E402
from jperceiver_amd.core import evaluation as ev                                # noqa: E402

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def gold(tag):
    if tag not in _CACHE:
        _CACHE[tag] = dict(np.load(os.path.join(GOLD, f"lidar_depth_{tag}.npz")))
    return _CACHE[tag]


def project(pts, P, H, W):
    """-> (pixel index, q2, velodyne x) of the points that land in the image, in file order"""
    v = pts[pts[:, 0] >= 0].astype(np.float64)
    vx = v[:, 0].copy()
    v[:, 3] = 1.0
    q = v @ np.asarray(P, dtype=np.float64).T
    with np.errstate(all="ignore"):
        u, w = np.round(q[:, 0] / q[:, 2]) - 1, np.round(q[:, 1] / q[:, 2]) - 1
        keep = (u >= 0) & (w >= 0) & (u < W) & (w < H)
    return (w[keep].astype(np.int64) * W + u[keep].astype(np.int64)), q[keep, 2], vx[keep], np.abs(v[keep] * np.abs(P[2])).sum(1)


def restate(pts, P, H, W, vel_depth=False):
    pix, q2, vx, _ = project(pts, P, H, W)
    d = vx if vel_depth else q2
    idx = np.arange(len(pix))
    mn = np.full(H * W, np.inf)
    np.minimum.at(mn, pix, d)
    first = np.full(H * W, len(pix) + 1)
    np.minimum.at(first, pix, idx)
    last = np.full(H * W, -1)
    np.maximum.at(last, pix, idx)
    has = last >= 0
    depth = np.where(has, mn, 0.0)
    for r in range(H - 1):
        a, b = r * W + W - 1, (r + 1) * W                   # one key in the reference's duplicate search
        if has[a] and has[b]:
            owner, other = (a, b) if first[a] < first[b] else (b, a)
            depth[owner] = min(mn[a], mn[b])
            depth[other] = d[last[other]]
    depth[depth < 0] = 0
    return depth.reshape(H, W)


def bound(pts, P, H, W):
    mags = project(pts, P, H, W)[3]
    return 16.0 * 2.0 ** -53 * float(mags.max())


def raw(points, P, hw, flip=None, vel_depth=False, poison=False):
    """jp_lidar_depth_map with BOTH outputs -> (out64, out32); poison: NaN bit patterns in the workspace and the outputs"""
    B, (H, W) = len(points), hw
    counts = [len(p) for p in points]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=DEV)
    pts = torch.from_numpy(np.concatenate(list(points) + [np.zeros((1, 4), np.float32)], 0)).to(DEV)
    Pm = torch.from_numpy(np.broadcast_to(np.asarray(P, dtype=np.float64), (B, 3, 4)).copy()).to(DEV)
    fl = None if flip is None else torch.tensor(flip, dtype=torch.uint8, device=DEV)
    nbytes = lib().fn["jp_lidar_depth_ws_bytes"](B, H, W)
    ws = torch.full((nbytes,), 0xFF if poison else 0x5A, dtype=torch.uint8, device=DEV)
    fill = float("nan") if poison else -7.0
    out64 = torch.full((B, H, W), fill, dtype=torch.float64, device=DEV)
    out32 = torch.full((B, H, W), fill, dtype=torch.float32, device=DEV)
    call("jp_lidar_depth_map", pts, offsets, Pm, fl, B, H, W, 1 if vel_depth else 0, out64, out32, ws)
    return out64, out32


def check(got, ref, tol):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape
    assert np.array_equal(got != 0, ref != 0), f"{int(((got != 0) != (ref != 0)).sum())} pixels differ in occupancy"
    err = float(np.abs(got - ref).max())
    print(f"max |d - ref| = {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    assert (got >= 0).all()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_equals_the_reference(tag):
    g = gold(tag)
    H, W = (int(v) for v in g["hw"])
    assert g["cond_half_dist"] >= 1e-9 and g["cond_pairs"] >= 5 and g["cond_negative"] >= 10
    assert g["cond_pairs_first_col0"] >= 1 and g["cond_pairs_first_colW"] >= 1 and g["cond_negative_shared"] >= 1
    assert np.array_equal(restate(g["points"], g["P"], H, W), g["depth"])
    assert np.array_equal(restate(g["points"], g["P"], H, W, True), g["depth_vel"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_single_scan_matches_the_reference(tag):
    g = gold(tag)
    H, W = (int(v) for v in g["hw"])
    out = ev.lidar_depth_maps([g["points"]], g["P"], (H, W))
    assert out.shape == (1, H, W) and out.dtype == torch.float64 and out.is_cuda
    check(out[0], g["depth"], bound(g["points"], g["P"], H, W))
    vel = ev.lidar_depth_maps([torch.from_numpy(g["points"])], torch.from_numpy(g["P"]), (H, W), vel_depth=True)
    assert np.array_equal(vel[0].cpu().numpy(), g["depth_vel"])                 # exact
    f32 = ev.lidar_depth_maps([g["points"]], g["P"], (H, W), dtype=torch.float32)
    assert f32.dtype == torch.float32 and torch.equal(f32, out.float())


@pytest.mark.parametrize("size_of", ["a", "b"])
def test_ragged_call_of_both_scans(size_of):
    ga, gb = gold("a"), gold("b")
    H, W = (int(v) for v in gold(size_of)["hw"])
    empty = np.zeros((0, 4), np.float32)
    scans = [ga["points"], empty, gb["points"]]
    Ps = np.stack([ga["P"], ga["P"], gb["P"]])
    out = ev.lidar_depth_maps(scans, Ps, (H, W))
    for i, g, tag in ((0, ga, "a"), (2, gb, "b")):
        ref = g["depth"] if tag == size_of else restate(g["points"], g["P"], H, W)
        check(out[i], ref, bound(g["points"], g["P"], H, W))
    assert float(out[1].abs().max()) == 0.0                                     # no point: an all-zero map
    vel = ev.lidar_depth_maps(scans, Ps, (H, W), vel_depth=True)
    for i, g, tag in ((0, ga, "a"), (2, gb, "b")):
        ref = g["depth_vel"] if tag == size_of else restate(g["points"], g["P"], H, W, True)
        assert np.array_equal(vel[i].cpu().numpy(), ref)
    # the items of a batch do not see each other
    alone = ev.lidar_depth_maps([gb["points"]], gb["P"], (H, W))
    assert torch.equal(alone[0], out[2])


def test_outputs_flip_poison_and_repeatability():
    ga, gb = gold("a"), gold("b")
    H, W = (int(v) for v in ga["hw"])
    scans, Ps = [ga["points"], gb["points"], ga["points"]], np.stack([ga["P"], gb["P"], ga["P"]])
    o64, o32 = raw(scans, Ps, (H, W))
    check(o64[0], ga["depth"], bound(ga["points"], ga["P"], H, W))
    assert torch.equal(o32, o64.float())                                        # bit for bit
    p64, p32 = raw(scans, Ps, (H, W), poison=True)                              # NaN-filled workspace and outputs
    assert torch.equal(p64, o64) and torch.equal(p32, o32)
    for _ in range(2):                                                          # run to run
        r64, r32 = raw(scans, Ps, (H, W))
        assert torch.equal(r64, o64) and torch.equal(r32, o32)
    f64, f32 = raw(scans, Ps, (H, W), flip=[1, 0, 1])
    assert torch.equal(f64[0], torch.flip(o64[0], [-1])) and torch.equal(f64[2], torch.flip(o64[2], [-1]))
    assert torch.equal(f64[1], o64[1]) and torch.equal(f32, f64.float())
    z64, _ = raw(scans, Ps, (H, W), flip=[0, 0, 0])
    assert torch.equal(z64, o64)
    api = ev.lidar_depth_maps(scans, Ps, (H, W), flip=[True, False, True])
    assert torch.equal(api, f64)
    # one output only
    only32 = ev.lidar_depth_maps(scans, Ps, (H, W), dtype=torch.float32)
    assert torch.equal(only32, o32)


def test_generate_depth_map_reads_kitti_files(tmp_path):
    g = gold("b")
    (tmp_path / "calib_cam_to_cam.txt").write_text(str(g["cam2cam_txt"]))
    (tmp_path / "calib_velo_to_cam.txt").write_text(str(g["velo2cam_txt"]))
    g["points"].tofile(tmp_path / "0000000000.bin")
    H, W = (int(v) for v in g["hw"])
    out = ev.generate_depth_map(str(tmp_path), str(tmp_path / "0000000000.bin"), cam=int(g["cam"]))
    assert out.shape == (H, W)
    check(out, g["depth"], bound(g["points"], g["P"], H, W))
    vel = ev.generate_depth_map(str(tmp_path), str(tmp_path / "0000000000.bin"), int(g["cam"]), True)
    assert np.array_equal(vel.cpu().numpy(), g["depth_vel"])


def test_kitti_sized_map_matches_the_restatement():
    """375 x 1242, 120 000 points (more than one stride of the scatter grid, pixel indices past 2^16), two different scans."""
    H, W, n = 375, 1242, 120000
    f = 721.5377
    K = np.array([[f, 0, 609.5593, 44.85728], [0, f, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
    rigid = np.array([[0.0, -1, 0, -0.004], [0, 0, -1, -0.076], [1, 0, 0, -0.272], [0, 0, 0, 1]])
    P = K @ rigid
    scans = []
    for seed in (11, 12):
        rng = np.random.default_rng(seed)
        x = rng.uniform(-5.0, 80.0, n)
        y, z = x * rng.uniform(-1.0, 1.0, n), x * rng.uniform(-0.3, 0.3, n)
        x[:200], y[:200], z[:200] = rng.uniform(0, 0.3, 200), rng.uniform(-0.07, 0.07, 200), rng.uniform(-0.1, -0.05, 200)
        scans.append(np.stack([x, y, z, rng.uniform(0, 1, n)], 1).astype(np.float32)[rng.permutation(n)])
    out = ev.lidar_depth_maps(scans, P, (H, W))
    for i, pts in enumerate(scans):
        ref = restate(pts, P, H, W)
        assert (ref != 0).sum() > 30000
        check(out[i], ref, bound(pts, P, H, W))
