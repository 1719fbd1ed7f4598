#!/usr/bin/env python
"""Generate tests/golden/lidar_depth_*.npz by running the REAL reference's mono/datasets/kitti_utils.py::generate_depth_map on the
CPU, on synthetic KITTI calibration files and Velodyne scans.  The reference is imported at generation time only (kitti_utils.py is
loaded by file path: `import mono.datasets` would pull in mmcv); no source of it is copied, and no test reads it.  `np.int`, which
the reference still uses, is restored for the call.

Usage:  python tools/make_lidar_golden.py /path/to/reference/checkout

Two items: lidar_depth_a.npz (48 x 20 px, 6000 points, camera 2) and lidar_depth_b.npz (64 x 24 px, 10000 points, camera 3).  Every
scan has many points per pixel, a cluster of points with x in [0, 0.3) close to the optical axis (negative and near-zero q2), points
that project outside the image on all four sides and points with x < 0.  Each file holds the scan, the two calibration files as
text, P, the image size and the reference's float64 maps for vel_depth False / True.

The generator ASSERTS, and stores under `cond_*`, what the tolerances of tests/test_lidar_depth_gpu.py rest on:
 (a) no projected q0/q2 or q1/q2 of a kept point lies within 1e-9 of a half-integer (no last-bit difference of a 4-term dot product
     can move a pixel) -- cond_half_dist is the smallest distance;
 (b) at least 5 pixel pairs (r, W-1) / (r+1, 0) with points on both sides (the reference's shared duplicate key), at least one with
     the earliest point in column 0 and one with it in column W-1 -- cond_pairs, cond_pairs_first_col0, cond_pairs_first_colW;
 (c) at least 10 in-bounds points with negative d, at least one of them in a pixel that also holds a positive return --
     cond_negative, cond_negative_shared.
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
BASELINE = {2: 0.06, 3: -0.47}                      # P_rect_0c[0, 3] / f: offset of camera c along the image x axis


def import_reference(ref):
    spec = importlib.util.spec_from_file_location("ref_kitti_utils", os.path.join(ref, "mono", "datasets", "kitti_utils.py"))
    ku = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ku)
    return ku


def fmt(a):
    return " ".join("%.6e" % v for v in np.asarray(a, dtype=np.float64).reshape(-1))


def small_rotation(rng, s):
    """exp of a small skew matrix (Rodrigues)"""
    w = s * rng.standard_normal(3)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / t
    return np.identity(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def calib_text(rng, W, H):
    f, cx, cy = 0.625 * W, 0.5 * W + 0.37, 0.5 * H - 0.21
    lines = ["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02"]
    for c, bx in BASELINE.items():
        P = np.array([[f, 0, cx, f * bx], [0, f, cy, 0.02 * c], [0, 0, 1, 0.003 * (c - 1)]])
        lines += [f"S_rect_0{c}: {fmt([W, H])}", f"P_rect_0{c}: {fmt(P)}"]
    lines.insert(2, f"R_rect_00: {fmt(small_rotation(rng, 0.01))}")
    axes = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])                 # velodyne (forward, left, up) -> camera (right, down, forward)
    velo = ["calib_time: 15-Mar-2012 11:37:16", f"R: {fmt(small_rotation(rng, 0.01) @ axes)}", f"T: {fmt([-0.004, -0.076, -0.272])}",
            "delta_f: 0.000000e+00 0.000000e+00", "delta_c: 0.000000e+00 0.000000e+00"]
    return "\n".join(lines) + "\n", "\n".join(velo) + "\n"


def scan(rng, n, bx):
    n_near = 60
    x = rng.uniform(-3.0, 25.0, n)
    y = x * rng.uniform(-1.2, 1.2, n)
    z = x * rng.uniform(-0.5, 0.5, n)
    x[:n_near] = rng.uniform(0.0, 0.3, n_near)                              # q2 = x - 0.27 or so: negative and near zero
    y[:n_near] = bx + rng.uniform(-0.04, 0.04, n_near)                      # on the optical axis of the camera (baseline bx)
    z[:n_near] = rng.uniform(-0.09, -0.05, n_near)
    pts = np.stack([x, y, z, rng.uniform(0, 1, n)], 1).astype(np.float32)
    return pts[rng.permutation(n)]


def conditions(pts, P, H, W):
    v = pts[pts[:, 0] >= 0].astype(np.float64)
    v[:, 3] = 1.0
    q = v @ P.T
    with np.errstate(all="ignore"):
        a, b = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        u, w = np.round(a) - 1, np.round(b) - 1
    keep = (u >= 0) & (w >= 0) & (u < W) & (w < H)
    outside = np.asarray([(u < 0).sum(), (u >= W).sum(), (w < 0).sum(), (w >= H).sum()], dtype=np.int64)      # left, right, above, below
    a, b, u, w, d = a[keep], b[keep], u[keep].astype(int), w[keep].astype(int), q[keep, 2]
    half = min(np.abs(a - np.floor(a) - 0.5).min(), np.abs(b - np.floor(b) - 0.5).min())
    first = {}
    for i, (r, c) in enumerate(zip(w, u)):
        first.setdefault((r, c), i)
    pairs = [(first[(r, W - 1)], first[(r + 1, 0)]) for r in range(H - 1) if (r, W - 1) in first and (r + 1, 0) in first]
    pix = w * W + u
    neg = d < 0
    pos_pix = set(pix[d > 0].tolist())
    return dict(cond_half_dist=np.float64(half), cond_pairs=np.int64(len(pairs)),
                cond_pairs_first_col0=np.int64(sum(b0 < a0 for a0, b0 in pairs)),
                cond_pairs_first_colW=np.int64(sum(a0 < b0 for a0, b0 in pairs)),
                cond_negative=np.int64(neg.sum()), cond_negative_shared=np.int64(sum(p in pos_pix for p in pix[neg].tolist())),
                n_in_bounds=np.int64(keep.sum()), n_behind=np.int64((pts[:, 0] < 0).sum()),
                n_near=np.int64(((pts[:, 0] >= 0) & (pts[:, 0] < 0.3)).sum()),
                n_outside=outside)


def make(ku, tag, seed, W, H, n, cam):
    rng = np.random.default_rng(seed)
    cam2cam, velo2cam = calib_text(rng, W, H)
    pts = scan(rng, n, BASELINE[cam])
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "calib_cam_to_cam.txt"), "w") as f:
            f.write(cam2cam)
        with open(os.path.join(tmp, "calib_velo_to_cam.txt"), "w") as f:
            f.write(velo2cam)
        velo_file = os.path.join(tmp, "0000000000.bin")
        pts.tofile(velo_file)
        np.int = int                                                        # removed from numpy 1.24; the reference still uses it
        depth = ku.generate_depth_map(tmp, velo_file, cam, False)
        depth_vel = ku.generate_depth_map(tmp, velo_file, cam, True)
        c2c = ku.read_calib_file(os.path.join(tmp, "calib_cam_to_cam.txt"))
        v2c = ku.read_calib_file(os.path.join(tmp, "calib_velo_to_cam.txt"))
    # the product the reference forms inside generate_depth_map, from ITS parse of the files
    rigid = np.vstack([np.hstack([v2c["R"].reshape(3, 3), v2c["T"][:, None]]), [0, 0, 0, 1.0]])
    rect = np.identity(4)
    rect[:3, :3] = c2c["R_rect_00"].reshape(3, 3)
    P = np.dot(np.dot(c2c[f"P_rect_0{cam}"].reshape(3, 4), rect), rigid)
    assert depth.shape == (H, W) and depth.dtype == np.float64
    cond = conditions(pts, P, H, W)
    assert cond["cond_half_dist"] >= 1e-9, cond
    assert cond["cond_pairs"] >= 5 and cond["cond_pairs_first_col0"] >= 1 and cond["cond_pairs_first_colW"] >= 1, cond
    assert cond["cond_negative"] >= 10 and cond["cond_negative_shared"] >= 1, cond
    assert cond["n_near"] >= 15 and cond["n_behind"] > 0 and (cond["n_outside"] > 0).all(), cond
    assert cond["n_in_bounds"] >= 2 * H * W, cond                            # many points per pixel
    name = f"lidar_depth_{tag}.npz"
    np.savez_compressed(os.path.join(OUT, name), points=pts, P=P, hw=np.asarray([H, W], dtype=np.int64), cam=np.int64(cam),
                        depth=depth, depth_vel=depth_vel, cam2cam_txt=np.asarray(cam2cam), velo2cam_txt=np.asarray(velo2cam), **cond)
    print(name, os.path.getsize(os.path.join(OUT, name)), "bytes;", "nonzero", int((depth != 0).sum()), "of", H * W,
          {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in cond.items()})


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ku = import_reference(os.path.abspath(sys.argv[1]))
    make(ku, "a", 0, 48, 20, 6000, 2)
    make(ku, "b", 1, 64, 24, 10000, 3)


if __name__ == "__main__":
    main()
