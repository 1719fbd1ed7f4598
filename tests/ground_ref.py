"""numpy restatement of csrc/ground.hip (jp_ground_fit) for the tests.  The gating of the moments kernel is one elementwise float64
numpy operation per operation of the kernel, in the order include/jperceiver_hip.h states, so each is rounded once as the kernel's
__dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn are; the ten sums are int64 (exact, order-free); the solve is float64 scalars in the
header's order (+ - x / sqrt are correctly rounded in numpy as the kernel's _rn intrinsics are).  Results compare with
np.array_equal."""
import math

import numpy as np

NS = 10
NAN = float("nan")


def inliers(depth, cam, gate, layout, occ, res_f, off, min_range, max_range, band):
    """depth (H, W) float32, cam (8,) (only fx, fy, cx, cy are read), gate (4,) [nx, ny, nz, h], layout (occ, occ) uint8 or None
    -> (ok (H, W) bool, X, Y, d (H, W) float64)"""
    H, W = depth.shape
    f = np.float64
    fx, fy, cx, cy = (f(x) for x in cam[:4])
    nx, ny, nz, h = (f(x) for x in gate)
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        d = depth.astype(np.float64)
        ok = (d >= f(min_range)) & (d <= f(max_range))
        X = u - cx
        X = X / fx
        X = X * d
        Y = v - cy
        Y = Y / fy
        Y = Y * d
        ok &= (np.abs(X) <= f(max_range)) & (np.abs(Y) <= f(max_range))
        a = nx * X
        b = ny * Y
        s = a + b
        c = nz * d
        s = s + c
        r = h - s
        ok &= (r >= -f(band)) & (r <= f(band))
        if layout is not None:
            uu = X / f(res_f)
            uu = uu + f(occ) * 0.5
            vv = d + f(off)
            vv = vv / f(res_f)
            ok &= (uu >= 0) & (uu < occ) & (vv >= 0) & (vv < occ)
            j = np.where(ok, np.floor(np.where(ok, uu, 0.0)), 0).astype(np.int64)
            i = occ - 1 - np.where(ok, np.floor(np.where(ok, vv, 0.0)), 0).astype(np.int64)
            ok &= layout[i, j] == 1
    return ok, X, Y, d


def moments(depth, cam, gate, layout, occ, res_f, off, min_range, max_range, band):
    """-> (10,) int64 [n, Sx, Sy, Sz, Sxx, Sxz, Szz, Sxy, Szy, Syy] in integer millimetres"""
    ok, X, Y, d = inliers(depth, cam, gate, layout, occ, res_f, off, min_range, max_range, band)

    def q(a):
        a = a[ok] * np.float64(1000.0)
        a = a + 0.5
        return np.floor(a).astype(np.int64)

    qx, qy, qz = q(X), q(Y), q(d)
    return np.array([qx.size, qx.sum(), qy.sum(), qz.sum(), (qx * qx).sum(), (qx * qz).sum(), (qz * qz).sum(), (qx * qy).sum(),
                     (qz * qy).sum(), (qy * qy).sum()], dtype=np.int64)


def solve(mom, min_points, min_spread, max_tilt_deg, h_lo, h_hi):
    """mom (10,) int64 -> (status, plane (4,) float64 or None, rms); the header's order, float64 scalars"""
    f = np.float64
    n = int(mom[0])
    if n < min_points:
        return 1, None, NAN
    with np.errstate(all="ignore"):
        N = f(n)
        Sx, Sy, Sz, Sxx, Sxz, Szz, Sxy, Szy, Syy = (f(int(x)) for x in mom[1:])
        mx, my, mz = Sx / N, Sy / N, Sz / N
        cxx = Sxx / N - mx * mx
        cxz = Sxz / N - mx * mz
        czz = Szz / N - mz * mz
        cxy = Sxy / N - mx * my
        czy = Szy / N - mz * my
        cyy = Syy / N - my * my
        det = cxx * czz - cxz * cxz
        t = f(1000.0) * f(min_spread)
        sp = t * t
        if not (cxx >= sp and czz >= sp and det >= f(0.01) * (cxx * czz)):
            return 2, None, NAN
        a = (cxy * czz - czy * cxz) / det
        b = (czy * cxx - cxy * cxz) / det
        c = my - (a * mx + b * mz)
        s = np.sqrt((a * a + f(1.0)) + b * b)
        plane = np.array([-a / s, f(1.0) / s, -b / s, (c / f(1000.0)) / s], dtype=np.float64)
        e = cyy - (a * cxy + b * czy)
        rms = (np.sqrt(e if e > 0.0 else f(0.0)) / s) / f(1000.0)
    cos_tilt = math.cos(max_tilt_deg * (math.pi / 180.0))
    if not (np.isfinite(plane).all() and np.isfinite(rms)) or plane[1] < cos_tilt or not (plane[3] >= h_lo and plane[3] <= h_hi):
        return 3, None, NAN
    return 0, plane, float(rms)


def fit(depth, layout, prior, cam, occ, res_f, off, min_range, max_range, band, rounds=2, min_points=200, min_spread=0.5,
        max_tilt_deg=10.0, h_lo=0.5, h_hi=4.0):
    """jp_ground_fit.  depth (B, 1, H, W) or (B, H, W) float32; layout (B, occ, occ) uint8 or None; prior (B, 4) or None (tracking: the
    plane in cam); cam (B, 8) float64, not modified.  -> (cam (B, 8) with the result in [:, 4:], mom (B, 10) int64, stat (B, 3))"""
    B = cam.shape[0]
    depth = np.asarray(depth, dtype=np.float32).reshape(B, depth.shape[-2], depth.shape[-1])
    cam = np.array(cam, dtype=np.float64)
    mom = np.zeros((B, NS), dtype=np.int64)
    stat = np.zeros((B, 3), dtype=np.float64)
    for b in range(B):
        for r in range(rounds):
            first = prior is not None and r == 0
            gate = prior[b] if first else cam[b, 4:]
            mom[b] = moments(depth[b], cam[b], gate, None if layout is None else layout[b], occ, res_f, off, min_range, max_range, band)
            status, plane, rms = solve(mom[b], min_points, min_spread, max_tilt_deg, h_lo, h_hi)
            if status == 0:
                cam[b, 4:] = plane
            elif first:
                cam[b, 4:] = prior[b]
            stat[b] = [status, float(mom[b, 0]), rms]
    return cam, mom, stat
