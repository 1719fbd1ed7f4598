"""float64 numpy restatement of csrc/depthbev.hip for the tests: the lift of jp_depth_bev_lift, the class rule of
jp_depth_bev_classes and the table of jp_bev_agree.  Every operation of the lift is one elementwise numpy operation on float64
arrays, in the order include/jperceiver_hip.h states, so each is rounded once as the kernel's __dmul_rn / __dadd_rn / __dsub_rn /
__ddiv_rn are and the results compare with np.array_equal."""
import numpy as np

INT_MAX, INT_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
NOT_OBSERVED = 255


def empty_grid(B, occ):
    g = np.zeros((B, 4, occ, occ), dtype=np.int32)
    g[:, 2], g[:, 3] = INT_MAX, INT_MIN
    return g


def cam_rows(B, fx, fy, cx, cy, plane=(0.0, 1.0, 0.0, 1.73)):
    """(B, 8) float64 [fx, fy, cx, cy, nx, ny, nz, h], the same row for every camera"""
    return np.tile(np.array([fx, fy, cx, cy, *plane], dtype=np.float64), (B, 1))


def cells_of(depth, cam, occ, res_f, off, min_range, max_range, h_min, h_max):
    """depth (H, W) float32, cam (8,) -> (ok (H, W) bool, i, j int64 (H, W) -- valid where ok --, hgt (H, W) float64)"""
    H, W = depth.shape
    f = np.float64
    fx, fy, cx, cy, nx, ny, nz, h = (f(x) for x in cam)
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
        a = nx * X
        b = ny * Y
        s = a + b
        c = nz * d
        s = s + c
        hgt = h - s
        ok &= (hgt >= f(h_min)) & (hgt <= f(h_max))
        uu = X / f(res_f)
        uu = uu + f(occ) * 0.5
        vv = d + f(off)
        vv = vv / f(res_f)
        ok &= (uu >= 0) & (uu < occ) & (vv >= 0) & (vv < occ)
        j = np.where(ok, np.floor(np.where(ok, uu, 0.0)), 0).astype(np.int64)
        i = occ - 1 - np.where(ok, np.floor(np.where(ok, vv, 0.0)), 0).astype(np.int64)
    return ok, i, j, hgt


def lift(grid, depth, cam, occ, res_f, off, min_range, max_range, h_min, h_max, obst_h, accumulate=False):
    """grid (B, 4, occ, occ) int32 in place; depth (B, 1, H, W) or (B, H, W) float32; cam (B, 8) float64"""
    B = grid.shape[0]
    depth = np.asarray(depth, dtype=np.float32).reshape(B, depth.shape[-2], depth.shape[-1])
    if not accumulate:
        grid[:] = empty_grid(B, occ)
    for b in range(B):
        ok, i, j, hgt = cells_of(depth[b], cam[b], occ, res_f, off, min_range, max_range, h_min, h_max)
        i, j, hg = i[ok], j[ok], hgt[ok]
        q = hg * np.float64(1000.0)
        q = q + 0.5
        q = np.floor(q).astype(np.int64).astype(np.int32)
        np.add.at(grid[b, 0], (i, j), 1)
        np.add.at(grid[b, 1], (i, j), (hg > np.float64(obst_h)).astype(np.int32))
        np.minimum.at(grid[b, 2], (i, j), q)
        np.maximum.at(grid[b, 3], (i, j), q)
    return grid


def keys(depth, cam, occ, res_f, off, min_range, max_range, h_min, h_max):
    """(B, H, W) int64: the cell index i * occ + j of every pixel, -1 where it is rejected (the key a lane of the kernel carries)"""
    B = cam.shape[0]
    depth = np.asarray(depth, dtype=np.float32).reshape(B, depth.shape[-2], depth.shape[-1])
    out = []
    for b in range(B):
        ok, i, j, _ = cells_of(depth[b], cam[b], occ, res_f, off, min_range, max_range, h_min, h_max)
        out.append(np.where(ok, i * occ + j, -1))
    return np.stack(out)


def classes(grid, min_points=1, obst_points=2):
    """grid (B, 4, occ, occ) -> (cls (B, occ, occ) uint8, height (B, occ, occ) float32 with NaN where cls is 255)"""
    n, no, hmax = grid[:, 0], grid[:, 1], grid[:, 3]
    cls = np.full(n.shape, 1, dtype=np.uint8)
    cls[no >= obst_points] = 2
    cls[n < min_points] = NOT_OBSERVED
    height = hmax.astype(np.float32) / np.float32(1000.0)
    height[cls == NOT_OBSERVED] = np.nan
    return cls, height


def agree(lifted, layout):
    """lifted, layout (B, ...) uint8 -> (B, 2, 3) int32"""
    B = lifted.shape[0]
    a, l = lifted.reshape(B, -1), layout.reshape(B, -1)
    out = np.zeros((B, 2, 3), dtype=np.int32)
    for x in (1, 2):
        for c in (0, 1, 2):
            out[:, x - 1, c] = ((a == x) & (l == c)).sum(1)
    return out
