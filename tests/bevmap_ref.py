"""float64 numpy restatement of csrc/bevmap.hip for the tests: the gather of jp_bev_fuse over the WHOLE map (no window: a window
that missed a cell would show), the class rule of jp_bev_map_classes and the marks of jp_bev_map_mark.  Every operation of the
gather is one numpy operation on float64 arrays, in the order include/jperceiver_hip.h states, so each is rounded once as the
kernel's __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn are and the results compare with torch.equal."""
import numpy as np

PALETTE = {0: (0, 0, 0), 1: (255, 255, 255), 2: (0, 0, 255), 255: (96, 96, 96)}


def fuse_one(counts, layout, T, occ, res_f, off, max_range, res, org_r, org_c):
    """counts (3, Mh, Mw) int32, updated in place; layout (occ, occ) uint8; T: the 12 or 16 doubles of a pose, row-major."""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    t00, t02, t03, t20, t22, t23 = T[0], T[2], T[3], T[8], T[10], T[11]
    _, Mh, Mw = counts.shape
    f = np.float64
    with np.errstate(all="ignore"):
        det = f(t00 * t22) - f(t02 * t20)
        if not (np.abs(det) >= 1e-6):
            return
        c = np.arange(Mw, dtype=np.float64)[None, :]
        r = np.arange(Mh, dtype=np.float64)[:, None]
        X = ((c + 0.5) - f(org_c)) * f(res)
        Z = ((f(org_r) - r) - 0.5) * f(res)
        dX = X - t03
        dZ = Z - t23
        a = t22 * dX
        b = t02 * dZ
        x = (a - b) / det
        a = t00 * dZ
        b = t20 * dX
        z = (a - b) / det
        u = x / f(res_f)
        u = u + f(occ) * 0.5
        v = z + f(off)
        v = v / f(res_f)
        hit = (u >= 0) & (u < occ) & (v >= 0) & (v < occ) & (z <= f(max_range))
    hit = np.broadcast_to(hit, (Mh, Mw))
    u = np.broadcast_to(u, (Mh, Mw))[hit]
    v = np.broadcast_to(v, (Mh, Mw))[hit]
    j = np.floor(u).astype(np.int64)
    i = occ - 1 - np.floor(v).astype(np.int64)
    cls = layout[i, j]
    counts[0][hit] += 1
    counts[1][hit] += (cls == 1).astype(np.int32)
    counts[2][hit] += (cls == 2).astype(np.int32)


def fuse(counts, layouts, poses, occ, res_f, off, max_range, res, org_r, org_c):
    """counts (B, 3, Mh, Mw) int32 in place; layouts (B, N, occ, occ) uint8; poses (B, N, 12 | 16) float64."""
    B, N = layouts.shape[:2]
    for b in range(B):
        for n in range(N):
            fuse_one(counts[b], layouts[b, n], poses[b, n], occ, res_f, off, max_range, res, org_r, org_c)
    return counts


def classes(counts, min_seen=1.0, road_frac=0.5, car_frac=0.5):
    """counts (B, 3, Mh, Mw) -> (cls (B, Mh, Mw) uint8, rgb (B, Mh, Mw, 3) uint8)"""
    seen, road, car = (counts[:, k].astype(np.float64) for k in range(3))
    cls = np.zeros(seen.shape, dtype=np.uint8)
    cls[(road + car) >= np.float64(road_frac) * seen] = 1
    cls[car >= np.float64(car_frac) * seen] = 2
    cls[seen < np.float64(min_seen)] = 255
    rgb = np.zeros(cls.shape + (3,), dtype=np.uint8)
    for k, col in PALETTE.items():
        rgb[cls == k] = col
    return cls, rgb


def cell_of(X, Z, res, org_r, org_c):
    """(row, col) as floats (floor taken, not yet bounded): the map cell that holds world (X, Z)"""
    with np.errstate(all="ignore"):
        return np.floor(np.float64(org_r) - np.float64(Z) / np.float64(res)), np.floor(np.float64(X) / np.float64(res) + np.float64(org_c))


def mark(rgb, traj, n, res, org_r, org_c, color):
    """rgb (B, Mh, Mw, 3) in place; traj (B, capacity, 12); color (R, G, B)"""
    B, Mh, Mw, _ = rgb.shape
    for b in range(B):
        for k in range(n):
            fr, fc = cell_of(traj[b, k, 3], traj[b, k, 11], res, org_r, org_c)
            if fc >= 0 and fc < Mw and fr >= 0 and fr < Mh:
                rgb[b, int(fr), int(fc)] = color
    return rgb


def yaw_pose(deg, tx=0.0, tz=0.0):
    """4 x 4 camera-to-world transform of a yaw about the y axis by a multiple of 90 degrees, with EXACT 0 / +-1 entries"""
    k = (int(deg) // 90) % 4
    assert deg % 90 == 0
    cs = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][k]
    T = np.identity(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = cs[0], cs[1], -cs[1], cs[0]
    T[0, 3], T[2, 3] = tx, tz
    return T


def general_pose(rng, max_t):
    """yaw anywhere, pitch and roll <= 0.1 rad, translation up to max_t metres in x and z"""
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    T = np.identity(4)
    T[:3, :3] = Ry @ Rx @ Rz
    T[0, 3], T[1, 3], T[2, 3] = rng.uniform(-max_t, max_t), rng.uniform(-1, 1), rng.uniform(-max_t, max_t)
    return T
