"""Plain numpy / Python restatement of jp_bev_tracks (csrc/bevtrack.hip) for the tests: loops over the cells, a sequential greedy loop,
and the float64 arithmetic one operation per line in the header's order (np.float64 scalars: every operation is rounded once).  It
shares no code with the package.  State and outputs have the layouts the header gives them."""
import math

import numpy as np

F = np.float64


def zero_state(B, occ, M):
    """no history"""
    return {"prev_labels": np.zeros((B, occ, occ), dtype=np.int32), "state_i": np.zeros((B, 2 + 2 * M), dtype=np.int32),
            "state_d": np.zeros((B, 12 + 2 * M), dtype=np.float64)}


def _six(T):
    T = np.asarray(T, dtype=np.float64).reshape(-1)                     # row-major 3 x 4 or 4 x 4
    return T[0], T[2], T[3], T[8], T[10], T[11]


def prev_cell(i, j, occ, res_f, off, T6, P6, det):
    """the cell of the previous camera's map that the centre of current cell (i, j) falls into, or None"""
    t00, t02, t03, t20, t22, t23 = T6
    p00, p02, p03, p20, p22, p23 = P6
    docc = F(occ)
    hocc = F(0.5) * docc
    x = F(j) + F(0.5)
    x = x - hocc
    x = x * res_f
    z = docc - F(0.5)
    z = z - F(i)
    z = z * res_f
    z = z - off
    a = t00 * x
    b = t02 * z
    X = a + b
    X = X + t03
    a = t20 * x
    b = t22 * z
    Z = a + b
    Z = Z + t23
    dX = X - p03
    dZ = Z - p23
    a = p22 * dX
    b = p02 * dZ
    xp = a - b
    xp = xp / det
    a = p00 * dZ
    b = p20 * dX
    zp = a - b
    zp = zp / det
    u = xp / res_f
    u = u + hocc
    v = zp + off
    v = v / res_f
    if not (u >= 0.0 and u < docc and v >= 0.0 and v < docc):
        return None
    return occ - 1 - int(math.floor(v)), int(math.floor(u))


def overlap_one(labels, prev_labels, n_prev, T, P, M, reach, off):
    """(M, M) int64: overlap[p][c]"""
    occ = labels.shape[0]
    ov = np.zeros((M, M), dtype=np.int64)
    n_prev = min(max(int(n_prev), 0), M)
    if n_prev == 0:
        return ov
    T6, P6 = _six(T), _six(P)
    with np.errstate(all="ignore"):
        a = P6[0] * P6[4]
        b = P6[1] * P6[3]
        det = a - b
        if not (abs(det) >= 1e-6):
            return ov
        if not all(np.isfinite(t) for t in T6):
            return ov
        res_f = F(40.0) / F(occ)
        off = F(off)
        cur, prev = labels.tolist(), prev_labels.tolist()
        for i in range(occ):
            for j in range(occ):
                c = cur[i][j]
                if not 0 <= c < M:
                    continue
                cell = prev_cell(i, j, occ, res_f, off, T6, P6, det)
                if cell is None:
                    continue
                for di in range(-reach, reach + 1):
                    for dj in range(-reach, reach + 1):
                        ii, jj = cell[0] + di, cell[1] + dj
                        if 0 <= ii < occ and 0 <= jj < occ and 0 <= prev[ii][jj] < n_prev:
                            ov[prev[ii][jj], c] += 1
    return ov


def greedy(ov, n_prev, n_cur, min_overlap):
    """the sequential definition: -> {c: (p, overlap)}"""
    used_p, match = set(), {}
    while True:
        best = None
        for p in range(n_prev):
            if p in used_p:
                continue
            for c in range(n_cur):
                if c in match:
                    continue
                if best is None or ov[p, c] > best[0]:                  # strictly greater: ties stay with the smaller p, then c
                    best = (int(ov[p, c]), p, c)
        if best is None or best[0] < min_overlap:
            return match
        used_p.add(best[1])
        match[best[2]] = (best[1], best[0])


def centroid_world(row, occ, off, T):
    t00, t02, t03, t20, t22, t23 = _six(T)
    res_f = F(40.0) / F(occ)
    docc = F(occ)
    hocc = F(0.5) * docc
    n, sr, sc = F(int(row[0])), F(int(row[5])), F(int(row[6]))
    x = sc / n
    x = x + F(0.5)
    x = x - hocc
    x = x * res_f
    z = sr / n
    z = (docc - F(0.5)) - z
    z = z * res_f
    z = z - F(off)
    a = t00 * x
    b = t02 * z
    X = a + b
    X = X + t03
    a = t20 * x
    b = t22 * z
    Z = a + b
    Z = Z + t23
    return X, Z


def step_one(labels, count, table, pose, prev_labels, state_i, state_d, M, reach, min_overlap, off):
    """one camera, one frame -> tracks (M, 4) int32, kin (M, 4) float64, stats (4) int32, and the rolled state"""
    occ = labels.shape[0]
    n_prev, next_id, n_cur = min(max(int(state_i[0]), 0), M), int(state_i[1]), min(max(int(count), 0), M)
    ov = overlap_one(labels, prev_labels, n_prev, pose, state_d[:12], M, reach, off)
    match = greedy(ov, n_prev, n_cur, min_overlap)
    tracks = np.tile(np.array([-1, 0, -1, 0], dtype=np.int32), (M, 1))
    kin = np.zeros((M, 4), dtype=np.float64)
    new_i, new_d = np.zeros_like(state_i), np.zeros_like(state_d)
    born = 0
    with np.errstate(all="ignore"):
        for c in range(n_cur):
            X, Z = centroid_world(table[c], occ, off, pose)
            if c in match:
                p, o = match[c]
                tracks[c] = [state_i[2 + 2 * p], state_i[3 + 2 * p] + 1, p, o]
                kin[c] = [X, Z, X - state_d[12 + 2 * p], Z - state_d[13 + 2 * p]]
            else:
                tracks[c] = [next_id + born, 1, -1, 0]
                kin[c] = [X, Z, 0.0, 0.0]
                born += 1
            new_i[2 + 2 * c], new_i[3 + 2 * c] = tracks[c, 0], tracks[c, 1]
            new_d[12 + 2 * c], new_d[13 + 2 * c] = X, Z
    new_i[0], new_i[1] = n_cur, next_id + born
    new_d[:12] = np.asarray(pose, dtype=np.float64).reshape(-1)[:12]
    stats = np.array([n_cur, len(match), born, n_prev - len(match)], dtype=np.int32)
    return tracks, kin, stats, labels.astype(np.int32).copy(), new_i, new_d


def step(labels, count, table, pose, state, M, reach=1, min_overlap=1, off=0.27):
    """labels (B, occ, occ), count (B), table (B, M, 12), pose (B, 12 | 16 | 4, 4), state: zero_state's dict (left unchanged)
    -> tracks (B, M, 4), kin (B, M, 4), stats (B, 4), the new state"""
    B = labels.shape[0]
    res = [step_one(labels[b], count[b], table[b], np.asarray(pose[b]).reshape(-1), state["prev_labels"][b], state["state_i"][b],
                    state["state_d"][b], M, reach, min_overlap, off) for b in range(B)]
    new = {"prev_labels": np.stack([r[3] for r in res]), "state_i": np.stack([r[4] for r in res]), "state_d": np.stack([r[5] for r in res])}
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]), new


# ---------------------------------------------------------------------------------------- scenes shared by the tests
def pose(theta_deg=0.0, tx=0.0, tz=0.0):
    """a 4 x 4 camera-to-world transform that turns by theta about the vertical axis and then shifts by (tx, tz) in the x-z plane"""
    c, s = math.cos(math.radians(theta_deg)), math.sin(math.radians(theta_deg))
    return np.array([[c, 0.0, s, tx], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, tz], [0.0, 0.0, 0.0, 1.0]])


def shift(m, di, dj, fill=0):
    """the map moved by di rows and dj columns; what leaves the map is lost, what enters is `fill`"""
    occ = m.shape[0]
    out = np.full_like(m, fill)
    out[max(di, 0):occ + min(di, 0), max(dj, 0):occ + min(dj, 0)] = m[max(-di, 0):occ + min(-di, 0), max(-dj, 0):occ + min(-dj, 0)]
    return out


def draw(rows, v=2):
    return np.array([[v if ch == "#" else 0 for ch in r] for r in rows], dtype=np.uint8)
