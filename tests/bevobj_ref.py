"""Plain numpy / Python restatement of jp_bev_objects (csrc/bevobj.hip) and of the host arithmetic of BevObjects.objects()
(apis/bevobj.py), for the tests: a breadth-first flood fill in raster order, the min_cells drop, the id order, the twelve fields
with and without a grid, and the metric formulas written out once more (they do not call the package)."""
import math
from collections import deque

import numpy as np

INT_MIN = -2 ** 31
FIELDS = ("cells", "r_min", "r_max", "c_min", "c_max", "sum_r", "sum_c", "first_cell", "edge_mask", "pts", "pts_obst", "hmax_mm")
N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def components(fg, conn):
    """fg: (occ, occ) bool -> list of components in raster order of their first cell, each the list of its cells' linear indices
    (breadth-first from that first cell)"""
    assert conn in (4, 8)
    occ = fg.shape[0]
    assert fg.shape == (occ, occ)
    nb = N8 if conn == 8 else N4
    todo = fg.astype(bool).tolist()
    out = []
    for i in range(occ):
        row = todo[i]
        for j in range(occ):
            if not row[j]:
                continue
            row[j] = False
            cells, queue = [], deque([(i, j)])
            while queue:
                r, c = queue.popleft()
                cells.append(r * occ + c)
                for dr, dc in nb:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < occ and 0 <= cc < occ and todo[rr][cc]:
                        todo[rr][cc] = False
                        queue.append((rr, cc))
            out.append(cells)
    return out


def objects_one(layout, grid, cls_value, conn, min_cells, max_objects):
    """one camera: layout (occ, occ) uint8, grid (4, occ, occ) int32 or None -> labels (occ, occ) int32, count, table (max_objects, 12) int32"""
    occ = layout.shape[0]
    labels = np.full(occ * occ, -1, dtype=np.int32)
    table = np.zeros((max_objects, 12), dtype=np.int64)
    nid = 0
    for cells in components(layout == cls_value, conn):
        if len(cells) < min_cells:
            continue                                                    # dropped before numbering: no id, its cells stay -1
        k = np.asarray(cells, dtype=np.int64)
        labels[k] = nid
        if nid < max_objects:
            r, c = k // occ, k % occ
            edge = (1 if r.min() == 0 else 0) | (2 if r.max() == occ - 1 else 0) | (4 if c.min() == 0 else 0) | (8 if c.max() == occ - 1 else 0)
            pts, pts_obst, hmax = 0, 0, INT_MIN
            if grid is not None:
                n = grid[0].reshape(-1)[k].astype(np.int64)
                pts, pts_obst = int(n.sum()), int(grid[1].reshape(-1)[k].astype(np.int64).sum())
                seen = grid[3].reshape(-1)[k][n > 0]
                hmax = int(seen.max()) if seen.size else INT_MIN
            table[nid] = [len(cells), r.min(), r.max(), c.min(), c.max(), r.sum(), c.sum(), k.min(), edge, pts, pts_obst, hmax]
        nid += 1
    return labels.reshape(occ, occ), nid, table.astype(np.int32)


def objects(layout, grid, cls_value=2, conn=8, min_cells=4, max_objects=64):
    """layout (B, occ, occ) uint8, grid (B, 4, occ, occ) int32 or None -> labels (B, occ, occ), count (B), table (B, max_objects, 12), int32"""
    res = [objects_one(layout[b], None if grid is None else grid[b], cls_value, conn, min_cells, max_objects) for b in range(layout.shape[0])]
    return (np.stack([r[0] for r in res]), np.asarray([r[1] for r in res], dtype=np.int32), np.stack([r[2] for r in res]))


def metrics(row, occ, off, pose=None):
    """the host formulas of one table row, float64: see the header for the cell convention"""
    cells, r_min, r_max, c_min, c_max, sum_r, sum_c, first_cell, edge, pts, pts_obst, hmax = (int(v) for v in row)
    res_f = 40.0 / occ
    x = (sum_c / cells + 0.5 - occ / 2) * res_f
    z = (occ - 0.5 - sum_r / cells) * res_f - off
    out = dict(cells=cells, x=x, z=z, width=(c_max - c_min + 1) * res_f, length=(r_max - r_min + 1) * res_f,
               range=(occ - 1 - r_max) * res_f - off, bearing_deg=math.degrees(math.atan2(x, z)), truncated=edge != 0, points=pts,
               obstacle_points=pts_obst, height=None if hmax == INT_MIN else hmax / 1000.0)
    if pose is not None:
        T = np.asarray(pose, dtype=np.float64).reshape(-1)             # row-major 3 x 4 or 4 x 4
        out["X_w"] = float(T[0] * x + T[2] * z + T[3])
        out["Z_w"] = float(T[8] * x + T[10] * z + T[11])
    return out


def object_list(count, table, occ, off, pose=None):
    """what BevObjects.objects() returns, from the reference's count and table"""
    out = []
    for b in range(table.shape[0]):
        n = min(int(count[b]), table.shape[1])
        out.append([{"id": i, **metrics(table[b, i], occ, off, None if pose is None else pose[b])} for i in range(n)])
    return out


# ---------------------------------------------------------------------------------------- hand-drawn maps shared by the tests
def serpentine(occ, v=2):
    """one-cell-wide path: every even row full, every odd row one cell at alternating ends -- it crosses every row seam"""
    m = np.zeros((occ, occ), dtype=np.uint8)
    m[0::2] = v
    for i in range(1, occ, 2):
        m[i, occ - 1 if (i // 2) % 2 == 0 else 0] = v
    return m


def spiral(occ, v=2):
    """a one-cell-wide square spiral with one-cell gaps, from (0, 0) inwards: right, down, left by occ - 1, then up and right by
    occ - 3, down and left by occ - 5, ..."""
    m = np.zeros((occ, occ), dtype=np.uint8)
    r = c = 0
    m[0, 0] = v
    length, turn = occ - 1, 0
    while length > 0:
        dr, dc = ((0, 1), (1, 0), (0, -1), (-1, 0))[turn % 4]
        for _ in range(length):
            r, c = r + dr, c + dc
            m[r, c] = v
        turn += 1
        if turn >= 3 and turn % 2 == 1:
            length -= 2
    return m


def u_shape(occ, v=2):
    """two arms in columns 1 and occ-2 from row 1 down, joined only in the last row; the left arm's top (1, 1) is the first cell"""
    m = np.zeros((occ, occ), dtype=np.uint8)
    m[1:, 1] = v
    m[2:, occ - 2] = v
    m[occ - 1, 1:occ - 1] = v
    return m


def stairs(occ, v=2):
    """the main diagonal: joined only by corners -- one object at conn 8, occ single cells at conn 4"""
    m = np.zeros((occ, occ), dtype=np.uint8)
    m[np.arange(occ), np.arange(occ)] = v
    return m


def checkerboard(occ, v=2):
    i, j = np.mgrid[0:occ, 0:occ]
    return np.where((i + j) % 2 == 0, v, 0).astype(np.uint8)


def corners(occ, v=2):
    m = np.zeros((occ, occ), dtype=np.uint8)
    m[0, 0] = m[0, occ - 1] = m[occ - 1, 0] = m[occ - 1, occ - 1] = v
    return m


def random_map(occ, density, cls_value, seed):
    """three classes: `density` of the cells hold cls_value, the rest is split between the two other classes of 0 / 1 / 2"""
    rng = np.random.default_rng(seed)
    others = [c for c in (0, 1, 2) if c != cls_value]
    m = np.asarray(others, dtype=np.uint8)[rng.integers(0, 2, size=(occ, occ))]
    m[rng.random((occ, occ)) < density] = cls_value
    return m


def random_grid(B, occ, seed):
    """(B, 4, occ, occ) int32: n in 0..5 with many zeros, n_obst <= n, heights of either sign -- also in the cells with n == 0,
    where the lift would leave INT_MAX / INT_MIN: their hmax_mm must not be read"""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 6, size=(B, occ, occ)) * (rng.random((B, occ, occ)) < 0.5)
    n_obst = (rng.integers(0, 6, size=(B, occ, occ)) % (n + 1))
    hmax = rng.integers(-900, 3000, size=(B, occ, occ))
    hmin = hmax - rng.integers(0, 500, size=(B, occ, occ))
    return np.stack([n, n_obst, hmin, hmax], axis=1).astype(np.int32)
