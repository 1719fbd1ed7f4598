"""jp_bev_objects (csrc/bevobj.hip) against the breadth-first reference of tests/bevobj_ref.py.  Everything is integer: labels, count
and table are compared byte for byte (tolerance 0).  Before every call the outputs AND the scratch are filled with 0x7f bytes -- what
comes back equal to the reference was written by the call -- and every call is made twice and the two results compared bit for bit.

The shapes are the smallest at which the labelling can go wrong: occ 37 and 65 (no wave width, run length or span of the numbering
kernel divides them; a wave's 64 cells straddle rows and, with two cameras, the border between the cameras), always two cameras with
different maps.  Geometric maps: a one-cell-wide serpentine that crosses every row seam at alternating ends, a spiral, a U whose arms
join only in the last row, stairs joined only by corners (one object at conn 8; occ objects at conn 4, more than the max_objects = 16
of these cases: count is the full number, the table holds the first 16, labels hold every id), a checkerboard, all foreground, all
background, single cells in the four corners with min_cells 1 and 2 -- each at both connectivities, without a grid and with a random
one (points in about half the cells, heights of either sign, so that some objects have no point at all: the INT_MIN sentinel).
Random three-class maps at densities 0.3, 0.5, 0.59 (the site-percolation threshold at conn 4: the longest union chains) and 0.7, at
occ 64 and 256, both connectivities, cls_value 1 and 2, min_cells 1 and 4, max_objects 64 and 4096.  Two sizes at which the code takes
another path or an index could overflow: occ 300 (past 256 the numbering kernel reads part of its span twice) and all foreground at
occ 1024, the limit (sum_r at its largest).  BevObjects.objects() against
the reference's host formulas: == for the integers, 1e-12 absolute for the float64 metric values (float64 on both sides, they differ
at most in operation order), with a quarter-turn pose and a translation for X_w, Z_w."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import _lib, ops                                               # noqa: E402
from jperceiver_amd.apis import BevObjects                                         # noqa: E402
from tests import bevobj_ref as R                                                  # noqa: E402

DEV = "cuda"
INT_MIN = -2 ** 31
GEOMETRIC = {
    "serpentine": R.serpentine, "spiral": R.spiral, "u_shape": R.u_shape, "stairs": R.stairs, "checkerboard": R.checkerboard,
    "full": lambda occ: np.full((occ, occ), 2, dtype=np.uint8), "empty": lambda occ: np.zeros((occ, occ), dtype=np.uint8),
    "corners": R.corners,
}
DENSITIES = (0.3, 0.5, 0.59, 0.7)


def _poisoned(shape, dtype):
    return torch.full(shape, 0x7f, device=DEV, dtype=torch.uint8).view(dtype) if dtype != torch.uint8 else torch.full(shape, 0x7f, device=DEV, dtype=dtype)


def _call(layout, grid, cls_value, conn, min_cells, max_objects):
    """one jp_bev_objects call on poisoned outputs and scratch -> labels, count, table as numpy"""
    B, occ = layout.shape[0], layout.shape[1]
    labels = _poisoned((B, occ, occ * 4), torch.int32)
    count = _poisoned((B * 4,), torch.int32)
    table = _poisoned((B, max_objects, 12 * 4), torch.int32)
    ws = _poisoned((int(_lib.lib().fn["jp_bev_objects_ws_bytes"](B, occ)),), torch.uint8)
    assert labels.shape == (B, occ, occ) and count.shape == (B,) and table.shape == (B, max_objects, 12) and int(count[0]) == 0x7f7f7f7f
    ops.call("jp_bev_objects", layout, grid, labels, count, table, ws, B, occ, cls_value, conn, min_cells, max_objects)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), count.cpu().numpy(), table.cpu().numpy()


def _check(layout, grid, cls_value, conn, min_cells, max_objects, want, what):
    lay = torch.from_numpy(layout).to(DEV)
    g = None if grid is None else torch.from_numpy(grid).to(DEV)
    a = _call(lay, g, cls_value, conn, min_cells, max_objects)
    b = _call(lay, g, cls_value, conn, min_cells, max_objects)
    for name, x, y, w in zip(("labels", "count", "table"), a, b, want):
        assert x.dtype == w.dtype == np.int32 and x.shape == w.shape, (what, name)
        assert x.tobytes() == y.tobytes(), (what, name, "two runs differ")
        if x.tobytes() != w.tobytes():
            bad = np.argwhere(x != w)
            raise AssertionError(f"{what}: {name} differs from the reference at {len(bad)} places, first {bad[0].tolist()}: "
                                 f"got {x[tuple(bad[0])]}, want {w[tuple(bad[0])]}")


@functools.lru_cache(maxsize=None)
def _geometric(name, occ):
    """camera 0: the named map; camera 1: the next map of the list, mirrored left-right -- different maps per camera"""
    names = list(GEOMETRIC)
    other = GEOMETRIC[names[(names.index(name) + 1) % len(names)]](occ)[:, ::-1]
    layout = np.ascontiguousarray(np.stack([GEOMETRIC[name](occ), other]))
    grid = R.random_grid(2, occ, seed=occ + names.index(name))
    return layout, grid


@functools.lru_cache(maxsize=None)
def _geometric_ref(name, occ, conn, min_cells, with_grid):
    layout, grid = _geometric(name, occ)
    return R.objects(layout, grid if with_grid else None, 2, conn, min_cells, 16)


@pytest.mark.parametrize("occ", [37, 65])
@pytest.mark.parametrize("name", list(GEOMETRIC))
def test_geometric_maps_equal_the_reference(name, occ):
    layout, grid = _geometric(name, occ)
    for conn in (4, 8):
        for min_cells in ((1, 2) if name == "corners" else (1,)):
            for with_grid in (False, True):
                want = _geometric_ref(name, occ, conn, min_cells, with_grid)
                _check(layout, grid if with_grid else None, 2, conn, min_cells, 16, want, (name, occ, conn, min_cells, with_grid))
    # what the maps are there to show, on the reference (the GPU equals it)
    lab, cnt, tab = _geometric_ref(name, occ, 8, 1, True)
    lab4, cnt4, tab4 = _geometric_ref(name, occ, 4, 1, True)
    if name in ("serpentine", "spiral", "u_shape", "full"):
        assert cnt[0] == cnt4[0] == 1
    if name == "u_shape":
        assert tab[0, 0, 7] == occ + 1
    if name == "stairs":
        assert cnt[0] == 1 and cnt4[0] == occ > 16 and lab4[0].max() == occ - 1 and tab4[0, 15, 7] == 15 * occ + 15
    if name == "checkerboard":
        assert cnt[0] == 1 and cnt4[0] == (occ * occ + 1) // 2
    if name == "empty":
        assert cnt[0] == 0 and (lab[0] == -1).all() and (tab[0] == 0).all()
    if name == "corners":
        assert cnt[0] == 4 and tab[0, :4, 8].tolist() == [5, 9, 6, 10] and (tab[0, 4:] == 0).all()
        two = _geometric_ref(name, occ, 8, 2, True)
        assert two[1][0] == 0 and (two[0][0] == -1).all() and (two[2][0] == 0).all()


def test_geometric_grids_exercise_the_sentinel():
    # some object of the cases above has no lifted point at all (hmax_mm = INT_MIN next to a non-zero grid), others have points
    tab = _geometric_ref("corners", 37, 8, 1, True)[2]
    tab4 = _geometric_ref("stairs", 65, 4, 1, True)[2]
    rows = np.concatenate([tab[0, :4], tab4[0, :16]])
    assert (rows[:, 11] == INT_MIN).any() and (rows[:, 11] != INT_MIN).any() and (rows[rows[:, 11] == INT_MIN, 9] == 0).all()
    assert (rows[:, 11] < 0).any() or (tab4[1, :, 11] < 0).any()        # heights of either sign


# ---------------------------------------------------------------------------------------- random maps
def _variants(di):
    """(cls_value, min_cells, max_objects, with_grid) per density index: every value of each appears at both occ and both conn"""
    return ((1, 1, 64, False), (2, 4, 4096, True)) if di % 2 == 0 else ((1, 4, 4096, True), (2, 1, 64, False))


@functools.lru_cache(maxsize=None)
def _random(occ, di, cls_value):
    layout = np.stack([R.random_map(occ, DENSITIES[di], cls_value, seed=1000 * occ + 10 * di + cam) for cam in (0, 1)])
    return layout, R.random_grid(2, occ, seed=7 * occ + di)


@functools.lru_cache(maxsize=None)
def _random_ref(occ, di, conn, variant):
    cls_value, min_cells, max_objects, with_grid = _variants(di)[variant]
    layout, grid = _random(occ, di, cls_value)
    return R.objects(layout, grid if with_grid else None, cls_value, conn, min_cells, max_objects)


def test_random_256_cases_at_4096_rows_are_not_all_in_overflow():
    seen = []
    for di in range(len(DENSITIES)):
        for conn in (4, 8):
            for v, (cls_value, min_cells, max_objects, _) in enumerate(_variants(di)):
                if max_objects == 4096:
                    seen += _random_ref(256, di, conn, v)[1].tolist()
    print("kept components of the 256 x 256 cases with 4096 rows:", seen)
    assert len(seen) == 16 and any(c <= 4096 for c in seen) and all(c > 0 for c in seen)


@pytest.mark.parametrize("occ", [64, 256])
@pytest.mark.parametrize("di", range(len(DENSITIES)))
def test_random_maps_equal_the_reference(di, occ):
    for conn in (4, 8):
        for v, (cls_value, min_cells, max_objects, with_grid) in enumerate(_variants(di)):
            layout, grid = _random(occ, di, cls_value)
            want = _random_ref(occ, di, conn, v)
            print(f"occ {occ} density {DENSITIES[di]} conn {conn} cls {cls_value} min_cells {min_cells} max_objects {max_objects}: "
                  f"kept {want[1].tolist()}")
            _check(layout, grid if with_grid else None, cls_value, conn, min_cells, max_objects, want,
                   (occ, DENSITIES[di], conn, cls_value, min_cells, max_objects))


@functools.lru_cache(maxsize=None)
def _past_256():
    layout = np.stack([R.serpentine(300), R.random_map(300, 0.55, 2, seed=300)])
    grid = R.random_grid(2, 300, seed=301)
    return layout, grid, {conn: R.objects(layout, grid, 2, conn, 2, 64) for conn in (4, 8)}


def test_occ_300_where_the_numbering_kernel_sweeps_its_tail_chunks_twice():
    # up to occ 256 a wave of the numbering kernel keeps the flags of its whole span in registers; beyond, the rest is read again
    layout, grid, want = _past_256()
    for conn in (4, 8):
        print(f"occ 300 conn {conn}: kept {want[conn][1].tolist()}")
        assert want[conn][1][0] == 1 and want[conn][1][1] > 1
        _check(layout, grid, 2, conn, 2, 64, want[conn], (300, conn))


def test_all_foreground_at_the_largest_occ():
    # occ 1024: the largest sums an int32 row can be asked to hold (sum_r = sum_c = 1024^2 * 1023 / 2), the longest chains, the
    # most chunks per wave; the answer is known without a flood fill
    occ = 1024
    layout = np.full((1, occ, occ), 1, dtype=np.uint8)
    half = occ * occ * (occ - 1) // 2
    assert half == 536346624 and 2 * half < 2 ** 31
    table = np.zeros((1, 3, 12), dtype=np.int32)
    table[0, 0] = [occ * occ, 0, occ - 1, 0, occ - 1, half, half, 0, 15, 0, 0, INT_MIN]
    want = (np.zeros((1, occ, occ), dtype=np.int32), np.ones(1, dtype=np.int32), table)
    for conn in (4, 8):
        _check(layout, None, 1, conn, 4, 3, want, (occ, conn))


# ---------------------------------------------------------------------------------------- the host API
def test_objects_equal_the_reference_host_formulas():
    occ, off = 37, 1.9
    layout = np.stack([R.u_shape(occ), R.random_map(occ, 0.3, 2, seed=5)])
    grid = R.random_grid(2, occ, seed=11)
    bo = BevObjects(2, occ, max_objects=8, min_cells=2, conn=8, cls=2, off=off, device=DEV)
    lay = torch.from_numpy(layout).to(DEV)
    db = types.SimpleNamespace(grid=torch.from_numpy(grid).to(DEV))
    # a quarter turn with a translation, and a second camera turned the other way
    pose = np.array([[[0.0, 0, -1, 10.0], [0, 1, 0, 0.5], [1, 0, 0, -3.0], [0, 0, 0, 1]],
                     [[0.0, 0, 1, -4.0], [0, 1, 0, 0.0], [-1, 0, 0, 25.0], [0, 0, 0, 1]]])
    for with_grid in (True, False):
        assert bo.find(lay.unsqueeze(1) if with_grid else lay, depth_bev=db if with_grid else None) is bo
        want_l, want_c, want_t = R.objects(layout, grid if with_grid else None, 2, 8, 2, 8)
        assert np.array_equal(bo.labels.cpu().numpy(), want_l) and np.array_equal(bo.count.cpu().numpy(), want_c)
        assert np.array_equal(bo.table.cpu().numpy(), want_t)
        assert want_c[0] == 1 and want_c[1] > 8 and bo.overflowed() == [False, True]
        for p in (None, pose, torch.from_numpy(pose[:, :3].reshape(2, 12).copy()).to(DEV)):
            got = bo.objects(pose=p)
            want = R.object_list(want_c, want_t, occ, off, None if p is None else pose)
            assert [len(g) for g in got] == [1, 8] == [len(w) for w in want]
            for g, w in zip(sum(got, []), sum(want, [])):
                assert list(g)[:12] == ["id", "cells", "x", "z", "width", "length", "range", "bearing_deg", "truncated", "points",
                                        "obstacle_points", "height"] and set(g) == set(w)
                for k, v in w.items():
                    if isinstance(v, float):
                        assert isinstance(g[k], float) and abs(g[k] - v) <= 1e-12, (k, g[k], v)
                    else:
                        assert g[k] == v and type(g[k]) is type(v), (k, g[k], v)
                if not with_grid:
                    assert g["height"] is None and g["points"] == 0 and g["obstacle_points"] == 0
    bo.reset()
    assert bo.objects() == [[], []] and int(bo.labels.max()) == -1
    with pytest.raises(ValueError, match="layout must be"):
        bo.find(lay[:1])
    with pytest.raises(ValueError, match="depth_bev has"):
        bo.find(lay, depth_bev=types.SimpleNamespace(grid=db.grid[:, :, :36, :36].contiguous()))
