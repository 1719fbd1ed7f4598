"""CPU-side checks of the BEV object instances (csrc/bevobj.hip, apis/bevobj.py BevObjects, PerceptionStream(objects=...)): the two
entry points are declared in the header, exported by the library and bound, with the documented argument names and types; the ABI
version is unchanged (the change is additive); the header states what a caller has to know; every refusal returns -1 with a message
before anything touches a device; `BevObjects` and `PerceptionStream(objects=...)` refuse what they cannot run; and the reference
the GPU tests compare against (tests/bevobj_ref.py) is itself checked against hand-drawn maps whose answers do not come from it."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib
from tests import bevobj_ref as R

P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: validation comes first
NAMES = ["layout", "grid", "labels", "count", "table", "ws", "B", "occ", "cls_value", "conn", "min_cells", "max_objects", "stream"]
TYPES = ["const uint8_t*", "const int*", "int*", "int*", "int*", "void*", "int", "int", "int", "int", "int", "int", "void*"]
INT_MIN = -2 ** 31


def test_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (jp_\w+)", out))
    for name in ("jp_bev_objects", "jp_bev_objects_ws_bytes"):
        assert name in protos and name in exported and name in L.fn, name
    assert L.fn["jp_abi_version"]() == 3
    assert [a for _, a in protos["jp_bev_objects"][1]] == NAMES
    assert [t for t, _ in protos["jp_bev_objects"][1]] == TYPES
    assert protos["jp_bev_objects"][0] == "int"
    assert protos["jp_bev_objects_ws_bytes"] == ("long", [("int", "B"), ("int", "occ")])
    # the int32 buffers are typed for ops.call: a float tensor in their place is refused before the call; the scratch is untyped
    assert L.ptr_dtypes["jp_bev_objects"][:6] == [torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32, None]
    # parent and size / id word per cell
    assert L.fn["jp_bev_objects_ws_bytes"](2, 37) == 2 * 4 * 2 * 37 * 37
    assert L.fn["jp_bev_objects_ws_bytes"](4, 256) == 2 * 4 * 4 * 256 * 256


def test_header_states_what_a_caller_has_to_know():
    text = " ".join(open(_lib.HEADER_PATH).read().split()).replace(" * ", " ")
    assert "ID ORDER: the kept components of a camera are numbered 0, 1, 2, ... in raster order of their first cell, the smallest i occ + j" in text
    assert "KEPT iff it has at least min_cells cells" in text and "dropped before numbering: it takes no id and its cells get -1" in text
    assert "labels carries the full id even at or above max_objects" in text and "count[b] > max_objects" in text
    assert "[cells, r_min, r_max, c_min, c_max, sum_r, sum_c, first_cell, edge_mask, pts, pts_obst, hmax_mm]" in text
    assert "INT_MIN when there is none" in text and "with grid == NULL the last three are 0, 0, INT_MIN" in text
    assert "Every output is fully overwritten" in text
    assert "ORDERING in a session: jp_bev_objects behind jp_layout_classes_u8, and with a grid behind jp_depth_bev_lift, all on one stream" in text
    assert "no workgroup waits on another" in text[text.index("BEV object instances"):text.index("jp_bev_objects_ws_bytes(int B")]
    assert "two runs give the same bytes" in text


def _rejected(L, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn["jp_bev_objects"](*args)
    assert rc == -1, (args, rc)
    msg = L.last_error()
    assert msg, args
    return msg


def test_bev_objects_rejects_bad_arguments():
    L = _lib.lib()
    #       layout grid labels count table ws B occ cls conn min max stream
    good = [P, P, P, P, P, P, 2, 64, 2, 8, 4, 64, None]
    idx = {n: i for i, n in enumerate(NAMES)}

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[idx[k]] = v
        return _rejected(L, *a)

    for name in ("layout", "labels", "count", "table", "ws"):
        assert "null" in bad(**{name: None})
    for name in ("B", "occ", "max_objects"):
        for v in (0, -3):
            assert "positive" in bad(**{name: v})
    for v in (0, -1):
        assert "min_cells" in bad(min_cells=v)
    for v in (0, 1, 6, 16, -8):
        assert "conn" in bad(conn=v)
    for v in (-1, 256, 1000):
        assert "cls_value" in bad(cls_value=v)
    msg = bad(occ=1025)
    assert "1024" in msg and "sum_r" in msg and "2^31" in msg
    assert "2^31" in bad(B=1, max_objects=(2 ** 31) // 12 + 1) and "max_objects" in bad(B=1, max_objects=(2 ** 31) // 12 + 1)
    assert "max_objects" in bad(B=4096, max_objects=65536)
    assert "occ" in bad(B=2048, occ=1024)                               # B occ occ = 2^31
    # grid may be null: the call gets past it to the next refusal
    assert "positive" in bad(grid=None, B=0)


def test_python_surface_refuses_what_it_cannot_run():
    from jperceiver_amd import apis
    from jperceiver_amd.apis import BevObjects, PerceptionStream, StreamFrame
    from jperceiver_amd.apis.bevobj import FIELDS, _objects_kw
    from jperceiver_amd.model import MONO
    from oracle import jp_oracle as J
    assert "BevObjects" in apis.__all__
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")
    assert FIELDS == R.FIELDS and len(FIELDS) == 12
    for name in ("find", "objects", "overflowed", "reset"):
        assert callable(getattr(BevObjects, name)), name
    with pytest.raises(TypeError, match="no CPU path"):
        BevObjects(1, 16, device="cpu")
    for kw, what in ((dict(conn=6), "conn"), (dict(min_cells=0), "min_cells"), (dict(max_objects=0), "max_objects"), (dict(cls=256), "cls")):
        with pytest.raises(ValueError, match=what):
            BevObjects(1, 16, device="cpu", **kw)
    with pytest.raises(ValueError, match="1024"):
        BevObjects(1, 1025, device="cpu")
    with pytest.raises(ValueError, match="positive"):
        BevObjects(0, 16, device="cpu")
    # the argument checks of find fire before anything is enqueued
    m = BevObjects.__new__(BevObjects)
    m.cameras, m.occ = 2, 16
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        m.find(torch.zeros((2, 16, 16), dtype=torch.uint8))
    with pytest.raises(TypeError, match="no CPU path"):
        m.find(np.zeros((2, 16, 16), dtype=np.uint8))
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        m.find(torch.zeros((2, 16, 16), dtype=torch.float32))
    # the session: a malformed `objects` is refused first; a model on the CPU has no path with objects either
    assert _objects_kw(None) is None and _objects_kw(True) == {} and _objects_kw(dict(conn=4)) == dict(conn=4)
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt).eval()
    with pytest.raises(TypeError, match="objects must be"):
        PerceptionStream(net, (94, 311), objects="yes")
    with pytest.raises(TypeError, match="unknown entries"):
        PerceptionStream(net, (94, 311), objects=dict(min_cell=2))
    with pytest.raises(ValueError, match="conn"):
        PerceptionStream(net, (94, 311), objects=dict(conn=5))
    with pytest.raises(RuntimeError, match="GPU"):
        PerceptionStream(net, (94, 311), objects=True)
    with pytest.raises(RuntimeError, match="GPU"):
        apis.Perceiver.stream(type("P", (), dict(model=net, out_size=None, min_depth=None, max_depth=None))(), (94, 311), objects=dict(conn=4))
    import inspect
    assert list(inspect.signature(PerceptionStream.__init__).parameters)[-1] == "objects"


# ---------------------------------------------------------------------------------------- the reference against hand-drawn maps
def _draw(rows, v=2):
    return np.array([[v if ch == "#" else 0 for ch in r] for r in rows], dtype=np.uint8)


def test_reference_diagonal_touch_is_one_object_at_conn_8_and_two_at_conn_4():
    m = _draw(["........",
               ".##.....",
               ".##.....",
               "...##...",
               "...##...",
               "........",
               "........",
               "........"])
    lab, n, tab = R.objects_one(m, None, 2, 8, 1, 4)
    assert n == 1 and tab[0].tolist() == [8, 1, 4, 1, 4, 20, 20, 9, 0, 0, 0, INT_MIN] and (tab[1:] == 0).all()
    assert ((lab == 0) == (m == 2)).all() and ((lab == -1) == (m != 2)).all()
    lab, n, tab = R.objects_one(m, None, 2, 4, 1, 4)
    assert n == 2
    assert tab[0].tolist() == [4, 1, 2, 1, 2, 6, 6, 9, 0, 0, 0, INT_MIN]
    assert tab[1].tolist() == [4, 3, 4, 3, 4, 14, 14, 27, 0, 0, 0, INT_MIN]
    assert lab[1, 1] == 0 and lab[3, 3] == 1


def test_reference_u_shape_is_one_object_that_starts_in_the_left_arm():
    occ = 9
    m = R.u_shape(occ)
    assert m[1, 1] == 2 and m[1, occ - 2] == 0 and m[2, occ - 2] == 2 and (m[occ - 1, 1:occ - 1] == 2).all() and (m[2:occ - 1, 2:occ - 2] == 0).all()
    for conn in (4, 8):
        lab, n, tab = R.objects_one(m, None, 2, conn, 1, 4)
        cells = (occ - 1) + (occ - 2) + (occ - 4)                       # left arm, right arm, the bar between them
        assert n == 1 and tab[0, 0] == cells and tab[0, 7] == occ + 1 and tab[0, 1:5].tolist() == [1, occ - 1, 1, occ - 2]
        assert tab[0, 8] == 2                                           # it touches the last row only
        assert (lab[m == 2] == 0).all()


def test_reference_min_cells_keeps_the_exact_size_and_drops_one_below_without_shifting_ids_wrongly():
    m = _draw(["##......",          # 3 cells: dropped at min_cells 4
               "#.......",
               "....##..",          # 4 cells: kept, id 0
               "....##..",
               "........",
               "#.......",          # 1 cell: dropped
               "...#####",          # 5 cells: kept, id 1
               "........"])
    lab, n, tab = R.objects_one(m, None, 2, 8, 4, 4)
    assert n == 2 and tab[0, 0] == 4 and tab[0, 7] == 2 * 8 + 4 and tab[1, 0] == 5 and tab[1, 7] == 6 * 8 + 3 and (tab[2:] == 0).all()
    assert lab[0, 0] == -1 and lab[1, 0] == -1 and lab[5, 0] == -1 and lab[2, 4] == 0 and lab[6, 7] == 1
    assert sorted(np.unique(lab).tolist()) == [-1, 0, 1]
    lab, n, tab = R.objects_one(m, None, 2, 8, 3, 4)
    assert n == 3 and tab[:3, 0].tolist() == [3, 4, 5] and lab[0, 0] == 0 and lab[2, 4] == 1 and lab[6, 7] == 2 and lab[5, 0] == -1
    lab, n, tab = R.objects_one(m, None, 2, 8, 1, 2)                    # four objects, a table of two: count and labels go on
    assert n == 4 and tab[:, 0].tolist() == [3, 4] and lab[5, 0] == 2 and lab[6, 7] == 3


def test_reference_edge_mask_at_each_border():
    for (i, j), bit in (((0, 3), 1), ((7, 3), 2), ((3, 0), 4), ((3, 7), 8), ((0, 0), 5), ((7, 7), 10), ((3, 3), 0)):
        m = np.zeros((8, 8), dtype=np.uint8)
        m[i, j] = 2
        lab, n, tab = R.objects_one(m, None, 2, 8, 1, 1)
        assert n == 1 and tab[0, 8] == bit, (i, j)
        assert R.metrics(tab[0], 8, 0.27)["truncated"] == (bit != 0)
    full = np.full((8, 8), 2, dtype=np.uint8)
    assert R.objects_one(full, None, 2, 4, 1, 1)[2][0].tolist() == [64, 0, 7, 0, 7, 224, 224, 0, 15, 0, 0, INT_MIN]


def test_reference_grid_fields_and_the_sentinel():
    m = _draw(["##..", "....", "..##", "...."])
    grid = np.zeros((4, 4, 4), dtype=np.int32)
    grid[0, 0, :2] = [2, 0]
    grid[1, 0, :2] = [1, 0]
    grid[3, 0, :2] = [-250, 9000]                                       # the 9000 stands in a cell without points: not read
    grid[3, 2, 2:] = [700, 800]                                         # object 1 has no points at all: the sentinel
    lab, n, tab = R.objects_one(m, grid, 2, 8, 1, 4)
    assert n == 2 and tab[0, 9:].tolist() == [2, 1, -250] and tab[1, 9:].tolist() == [0, 0, INT_MIN]
    a, b = R.metrics(tab[0], 4, 0.27), R.metrics(tab[1], 4, 0.27)
    assert a["points"] == 2 and a["obstacle_points"] == 1 and a["height"] == -0.25 and b["height"] is None


@pytest.mark.parametrize("off", [0.27, 1.9])
def test_reference_metrics_of_a_2x3_block_at_occ_16(off):
    # rows 4..5, columns 9..11 of a 16 x 16 layout: cells are 2.5 m a side
    m = np.zeros((16, 16), dtype=np.uint8)
    m[4:6, 9:12] = 2
    lab, n, tab = R.objects_one(m, None, 2, 8, 4, 8)
    assert n == 1 and tab[0].tolist() == [6, 4, 5, 9, 11, 27, 60, 73, 0, 0, 0, INT_MIN]
    got = R.metrics(tab[0], 16, off)
    # by hand: columns 9..11 cover x in [2.5, 10): centre 6.25; rows 4..5 cover z in [25 - off, 30 - off): centre 27.5 - off
    assert abs(got["x"] - 6.25) <= 1e-12 and abs(got["z"] - (27.5 - off)) <= 1e-12
    assert got["width"] == 7.5 and got["length"] == 5.0 and abs(got["range"] - (25.0 - off)) <= 1e-12
    assert abs(got["bearing_deg"] - math.degrees(math.atan2(6.25, 27.5 - off))) <= 1e-12
    assert got["truncated"] is False and got["height"] is None and got["points"] == 0 and got["cells"] == 6
    # a quarter turn to the left with a translation: camera +z is world -X, camera +x is world +Z
    T = np.array([[0.0, 0, -1, 10.0], [0, 1, 0, 0], [1, 0, 0, -3.0], [0, 0, 0, 1]])
    w = R.metrics(tab[0], 16, off, T)
    assert abs(w["X_w"] - (10.0 - (27.5 - off))) <= 1e-12 and abs(w["Z_w"] - (6.25 - 3.0)) <= 1e-12
    # the package's own host arithmetic agrees
    from jperceiver_amd.apis.bevobj import object_metrics
    mine = object_metrics(tab[0], 16, off, T.reshape(-1))
    assert set(mine) == set(w)
    for k, v in w.items():
        assert mine[k] == v or abs(mine[k] - v) <= 1e-12, k


def test_reference_generators_draw_what_they_say():
    for occ in (9, 37):
        for gen in (R.serpentine, R.spiral):
            m = gen(occ)
            for conn in (4, 8):
                assert len(R.components(m == 2, conn)) == 1, (gen.__name__, occ, conn)
        s = R.serpentine(occ)
        assert (s[0::2] == 2).all() and all((s[i] == 2).sum() == 1 for i in range(1, occ, 2))
        st = R.stairs(occ)
        assert len(R.components(st == 2, 8)) == 1 and len(R.components(st == 2, 4)) == occ
        cb = R.checkerboard(occ)
        assert len(R.components(cb == 2, 8)) == 1 and len(R.components(cb == 2, 4)) == (occ * occ + 1) // 2
        assert len(R.components(R.corners(occ) == 2, 8)) == 4
    m = R.random_map(64, 0.59, 1, 3)
    assert set(np.unique(m).tolist()) == {0, 1, 2} and abs((m == 1).mean() - 0.59) < 0.03
