"""CPU-side checks of the BEV object tracks (csrc/bevtrack.hip, apis/bevtrack.py BevTracker, PerceptionStream(objects=dict(track=...))):
the two entry points are declared in the header, exported by the library and bound, with the documented argument names and types;
the ABI version is unchanged (the change is additive); the header states what a caller has to know; every refusal returns -1 with a
message that names the argument before anything touches a device; `BevTracker` and the session refuse what they cannot run; and the
reference the GPU tests compare against (tests/bevtrack_ref.py) is itself checked against hand-drawn cases whose answers are worked
out by hand in the comments (16 x 16 maps: cells of 2.5 m; min_cells 1 throughout, so that a single cell is an object)."""
import ctypes
import inspect
import math
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib
from tests import bevobj_ref as O
from tests import bevtrack_ref as R

P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: validation comes first
NAMES = ["labels", "count", "table", "pose", "pose_stride", "prev_labels", "state_i", "state_d", "tracks", "kin", "stats", "ws", "B",
         "occ", "max_objects", "reach", "min_overlap", "off", "stream"]
TYPES = ["const int*", "const int*", "const int*", "const double*", "int", "int*", "int*", "double*", "int*", "double*", "int*", "void*",
         "int", "int", "int", "int", "int", "double", "void*"]
POINTERS = [n for n, t in zip(NAMES, TYPES) if t.endswith("*") and n != "stream"]
OCC, RES, OFF = 16, 2.5, 0.27
I4 = np.identity(4)


def test_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (jp_\w+)", out))
    for name in ("jp_bev_tracks", "jp_bev_tracks_ws_bytes"):
        assert name in protos and name in exported and name in L.fn, name
    assert L.fn["jp_abi_version"]() == 3
    assert [a for _, a in protos["jp_bev_tracks"][1]] == NAMES
    assert [t for t, _ in protos["jp_bev_tracks"][1]] == TYPES
    assert protos["jp_bev_tracks"][0] == "int"
    assert protos["jp_bev_tracks_ws_bytes"] == ("long", [("int", "B"), ("int", "occ"), ("int", "max_objects")])
    i32, f64 = torch.int32, torch.float64
    assert L.ptr_dtypes["jp_bev_tracks"][:12] == [i32, i32, i32, f64, None, i32, i32, f64, i32, f64, i32, None]
    # the overlap matrix: one int32 per pair of table rows and camera
    ws = L.fn["jp_bev_tracks_ws_bytes"]
    assert ws(2, 37, 64) == 4 * 2 * 64 * 64 and ws(1, 256, 256) == 4 * 256 * 256 and ws(3, 1024, 1) == 12
    for bad in ((0, 64, 64), (2, 0, 64), (2, 64, 0), (-1, 64, 64), (2, -5, 64), (2, 64, -1)):
        assert ws(*bad) == 0, bad


def test_header_states_what_a_caller_has_to_know():
    text = " ".join(open(_lib.HEADER_PATH).read().split()).replace(" * ", " ")
    block = text[text.index("BEV object tracks"):text.index("jp_bev_tracks_ws_bytes(int B")]
    for sentence in (
            "current cells are gathered from the previous map",
            "x = ((j + 0.5) - 0.5 occ) res_f, z = ((occ - 0.5) - i) res_f - off",
            "det = P[0][0] P[2][2] - P[0][2] P[2][0]",
            "j' = floor(u), i' = occ - 1 - floor(v)",
            "TIE-BREAK: the smaller p, then the smaller c",
            "in ascending object id each takes track = next_id++",
            "ids >= max_objects exist in labels but are not tracked",
            "a track ends in the first frame it is not matched",
            "tracks (B,M,4) int32, row c = [track_id, age, prev_obj (-1 for a birth), overlap (0 for a birth)], rows >= n_cur are [-1, 0, -1, 0]",
            "kin (B,M,4) float64, row c = [X_w, Z_w, dX_w, dZ_w]",
            "stats (B,4) int32 = [n_cur, matched, born, ended]",
            "state_i (B, 2 + 2 M) int32 = [n_prev, next_id,",
            "state_d (B, 12 + 2 M) float64",
            "ZEROED STATE MEANS NO HISTORY",
            "Every output is fully overwritten",
            "no workgroup waits on another",
            "two runs give the same bytes",
            "the call zeroes it itself",
            "ORDERING in a session: jp_bev_tracks behind jp_bev_objects (it reads labels, count and table) and behind jp_stream_traj_push"):
        assert sentence in block, sentence


def _rejected(L, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn["jp_bev_tracks"](*args)
    assert rc == -1, (args, rc)
    msg = L.last_error()
    assert msg, args
    return msg


def test_bev_tracks_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, P, P, 16, P, P, P, P, P, P, P, 2, 64, 64, 1, 1, 0.27, None]
    idx = {n: i for i, n in enumerate(NAMES)}

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[idx[k]] = v
        return _rejected(L, *a)

    for name in POINTERS:
        msg = bad(**{name: None})
        assert "null" in msg and name in msg, name
    for name in ("B", "occ", "max_objects"):
        for v in (0, -3):
            msg = bad(**{name: v})
            assert "positive" in msg and name in msg
    msg = bad(occ=1025)
    assert "occ" in msg and "1024" in msg
    for v in (257, 4096):
        msg = bad(max_objects=v)
        assert "max_objects" in msg and "256" in msg and "square" in msg
    for v in (-1, 4, 100):
        assert "reach" in bad(reach=v)
    for v in (0, -2):
        assert "min_overlap" in bad(min_overlap=v)
    for v in (0, 4, 11, 13, 15, 17, 32, -12):
        assert "pose_stride" in bad(pose_stride=v)
    for v in (float("nan"), float("inf"), -float("inf")):
        assert "off" in bad(off=v)
    msg = bad(B=2048, occ=1024)                                         # B occ occ = 2^31
    assert "occ" in msg and "2^31" in msg
    msg = bad(B=32768, occ=8, max_objects=256)                          # B M M = 2^31
    assert "max_objects" in msg and "2^31" in msg
    assert "positive" in bad(stream=None, B=0)                          # the stream may be null (the default stream)


def test_python_surface_refuses_what_it_cannot_run():
    from jperceiver_amd import apis
    from jperceiver_amd.apis import BevTracker, PerceptionStream, StreamFrame
    from jperceiver_amd.apis.bevobj import _objects_kw
    from jperceiver_amd.apis.bevtrack import _track_kw
    from jperceiver_amd.model import MONO
    from oracle import jp_oracle as J
    assert "BevTracker" in apis.__all__
    assert list(inspect.signature(BevTracker.__init__).parameters) == ["self", "cameras", "occ", "max_objects", "reach", "min_overlap", "off", "device"]
    d = {k: v.default for k, v in inspect.signature(BevTracker.__init__).parameters.items()}
    assert (d["max_objects"], d["reach"], d["min_overlap"], d["off"], d["device"]) == (64, 1, 1, 0.27, "cuda")
    for name in ("update", "tracks", "stats_host", "reset"):
        assert callable(getattr(BevTracker, name)), name
    with pytest.raises(TypeError, match="no CPU path"):
        BevTracker(1, 16, device="cpu")
    for kw, what in ((dict(max_objects=0), "max_objects"), (dict(max_objects=257), "square"), (dict(reach=4), "reach"), (dict(reach=-1), "reach"),
                     (dict(min_overlap=0), "min_overlap"), (dict(off=float("nan")), "off")):
        with pytest.raises(ValueError, match=what):
            BevTracker(1, 16, device="cpu", **kw)
    with pytest.raises(ValueError, match="1024"):
        BevTracker(1, 1025, device="cpu")
    with pytest.raises(ValueError, match="positive"):
        BevTracker(0, 16, device="cpu")
    # the argument checks of update fire before anything is enqueued
    t = BevTracker.__new__(BevTracker)
    t.cameras, t.occ, t.max_objects = 2, 16, 8
    with pytest.raises(TypeError, match="no CPU path"):
        t.update(object(), torch.zeros((2, 4, 4), dtype=torch.float64))
    cpu_objects = type("O", (), dict(labels=torch.zeros((2, 16, 16), dtype=torch.int32), count=torch.zeros(2, dtype=torch.int32),
                                     table=torch.zeros((2, 8, 12), dtype=torch.int32)))()
    with pytest.raises(TypeError, match="no CPU path"):
        t.update(cpu_objects, torch.zeros((2, 4, 4), dtype=torch.float64))
    # the session: a malformed `track` is refused with the other early refusals, before the model is looked at
    assert _track_kw(None) is None and _track_kw(False) is None and _track_kw(True) == {} and _track_kw(dict(reach=2)) == dict(reach=2)
    assert _objects_kw(True) == {} and _objects_kw(dict(conn=4)) == dict(conn=4) and _objects_kw(dict(track=True)) == dict(track=True)
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt).eval()
    for value in ("yes", 1, [1]):
        with pytest.raises(TypeError, match="track must be"):
            PerceptionStream(net, (94, 311), objects=dict(track=value))
    with pytest.raises(TypeError, match="unknown entries"):
        PerceptionStream(net, (94, 311), objects=dict(track=dict(rech=1)))
    with pytest.raises(ValueError, match="reach"):
        PerceptionStream(net, (94, 311), objects=dict(track=dict(reach=4)))
    with pytest.raises(ValueError, match="min_overlap"):
        PerceptionStream(net, (94, 311), objects=dict(conn=4, track=dict(min_overlap=0)))
    with pytest.raises(ValueError, match="square"):
        PerceptionStream(net, (94, 311), objects=dict(max_objects=300, track=True))
    with pytest.raises(TypeError, match="unknown entries"):
        PerceptionStream(net, (94, 311), objects=dict(tracks=True))
    for ok in (dict(track=True), dict(track=dict(reach=2, min_overlap=3), conn=4), dict(track=False), dict(max_objects=300)):
        with pytest.raises(RuntimeError, match="GPU"):
            PerceptionStream(net, (94, 311), objects=ok)
    with pytest.raises(RuntimeError, match="GPU"):
        apis.Perceiver.stream(type("P", (), dict(model=net, out_size=None, min_depth=None, max_depth=None))(), (94, 311), objects=dict(track=True))
    assert list(inspect.signature(PerceptionStream.__init__).parameters)[-1] == "objects"
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")


# ---------------------------------------------------------------------------------------- the reference against hand-drawn cases
def _blank():
    return np.zeros((OCC, OCC), dtype=np.uint8)


def _block(r0, r1, c0, c1):
    m = _blank()
    m[r0:r1 + 1, c0:c1 + 1] = 2
    return m


def _frames(maps, poses, M=4, reach=1, min_overlap=1, off=OFF):
    """one camera: the maps labelled at min_cells 1 and chained through the reference -> [(tracks, kin, stats, state)] per frame"""
    state, out = R.zero_state(1, OCC, M), []
    for m, T in zip(maps, poses):
        lab, n, tab = O.objects_one(m, None, 2, 8, 1, M)
        tr, kin, st, state = R.step(lab[None], np.array([n], dtype=np.int32), tab[None], np.asarray(T)[None], state, M, reach, min_overlap, off)
        out.append((tr[0], kin[0], st[0], state))
    return out


def test_reference_block_that_moves_two_cells_keeps_its_track():
    # rows 6..7 then rows 4..5, columns 9..11, identity poses.  Centroids: x = (10.5 - 8) 2.5 = 6.25; z = (15.5 - 6.5) 2.5 - off
    # = 22.5 - off, then (15.5 - 4.5) 2.5 - off = 27.5 - off: both in [16, 32), where 22.5 and 27.5 lie on the grid of doubles, so
    # the two roundings of "- off" are the same and the difference is exactly 5 = 2 res_f.  Votes at reach 1: only current row 5
    # has previous cells (row 6) in its neighbourhood: columns 9, 10, 11 see 2, 3, 2 of them = 7.
    (t0, k0, s0, _), (t1, k1, s1, st) = _frames([_block(6, 7, 9, 11), _block(4, 5, 9, 11)], [I4, I4])
    assert s0.tolist() == [1, 0, 1, 0] and t0.tolist() == [[0, 1, -1, 0]] + [[-1, 0, -1, 0]] * 3
    assert k0[0].tolist() == [6.25, 22.5 - OFF, 0.0, 0.0] and (k0[1:] == 0).all()
    assert s1.tolist() == [1, 1, 0, 0] and t1.tolist() == [[0, 2, 0, 7]] + [[-1, 0, -1, 0]] * 3
    assert k1[0, 2] == 0.0 and k1[0, 3] == 2 * RES and k1[0, 0] == 6.25 and k1[0, 1] == 27.5 - OFF
    assert st["state_i"][0].tolist() == [1, 1, 0, 2] + [0] * 6 and st["state_d"][0, :12].tolist() == I4.reshape(-1)[:12].tolist()
    assert st["state_d"][0, 12:14].tolist() == [6.25, 27.5 - OFF] and (st["state_d"][0, 14:] == 0).all()
    assert np.array_equal(st["prev_labels"][0] == 0, _block(4, 5, 9, 11) == 2)


def test_reference_pose_that_cancels_the_motion_gives_zero_displacement():
    # the block stands still in the world (rows 4..5 seen from the origin) and the camera drives 5 m forward: it is seen two rows
    # nearer (rows 6..7).  Every current cell lands on the previous cell it came from: 6 votes at reach 0; Z_w = (22.5 - off) + 5,
    # which by the argument above is the double 27.5 - off of the first frame: d == 0 exactly.
    (t0, k0, s0, _), (t1, k1, s1, _) = _frames([_block(4, 5, 9, 11), _block(6, 7, 9, 11)], [I4, R.pose(0.0, 0.0, 5.0)], reach=0)
    assert t1[0].tolist() == [0, 2, 0, 6] and s1.tolist() == [1, 1, 0, 0]
    assert k1[0].tolist() == [6.25, 27.5 - OFF, 0.0, 0.0] and k0[0].tolist() == [6.25, 27.5 - OFF, 0.0, 0.0]


def test_reference_quarter_turn_pose():
    # previous frame, identity pose: one cell at (4, 5): x' = (5.5 - 8) 2.5 = -6.25, z' = 11.5 * 2.5 - off = 28.75 - off.
    # current frame: one cell at (10, 9): x = 3.75, z = 5.5 * 2.5 - off = 13.75 - off, under a quarter turn X = -z + tx, Z = x + tz
    # with tx = 7.5 - off, tz = 25 - off: X = -6.25, Z = 28.75 - off -- the centre of the previous cell.  One vote at reach 0.
    T = np.array([[0.0, 0, -1, 7.5 - OFF], [0, 1, 0, 0], [1, 0, 0, 25.0 - OFF], [0, 0, 0, 1]])
    prev, cur = _blank(), _blank()
    prev[4, 5] = cur[10, 9] = 2
    assert R.prev_cell(10, 9, OCC, np.float64(RES), np.float64(OFF), R._six(T), R._six(I4), np.float64(1.0)) == (4, 5)
    (_, k0, _, _), (t1, k1, s1, st) = _frames([prev, cur], [I4, T], reach=0)
    assert t1[0].tolist() == [0, 2, 0, 1] and s1.tolist() == [1, 1, 0, 0]
    assert k0[0, :2].tolist() == [-6.25, 28.75 - OFF]
    assert abs(k1[0, 0] + 6.25) <= 1e-12 and abs(k1[0, 1] - (28.75 - OFF)) <= 1e-12 and abs(k1[0, 2]) <= 1e-12 and abs(k1[0, 3]) <= 1e-12
    assert st["state_d"][0, :12].tolist() == T.reshape(-1)[:12].tolist()
    # one cell to the side of the target and reach 0: no vote, a birth
    prev2 = _blank()
    prev2[4, 6] = 2
    (_, _, _, _), (t1, _, s1, _) = _frames([prev2, cur], [I4, T], reach=0)
    assert t1[0].tolist() == [1, 1, -1, 0] and s1.tolist() == [1, 0, 1, 1]


def test_reference_tie_between_two_previous_objects_goes_to_the_smaller_id():
    # previous: A = row 5 columns 2..3 (id 0), B = row 5 columns 5..6 (id 1); current: one bar, row 5 columns 2..6.  Reach 0:
    # overlap[A][0] = overlap[B][0] = 2: A wins, B ends.
    a = _blank()
    a[5, 2:4] = a[5, 5:7] = 2
    b = _blank()
    b[5, 2:7] = 2
    (t0, _, s0, _), (t1, _, s1, st) = _frames([a, b], [I4, I4], reach=0)
    assert s0.tolist() == [2, 0, 2, 0] and t0[:2].tolist() == [[0, 1, -1, 0], [1, 1, -1, 0]]
    assert s1.tolist() == [1, 1, 0, 1] and t1.tolist() == [[0, 2, 0, 2]] + [[-1, 0, -1, 0]] * 3
    assert st["state_i"][0, :4].tolist() == [1, 2, 0, 2]
    # the tie-break is by id, not by position: with B drawn first in raster order (one row up) B is id 0 and wins
    a2 = _blank()
    a2[5, 2:4] = a2[4, 5:7] = 2
    b2 = _blank()
    b2[5, 2:4] = b2[4, 5:7] = b2[4:6, 4] = 2
    (t0, _, _, _), (t1, _, s1, _) = _frames([a2, b2], [I4, I4], reach=0)
    assert t1[0].tolist() == [0, 2, 0, 2] and s1.tolist() == [1, 1, 0, 1]


def test_reference_split_keeps_the_id_with_the_larger_part():
    # previous: row 5 columns 2..8; current: columns 2..3 (id 0, 2 votes) and columns 5..8 (id 1, 4 votes) at reach 0: id 1 keeps
    # track 0, id 0 is born with the next id, 1
    a = _blank()
    a[5, 2:9] = 2
    b = _blank()
    b[5, 2:4] = b[5, 5:9] = 2
    (_, _, _, _), (t1, k1, s1, st) = _frames([a, b], [I4, I4], reach=0)
    assert s1.tolist() == [2, 1, 1, 0]
    assert t1[:2].tolist() == [[1, 1, -1, 0], [0, 2, 0, 4]]
    assert k1[0, 2:].tolist() == [0.0, 0.0] and k1[1, 2] == (7.0 - 5.5) * RES and k1[1, 3] == 0.0
    assert st["state_i"][0, :6].tolist() == [2, 2, 1, 1, 0, 2]


def test_reference_reach_0_against_reach_1_for_a_cell_that_moved_one_cell():
    a, b = _blank(), _blank()
    a[7, 7] = b[7, 8] = 2
    (_, _, _, _), (t1, _, s1, _) = _frames([a, b], [I4, I4], reach=0)
    assert t1[0].tolist() == [1, 1, -1, 0] and s1.tolist() == [1, 0, 1, 1]
    (_, _, _, _), (t1, k1, s1, _) = _frames([a, b], [I4, I4], reach=1)
    assert t1[0].tolist() == [0, 2, 0, 1] and s1.tolist() == [1, 1, 0, 0] and k1[0, 2] == RES
    # two cells away: reach 1 misses, reach 2 finds it
    c = _blank()
    c[5, 9] = 2
    assert _frames([a, c], [I4, I4], reach=1)[1][2].tolist() == [1, 0, 1, 1]
    assert _frames([a, c], [I4, I4], reach=2)[1][0][0].tolist() == [0, 2, 0, 1]


def test_reference_overlap_below_min_overlap_is_a_birth():
    # rows 4..5 x columns 4..5, moved one cell right: 2 cells overlap at reach 0
    (_, _, _, _), (t1, _, s1, _) = _frames([_block(4, 5, 4, 5), _block(4, 5, 5, 6)], [I4, I4], reach=0, min_overlap=3)
    assert t1[0].tolist() == [1, 1, -1, 0] and s1.tolist() == [1, 0, 1, 1]
    (_, _, _, _), (t1, _, s1, _) = _frames([_block(4, 5, 4, 5), _block(4, 5, 5, 6)], [I4, I4], reach=0, min_overlap=2)
    assert t1[0].tolist() == [0, 2, 0, 2] and s1.tolist() == [1, 1, 0, 0]


def test_reference_singular_previous_pose_and_nan_current_pose_give_births():
    m = _block(4, 5, 4, 5)
    sing = np.array([[1.0, 0, 2, 0], [0, 1, 0, 0], [0.5, 0, 1, 0], [0, 0, 0, 1]])          # det = 1 * 1 - 2 * 0.5 = 0
    res = _frames([m, m, m], [sing, I4, I4])
    assert [r[2].tolist() for r in res] == [[1, 0, 1, 0], [1, 0, 1, 1], [1, 1, 0, 0]]
    assert [r[0][0].tolist() for r in res] == [[0, 1, -1, 0], [1, 1, -1, 0], [1, 2, 0, 16]]
    nan = I4.copy()
    nan[2, 3] = float("nan")
    res = _frames([m, m, m], [I4, nan, I4])
    assert [r[2].tolist() for r in res] == [[1, 0, 1, 0], [1, 0, 1, 1], [1, 0, 1, 1]]       # the frame after it has a NaN previous pose
    assert [r[0][0, 0] for r in res] == [0, 1, 2]
    assert res[1][1][0, 0] == (4.5 + 0.5 - 8) * RES and math.isnan(res[1][1][0, 1]) and res[1][1][0, 2:].tolist() == [0.0, 0.0]
    inf = I4.copy()
    inf[0, 0] = float("inf")
    assert _frames([m, m], [I4, inf])[1][2].tolist() == [1, 0, 1, 1]


def test_reference_ids_at_or_above_max_objects_are_not_tracked():
    # two objects, a table of one row: the second exists in labels (id 1) and is ignored
    a = _blank()
    a[2, 2] = a[9, 9] = 2
    lab, n, tab = O.objects_one(a, None, 2, 8, 1, 1)
    assert n == 2 and lab[9, 9] == 1 and tab.shape == (1, 12)
    res = _frames([a, a], [I4, I4], M=1, reach=0)
    assert res[0][0].tolist() == [[0, 1, -1, 0]] and res[0][2].tolist() == [1, 0, 1, 0]
    assert res[1][0].tolist() == [[0, 2, 0, 1]] and res[1][2].tolist() == [1, 1, 0, 0]
    assert res[1][3]["state_i"][0].tolist() == [1, 1, 0, 2] and res[1][3]["prev_labels"][0, 9, 9] == 1
    # the ignored object does not vote either: moved onto the first one's old place it gives no match
    b = _blank()
    b[0, 0] = b[2, 2] = 2                                               # ids: (0, 0) -> 0, (2, 2) -> 1 (ignored)
    assert _frames([a, b], [I4, I4], M=1, reach=0)[1][2].tolist() == [1, 0, 1, 1]


def test_reference_births_take_ids_in_object_order_and_next_id_is_carried():
    f0 = _blank()
    f0[5, 5] = f0[9, 9] = 2                                             # ids 0, 1 -> tracks 0, 1
    f1 = f0.copy()
    f1[1, 12] = f1[12, 1] = 2                                           # ids: (1,12) 0 born, (5,5) 1, (9,9) 2, (12,1) 3 born
    f2 = _blank()
    f2[14, 3] = f2[0, 1] = 2                                            # nothing overlaps: two births, four ends
    res = _frames([f0, f1, f2], [I4, I4, I4], M=4, reach=1)
    assert res[0][0][:, 0].tolist() == [0, 1, -1, -1] and res[0][3]["state_i"][0, 1] == 2
    assert res[1][0].tolist() == [[2, 1, -1, 0], [0, 2, 0, 1], [1, 2, 1, 1], [3, 1, -1, 0]]
    assert res[1][2].tolist() == [4, 2, 2, 0] and res[1][3]["state_i"][0, 1] == 4
    assert res[2][0].tolist() == [[4, 1, -1, 0], [5, 1, -1, 0], [-1, 0, -1, 0], [-1, 0, -1, 0]]
    assert res[2][2].tolist() == [2, 0, 2, 4] and res[2][3]["state_i"][0].tolist() == [2, 6, 4, 1, 5, 1, 0, 0, 0, 0]
