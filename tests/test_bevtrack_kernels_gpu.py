"""jp_bev_tracks (csrc/bevtrack.hip) against the plain-Python reference of tests/bevtrack_ref.py.  Every comparison is BYTE equality of
tracks, kin, stats and the rolled state (prev_labels, state_i, state_d): the integers are exact, and the float64 values are
single-rounded operations in the order the header states.  Before every call tracks, stats and the scratch are filled with 0x7f
bytes and kin with NaN -- what comes back equal to the reference was written by the call -- and every call is made twice from the
same state and the two results compared byte for byte.

Shapes are the smallest at which the kernels can go wrong: occ 8 (less than one wave), 37 and 65 (ragged waves: a wave's 64 cells
straddle rows), 64 (one wave per row), 130 (more than one workgroup of the vote per camera, ragged), one and two cameras with
different maps and poses; max_objects 1, 2 and 64 with count > max_objects (ids beyond the table vote for nothing), and 100, where
the matrix no longer fits the LDS tile and the vote takes its other form; reach 0 .. 3 with objects on the map's border so that
neighbourhoods clip; pose_stride 12 and 16.  Scenes: the generators of tests/bevobj_ref.py -- random_map at 0.59 and the
checkerboard labelled 4-connected (many tiny objects), corners, stairs -- moved by integer shifts and by rigid poses with rotation,
three frames chained through the state; the tie and split maps of tests/test_bevtrack_abi_cpu.py; a singular and a NaN pose; and
`BevTracker` itself: first frame, chain, reset() reproducing the first run, and the host read."""
import functools
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import _lib, ops                                               # noqa: E402
from jperceiver_amd.apis import BevTracker                                         # noqa: E402
from tests import bevobj_ref as O                                                  # noqa: E402
from tests import bevtrack_ref as R                                                # noqa: E402

DEV = "cuda"
OUT = ("tracks", "kin", "stats", "prev_labels", "state_i", "state_d")
OCCS = (8, 37, 64, 65, 130)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call(labels, count, table, pose, state, M, reach, min_overlap, off):
    """one jp_bev_tracks call on a copy of `state` and poisoned outputs -> dict of numpy arrays (OUT)"""
    B, occ = labels.shape[0], labels.shape[1]
    st = {k: _dev(v) for k, v in state.items()}
    tracks = torch.full((B, M, 4 * 4), 0x7f, device=DEV, dtype=torch.uint8).view(torch.int32)
    stats = torch.full((B, 4 * 4), 0x7f, device=DEV, dtype=torch.uint8).view(torch.int32)
    kin = torch.full((B, M, 4), float("nan"), device=DEV, dtype=torch.float64)
    ws = torch.full((int(_lib.lib().fn["jp_bev_tracks_ws_bytes"](B, occ, M)),), 0x7f, device=DEV, dtype=torch.uint8)
    p = _dev(pose)
    ops.call("jp_bev_tracks", _dev(labels), _dev(count), _dev(table), p, p.shape[1], st["prev_labels"], st["state_i"], st["state_d"],
             tracks, kin, stats, ws, B, occ, M, reach, min_overlap, off)
    torch.cuda.synchronize()
    got = {"tracks": tracks, "kin": kin, "stats": stats, **st}
    return {k: v.cpu().numpy() for k, v in got.items()}


def _same(got, want, what):
    for name in OUT:
        x, w = got[name], want[name]
        assert x.dtype == w.dtype and x.shape == w.shape, (what, name, x.dtype, w.dtype, x.shape, w.shape)
        if x.tobytes() != w.tobytes():
            bad = np.argwhere(~((x == w) | ((x != x) & (w != w)))) if x.dtype == np.float64 else np.argwhere(x != w)
            at = tuple(bad[0]) if len(bad) else None
            raise AssertionError(f"{what}: {name} differs at {len(bad)} places (0: only in the bits of a NaN), first {at}: "
                                 f"got {x[at] if at else None}, want {w[at] if at else None}")


def _labelled(layouts, conn, min_cells, M):
    return O.objects(np.ascontiguousarray(layouts), None, 2, conn, min_cells, M)


def _flat(poses, stride):
    """(B, 4, 4) -> (B, 12) or (B, 16)"""
    return np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(len(poses), 16)[:, :stride])


def _chain(frames, M, reach, min_overlap, off, stride, what):
    """frames: [(labels, count, table, poses (B, 4, 4))]; the GPU and the reference chained side by side, each through its own state"""
    B, occ = frames[0][0].shape[:2]
    state = R.zero_state(B, occ, M)
    seen = []
    for k, (lab, cnt, tab, poses) in enumerate(frames):
        pose = _flat(poses, stride)
        tr, kin, st, new = R.step(lab, cnt, tab, pose, state, M, reach, min_overlap, off)
        want = {"tracks": tr, "kin": kin, "stats": st, **new}
        a = _call(lab, cnt, tab, pose, state, M, reach, min_overlap, off)
        b = _call(lab, cnt, tab, pose, state, M, reach, min_overlap, off)
        for name in OUT:
            assert a[name].tobytes() == b[name].tobytes(), (what, k, name, "two runs differ")
        _same(a, want, (what, k))
        state = {n: a[n] for n in ("prev_labels", "state_i", "state_d")}          # the GPU's own state goes on
        seen.append(st)
    return seen


def _poses(B, k):
    """frame k: camera b turned by k (3 + 2 b) degrees and moved by fractions of a cell -- rigid, different per camera"""
    return np.stack([R.pose(k * (3.0 + 2.0 * b), 0.4 * k * (b + 1), 0.7 * k - 0.2 * b) for b in range(B)])


@functools.lru_cache(maxsize=None)
def _scene(name, occ, B):
    """-> [(labels, count, table, poses)] x 3 frames, (M, reach, min_overlap, stride)"""
    eye = np.stack([np.identity(4)] * B)
    if name == "random":                                                # many tiny objects, far more than the table's 64 rows at occ >= 37
        M, par = 64, (1, 1, 16)
        base = [O.random_map(occ, 0.59, 2, seed=31 * occ + b) for b in range(B)]
        maps = [base, [R.shift(m, 1, -1) for m in base], [R.shift(m, -1, 2 + b) for b, m in enumerate(base)]]
        poses = [eye, eye, _poses(B, 1)]
        conn, min_cells = 4, 1
    elif name == "corners":                                             # single cells in the corners: every neighbourhood clips
        M, par = 2, (3, 1, 12)
        base = [O.corners(occ) for _ in range(B)]
        maps = [base, [R.shift(m, 0, 0) if b == 0 else np.ascontiguousarray(m[::-1]) for b, m in enumerate(base)],
                [R.shift(m, 2, 1) for m in base]]
        poses = [eye, eye, eye]
        conn, min_cells = 8, 1
    elif name == "checkerboard":                                        # a shift by one column turns it into its complement
        M, par = 64, (2, 1, 12)                                         # every vote count is small: the rounds are full of ties
        base = [O.checkerboard(occ) for _ in range(B)]
        maps = [base, [R.shift(m, 0, 1 + b) for b, m in enumerate(base)], base]
        poses = [eye, _poses(B, 1), _poses(B, 2)]
        conn, min_cells = 4, 1
    else:                                                               # stairs: one long object, a table of one row
        M, par = 1, (0 if occ % 2 else 2, 3, 16)
        base = [O.stairs(occ) if b == 0 else np.ascontiguousarray(O.stairs(occ)[:, ::-1]) for b in range(B)]
        maps = [base, [R.shift(m, 1, 0) for m in base], base]
        poses = [_poses(B, 2), _poses(B, 2), _poses(B, 3)]
        conn, min_cells = 8, 1
    frames = [_labelled(np.stack(m), conn, min_cells, M) + (p,) for m, p in zip(maps, poses)]
    return frames, (M,) + par


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("occ", OCCS)
def test_three_chained_frames_equal_the_reference(occ, B):
    for name in ("random", "corners", "checkerboard", "stairs"):
        frames, (M, reach, min_overlap, stride) = _scene(name, occ, B)
        stats = _chain(frames, M, reach, min_overlap, 0.27, stride, (name, occ, B))
        print(f"occ {occ}, {B} camera(s), {name}: max_objects {M}, reach {reach}, count {frames[0][1].tolist()}, "
              f"stats per frame {[s.tolist() for s in stats]}")
        assert (stats[0][:, 1] == 0).all() and (stats[0][:, 2] == np.minimum(frames[0][1], M)).all()      # the first frame: births only
        if name in ("corners", "stairs") or (name == "checkerboard" and occ >= 37):
            assert (frames[0][1] > M).all() or name == "stairs"         # count > max_objects: the ids beyond the table are ignored
        if name == "random":
            assert all((s[:, 1] > 0).all() for s in stats[1:])          # something was matched in the later frames


@pytest.mark.parametrize("reach", [0, 1, 2, 3])
def test_every_reach_at_the_border(reach):
    # occ 37, two cameras: the corners and their mirror image, and a full first row / column: every neighbourhood clips
    occ = 37
    edge = np.zeros((occ, occ), dtype=np.uint8)
    edge[0, :] = edge[:, 0] = edge[occ - 1, 5:9] = edge[7:9, occ - 1] = 2
    maps = [[O.corners(occ), edge], [O.corners(occ), R.shift(edge, 1, 1)], [R.shift(O.corners(occ), -1, -1), R.shift(edge, -1, 0)]]
    frames = [_labelled(np.stack(m), 8, 1, 8) + (_poses(2, 0),) for m in maps]
    for stride in (12, 16):
        stats = _chain(frames, 8, reach, 1, 1.9, stride, ("border", reach, stride))
    assert stats[1][0].tolist() == [4, 4, 0, 0]                         # the corners stand still: each one finds itself at any reach


def test_the_matrix_beyond_the_lds_tile_and_the_three_forms_of_the_vote(monkeypatch):
    # max_objects 100 > 64: the wave-local runs straight to global memory (the default there); and at 64 the three forms by hand
    frames, _ = _scene("random", 65, 2)
    maps = [np.stack([O.random_map(65, 0.59, 2, seed=31 * 65 + b) for b in range(2)])]
    maps.append(np.stack([R.shift(m, 1, -1) for m in maps[0]]))
    big = [_labelled(m, 4, 1, 100) + (_poses(2, k),) for k, m in enumerate(maps)]
    stats = _chain(big, 100, 2, 1, 0.27, 16, "max_objects 100")
    assert (stats[1][:, 0] == np.minimum(big[1][1], 100)).all() and (stats[1][:, 0] > 64).all() and (stats[1][:, 1] > 0).all()
    for mode in ("0", "1", "2"):
        monkeypatch.setenv("JP_BEV_TRACKS_VOTE", mode)
        _chain(frames[:2], 64, 1, 1, 0.27, 16, ("vote form", mode))
        _chain(big, 100, 1, 2, 0.27, 12, ("vote form, 100 rows", mode))


def test_tie_and_split_maps():
    # the maps of tests/test_bevtrack_abi_cpu.py as the two cameras of one call: camera 0 the tie (two previous objects, one
    # current, equal votes: the smaller previous id wins, the other ends), camera 1 the split (the larger part keeps the id)
    occ = 16
    tie0, tie1, split0, split1 = (np.zeros((occ, occ), dtype=np.uint8) for _ in range(4))
    tie0[5, 2:4] = tie0[5, 5:7] = tie1[5, 2:7] = 2
    split0[5, 2:9] = split1[5, 2:4] = split1[5, 5:9] = 2
    eye = np.stack([np.identity(4)] * 2)
    frames = [_labelled(np.stack(m), 8, 1, 4) + (eye,) for m in ([tie0, split0], [tie1, split1])]
    state = R.zero_state(2, occ, 4)
    for k, (lab, cnt, tab, poses) in enumerate(frames):
        got = _call(lab, cnt, tab, _flat(poses, 16), state, 4, 0, 1, 0.27)
        state = {n: got[n] for n in ("prev_labels", "state_i", "state_d")}
    assert got["stats"].tolist() == [[1, 1, 0, 1], [2, 1, 1, 0]]
    assert got["tracks"][0].tolist() == [[0, 2, 0, 2]] + [[-1, 0, -1, 0]] * 3
    assert got["tracks"][1].tolist() == [[1, 1, -1, 0], [0, 2, 0, 4]] + [[-1, 0, -1, 0]] * 2
    assert got["kin"][1, 1, 2] == 1.5 * 2.5 and got["kin"][1, 1, 3] == 0.0 and (got["kin"][:, 2:] == 0).all()
    _chain(frames, 4, 0, 1, 0.27, 16, "tie and split")


def test_singular_and_nan_poses_give_births():
    occ = 37
    m = np.stack([O.corners(occ), O.stairs(occ)])
    lab = _labelled(m, 8, 1, 8)
    eye = np.stack([np.identity(4)] * 2)
    sing = eye.copy()
    sing[0] = [[1.0, 0, 2, 0], [0, 1, 0, 0], [0.5, 0, 1, 0], [0, 0, 0, 1]]           # camera 0: det = 0
    nan = eye.copy()
    nan[1, 2, 3] = float("nan")                                                       # camera 1: a NaN translation
    stats = _chain([lab + (sing,), lab + (nan,), lab + (eye,), lab + (eye,)], 8, 1, 1, 0.27, 16, "singular, NaN")
    assert [s.tolist() for s in stats] == [[[4, 0, 4, 0], [1, 0, 1, 0]], [[4, 0, 4, 4], [1, 0, 1, 1]], [[4, 4, 0, 0], [1, 0, 1, 1]],
                                           [[4, 4, 0, 0], [1, 1, 0, 0]]]


def test_tracker_first_frame_chain_reset_and_the_host_read():
    occ, B, M = 65, 2, 64
    frames, (_, reach, min_overlap, _) = _scene("random", occ, B)
    tr = BevTracker(B, occ, max_objects=M, reach=reach, min_overlap=min_overlap, off=0.27, device=DEV)
    assert tr.tracks() == [[], []] and tr.stats_host() == [dict(n_cur=0, matched=0, born=0, ended=0)] * 2

    def run():
        out = []
        for lab, cnt, tab, poses in frames:
            bo = types.SimpleNamespace(labels=_dev(lab), count=_dev(cnt), table=_dev(tab))
            assert tr.update(bo, _dev(poses)) is tr                     # (B, 4, 4)
            out.append({"tracks": tr.tracks_i.clone(), "kin": tr.kin.clone(), "stats": tr.stats.clone(), "prev_labels": tr._prev_labels.clone(),
                        "state_i": tr._state_i.clone(), "state_d": tr._state_d.clone()})
        torch.cuda.synchronize()
        return [{k: v.cpu().numpy() for k, v in o.items()} for o in out]

    first = run()
    state = R.zero_state(B, occ, M)
    for k, (lab, cnt, tab, poses) in enumerate(frames):
        t, kin, st, state = R.step(lab, cnt, tab, poses, state, M, reach, min_overlap, 0.27)
        _same(first[k], {"tracks": t, "kin": kin, "stats": st, **state}, ("tracker", k))
    # the host read of the last frame
    rows = tr.tracks(dt=0.1)
    plain = tr.tracks()
    assert [len(r) for r in rows] == np.minimum(frames[-1][1], M).tolist() and tr.stats_host()[0] == dict(zip(("n_cur", "matched", "born", "ended"), st[0].tolist()))
    for b in range(B):
        for i, (r, q) in enumerate(zip(rows[b], plain[b])):
            assert list(r) == ["id", "track", "age", "prev_id", "overlap", "X_w", "Z_w", "dX_w", "dZ_w", "speed"]
            assert [r["id"], r["track"], r["age"], r["prev_id"], r["overlap"]] == [i] + t[b, i].tolist()
            assert [r["X_w"], r["Z_w"], r["dX_w"], r["dZ_w"]] == kin[b, i].tolist()
            if r["age"] == 1:
                assert r["speed"] is None and q["speed"] is None and r["prev_id"] == -1
            else:
                assert q["speed"] == math.hypot(kin[b, i, 2], kin[b, i, 3]) and r["speed"] == q["speed"] / 0.1
    assert any(r["age"] == 3 for r in rows[0]) and any(r["age"] == 1 for r in rows[0])
    # pose given as (B, 16) and (B, 12) is the same call
    bo = types.SimpleNamespace(labels=_dev(frames[0][0]), count=_dev(frames[0][1]), table=_dev(frames[0][2]))
    held = {}
    for shape in ((B, 4, 4), (B, 16), (B, 12)):
        tr.reset()
        p = _dev(frames[2][3]).reshape(B, 16)
        tr.update(bo, p[:, :12].contiguous() if shape == (B, 12) else p.reshape(shape))
        held[shape] = (tr.kin.clone(), tr._state_d.clone())
    assert all(torch.equal(held[(B, 4, 4)][i], held[s][i]) for s in held for i in (0, 1))
    with pytest.raises(ValueError, match="pose must be"):
        tr.update(bo, _dev(frames[0][3])[:1])
    with pytest.raises(ValueError, match="objects has"):
        tr.update(types.SimpleNamespace(labels=bo.labels, count=bo.count, table=bo.table[:, :8].contiguous()), _dev(frames[0][3]))
    # reset: no history, and the same frames give the same bytes again
    tr.reset()
    assert int(tr._state_i.abs().sum()) == 0 and float(tr._state_d.abs().sum()) == 0.0 and int(tr._prev_labels.abs().sum()) == 0
    assert tr.tracks() == [[], []] and tr.tracks_i[0, 0].tolist() == [-1, 0, -1, 0]
    again = run()
    for k in range(len(frames)):
        for name in OUT:
            assert first[k][name].tobytes() == again[k][name].tobytes(), (k, name)
