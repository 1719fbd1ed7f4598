"""PerceptionStream(objects=dict(track=...)) on the 256^2 synthetic model (occ_map_size 64) and the 94 x 311 frames of
tests/test_stream_session_gpu.py (its helpers are imported: the module shares one model and the frames), cameras 1 and 2, five
pushes.  These tests assert EQUALITY (the tracking itself is the ground of tests/test_bevtrack_kernels_gpu.py):

* after every push the session's .tracks.tracks_i, .kin and .stats -- and its rolled state -- equal, bit for bit, a stand-alone
  `BevTracker.update(objects, frame.pose)` fed clones of that push's labels, count and table, and the reference of
  tests/bevtrack_ref.py; the synthetic checkpoint's layouts are mostly car cells in one or two blobs, so the road class (cls=1,
  scattered cells, min_cells=1, conn=4) is run as well, with reach 2 and min_overlap 2;
* the six StreamFrame tensors, the trajectory and the s.objects buffers of a `track` session are bit-equal to an objects=True session's;
* launches counted at ops.call: a push of a `track` session issues exactly the calls of an objects=True session plus one
  jp_bev_tracks, directly behind jp_stream_traj_push (and so behind jp_bev_objects);
* reset() empties the tracker and the re-run reproduces the first run."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd.apis import BevTracker, Perceiver, PerceptionStream, StreamFrame  # noqa: E402
from tests import bevtrack_ref as R                                                # noqa: E402
from tests.test_frozen_model_gpu import _count                                     # noqa: E402
from tests.test_stream_session_gpu import FIELDS, NF, SRC, _World                  # noqa: E402

OCC = 64
OBJ = ("labels", "count", "table")
TRK = ("tracks_i", "kin", "stats", "_prev_labels", "_state_i", "_state_d")
KINDS = {"car": dict(track=True), "road": dict(cls=1, min_cells=1, conn=4, max_objects=16, track=dict(reach=2, min_overlap=2))}


@pytest.fixture(scope="module")
def world():
    return _World()


def _run(s, frames):
    out = []
    for k in range(NF):
        f = s.push(frames[k])
        rec = {n: (None if getattr(f, n) is None else getattr(f, n).clone()) for n in FIELDS + ("pose",)}
        rec["index"] = f.index
        if s.objects is not None:
            rec.update({n: getattr(s.objects, n).clone() for n in OBJ})
        if s.tracks is not None:
            rec.update({n: getattr(s.tracks, n).clone() for n in TRK})
        out.append(rec)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cams", [1, 2])
def test_session_equals_stand_alone_update(world, cams, kind):
    kw = KINDS[kind]
    s = PerceptionStream(world.model, SRC, cameras=cams, objects=kw)
    tk = {**dict(reach=1, min_overlap=1), **(kw["track"] if isinstance(kw["track"], dict) else {})}
    M = kw.get("max_objects", 64)
    assert isinstance(s.tracks, BevTracker) and (s.tracks.cameras, s.tracks.occ, s.tracks.max_objects) == (cams, OCC, M)
    assert (s.tracks.reach, s.tracks.min_overlap, s.tracks.off) == (tk["reach"], tk["min_overlap"], 0.27) and s.objects.max_objects == M
    recs = _run(s, world.frames[cams])
    alone = BevTracker(cams, OCC, max_objects=M, **tk)
    state = R.zero_state(cams, OCC, M)
    for k, r in enumerate(recs):
        bo = types.SimpleNamespace(**{n: r[n].clone() for n in OBJ})
        assert alone.update(bo, r["pose"].clone()) is alone
        for n in TRK:
            assert torch.equal(getattr(alone, n), r[n]), (k, n)
        tr, kin, st, state = R.step(r["labels"].cpu().numpy(), r["count"].cpu().numpy(), r["table"].cpu().numpy(),
                                    r["pose"].cpu().numpy().reshape(cams, 16), state, M, tk["reach"], tk["min_overlap"], 0.27)
        print(f"{cams} camera(s), {kind}, frame {k}: [n_cur, matched, born, ended] {st.tolist()}")
        want = {"tracks_i": tr, "kin": kin, "stats": st, "_prev_labels": state["prev_labels"], "_state_i": state["state_i"],
                "_state_d": state["state_d"]}
        for n in TRK:
            assert r[n].cpu().numpy().tobytes() == want[n].tobytes(), (k, n)
        assert (st[:, 1] == 0).all() if k == 0 else True
    rows = s.tracks.tracks(dt=0.1)
    assert len(rows) == cams and [len(x) for x in rows] == st[:, 0].tolist()


@pytest.mark.parametrize("cams", [1, 2])
def test_outputs_and_objects_are_unchanged_by_track(world, cams):
    plain = PerceptionStream(world.model, SRC, cameras=cams, objects=True)
    assert plain.tracks is None
    a = _run(plain, world.frames[cams])
    s = Perceiver(world.model, frozen=True).stream(SRC, cameras=cams, objects=dict(track=True))
    b = _run(s, world.frames[cams])
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")
    for k in range(NF):
        assert a[k]["index"] == b[k]["index"] == k
        for f in FIELDS + ("pose",) + OBJ:
            if a[k][f] is None:
                assert b[k][f] is None
            else:
                assert torch.equal(a[k][f], b[k][f]), (k, f)
    assert torch.equal(plain.trajectory(), s.trajectory())


def test_a_push_with_track_has_one_call_more(world, monkeypatch):
    fr = world.frames[2]
    s = PerceptionStream(world.model, SRC, cameras=2, objects=dict(track=True))
    o = PerceptionStream(world.model, SRC, cameras=2, objects=True)
    off = PerceptionStream(world.model, SRC, cameras=2, objects=dict(track=False))
    plain = world.session(2)
    for k in (0, 1):
        for x in (s, o, off, plain):
            x.push(fr[k])
    cs = _count(monkeypatch, lambda: s.push(fr[2]))
    co = _count(monkeypatch, lambda: o.push(fr[2]))
    cf = _count(monkeypatch, lambda: off.push(fr[2]))
    cp = _count(monkeypatch, lambda: plain.push(fr[2]))
    torch.cuda.synchronize()
    print(f"C-ABI calls per push: plain {len(cp)}, with objects {len(co)}, with objects and track {len(cs)}")
    assert cs.count("jp_bev_tracks") == 1 and "jp_bev_tracks" not in co and "jp_bev_tracks" not in cp and off.tracks is None and cf == co
    assert cs[cs.index("jp_stream_traj_push") + 1] == "jp_bev_tracks" and cs.index("jp_bev_objects") < cs.index("jp_bev_tracks")
    assert [c for c in cs if c != "jp_bev_tracks"] == co and len(cs) == len(co) + 1 and len(co) == len(cp) + 1


def test_reset_empties_the_tracker_and_reproduces_the_first_run(world):
    s = PerceptionStream(world.model, SRC, cameras=2, objects=KINDS["road"])
    held = s.tracks
    first = _run(s, world.frames[2])
    s.reset()
    assert s.tracks is held and held.tracks() == [[], []] and int(held._state_i.abs().sum()) == 0 and int(held._prev_labels.abs().sum()) == 0
    again = _run(s, world.frames[2])
    for k in range(NF):
        for n in TRK + OBJ + ("layout",):
            assert torch.equal(first[k][n], again[k][n]), (k, n)
