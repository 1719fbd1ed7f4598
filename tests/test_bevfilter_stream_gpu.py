"""PerceptionStream(objects=dict(track=dict(filter=...))) on the 256^2 synthetic model (occ_map_size 64) and the 94 x 311 frames of
tests/test_stream_session_gpu.py (its helpers are imported: the module shares one model and the frames), cameras 1 and 2, five
pushes.  These tests assert EQUALITY (the filter itself is the ground of tests/test_bevfilter_kernels_gpu.py):

* after every push the session's .track_filter buffers -- slots_i, slots_d, the head, obj_slot and fstats -- equal, bit for bit, a
  stand-alone `BevTrackFilter.update` fed clones of that push's tracks_i, kin and stats, and the reference of tests/bevfilter_ref.py;
  the synthetic checkpoint's layouts are mostly car cells in one or two blobs, so the road class (cls=1, scattered cells,
  min_cells=1, conn=4) is run as well, with fewer slots than objects, max_coast 1, min_hits 2 and a gate of 1.5 m;
* the StreamFrame tensors, the trajectory, the s.objects and the s.tracks buffers of a `filter` session are bit-equal to a track=True
  session's;
* launches counted at ops.call: a push of a `filter` session issues exactly the calls of a track=True session plus one
  jp_bev_track_filter, directly behind jp_bev_tracks; the default and the track=True session issue what they issued before;
* reset() empties the filter with the tracker and the re-run reproduces the first run."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd.apis import BevTrackFilter, Perceiver, PerceptionStream, StreamFrame  # noqa: E402
from tests import bevfilter_ref as R                                               # noqa: E402
from tests.test_frozen_model_gpu import _count                                     # noqa: E402
from tests.test_stream_session_gpu import FIELDS, NF, SRC, _World                  # noqa: E402

OCC = 64
OBJ = ("labels", "count", "table")
TRK = ("tracks_i", "kin", "stats", "_prev_labels", "_state_i", "_state_d")
FLT = ("slots_i", "slots_d", "_head", "obj_slot", "fstats")
ROAD_FILTER = dict(max_tracks=12, max_coast=1, min_hits=2, gate=1.5)
KINDS = {"car": dict(track=dict(filter=True)),
         "road": dict(cls=1, min_cells=1, conn=4, max_objects=16, track=dict(reach=2, min_overlap=2, filter=ROAD_FILTER))}


@pytest.fixture(scope="module")
def world():
    return _World()


def _run(s, frames):
    out = []
    for k in range(NF):
        f = s.push(frames[k])
        rec = {n: (None if getattr(f, n) is None else getattr(f, n).clone()) for n in FIELDS + ("pose",)}
        rec["index"] = f.index
        rec.update({n: getattr(s.objects, n).clone() for n in OBJ})
        rec.update({n: getattr(s.tracks, n).clone() for n in TRK})
        if s.track_filter is not None:
            rec.update({n: getattr(s.track_filter, n).clone() for n in FLT})
        out.append(rec)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cams", [1, 2])
def test_session_equals_stand_alone_update_and_the_reference(world, cams, kind):
    kw = KINDS[kind]
    s = PerceptionStream(world.model, SRC, cameras=cams, objects=kw)
    fk = kw["track"]["filter"] if isinstance(kw["track"]["filter"], dict) else {}
    M = kw.get("max_objects", 64)
    S = fk.get("max_tracks", min(256, 2 * M))
    par = dict(max_coast=fk.get("max_coast", 3), min_hits=fk.get("min_hits", 3), gate=fk.get("gate", 2.0), meas_sigma=40.0 / OCC,
               vel_sigma0=3.0, accel_sigma=0.5)
    f = s.track_filter
    assert isinstance(f, BevTrackFilter) and (f.cameras, f.max_objects, f.max_tracks) == (cams, M, S)
    assert dict(max_coast=f.max_coast, min_hits=f.min_hits, gate=f.gate, meas_sigma=f.meas_sigma, vel_sigma0=f.vel_sigma0,
                accel_sigma=f.accel_sigma) == par
    assert (s.tracks.reach, s.tracks.min_overlap) == (kw["track"].get("reach", 1), kw["track"].get("min_overlap", 1))
    recs = _run(s, world.frames[cams])
    alone = BevTrackFilter(cams, max_objects=M, occ=OCC, **fk)
    state = R.zero_state(cams, S)
    for k, r in enumerate(recs):
        tr = types.SimpleNamespace(tracks_i=r["tracks_i"].clone(), kin=r["kin"].clone(), stats=r["stats"].clone())
        assert alone.update(tr) is alone
        for n in FLT:
            assert torch.equal(getattr(alone, n), r[n]), (k, n)
        oslot, fs, state = R.step(r["tracks_i"].cpu().numpy(), r["kin"].cpu().numpy(), r["stats"].cpu().numpy(), state, M, S, **par)
        print(f"{cams} camera(s), {kind}, frame {k}: [live, confirmed, coasting, continued, reacquired, born, ended, dropped] {fs.tolist()}")
        want = {"slots_i": state["slots_i"], "slots_d": state["slots_d"], "_head": state["head"], "obj_slot": oslot, "fstats": fs}
        for n in FLT:
            assert r[n].cpu().numpy().tobytes() == want[n].tobytes(), (k, n)
        assert (fs[:, 5] == r["stats"].cpu().numpy()[:, 0].clip(max=S)).all() if k == 0 else True        # the first frame: births only
    rows = f.tracks(dt=0.1)
    assert len(rows) == cams and [len(x) for x in rows] == fs[:, 0].tolist()


@pytest.mark.parametrize("cams", [1, 2])
def test_outputs_objects_and_tracks_are_unchanged_by_filter(world, cams):
    plain = PerceptionStream(world.model, SRC, cameras=cams, objects=dict(track=True))
    assert plain.track_filter is None and PerceptionStream(world.model, SRC, cameras=cams, objects=dict(track=dict(filter=False))).track_filter is None
    a = _run(plain, world.frames[cams])
    s = Perceiver(world.model, frozen=True).stream(SRC, cameras=cams, objects=dict(track=dict(filter=True)))
    b = _run(s, world.frames[cams])
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")
    for k in range(NF):
        assert a[k]["index"] == b[k]["index"] == k
        for f in FIELDS + ("pose",) + OBJ + TRK:
            if a[k][f] is None:
                assert b[k][f] is None
            else:
                assert torch.equal(a[k][f], b[k][f]), (k, f)
    assert torch.equal(plain.trajectory(), s.trajectory())


def test_a_push_with_filter_has_one_call_more(world, monkeypatch):
    fr = world.frames[2]
    s = PerceptionStream(world.model, SRC, cameras=2, objects=dict(track=dict(filter=True)))
    t = PerceptionStream(world.model, SRC, cameras=2, objects=dict(track=True))
    off = PerceptionStream(world.model, SRC, cameras=2, objects=dict(track=dict(filter=False)))
    o = PerceptionStream(world.model, SRC, cameras=2, objects=True)
    plain = world.session(2)
    assert plain.track_filter is None and o.track_filter is None and t.track_filter is None and off.track_filter is None
    for k in (0, 1):
        for x in (s, t, off, o, plain):
            x.push(fr[k])
    cs, ct, cf, co, cp = (_count(monkeypatch, lambda x=x: x.push(fr[2])) for x in (s, t, off, o, plain))
    torch.cuda.synchronize()
    print(f"C-ABI calls per push: plain {len(cp)}, with objects {len(co)}, with tracks {len(ct)}, with tracks and filter {len(cs)}")
    name = "jp_bev_track_filter"
    assert cs.count(name) == 1 and all(name not in c for c in (ct, cf, co, cp)) and cf == ct
    assert cs[cs.index("jp_bev_tracks") + 1] == name and [c for c in cs if c != name] == ct and len(cs) == len(ct) + 1
    # what the sessions without the filter issued before: tracks = objects + one jp_bev_tracks behind the trajectory, objects = plain + one
    assert [c for c in ct if c != "jp_bev_tracks"] == co and ct[ct.index("jp_stream_traj_push") + 1] == "jp_bev_tracks"
    assert len(ct) == len(co) + 1 and len(co) == len(cp) + 1 and [c for c in co if c != "jp_bev_objects"] == cp


def test_reset_empties_the_filter_and_reproduces_the_first_run(world):
    s = PerceptionStream(world.model, SRC, cameras=2, objects=KINDS["road"])
    held = s.track_filter
    first = _run(s, world.frames[2])
    s.reset()
    assert s.track_filter is held and held.tracks() == [[], []] and int(held.slots_i.abs().sum()) == 0 and int(held._head.abs().sum()) == 0
    assert float(held.slots_d.abs().sum()) == 0.0 and int(s.tracks._state_i.abs().sum()) == 0
    again = _run(s, world.frames[2])
    for k in range(NF):
        for n in FLT + TRK + OBJ + ("layout",):
            assert torch.equal(first[k][n], again[k][n]), (k, n)
