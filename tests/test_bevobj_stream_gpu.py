"""PerceptionStream(objects=...) on the 256^2 synthetic model (occ_map_size 64) and the 94 x 311 frames of
tests/test_stream_session_gpu.py (its helpers are imported: the module shares one model and the frames), cameras 1 and 2, five
pushes.  These tests assert EQUALITY (the labelling itself is the ground of tests/test_bevobj_kernels_gpu.py):

* after every push the session's .objects.labels, .count and .table equal, bit for bit, a stand-alone `BevObjects.find` on a clone
  of that push's layout -- and the breadth-first reference of tests/bevobj_ref.py; the synthetic checkpoint's layouts are mostly car
  cells in one or two blobs, so the road class (cls=1, scattered cells) with min_cells=1 and conn=4 is run as well;
* with depth_bev=dict(K=...) as well, they equal `find(layout, depth_bev=s.depth_bev)` and the reference given the session's grid;
* launches counted at ops.call: jp_bev_objects once per push, directly behind jp_layout_classes_u8 (behind jp_bev_agree in a
  depth_bev session: behind the lift); a session without `objects` has no such call and issues exactly the calls of an `objects`
  session minus that one -- the same number as before `objects` existed;
* the six StreamFrame tensors and the trajectory of an `objects` session are bit-equal to a default session's;
* reset() empties the outputs and the re-run reproduces the first run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd.apis import BevObjects, Perceiver, PerceptionStream, StreamFrame  # noqa: E402
from tests import bevobj_ref as R                                                  # noqa: E402
from tests.test_frozen_model_gpu import _count                                     # noqa: E402
from tests.test_stream_session_gpu import FIELDS, HW, NF, SRC, _World              # noqa: E402

OCC = 64
OUT = ("labels", "count", "table")
DB = dict(cam_height=1.6, pitch_deg=2.0, min_range=0.01, max_range=100.0, h_min=-50.0, h_max=50.0, obst_h=1.6)   # tests/test_depthbev_stream_gpu.py
KINDS = {"car": dict(), "road": dict(cls=1, min_cells=1, conn=4, max_objects=16)}


def _K(cams):
    K = np.tile(np.identity(3), (cams, 1, 1))
    for c in range(cams):
        K[c, 0, 0], K[c, 1, 1], K[c, 0, 2], K[c, 1, 2] = 3.0 + c, 10.0, 155.5 - 9.0 * c, 47.0
    return K


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
            rec.update({n: getattr(s.objects, n).clone() for n in OUT})
        if s.depth_bev is not None:
            rec["grid"] = s.depth_bev.grid.clone()
        out.append(rec)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cams", [1, 2])
def test_session_equals_stand_alone_find(world, cams, kind):
    kw = KINDS[kind]
    s = PerceptionStream(world.model, SRC, cameras=cams, objects=kw or True)
    assert isinstance(s.objects, BevObjects) and s.objects.occ == OCC and s.objects.cameras == cams and s.objects.off == 0.27
    recs = _run(s, world.frames[cams])
    alone = BevObjects(cams, OCC, **kw)
    full = {**dict(max_objects=64, min_cells=4, conn=8, cls=2), **kw}
    for k, r in enumerate(recs):
        alone.find(r["layout"].clone())
        for n in OUT:
            assert torch.equal(getattr(alone, n), r[n]), (k, n)
        want = R.objects(r["layout"].cpu().numpy(), None, full["cls"], full["conn"], full["min_cells"], full["max_objects"])
        print(f"{cams} camera(s), {kind}, frame {k}: kept {want[1].tolist()}, class cells {[int((x == full['cls']).sum()) for x in r['layout']]}")
        for n, w in zip(OUT, want):
            assert np.array_equal(r[n].cpu().numpy(), w), (k, n)
    assert len(s.objects.objects(pose=recs[-1]["pose"])) == cams


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cams", [1, 2])
def test_session_with_depth_bev_passes_the_grid(world, cams, kind):
    kw = {**dict(max_objects=64, min_cells=4, conn=8, cls=2), **KINDS[kind]}
    s = PerceptionStream(world.model, SRC, cameras=cams, depth_bev=dict(K=_K(cams), **DB), objects=kw)
    recs = _run(s, world.frames[cams])
    alone = BevObjects(cams, OCC, **kw)
    points = 0
    for k, r in enumerate(recs):
        s.depth_bev.grid.copy_(r["grid"])
        alone.find(r["layout"].clone(), depth_bev=s.depth_bev)
        for n in OUT:
            assert torch.equal(getattr(alone, n), r[n]), (k, n)
        want = R.objects(r["layout"].cpu().numpy(), r["grid"].cpu().numpy(), kw["cls"], kw["conn"], kw["min_cells"], kw["max_objects"])
        for n, w in zip(OUT, want):
            assert np.array_equal(r[n].cpu().numpy(), w), (k, n)
        points += int(want[2][:, :, 9].sum())
    print(f"{cams} camera(s), {kind}: lifted points inside the objects of the five frames: {points}")


@pytest.mark.parametrize("cams", [1, 2])
def test_outputs_are_unchanged_by_objects(world, cams):
    plain = world.session(cams)
    assert plain.objects is None
    a = _run(plain, world.frames[cams])
    s = Perceiver(world.model, frozen=True).stream(SRC, cameras=cams, objects=True)
    b = _run(s, world.frames[cams])
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")
    for k in range(NF):
        assert a[k]["index"] == b[k]["index"] == k
        for f in FIELDS + ("pose",):
            if a[k][f] is None:
                assert b[k][f] is None
            else:
                assert torch.equal(a[k][f], b[k][f]), (k, f)
    assert torch.equal(plain.trajectory(), s.trajectory())


def test_launches_of_a_push_with_and_without_objects(world, monkeypatch):
    fr = world.frames[2]
    s = PerceptionStream(world.model, SRC, cameras=2, objects=True)
    both = PerceptionStream(world.model, SRC, cameras=2, depth_bev=dict(K=_K(2), **DB), objects=True)
    lift = PerceptionStream(world.model, SRC, cameras=2, depth_bev=dict(K=_K(2), **DB))
    plain = world.session(2)
    for k in (0, 1):
        for x in (s, both, lift, plain):
            x.push(fr[k])
    cs = _count(monkeypatch, lambda: s.push(fr[2]))
    cb = _count(monkeypatch, lambda: both.push(fr[2]))
    cl = _count(monkeypatch, lambda: lift.push(fr[2]))
    cp = _count(monkeypatch, lambda: plain.push(fr[2]))
    torch.cuda.synchronize()
    print(f"C-ABI calls per push: plain {len(cp)}, with objects {len(cs)}, with the lift {len(cl)}, with both {len(cb)}")
    assert cs.count("jp_bev_objects") == 1 and cb.count("jp_bev_objects") == 1 and "jp_bev_objects" not in cp and "jp_bev_objects" not in cl
    assert cs[cs.index("jp_layout_classes_u8") + 1] == "jp_bev_objects"
    i = cb.index("jp_layout_classes_u8")
    assert cb[i + 1:i + 4] == ["jp_depth_bev_classes", "jp_bev_agree", "jp_bev_objects"] and cb.index("jp_depth_bev_lift") < i
    # nothing else about a push changes: without `objects` a session issues what it issued before the keyword existed
    assert [c for c in cs if c != "jp_bev_objects"] == cp and len(cp) == len(cs) - 1
    assert [c for c in cb if c != "jp_bev_objects"] == cl
    assert cp.count("jp_stream_pose_pair") == cp.count("jp_stream_traj_push") == cp.count("jp_layout_classes_u8") == 1


def test_reset_empties_the_outputs_and_reproduces_the_first_run(world):
    s = PerceptionStream(world.model, SRC, cameras=2, objects=KINDS["road"])
    held = s.objects
    first = _run(s, world.frames[2])
    s.reset()
    assert s.objects is held and int(held.labels.max()) == -1 and int(held.count.abs().sum()) == 0 and int(held.table.abs().sum()) == 0
    again = _run(s, world.frames[2])
    for k in range(NF):
        for n in OUT + ("layout",):
            assert torch.equal(first[k][n], again[k][n]), (k, n)
