"""PerceptionStream(bev_map=...) and BevMap on the 256^2 synthetic model and the 94 x 311 frames of tests/test_stream_session_gpu.py
(its helpers are imported, the module shares one model and the frames), cameras 1 and 2, five frames; the layouts are 64 x 64
cells of 0.625 m and the map is 160 x 144 cells of the same size around the start pose.

* with the map every per-frame output and the trajectory are bit-identical to a session without it, and StreamFrame is unchanged;
* the session's counts equal (torch.equal) BevMap.fuse of the cloned per-frame layouts with s.trajectory(), and the float64 numpy
  restatement tests/bevmap_ref.py; for one camera also BevMap.fuse on what perceive_video returns -- its poses agree with the
  session's to 1e-12 (tests/test_stream_session_gpu.py), not bitwise, so the counts are compared exactly only when the two pose
  sets are bit-equal and otherwise the share of map cells whose votes differ must be below 1 % (printed);
* launches counted at ops.call: exactly one jp_bev_fuse per push, none in a default session, and nothing else changes;
* reset() zeroes the map and the re-run reproduces it; two cameras keep separate maps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd.apis import BevMap, PerceptionStream, StreamFrame               # noqa: E402
from tests import bevmap_ref as R                                                  # noqa: E402
from tests.test_frozen_model_gpu import _count                                     # noqa: E402
from tests.test_stream_session_gpu import FIELDS, NF, SRC, _World, _run            # noqa: E402

CELLS = (160, 144)
OCC = 64


@pytest.fixture(scope="module")
def world():
    return _World()


def _session(world, cams, **kw):
    return PerceptionStream(world.model, SRC, cameras=cams, bev_map=dict(cells=CELLS, **kw))


def _layouts(frames):
    """(cams, NF, occ, occ) from the cloned frames of a run"""
    return torch.stack([f["layout"] for f in frames], 1).contiguous()


@pytest.mark.parametrize("cams", [1, 2])
def test_outputs_are_unchanged_by_the_map(world, cams):
    plain = world.session(cams)
    assert plain.bev_map is None
    a = _run(plain, world.frames[cams])
    s = _session(world, cams)
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
    assert plain.bev_map is None and isinstance(s.bev_map, BevMap)


@pytest.mark.parametrize("cams", [1, 2])
def test_session_map_equals_offline_fuse_and_the_reference(world, cams):
    s = _session(world, cams)
    frames = _run(s, world.frames[cams])
    m = s.bev_map
    assert (m.cameras, m.occ, m.cells, m.off, m.res, m.origin) == (cams, OCC, CELLS, 0.27, 40.0 / OCC, (80.0, 72.0))
    counts = m.counts.clone()
    assert counts.shape == (cams, 3) + CELLS and counts.dtype == torch.int32
    seen = counts[:, 0]
    assert int(seen.sum()) > 0 and int(seen.max()) <= NF
    assert bool((counts[:, 1] + counts[:, 2] <= seen).all()) and bool((counts >= 0).all())
    lay, traj = _layouts(frames), s.trajectory()
    assert lay.shape == (cams, NF, OCC, OCC) and traj.shape == (cams, NF, 12)
    # the same votes from the kept layouts and the trajectory, in one call (pose_stride 12, N = 5: the atomic kernel) ...
    off = BevMap(cams, OCC, cells=CELLS).fuse(lay, traj)
    assert torch.equal(off.counts, counts)
    # ... from the global poses the frames returned (4 x 4)
    poses = torch.stack([f["pose"] for f in frames], 1)
    assert torch.equal(BevMap(cams, OCC, cells=CELLS).fuse(lay, poses).counts, counts)
    # ... and from the float64 numpy restatement over the whole map
    want = R.fuse(np.zeros((cams, 3) + CELLS, dtype=np.int32), lay.cpu().numpy(), traj.cpu().numpy(), OCC, 40.0 / OCC, 0.27, 40.0,
                  40.0 / OCC, 80.0, 72.0)
    assert np.array_equal(counts.cpu().numpy(), want)
    # classes and image of the live map against the restated rule; the marks sit where cell_of says
    wcls, wrgb = R.classes(want)
    assert np.array_equal(m.classes().cpu().numpy(), wcls)
    tr = traj.cpu().numpy()
    img = m.rgb(trajectory=traj).cpu().numpy()
    assert np.array_equal(img, R.mark(wrgb.copy(), tr, NF, m.res, 80.0, 72.0, (255, 0, 0)))
    assert img[0][m.cell_of(tr[0, 0, 3], tr[0, 0, 11])].tolist() == [255, 0, 0] and m.cell_of(0.0, 0.0) == (80, 72)
    if cams == 1:
        seq = torch.cat([world.resized(1, k) for k in range(NF)])
        v = world.per.perceive_video(seq, batch=1)
        vm = BevMap(1, OCC, cells=CELLS).fuse(v.layout, v.trajectory)
        assert torch.equal(v.layout, lay[0])
        same_poses = np.array_equal(v.trajectory[:, :3].reshape(NF, 12), tr[0])
        differ = float((vm.counts != counts).any(1).float().mean())
        print(f"perceive_video poses bit-equal to the session's: {same_poses}; share of map cells with other votes: {differ:.4%}")
        if same_poses:
            assert torch.equal(vm.counts, counts)
        else:
            assert differ < 0.01


def test_launches_of_a_push_with_and_without_the_map(world, monkeypatch):
    fr = world.frames[2]
    s, plain = _session(world, 2), world.session(2)
    first = _count(monkeypatch, lambda: s.push(fr[0]))              # the push that makes the map
    for k in (0, 1):
        plain.push(fr[k])
    s.push(fr[1])
    cs = _count(monkeypatch, lambda: s.push(fr[2]))
    cp = _count(monkeypatch, lambda: plain.push(fr[2]))
    torch.cuda.synchronize()
    print(f"launches per frame: with the map {len(cs)}, without {len(cp)}")
    assert first.count("jp_bev_fuse") == 1 and cs.count("jp_bev_fuse") == 1 and cs[-1] == "jp_bev_fuse"
    assert cs[-2] == "jp_stream_traj_push"                          # the ordering rule: behind the launch that finishes the pose
    assert not any(c.startswith("jp_bev") for c in cp)
    assert cs[:-1] == cp                                            # nothing else about a push changes


def test_reset_zeroes_the_map_and_the_rerun_reproduces_it(world):
    s = _session(world, 2)
    _run(s, world.frames[2])
    first = s.bev_map.counts.clone()
    held = s.bev_map
    assert int(first.sum()) > 0
    s.reset()
    assert s.bev_map is held and int(s.bev_map.counts.abs().sum()) == 0
    _run(s, world.frames[2])
    assert torch.equal(s.bev_map.counts, first)
    _run(s, world.frames[2][:2])                                    # without a reset the map goes on accumulating
    assert int(s.bev_map.counts[:, 0].sum()) > int(first[:, 0].sum())


def test_two_cameras_keep_separate_maps(world):
    s = _session(world, 2)
    frames = _run(s, world.frames[2])
    counts, lay, traj = s.bev_map.counts, _layouts(frames), s.trajectory()
    assert not torch.equal(counts[0], counts[1])
    for c in (0, 1):
        one = BevMap(1, OCC, cells=CELLS).fuse(lay[c], traj[c])
        assert torch.equal(one.counts[0], counts[c]), c
    # keyword arguments reach the map: argo's offset and a shorter range give other votes
    t = _session(world, 2, off=1.9, max_range=15.0)
    _run(t, world.frames[2])
    assert (t.bev_map.off, t.bev_map.max_range) == (1.9, 15.0)
    assert int(t.bev_map.counts[:, 0].sum()) < int(counts[:, 0].sum())
