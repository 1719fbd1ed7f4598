"""PerceptionStream(depth_bev=...) on the 256^2 synthetic model and the 94 x 311 frames of tests/test_stream_session_gpu.py (its
helpers are imported: the module shares one model and the frames), cameras 1 and 2, three frames; the depth maps are 256 x 256, the
layouts and the lifted grid 64 x 64 cells of 0.625 m.  The synthetic checkpoint's depths are no street scene (measured: 0.15 to
0.27 m over a whole frame), so the session is given wide ranges (every depth between 1 cm and 100 m, heights within 50 m of the
plane), a very short focal length (the rays of one image row fan out over some 30 cells in spite of the small depths) and an
obstacle height at the camera's, which the rays above and below the principal point straddle -- printed per run: points
accepted, cells observed, the agreement table.

* the session's .grid, .cls and .agree after a push equal (torch.equal) a `DepthBev` with the same arguments applied to the
  cloned depth and layout of that push, and the float64 numpy restatement tests/depthbev_ref.py;
* with the lift every StreamFrame tensor and the trajectory are bit-equal to a default session's, and StreamFrame is unchanged;
* launches counted at ops.call: the three new entry points once each per push, the lift right behind jp_disp_resize_depth, the
  classes right behind jp_layout_classes_u8 and jp_bev_agree behind that; none in a default session, nothing else changes;
* reset() empties the grid and the re-run reproduces the first run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd.apis import DepthBev, PerceptionStream, StreamFrame            # noqa: E402
from tests import depthbev_ref as R                                                # noqa: E402
from tests.test_frozen_model_gpu import _count                                     # noqa: E402
from tests.test_stream_session_gpu import FIELDS, HW, SRC, _World                  # noqa: E402

NF = 3
OCC = 64
KW = dict(cam_height=1.6, pitch_deg=2.0, min_range=0.01, max_range=100.0, h_min=-50.0, h_max=50.0, obst_h=1.6)
FX, FY = 3.0, 10.0
NEW = ("jp_depth_bev_lift", "jp_depth_bev_classes", "jp_bev_agree")


def _K(cams):
    K = np.tile(np.identity(3), (cams, 1, 1))
    for c in range(cams):
        K[c, 0, 0], K[c, 1, 1], K[c, 0, 2], K[c, 1, 2] = FX + c, FY, 155.5 - 9.0 * c, 47.0
    return K


@pytest.fixture(scope="module")
def world():
    return _World()


def _session(world, cams, **kw):
    return PerceptionStream(world.model, SRC, cameras=cams, depth_bev=dict(K=_K(cams), **{**KW, **kw}))


def _run(s, frames):
    """push the first NF frames; per frame the cloned StreamFrame tensors and, for a depth_bev session, the cloned grid / cls / agree"""
    out = []
    for k in range(NF):
        f = s.push(frames[k])
        rec = {n: (None if getattr(f, n) is None else getattr(f, n).clone()) for n in FIELDS + ("pose",)}
        rec["index"] = f.index
        if s.depth_bev is not None:
            rec.update(grid=s.depth_bev.grid.clone(), cls=s.depth_bev.cls.clone(), agree=s.depth_bev.agree.clone())
        out.append(rec)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cams", [1, 2])
def test_session_equals_depth_bev_on_the_cloned_outputs(world, cams):
    s = _session(world, cams)
    db = s.depth_bev
    assert isinstance(db, DepthBev) and (db.cameras, db.occ, db.src_hw, db.depth_hw, db.off) == (cams, OCC, SRC, (HW, HW), 0.27)
    cam = db.cam.cpu().numpy()
    assert cam[:, 0].tolist() == [(FX + c) * (HW / SRC[1]) for c in range(cams)] and cam[0, 7] == 1.6
    recs = _run(s, world.frames[cams])
    off = DepthBev(cams, OCC, _K(cams), SRC, depth_hw=(HW, HW), **KW)
    for k, r in enumerate(recs):
        assert r["grid"].shape == (cams, 4, OCC, OCC) and r["cls"].shape == (cams, OCC, OCC) and r["agree"].shape == (cams, 2, 3)
        off.lift(r["depth"])
        assert torch.equal(off.grid, r["grid"]), k
        assert torch.equal(off.agreement(r["layout"]), r["agree"]) and torch.equal(off.cls, r["cls"]), k
        depth = r["depth"].cpu().numpy()
        want = R.lift(R.empty_grid(cams, OCC), depth, cam, OCC, 40.0 / OCC, 0.27, KW["min_range"], KW["max_range"], KW["h_min"], KW["h_max"],
                      KW["obst_h"])
        wcls, _ = R.classes(want)
        wagree = R.agree(wcls, r["layout"].cpu().numpy())
        print(f"{cams} camera(s), frame {k}: depth {depth.min():.3f} .. {depth.max():.3f} m, points accepted {int(want[:, 0].sum())} of "
              f"{depth.size}, cells observed {int((wcls != 255).sum())} of {wcls.size}, agreement {wagree.tolist()}")
        assert np.array_equal(r["grid"].cpu().numpy(), want), k
        assert np.array_equal(r["cls"].cpu().numpy(), wcls) and np.array_equal(r["agree"].cpu().numpy(), wagree), k
        assert want[:, 0].sum() > 0 and wagree.sum() == (wcls != 255).sum()         # every layout value is 0, 1 or 2
    if cams == 2:
        assert not torch.equal(recs[0]["grid"][0], recs[0]["grid"][1])
    # keyword arguments reach the lift: argo's offset and a short range give another grid
    t = _session(world, cams, off=1.9, max_range=0.5)
    assert (t.depth_bev.off, t.depth_bev.max_range) == (1.9, 0.5)
    t.push(world.frames[cams][0])
    assert not torch.equal(t.depth_bev.grid, recs[0]["grid"])


@pytest.mark.parametrize("cams", [1, 2])
def test_outputs_are_unchanged_by_the_lift(world, cams):
    plain = world.session(cams)
    assert plain.depth_bev is None
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


def test_launches_of_a_push_with_and_without_the_lift(world, monkeypatch):
    fr = world.frames[2]
    s, plain = _session(world, 2), world.session(2)
    for k in (0, 1):
        plain.push(fr[k])
        s.push(fr[k])
    cs = _count(monkeypatch, lambda: s.push(fr[2]))
    cp = _count(monkeypatch, lambda: plain.push(fr[2]))
    torch.cuda.synchronize()
    print(f"launches per frame: with the lift {len(cs)}, without {len(cp)}")
    assert all(cs.count(n) == 1 for n in NEW) and not any(n in cp for n in NEW)
    assert cs[cs.index("jp_disp_resize_depth") + 1] == "jp_depth_bev_lift"
    i = cs.index("jp_layout_classes_u8")
    assert cs[i + 1:i + 3] == ["jp_depth_bev_classes", "jp_bev_agree"]
    assert [c for c in cs if c not in NEW] == cp                    # nothing else about a push changes


def test_reset_reproduces_the_first_run(world):
    s = _session(world, 2)
    first = _run(s, world.frames[2])
    held = s.depth_bev
    s.reset()
    assert s.depth_bev is held and np.array_equal(held.grid.cpu().numpy(), R.empty_grid(2, OCC)) and bool((held.cls == 255).all())
    again = _run(s, world.frames[2])
    for k in range(NF):
        for n in ("grid", "cls", "agree", "depth", "layout"):
            assert torch.equal(first[k][n], again[k][n]), (k, n)
