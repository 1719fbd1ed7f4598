"""PerceptionStream(depth_bev=dict(K=..., ground=...)) on the 256^2 synthetic model and the 94 x 311 frames of
tests/test_stream_session_gpu.py (its helpers are imported: the module shares one model and the frames), cameras 1 and 2, three
frames.  The synthetic checkpoint's depths are no street scene (0.15 to 0.27 m over a whole frame), so the session gets the wide
ranges of tests/test_depthbev_stream_gpu.py and a fit that is as wide: a band of 3 m, a spread of 1 cm, heights from 1 cm to 50 m,
tilts up to 89 degrees.  Most fits still come back rejected, a few are accepted (then tracking and the prior part ways) -- printed
per frame: status, inliers, plane.  These tests assert EQUALITY, not acceptance
(acceptance is the ground of tests/test_ground_kernels_gpu.py):

* after every push the session's .cam, .mom, .stat, .grid, .cls and .agree equal (torch.equal / array_equal) a stand-alone
  `DepthBev(ground=...)` applied to the cloned depth and layout of that push -- fit, lift, agreement -- and the numpy restatements
  tests/ground_ref.py and tests/depthbev_ref.py; with a prior (every frame starts from the constructor's plane), tracking (every
  frame starts from the last result) and tracking without the layout gate;
* launches counted at ops.call: jp_ground_fit once per push, and the order jp_layout_classes_u8 -> jp_ground_fit ->
  jp_depth_bev_lift -> jp_depth_bev_classes -> jp_bev_agree; no jp_ground_fit in a depth_bev session without `ground` nor in a
  default session, and nothing else about a push changes;
* the StreamFrame tensors and the trajectory are bit-equal to a default session's;
* reset() restores the constructor's plane and the re-run reproduces the first run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd.apis import DepthBev, PerceptionStream, StreamFrame            # noqa: E402
from tests import depthbev_ref as R                                                # noqa: E402
from tests import ground_ref as G                                                  # noqa: E402
from tests.test_frozen_model_gpu import _count                                     # noqa: E402
from tests.test_stream_session_gpu import FIELDS, HW, SRC, _World                  # noqa: E402

NF = 3
OCC = 64
KW = dict(cam_height=1.6, pitch_deg=2.0, min_range=0.01, max_range=100.0, h_min=-50.0, h_max=50.0, obst_h=1.6)
GROUND = dict(rounds=2, band=3.0, parts=8, min_points=50, min_spread=0.01, max_tilt_deg=89.0, h_lo=0.01, h_hi=50.0)
FX, FY = 3.0, 10.0
LIFT = ("jp_depth_bev_lift", "jp_depth_bev_classes", "jp_bev_agree")
MODES = {"prior": dict(track=False), "tracking": dict(track=True), "tracking-free": dict(track=True, use_layout=False)}
STATE = ("cam", "mom", "stat", "grid", "cls", "agree")


def _K(cams):
    K = np.tile(np.identity(3), (cams, 1, 1))
    for c in range(cams):
        K[c, 0, 0], K[c, 1, 1], K[c, 0, 2], K[c, 1, 2] = FX + c, FY, 155.5 - 9.0 * c, 47.0
    return K


@pytest.fixture(scope="module")
def world():
    return _World()


def _eq(a, b):
    """bit-equal tensors, NaN equal to NaN (the rms of a rejected fit)"""
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=a.is_floating_point())


def _session(world, cams, ground):
    return PerceptionStream(world.model, SRC, cameras=cams, depth_bev=dict(K=_K(cams), **KW, ground=ground))


def _run(s, frames):
    """push the first NF frames; per frame the cloned StreamFrame tensors and, for a ground session, the cloned state of its DepthBev"""
    out = []
    for k in range(NF):
        f = s.push(frames[k])
        rec = {n: (None if getattr(f, n) is None else getattr(f, n).clone()) for n in FIELDS + ("pose",)}
        rec["index"] = f.index
        if s.depth_bev is not None and s.depth_bev.ground_kw is not None:
            rec.update({n: getattr(s.depth_bev, n).clone() for n in STATE})
        out.append(rec)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cams", [1, 2])
def test_session_equals_stand_alone_fit_and_lift(world, cams, mode):
    g = {**GROUND, **MODES[mode]}
    s = _session(world, cams, g)
    db = s.depth_bev
    assert isinstance(db, DepthBev) and db.ground_kw["track"] == g["track"] and db.ground_kw["parts"] == 8
    cam0 = db.cam.cpu().numpy()
    assert np.array_equal(db.plane0.cpu().numpy(), cam0[:, 4:]) and cam0[0, 7] == 1.6
    recs = _run(s, world.frames[cams])
    off = DepthBev(cams, OCC, _K(cams), SRC, depth_hw=(HW, HW), **KW, ground=g)
    cam = cam0
    for k, r in enumerate(recs):
        layout = r["layout"] if g.get("use_layout", True) else None
        off.fit_ground(r["depth"], layout).lift(r["depth"])
        off.agreement(r["layout"])
        for n in STATE:
            assert _eq(getattr(off, n), r[n]), (k, n)
        depth = r["depth"].cpu().numpy()
        lay = None if layout is None else layout.cpu().numpy()
        prior = None if g["track"] else cam0[:, 4:].copy()
        cam, mom, stat = G.fit(depth, lay, prior, cam, OCC, 40.0 / OCC, 0.27, KW["min_range"], KW["max_range"], g["band"], g["rounds"],
                               g["min_points"], g["min_spread"], g["max_tilt_deg"], g["h_lo"], g["h_hi"])
        print(f"{cams} camera(s), {mode}, frame {k}: status {stat[:, 0].tolist()} inliers {mom[:, 0].tolist()} plane {cam[:, 4:].round(4).tolist()}")
        assert np.array_equal(r["cam"].cpu().numpy(), cam) and np.array_equal(r["mom"].cpu().numpy(), mom), k
        assert np.array_equal(r["stat"].cpu().numpy(), stat, equal_nan=True), k
        want = R.lift(R.empty_grid(cams, OCC), depth, cam, OCC, 40.0 / OCC, 0.27, KW["min_range"], KW["max_range"], KW["h_min"], KW["h_max"],
                      KW["obst_h"])
        wcls, _ = R.classes(want)
        assert np.array_equal(r["grid"].cpu().numpy(), want) and np.array_equal(r["cls"].cpu().numpy(), wcls), k
        assert np.array_equal(r["agree"].cpu().numpy(), R.agree(wcls, r["layout"].cpu().numpy())), k
    # the host helper reads the live plane
    got = db.ground()
    assert np.array_equal(got["plane"], cam[:, 4:]) and np.array_equal(got["status"], stat[:, 0].astype(np.int64))
    assert np.array_equal(got["height_ratio"], cam[:, 7] / 1.6)


@pytest.mark.parametrize("cams", [1, 2])
def test_outputs_are_unchanged_by_the_fit(world, cams):
    plain = world.session(cams)
    a = _run(plain, world.frames[cams])
    s = _session(world, cams, GROUND)
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


def test_launches_of_a_push_with_and_without_the_fit(world, monkeypatch):
    fr = world.frames[2]
    s, lift, plain = _session(world, 2, GROUND), _session(world, 2, None), world.session(2)
    assert lift.depth_bev.ground_kw is None and not hasattr(lift.depth_bev, "mom")
    for k in (0, 1):
        for x in (s, lift, plain):
            x.push(fr[k])
    cs = _count(monkeypatch, lambda: s.push(fr[2]))
    cl = _count(monkeypatch, lambda: lift.push(fr[2]))
    cp = _count(monkeypatch, lambda: plain.push(fr[2]))
    torch.cuda.synchronize()
    print(f"launches per frame: with the fit {len(cs)}, with the lift alone {len(cl)}, without {len(cp)}")
    assert cs.count("jp_ground_fit") == 1 and "jp_ground_fit" not in cl and "jp_ground_fit" not in cp
    assert all(cs.count(n) == 1 for n in LIFT)
    i = cs.index("jp_layout_classes_u8")
    assert cs[i + 1:i + 5] == ["jp_ground_fit", "jp_depth_bev_lift", "jp_depth_bev_classes", "jp_bev_agree"]
    assert cs[cs.index("jp_disp_resize_depth") + 1] != "jp_depth_bev_lift"
    # a session without `ground` keeps its order, and nothing else about a push changes
    assert cl[cl.index("jp_disp_resize_depth") + 1] == "jp_depth_bev_lift"
    assert [c for c in cs if c not in LIFT + ("jp_ground_fit",)] == cp == [c for c in cl if c not in LIFT]


def test_reset_restores_the_plane_and_reproduces_the_first_run(world):
    s = _session(world, 2, {**GROUND, "track": True})
    held = s.depth_bev
    cam0 = held.cam.clone()
    first = _run(s, world.frames[2])
    s.reset()
    assert s.depth_bev is held and torch.equal(held.cam, cam0) and torch.equal(held.cam[:, 4:], held.plane0)
    assert held.ground()["status"].tolist() == [-1, -1]
    again = _run(s, world.frames[2])
    for k in range(NF):
        for n in STATE + ("depth", "layout"):
            assert _eq(first[k][n], again[k][n]), (k, n)
