"""CPU-side checks of the ground-plane fit (csrc/ground.hip, apis/depthbev.py DepthBev(ground=...)): jp_ground_fit is declared in the
header, exported by the library and bound, with the documented argument names and types; the ABI version is unchanged (the change
is additive); every refusal returns -1 with a message before anything touches a device; `DepthBev(ground=...)`, `fit_ground` and
`PerceptionStream(depth_bev=dict(ground=...))` refuse what they cannot run; and the numpy reference the GPU tests compare against
(tests/ground_ref.py) is itself checked against answers that do not come from it: analytic planes it has to recover, a wall it has
to ignore, a layout gate counted pixel by pixel in plain Python, and the two rejections a caller meets first.

The analytic scenes are 48 x 200 images, fx = fy = 64, cx = 100, cy = 16, occ 16, band 0.3 and a level prior.  A plane of pitch p,
roll r and height h has the normal (tan r, 1, tan p) / |.| -- so that pitch = atan2(nz, ny) and roll = atan2(nx, ny), as
`DepthBev.ground()` reports them -- and is seen at depth h / (nx x' + ny y' + nz) along the ray (x', y', 1)."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib
from tests import ground_ref as G

P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: validation comes first
NAMES = ["depth", "layout", "prior", "cam", "part", "mom", "stat", "B", "H", "W", "occ", "res_f", "off", "min_range", "max_range", "band",
         "rounds", "parts", "min_points", "min_spread", "max_tilt_deg", "h_lo", "h_hi", "stream"]
TYPES = ["const float*", "const uint8_t*", "const double*", "double*", "long long*", "long long*", "double*", "int", "int", "int", "int",
         "double", "double", "double", "double", "double", "int", "int", "int", "double", "double", "double", "double", "void*"]


def test_symbol_is_declared_exported_and_bound():
    L = _lib.lib()
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "jp_ground_fit" in protos and "jp_ground_fit" in set(re.findall(r" T (jp_\w+)", out)) and "jp_ground_fit" in L.fn
    assert L.fn["jp_abi_version"]() == 3
    assert [a for _, a in protos["jp_ground_fit"][1]] == NAMES
    assert [t for t, _ in protos["jp_ground_fit"][1]] == TYPES
    assert protos["jp_ground_fit"][0] == "int"
    # the int64 buffers are typed for ops.call: a float tensor in their place is refused before the call
    assert L.ptr_dtypes["jp_ground_fit"][4:6] == [torch.int64, torch.int64]
    # the header states the ten sums, the order of the solve, the status codes and the ordering a caller has to keep
    text = " ".join(open(_lib.HEADER_PATH).read().split()).replace(" * ", " ")
    assert "[n, sum qx, sum qy, sum qz, sum qx qx, sum qx qz, sum qz qz, sum qx qy, sum qz qy, sum qy qy]" in text
    assert "r = h - ((nx X + ny Y) + nz d)" in text and "qx = (long long)floor(X 1000 + 0.5)" in text
    assert "det = cxx czz - cxz cxz; a = (cxy czz - czy cxz) / det; b = (czy cxx - cxy cxz) / det; c = my - (a mx + b mz)" in text
    assert "s = sqrt((a a + 1) + b b); plane = (-a / s, 1 / s, -b / s, (c / 1000) / s)" in text
    for code in ("1 = too few points", "2 = ill-conditioned", "3 = out of bounds", "0 = accepted"):
        assert code in text, code
    assert "ORDERING in a session: jp_ground_fit behind" in text and "stat[b] = [status, n, rms] of the LAST round" in text


def _rejected(L, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn["jp_ground_fit"](*args)
    assert rc == -1, (args, rc)
    msg = L.last_error()
    assert msg, args
    return msg


def test_ground_fit_rejects_bad_arguments():
    L = _lib.lib()
    #       depth layout prior cam part mom stat B  H   W    occ res_f off   min  max   band rounds parts minp spread tilt  h_lo h_hi stream
    good = [P, P, P, P, P, P, P, 2, 48, 200, 16, 2.5, 0.27, 1.0, 40.0, 0.3, 2, 64, 200, 0.5, 10.0, 0.5, 4.0, None]
    idx = {n: i for i, n in enumerate(NAMES)}

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[idx[k]] = v
        return _rejected(L, *a)

    for name in ("depth", "cam", "part", "mom", "stat"):
        assert "null" in bad(**{name: None})
    for name in ("B", "H", "W", "rounds", "parts"):
        for v in (0, -3):
            assert "positive" in bad(**{name: v})
    assert "1024" in bad(parts=1025)
    for v in (0, -1):
        assert "occ" in bad(occ=v)
    for v in (0.0, -0.5, float("nan")):
        assert "greater than zero" in bad(res_f=v)
        assert "band" in bad(band=v)
    for v in (0.0, -1.0, 1000.5, float("inf"), float("nan")):
        assert "max_range" in bad(max_range=v)
    # 16384 x 16384 pixels at 1000 m: 2^28 * 10^12 >= 2^62, the int64 sums of squares could overflow
    msg = bad(B=1, H=16384, W=16384, max_range=1000.0)
    assert "overflow" in msg and "2^62" in msg
    assert "2^31" in bad(B=2, H=32768, W=32768)
    assert "2^31" in bad(B=8, H=32768, W=32768)
    # what is allowed to be null, or to be anything without a layout, gets past the validation of the others
    assert "positive" in bad(layout=None, prior=None, occ=0, B=0)


def test_python_surface_refuses_what_it_cannot_run():
    from jperceiver_amd.apis import DepthBev, PerceptionStream, StreamFrame
    from jperceiver_amd.apis.depthbev import GROUND_DEFAULTS, GROUND_STATUS, _ground_kw
    from jperceiver_amd.model import MONO
    from oracle import jp_oracle as J
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")
    for name in ("fit_ground", "ground", "reset", "lift"):
        assert callable(getattr(DepthBev, name)), name
    assert list(GROUND_DEFAULTS) == ["rounds", "band", "use_layout", "track", "parts", "min_points", "min_spread", "max_tilt_deg", "h_lo", "h_hi"]
    assert sorted(GROUND_STATUS) == [-1, 0, 1, 2, 3]
    assert _ground_kw(None) is None and _ground_kw(True) == GROUND_DEFAULTS
    kw = _ground_kw(dict(rounds=3, track=1))
    assert kw["rounds"] == 3 and kw["track"] is True and kw["band"] == GROUND_DEFAULTS["band"]
    K = np.array([[64.0, 0, 100], [0, 64.0, 16], [0, 0, 1]])
    with pytest.raises(TypeError, match="ground must be"):
        DepthBev(1, 16, K, (48, 200), device="cpu", ground=3)
    with pytest.raises(TypeError, match="unknown entries"):
        DepthBev(1, 16, K, (48, 200), device="cpu", ground=dict(bands=0.3))
    with pytest.raises(ValueError, match="rounds"):
        DepthBev(1, 16, K, (48, 200), device="cpu", ground=dict(rounds=0))
    with pytest.raises(ValueError, match="parts"):
        DepthBev(1, 16, K, (48, 200), device="cpu", ground=dict(parts=2000))
    with pytest.raises(ValueError, match="band"):
        DepthBev(1, 16, K, (48, 200), device="cpu", ground=dict(band=0.0))
    with pytest.raises(TypeError, match="CUDA"):
        DepthBev(1, 16, K, (48, 200), device="cpu", ground=True)
    # the argument checks of fit_ground fire before anything is enqueued
    m = DepthBev.__new__(DepthBev)
    m.cameras, m.occ, m.depth_hw, m.ground_kw = 1, 16, (48, 200), None
    with pytest.raises(RuntimeError, match="ground=True"):
        m.fit_ground(torch.zeros((1, 1, 48, 200)))
    with pytest.raises(RuntimeError, match="ground=True"):
        m.ground()
    m.ground_kw = _ground_kw(True)
    with pytest.raises(TypeError, match="float32 CUDA tensor"):
        m.fit_ground(torch.zeros((1, 1, 48, 200)))
    with pytest.raises(TypeError, match="float32 CUDA tensor"):
        m.fit_ground(np.zeros((1, 1, 48, 200), dtype=np.float32))
    # the session: a malformed `ground` is refused first; a model on the CPU has no path with the fit either
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt).eval()
    with pytest.raises(TypeError, match="ground must be"):
        PerceptionStream(net, (94, 311), depth_bev=dict(K=K, ground="yes"))
    with pytest.raises(TypeError, match="unknown entries"):
        PerceptionStream(net, (94, 311), depth_bev=dict(K=K, ground=dict(round=2)))
    with pytest.raises(RuntimeError, match="GPU"):
        PerceptionStream(net, (94, 311), depth_bev=dict(K=K, ground=True))


# ---------------------------------------------------------------------------------------- the reference against analytic planes
OCC, H, W = 16, 48, 200
RES, FX, CX, CY = 40.0 / OCC, 64.0, 100.0, 16.0
CAM = np.array([FX, FX, CX, CY, 0.0, 1.0, 0.0, 0.0])                  # the plane columns are not read: the gate is passed on its own
ARGS = dict(occ=OCC, res_f=RES, off=0.27, min_range=1.0, max_range=40.0, band=0.3)


def _normal(pitch_deg, roll_deg):
    n = np.array([math.tan(math.radians(roll_deg)), 1.0, math.tan(math.radians(pitch_deg))])
    return n / np.linalg.norm(n)


def _plane_depth(pitch_deg, roll_deg, h):
    """(H, W) float32: depth of the plane along every ray, 0 (rejected) where the ray does not meet it in front of the camera"""
    nx, ny, nz = _normal(pitch_deg, roll_deg)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    den = nx * (u - CX) / FX + ny * (v - CY) / FX + nz
    with np.errstate(all="ignore"):
        d = np.where(den > 1e-9, h / np.where(den > 1e-9, den, 1.0), 0.0)
    return d.astype(np.float32)


def _fit(depth, prior_h, layout=None, rounds=2, **kw):
    cam = CAM[None].copy()
    cam[0, 4:] = [9.0, 9.0, 9.0, 9.0]                                  # must not be read: round 1 gates with the prior
    prior = np.array([[0.0, 1.0, 0.0, prior_h]])
    return G.fit(depth[None, None], None if layout is None else layout[None], prior, cam, rounds=rounds, **{**ARGS, **kw})


@pytest.mark.parametrize("pitch,roll,h,prior_h", [(2.0, 1.0, 1.65, 1.5), (-3.0, 2.0, 1.4, 1.73)])
def test_reference_recovers_a_tilted_plane(pitch, roll, h, prior_h):
    depth = _plane_depth(pitch, roll, h)
    want = np.array([*_normal(pitch, roll), h])
    cam1, mom1, stat1 = _fit(depth, prior_h, rounds=1)
    cam, mom, stat = _fit(depth, prior_h, rounds=2)
    err = np.abs(cam[0, 4:] - want)
    print(f"pitch {pitch} roll {roll} h {h} from prior h {prior_h}: inliers round 1 {mom1[0, 0]}, round 2 {mom[0, 0]}; after 2 rounds "
          f"normal error {err[:3].max():.2e}, height error {err[3]:.2e} m, rms {stat[0, 2]:.2e} m")
    assert stat1[0, 0] == 0 and stat[0, 0] == 0 and mom1[0, 0] >= 1000 and mom[0, 0] >= mom1[0, 0]
    assert err[3] <= 1e-3 and (err[:3] <= 1e-3).all()                  # one quantum (1 mm) in h, 1e-3 in every normal component
    assert stat[0, 1] == mom[0, 0] and 0.0 <= stat[0, 2] <= 1e-3
    # pitch and roll as DepthBev.ground() reports them
    assert abs(math.degrees(math.atan2(cam[0, 6], cam[0, 5])) - pitch) <= 0.06
    assert abs(math.degrees(math.atan2(cam[0, 4], cam[0, 5])) - roll) <= 0.06


def test_reference_recovers_the_level_plane_exactly():
    depth = _plane_depth(0.0, 0.0, 1.5)
    assert depth[19, 0] == np.float32(1.5 * FX / 3)                     # depth = h fy / (v - cy) below the horizon
    cam, mom, stat = _fit(depth, 1.5)
    n = int(mom[0, 0])
    # every inlier sits at Y = 1.5 m: 1500 mm each, whatever its depth was rounded to in float32
    assert n > 1000 and mom[0, 2] == 1500 * n and mom[0, 9] == 1500 * 1500 * n
    assert mom[0, 7] == 1500 * mom[0, 1] and mom[0, 8] == 1500 * mom[0, 3]
    assert stat[0].tolist() == [0.0, float(n), 0.0]
    assert cam[0, 4:].tolist() == [0.0, 1.0, 0.0, 1.5]


def test_reference_ignores_a_wall_outside_the_band():
    # a wall 10 m ahead over columns 40..119, standing on the ground: its pixels more than `band` above the ground add nothing
    depth = _plane_depth(0.0, 0.0, 1.5)
    wall = np.zeros((H, W), dtype=bool)
    wall[4:, 40:120] = True
    wall &= ~((depth > 0) & (depth < 10.0))
    depth[wall] = 10.0
    v = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    resid = 1.5 - (v - CY) / FX * 10.0                                  # height of a wall pixel above the level plane
    outside = wall & (np.abs(resid) > 0.3 + 1e-9)
    inside = wall & (np.abs(resid) < 0.3 - 1e-9)
    assert outside.sum() > 1000 and inside.sum() > 100 and (outside | inside).sum() == wall.sum()
    gate = np.array([0.0, 1.0, 0.0, 1.5])
    got = G.moments(depth, CAM, gate, None, **ARGS)
    cut = depth.copy()
    cut[outside] = 0.0
    assert np.array_equal(got, G.moments(cut, CAM, gate, None, **ARGS))
    cut[inside] = 0.0                                                   # the foot of the wall, inside the band, does count
    assert got[0] - G.moments(cut, CAM, gate, None, **ARGS)[0] == inside.sum()


def test_reference_layout_gate_counts_road_cells_only():
    depth = _plane_depth(0.0, 0.0, 1.5)
    rng = np.random.default_rng(3)
    layout = rng.integers(0, 3, size=(OCC, OCC), dtype=np.uint8)
    gate = np.array([0.0, 1.0, 0.0, 1.5])
    # which pixels stand over a road cell, found without the reference: plain Python floats, pixel by pixel
    road = np.zeros((H, W), dtype=bool)
    n_all = 0
    for v in range(H):
        for u in range(W):
            d = float(depth[v, u])
            if not 1.0 <= d <= 40.0:
                continue
            X = (u - CX) / FX * d
            Y = (v - CY) / FX * d
            if abs(X) > 40.0 or abs(1.5 - Y) > 0.3:
                continue
            n_all += 1
            uu, vv = X / RES + 0.5 * OCC, (d + 0.27) / RES
            if 0.0 <= uu < OCC and 0.0 <= vv < OCC:
                road[v, u] = layout[OCC - 1 - int(vv), int(uu)] == 1
    free = G.moments(depth, CAM, gate, None, **ARGS)
    got = G.moments(depth, CAM, gate, layout, **ARGS)
    assert free[0] == n_all and 100 < road.sum() < n_all and got[0] == road.sum()
    cut = depth.copy()
    cut[~road] = 0.0
    assert np.array_equal(got, G.moments(cut, CAM, gate, None, **ARGS))
    assert G.moments(depth, CAM, gate, np.zeros_like(layout), **ARGS).tolist() == [0] * 10
    assert np.array_equal(G.moments(depth, CAM, gate, np.ones_like(layout), **ARGS), G.moments(depth, CAM, gate, 1 + 0 * layout, **ARGS))


def test_reference_too_few_points_leaves_the_plane():
    # 10 degrees of pitch seen from a level prior: the residual passes 0.3 m at 1.8 m of depth, the nearest pixel is 2.3 m away
    depth = _plane_depth(10.0, 0.0, 1.5)
    cam, mom, stat = _fit(depth, 1.5)
    assert mom[0].tolist() == [0] * 10
    assert stat[0, :2].tolist() == [1.0, 0.0] and np.isnan(stat[0, 2])
    assert cam[0, 4:].tolist() == [0.0, 1.0, 0.0, 1.5]                  # round 1 was given a prior: it is what the call leaves
    # tracking (no prior): the plane in cam is the gate and stays as it is
    start = CAM[None].copy()
    start[0, 4:] = [0.0, 1.0, 0.0, 1.5]
    cam, mom, stat = G.fit(depth[None, None], None, None, start, **ARGS)
    assert stat[0, 0] == 1 and np.array_equal(cam, start)


def test_reference_one_image_row_is_ill_conditioned():
    depth = _plane_depth(0.0, 0.0, 1.5)
    row = np.zeros_like(depth)
    row[24] = depth[24]                                                 # 200 pixels at one depth (12 m): no spread along z
    cam, mom, stat = _fit(row, 1.5, min_points=100)
    assert mom[0, 0] == W and stat[0, :2].tolist() == [2.0, float(W)] and np.isnan(stat[0, 2])
    assert cam[0, 4:].tolist() == [0.0, 1.0, 0.0, 1.5]
    # (with the default min_points = 200 the same row is still status 2: n = 200 is not below it)
    assert _fit(row, 1.5)[2][0, 0] == 2
