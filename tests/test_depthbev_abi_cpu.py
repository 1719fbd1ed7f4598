"""CPU-side checks of the depth-to-BEV lift (csrc/depthbev.hip, apis/depthbev.py): the three entry points are declared in the header,
exported by the library and bound, with the documented argument names and pointer types; the ABI version is unchanged (the change is
additive); every refusal returns -1 with a message before anything touches a device; `DepthBev` and
`PerceptionStream(depth_bev=...)` import and refuse what they cannot run; and the numpy reference the GPU tests compare against
(tests/depthbev_ref.py) is itself checked against known answers that do not come from it: a flat ground plane, a fronto-parallel
wall standing on it, depths that must add nothing, a pitched plane and a hand-counted agreement table.  fx = fy = 64 and h = 1.5
keep the divisions exact where an answer depends on them."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib
from tests import depthbev_ref as R

SYMBOLS = ("jp_depth_bev_lift", "jp_depth_bev_classes", "jp_bev_agree")
P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: validation comes first


def test_new_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (jp_\w+)", out))
    for s in SYMBOLS:
        assert s in protos, s
        assert s in exported, s
        assert s in L.fn
    assert L.fn["jp_abi_version"]() == 3
    names = {s: [a for _, a in protos[s][1]] for s in SYMBOLS}
    types = {s: [t for t, _ in protos[s][1]] for s in SYMBOLS}
    assert names["jp_depth_bev_lift"] == ["depth", "cam", "grid", "B", "H", "W", "occ", "res_f", "off", "min_range", "max_range", "h_min",
                                          "h_max", "obst_h", "accumulate", "stream"]
    assert names["jp_depth_bev_classes"] == ["grid", "cls", "height", "B", "cells", "min_points", "obst_points", "stream"]
    assert names["jp_bev_agree"] == ["lifted", "layout", "out", "B", "cells", "stream"]
    assert types["jp_depth_bev_lift"] == ["const float*", "const double*", "int*", "int", "int", "int", "int", "double", "double", "double",
                                          "double", "double", "double", "double", "int", "void*"]
    assert types["jp_depth_bev_classes"] == ["const int*", "uint8_t*", "float*", "int", "int", "int", "int", "void*"]
    assert types["jp_bev_agree"] == ["const uint8_t*", "const uint8_t*", "int*", "int", "int", "void*"]
    # the header states the order of the arithmetic and the conventions a caller has to know
    text = " ".join(open(_lib.HEADER_PATH).read().split()).replace(" * ", " ")
    assert "hgt = h - ((nx X + ny Y) + nz d)" in text
    assert "uu = X / res_f + 0.5 occ" in text and "vv = (d + off) / res_f" in text
    assert "[0, 0, INT_MAX, INT_MIN]" in text and "OVERWRITTEN" in text


def _rejected(L, name, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn[name](*args)
    assert rc == -1, (name, args, rc)
    msg = L.last_error()
    assert msg, (name, args)
    return msg


def test_lift_rejects_bad_arguments():
    L = _lib.lib()
    #       depth cam grid B  H   W    occ res_f off   min  max   h_min h_max obst acc stream
    good = [P, P, P, 2, 24, 200, 16, 2.5, 0.27, 1.0, 40.0, -1.0, 3.0, 0.3, 0, None]
    for i in (0, 1, 2):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_depth_bev_lift", *a)
    for i in (3, 4, 5, 6):
        for bad in (0, -3):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_depth_bev_lift", *a)
    for bad in (0.0, -0.5, float("nan")):
        a = list(good)
        a[7] = bad
        assert "greater than zero" in _rejected(L, "jp_depth_bev_lift", *a)
    for i in (11, 12):
        for bad in (1.5e6, -1.5e6, float("inf"), float("nan")):
            a = list(good)
            a[i] = bad
            assert "1e6" in _rejected(L, "jp_depth_bev_lift", *a)
    a = list(good)
    a[3], a[4], a[5] = 2, 32768, 32768                      # B H W = 2^31
    assert "2^31" in _rejected(L, "jp_depth_bev_lift", *a)
    a[3] = 8                                                # ... and beyond
    assert "2^31" in _rejected(L, "jp_depth_bev_lift", *a)
    a = list(good)
    a[6] = 32768                                            # a grid no int index reaches
    assert "2^31" in _rejected(L, "jp_depth_bev_lift", *a)


def test_classes_and_agree_reject_bad_arguments():
    L = _lib.lib()
    good = [P, P, None, 2, 256, 1, 2, None]                 # height is optional
    for i in (0, 1):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_depth_bev_classes", *a)
    for i in (3, 4):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_depth_bev_classes", *a)
    good = [P, P, P, 2, 256, None]
    for i in (0, 1, 2):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_bev_agree", *a)
    for i in (3, 4):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_bev_agree", *a)


def test_depth_bev_imports_and_refuses_what_it_cannot_run():
    from jperceiver_amd.apis import DepthBev, PerceptionStream, StreamFrame, Perceiver, agreement_scores
    from jperceiver_amd.apis.depthbev import _cam_rows
    from jperceiver_amd.model import MONO
    from oracle import jp_oracle as J
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")
    for name in ("lift", "classes", "height", "agreement", "reset"):
        assert callable(getattr(DepthBev, name)), name
    K = np.array([[64.0, 0, 48], [0, 64.0, 16], [0, 0, 1]])
    with pytest.raises(TypeError, match="CUDA"):
        DepthBev(1, 16, K, (48, 96), device="cpu")
    with pytest.raises(ValueError, match="positive"):
        DepthBev(0, 16, K, (48, 96), device="cpu")
    with pytest.raises(ValueError, match="K must be"):
        DepthBev(2, 16, np.zeros((3, 3, 3)), (48, 96), device="cpu")
    with pytest.raises(ValueError, match="plane"):
        DepthBev(1, 16, K, (48, 96), plane=(0, 1, 0), device="cpu")
    with pytest.raises(ValueError, match="1e6"):
        DepthBev(1, 16, K, (48, 96), h_max=2e6, device="cpu")
    # K is scaled from the camera frames to the depth maps; the plane comes from the height and the pitch, or as given
    rows = _cam_rows(2, K, (48, 96), (96, 288), 1.73, 0.0, None)
    assert rows.shape == (2, 8) and rows[1].tolist() == [192.0, 128.0, 144.0, 32.0, 0.0, 1.0, 0.0, 1.73]
    K4 = np.tile(np.identity(4), (2, 1, 1))
    K4[:, :3, :3] = K
    K4[1, 0, 0] = 32.0
    rows = _cam_rows(2, torch.from_numpy(K4), (48, 96), (48, 96), 1.5, 30.0, None)
    assert rows[:, 0].tolist() == [64.0, 32.0] and rows[0, 4] == 0.0 and rows[0, 7] == 1.5
    assert abs(rows[0, 5] - math.sqrt(3) / 2) < 1e-15 and abs(rows[0, 6] - 0.5) < 1e-15
    assert _cam_rows(1, K, (48, 96), (48, 96), 1.5, 30.0, (0.1, 0.9, 0.2, 2.0))[0, 4:].tolist() == [0.1, 0.9, 0.2, 2.0]
    # the argument checks fire before anything is enqueued: CPU tensors and wrong dtypes have no path
    m = DepthBev.__new__(DepthBev)
    m.cameras, m.occ, m.depth_hw = 1, 16, (48, 96)
    with pytest.raises(TypeError, match="float32 CUDA tensor"):
        m.lift(torch.zeros((1, 1, 48, 96)))
    with pytest.raises(TypeError, match="float32 CUDA tensor"):
        m.lift(np.zeros((1, 1, 48, 96), dtype=np.float32))
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        m.agreement(torch.zeros((1, 16, 16), dtype=torch.uint8))
    # the host helper: plain ratios, NaN where a denominator is 0
    s = agreement_scores(np.array([[30, 60, 2], [10, 20, 6]]), cells=256)
    assert s == {"road_on_ground": 0.75, "car_on_obstacle": 0.75, "observed": 0.5}
    s = agreement_scores(torch.zeros((2, 2, 3), dtype=torch.int32))
    assert all(np.isnan(v).all() and v.shape == (2,) for v in s.values())
    with pytest.raises(ValueError, match="2, 3"):
        agreement_scores(np.zeros((3, 2)))
    # the session: the argument is checked first; a model on the CPU has no path with or without the lift
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt).eval()
    with pytest.raises(TypeError, match="depth_bev"):
        PerceptionStream(net, (94, 311), depth_bev=True)
    with pytest.raises(ValueError, match="K"):
        PerceptionStream(net, (94, 311), depth_bev=dict(cam_height=1.6))
    with pytest.raises(RuntimeError, match="GPU"):
        PerceptionStream(net, (94, 311), depth_bev=dict(K=K))
    with pytest.raises(RuntimeError, match="GPU"):
        Perceiver(net).stream((94, 311), depth_bev=dict(K=K))


# ---------------------------------------------------------------------------------------- the reference against known answers
OCC, H, W = 16, 48, 96
RES, FX, CX, CY, HC = 40.0 / OCC, 64.0, 48.0, 16.0, 1.5
ICY = 16
ARGS = dict(occ=OCC, res_f=RES, off=0.27, min_range=1.0, max_range=40.0, h_min=-1.0, h_max=3.0, obst_h=0.3)


def _ground(plane=(0.0, 1.0, 0.0, HC)):
    """depth (H, W) float32 of the plane n . P = h seen by the camera; 0 (rejected) where the ray does not meet it in front"""
    nx, ny, nz, h = plane
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    den = nx * (u - CX) / FX + ny * (v - CY) / FX + nz
    with np.errstate(all="ignore"):
        d = np.where(den > 1e-9, h / np.where(den > 1e-9, den, 1.0), 0.0)
    return d.astype(np.float32)


def _lifted(depth, plane=(0.0, 1.0, 0.0, HC), **kw):
    cam = R.cam_rows(1, FX, FX, CX, CY, plane)
    return R.lift(R.empty_grid(1, OCC), depth[None, None], cam, **{**ARGS, **kw})[0]


def test_reference_flat_ground_is_ground_everywhere():
    depth = _ground()
    assert depth[ICY + 3, 0] == np.float32(HC * FX / 3)        # depth = h fy / (v - cy) below the horizon
    g = _lifted(depth)
    # the pixels that count, found without the reference: plain Python floats, pixel by pixel
    want = 0
    for v in range(H):
        for u in range(W):
            d = float(depth[v, u])
            X = (u - CX) / FX * d
            want += int(1.0 <= d <= 40.0 and d + 0.27 < 40.0 and -20.0 <= X < 20.0)
    assert want > 1000 and int(g[0].sum()) == want
    seen = g[0] > 0
    assert int(g[1].sum()) == 0
    assert np.abs(g[2][seen]).max() <= 1 and np.abs(g[3][seen]).max() <= 1
    assert (g[2][~seen] == R.INT_MAX).all() and (g[3][~seen] == R.INT_MIN).all()
    cls, height = R.classes(g[None])
    assert (cls[0][seen] == 1).all() and (cls[0][~seen] == 255).all() and seen.sum() > 40
    assert np.isnan(height[0][~seen]).all() and np.abs(height[0][seen]).max() <= 0.001
    # nearer rows of the grid hold more pixels than farther ones: the pile-up the kernel's run aggregation is for
    assert g[0, OCC - 2].sum() > g[0, 2].sum()


def test_reference_wall_at_ten_metres():
    # a wall 10 m ahead over image columns 16..79, its top 8 pixels above the principal point (1.25 m above the camera), standing on
    # the ground; sky (0 = rejected) above it and the ground everywhere else
    depth = _ground()
    depth[:ICY + 1] = 0.0
    wall = np.zeros((H, W), dtype=bool)
    wall[8:, 16:80] = True
    wall &= ~((depth > 0) & (depth < 10.0))                 # the ground in front of the wall hides its foot
    depth[wall] = 10.0
    g = _lifted(depth)
    cls, height = R.classes(g[None])
    cls, height = cls[0], height[0]
    row = OCC - 1 - 4                                       # (10 + 0.27) / 2.5 = 4.108
    cols = slice(6, 10)                                     # X = (u - 48) / 64 * 10 in [-5, 4.84]: uu in [6, 9.94]
    assert (cls[row, cols] == 2).all()
    assert [i for i in range(OCC) if (cls[i] == 2).any()] == [row]
    assert (cls[row] == 2).sum() == 4
    assert (cls[:row, cols] == 255).all()                   # behind the wall, inside its width: not observed
    assert (cls[:row, :6] == 1).any() and (cls[:row, 10:] == 1).any()       # beside it the ground goes on
    assert (cls[row + 1:OCC - 1, cols] == 1).all()          # and in front of it ...
    assert (cls[OCC - 1] == 255).all()                      # ... down to the image's lower edge: 96 / 31 = 3.1 m, the last row ends at 2.23
    assert (g[3, row, cols] == 2750).all() and (height[row, cols] == np.float32(2.75)).all()      # 1.5 + 8 / 64 * 10
    assert int(g[1].sum()) == int(g[1, row, cols].sum()) > 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 0.0, -5.0, 40.5, 0.999])
def test_reference_rejected_depths_add_nothing(bad):
    g = _lifted(np.full((H, W), bad, dtype=np.float32))
    assert np.array_equal(g, R.empty_grid(1, OCC)[0])
    depth = _ground()
    base = _lifted(depth)
    depth2 = depth.copy()
    depth2[:ICY + 1] = bad                         # the rejected part of the ground image, replaced
    assert np.array_equal(_lifted(depth2), base)


def test_reference_pitched_plane_is_ground_again():
    a = math.radians(10.0)
    plane = (0.0, math.cos(a), math.sin(a), HC)
    depth = _ground(plane)
    g = _lifted(depth, plane)
    seen = g[0] > 0
    assert seen.sum() > 40 and int(g[1].sum()) == 0
    assert np.abs(g[2][seen]).max() <= 1 and np.abs(g[3][seen]).max() <= 1
    assert (R.classes(g[None])[0][0][seen] == 1).all()
    flat = _lifted(depth)                                   # the same depths under the level plane: the far ground seems to rise
    assert flat[1].sum() > 0
    # accumulate: a second lift on top doubles the counts and leaves the extremes
    cam = R.cam_rows(1, FX, FX, CX, CY, plane)
    twice = R.lift(g[None].copy(), depth[None, None], cam, accumulate=True, **ARGS)[0]
    assert np.array_equal(twice[:2], 2 * g[:2]) and np.array_equal(twice[2:], g[2:])


def test_reference_agreement_table_by_hand():
    lifted = np.array([[[1, 1, 2, 255], [2, 1, 255, 2]]], dtype=np.uint8)
    layout = np.array([[[1, 0, 2, 1], [1, 1, 2, 7]]], dtype=np.uint8)
    #   ground: (1,1) (1,0) (1,1) -> background 1, road 2, car 0;  obstacle: (2,2) (2,1) (2,7: counted nowhere) -> road 1, car 1
    assert R.agree(lifted, layout).tolist() == [[[1, 2, 0], [0, 1, 1]]]
    assert R.agree(np.full((2, 3, 3), 255, dtype=np.uint8), np.ones((2, 3, 3), dtype=np.uint8)).tolist() == [[[0] * 3] * 2] * 2
    cls, height = R.classes(np.array([[[[0, 1, 3, 5]], [[0, 0, 2, 1]], [[R.INT_MAX, 5, -20, 0]], [[R.INT_MIN, 5, 1500, 299]]]], dtype=np.int32))
    assert cls.reshape(-1).tolist() == [255, 1, 2, 1]
    assert np.isnan(height[0, 0, 0]) and height[0, 0, 1:].tolist() == [np.float32(0.005), np.float32(1.5), np.float32(0.299)]
    cls, _ = R.classes(np.array([[[[0, 1, 3, 5]], [[0, 0, 2, 1]], [[0] * 4], [[0] * 4]]], dtype=np.int32), min_points=2, obst_points=1)
    assert cls.reshape(-1).tolist() == [255, 255, 2, 2]
