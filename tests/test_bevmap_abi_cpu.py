"""CPU-side checks of the world-frame BEV map (csrc/bevmap.hip, apis/bevmap.py): the three entry points are declared in the header,
exported by the library and bound; the ABI version is unchanged (the change is additive); argument names and pointer types are the
documented ones; null, non-positive and res <= 0 arguments are refused with a message before anything touches a device; `BevMap`
and `PerceptionStream(bev_map=...)` import and refuse what they cannot run; `StreamFrame` keeps its fields; and the numpy
reference the GPU tests compare against (tests/bevmap_ref.py) is itself checked against hand-computed placements."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib
from tests import bevmap_ref as R

SYMBOLS = ("jp_bev_fuse", "jp_bev_map_classes", "jp_bev_map_mark")
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
    assert names["jp_bev_fuse"] == ["layout", "pose", "pose_stride", "N", "counts", "B", "occ", "res_f", "off", "max_range", "Mh", "Mw",
                                    "res", "org_r", "org_c", "stream"]
    assert names["jp_bev_map_classes"] == ["counts", "cls", "rgb", "B", "cells", "min_seen", "road_frac", "car_frac", "stream"]
    assert names["jp_bev_map_mark"] == ["rgb", "B", "Mh", "Mw", "traj", "n", "capacity", "res", "org_r", "org_c", "color", "stream"]
    # element types the binding checks tensors against: classes are bytes, poses float64, counts int32
    assert types["jp_bev_fuse"] == ["const uint8_t*", "const double*", "int", "int", "int*", "int", "int", "double", "double", "double",
                                    "int", "int", "double", "double", "double", "void*"]
    assert types["jp_bev_map_classes"] == ["const int*", "uint8_t*", "uint8_t*", "int", "int", "double", "double", "double", "void*"]
    assert types["jp_bev_map_mark"] == ["uint8_t*", "int", "int", "int", "const double*", "int", "int", "double", "double", "double", "int",
                                        "void*"]
    # the header states the conventions a caller has to know
    text = " ".join(open(_lib.HEADER_PATH).read().split()).replace(" * ", " ")
    assert "AFTER its jp_stream_traj_push" in text
    assert "height above the ground is dropped" in text


def _rejected(L, name, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn[name](*args)
    assert rc == -1, (name, args, rc)
    msg = L.last_error()
    assert msg, (name, args)
    return msg


def test_fuse_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, 16, 1, P, 2, 16, 2.5, 0.27, 40.0, 48, 40, 2.5, 24.0, 20.0, None]
    for i in (0, 1, 4):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_bev_fuse", *a)
    for i in (3, 5, 6, 10, 11):
        for bad in (0, -3):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_bev_fuse", *a)
    for i in (7, 12):                                       # res_f, res
        for bad in (0.0, -0.5, float("nan")):
            a = list(good)
            a[i] = bad
            assert "greater than zero" in _rejected(L, "jp_bev_fuse", *a)
    for bad in (0, 11, -16):                                # a pose is at least the 12 doubles of rows 0..2
        a = list(good)
        a[2] = bad
        assert "pose_stride" in _rejected(L, "jp_bev_fuse", *a)
    a = list(good)
    a[3], a[5] = 256, 256                                   # B * N is a grid dimension
    assert "65535" in _rejected(L, "jp_bev_fuse", *a)
    a = list(good)
    a[12] = 1e-9                                            # a window that no grid could hold
    assert "32768" in _rejected(L, "jp_bev_fuse", *a)


def test_map_classes_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, None, 2, 48 * 40, 1.0, 0.5, 0.5, None]     # rgb is optional
    for i in (0, 1):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_bev_map_classes", *a)
    for i in (3, 4):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_bev_map_classes", *a)


def test_map_mark_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, 2, 48, 40, P, 3, 4, 2.5, 24.0, 20.0, 0xff, None]
    for i in (0, 4):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_bev_map_mark", *a)
    for i in (1, 2, 3, 5, 6):
        for bad in (0, -2):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_bev_map_mark", *a)
    a = list(good)
    a[5] = 5                                                # more rows than the trajectory holds
    assert "capacity" in _rejected(L, "jp_bev_map_mark", *a)
    for bad in (0.0, -1.0, float("nan")):
        a = list(good)
        a[7] = bad
        assert "greater than zero" in _rejected(L, "jp_bev_map_mark", *a)


def test_bev_map_imports_and_refuses_what_it_cannot_run():
    from jperceiver_amd.apis import BevMap, PerceptionStream, StreamFrame, Perceiver
    from jperceiver_amd.model import MONO
    from oracle import jp_oracle as J
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")
    for name in ("fuse", "classes", "rgb", "reset", "cell_of"):
        assert callable(getattr(BevMap, name)), name
    with pytest.raises(TypeError, match="CUDA"):
        BevMap(1, 16, cells=(8, 8), device="cpu")
    with pytest.raises(ValueError, match="positive"):
        BevMap(0, 16, device="cpu")
    with pytest.raises(ValueError, match="res"):
        BevMap(1, 16, res=0.0, device="cpu")
    # the argument checks of fuse fire before anything is enqueued: CPU tensors and wrong dtypes have no path
    m = BevMap.__new__(BevMap)
    m.cameras, m.occ, m.cells, m.res_f, m.res, m.origin = 1, 16, (48, 40), 2.5, 2.5, (24.0, 20.0)
    m.device = torch.device("cuda", 0)
    lay, poses = torch.zeros((3, 16, 16), dtype=torch.uint8), torch.zeros((3, 4, 4), dtype=torch.float64)
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        m.fuse(lay, poses)
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        m.fuse(lay.float(), poses)
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        m.fuse(lay.numpy(), poses)
    with pytest.raises(TypeError, match="float64"):
        m._poses(poses)                                     # a CPU tensor: host poses come as numpy
    with pytest.raises(TypeError, match="float64"):
        m._poses(np.zeros((3, 4, 4), dtype=np.float32))
    assert m.cell_of(0.0, 0.0) == (24, 20) and m.cell_of(-0.1, 0.1) == (23, 19) and m.cell_of(2.5, -2.5) == (25, 21)
    # the session: the argument is checked first; a model on the CPU has no path with or without a map
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt).eval()
    with pytest.raises(TypeError, match="bev_map"):
        PerceptionStream(net, (94, 311), bev_map="yes")
    with pytest.raises(RuntimeError, match="GPU"):
        PerceptionStream(net, (94, 311), bev_map=True)
    with pytest.raises(RuntimeError, match="GPU"):
        Perceiver(net).stream((94, 311), bev_map=dict(cells=(64, 64)))


# ---------------------------------------------------------------------------------------- the reference checks itself
OCC, MH, MW, ORG = 16, 48, 40, (30.0, 18.0)
RES = 40.0 / OCC


def _layout(seed=3):
    return np.random.default_rng(seed).integers(0, 3, size=(OCC, OCC), dtype=np.uint8)


def _fused(layout, T, **kw):
    a = dict(occ=OCC, res_f=RES, off=0.0, max_range=40.0, res=RES, org_r=ORG[0], org_c=ORG[1])
    a.update(kw)
    counts = np.zeros((3, MH, MW), dtype=np.int32)
    R.fuse_one(counts, layout, np.asarray(T).reshape(-1), **a)
    return counts


def _pasted(block, r0, c0):
    """counts a map holds when `block` (occ x occ classes) lies with its top-left cell at (r0, c0); parts off the map are cut"""
    want = np.zeros((3, MH, MW), dtype=np.int32)
    for i in range(block.shape[0]):
        for j in range(block.shape[1]):
            r, c = r0 + i, c0 + j
            if 0 <= r < MH and 0 <= c < MW:
                want[0, r, c] = 1
                want[1, r, c] = block[i, j] == 1
                want[2, r, c] = block[i, j] == 2
    return want


def test_reference_identity_pastes_the_layout():
    lay = _layout()
    got = _fused(lay, np.identity(4))
    # rows org_r - occ .. org_r - 1 (the far edge of row 0 is 40 m ahead), columns org_c - occ/2 .. org_c + occ/2 - 1
    want = _pasted(lay, 30 - OCC, 18 - OCC // 2)
    assert np.array_equal(got, want)
    assert got[0].sum() == OCC * OCC and got[0].max() == 1
    assert np.array_equal(_fused(lay, np.identity(4)[:3]), want)            # 12 doubles: rows 0..2


@pytest.mark.parametrize("a,b", [(3, 5), (-7, -4), (0, 20), (14, 0), (-40, 0), (0, -60)])
def test_reference_whole_cell_translation_shifts_it(a, b):
    lay = _layout(5)
    T = np.identity(4)
    T[0, 3], T[2, 3] = a * RES, b * RES                     # a cells to the right, b cells forward (up the rows)
    got = _fused(lay, T)
    assert np.array_equal(got, _pasted(lay, 30 - OCC - b, 18 - OCC // 2 + a))
    if (a, b) in ((-40, 0), (0, -60)):
        assert got.sum() == 0                               # wholly off the map


def test_reference_quarter_turn_is_rot90():
    lay = _layout(7)
    # camera forward = world +X (to the right on the map), camera right = world -Z (down the map): the image turned clockwise
    got = _fused(lay, R.yaw_pose(90))
    assert np.array_equal(got, _pasted(np.rot90(lay, -1), 30 - OCC // 2, 18))
    got = _fused(lay, R.yaw_pose(180))
    assert np.array_equal(got, _pasted(np.rot90(lay, 2), 30, 18 - OCC // 2))
    got = _fused(lay, R.yaw_pose(270))
    assert np.array_equal(got, _pasted(np.rot90(lay, 1), 30 - OCC // 2, 18 - OCC))


def test_reference_skips_singular_and_nan_poses_and_honours_max_range():
    lay = _layout(9)
    T = np.identity(4)
    T[0, 0] = 1e-7
    assert _fused(lay, T).sum() == 0
    assert _fused(lay, np.full((4, 4), np.nan)).sum() == 0
    got = _fused(lay, np.identity(4), max_range=15.0)       # cell centres up to 15 m ahead: 6 rows of 2.5 m
    assert np.array_equal(got, _pasted(lay[OCC - 6:], 30 - 6, 18 - OCC // 2))


def test_reference_class_rule_and_marks():
    counts = np.zeros((1, 3, 2, 4), dtype=np.int32)
    #                 seen road car
    cells = [(0, 0, 0), (4, 2, 0), (4, 1, 0), (4, 0, 2), (4, 1, 1), (4, 0, 1), (3, 3, 0), (1, 0, 0)]
    for k, (s, r, c) in enumerate(cells):
        counts[0, :, k // 4, k % 4] = (s, r, c)
    cls, rgb = R.classes(counts, 1.0, 0.5, 0.5)
    assert cls.reshape(-1).tolist() == [255, 1, 0, 2, 1, 0, 1, 0]
    assert rgb[0, 0, 0].tolist() == [96, 96, 96] and rgb[0, 0, 1].tolist() == [255, 255, 255] and rgb[0, 0, 3].tolist() == [0, 0, 255]
    cls2, _ = R.classes(counts, 4.0, 0.5, 0.5)
    assert cls2.reshape(-1).tolist() == [255, 1, 0, 2, 1, 0, 255, 255]
    img = np.zeros((1, MH, MW, 3), dtype=np.uint8)
    traj = np.zeros((1, 4, 12))
    traj[0, 1, 3], traj[0, 1, 11] = 2.5, 5.0                # one cell right, two cells forward
    traj[0, 2, 3] = 1e9                                     # off the map
    traj[0, 3, 11] = np.nan
    R.mark(img, traj, 4, RES, ORG[0], ORG[1], (255, 0, 0))
    on = np.argwhere(img[0, :, :, 0] == 255).tolist()
    assert on == [[28, 19], [30, 18]]
