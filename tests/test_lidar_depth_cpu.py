"""CPU-side checks of the LiDAR depth ground truth and the batched depth scorer: the KITTI calibration readers reproduce the
reference's projection matrix on the golden calibration files (tests/golden/lidar_depth_*.npz, tools/make_lidar_golden.py), the four
new entry points are declared and exported, refuse bad arguments with a message before anything touches a device, and their
workspace sizes are positive and grow with B; the ABI version is unchanged (the change is additive)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib
from jperceiver_amd.datasets.kitti_calib import load_velodyne_points, read_calib_file, velo_to_image

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYMBOLS = ("jp_lidar_depth_ws_bytes", "jp_lidar_depth_map", "jp_depth_eval_batch_ws_bytes", "jp_depth_eval_batch")
P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: validation comes first


def _write_calib(tmp_path, g):
    (tmp_path / "calib_cam_to_cam.txt").write_text(str(g["cam2cam_txt"]))
    (tmp_path / "calib_velo_to_cam.txt").write_text(str(g["velo2cam_txt"]))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_velo_to_image_reproduces_the_reference_matrix(tmp_path, tag):
    g = np.load(os.path.join(GOLD, f"lidar_depth_{tag}.npz"))
    _write_calib(tmp_path, g)
    Pm, hw = velo_to_image(str(tmp_path), cam=int(g["cam"]))
    assert Pm.shape == (3, 4) and Pm.dtype == np.float64
    assert hw == tuple(int(v) for v in g["hw"])
    # the same three float64 products in the same order: 1e-15 relative (of each row's largest entry) is a few ulps
    assert (np.abs(Pm - g["P"]) <= 1e-15 * np.abs(g["P"]).max(1, keepdims=True)).all()
    other = velo_to_image(str(tmp_path), cam=5 - int(g["cam"]))[0]
    assert np.abs(other - g["P"]).max() > 1.0                       # the other camera's baseline term


def test_read_calib_file_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    data = {"S_rect_02": np.array([1242.0, 375.0]), "R_rect_00": rng.standard_normal(9), "P_rect_02": rng.standard_normal(12) * 700,
            "T": rng.standard_normal(3)}
    lines = ["calib_time: 09-Jan-2012 13:57:47"] + [k + ": " + " ".join(repr(float(v)) for v in a) for k, a in data.items()]
    path = tmp_path / "calib.txt"
    path.write_text("\n".join(lines) + "\n")
    back = read_calib_file(path)
    assert back["calib_time"] == "09-Jan-2012 13:57:47"             # not numbers: kept as text (the colons of the time included)
    assert set(back) == set(data) | {"calib_time"}
    for k, a in data.items():
        assert back[k].dtype == np.float64 and np.array_equal(back[k], a), k
    # '%.6e', the format of the KITTI files
    path.write_text("R: " + " ".join("%.6e" % v for v in data["R_rect_00"]) + "\n")
    np.testing.assert_allclose(read_calib_file(path)["R"], data["R_rect_00"], rtol=1e-6)


def test_load_velodyne_points(tmp_path):
    pts = np.random.default_rng(1).standard_normal((37, 4)).astype(np.float32)
    f = tmp_path / "0000000000.bin"
    pts.tofile(f)
    back = load_velodyne_points(f)
    assert back.dtype == np.float32 and np.array_equal(back, pts)
    pts.reshape(-1)[:-1].tofile(f)
    with pytest.raises(ValueError):
        load_velodyne_points(f)


def test_new_symbols_are_declared_and_exported():
    L = _lib.lib()
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (jp_\w+)", out))
    for s in SYMBOLS:
        assert s in protos and s in exported and s in L.fn, s
    assert L.fn["jp_abi_version"]() == 3
    names = lambda f: [a for _, a in protos[f][1]]                                         # noqa: E731
    assert names("jp_lidar_depth_ws_bytes") == ["B", "H", "W"]
    assert names("jp_lidar_depth_map") == ["pts", "offsets", "P", "flip", "B", "H", "W", "vel_depth", "out64", "out32", "ws", "stream"]
    assert names("jp_depth_eval_batch_ws_bytes") == ["B", "H", "W"]
    assert names("jp_depth_eval_batch") == ["disp", "gt", "B", "h", "w", "H", "W", "y0", "y1", "x0", "x1", "mask_min", "mask_max",
                                            "min_depth", "max_depth", "fixed_scale", "sums", "med", "ws", "stream"]
    for f in ("jp_lidar_depth_ws_bytes", "jp_depth_eval_batch_ws_bytes"):
        assert protos[f][0] == "long"


def _rejected(L, name, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn[name](*args)
    assert rc == -1, (name, args, rc)
    msg = L.last_error()
    assert msg, (name, args)
    return msg


@pytest.mark.parametrize("name", ["jp_lidar_depth_ws_bytes", "jp_depth_eval_batch_ws_bytes"])
def test_ws_bytes_positive_monotone_and_checked(name):
    L = _lib.lib()
    for bad in ((0, 375, 1242), (-1, 375, 1242), (1, 0, 1242), (1, 375, 0), (1, -3, 1242), (1, 375, -7)):
        _rejected(L, name, *bad)
    sizes = [L.fn[name](B, 375, 1242) for B in (1, 2, 3, 8, 64)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    assert L.fn[name](1, 20, 48) > 0


def test_lidar_depth_ws_holds_keys_and_border_indices():
    # one 64-bit key per pixel + first / last point index for the two border columns of every row
    assert _lib.lib().fn["jp_lidar_depth_ws_bytes"](3, 20, 48) == 3 * (20 * 48 + 4 * 20) * 8
    _rejected(_lib.lib(), "jp_lidar_depth_ws_bytes", 1, 20, 1)      # the shared key needs two border columns


def test_lidar_depth_map_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, P, None, 2, 20, 48, 0, P, P, P, None]             # flip may be NULL
    for i in (0, 1, 2, 10):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_lidar_depth_map", *a)
    a = list(good)
    a[8] = a[9] = None                                               # both outputs missing
    assert "null" in _rejected(L, "jp_lidar_depth_map", *a)
    for i, bads in ((4, (0, -1)), (5, (0, -20)), (6, (1, 0, -48))):
        for bad in bads:
            a = list(good)
            a[i] = bad
            _rejected(L, "jp_lidar_depth_map", *a)


def test_depth_eval_batch_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, 3, 24, 80, 37, 124, 15, 36, 4, 119, 1e-3, 80.0, 0.1, 100.0, 0.0, P, P, P, None]
    for i in (0, 1, 16, 17, 18):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_depth_eval_batch", *a)
    for i in (2, 3, 4, 5, 6):
        for bad in (0, -2):
            a = list(good)
            a[i] = bad
            _rejected(L, "jp_depth_eval_batch", *a)
    for i in (13, 14):
        a = list(good)
        a[i] = 0.0
        _rejected(L, "jp_depth_eval_batch", *a)


def test_public_api_imports_and_refuses_cpu_tensors():
    from jperceiver_amd.apis import evaluate_depth_lidar                                                             # noqa: F401
    from jperceiver_amd.core.evaluation import eval_depth_batch, generate_depth_map, lidar_depth_maps               # noqa: F401
    with pytest.raises(RuntimeError):
        eval_depth_batch(torch.rand(2, 1, 24, 80), torch.rand(2, 37, 124))
    with pytest.raises(ValueError):
        lidar_depth_maps([np.zeros((5, 3), np.float32)], np.zeros((3, 4)), (20, 48))
    with pytest.raises(ValueError):
        lidar_depth_maps([], np.zeros((3, 4)), (20, 48))
