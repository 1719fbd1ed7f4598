"""CPU-side checks of the odometry evaluation feature: the seven entry points of csrc/odometry.hip are declared and exported with
the documented argument names, refuse null pointers and out-of-range integers with a message before anything touches a device, the
ABI version is unchanged (the change is additive), the public names import and refuse CPU tensors, and the KITTI pose text files
round-trip."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib

SYMBOLS = ("jp_pose_chain_ws_bytes", "jp_pose_chain_f64", "jp_odom_segments_ws_bytes", "jp_odom_segment_errors",
           "jp_traj_moments_ws_bytes", "jp_traj_moments", "jp_poses_transform_f64")
P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: validation comes first
LENGTHS = (ctypes.c_double * 8)(100, 200, 300, 400, 500, 600, 700, 800)
LP = ctypes.c_void_p(ctypes.addressof(LENGTHS))
A12 = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
AP = ctypes.c_void_p(ctypes.addressof(A12))


def test_new_symbols_are_declared_and_exported():
    L = _lib.lib()
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (jp_\w+)", out))
    for s in SYMBOLS:
        assert s in protos, s
        assert s in exported, s
        assert s in L.fn
    assert L.fn["jp_abi_version"]() == 3
    names = lambda f: [a for _, a in protos[f][1]]                                         # noqa: E731
    assert names("jp_pose_chain_ws_bytes") == ["n"]
    assert names("jp_pose_chain_f64") == ["T", "n", "invert", "poses", "ws", "stream"]
    assert names("jp_odom_segments_ws_bytes") == ["n", "step", "nlen"]
    assert names("jp_odom_segment_errors") == ["gt", "pred", "n", "step", "lengths", "nlen", "dist", "last_frame", "table", "ws",
                                               "stream"]
    assert names("jp_traj_moments_ws_bytes") == ["n"]
    assert names("jp_traj_moments") == ["x", "y", "n", "out", "ws", "stream"]
    assert names("jp_poses_transform_f64") == ["poses", "n", "A", "scale", "out", "stream"]
    for f in ("jp_pose_chain_ws_bytes", "jp_odom_segments_ws_bytes", "jp_traj_moments_ws_bytes"):
        assert protos[f][0] == "long"


def _rejected(L, name, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn[name](*args)
    assert rc == -1, (name, args, rc)
    msg = L.last_error()
    assert msg, (name, args)
    return msg


def test_pose_chain_rejects_bad_arguments():
    L = _lib.lib()
    for bad in (0, -1):
        _rejected(L, "jp_pose_chain_ws_bytes", bad)
    # one 12-double aggregate per block of 256 transforms
    assert L.fn["jp_pose_chain_ws_bytes"](1) == 96 and L.fn["jp_pose_chain_ws_bytes"](256) == 96
    assert L.fn["jp_pose_chain_ws_bytes"](257) == 192 and L.fn["jp_pose_chain_ws_bytes"](16384) == 64 * 96
    good = [P, 10, 1, P, P, None]
    for i in (0, 3, 4):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_pose_chain_f64", *a)
    for bad in (0, -7):
        a = list(good)
        a[1] = bad
        _rejected(L, "jp_pose_chain_f64", *a)


def test_segment_errors_reject_bad_arguments():
    L = _lib.lib()
    for args in ((0, 10, 8), (-1, 10, 8), (100, 0, 8), (100, -2, 8), (100, 10, 0), (100, 10, 17), (100, 10, -1)):
        _rejected(L, "jp_odom_segments_ws_bytes", *args)
    assert L.fn["jp_odom_segments_ws_bytes"](4661, 10, 8) > 0
    good = [P, P, 100, 10, LP, 8, P, P, P, P, None]
    for i in (0, 1, 4, 6, 7, 8, 9):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_odom_segment_errors", *a)
    for i, bads in ((2, (0, -1)), (3, (0, -10)), (5, (0, -1, 17))):
        for bad in bads:
            a = list(good)
            a[i] = bad
            _rejected(L, "jp_odom_segment_errors", *a)
    for badlen in (0.0, -100.0, float("nan")):
        lb = (ctypes.c_double * 2)(100.0, badlen)
        a = list(good)
        a[4], a[5] = ctypes.c_void_p(ctypes.addressof(lb)), 2
        assert "positive" in _rejected(L, "jp_odom_segment_errors", *a)


def test_moments_and_transform_reject_bad_arguments():
    L = _lib.lib()
    for bad in (0, -1):
        _rejected(L, "jp_traj_moments_ws_bytes", bad)
    assert L.fn["jp_traj_moments_ws_bytes"](1) > 0
    assert L.fn["jp_traj_moments_ws_bytes"](10 ** 6) == L.fn["jp_traj_moments_ws_bytes"](10 ** 7)      # a bounded number of partials
    good = [P, P, 100, P, P, None]
    for i in (0, 1, 3, 4):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_traj_moments", *a)
    for bad in (0, -3):
        a = list(good)
        a[2] = bad
        _rejected(L, "jp_traj_moments", *a)
    good = [P, 100, AP, 2.0, P, None]
    for i in (0, 2, 4):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_poses_transform_f64", *a)
    for bad in (0, -3):
        a = list(good)
        a[1] = bad
        _rejected(L, "jp_poses_transform_f64", *a)


def test_public_api_imports_and_refuses_cpu_tensors():
    from jperceiver_amd.apis import (chain_poses_device, odometry_device, evaluate_odometry, read_kitti_poses,      # noqa: F401
                                     write_kitti_poses)
    from jperceiver_amd.core.evaluation import umeyama_alignment, align_poses, eval_odometry
    T = torch.eye(4).repeat(3, 1, 1)
    with pytest.raises(RuntimeError):
        chain_poses_device(T)
    traj = torch.eye(4, dtype=torch.float64)[:3].reshape(1, 12).repeat(5, 1)
    with pytest.raises(RuntimeError):
        umeyama_alignment(traj, traj, True)
    with pytest.raises(RuntimeError):
        align_poses(traj, traj, "7dof")
    with pytest.raises(RuntimeError):
        eval_odometry(traj, traj)
    with pytest.raises(_lib.JPerceiverHipError):
        _lib.call("jp_traj_moments", traj, traj, 5, torch.zeros(19, dtype=torch.float64), torch.zeros(8, dtype=torch.uint8))


def test_kitti_pose_files_round_trip(tmp_path):
    from jperceiver_amd.apis import read_kitti_poses, write_kitti_poses
    rng = np.random.default_rng(0)
    poses = rng.standard_normal((7, 12)) * np.array([1, 1, 1, 300] * 3)
    p12 = tmp_path / "12.txt"
    write_kitti_poses(p12, poses)
    first = p12.read_text().splitlines()[0].split(" ")
    assert len(first) == 12 and all(re.fullmatch(r"-?\d\.\d{8}e[+-]\d\d", w) for w in first)       # '%1.8e', as the script writes
    back = read_kitti_poses(p12)
    assert back.shape == (7, 12) and back.dtype == np.float64
    np.testing.assert_allclose(back, poses, rtol=1e-8)                # 9 significant digits: half a unit of the ninth
    write_kitti_poses(p12, torch.from_numpy(back))                    # tensors too; a second trip is exact
    assert np.array_equal(read_kitti_poses(p12), back)
    p13 = tmp_path / "13.txt"                                         # loadPoses' second layout: the frame index first
    np.savetxt(p13, np.concatenate([np.arange(7)[:, None], back], 1), fmt="%1.8e")
    assert np.array_equal(read_kitti_poses(p13), back)
    one = tmp_path / "one.txt"                                        # a single line stays (1, 12)
    write_kitti_poses(one, back[:1])
    assert read_kitti_poses(one).shape == (1, 12)
    bad = tmp_path / "bad.txt"
    np.savetxt(bad, back[:, :11])
    with pytest.raises(ValueError):
        read_kitti_poses(bad)
