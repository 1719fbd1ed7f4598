"""CPU-side checks of the streaming perception feature (csrc/stream.hip, apis/stream.py): the two entry points are declared in
the header, exported by the library and bound; the ABI version is unchanged (the change is additive); the argument names are
the documented ones; null and non-positive arguments are refused with a message before anything touches a device; and
`PerceptionStream` imports, refuses a train-mode model, refuses a model that is not on the GPU (there is no CPU path: a session
cannot take frames without a device) and refuses frames that are not raw uint8 camera frames of the session's shape."""
import ctypes
import re
import subprocess

import pytest
import torch

from jperceiver_amd import _lib

SYMBOLS = ("jp_stream_pose_pair", "jp_stream_traj_push")
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
    assert [a for _, a in protos["jp_stream_pose_pair"][1]] == ["frame", "ring", "count", "pair", "amax_out", "B", "H", "W", "stream"]
    assert [a for _, a in protos["jp_stream_traj_push"][1]] == ["T", "pose", "traj", "count", "B", "capacity", "stream"]
    # element types the binding checks tensors against: the counter is int32, pose and trajectory are float64
    assert [t for t, _ in protos["jp_stream_pose_pair"][1]][:5] == ["const float*", "float*", "const int*", "float*", "float*"]
    assert [t for t, _ in protos["jp_stream_traj_push"][1]][:4] == ["const float*", "double*", "double*", "int*"]


def _rejected(L, name, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn[name](*args)
    assert rc == -1, (name, args, rc)
    msg = L.last_error()
    assert msg, (name, args)
    return msg


def test_pose_pair_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, P, P, None, 2, 40, 56, None]              # amax_out is optional
    for i in (0, 1, 2, 3):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_stream_pose_pair", *a)
    for i in (5, 6, 7):
        for bad in (0, -3):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_stream_pose_pair", *a)


def test_traj_push_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, P, P, 2, 4, None]
    for i in (0, 1, 2, 3):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_stream_traj_push", *a)
    for i in (4, 5):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_stream_traj_push", *a)


def test_perception_stream_imports_and_refuses_what_it_cannot_run():
    from jperceiver_amd.apis import PerceptionStream, StreamFrame, Perceiver
    from jperceiver_amd.model import MONO
    from oracle import jp_oracle as J
    assert StreamFrame._fields == ("index", "disp", "depth", "layout", "cam_T_cam", "pose")
    assert callable(Perceiver.stream)
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt)
    assert net.training
    with pytest.raises(RuntimeError, match="eval-mode"):
        PerceptionStream(net, (94, 311))
    with pytest.raises(RuntimeError, match="eval-mode"):
        net.eval_branch("depth_encoder", None)
    # an eval-mode model on the CPU: the session runs HIP kernels only, so neither it nor CPU frames have a path
    with pytest.raises(RuntimeError, match="GPU"):
        PerceptionStream(net.eval(), (94, 311))
    with pytest.raises(RuntimeError, match="GPU"):
        Perceiver(net).stream((94, 311))
    # the frame check fires before anything is enqueued: float frames (what `perceive` takes) and wrong shapes are refused
    s = PerceptionStream.__new__(PerceptionStream)
    s.cameras, s.src_hw, s.dev = 2, (94, 311), torch.device("cuda", 0)
    with pytest.raises(TypeError, match="uint8"):
        s._check_frames(torch.zeros(2, 94, 311, 3))
    with pytest.raises(TypeError, match="uint8"):
        s._check_frames(None)
    for shape in ((1, 94, 311, 3), (2, 3, 94, 311), (2, 94, 311)):
        with pytest.raises(ValueError, match="shape"):
            s._check_frames(torch.zeros(shape, dtype=torch.uint8))
    s._check_frames(torch.zeros(2, 94, 311, 3, dtype=torch.uint8))      # host frames of the right kind pass the check
