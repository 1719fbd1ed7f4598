"""CPU-side checks of the video perception feature: the five entry points of csrc/perception.hip are declared and exported,
refuse null / non-positive arguments with a message before anything touches a device, the ABI version is unchanged (the
change is additive), and the public names import and refuse a training-mode model."""
import ctypes
import re
import subprocess

import pytest
import torch

from jperceiver_amd import _lib

SYMBOLS = ("jp_disp_resize_depth", "jp_quantiles_ws_bytes", "jp_quantiles", "jp_colorize_u8", "jp_layout_classes_u8")
P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: validation comes first


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
    # the documented shapes of the calls
    assert [a for _, a in protos["jp_disp_resize_depth"][1]] == ["disp", "depth_out", "disp_out", "B", "h", "w", "OH", "OW", "min_depth",
                                                                 "max_depth", "stream"]
    assert [a for _, a in protos["jp_quantiles"][1]] == ["x", "rows", "n", "q", "nq", "out", "ws", "stream"]
    assert [a for _, a in protos["jp_colorize_u8"][1]] == ["x", "rows", "n", "vmin_vmax", "lut", "out", "stream"]
    assert [a for _, a in protos["jp_layout_classes_u8"][1]] == ["road_logits", "car_logits", "cls", "rgb", "B", "HW", "stream"]


def _rejected(L, name, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn[name](*args)
    assert rc == -1, (name, args, rc)
    msg = L.last_error()
    assert msg, (name, args)
    return msg


def test_disp_resize_depth_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, None, 1, 4, 4, 8, 8, 0.1, 100.0, None]
    for i in (0, 1):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_disp_resize_depth", *a)
    for i in (3, 4, 5, 6, 7):
        for bad in (0, -3):
            a = list(good)
            a[i] = bad
            _rejected(L, "jp_disp_resize_depth", *a)
    for lo, hi in ((0.0, 100.0), (-1.0, 100.0), (5.0, 5.0), (5.0, 1.0)):
        a = list(good)
        a[8], a[9] = lo, hi
        assert "depth" in _rejected(L, "jp_disp_resize_depth", *a)


def test_quantiles_reject_bad_arguments():
    L = _lib.lib()
    for bad in (0, -1, 65):
        _rejected(L, "jp_quantiles_ws_bytes", bad)
    assert L.fn["jp_quantiles_ws_bytes"](1) > 0
    assert L.fn["jp_quantiles_ws_bytes"](64) == 64 * L.fn["jp_quantiles_ws_bytes"](1)
    q = (ctypes.c_float * 4)(0.0, 0.5, 0.95, 1.0)
    qp = ctypes.c_void_p(ctypes.addressof(q))
    good = [P, 2, 100, qp, 4, P, P, None]
    for i in (0, 3, 5, 6):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_quantiles", *a)
    for i, bads in ((1, (0, -1, 65)), (2, (0, -5)), (4, (0, -1, 5))):
        for bad in bads:
            a = list(good)
            a[i] = bad
            _rejected(L, "jp_quantiles", *a)
    for badq in (-0.25, 1.5, float("nan")):
        qb = (ctypes.c_float * 1)(badq)
        a = list(good)
        a[3], a[4] = ctypes.c_void_p(ctypes.addressof(qb)), 1
        assert "[0,1]" in _rejected(L, "jp_quantiles", *a)


def test_colorize_and_layout_classes_reject_bad_arguments():
    L = _lib.lib()
    good = [P, 2, 16, P, P, P, None]
    for i in (0, 3, 4, 5):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_colorize_u8", *a)
    for i in (1, 2):
        for bad in (0, -2):
            a = list(good)
            a[i] = bad
            _rejected(L, "jp_colorize_u8", *a)
    good = [P, None, P, None, 2, 16, None]               # car_logits and rgb are optional
    for i in (0, 2):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_layout_classes_u8", *a)
    for i in (4, 5):
        for bad in (0, -2):
            a = list(good)
            a[i] = bad
            _rejected(L, "jp_layout_classes_u8", *a)


def test_public_api_imports_and_refuses_a_training_mode_model():
    from jperceiver_amd.apis import Perceiver, colorize_disp, layout_rgb, default_lut
    from jperceiver_amd.model import MONO
    from oracle import jp_oracle as J
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt)
    assert net.training
    with pytest.raises(RuntimeError):
        Perceiver(net)
    with pytest.raises(RuntimeError):
        net.predict_poses({("color_aug", 0, 0): torch.zeros(1, 3, 256, 256)})
    p = Perceiver(net.eval(), out_size=(375, 1242))
    assert (p.min_depth, p.max_depth) == (float(opt.min_depth), float(opt.max_depth)) and p.out_size == (375, 1242)
    with pytest.raises(RuntimeError):
        net.predict_poses({("color_aug", 0, 0): torch.zeros(1, 3, 256, 256), ("color_aug", -1, 0): torch.zeros(1, 3, 256, 256)},
                          frame_ids=[0, -1])            # eval mode, CPU tensors: the product path has no CPU fallback
    # the kernels take device tensors only; the checks fire before a stream is touched
    with pytest.raises(TypeError):
        colorize_disp(torch.zeros(1, 1, 8, 8), default_lut())
    with pytest.raises(TypeError):
        layout_rgb(torch.zeros(1, 8, 8, dtype=torch.uint8))
    lut = default_lut()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)
