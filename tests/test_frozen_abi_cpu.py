"""CPU-side checks of frozen inference: the two entry points of csrc/frozen.hip are declared and exported, refuse null pointers
and non-positive sizes with the library's argument error before anything touches a device, the entry point they stand in for keeps
its signature (the change is additive; the ABI version itself is tests/test_abi.py's to pin), and the public names import, attach their state without a GPU and refuse a training-mode model."""
import ctypes
import re
import subprocess

import pytest
import torch

from jperceiver_amd import _lib

SYMBOLS = ("jp_bn_fold_conv", "jp_add_relu")
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
    assert [a for _, a in protos["jp_bn_fold_conv"][1]] == ["w", "conv_bias", "gamma", "beta", "running_mean", "running_var", "eps",
                                                            "w_out", "bias_out", "Cout", "K", "stream"]
    assert [a for _, a in protos["jp_add_relu"][1]] == ["a", "b", "out", "n", "relu", "amax_out", "stream"]
    # existing entry points keep their signatures: the BatchNorm they replace on the frozen route is still there as it was
    assert [a for _, a in protos["jp_bn_eval_fwd"][1]] == ["x", "gamma", "beta", "running_mean", "running_var", "residual", "y", "N",
                                                           "C", "HW", "eps", "relu", "stream"]


def _rejected(L, name, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn[name](*args)
    assert rc == -1, (name, args, rc)
    msg = L.last_error()
    assert msg, (name, args)
    return msg


def test_bn_fold_conv_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, None, P, P, P, P, 1e-5, P, P, 5, 147, None]          # conv_bias is optional
    for i in (0, 2, 3, 4, 5, 7, 8):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_bn_fold_conv", *a)
    for i in (9, 10):
        for bad in (0, -3):
            a = list(good)
            a[i] = bad
            assert "positive" in _rejected(L, "jp_bn_fold_conv", *a)
    a = list(good)
    a[6] = -1.0
    assert "eps" in _rejected(L, "jp_bn_fold_conv", *a)


def test_add_relu_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, P, 16, 1, None, None]                              # amax_out is optional
    for i in (0, 1, 2):
        a = list(good)
        a[i] = None
        assert "null" in _rejected(L, "jp_add_relu", *a)
    for bad in (0, -1, -(1 << 40)):
        a = list(good)
        a[3] = bad
        assert "positive" in _rejected(L, "jp_add_relu", *a)


def test_public_api_attaches_state_and_refuses_a_training_mode_model():
    from jperceiver_amd import ops
    from jperceiver_amd.apis import Perceiver, freeze, unfreeze
    from jperceiver_amd.model import MONO, modules as M
    from oracle import jp_oracle as J
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt)
    assert net.training
    with pytest.raises(RuntimeError, match="eval-mode"):
        freeze(net)
    with pytest.raises(RuntimeError, match="eval-mode"):
        freeze(net.DepthEncoder)
    net.eval()
    keys = list(net.state_dict())
    assert freeze(net) is net and M.is_frozen(net)
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 100 and all("_frozen" in b.__dict__ for b in bns)       # 3 x 20 encoder + 4 x 10 decoder BatchNorms, all conv-fed
    assert list(net.state_dict()) == keys                                       # the folded tensors are no part of a checkpoint
    # one BatchNorm alone back in train mode: its pair (and with it its block) is off the frozen route
    blk = net.DepthEncoder.encoder.layer1[0]
    assert M.frozen_of(blk.conv1, blk.bn1.train()) is None
    blk.bn1.eval()
    with pytest.raises(RuntimeError, match="GPU"):                              # folding is a HIP kernel: no CPU path
        M.frozen_of(blk.conv1, blk.bn1)
    assert unfreeze(net) is net and not M.is_frozen(net)
    assert M.frozen_of(blk.conv1, blk.bn1) is None
    Perceiver(net)
    assert not M.is_frozen(net)
    Perceiver(net, frozen=True)
    assert M.is_frozen(net)
    with pytest.raises(RuntimeError):
        Perceiver(net.train(), frozen=True)
    # ops.add_relu is forward-only
    with ops.recording(ops.Tape()), pytest.raises(RuntimeError, match="forward-only"):
        ops.add_relu(ops.Var(torch.zeros(4)), ops.Var(torch.zeros(4)))


def test_a_pair_that_cannot_be_folded_is_refused_by_the_constructor():
    from jperceiver_amd.model import modules as M
    conv = torch.nn.Conv2d(4, 8, 3, padding=1)
    M.FrozenConvBN(conv, M.BatchNorm2d(8))
    with pytest.raises(ValueError, match="BatchNorm2d"):                        # a plain torch BatchNorm keeps no count of train-mode forwards
        M.FrozenConvBN(conv, torch.nn.BatchNorm2d(8))
    with pytest.raises(ValueError):
        M.FrozenConvBN(torch.nn.Linear(4, 8), M.BatchNorm2d(8))
    with pytest.raises(ValueError, match="does not sit behind"):
        M.FrozenConvBN(conv, M.BatchNorm2d(4))
    with pytest.raises(ValueError, match="does not sit behind"):
        M.FrozenConvBN(torch.nn.Conv2d(4, 8, 3, padding=1, padding_mode="reflect"), M.BatchNorm2d(8))
