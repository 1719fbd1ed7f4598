"""Frozen inference block by block against float64: folding an eval-mode BatchNorm into its convolution must not cost accuracy.

Four blocks at B = 2 -- (a) BasicBlock 64 -> 64, stride 1, on 16x16; (b) BasicBlock 64 -> 128, stride 2 with its downsample
branch, on 16x16; (c) the ResNet stem (input normalisation, 7x7 / 2 convolution, BatchNorm, ReLU, 3x3 / 2 max-pool) on 3x32x32;
(d) the first `conv -> BN -> ReLU` stage of the BEV decoder at its real channel counts (128 -> 256, with a convolution bias) on
8x8 -- each run on today's eval route (jp_bn_eval_fwd behind the convolution) and on the frozen route, and compared with the
same block built from torch.nn.functional.conv2d / batch_norm(training=False) / relu in float64 on the CPU from the same
tensors.  gamma carries a negative entry, one of 1e-3 and one of exactly 0; running_var is drawn in [0.25, 4], the means are
non-zero.

    e = max |out - ref| / max |ref|   over EVERY output element;   required: e_frozen <= 4 * e_eager

The factor is a margin, not a measurement: folding adds one rounding per weight, so both errors are of one order, and the ratio
of two such maxima fluctuates from draw to draw.  The figures observed on an MI355X are in profiles/frozen_inference.md."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                                                  # noqa: E402
from jperceiver_amd.model import modules as M                                   # noqa: E402
from jperceiver_amd.ops import Var, ACT_RELU                                    # noqa: E402

DEV = "cuda"
B = 2


def _randomise(mod, seed):
    """Kaiming-like convolution weights, biases of a few tenths, BatchNorm tensors as described above."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.BatchNorm2d):
                C = m.num_features
                gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
                gamma[0], gamma[1], gamma[2] = -0.75, 1e-3, 0.0
                m.weight.copy_(gamma)
                m.bias.copy_(0.5 * torch.randn(C, generator=g))
                sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
                m.running_mean.copy_(sign * (0.2 + 0.8 * torch.rand(C, generator=g)))
                m.running_var.copy_(0.25 + 3.75 * torch.rand(C, generator=g))
    return mod


def _d(t):
    return t.detach().cpu().double()


def _conv64(conv, x):
    return F.conv2d(x, _d(conv.weight), None if conv.bias is None else _d(conv.bias), conv.stride, conv.padding)


def _bn64(bn, x):
    return F.batch_norm(x, _d(bn.running_mean), _d(bn.running_var), _d(bn.weight), _d(bn.bias), False, 0.0, bn.eps)


def _block64(blk, x):
    out = F.relu(_bn64(blk.bn1, _conv64(blk.conv1, x)))
    out = _bn64(blk.bn2, _conv64(blk.conv2, out))
    res = x if blk.downsample is None else _bn64(blk.downsample[1], _conv64(blk.downsample[0], x))
    return [F.relu(out + res)]


def _case_block(stride):
    planes = 64 if stride == 1 else 128
    ds = None if stride == 1 else nn.Sequential(nn.Conv2d(64, planes, 1, stride, bias=False), M.BatchNorm2d(planes))
    blk = _randomise(M.BasicBlock(64, planes, stride, ds), seed=10 + stride).eval()
    x = torch.randn(B, 64, 16, 16, generator=torch.Generator().manual_seed(20 + stride))
    ref = _block64(blk, x.double())
    blk.to(DEV)
    return blk, ref, lambda: [blk._fwd(Var(x.to(DEV))).t]


def _case_stem():
    net = M.ResNet()
    for name in ("layer1", "layer2", "layer3", "layer4"):
        setattr(net, name, nn.Sequential())                   # the stem alone: features() then returns [level 0, pooled x 4]
    _randomise(net, seed=31).eval()
    x = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(32))
    f0 = F.relu(_bn64(net.bn1, _conv64(net.conv1, (x.double() - 0.45) / 0.225)))
    ref = [f0, F.max_pool2d(f0, 3, 2, 1)]
    net.to(DEV)

    def run():
        feats = net.features(Var(x.to(DEV)), need_f0=True)
        return [feats[0].t, feats[1].t]

    return net, ref, run


def _case_decoder_stage():
    dec = _randomise(M.Decoder(np.array([64, 64, 128, 256, 512])), seed=41).eval()
    c0, b0 = dec.decoder[0], dec.decoder[1]
    assert (c0.in_channels, c0.out_channels) == (128, 256) and c0.bias is not None
    x = torch.randn(B, 128, 8, 8, generator=torch.Generator().manual_seed(42))
    ref = [F.relu(_bn64(b0, _conv64(c0, x.double())))]
    dec.to(DEV)

    def run():
        fz = M.frozen_of(c0, b0)
        xv = Var(x.to(DEV))
        if fz is not None:
            return [fz.apply(xv, ACT_RELU).t]
        return [M.bn_apply(b0, M.conv_apply(c0, xv), relu=True).t]

    return dec, ref, run


CASES = {"a_block_64_64_s1": lambda: _case_block(1), "b_block_64_128_s2_downsample": lambda: _case_block(2),
         "c_stem_7x7_s2_maxpool": _case_stem, "d_bev_decoder_stage_128_256": _case_decoder_stage}


def _err(outs, refs):
    e = 0.0
    for o, r in zip(outs, refs):
        o = o.cpu().double()
        assert o.shape == r.shape and torch.isfinite(o).all()
        e = max(e, float((o - r).abs().max() / r.abs().max()))
    return e


@pytest.mark.parametrize("name", list(CASES))
def test_frozen_block_is_as_close_to_float64_as_the_eval_route(name, monkeypatch):
    mod, ref, run = CASES[name]()
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda n, *a: (calls.append(n), real(n, *a))[1])
    e_eager = _err(run(), ref)
    n_bn = calls.count("jp_bn_eval_fwd")
    assert n_bn >= 1 and "jp_add_relu" not in calls and "jp_bn_fold_conv" not in calls
    M.freeze_module(mod)
    del calls[:]
    e_frozen = _err(run(), ref)
    assert "jp_bn_eval_fwd" not in calls                       # the frozen route really ran
    assert calls.count("jp_add_relu") == (1 if "block" in name and name[0] in "ab" else 0)
    print(f"frozen block {name}: e_frozen {e_frozen:.3e}  e_eager {e_eager:.3e}  ratio {e_frozen / e_eager:.2f}  "
          f"({n_bn} BatchNorm passes folded away)")
    assert e_eager > 0
    assert e_frozen <= 4.0 * e_eager, (name, e_frozen, e_eager)
