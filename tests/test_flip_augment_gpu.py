"""Horizontal flip + batched ColorJitter of the device-side input pipeline on the GPU.

The flip is pinned through a double mirror against Pillow's own output (tests/golden/preprocess.npz): a flagged item whose
source was mirrored on the host must reproduce the golden output of the unmirrored image exactly.  The batched jitter is
held to the torchvision restatement with the bound of the per-op path (2e-5) and to bit-equality between two runs.
Every buffer the pipeline allocates is poisoned first (NaN, 0xFF for uint8), so an element a kernel does not write shows."""
import os

import numpy as np
import pytest
import torch

from jperceiver_amd import synthetic as syn
from jperceiver_amd.datasets import ColorJitterParams
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu

RESIZE = ["down", "up", "mixed", "same_w"]
CALIB = ("K", "inv_K", "odometry_K", "Tr_cam2_velo")


@pytest.fixture(autouse=True)
def poisoned_buffers(monkeypatch):
    """torch.empty hands out NaN / 0xFF: the output and scratch buffers DevicePreprocessor allocates are poisoned before each call"""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(0xFF)
        return t
    monkeypatch.setattr(torch, "empty", empty)


def _mirror(a):
    return np.ascontiguousarray(a[:, ::-1])


def _flags(bits):
    return torch.tensor(bits, dtype=torch.uint8).cuda()


def _both_batches(img):
    """[img, mirrored, img] with flags [0,1,0] and the complementary batch: every item must come out as the unmirrored resize"""
    m = _mirror(img)
    yield torch.from_numpy(np.stack([img, m, img])).cuda(), _flags([0, 1, 0])
    yield torch.from_numpy(np.stack([m, img, m])).cuda(), _flags([1, 0, 1])


def test_flipped_resize_is_bit_exact_pillow():
    from jperceiver_amd.datasets import DevicePreprocessor
    g = np.load(os.path.join(GOLDEN, "preprocess.npz"))
    pre = DevicePreprocessor(64, 64, "cuda")
    for name in RESIZE:
        H, W, OH, OW = (int(v) for v in g[f"resize/{name}/shape"])
        img = (syn.hash_uniform(21, ("pp", name), (H, W, 3)) * 256).astype(np.uint8)
        gold = g[f"resize/{name}/out"]
        ref = torch.from_numpy(gold).permute(2, 0, 1).float() / 255.0                                 # ToTensor
        for batch, flags in _both_batches(img):
            f, u8 = pre.resize_u8(batch, OH, OW, want_u8=True, flip=flags)
            for i in range(3):
                np.testing.assert_array_equal(u8[i].cpu().numpy(), gold, err_msg=f"{name} item {i}")
                assert torch.equal(f[i].cpu(), ref), (name, i)
            assert torch.equal(pre.resize_u8(batch, OH, OW, flip=flags), f)                          # without the uint8 output
            # no flags, and flags that are all zero: the existing path, bit for bit
            f0, u0 = pre.resize_u8(batch, OH, OW, want_u8=True)
            fn, un = pre.resize_u8(batch, OH, OW, want_u8=True, flip=None)
            fz, uz = pre.resize_u8(batch, OH, OW, want_u8=True, flip=_flags([0, 0, 0]))
            assert torch.equal(f0, fn) and torch.equal(u0, un) and torch.equal(f0, fz) and torch.equal(u0, uz), name
    img = (syn.hash_uniform(21, ("pp", "chain"), (80, 200, 3)) * 256).astype(np.uint8)
    for batch, flags in _both_batches(img):
        full, full8 = pre.resize_u8(batch, 38, 124, want_u8=True, flip=flags)
        net, net8 = pre.resize_u8(full8, 64, 64, want_u8=True)
        for i in range(3):
            np.testing.assert_array_equal(full8[i].cpu().numpy(), g["resize/chain/full"])
            np.testing.assert_array_equal(net8[i].cpu().numpy(), g["resize/chain/net"])
            assert torch.equal(full[i].cpu(), torch.from_numpy(g["resize/chain/full"]).permute(2, 0, 1).float() / 255.0)


@pytest.mark.parametrize("C", [3, 1])
def test_flip_without_a_resize_is_a_mirror(C):
    from jperceiver_amd.datasets import DevicePreprocessor
    pre = DevicePreprocessor(7, 13, "cuda")
    x = (syn.hash_uniform(23, ("same", C), (3, 7, 13, C)) * 256).astype(np.uint8)
    want = x.copy()
    want[1] = x[1][:, ::-1]
    f, u8 = pre.resize_u8(torch.from_numpy(x).cuda(), 7, 13, want_u8=True, flip=_flags([0, 1, 0]))
    np.testing.assert_array_equal(u8.cpu().numpy(), want)
    assert torch.equal(f.cpu(), torch.from_numpy(want).permute(0, 3, 1, 2).float() / 255.0)
    f1 = pre.resize_u8(torch.from_numpy(x).cuda(), 7, 13, flip=_flags([0, 1, 0]))
    assert torch.equal(f1, f)
    f0, u0 = pre.resize_u8(torch.from_numpy(x).cuda(), 7, 13, want_u8=True)
    fz, uz = pre.resize_u8(torch.from_numpy(x).cuda(), 7, 13, want_u8=True, flip=_flags([0, 0, 0]))
    assert torch.equal(f0, fz) and torch.equal(u0, uz)
    with pytest.raises(ValueError):
        pre.resize_u8(torch.from_numpy(x).cuda(), 7, 13, flip=_flags([0, 1]))


def test_flipped_topview_matches_reference_processing():
    from jperceiver_amd.datasets import DevicePreprocessor
    g = np.load(os.path.join(GOLDEN, "preprocess.npz"))
    pre = DevicePreprocessor(128, 128, "cuda")
    for name in ("sq", "rect", "up"):
        h, w, S = (int(v) for v in g[f"topview/{name}/shape"])
        lab = ((syn.hash_uniform(22, ("tv", name), (h, w)) > 0.55) * 255).astype(np.uint8)
        for mode, arr in (("L", lab), ("RGB", np.stack([lab, lab, lab], -1))):
            batch = torch.from_numpy(np.stack([_mirror(arr), arr, _mirror(arr)])).cuda()
            out = pre.topview(batch, S, flip=_flags([1, 0, 1]))
            assert out.shape == (3, 1, S, S)
            for i in range(3):
                np.testing.assert_array_equal(out[i, 0].cpu().numpy().astype(np.uint8), g[f"topview/{name}/{mode}"],
                                              err_msg=f"{name} {mode} item {i}")
            assert torch.equal(pre.topview(batch, S, flip=_flags([0, 0, 0])), pre.topview(batch, S))
        batch = torch.from_numpy(np.stack([lab, _mirror(lab)])).cuda()
        out = pre.topview(batch, S, both=True, flip=_flags([0, 1]))
        for i in range(2):
            np.testing.assert_array_equal(out[i, 0].cpu().numpy().astype(np.uint8), g[f"topview_both/{name}"])


# ------------------------------------------------------------------------------------------- __call__
H, W, FR, N, FULL = 32, 48, [0, -1, 1], 4, (36, 54)


def _raw(seed=60, n=N):
    raw = {("color", f, -1): (torch.from_numpy(syn.hash_uniform(seed, ("rawf", f), (n, 40, 60, 3))) * 256).to(torch.uint8) for f in FR}
    raw[("bothS", 0, 0)] = torch.from_numpy(((syn.hash_uniform(seed, "bs", (n, 50, 70)) > 0.55) * 255).astype(np.uint8))
    raw[("bothD", 0, 0)] = torch.from_numpy(((syn.hash_uniform(seed, "bd", (n, 50, 70, 3)) > 0.5) * 255).astype(np.uint8))
    raw[("both_dynamic", 0, 0)] = torch.from_numpy((syn.hash_uniform(seed, "bb", (n, 33, 41)) * 3).astype(np.uint8) * 127 + 1)
    for j, k in enumerate(CALIB):
        raw[k] = torch.from_numpy(syn.hash_uniform(seed, ("cal", j), (n, 4, 4)).astype(np.float32))
    return raw


def _host_mirrored(raw, flips):
    out = {}
    for k, v in raw.items():
        if isinstance(k, tuple):                            # images and labels: (N, h, w[, C]), the width is axis 2
            v = v.clone()
            for i, fl in enumerate(flips):
                if fl:
                    v[i] = raw[k][i].flip(1)
        out[k] = v
    return out


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def test_call_with_flip_equals_the_host_mirror():
    from jperceiver_amd.datasets import DevicePreprocessor
    pre = DevicePreprocessor(H, W, "cuda")
    raw, flips = _raw(), [1, 0, 1, 0]
    dev = _cuda(raw)
    out = pre(dev, FR, FULL, do_color_aug=False, do_flip=flips)
    assert pre.last_flip == [True, False, True, False] and pre.last_jitter == {}
    ref = pre(_cuda(_host_mirrored(raw, flips)), FR, FULL, do_color_aug=False, do_flip=False)
    assert pre.last_flip == [False] * N
    assert set(out) == set(ref) and len(out) == 1 + 2 * len(FR) + 3 + len(CALIB)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
        assert not torch.isnan(out[k]).any(), k
    for k in CALIB:
        assert torch.equal(out[k].cpu(), raw[k]), k
    # the flip does something: a flagged item differs from the unflipped call, an unflagged one does not
    plain = pre(dev, FR, FULL, do_color_aug=False)
    for k in [("color", 0, -1), ("color", 1, 0), ("color_aug", -1, 0), ("bothS", 0, 0), ("bothD", 0, 0), ("both_dynamic", 0, 0)]:
        assert not torch.equal(out[k][0], plain[k][0]) and torch.equal(out[k][1], plain[k][1]), k
    with pytest.raises(ValueError):
        pre(dev, FR, FULL, do_color_aug=False, do_flip=[1, 0, 1])


@pytest.mark.parametrize("jitter", ["per_frame", "per_item"])
def test_call_with_flip_and_jitter_equals_the_host_mirror(jitter):
    from jperceiver_amd.datasets import DevicePreprocessor
    pre = DevicePreprocessor(H, W, "cuda")
    raw, flips, coins = _raw(), [1, 0, 1, 0], [1, 1, 0, 0]
    out = pre(_cuda(raw), FR, FULL, do_color_aug=coins, do_flip=flips, generator=torch.Generator().manual_seed(2), jitter=jitter)
    P = pre.last_jitter
    ref = pre(_cuda(_host_mirrored(raw, flips)), FR, FULL, do_color_aug=coins, do_flip=False,
              generator=torch.Generator().manual_seed(2), jitter=jitter)
    assert set(P) == set(pre.last_jitter) == {(i, f) for i in (0, 1) for f in FR}
    assert all(P[k].order == pre.last_jitter[k].order and P[k].factors == pre.last_jitter[k].factors for k in P)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    for f in FR:
        assert not torch.equal(out[("color_aug", f, 0)][0], out[("color", f, 0)][0])
        assert torch.equal(out[("color_aug", f, 0)][2:], out[("color", f, 0)][2:])


# ------------------------------------------------------------------------------------------- batched jitter
def _jitter_inputs(h, w):
    x = torch.rand(4, 3, h, w, generator=torch.Generator().manual_seed(7))
    x[0, :, :min(4, h - 1)] = 0.5              # grey pixels: hue undefined (maxc == minc branch)
    x[1, :, :2] = 0.0
    return x


def _params(order, factors):
    p = ColorJitterParams()
    p.order, p.factors = list(order), list(factors)
    return p


def _check_batched(pre, x, plist, tag):
    from oracle import tv_restated as TV
    got = pre.color_jitter_batched_(x.clone().cuda(), plist).cpu()
    for i, p in enumerate(plist):
        if p is None:
            assert torch.equal(got[i], x[i]), (tag, i)
            continue
        ref = TV.color_jitter(x[i:i + 1].clone(), p.order, p.factors)
        err = float((got[i:i + 1] - ref).abs().max())
        assert err < 2e-5, (tag, i, p.order, err)


@pytest.mark.parametrize("hw", [(32, 48), (5, 7), (31, 47)])
def test_batched_color_jitter_matches_torchvision_restatement(hw):
    """(32, 48): the inputs of the per-op test; (5, 7): fewer pixels than a workgroup has threads; (31, 47): not a multiple of it."""
    from jperceiver_amd.datasets import DevicePreprocessor
    pre = DevicePreprocessor(hw[0], hw[1], "cuda")
    x = _jitter_inputs(*hw)
    for seed in range(6):                      # three parameter sets and an untouched image in one launch
        ps = [ColorJitterParams(generator=torch.Generator().manual_seed(seed + 10 * j)) for j in range(3)]
        assert len({tuple(p.order) + tuple(p.factors) for p in ps}) == 3
        _check_batched(pre, x, ps + [None], ("seed", seed))
        _check_batched(pre, x, [None] + ps, ("seed, shifted", seed))
    strong = [1.7, 0.3, 1.9, -0.45]
    for shift in range(4):                     # each op alone, strong factors; every image meets every op
        _check_batched(pre, x, [_params([(i + shift) % 4], strong) for i in range(4)], ("alone", shift))
    for seed in range(3):                      # contrast first, in the middle (twice) and last
        f = ColorJitterParams(generator=torch.Generator().manual_seed(20 + seed)).factors
        orders = ([1, 0, 2, 3], [3, 1, 0, 2], [0, 2, 1, 3], [2, 3, 0, 1])
        _check_batched(pre, x, [_params(o, f) for o in orders], ("contrast position", seed))
    _check_batched(pre, x, [_params([0, 1], strong), _params([1], strong), None, _params([3, 2, 1], strong)], "short chains")
    with pytest.raises(ValueError):
        pre.color_jitter_batched_(x.clone().cuda(), [None] * 3)


def test_batched_color_jitter_is_bit_reproducible():
    from jperceiver_amd.datasets import DevicePreprocessor
    pre = DevicePreprocessor(64, 96, "cuda")
    x = torch.rand(3, 3, 64, 96, generator=torch.Generator().manual_seed(8))
    ps = [ColorJitterParams(generator=torch.Generator().manual_seed(s)) for s in range(3)]
    ps[1].order = [0, 2, 3, 1]                 # contrast last: its mean depends on the whole chain
    a = pre.color_jitter_batched_(x.clone().cuda(), ps)
    b = pre.color_jitter_batched_(x.clone().cuda(), ps)
    assert torch.equal(a, b) and not torch.isnan(a).any() and not torch.equal(a.cpu(), x)


def test_call_batched_equals_per_op_path():
    from jperceiver_amd.datasets import DevicePreprocessor
    pre = DevicePreprocessor(H, W, "cuda")
    raw, flips, coins = _raw(61), [0, 1, 1, 0], [1, 0, 1, 0]
    kw = dict(do_color_aug=coins, do_flip=flips)
    for jitter in ("per_frame", "per_item"):
        a = pre(_cuda(raw), FR, FULL, generator=torch.Generator().manual_seed(4), jitter=jitter, batched=False, **kw)
        Pa = pre.last_jitter
        b = pre(_cuda(raw), FR, FULL, generator=torch.Generator().manual_seed(4), jitter=jitter, batched=True, **kw)
        assert all(Pa[k].order == pre.last_jitter[k].order and Pa[k].factors == pre.last_jitter[k].factors for k in Pa)
        assert set(a) == set(b)
        for k in a:
            if k[0] != "color_aug":
                assert torch.equal(a[k], b[k]), k
                continue
            err = float((a[k] - b[k]).abs().max())
            assert err <= 1e-6, (k, err)
            assert torch.equal(a[k][1], b[k][1]) and torch.equal(a[k][3], b[k][3]), k          # not augmented: bit-equal
            assert torch.equal(b[k][1], b[("color", k[1], 0)][1])
            assert float((b[k][0] - b[("color", k[1], 0)][0]).abs().max()) > 1e-3


def test_device_loader_runs_the_batched_flipped_pipeline():
    from jperceiver_amd.datasets import DeviceLoader, DevicePreprocessor
    pre, pre2 = DevicePreprocessor(H, W, "cuda"), DevicePreprocessor(H, W, "cuda")
    raws = [_raw(70 + i, n=3) for i in range(4)]
    g = torch.Generator().manual_seed(12)
    loader = DeviceLoader(iter(raws), "cuda", depth=2,
                          preprocess=lambda raw: pre(raw, FR, FULL, do_flip=None, do_color_aug=None, generator=g, batched=True))
    g2 = torch.Generator().manual_seed(12)
    n, seen_flip, seen_aug = 0, set(), set()
    for batch, raw in zip(loader, raws):
        ref = pre2(_cuda(raw), FR, FULL, do_flip=None, do_color_aug=None, generator=g2, batched=True)
        seen_flip |= set(pre2.last_flip)
        seen_aug |= {bool(pre2.last_jitter)}
        assert set(batch) == set(ref)
        for k in ref:
            assert torch.equal(batch[k], ref[k]), (n, k)
        n += 1
    assert n == 4 and seen_flip == {True, False} and True in seen_aug
