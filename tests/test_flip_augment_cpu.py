"""Horizontal flip + batched ColorJitter of the device-side input pipeline, the parts that need no GPU: the new entry points
exist and validate their arguments before touching a device, the pure draw helper consumes the generator in the documented
order (colour coins, flip coins, jitter parameters), the parameter table has the layout the kernel reads, and Pillow itself
agrees that resizing a mirrored image is the two-pass resampler run on the mirrored array (the double-mirror argument the GPU
tests use against tests/golden/preprocess.npz)."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib
from jperceiver_amd import synthetic as syn
from jperceiver_amd.datasets import ColorJitterParams
from tests.test_input_pipeline import _two_pass

NEW = ("jp_resample_h_u8_flip", "jp_u8_to_tensor_flip", "jp_topview_u8_flip", "jp_color_jitter_batched",
       "jp_color_jitter_batched_ws_doubles")
P = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced: the argument check comes first


def test_new_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (jp_\w+)", out))
    for name in NEW:
        assert name in protos, name
        assert name in exported, name
    args = lambda n: [a for _, a in protos[n][1]]
    assert args("jp_resample_h_u8_flip") == ["src", "dst", "bounds", "kk", "flip", "N", "H", "W", "OW", "C", "ksize", "stream"]
    assert args("jp_u8_to_tensor_flip") == ["src", "dst_f", "dst_u8", "flip", "N", "H", "W", "C", "stream"]
    assert args("jp_topview_u8_flip") == ["src", "dst", "flip", "N", "h", "w", "C", "S", "exact255", "stream"]
    assert args("jp_color_jitter_batched") == ["x", "params", "ws", "N", "HW", "stream"]
    assert protos["jp_color_jitter_batched_ws_doubles"][0] == "long"


def _rejected(L, name, *a):
    rc = L.fn[name](*a)
    return rc != 0 and name[3:] in L.last_error()


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    L = _lib.lib()
    good = [P, P, P, P, None, 2, 4, 6, 5, 3, 7, None]                  # flip (index 4) and stream may be null
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (5, 0), (6, 0), (7, -1), (8, 0), (9, 0), (10, 0)):
        a = list(good)
        a[i] = bad
        assert _rejected(L, "jp_resample_h_u8_flip", *a), i
    good = [P, P, P, None, 2, 4, 6, 3, None]
    for i, bad in ((0, None), (4, 0), (5, -3), (6, 0), (7, 0)):
        a = list(good)
        a[i] = bad
        assert _rejected(L, "jp_u8_to_tensor_flip", *a), i
    assert _rejected(L, "jp_u8_to_tensor_flip", P, None, None, None, 2, 4, 6, 3, None)          # both outputs null
    assert _rejected(L, "jp_u8_to_tensor_flip", P, None, P, None, 2, 4, 6, 3, None)             # a mirror in place
    good = [P, P, None, 2, 4, 6, 3, 5, 0, None]
    for i, bad in ((0, None), (1, None), (3, 0), (4, 0), (5, 0), (6, 2), (7, 0)):
        a = list(good)
        a[i] = bad
        assert _rejected(L, "jp_topview_u8_flip", *a), i
    good = [P, P, P, 2, 35, None]
    for i, bad in ((0, None), (1, None), (2, None), (3, 0), (3, -1), (4, 0)):
        a = list(good)
        a[i] = bad
        assert _rejected(L, "jp_color_jitter_batched", *a), i
    ws = L.fn["jp_color_jitter_batched_ws_doubles"]
    assert ws(0, 35) < 0 and ws(3, 0) < 0 and "color_jitter_batched_ws_doubles" in L.last_error()
    for HW in (1, 35, 256, 257, 1457, 1024 * 1024):
        sizes = [ws(n, HW) for n in range(1, 10)]
        assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])), HW
        assert sizes[3] == 4 * sizes[0]


def _same(a: ColorJitterParams, b: ColorJitterParams):
    return a.order == b.order and a.factors == b.factors


@pytest.mark.parametrize("jitter", ["per_frame", "per_item"])
def test_draws_without_flip_are_the_old_draws(jitter):
    from jperceiver_amd.datasets import draw_augmentation
    N, FR = 6, [0, -1, 1]
    g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    coins, flips, params = draw_augmentation(N, FR, None, False, g1, jitter)
    # the documented old order: N coins, then per item (and per frame) one ColorJitterParams
    ref_coins = (torch.rand(N, generator=g2) > 0.5).tolist()
    ref = {}
    for i, c in enumerate(ref_coins):
        if not c:
            continue
        shared = ColorJitterParams(generator=g2) if jitter == "per_item" else None
        for f in FR:
            ref[(i, f)] = shared if shared is not None else ColorJitterParams(generator=g2)
    assert coins == ref_coins and 0 < sum(coins) < N
    assert flips == [False] * N
    assert set(params) == set(ref) and all(_same(params[k], ref[k]) for k in ref)
    if jitter == "per_item":
        assert all(params[(i, f)] is params[(i, FR[0])] for (i, f) in params)
    assert torch.equal(g1.get_state(), g2.get_state())
    with pytest.raises(ValueError):
        draw_augmentation(N, FR, None, False, g1, "per_batch")


def test_flip_coins_follow_the_colour_coins():
    from jperceiver_amd.datasets import draw_augmentation
    N, FR = 7, [0, -1, 1]
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    coins, flips, params = draw_augmentation(N, FR, None, None, g1, "per_frame")
    assert coins == (torch.rand(N, generator=g2) > 0.5).tolist()
    assert flips == (torch.rand(N, generator=g2) > 0.5).tolist() and 0 < sum(flips) < N
    for i in range(N):
        for f in FR:
            if coins[i]:
                assert _same(params[(i, f)], ColorJitterParams(generator=g2))
    assert len(params) == 3 * sum(coins)
    assert torch.equal(g1.get_state(), g2.get_state())


def test_explicit_sequences_draw_nothing_for_their_coin():
    from jperceiver_amd.datasets import draw_augmentation
    N, FR = 4, [0, 1]
    g = torch.Generator().manual_seed(9)
    before = g.get_state().clone()
    coins, flips, params = draw_augmentation(N, FR, [0, 0, 0, 0], [1, 0, 1, 0], g, "per_frame")
    assert coins == [False] * 4 and flips == [True, False, True, False] and params == {}
    assert torch.equal(g.get_state(), before)
    assert draw_augmentation(N, FR, False, True, g, "per_frame")[:2] == ([False] * 4, [True] * 4)
    assert torch.equal(g.get_state(), before)
    # an explicit colour sequence: only the flip coins, then the parameters
    g2 = torch.Generator().manual_seed(9)
    coins, flips, params = draw_augmentation(N, FR, [1, 0, 0, 0], None, g, "per_item")
    assert flips == (torch.rand(N, generator=g2) > 0.5).tolist()
    assert _same(params[(0, 0)], ColorJitterParams(generator=g2)) and params[(0, 1)] is params[(0, 0)]
    assert torch.equal(g.get_state(), g2.get_state())
    with pytest.raises(ValueError):
        draw_augmentation(N, FR, False, [1, 0, 1], g, "per_frame")
    with pytest.raises(ValueError):
        draw_augmentation(N, FR, [1, 0, 1, 0, 1], False, g, "per_frame")


def test_parameter_table_layout():
    from jperceiver_amd.datasets import color_jitter_table
    p = ColorJitterParams(generator=torch.Generator().manual_seed(1))
    q = ColorJitterParams()
    q.order, q.factors = [3, 1], [1.7, 0.3, 1.9, -0.45]
    tab = color_jitter_table([p, None, q])
    assert tab.shape == (3, 9) and tab.dtype == np.int32
    assert tab[0, 0] == 4 and tab[0, 1:5].tolist() == p.order
    assert tab[0, 5:].view(np.float32).tolist() == [np.float32(p.factors[op]) for op in p.order]
    assert not tab[1].any()
    assert tab[2, :5].tolist() == [2, 3, 1, 0, 0]
    assert tab[2, 5:7].view(np.float32).tolist() == [np.float32(-0.45), np.float32(0.3)]
    q.order = [1, 0, 1]
    with pytest.raises(ValueError):
        color_jitter_table([q])


def test_pillow_resizes_a_mirrored_image_like_the_two_pass_on_the_mirrored_array():
    try:
        from PIL import Image
    except ImportError:
        return
    flip_lr = getattr(Image, "Transpose", Image).FLIP_LEFT_RIGHT
    img = (syn.hash_uniform(3, "live", (41, 77, 3)) * 256).astype(np.uint8)
    pil = np.asarray(Image.fromarray(img).transpose(flip_lr).resize((32, 64), Image.LANCZOS))
    np.testing.assert_array_equal(_two_pass(np.ascontiguousarray(img[:, ::-1]), 64, 32), pil)
