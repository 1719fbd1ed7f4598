"""The two kernels of frozen inference (csrc/frozen.hip) through the C ABI.

* jp_bn_fold_conv: folded weights and bias BIT-EQUAL to the formula evaluated operation by operation in numpy float64 and rounded
  to float32 once -- s = gamma / sqrt(var + eps), w' = w * s, b' = beta + (b - mean) * s -- for an odd row length that is no
  multiple of any vector width (Cout 5, K 147) and a block-sized one (Cout 64, K 576), running_var in [0.25, 4], non-zero means,
  a negative, a tiny (1e-3) and an exactly zero gamma (nothing is clamped), with and without a convolution bias.  The outputs
  are poisoned with NaN before the call.
* jp_add_relu: bit-equal to torch.relu(a + b) / a + b on the CPU for n in {1, 3, 4, 1027, 64*16*16*2}, `out` separate and `out`
  aliasing `a`, NaN-poisoned separate outputs, and the magnitude slot holds max|out| exactly; plus operands that do not sit on
  a 16-byte boundary (the all-scalar path)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd._lib import call, lib                     # noqa: E402

DEV = "cuda"
EPS = 1e-5


def _slot_value(slot):
    """the magnitude a slot holds: the largest of its ways (bit patterns of non-negative floats order like the floats)"""
    return float(slot.cpu().view(torch.int32).max().reshape(1).view(torch.float32))


def _fold_case(Cout, K, bias, seed):
    g = np.random.default_rng(seed)
    w = g.standard_normal((Cout, K)).astype(np.float32)
    gamma = (1.0 + 0.5 * g.standard_normal(Cout)).astype(np.float32)
    gamma[0], gamma[1], gamma[2] = -0.75, 1e-3, 0.0
    beta = g.standard_normal(Cout).astype(np.float32)
    mean = (g.uniform(0.2, 1.0, Cout) * g.choice([-1.0, 1.0], Cout)).astype(np.float32)          # non-zero
    var = g.uniform(0.25, 4.0, Cout).astype(np.float32)
    cb = g.standard_normal(Cout).astype(np.float32) if bias else None
    return w, cb, gamma, beta, mean, var


def _fold_ref(w, cb, gamma, beta, mean, var, eps):
    f8 = np.float64
    s = gamma.astype(f8) / np.sqrt(var.astype(f8) + f8(np.float32(eps)))            # the ABI carries eps as a float
    b = cb.astype(f8) if cb is not None else np.zeros_like(s)
    return (w.astype(f8) * s[:, None]).astype(np.float32), (beta.astype(f8) + (b - mean.astype(f8)) * s).astype(np.float32)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("Cout,K", [(5, 3 * 7 * 7), (64, 64 * 3 * 3)])
def test_bn_fold_conv_is_the_float64_formula_rounded_once(Cout, K, bias):
    w, cb, gamma, beta, mean, var = _fold_case(Cout, K, bias, seed=Cout + K + int(bias))
    rw, rb = _fold_ref(w, cb, gamma, beta, mean, var, EPS)
    d = lambda a: None if a is None else torch.from_numpy(a).to(DEV)                  # noqa: E731
    w_out = torch.full((Cout, K), float("nan"), device=DEV)
    b_out = torch.full((Cout,), float("nan"), device=DEV)
    call("jp_bn_fold_conv", d(w), d(cb), d(gamma), d(beta), d(mean), d(var), EPS, w_out, b_out, Cout, K)
    gw, gb = w_out.cpu().numpy(), b_out.cpu().numpy()
    nw = int((gw.view(np.uint32) != rw.view(np.uint32)).sum())
    nb = int((gb.view(np.uint32) != rb.view(np.uint32)).sum())
    print(f"bn_fold_conv Cout={Cout} K={K} bias={bias}: {nw} weights / {nb} biases differ in bits from the float64 formula")
    assert nw == 0 and nb == 0
    # the three special channels came out as the formula says, unclamped
    assert (np.sign(gw[0]) == -np.sign(w[0])).all()
    assert np.abs(gw[1]).max() <= 1e-3 * np.abs(w[1]).max() / np.sqrt(0.25) * 1.0001 and np.abs(gw[1]).max() > 0
    assert not gw[2].any() and gb[2] == beta[2]


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 64 * 16 * 16 * 2])
def test_add_relu_is_bit_equal_and_reports_its_magnitude(n, relu, alias):
    g = torch.Generator().manual_seed(n + 7 * relu)
    a_h, b_h = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n >= 4:
        b_h[1] = -a_h[1]                                             # an exact zero sum
    ref = torch.relu(a_h + b_h) if relu else a_h + b_h
    a, b = a_h.to(DEV), b_h.to(DEV)
    out = a if alias else torch.full((n,), float("nan"), device=DEV)
    slot = torch.zeros(int(lib().fn["jp_amax_slot_floats"]()), device=DEV)
    call("jp_add_relu", a, b, out, n, relu, slot)
    got = out.cpu()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (n, relu, alias)
    if not alias:
        assert torch.equal(a.cpu(), a_h)                             # the inputs are read only
    assert torch.equal(b.cpu(), b_h)
    amax = _slot_value(slot)
    assert amax == float(ref.abs().max()), (amax, float(ref.abs().max()))
    # amax_out == NULL: the same output
    out2 = torch.full((n,), float("nan"), device=DEV)
    call("jp_add_relu", a_h.to(DEV), b, out2, n, relu, None)
    assert torch.equal(out2.cpu().view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize("off", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)])
def test_add_relu_on_operands_off_the_16_byte_boundary(off):
    n = 1027
    g = torch.Generator().manual_seed(sum(off))
    a_h, b_h = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ref = torch.relu(a_h + b_h)
    bufs = [torch.full((n + 8,), float("nan"), device=DEV) for _ in range(3)]
    a, b, out = (buf[o:o + n] for buf, o in zip(bufs, off))
    a.copy_(a_h)
    b.copy_(b_h)
    slot = torch.zeros(int(lib().fn["jp_amax_slot_floats"]()), device=DEV)
    call("jp_add_relu", a, b, out, n, 1, slot)
    assert torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32))
    o = off[2]
    assert torch.isnan(bufs[2][:o]).all() and torch.isnan(bufs[2][o + n:]).all()     # nothing written outside [0, n)
    assert _slot_value(slot) == float(ref.max())


def test_add_relu_treats_nan_and_negative_zero_as_the_eval_batchnorm_does():
    """The stated choice (include/jperceiver_hip.h): with relu the pass answers like jp_bn_eval_fwd's fmaxf(r, 0) -- a NaN sum
    becomes 0 (torch.relu would keep it), -0.0 becomes +0.0; without relu the sum is stored as it is.  max |out| skips a NaN."""
    nan, n = float("nan"), 9                                            # two 16-byte groups and a scalar tail
    a_h = torch.tensor([nan, -0.0, 1.0, -2.0, 0.5, nan, 3.0, -0.0, nan])
    b_h = torch.tensor([1.0, -0.0, nan, 0.5, 0.25, nan, -1.0, 0.0, -0.0])
    s = a_h + b_h
    for relu, ref in ((1, torch.where(s > 0, s, torch.zeros(n))), (0, s)):
        out = torch.full((n,), 7.0, device=DEV)
        slot = torch.zeros(int(lib().fn["jp_amax_slot_floats"]()), device=DEV)
        call("jp_add_relu", a_h.to(DEV), b_h.to(DEV), out, n, relu, slot)
        got = out.cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (relu, got)
        keep = ~torch.isnan(ref)
        assert torch.equal(got[keep].view(torch.int32), ref[keep].view(torch.int32)), (relu, got)       # bit pattern: the sign of zero too
        assert _slot_value(slot) == float(ref[keep].abs().max())
