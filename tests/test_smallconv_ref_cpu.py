"""What tests/test_smallconv_f64_gpu.py rests on, checked without a GPU: the float64 reference (tests/smallconv_ref.py) against an
independent gather-by-index evaluation, forward and backward; every path claim of the case tables, through the launch mirrors of
tests/smallconv_cases.py; the term sums; the share of ambiguous ReLU gates; and the bars against the recomputed fp32 yardsticks."""
import functools

import pytest
import torch

from tests import smallconv_cases as C
from tests import smallconv_ref as R
from tests.smallconv_cases import CASES


# --------------------------------------------------------------------------------------------------- reference vs gather evaluation
@pytest.mark.parametrize("name", C.GATHER_CASES)
def test_reference_agrees_with_gather_evaluation(name):
    """forward and the three gradients (the backward of an index gather is the transposed gather); 1e-13 of the term sums: both are
    float64 sums of the same products in another order"""
    case, inp = CASES[name], C.inputs(name)
    fwd = C.reference(name)
    g = inp.dy.double()
    ref = R.backward(inp, case, g)
    evaluations = [lambda xs, w: R.gather_forward(xs, w, case)]
    if C.up_head(case):
        evaluations.append(lambda xs, w: R.up_head_gather_forward(xs[0], w, case))
    for ev in evaluations:
        xs = [x.double().requires_grad_(True) for x in inp.xs]
        w = inp.w.double().requires_grad_(True)
        pre = ev(xs, w)
        pre.backward(g)
        b = inp.b.double().view(1, -1, 1, 1) if inp.b is not None else 0.0
        assert R.worst(pre.detach() + b, fwd.pre, fwd.S) < 1e-13
        for x, dx, S in zip(xs, ref.dxs, ref.S_dxs):
            assert R.worst(x.grad, dx, S) < 1e-13
        assert R.worst(w.grad, ref.dw, ref.S_dw) < 1e-13


def test_chain_is_exact_on_exact_data():
    """the fp32 chain (forward, input, weight and bias gradients) on small integers, where every fp32 sum is exact, equals the float64
    reference: the chain's index bookkeeping (readers of an upsampled, reflected element) is right"""
    for name in ("U2", "S4r", "S4z", "S5"):
        case, inp = CASES[name], C.inputs(name)
        q = R.Inputs([(x.clamp(-2, 2) * 4).round() for x in inp.xs], (inp.w * 8).clamp(-3, 3).round(),
                     None if inp.b is None else inp.b.round(), (inp.dy * 2).round())
        lin = case._replace(act=R.ACT_NONE)
        got, fwd = R.chain32(q, lin), R.forward(q, lin)
        ref = R.backward(q, lin, q.dy.double())
        assert torch.equal(got["y"].double(), fwd.pre)
        for d, r in zip(got["dxs"], ref.dxs):
            assert torch.equal(d.double(), r)
        assert torch.equal(got["dw"].double(), ref.dw)
        if q.b is not None:
            assert torch.equal(got["db"].double(), ref.db)


# --------------------------------------------------------------------------------------------------- path claims
def _u(name):
    c = CASES[name]
    return c.N, c.srcs[0][0], c.H // 2, c.W // 2


def test_routes():
    for name, case in CASES.items():
        want = {"U": "up_head", "S": "small", "C": "c16"}[name[0]]
        if name in ("U8a", "U8b"):           # rejected by up_head() (769 > 768, 7 < 8): conv_small with an upsampled segment
            assert not C.up_head(case) and C.small_head(case) and case.srcs[0][1] == 1
            want = "small"
        assert C.route(case) == want, name
    assert not C.small_head(CASES["C1"]) and not C.c16_ok(CASES["S1"])


def test_disparity_head_paths():
    f = {n: C.up_fwd(*_u(n)) for n in ("U1", "U2", "U3", "U4", "U5", "U6", "U7")}
    # U1: smallest legal head, scalar forward, every pixel on all four clamp lines (h = wd = 2: i - 1 and i + 1 both clamp)
    assert f["U1"]["kernel"] == "up_head_fwd_kernel" and _u("U1")[2:] == (2, 2) and CASES["U1"].H == 4
    # U2: scalar forward (wd % 4 != 0), dgrad tail of 1 channel, weight-gradient block tail of 5
    assert f["U2"]["kernel"] == "up_head_fwd_kernel" and _u("U2")[3] % 4 != 0
    assert _u("U2")[1] % 4 == 1 and C.up_wgrad(*_u("U2"))["block_tail"] == 5
    # U3: fwd2s<4>, cq = 3, last group 1 channel; 90 pairs = 2 workgroups, 26 live lanes in the second; dgrad tail of 2
    assert f["U3"]["kernel"] == "up_head_fwd2s_kernel<4>" and f["U3"]["groups"] == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert (f["U3"]["wgs"], f["U3"]["last"]) == (2, 26) and _u("U3")[1] % 4 == 2
    # U4: fwd2s<4> with an empty fourth group; wd = 4: both pairs of a row touch a clamped column
    assert f["U4"]["kernel"] == "up_head_fwd2s_kernel<4>" and f["U4"]["groups"][3] == (9, 9) and _u("U4")[3] == 4
    # U5: the one-chain two-pixel kernel (16512 pairs > 16384), ragged last workgroup; 8 bands, the last one ragged
    assert f["U5"]["kernel"] == "up_head_fwd2_kernel" and _u("U5")[2] * _u("U5")[3] // 2 == 16512 and 0 < f["U5"]["last"] < 256
    w5 = C.up_wgrad(*_u("U5"))
    assert w5["nb"] == 8 and 0 < w5["last_band"] < w5["band"]
    # U6: fwd2s<4>; 2 bands x 2 images folded
    w6 = C.up_wgrad(*_u("U6"))
    assert f["U6"]["kernel"] == "up_head_fwd2s_kernel<4>" and w6["nb"] == 2 and w6["folded"] == 4
    # U7: the top of the ABI's range: 48 KiB of slot weights
    assert f["U7"]["lds"] == 48 * 1024 and C.up_head(CASES["U7"])
    # the three tiers are told apart by the scratch size alone
    for n in ("U2", "U6"):
        w = C.up_wgrad(*_u(n))
        assert 0 < w["d_floats"] < w["ws_floats"]


def test_small_conv_paths():
    s = {n: C.small_wgrad(CASES[n]) for n in CASES if C.route(CASES[n]) == "small"}
    # S1: tiled, two 64-row bands (the second 3 rows), ragged 16-row and 64-column tiles
    assert s["S1"]["tiled"] and s["S1"]["grid"] == (2, 6, 2) and CASES["S1"].H - 64 == 3 and CASES["S1"].H % 16 and CASES["S1"].W % 64
    # S2: 49104 of 49152 bytes of LDS weights
    assert s["S2"]["lds"] == 49104 and C.small_head(CASES["S2"])
    assert not C.small_head(CASES["S2"]._replace(srcs=((342, 0),)))
    # S3: H = 1 -> the chunked kernel on a single source
    assert not s["S3"]["tiled"] and s["S3"]["grid"] == (1, 3, 2)
    # S4: chunked, 2 pixel chunks, three segments with a half-resolution one in the middle
    for n in ("S4r", "S4z"):
        assert not s[n]["tiled"] and s[n]["grid"] == (2, 8, 1) and s[n]["chunk"] == 4608
        assert [u for _, u in CASES[n].srcs] == [0, 1, 0]
    # S5, U8: an upsampled source that is not an up-head -> chunked
    for n in ("S5", "U8a", "U8b"):
        assert not s[n]["tiled"] and CASES[n].srcs[0][1] == 1
    assert CASES["S5"].Cout == 3


def test_c16_paths():
    w = {n: C.c16_wgrad(CASES[n]) for n in ("C1", "C2", "C3")}
    assert w["C1"]["ntiles"] == 16 and not C.c16_ok(CASES["C1"]._replace(H=32))            # smallest legal shape
    # C2: 576 tiles on 512 workgroups: 64 take a second tile; a workgroup's two tiles lie in different images
    assert (w["C2"]["ntiles"], w["C2"]["grid"], w["C2"]["second_tile"]) == (576, 512, 64)
    assert all(T // w["C2"]["tiles_per_image"] != (T + 512) // w["C2"]["tiles_per_image"] for T in range(64))
    # C2's source is stored at half resolution: UPIN forward and weight gradient.  (Its input gradient is the full-resolution c16
    # dgrad followed by jp_upsample2x_bwd: jp_conv2d_dgrad passes up = 0, the only caller of jp_c16_dgrad, so the SUMOUT
    # instantiation of c16_conv_kernel is not reachable through the ABI.)
    assert CASES["C2"].srcs[0][1] == 1
    assert w["C3"]["ntiles"] == 144 and w["C3"]["second_tile"] == 0 and CASES["C3"].N == 3


def test_mirrored_expressions_stand_in_the_sources():
    """the launch expressions the mirrors restate, found in the kernel sources: a changed threshold fails here, not silently"""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jperceiver_amd", "csrc")
    wanted = {
        "conv_common.h": ["c0 >= 8 && c0 <= 768", "H % 2 == 0 && W % 2 == 0 && H >= 4 && W >= 4", "(long)Cout * Cin * 9 * 4 <= 48 * 1024"],
        "conv_small.hip": ["constexpr int TPB = 256;", "if (wd % 4 == 0) {", "(long)N * h * (wd / 2) <= 8L * 2048", "jp_cdiv(h * (wd / 2), 64)",
                           "std::max(1, std::min(hw / (TPB * 16), 16))", "jp_cdiv(jp_cdiv(hw, bands), TPB) * TPB",
                           "return 16L * N * hw + 16L * C * jp_cdiv(hw, band) * N;", "ws_floats >= 16L * N * hw",
                           "constexpr int UP_CB = 8;", "constexpr int UPD_CB = 8;", "const int cq = (C + groups - 1) / groups",
                           "for (; c + 4 <= C; c += 4) {", "src.nseg == 1 && src.s[0].sh == 0 && H >= 2 && W >= 2",
                           "*grid = dim3(jp_cdiv(H, 64), Cin, N)", "std::max(1, 2048 / std::max(1, Cin * N))", "std::max(1, H * W / 4096)",
                           "jp_cdiv(jp_cdiv(H * W, chunks), TPB) * TPB"],
        "conv_c16.hip": ["constexpr int WG_R = 4, WG_C = 64;", "Cin == 16 && Cout == 16 && KH == 3 && stride == 1 && pad == 1 && pad_mode == 0",
                         "H % 32 == 0 && W % 64 == 0 && H >= 64", "const int ntiles = N * (H / WG_R) * (W / WG_C);",
                         "const dim3 grid(std::min(ntiles, 512));", "std::min(N * (H / WG_R) * (W / WG_C), 512) * Cout * Cin * 9"],
    }
    for fname, lines in wanted.items():
        with open(os.path.join(csrc, fname)) as f:
            text = f.read()
        for line in lines:
            assert line in text, f"{fname} no longer holds `{line}`: tests/smallconv_cases.py mirrors it"


# --------------------------------------------------------------------------------------------------- term sums, gates, bars
@functools.lru_cache(maxsize=None)
def _yardsticks(name):
    case, inp = CASES[name], C.inputs(name)
    out = []
    for fn in (R.aten32, R.chain32):
        figs, up = C.evaluate(name, fn(inp, case))
        assert up.wrong == 0, f"{name}: a yardstick's unambiguous ReLU gate differs from the reference's"
        out.append(figs)
    return out


def test_term_sums_are_positive():
    """S == 0 only where a sum has no term: the weight-gradient taps of the one-row map S3 that read nothing but padding"""
    for name, case in CASES.items():
        inp, fwd = C.inputs(name), C.reference(name)
        bwd = R.backward(inp, case, R.upstream(inp, case, fwd, R.activation(fwd.pre, case.act), 0.0).g)
        assert bool((fwd.S > 0).all()), name
        assert all(bool((s > 0).all()) for s in bwd.S_dxs), name
        assert bool((bwd.S_db > 0).all()), name
        if name == "S3":
            assert bool((bwd.S_dw[:, :, 1] > 0).all()) and bool((bwd.S_dw[:, :, 0::2] == 0).all()) and bool((bwd.dw[:, :, 0::2] == 0).all())
        else:
            assert bool((bwd.S_dw > 0).all()), name


def test_ambiguous_gate_share():
    for name in ("C2", "C3"):
        case, fwd = CASES[name], C.reference(name)
        share = float(R.ambiguous(fwd, case, C.BARS[(case.family, "fwd")]).double().mean())
        print(f"  {name}: ambiguous gates {share:.2e} of the elements (cap {C.AMBIGUOUS_CAP})")
        assert share <= C.AMBIGUOUS_CAP
    assert not bool(R.ambiguous(C.reference("C1"), CASES["C1"], 1.0).any())           # no activation, no gate


def test_bars_match_recomputed_yardsticks():
    """the committed yardstick figures have not drifted by more than 2x, and every bar is 8 x the larger one, rounded up to one digit"""
    worst = {}
    for name, case in CASES.items():
        aten, chain = _yardsticks(name)
        for q in aten:
            a, c = worst.get((case.family, q), (0.0, 0.0))
            worst[(case.family, q)] = (max(a, aten[q]), max(c, chain[q]))
    assert set(worst) == set(C.YARDSTICKS) == set(C.BARS)
    for key, (a, c) in sorted(worst.items()):
        ca, cc = C.YARDSTICKS[key]
        print(f"  {key[0]:6s}{key[1]:4s} aten32 {a:.3e} (committed {ca:.3e})   chain32 {c:.3e} (committed {cc:.3e})   bar {C.BARS[key]:.0e}")
        assert ca / 2 <= a <= ca * 2 and cc / 2 <= c <= cc * 2, key
        assert C.BARS[key] == C.bar_of(ca, cc)
        assert C.MARGIN * max(ca, cc) <= C.BARS[key] < 10 * C.MARGIN * max(ca, cc)
