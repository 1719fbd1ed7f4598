"""CPU checks behind tests/test_dense_f64_gpu.py (no GPU):

1. tests/dense_ref.py agrees at 1e-12 with torch's float64 evaluation of the same operation (matmul / baddbmm, sum, max, gather,
   scatter_add, mean, softmax, rot90, autograd through the two chains) and with the oracle's _max_dim1, cvp and CCT algebra; the
   column max keeps the first-maximum rule on planted ties and hands a NaN through with the row of the first NaN;
2. every case built for a launch path lies on it, by the Python mirror of the launch expressions of small.hip / pointwise.hip, and
   the mirrored source lines stand verbatim in the two files;
3. every input condition: the share of gates / columns that may take the device's decision is within MASK_CAP for every committed
   seed, by the reference alone (recorded below); the softmax cases are finite and hold every listed difference; the NaN, Inf, tie and
   constant-column cases are what they claim; the adjoint totals are no multiples of 256 where the issue asks for that;
4. the arithmetic of every derived bound, in float64 from the mirror;
5. the bars of the GPU file follow from the fp32 evaluation's own error against the float64 reference (dense_cases.BARS).
"""
import os
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import jp_oracle as J
from tests import dense_cases as C
from tests import dense_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _r(name, *shape):
    return C.randn("cpu " + name, *shape).double()


def _close(a, b, tol=1e-12):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------- 1. restatement == torch in float64
@pytest.mark.parametrize("name", [n for n in C.GEMM_CASES if not n.startswith("step")])
def test_gemm_matches_baddbmm_f64(name):
    g = C.gemm_case(name)
    c = g.case
    a, b = R.gemm_operands(g.A.double(), g.B.double(), *g.abi[:5], *g.abi[6:8], *g.abi[9:12])
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())            # no padding was read
    old = g.C.double()[g.ic]
    want = c["alpha"] * torch.bmm(a, b) + (c["beta"] * old if c["beta"] != 0 else 0)
    _close(g.ref[g.ic], want)
    assert bool(torch.isfinite(g.ref[g.ic]).all()), "beta = 0 must not hand the NaN of C through"
    _close(g.mag, abs(c["alpha"]) * torch.bmm(a.abs(), b.abs()) + ((c["beta"] * old).abs() if c["beta"] != 0 else 0))
    assert torch.equal(g.ref[g.padmask], g.C.double()[g.padmask])                     # padding untouched
    # the layouts are what ops.linear_act / ops_loss.bmm_tn pass: plain row-major tensors
    M, N, K, batch = c["M"], c["N"], c["K"], c["batch"]
    if c["pad"] == (0, 0, 0) and not c["shareA"]:
        A = g.A.double().view(batch, *((K, M) if c["tA"] else (M, K)))
        B = g.B.double().view(batch, *((N, K) if c["tB"] else (K, N)))
        _close(a, A.transpose(1, 2) if c["tA"] else A, 0)
        _close(b, B.transpose(1, 2) if c["tB"] else B, 0)


def test_rows_match_torch_f64():
    y, b = _r("y", 33, 17), _r("b", 17)
    for kind, fn in ((0, lambda t: t), (1, F.relu), (2, lambda t: F.leaky_relu(t, 0.01)), (3, torch.sigmoid)):
        _close(R.bias_act_rows(y, b, kind)[0], fn(y + b))
    _close(R.bias_act_rows(y, None, 1)[0], F.relu(y))
    _close(R.colsum(y)[0], y.sum(0))
    _close(R.colsum(y, b)[0], y.sum(0) + b)
    _close(R.colsum(y)[1], y.abs().sum(0))
    x, w = _r("x", 2, 5, 17), _r("w", 7, 17)
    _close(R.linear(x, w, b[:7]), F.linear(x, w, b[:7]))


def test_colmax_matches_torch_and_the_oracle():
    for shape in C.COLMAX_SHAPES:
        for kind in C.COLMAX_DATA:
            E = C.colmax_input(shape, kind).double()
            val, idx = R.colmax(E)
            tv, ti = J._max_dim1(E)
            assert torch.equal(torch.isnan(val), torch.isnan(tv))
            assert torch.equal(torch.nan_to_num(val, nan=0.0), torch.nan_to_num(tv, nan=0.0)), (shape, kind)
            first = (E == val.unsqueeze(1)) | (torch.isnan(E) & torch.isnan(val).unsqueeze(1))
            assert torch.equal(idx, first.double().argmax(1)), "not the FIRST maximal row"      # argmax of a 0/1 mask: its first 1
            assert bool(first.gather(1, ti.unsqueeze(1)).all())                                  # torch's index names a maximal element too
            if kind.startswith("nan"):
                assert bool(torch.isnan(val).all()) and bool((idx == C.colmax_nan_row(shape, kind)).all())
                assert bool(torch.isnan(tv).all()) and bool(torch.isnan(E.gather(1, ti.unsqueeze(1))).all())
            dval = _r("dval", *val.shape)
            Ea = torch.nan_to_num(E, nan=0.0, posinf=0.0, neginf=0.0).requires_grad_(True)
            R.select_rows(Ea, idx).backward(dval)
            assert torch.equal(R.colmax_bwd(dval, idx, shape[1]), Ea.grad)


def test_gather_matches_torch_f64():
    for shape in C.GATHER_SHAPES:
        B, Cc, Nn = shape
        for kind in C.GATHER_INDEX:
            idx = C.gather_index(shape, kind)
            V = _r("V", *shape).requires_grad_(True)
            T = R.gather_cols(V, idx)
            assert torch.equal(T, torch.gather(V, 2, idx.view(B, 1, Nn).expand(-1, Cc, -1)))
            dT = _r("dT", *shape)
            T.backward(dT)
            dV, mag, hits = R.gather_cols_bwd(dT, idx)
            _close(dV, V.grad)
            _close(dV, torch.zeros(shape, dtype=F64).scatter_add_(2, idx.view(B, 1, Nn).expand(-1, Cc, -1), dT))
            assert bool((dV[(hits == 0).unsqueeze(1).expand(-1, Cc, -1)] == 0).all())
            assert int(hits.sum()) == B * Nn
    x = _r("label", 2, 1, 8, 8)
    assert torch.equal(R.gather_cols(x.view(2, 1, 64), R.rot270_index(8).expand(2, -1)).view(2, 1, 8, 8), torch.rot90(x, 3, (2, 3)))


def test_mean_product_softmax_match_torch_f64():
    x = _r("mean", 65, 7).requires_grad_(True)
    m = x.mean(1) * 0.01
    _close(R.spatial_mean(x, 0.01)[0], m)
    d = _r("dmean", 65)
    m.backward(d)
    _close(R.spatial_mean_bwd(d, 7, 0.01), x.grad)
    attn, V, dO = _r("attn", 2, 5, 5).requires_grad_(True), _r("V", 2, 3, 5, 5).requires_grad_(True), _r("dO", 2, 3, 5, 5)
    out = attn.unsqueeze(1) @ V
    _close(R.bcast_matmul(attn, V), out)
    _close(R.bcast_matmul_terms(attn, V), attn.abs().unsqueeze(1) @ V.abs())
    out.backward(dO)
    da, _, dv, _ = R.bcast_matmul_bwd(attn, V, dO)
    _close(da, attn.grad)
    _close(dv, V.grad)
    a, s, g = _r("a", 3, 5, 37).requires_grad_(True), _r("s", 3, 1, 37).requires_grad_(True), _r("g", 3, 5, 37)
    y = a * s
    _close(R.mul_bcast_c(a, s), y, 0)
    y.backward(g)
    _close(R.mul_bcast_c_bwd_s(g, a)[0], s.grad[:, 0])
    for shape in C.SOFTMAX_CASES:
        xs = C.softmax_input(shape)
        _close(R.softmax_c2(xs), torch.softmax(xs.double(), 1))


def test_chains_match_torch_and_the_oracle_f64():
    ref = C.mlp_reference()
    inp = ref.inp
    L = [getattr(inp, n).double().requires_grad_(True) for n in C.MLP_LEAVES]
    cx = SimpleNamespaceP({"m.transform_module.fc_transform.0.weight": L[1], "m.transform_module.fc_transform.0.bias": L[2],
                           "m.transform_module.fc_transform.2.weight": L[3], "m.transform_module.fc_transform.2.bias": L[4],
                           "m.retransform_module.fc_transform.0.weight": L[1], "m.retransform_module.fc_transform.0.bias": L[2],
                           "m.retransform_module.fc_transform.2.weight": L[3], "m.retransform_module.fc_transform.2.bias": L[4]})
    y = J.cvp(cx, "m", L[0])[0]
    y.backward(inp.dy.double())
    own = C.mlp_evaluate(ref, [p > 0 for p in ref.pre])
    for key, t in zip(C.MLP_KEYS, [y.detach()] + [t.grad for t in L]):
        _close(own[key], t)
    # the CCT algebra against torch.bmm / max / gather / matmul, as oracle.jp_oracle.cct composes them
    ref = C.cct_reference()
    inp = ref.inp
    B, Ck, Cc, n = C.CCT_DIMS
    k, q, v, res, kd, qd, vd = L = [getattr(inp, nm).double().requires_grad_(True) for nm in C.CCT_LEAVES]
    S, arg = J._max_dim1(torch.bmm(k.permute(0, 2, 1), q))
    T = torch.gather(v, 2, arg.view(B, 1, -1).expand(-1, Cc, -1)).view(B, Cc, n, n)
    attn, arg_d = J._max_dim1(kd.permute(0, 2, 1) @ qd)
    out = res + T * S.view(B, 1, n, n) + attn.view(B, 1, n, n) @ vd
    out.backward(inp.go.double())
    assert torch.equal(arg, ref.amb[0].idx) and torch.equal(arg_d, ref.amb[1].idx)
    own = C.cct_evaluate(ref, [a.idx for a in ref.amb])
    for key, t in zip(C.CCT_KEYS, [out.detach(), S.detach(), attn.detach()] + [t.grad for t in L]):
        _close(own[key], t)


class SimpleNamespaceP:
    """the one attribute oracle.jp_oracle.cvp reads of its context"""
    def __init__(self, P):
        self.P = P


# ------------------------------------------------------------------------------------------- 2. launch paths
def test_mirrored_lines_stand_in_the_source():
    for path, lines in C.SOURCE_LINES.items():
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for key, (line, count) in lines.items():
            assert text.count(line) == count, f"{key}: {path} changed; update dense_cases.SOURCE_LINES, its mirror and the cases"
    assert (C.TS, C.CS_COLS, C.CS_LANES, C.WG_SMALL, C.WG, C.BIAS_BLOCK_CAP, C.TPB) == (16, 64, 16, 64, 256, 65535, 256)
    assert C.CS_COLS * C.CS_LANES == 1024


@pytest.mark.parametrize("name", list(C.GEMM_CASES))
def test_gemm_cases_take_their_paths(name):
    c = C.GEMM_CASES[name]
    L = C.gemm_launch(c["M"], c["N"], c["K"])
    assert c["claim"], name
    for k, v in c["claim"].items():
        assert getattr(L, k) == v, (name, k, getattr(L, k), v)


def test_gemm_cases_cover_what_the_single_old_shape_missed():
    Ls = {n: C.gemm_launch(c["M"], c["N"], c["K"]) for n, c in C.GEMM_CASES.items()}
    assert C.gemm_launch(10, 36, 36).row_tiles == 1 and C.gemm_launch(36, 36, 10).row_tiles == 3          # the old shape's three calls
    f = Ls["forward form"]
    assert f.row_tiles == 3 and f.col_tiles == 2 and f.k_trips == 2 and min(f.row_short, f.col_short, f.k_short) > 0
    g = C.GEMM_CASES
    assert g["forward form"]["tB"] and g["weight-gradient form"]["tA"] and g["weight-gradient form"]["beta"] == 1
    assert g["both transposes"]["tA"] and g["both transposes"]["tB"]
    assert g["exact K chunk"]["K"] == C.TS and g["K chunk plus one"]["K"] == C.TS + 1
    assert (g["scaled"]["alpha"], g["scaled"]["beta"]) == (-0.5, 0.25)
    assert g["padded leading dimensions"]["pad"] == (3, 5, 2)
    # only the padded case has lda != K on a non-transposed A: a kernel that takes K for lda fails there alone
    for n, c in g.items():
        lda = C.gemm_args(c)[0]
        assert (lda != c["K"] and not c["tA"]) == (n == "padded leading dimensions"), n
    # the batched cases are bmm_tn's three calls for k, q (3, 5, 37): strides C N, C N, N N / C N, N N, C N
    for n, want in (("batched", (5 * 37, 5 * 37, 37 * 37)), ("batched adjoint dk", (5 * 37, 37 * 37, 5 * 37)),
                    ("batched adjoint dq", (5 * 37, 37 * 37, 5 * 37))):
        assert C.gemm_args(g[n])[3:6] == want, n
    assert C.gemm_args(g["shared operand"])[3] == 0
    for n in C.GEMM_CASES:
        gc = C.gemm_case(n)
        if gc.case["beta"] == 0:
            assert bool(torch.isnan(gc.C[gc.ic]).all())            # written onto NaN
        else:
            assert float(gc.C[gc.ic].abs().min()) > 0              # added onto a non-empty C
        assert bool((gc.C[gc.padmask] == C.SENTINEL).all())
    assert int(C.gemm_case("padded leading dimensions").padmask.sum()) == 33 * 2


def test_row_cases_take_their_paths():
    for shape, claim in C.COLSUM_CASES.items():
        L = C.colsum_launch(*shape)
        for k, v in claim.items():
            assert getattr(L, k) == v, (shape, k, getattr(L, k), v)
    assert C.colsum_launch(10, 36).trips == 1                    # the old shape never took a second trip ...
    assert sum(C.colsum_launch(*s).trips > 1 for s in C.COLSUM_CASES) == 4          # ... four cases here do
    assert any(s[1] == 1 for s in C.COLSUM_CASES) and any(C.BIAS_CASES[n][1] == 1 for n in C.BIAS_CASES)
    assert {C.BIAS_CASES[n][2] for n in C.BIAS_CASES if n.startswith("33x17 act")} == {0, 1, 2, 3}
    for n, (M, N, act, b) in C.BIAS_CASES.items():
        assert not C.bias_launch(M * N).strides
    big = C.bias_launch(C.BIAS_BIG_TOTAL)
    assert big.blocks == C.BIAS_BLOCK_CAP and big.strides and big.tail == 77
    assert C.BIAS_BIG_TOTAL % C.BIAS_BIG_N == 0 and C.BIAS_BIG_TOTAL == 65535 * 256 + 77


def test_index_cases_take_their_paths():
    for (B, Rr, Cn), claim in C.COLMAX_SHAPES.items():
        L = C.index_launch(B * Cn, C.WG_SMALL)
        assert (L.blocks, L.idle) == claim["fwd"]
        L = C.index_launch(B * Rr * Cn, C.WG)
        assert (L.blocks, L.idle) == claim["bwd"]
    assert sum(B * Rr * Cn % 256 != 0 for B, Rr, Cn in C.COLMAX_SHAPES) == 2          # adjoint totals that are no multiple of 256
    assert max(C.index_launch(B * Cn, 64).blocks for B, _, Cn in C.COLMAX_SHAPES) > 1
    for (B, Cc, Nn), claim in C.GATHER_SHAPES.items():
        L = C.index_launch(B * Cc * Nn, C.WG)
        assert (L.blocks, L.idle) == claim
    assert C.index_launch(2 * C.ROT_N ** 2, C.WG).blocks == 512
    for (BC, HW), (fwd, bwd) in C.MEAN_CASES.items():
        assert (C.index_launch(BC, C.WG_SMALL).blocks, C.index_launch(BC * HW, C.WG).blocks) == (fwd, bwd)
    for (B, Cc, n), (fwd, bwd_a) in C.BCAST_CASES.items():
        assert (C.index_launch(B * Cc * n * n, C.WG).blocks, C.index_launch(B * n * n, C.WG_SMALL).blocks) == (fwd, bwd_a)
    for (B, Cc, HW), blocks in C.MUL_CASES.items():
        assert min(C.cdiv(B * Cc * HW, C.TPB), C.POINTWISE_BLOCK_CAP) == blocks


# ------------------------------------------------------------------------------------------- 3. input conditions and caps
def test_special_energies_are_what_they_claim():
    for shape in C.COLMAX_SHAPES:
        B, Rr, Cn = shape
        E = C.colmax_input(shape, "ties")
        assert torch.equal(E * 2, torch.round(E * 2))
        if Rr > 1:
            top = E.max(1).values
            assert int(((E == top.unsqueeze(1)).sum(1) > 1).sum()) > 0.2 * B * Cn, "hardly any column has an exact tie"
        E = C.colmax_input(shape, "constant column")
        assert bool((E[:, :, 0] == (0.75 if Cn > 1 else -2.0)).all()) and bool((E[:, :, Cn // 2] == -2.0).all())
        E = C.colmax_input(shape, "-inf column")
        assert bool(torch.isinf(E[:, :, Cn // 2]).all()) and bool((E[:, :, Cn // 2] < 0).all())
        E = C.colmax_input(shape, "+inf")
        assert bool((E[:, Rr // 2] == float("inf")).all()) and int(torch.isnan(E).sum()) == 0
        for kind in ("nan row 0", "nan middle", "nan last"):
            E = C.colmax_input(shape, kind)
            assert bool((torch.isnan(E).sum(1) == 1).all()) and bool(torch.isnan(E[:, C.colmax_nan_row(shape, kind)]).all())
    for shape in C.GATHER_SHAPES:
        B, _, Nn = shape
        rep, eq, perm = (C.gather_index(shape, k) for k in C.GATHER_INDEX)
        for idx in (rep, eq, perm):
            assert idx.dtype == torch.int64 and idx.shape == (B, Nn) and int(idx.min()) >= 0 and int(idx.max()) < Nn
            assert B == 1 or not torch.equal(idx[0], idx[1])                       # a different row per batch
        assert all(len(set(r.tolist())) < Nn for r in rep) and all(len(set(r.tolist())) == 1 for r in eq)
        assert all(sorted(r.tolist()) == list(range(Nn)) for r in perm)


def test_softmax_cases_hold_every_difference():
    for shape in C.SOFTMAX_CASES[1:]:
        x = C.softmax_input(shape)
        assert bool(torch.isfinite(x).all())
        d = (x[:, 1].double() - x[:, 0].double()).reshape(-1)
        for want in C.SOFTMAX_DIFFS:
            assert bool(((d - want).abs() <= 1e-5 * max(1.0, abs(want))).any()), (shape, want)
        assert float(x.max()) >= 190 and float(x.min()) <= -190          # exp overflows / underflows in fp32 without the max subtraction
    assert len(C.softmax_single_inputs()) == len(C.SOFTMAX_DIFFS) and C.SOFTMAX_CASES[0] == (1, 1)
    assert set(abs(d) for d in C.SOFTMAX_DIFFS) == {0.0, 1e-3, 20.0, 90.0, 200.0}


def test_ambiguous_shares_are_within_the_cap():
    """recorded: no committed seed has an ambiguous column; the MLP's ambiguous gates are printed below"""
    for shape in C.AMBIGUITY_SHAPES:
        a = C.energy_ambiguity(C.randn(f"amb k {shape}", *shape), C.randn(f"amb q {shape}", *shape))
        print(f"k, q {shape}: ambiguous columns {float(a.amb.double().mean()):.2e}, smallest top-two gap {float(a.gap.min()):.2e}, "
              f"largest allowance {float(a.allow.max()):.2e}")
        assert float(a.amb.double().mean()) <= C.MASK_CAP
        assert float(a.allow.max()) <= 18 * C.U * 64                    # (K + 2) u sum |terms| with sum |terms| far below 64
    cct = C.cct_reference()
    for nm, a, s in zip(("cross-view", "depth"), cct.amb, cct.share):
        print(f"CCT chain, {nm} energy: ambiguous columns {s:.2e}, smallest gap {float(a.gap.min()):.2e}, largest allowance "
              f"{float(a.allow.max()):.2e}")
        assert s == 0.0, "the committed seeds were chosen to need no ambiguous column"
    mlp = C.mlp_reference()
    for layer, (a, s) in enumerate(zip(mlp.amb, mlp.share)):
        print(f"MLP chain, layer {layer + 1}: ambiguous gates {int(a.sum())} of {a.numel()} ({s:.2e})")
        assert s <= C.MASK_CAP
    # the replay rules notice a wrong decision
    a = cct.amb[0]
    assert C.replay_index(a, a.idx)[1] == 0 and C.replay_index(a, (a.idx + 1) % 64)[1] > 0
    assert C.replay_index(a, a.second)[1] == a.idx.numel()                # unambiguous columns: the runner-up is wrong everywhere
    p, m = mlp.pre[0], mlp.amb[0]
    assert C.replay_gate(p, m, p > 0)[1] == 0 and C.replay_gate(p, m, p <= 0)[1] == int((~m).sum())


# ------------------------------------------------------------------------------------------- 4. derived bounds
def test_derived_bounds_arithmetic():
    u = 2.0 ** -24
    assert C.U == u and C.gemm_bound(1) == 4 * u and C.gemm_bound(1024) == 1027 * u
    assert C.colsum_bound(1) == 17 * u and C.colsum_bound(16) == 17 * u and C.colsum_bound(17) == 18 * u and C.colsum_bound(1024) == 80 * u
    assert C.mean_bound(1) == u and C.mean_bound(120) == 120 * u and C.MEAN_BWD_BOUND == 2 * u
    assert C.bias_bound(0) == C.bias_bound(1) == u and C.bias_bound(2) == 2 * u
    assert C.gate_allowance(64, torch.tensor(1.0, dtype=F64)) == 66 * u and C.SOFTMAX_SUM_BOUND == 2 * u
    # a serial fp32 sum stays inside its bound: emulate the GEMM's fmaf chain and the column sum's lanes in fp32 on the CPU
    g = C.gemm_case("forward form")
    a, b = R.gemm_operands(g.A, g.B, *g.abi[:5], *g.abi[6:8], *g.abi[9:12])
    acc = torch.zeros(1, 33, 17)
    for k in range(19):
        acc = (a[:, :, k:k + 1].double() * b[:, k:k + 1, :].double() + acc.double()).float()          # fmaf: one rounding
    assert C.err_terms(acc, g.ref[g.ic], g.mag) <= C.gemm_bound(19)
    c = C.colsum_case((100, 130))
    part = torch.zeros(16, 130)
    for r in range(100):
        part[r % 16] += c.x[r]
    s = part[0].clone()
    for k in range(1, 16):
        s += part[k]
    assert C.err_terms(s, *c.write) <= C.colsum_bound(100)
    assert C.err_terms(s + c.out0, *c.add) <= C.colsum_bound(100)
    # where the measured bar is the smaller one it is the one that holds
    assert C.sum_bar("gemm", C.gemm_bound(1024)) == C.BARS["gemm"] < C.gemm_bound(1024)
    assert C.sum_bar("gemm", C.gemm_bound(1)) == min(C.gemm_bound(1), C.BARS["gemm"])


# ------------------------------------------------------------------------------------------- 5. bars from the fp32 evaluation's error
def fp32_figures():
    """-> ({family: largest error of the fp32 CPU evaluation}, [(family, case, error)...])"""
    e = {k: 0.0 for k in C.ORACLE_ERR}
    per_case = []

    def up(key, case, v):
        e[key] = max(e[key], v)
        per_case.append((key, case, v))

    for name in C.GEMM_CASES:
        g = C.gemm_case(name)
        up("gemm", name, C.gemm_figure(g, C.gemm_fp32(g)))
    for name in C.BIAS_CASES:
        c = C.bias_case(name)
        got = C.bias_fp32(c)
        if c.act == 3:
            up("sigmoid", name, float((got.double() - c.want).abs().max()))
        else:
            up("bias_act", name, C.err_terms(got, c.want, c.mag))
    for shape in C.COLSUM_CASES:
        c = C.colsum_case(shape)
        up("colsum", shape, C.err_terms(c.x.sum(0), *c.write))
        up("colsum", (shape, "add"), C.err_terms(c.out0 + c.x.sum(0), *c.add))
    for shape in C.GATHER_SHAPES:
        B, Cc, Nn = shape
        for kind in C.GATHER_INDEX:
            idx = C.gather_index(shape, kind)
            dT = C.randn(f"gather dT {shape}", *shape)
            want, mag, _ = R.gather_cols_bwd(dT, idx)
            got = torch.zeros(shape).scatter_add_(2, idx.view(B, 1, Nn).expand(-1, Cc, -1), dT)
            up("gather_bwd", (shape, kind), C.err_terms(got, want, mag))
    for shape in C.MEAN_CASES:
        x, d = C.randn(f"mean {shape}", *shape), C.randn(f"mean d {shape}", shape[0])
        up("spatial_mean", shape, C.err_terms(x.mean(1) * C.MEAN_SCALE, *R.spatial_mean(x, C.MEAN_SCALE32)))
        xa = x.clone().requires_grad_(True)
        (xa.mean(1) * C.MEAN_SCALE).backward(d)
        want = R.spatial_mean_bwd(d, shape[1], C.MEAN_SCALE32)
        up("spatial_mean_bwd", shape, C.err_terms(xa.grad, want, want.abs()))
    for shape in C.BCAST_CASES:
        B, Cc, n = shape
        attn, V, dO = (C.randn(f"bcast {nm} {shape}", *s) for nm, s in (("attn", (B, n, n)), ("V", (B, Cc, n, n)), ("dO", (B, Cc, n, n))))
        a32, v32 = attn.clone().requires_grad_(True), V.clone().requires_grad_(True)
        out = a32.unsqueeze(1) @ v32
        out.backward(dO)
        up("bcast_fwd", shape, C.err_terms(out, R.bcast_matmul(attn.double(), V.double()), R.bcast_matmul_terms(attn.double(), V.double())))
        da, da_mag, dv, dv_mag = R.bcast_matmul_bwd(attn, V, dO)
        up("bcast_bwd_a", shape, C.err_terms(a32.grad, da, da_mag))
        up("bcast_bwd_v", shape, C.err_terms(v32.grad, dv, dv_mag))
    for shape in C.MUL_CASES:
        g, a = C.randn(f"mul g {shape}", *shape), C.randn(f"mul a {shape}", *shape)
        up("mul_bwd_s", shape, C.err_terms((g * a).sum(1), *R.mul_bcast_c_bwd_s(g, a)))
    for shape in C.SOFTMAX_CASES:
        x = C.softmax_input(shape)
        up("softmax", shape, float((torch.softmax(x, 1).double() - R.softmax_c2(x)).abs().max()))
    for x in C.softmax_single_inputs():
        up("softmax", "(1, 1) " + str(float(x[0, 1, 0] - x[0, 0, 0])), float((torch.softmax(x, 1).double() - R.softmax_c2(x)).abs().max()))
    ref = C.mlp_reference()
    want, _, gates = C.mlp_replay(ref, [p > 0 for p in ref.pre])
    got = C.mlp_evaluate(ref, gates, torch.float32)
    seeds = C.chain_seeds("mlp", want, C.MLP_LEAVES)
    added = {k: (v + seeds[k[1:]] if k[0] == "d" else v) for k, v in got.items()}
    for figs in (C.chain_figures("mlp", got, want), C.chain_figures("mlp", added, want, seeds)):
        for label, v, key in figs:
            up(key, label, v)
    ref = C.cct_reference()
    want, _, idx = C.cct_replay(ref, [a.idx for a in ref.amb])
    got = C.cct_evaluate(ref, idx, torch.float32)
    seeds = C.chain_seeds("cct", want, C.CCT_LEAVES)
    added = {k: (v + seeds[k[1:]] if k[0] == "d" else v) for k, v in got.items()}
    for figs in (C.chain_figures("cct", got, want), C.chain_figures("cct", added, want, seeds)):
        for label, v, key in figs:
            up(key, label, v)
    return e, per_case


def test_bars_follow_from_the_fp32_evaluation():
    t0 = time.time()
    with C.one_thread():
        measured, per_case = fp32_figures()
    for k, case, v in per_case:
        print(f"{k:18s} {str(case):52s} fp32 evaluation error {v:.3e}")
    for k, v in measured.items():
        print(f"{k:18s} fp32 evaluation error {v:.3e}  recorded {C.ORACLE_ERR[k]:.3e}  bar {C.BARS[k]:.0e}")
    print(f"references and fp32 evaluations built in {time.time() - t0:.1f} s")
    for k, v in measured.items():
        # the recorded figures reproduce (25 % of room for another CPU's vector width and libm), and no recorded figure, and so no
        # bar, is far above what is measured
        assert v <= 1.25 * C.ORACLE_ERR[k], k
        assert v >= 0.25 * C.ORACLE_ERR[k], k
    assert set(C.BARS) == set(C.ORACLE_ERR) == set(C.FORMER_BARS)
    from tests.photometric_cases import round_up_1sig           # the suite's rule, which dense_cases restates
    assert all(C.round_up_1sig(8 * v) == round_up_1sig(8 * v) for v in C.ORACLE_ERR.values())
    for k, bar in C.BARS.items():
        rule = C.round_up_1sig(8 * C.ORACLE_ERR[k]) if C.ORACLE_ERR[k] > 0 else 0.0
        if C.FORMER_BARS[k] is not None and rule > C.FORMER_BARS[k]:
            assert bar == C.FORMER_BARS[k], k                    # never looser than tests/test_kernels_gpu.py
        else:
            assert bar == pytest.approx(rule, rel=1e-9), k
