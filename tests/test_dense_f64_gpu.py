"""The dense algebra of the BEV-layout head -- the twelve entry points of jperceiver_amd/csrc/small.hip and jp_mul_bcast_c,
jp_mul_bcast_c_bwd_s and jp_softmax_c2 of pointwise.hip -- per element against FLOAT64 references (tests/dense_ref.py on the CPU), at
the smallest shapes that reach every tile, ragged tail, trip of a row loop and workgroup count, plus the step's own shapes
(tests/dense_cases.py mirrors the launch constants; tests/test_dense_ref_cpu.py checks every path claim, and every condition below,
without a GPU).

Every kernel is called through the C ABI (_lib.call), so strides, leading dimensions, NULL arguments and what the output buffer held
before are visible; every output buffer is NaN before the call unless the case accumulates into it.  The two chains (the CVP MLP's
two linear_acts; the CCT algebra bmm_tn -> colmax -> gather_cols -> mul_bcast_c plus bmm_tn -> colmax -> bcast_matmul) go through
ops / ops_loss on a Tape, once into fresh gradients and once adding onto seeded gradients of every leaf.

Ambiguous decisions.  A ReLU gate of a chain whose float64 pre-activation lies within (K + 2) 2^-24 sum |terms| of zero takes the
device's decision; a column whose two largest float64 energies lie within that allowance (the larger of the two) of each other
takes the device's index if it names one of those two.  Everywhere else the device must agree with the reference.  At most 0.5 % of
a case may be decided by the device; the committed seeds have NO ambiguous gate (0 of 16 384 in either layer) and NO ambiguous
column (smallest top-two gap 8.3e-4 / 4.5e-3 against allowances of at most 2.6e-5; for standard-normal k, q at (8, 16, 64),
(2, 16, 64), (2, 16, 1024): gaps 1.0e-4, 2.4e-2, 2.9e-4 against at most 3.1e-5).  The kernel-level column-max tests give E directly:
their decisions are exact and need no mask.

Bars.  Sums and products: per element |err| / sum |terms| (|a b| per product, plus |beta c| or the seeded value in add cases), held
to the SMALLER of (a) the derived first-order bound of the kernel's own summation (derived in tests/dense_cases.py next to the loop
it describes) and (b) 8 x the largest error of an fp32 CPU evaluation (ATen) against the float64 reference over the family's cases,
rounded up to one significant digit.  No hardware allowance is added.  (fp32 figures: x86-64 CPU, one thread;
tests/test_dense_ref_cpu.py recomputes them.)

  family             (a) derived                 fp32 evaluation   (b)      largest measured on the MI355X
  GEMM               (K + 3) u                   2.97e-7           3e-6     2.97e-7 (1024 x 64 x 64; 4.1e-8 .. 2.4e-7 elsewhere)
  bias + act 0..2    1 u (leaky: 2 u)            5.96e-8           5e-7     5.96e-8 (the cap case included)
  sigmoid            max |err|                   6.92e-8           6e-7     7.75e-8
  column sum         (ceil(M / 16) + 16) u       8.62e-8           7e-7     8.62e-8
  gather adjoint     hits u                      1.42e-7           2e-6     1.42e-7 (0.55 of min(hits u, 2e-6) at most)
  spatial mean       HW u                        1.04e-7           9e-7     1.01e-7 ((1, 1): 4.6e-8 against 1 u = 5.96e-8)
  its adjoint        2 u                         9.14e-8           8e-7     9.14e-8
  n x n product      n u                         1.84e-7           2e-6     1.84e-7
  its dattn          C n u                       1.24e-7           1e-6     1.38e-7
  its dV             n u                         1.82e-7           2e-6     1.82e-7
  ds of a * s        C u                         1.14e-7           1e-6     1.30e-7
  softmax            max |err|                   8.65e-8           7e-7     9.50e-8; |y0 + y1 - 1| 8.94e-8 against 2 u = 1.19e-7

The scale of the spatial mean is the fp32 value of 0.01 in the references (what the kernels receive), as eps is in the BatchNorm
suite.  Many device figures equal ATen's to the last digit: at these sizes both sum serially in the same order.

Exact by construction, held bit for bit: the column max and its index (first maximum; NaN gives NaN and the row of the first NaN),
its scatter adjoint, the gather, the single product a * s, the padding columns of C, and a second run of the column sum.

Chains, per tensor max |err| / max |ref| under the 8 x rule against an fp32 autograd evaluation with the same replayed decisions
(held to before: tests/test_kernels_gpu.py::test_linear_and_cct_algebra, relative to max(1, max |ref|)):

  y 2.16e-7 -> 2e-6 (1.1e-4)      dx 2.77e-7 -> 3e-6 (2.1e-4)     dw1 3.19e-7 -> 3e-6 (2.1e-4)    db1 1.24e-7 -> 1e-6 (2.1e-4)
  dw2 2.77e-7 -> 3e-6 (2.1e-4)    db2 1.48e-7 -> 2e-6 (2.1e-4)    out 1.42e-7 -> 2e-6 (1.1e-4)    S 1.24e-7 -> 1e-6 (--)
  attn 1.38e-7 -> 2e-6 (--)       dk 1.55e-7 -> 2e-6 (2.1e-4)     dq 1.21e-7 -> 1e-6 (2.1e-4)     dv 1.03e-7 -> 9e-7 (2.1e-4)
  dres 2.92e-8 -> 3e-7 (--)       dkd 1.55e-7 -> 2e-6 (2.1e-4)    dqd 1.40e-7 -> 2e-6 (2.1e-4)    dvd 1.35e-7 -> 2e-6 (2.1e-4)

Measured on the MI355X (the larger of the fresh and the add run): y 2.16e-7, dx 2.77e-7, dw1 3.19e-7, db1 1.36e-7, dw2 2.77e-7,
db2 9.4e-8, out 1.42e-7, S 1.24e-7, attn 1.38e-7, dk 5.83e-7, dq 6.57e-7, dv 1.03e-7, dres 2.92e-8, dkd 5.23e-7, dqd 4.56e-7,
dvd 1.35e-7 (dk, dq, dkd, dqd carry dS / dattn: the serial sums over 128 and 1024 terms against ATen's blocked ones).  The whole file runs in 4 s.

Every test prints its figures before it asserts them (pytest -s).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops, ops_loss                                       # noqa: E402
from jperceiver_amd._lib import call                                           # noqa: E402
from jperceiver_amd.model import net                                           # noqa: E402
from jperceiver_amd.ops import Var, Tape, recording                            # noqa: E402
from tests import dense_cases as C                                             # noqa: E402
from tests import dense_ref as R                                               # noqa: E402

DEV = "cuda"
NAN = float("nan")


def _poison(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _hold(label, err, bar):
    """print, then return the failure text (or None)"""
    print(f"  {label:52s} {err:.3e}   bar {bar:.3e}")
    return None if err <= bar else f"{label}: {err:.3e} > {bar:.3e}"


def _assert(bad):
    bad = [b for b in bad if b]
    assert not bad, "; ".join(bad)


def _finite(t, what):
    """print the count of non-finite elements, then return the failure text (or None): asserted with the figures, after them"""
    n = int((~torch.isfinite(t)).sum())
    print(f"  {what}: non-finite elements {n} of {t.numel()}")
    return f"{what}: {n} non-finite elements (a NaN of the poisoned buffer, or an overflow, is left)" if n else None


def _flag(ok, text):
    return None if ok else text


# ------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("name", list(C.GEMM_CASES))
def test_gemm_f64(name):
    g = C.gemm_case(name)
    c = g.case
    L = C.gemm_launch(c["M"], c["N"], c["K"])
    print(f"  {L.row_tiles} x {L.col_tiles} tiles ({L.row_short} rows, {L.col_short} columns short), {L.k_trips} K trips "
          f"({L.k_short} short), batch {c['batch']}, tA {c['tA']} tB {c['tB']} alpha {c['alpha']} beta {c['beta']} pad {c['pad']}")
    Cd = g.C.to(DEV)
    call("jp_gemm_strided_batched", g.A.to(DEV), g.B.to(DEV), Cd, *g.abi)
    got = Cd.cpu()
    pad_changed = int((C.bits(got[g.padmask]) != C.bits(g.C[g.padmask])).sum())
    print(f"  padding elements of C that changed: {pad_changed} of {int(g.padmask.sum())}")
    _assert([_hold("|err| / sum |terms|", C.gemm_figure(g, got), C.sum_bar("gemm", C.gemm_bound(c["K"]))), _finite(got[g.ic], "C"),
             _flag(pad_changed == 0, "a padding column of C changed")])


# ------------------------------------------------------------------------------------------- bias + activation
def _bias_run(c):
    y = c.y.to(DEV).clone()
    call("jp_bias_act_rows", y, _dev(c.bias), c.M, c.N, c.act)
    return y.cpu()


@pytest.mark.parametrize("name", list(C.BIAS_CASES))
def test_bias_act_rows_f64(name):
    c = C.bias_case(name)
    got = _bias_run(c)
    bad = [_finite(got, "y")]
    if c.act == R.ACT_SIGMOID:
        bad.append(_hold("sigmoid max |err|", float((got.double() - c.want).abs().max()), C.BARS["sigmoid"]))
    else:
        if c.act in (R.ACT_RELU, R.ACT_LEAKY):          # the fp32 add is correctly rounded: every gate is the reference's
            wrong = int(((got > 0) != (c.pre > 0)).sum())
            print(f"  gates that differ from the reference: {wrong}")
            bad.append(_flag(wrong == 0, f"{wrong} gates differ from the reference"))
        bad.append(_hold("|err| / (|y| + |bias|)", C.err_terms(got, c.want, c.mag), C.sum_bar("bias_act", C.bias_bound(c.act))))
    _assert(bad)


def test_bias_act_rows_strides_above_the_block_cap():
    c = C.bias_big_case()
    L = C.bias_launch(c.M * c.N)
    print(f"  {c.M} x {c.N} = {c.M * c.N} elements, {L.blocks} workgroups, {L.tail} elements beyond one pass")
    got = _bias_run(c)
    _assert([_finite(got, "y"), _hold("|err| / (|y| + |bias|)", C.err_terms(got, c.want, c.mag), C.sum_bar("bias_act", C.bias_bound(0)))])


# ------------------------------------------------------------------------------------------- column sum
@pytest.mark.parametrize("shape", list(C.COLSUM_CASES), ids=str)
def test_colsum_f64(shape):
    M, N = shape
    c = C.colsum_case(shape)
    L = C.colsum_launch(M, N)
    print(f"  {L.blocks} workgroups ({L.col_short} columns short), {L.trips} trips of the row loop ({L.lanes_short} lanes one fewer)")
    x = c.x.to(DEV)
    bad = []
    for mode, acc, (want, mag) in (("write", 0, c.write), ("add", 1, c.add)):
        runs = []
        for _ in range(2):
            out = c.out0.to(DEV).clone() if acc else _poison(N)
            call("jp_colsum", x, out, M, N, acc)
            runs.append(out.cpu())
        differ = int((C.bits(runs[0]) != C.bits(runs[1])).sum())
        print(f"  {mode}: elements of a second run that differ {differ}")
        bad += [_finite(runs[0], mode), _flag(differ == 0, f"{mode}: the fixed summation order must make two runs bit-equal")]
        bad.append(_hold(f"{mode}: |err| / sum |terms|", C.err_terms(runs[0], want, mag), C.sum_bar("colsum", C.colsum_bound(M))))
    _assert(bad)


# ------------------------------------------------------------------------------------------- column max
@pytest.mark.parametrize("shape", list(C.COLMAX_SHAPES), ids=str)
@pytest.mark.parametrize("kind", C.COLMAX_DATA)
def test_colmax_bit_for_bit(shape, kind):
    B, Rr, Cn = shape
    E = C.colmax_input(shape, kind)
    want_val, want_idx = R.colmax(E)
    Ed = E.to(DEV)
    val, arg = _poison(B, Cn), torch.full((B, Cn), -1, device=DEV, dtype=torch.int64)
    call("jp_colmax", Ed, val, arg, B, Rr, Cn)
    val2 = _poison(B, Cn)
    call("jp_colmax", Ed, val2, None, B, Rr, Cn)
    val, arg, val2 = val.cpu(), arg.cpu(), val2.cpu()
    nv, ni = int((C.bits(val) != C.bits(want_val)).sum()), int((arg != want_idx).sum())
    print(f"  {B * Cn} columns of {Rr}: values that differ {nv}, indices that differ {ni}, with arg = NULL {int((C.bits(val2) != C.bits(val)).sum())}")
    # the scatter adjoint, on the reference's index
    dval = C.randn(f"colmax dval {shape}", B, Cn)
    dE = _poison(B, Rr, Cn)
    call("jp_colmax_bwd", dval.to(DEV), want_idx.to(DEV), dE, B, Rr, Cn)
    dE = dE.cpu()
    nd = int((C.bits(dE) != C.bits(R.colmax_bwd(dval, want_idx, Rr))).sum())
    print(f"  adjoint: {B * Rr * Cn} elements ({B * Rr * Cn % 256} beyond whole workgroups), that differ {nd}")
    if kind.startswith("nan"):
        assert bool(torch.isnan(val).all()), "a NaN energy came out of the column max as a finite value"
        assert bool((arg == C.colmax_nan_row(shape, kind)).all()), "the index does not name the NaN element"
    assert nv == 0 and ni == 0
    assert torch.equal(C.bits(val2), C.bits(val)), "arg = NULL changed the values"
    assert nd == 0


# ------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("shape", list(C.GATHER_SHAPES), ids=str)
@pytest.mark.parametrize("kind", C.GATHER_INDEX)
def test_gather_cols_f64(shape, kind):
    B, Cc, Nn = shape
    idx = C.gather_index(shape, kind)
    V, dT = C.randn(f"gather V {shape}", *shape), C.randn(f"gather dT {shape}", *shape)
    T = _poison(*shape)
    call("jp_gather_cols", V.to(DEV), idx.to(DEV), T, B, Cc, Nn)
    dV = _poison(*shape)
    call("jp_gather_cols_bwd", dT.to(DEV), idx.to(DEV), dV, B, Cc, Nn)
    dV = dV.cpu()
    want, mag, hits = R.gather_cols_bwd(dT, idx)
    hits = hits.unsqueeze(1).expand(-1, Cc, -1)
    fwd_diff = int((C.bits(T.cpu()) != C.bits(R.gather_cols(V, idx))).sum())
    unselected = dV[hits == 0]
    nonzero = int((unselected != 0).sum())          # (a NaN left of the poisoned buffer counts: NaN != 0)
    print(f"  gathered elements that differ {fwd_diff}; unselected adjoint elements that are not exactly 0: {nonzero} of {unselected.numel()}")
    ratio = ((dV.double() - want).abs() / mag.clamp(min=1e-300))[hits > 0]
    bound = torch.clamp(hits[hits > 0] * C.U, max=C.BARS["gather_bwd"])
    worst = float((ratio / bound).max())
    print(f"  hits per element up to {int(hits.max())}; largest |err| / sum |terms| {float(ratio.max()):.3e}; largest share of its bar "
          f"(min(hits u, {C.BARS['gather_bwd']:.0e})) {worst:.3f}")
    _assert([_flag(fwd_diff == 0, "the gather is not bit-equal"), _finite(dV, "dV"),
             _flag(nonzero == 0, "an element that no index names is not exactly 0"), _flag(worst <= 1.0, f"adjoint at {worst:.3f} of its bar")])


def test_rot270_is_rot90_k3():
    n = C.ROT_N
    x = C.randn("rot270", 2, 1, n, n)
    got = net.rot270(x.to(DEV)).cpu()
    d_rot = int((C.bits(got) != C.bits(torch.rot90(x, 3, (2, 3)))).sum())
    d_ref = int((C.bits(got.view(2, 1, n * n)) != C.bits(R.gather_cols(x.view(2, 1, n * n), R.rot270_index(n).expand(2, -1)))).sum())
    print(f"  elements that differ from torch.rot90(k=3): {d_rot}, from the reference gather: {d_ref}")
    assert d_rot == 0 and d_ref == 0


# ------------------------------------------------------------------------------------------- spatial mean
@pytest.mark.parametrize("shape", list(C.MEAN_CASES), ids=str)
def test_spatial_mean_f64(shape):
    BC, HW = shape
    x, d = C.randn(f"mean {shape}", BC, HW), C.randn(f"mean d {shape}", BC)
    out, dx = _poison(BC), _poison(BC, HW)
    call("jp_spatial_mean", x.to(DEV), out, BC, HW, C.MEAN_SCALE)
    call("jp_spatial_mean_bwd", d.to(DEV), dx, BC, HW, C.MEAN_SCALE)
    out, dx = out.cpu(), dx.cpu()
    want, mag = R.spatial_mean(x, C.MEAN_SCALE32)
    wb = R.spatial_mean_bwd(d, HW, C.MEAN_SCALE32)
    _assert([_hold("mean: |err| / sum |terms|", C.err_terms(out, want, mag), C.sum_bar("spatial_mean", C.mean_bound(HW))),
             _hold("adjoint: |err| / |value|", C.err_terms(dx, wb, wb.abs()), C.sum_bar("spatial_mean_bwd", C.MEAN_BWD_BOUND)),
             _finite(out, "mean"), _finite(dx, "dx")])


# ------------------------------------------------------------------------------------------- per-channel n x n product
@pytest.mark.parametrize("shape", list(C.BCAST_CASES), ids=str)
def test_bcast_matmul_f64(shape):
    B, Cc, n = shape
    attn, V, dO = (C.randn(f"bcast {nm} {shape}", *s) for nm, s in (("attn", (B, n, n)), ("V", (B, Cc, n, n)), ("dO", (B, Cc, n, n))))
    ad, Vd, dOd = attn.to(DEV), V.to(DEV), dO.to(DEV)
    out = _poison(B, Cc, n, n)
    call("jp_bcast_matmul_fwd", ad, Vd, out, B, Cc, n)
    da, dv = _poison(B, n, n), _poison(B, Cc, n, n)
    call("jp_bcast_matmul_bwd", ad, Vd, dOd, da, dv, B, Cc, n)
    da_only = _poison(B, n, n)
    call("jp_bcast_matmul_bwd", ad, Vd, dOd, da_only, None, B, Cc, n)
    dv_only = _poison(B, Cc, n, n)
    call("jp_bcast_matmul_bwd", ad, Vd, dOd, None, dv_only, B, Cc, n)
    out, da, dv, da_only, dv_only = (t.cpu() for t in (out, da, dv, da_only, dv_only))
    null_diff = int((C.bits(da_only) != C.bits(da)).sum()) + int((C.bits(dv_only) != C.bits(dv)).sum())
    print(f"  elements that differ when the other output is NULL: {null_diff}")
    wa, wa_mag, wv, wv_mag = R.bcast_matmul_bwd(attn, V, dO)
    _assert([_hold("out: |err| / sum |terms|", C.err_terms(out, R.bcast_matmul(attn.double(), V.double()),
                                                           R.bcast_matmul_terms(attn.double(), V.double())), C.sum_bar("bcast_fwd", n * C.U)),
             _hold("dattn: |err| / sum |terms|", C.err_terms(da, wa, wa_mag), C.sum_bar("bcast_bwd_a", Cc * n * C.U)),
             _hold("dV: |err| / sum |terms|", C.err_terms(dv, wv, wv_mag), C.sum_bar("bcast_bwd_v", n * C.U)),
             _finite(out, "out"), _finite(da, "dattn"), _finite(dv, "dV"), _flag(null_diff == 0, "a NULL output changed the other one")])


# ------------------------------------------------------------------------------------------- channel-broadcast product, softmax
@pytest.mark.parametrize("shape", list(C.MUL_CASES), ids=str)
def test_mul_bcast_c_f64(shape):
    B, Cc, HW = shape
    a, g, s = C.randn(f"mul a {shape}", *shape), C.randn(f"mul g {shape}", *shape), C.randn(f"mul s {shape}", B, 1, HW)
    out, ds = _poison(*shape), _poison(B, HW)
    call("jp_mul_bcast_c", a.to(DEV), s.to(DEV), out, B, Cc, HW)
    call("jp_mul_bcast_c_bwd_s", g.to(DEV), a.to(DEV), ds, B, Cc, HW)
    out, ds = out.cpu(), ds.cpu()
    d32 = int((C.bits(out) != C.bits(a * s)).sum())
    d64 = int((C.bits(out) != C.bits(R.mul_bcast_c(a.double(), s.double()).float())).sum())
    print(f"  products that differ from the fp32 product {d32}, from the rounded float64 product {d64}")
    _assert([_hold("ds: |err| / sum |terms|", C.err_terms(ds, *R.mul_bcast_c_bwd_s(g, a)), C.sum_bar("mul_bwd_s", Cc * C.U)), _finite(ds, "ds"),
             _flag(d32 == 0 and d64 == 0, "one fp32 product must equal the fp32 product bit for bit")])


def _softmax_check(x):
    N, _, HW = x.shape
    y = _poison(N, 2, HW)
    call("jp_softmax_c2", x.to(DEV), y, N, HW)
    y = y.cpu()
    return _finite(y, "softmax"), float((y.double() - R.softmax_c2(x)).abs().max()), float((y[:, 0].double() + y[:, 1].double() - 1).abs().max())


@pytest.mark.parametrize("shape", C.SOFTMAX_CASES, ids=str)
def test_softmax_c2_f64(shape):
    runs = C.softmax_single_inputs() if shape == (1, 1) else [C.softmax_input(shape)]
    bad = []
    for x in runs:
        nonfinite, err, off = _softmax_check(x)
        tag = f"difference {float(x[0, 1, 0] - x[0, 0, 0]):g}: " if shape == (1, 1) else ""
        bad += [nonfinite, _hold(tag + "max |err|", err, C.BARS["softmax"]), _hold(tag + "max |y0 + y1 - 1|", off, C.SOFTMAX_SUM_BOUND)]
    _assert(bad)


# ------------------------------------------------------------------------------------------- chains
def _leaf(t, seed):
    return Var(t.to(DEV), True, seed.to(DEV).clone() if seed is not None else None)


def _check_chain(prefix, got, want, seeds, decisions):
    """decisions: the failure text of the gates / indices (or None); figures first, then every assertion"""
    _assert([_hold(label, err, C.BARS[key]) for label, err, key in C.chain_figures(prefix, got, want, seeds)]
            + [_finite(t, k) for k, t in got.items()] + [decisions])


@pytest.mark.parametrize("mode", ["fresh", "add"])
def test_mlp_chain_f64(mode):
    """TransformModule._fwd's two linear_acts on (2, 128, 8, 8): 256 rows of 64 features, ReLU twice"""
    ref = C.mlp_reference()
    inp = ref.inp
    B, Cc, H, W = C.MLP_SHAPE
    seeds = C.chain_seeds("mlp", C.mlp_replay(ref, [p > 0 for p in ref.pre])[0], C.MLP_LEAVES) if mode == "add" else None
    # parameter gradients accumulate into a buffer that exists before the step: zeros in the fresh run
    L = {n: _leaf(getattr(inp, n), seeds[n] if seeds else (None if n == "x" else torch.zeros_like(getattr(inp, n)))) for n in C.MLP_LEAVES}
    tape = Tape()
    with recording(tape):
        v = ops_loss.view(L["x"], (B, Cc, H * W))
        h = ops.linear_act(v, L["w1"], L["b1"], ops.ACT_RELU)
        y = ops.linear_act(h, L["w2"], L["b2"], ops.ACT_RELU)
        y = ops_loss.view(y, (B, Cc, H, W))
    dev_gates = [h.t.cpu() > 0, y.t.cpu().view(B, Cc, H * W) > 0]
    yt = y.t.cpu().clone()
    y.g = inp.dy.to(DEV).clone()
    tape.backward()
    torch.cuda.synchronize()
    want, wrong, _ = C.mlp_replay(ref, dev_gates)
    print(f"  ambiguous gates {ref.share[0]:.2e} / {ref.share[1]:.2e} of the two layers (cap {C.MASK_CAP}); unambiguous gates that differ {wrong}")
    got = dict(y=yt, **{"d" + n: L[n].g.cpu().view(getattr(inp, n).shape) for n in C.MLP_LEAVES})
    _check_chain("mlp", got, want, seeds, _flag(max(ref.share) <= C.MASK_CAP and wrong == [0, 0],
                                                f"the device's ReLU gate differs on {wrong} unambiguous elements, or the share is over the cap"))


@pytest.mark.parametrize("mode", ["fresh", "add"])
def test_cct_chain_f64(mode):
    """CrossViewTransformer._fwd without its convolutions: k, q (2, 16, 64), v (2, 128, 64), residual and depth values (2, 128, 8, 8)"""
    ref = C.cct_reference()
    inp = ref.inp
    B, Ck, Cc, n = C.CCT_DIMS
    seeds = C.chain_seeds("cct", C.cct_replay(ref, [a.idx for a in ref.amb])[0], C.CCT_LEAVES) if mode == "add" else None
    L = {nm: _leaf(getattr(inp, nm), seeds[nm] if seeds else None) for nm in C.CCT_LEAVES}
    v = ops_loss.view
    tape = Tape()
    with recording(tape):
        front_star, arg = ops_loss.colmax(ops_loss.bmm_tn(L["k"], L["q"]))
        T = v(ops_loss.gather_cols(L["v"], arg), (B, Cc, n, n))
        S = v(front_star, (B, 1, n, n))
        out = ops.add(L["res"], ops_loss.mul_bcast_c(T, S))
        attn, arg_d = ops_loss.colmax(ops_loss.bmm_tn(L["kd"], L["qd"]))
        attn = v(attn, (B, 1, n, n))
        out = ops.add(out, ops_loss.bcast_matmul(attn, L["vd"]))
    got = dict(out=out.t.cpu().clone(), S=S.t.cpu().view(B, n * n).clone(), attn=attn.t.cpu().view(B, n * n).clone())
    out.g = inp.go.to(DEV).clone()
    tape.backward()
    torch.cuda.synchronize()
    want, wrong, _ = C.cct_replay(ref, [arg.cpu(), arg_d.cpu()])
    print(f"  ambiguous columns {ref.share[0]:.2e} / {ref.share[1]:.2e} of the two energies (cap {C.MASK_CAP}); wrong indices {wrong}")
    got.update({"d" + nm: L[nm].g.cpu().view(getattr(inp, nm).shape) for nm in C.CCT_LEAVES})
    _check_chain("cct", got, want, seeds, _flag(max(ref.share) <= C.MASK_CAP and wrong == [0, 0],
                                                f"the device's index is wrong on {wrong} columns, or the share is over the cap"))
