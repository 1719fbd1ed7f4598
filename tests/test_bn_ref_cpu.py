"""CPU checks behind tests/test_bn_f64_gpu.py (no GPU):

1. tests/bn_ref.py agrees with ATen evaluated in float64 -- F.batch_norm in train and eval mode with the running statistics after one
   and two updates, F.max_pool2d(return_indices=True) with the converted argmax byte, and autograd through the same ops -- and keeps
   the first-maximum rule on planted exact ties;
2. every case built for a launch path lies on it, by the Python mirror of chunking() and of the launch expressions, and the mirrored
   source lines stand verbatim in bn.hip; the workspace queries of the library return what the mirror predicts;
3. the share of elements / windows that take the device's decision is within MASK_CAP for every committed seed, by the reference alone;
4. the bars of the GPU file follow from the fp32 evaluation's own error against the float64 reference (bn_cases.BARS);
5. every reference builds in seconds.
"""
import os
import time

import pytest
import torch
import torch.nn.functional as F

from jperceiver_amd import _lib
from tests import bn_cases as C
from tests import bn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _small(shape, res, seed=3):
    inp = C.train_inputs(shape, res, seed)
    return inp, [None if t is None else t.double() for t in (inp.x, inp.gamma, inp.beta, inp.rm, inp.rv, inp.dy, inp.residual)]


# ------------------------------------------------------------------------------------------- 1. restatement == ATen in float64
@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (3, 5, 7, 9), (2, 4, 6, 10)])
@pytest.mark.parametrize("mode", list(C.MODES))
@pytest.mark.parametrize("nup", [1, 2])
def test_train_matches_aten_f64(shape, mode, nup):
    relu, res = C.MODES[mode]
    _, (x, gamma, beta, rm, rv, dy, r) = _small(shape, res)
    ref = R.bn_train_fwd(x, gamma, beta, r, relu, C.EPS, C.MOMENTUM, nup, rm, rv)
    xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    ra = r.clone().requires_grad_(True) if res else None
    rm2, rv2 = rm.clone(), rv.clone()
    for _ in range(nup):
        y = F.batch_norm(xa, rm2, rv2, ga, ba, True, C.MOMENTUM, C.EPS)
    pre = y + ra if res else y
    y = F.relu(pre) if relu else pre
    assert C.err_max(ref.y, y) <= 1e-12 and C.err_max(ref.pre, pre) <= 1e-12
    assert C.err_max(ref.rm, rm2) <= 1e-12 and C.err_max(ref.rv, rv2) <= 1e-12
    _, m, i = torch.native_batch_norm(x, gamma, beta, None, None, True, C.MOMENTUM, C.EPS)
    assert C.err_max(ref.mean, m) <= 1e-12 and C.err_max(ref.invstd, i) <= 1e-12
    y.backward(dy)
    bwd = R.bn_train_bwd(dy, x, ref.mean, ref.invstd, gamma, (ref.pre > 0) if relu else None)
    assert C.err_max(bwd.dx, xa.grad) <= 1e-11
    assert C.err_max(bwd.dgamma, ga.grad) <= 1e-11 and C.err_max(bwd.dbeta, ba.grad) <= 1e-11
    if res:
        assert C.err_max(bwd.dres, ra.grad) <= 1e-12
    n = shape[0] * shape[2] * shape[3]
    if n == 2:                                         # the unbiased factor at the smallest count: 2
        assert C.unbiased_factor(n) == 2.0
        assert C.err_max(ref.rv, C.MOMENTUM * 2 * ref.var + (1 - C.MOMENTUM) * rv if nup == 1 else ref.rv) <= 1e-12


@pytest.mark.parametrize("res,relu", [(False, False), (True, True)])
def test_eval_and_channel_sum_match_aten_f64(res, relu):
    _, (x, gamma, beta, rm, rv, dy, r) = _small((3, 5, 7, 9), res)
    rv[0] = 0.0
    y = F.batch_norm(x, rm, rv, gamma, beta, False, C.MOMENTUM, C.EPS)
    y = y + r if res else y
    y = F.relu(y) if relu else y
    assert C.err_max(R.bn_eval_fwd(x, gamma, beta, rm, rv, r, relu, C.EPS), y) <= 1e-12
    assert C.err_max(R.channel_sum(x), x.transpose(0, 1).reshape(5, -1).sum(1)) <= 1e-13


@pytest.mark.parametrize("shape,nup", [((2, 3, 4, 4), 1), ((2, 4, 12, 20), 2)])
def test_pool_matches_aten_f64(shape, nup):
    _, (x, gamma, beta, rm, rv, _, _) = _small(shape, False)
    N, C_, H, W = shape
    ref = R.bn_relu_pool_fwd(x, gamma, beta, C.EPS, C.MOMENTUM, nup, rm, rv)
    xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    rm2, rv2 = rm.clone(), rv.clone()
    for _ in range(nup):
        y = F.batch_norm(xa, rm2, rv2, ga, ba, True, C.MOMENTUM, C.EPS)
    pooled, flat = F.max_pool2d(F.relu(y), 3, 2, 1, return_indices=True)
    assert C.err_max(ref.pooled, pooled) <= 1e-12
    assert torch.equal(ref.idx, C.byte_from_flat(flat, H, W))           # relu zeroes half the map: many exact ties
    assert torch.equal(R.argmax_position(ref.idx, H, W), flat)
    assert C.err_max(ref.bn.rm, rm2) <= 1e-12 and C.err_max(ref.bn.rv, rv2) <= 1e-12
    dpool = torch.randn(pooled.shape, generator=torch.Generator().manual_seed(5), dtype=F64)
    pooled.backward(dpool)
    bwd = R.bn_relu_pool_bwd(dpool, ref.idx, x, ref.bn.mean, ref.bn.invstd, gamma, ref.bn.pre > 0)
    assert C.err_max(bwd.dx, xa.grad) <= 1e-11
    assert C.err_max(bwd.dgamma, ga.grad) <= 1e-11 and C.err_max(bwd.dbeta, ba.grad) <= 1e-11


def test_first_maximum_on_planted_ties():
    a = torch.zeros(1, 1, 4, 4, dtype=F64)
    a[0, 0, 1, 1] = a[0, 0, 1, 2] = a[0, 0, 2, 1] = 3.0                # three equal maxima in the window of pooled (1, 1)
    a[0, 0, 0, 3] = a[0, 0, 1, 3] = 2.0
    cand = R.pool_candidates(a)
    best, idx = R.first_max(cand)
    # pooled (0, 0): rows -1..1, cols -1..1 -> (1, 1) is candidate ky 2, kx 2;  (1, 1): rows 1..3, cols 1..3 -> (1, 1) is ky 0, kx 0
    assert idx[0, 0].tolist() == [[8, 6], [2, 0]] and best[0, 0].tolist() == [[3.0, 3.0], [3.0, 3.0]]
    z = torch.zeros(1, 1, 4, 4, dtype=F64)                              # all equal: the first candidate INSIDE the map
    assert R.first_max(R.pool_candidates(z))[1][0, 0].tolist() == [[4, 3], [1, 0]]
    _, flat = F.max_pool2d(a, 3, 2, 1, return_indices=True)
    assert torch.equal(C.byte_from_flat(flat, 4, 4), idx)
    back = R.scatter_pooled(torch.ones(1, 1, 2, 2, dtype=F64), idx, 4, 4)      # all four windows picked input (1, 1)
    assert back[0, 0, 1, 1] == 4.0 and back.sum() == 4.0


def test_groups_update_the_running_statistics_in_order():
    inp = C.train_inputs((6, 5, 7, 9), False, groups=3)
    x, gamma, beta, rm, rv = (t.double() for t in (inp.x, inp.gamma, inp.beta, inp.rm, inp.rv))
    outs, rm3, rv3 = R.grouped_fwd(R.bn_train_fwd, 3, x, gamma, beta, rm, rv, relu=False, eps=C.EPS, momentum=C.MOMENTUM, n_updates=2)
    rm2, rv2 = rm.clone(), rv.clone()
    for g in range(3):
        for _ in range(2):
            y = F.batch_norm(x[2 * g:2 * g + 2], rm2, rv2, gamma, beta, True, C.MOMENTUM, C.EPS)
        assert C.err_max(outs[g].y, y) <= 1e-12
    assert C.err_max(rm3, rm2) <= 1e-12 and C.err_max(rv3, rv2) <= 1e-12
    means = torch.stack([o.mean for o in outs])
    assert float((means[1] - means[0]).abs().min()) > 2.0               # the groups are far apart


# ------------------------------------------------------------------------------------------- 2. launch paths
def test_mirrored_lines_stand_in_the_source():
    with open(os.path.join(ROOT, C.BN_HIP)) as f:
        text = f.read()
    for key, line in C.SOURCE_LINES.items():
        assert line in text, f"{key}: bn.hip changed; update bn_cases.SOURCE_LINES, its mirror and the cases"
    assert text.count(C.SOURCE_LINES["fold4"]) == 2 and text.count(C.SOURCE_LINES["fold1"]) == 3
    assert text.count(C.SOURCE_LINES["gx"]) == 3


@pytest.mark.parametrize("shape", list(C.TRAIN_CASES) + list(C.FOLD_CASES))
def test_train_cases_take_their_paths(shape):
    N, C_, H, W = shape
    claim = dict({**C.TRAIN_CASES, **C.FOLD_CASES}[shape])
    L = C.launch(N, C_, H * W)
    count = claim.pop("count", None)
    if count is not None:
        assert N * H * W == count
    for k, v in claim.items():
        assert getattr(L, k) == v, (shape, k, getattr(L, k), v)
    if shape in C.TRAIN_CASES:
        assert not L.folds                       # only the fold cases reach a fold below the last one
    if "strides" not in claim:
        assert not L.strides


def test_fold_needs_the_large_cases():
    # a fold below the final one needs more than 8192 elements per chunk, a chunk that long needs N * C * HW >= 2048 * 8193
    for N, C_, HW in ((1, 1, 8193 * 2048 - 1), (2, 1024, 8192), (1, 64, 262144)):
        L = C.launch(N, C_, HW)
        assert L.folds == (L.chunk > 8192)
    assert min(N * C_ * H * W for N, C_, H, W in C.FOLD_CASES) >= 2048 * 8193


def test_pool_cases_take_their_paths():
    L = C.pool_launch(2, 3, 4, 4)
    assert (L.tile_rows, L.tile_cols, L.bands, L.stats.CH, L.pooled.CH) == (1, 1, 1, 1, 1) and L.tile_col_short == 62
    L = C.pool_launch(2, 4, 260, 64)
    assert L.OH == 130 and L.RB == 32 and L.bands == 5 and L.band_short == 30
    assert L.tile_rows == 9 and L.tile_row_short == 14 and L.OW == 32 and L.tile_cols == 1 and L.tile_col_short == 32
    assert (L.pooled.CH, L.pooled.chunk, L.pooled.short) == (2, 2080, 0) and (L.stats.CH, L.stats.chunk) == (8, 2080)
    L = C.pool_launch(1, 2, 4, 6152)
    assert (L.pooled.CH, L.pooled.chunk, L.pooled.short) == (3, 2051, 1) and L.OW == 3076
    assert L.tile_cols == 49 and L.tile_col_short == 60 and L.RB == 8 and L.bands == 1
    assert L.OW % 2 == 0 and L.OW // 2 == 1538               # the last 2-column unit has no right neighbour
    L = C.pool_launch(2, 16, 64, 128)                          # one group of the pose-stem configuration
    assert (L.stats.CH, L.stats.chunk, L.stats.stats) == (4, 2048, "float4") and L.pooled.CH == 1 and L.bands == 4


def test_special_eval_group_and_sum_cases_take_their_paths():
    N, C_, H, W = C.SPECIAL_SHAPE
    L = C.launch(N, C_, H * W)
    assert (L.CH, L.chunk, L.stats) == (4, 2052, "float4")
    L = C.launch(2, 3, 8 * 1026)                               # one group of 4x3x8x1026
    assert (L.CH, L.chunk, L.stats) == (4, 2052, "float4")
    assert C.launch(1, 2, 4 * 16385).strides and not C.launch(3, 5, 63).strides
    assert [C.chunking(N, C_, H * W)[0] for N, C_, H, W in C.CHANNEL_SUM_CASES] == [4, 3, 1, 1]
    assert C.launch(16, 128, 93 * 89).iters == 33


def test_workspace_queries_match_the_mirror():
    L = _lib.lib()
    shapes = list(C.TRAIN_CASES) + list(C.FOLD_CASES) + [c[0] for c in C.POOL_CASES.values()] + [(7, 300, 1, 5000), (1, 1, 1, 1 << 20)]
    for N, C_, H, W in shapes:
        assert L.fn["jp_bn_ws_doubles"](N, C_, H * W) == C.bn_ws_doubles(N, C_, H * W), (N, C_, H, W)
        assert L.fn["jp_channel_sum_ws_floats"](N, C_, H * W) == C.channel_sum_ws_floats(N, C_, H * W), (N, C_, H, W)
    for shape, groups, _, _ in C.POOL_CASES.values():
        N, C_, H, W = shape
        assert L.fn["jp_bn_relu_pool_bwd_ws_doubles"](N // groups, C_, H, W) == C.pool_bwd_ws_doubles(N // groups, C_, H, W)
    assert C.bn_ws_doubles(1, 2, 4 * 16385) == 2 * 2 * 32 and C.pool_bwd_ws_doubles(1, 2, 4, 6152) == 2 * 2 * 3 + 2


# ------------------------------------------------------------------------------------------- 3. masks
@pytest.mark.parametrize("shape", list(C.TRAIN_CASES) + list(C.FOLD_CASES))
def test_ambiguous_gate_share(shape):
    for mode in (("relu",) if shape in C.FOLD_CASES else ("relu", "relu+res")):
        ref = C.train_reference(shape, mode)
        print(f"{shape} {mode}: ambiguous gates {ref.amb_share:.2e}")
        assert ref.amb_share <= C.MASK_CAP
        assert 0.2 < float((ref.pre > 0).double().mean()) < 0.8          # both sides of the gate are there


@pytest.mark.parametrize("name", list(C.POOL_CASES) + list(C.GROUP_CASES))
def test_ambiguous_window_share(name):
    if name in C.GROUP_CASES:
        shape, groups = C.GROUP_CASES[name]
        for mode in ("relu", "relu+res"):
            assert C.train_reference(shape, mode, groups).amb_share <= C.MASK_CAP
        return
    ref = C.pool_reference(name)
    ties = float((ref.cand == ref.cand.amax(0)).sum(0).gt(1).double().mean())
    print(f"pool {name}: ambiguous windows {ref.win_share:.2e}, ambiguous gates {ref.amb_share:.2e}, windows with an exact tie {ties:.3f}")
    assert ref.win_share <= C.MASK_CAP and ref.amb_share <= C.MASK_CAP
    assert ties > 0.01                                                    # the first-maximum rule decides a good share of the windows
    # with the reference's own decisions the figures are those of the reference against itself: nothing is flagged
    got = dict(y=ref.pooled.float(), idx=ref.idx)
    _, wrong_idx, wrong_gate = C.pool_backward(ref, got["y"], got["idx"])
    assert wrong_idx == 0 and wrong_gate == 0


def test_the_checks_would_notice_a_wrong_argmax_or_gate():
    ref = C.pool_reference("2x3x4x4")
    other = (ref.idx + 1) % 9
    assert C.pool_backward(ref, ref.pooled.float(), other)[1] > 0
    assert C.pool_backward(ref, torch.zeros_like(ref.pooled).float(), ref.idx)[2] > 0        # every gate closed
    r = C.train_reference((3, 5, 7, 9), "relu")
    assert C.train_backward(r, torch.ones_like(r.y))[1] > 0


# ------------------------------------------------------------------------------------------- 4. bars from the fp32 evaluation's error
def _oracle_errors():
    e = {k: 0.0 for k in C.ORACLE_ERR}
    per_case = []

    def up(figs, case):
        for label, v, key in figs:
            e[key] = max(e[key], v)
            per_case.append((key, case, v))

    for shape in C.TRAIN_CASES:
        for mode in C.MODES:
            ref = C.train_reference(shape, mode)
            for nup in (1, 2):
                figs, wrong = C.train_figures(ref, C.train_oracle(ref, nup), nup)
                assert wrong == 0, (shape, mode)
                up(figs, (shape, mode, nup))
    for shape in C.FOLD_CASES:
        ref = C.train_reference(shape, "relu")
        figs, wrong = C.train_figures(ref, C.train_oracle(ref, 1), 1)
        assert wrong == 0, shape
        up(figs, (shape, "relu", 1))
    for name, (shape, groups) in C.GROUP_CASES.items():
        for mode, nup in C.GROUP_RUNS:
            ref = C.train_reference(shape, mode, groups)
            figs, wrong = C.train_figures(ref, C.train_oracle(ref, nup), nup)
            assert wrong == 0, name
            up(figs, (name, mode, nup))
    for name, (shape, groups, nup, _) in C.POOL_CASES.items():
        ref = C.pool_reference(name)
        figs, wrong_idx, wrong_gate = C.pool_figures(ref, C.pool_oracle(ref, nup), nup)
        assert wrong_idx == 0 and wrong_gate == 0, name
        up(figs, ("pool " + name, "", nup))
    return e, per_case


def test_bars_follow_from_the_oracle_error():
    measured, per_case = _oracle_errors()
    for k, case, v in per_case:
        print(f"{k:14s} {str(case):44s} fp32 evaluation error {v:.3e}")
    for k, v in measured.items():
        print(f"{k:14s} fp32 evaluation error {v:.3e}  recorded {C.ORACLE_ERR[k]:.2e}  bar {C.BARS[k]:.0e}")
    for k, v in measured.items():
        # the recorded figures reproduce (25 % of room for another CPU's vector width and libm)
        assert v <= 1.25 * C.ORACLE_ERR[k], k
        if k not in ("dgamma", "dbeta", "dgamma_max", "dbeta_max"):       # (those depend on the order in which ATen sums a channel)
            assert v >= 0.25 * C.ORACLE_ERR[k], k          # nor is a recorded figure, and so a bar, far above what is measured
    assert set(C.BARS) == set(C.ORACLE_ERR) == set(C.FORMER_BARS)
    for k, bar in C.BARS.items():
        rule = C.round_up_1sig(8 * C.ORACLE_ERR[k]) if C.ORACLE_ERR[k] > 0 else 0.0
        if C.FORMER_BARS[k] is not None and rule > C.FORMER_BARS[k]:
            assert k in C.BAR_NOTES and bar == C.FORMER_BARS[k], k    # never looser than tests/test_kernels_gpu.py
        else:
            assert bar == pytest.approx(rule, rel=1e-9), k


# ------------------------------------------------------------------------------------------- 5. derived bounds, special inputs, timing
def test_special_channels_are_what_they_claim():
    for name, kinds in C.SPECIAL_TENSORS.items():
        ref = C.special_reference(name)
        for c, kind in enumerate(kinds):
            x = ref.inp.x[:, c].double()
            b = C.special_bounds(ref, c)
            rel = abs(float(ref.mean[0, c])) / max(float(ref.var[0, c]) ** 0.5, 1e-300)
            print(f"{name}[{c}] {kind:8s} mean {float(ref.mean[0, c]):10.4f} var {float(ref.var[0, c]):.4e} |mean|/std {rel:.3g} "
                  f"var bound {b.var_bound:.3e} rho {b.rho:.3e}")
            if kind in C.SPECIAL_VALUES:
                assert float(ref.var[0, c]) == 0.0 and bool((x == x[0, 0, 0]).all())        # two-pass: exactly 0 in float64
                assert float(ref.invstd[0, c]) == pytest.approx(C.EPS32 ** -0.5, rel=1e-15)
                assert bool((ref.y[:, c] == float(ref.inp.beta[c])).all())
            elif kind.startswith("offset"):
                assert 1800 < rel < 2200
            else:
                assert rel < 1 and b.rho < 1e-4               # an ordinary channel: the derived bound is far below the measured bars' scale
    assert float(torch.tensor(3.3, dtype=torch.float32)) != 3.3 and float(torch.tensor(0.25, dtype=torch.float32)) == 0.25


def test_channel_sum_bound_notices_a_dropped_element():
    for shape in C.CHANNEL_SUM_CASES[:3]:
        x, out0 = C.channel_sum_inputs(shape)
        _, bound = C.channel_sum_bound(x, None)
        typical = float(x.abs().median())
        assert float(bound.max()) < 0.1 * typical, shape              # leaving one typical element out is 10 bounds away


def test_references_build_in_seconds():
    for fn, args in ((C.train_reference, ((16, 128, 96, 96), "relu")), (C.train_reference, ((16, 128, 93, 89), "relu")),
                     (C.train_reference, ((8, 128, 64, 64), "relu+res")), (C.pool_reference, ("4x16x64x128 g2",))):
        fn.cache_clear()
        t = time.perf_counter()
        fn(*args)
        dt = time.perf_counter() - t
        print(f"{fn.__name__}{args}: {dt:.2f} s")
        assert dt < 15.0
