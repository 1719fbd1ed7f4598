"""Batched depth scoring (csrc/evalmetrics.hip::jp_depth_eval_batch, core/evaluation.py::eval_depth_batch,
apis/inference.py::evaluate_depth_lidar) against the per-image chain it restates, core/evaluation.py::eval_depth.

B = 3, disp (1,1,24,80) each, ground truth 37 x 124 with about 30 % zeros; item 1 has no valid pixel inside the Garg crop, items 0
and 2 have an even and an odd number of valid pixels (both branches of np.median).

Where the bounds come from: the batch performs the same float32 operations per pixel, so the valid count, both medians (exact order
statistics), hence `scale`, and the a1 / a2 / a3 counts must be EQUAL.  The four remaining sums add the same non-negative float64
terms in another order (eval_depth merges its partial sums with atomics, in arrival order): two orders of a sum of n non-negative
doubles differ by at most 2 n 2^-53 relative, and rmse / rmse_log (square roots) by half of that.
"""
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import synthetic as syn                                     # noqa: E402
from jperceiver_amd._lib import call, lib                                       # noqa: E402
from jperceiver_amd.apis import evaluate_depth, evaluate_depth_lidar            # noqa: E402
from jperceiver_amd.core import evaluation as ev                                # noqa: E402
from jperceiver_amd.model import MONO                                           # noqa: E402
from oracle import jp_oracle as J                                               # noqa: E402

DEV = "cuda"
B, h, w, H, W = 3, 24, 80, 37, 124
EXACT = ("n_valid", "scale", "a1", "a2", "a3")
SUMMED = ("abs_rel", "sq_rel", "rmse", "rmse_log")
_CACHE = {}


def data():
    """(disp (3,1,24,80), gt (3,37,124)) on the device, and eval_depth's dict per item -- computed once"""
    if not _CACHE:
        rng = np.random.default_rng(7)
        disp = rng.uniform(0.02, 0.9, size=(B, 1, h, w)).astype(np.float32)
        gt = rng.uniform(0.5, 85.0, size=(B, H, W)).astype(np.float32)       # some beyond the 80 m mask
        gt[rng.uniform(size=gt.shape) < 0.3] = 0.0
        y0, y1, x0, x1 = ev._garg_crop(H, W)
        gt[1, y0:y1, x0:x1] = 0.0                                               # item 1: returns outside the crop only

        def n_valid(g):
            c = g[y0:y1, x0:x1]
            return int(((c > ev.MIN_DEPTH) & (c < ev.MAX_DEPTH)).sum())

        for item, parity in ((0, 0), (2, 1)):
            if n_valid(gt[item]) % 2 != parity:
                ys, xs = np.nonzero((gt[item, y0:y1, x0:x1] > ev.MIN_DEPTH) & (gt[item, y0:y1, x0:x1] < ev.MAX_DEPTH))
                gt[item, y0 + ys[0], x0 + xs[0]] = 0.0
        assert n_valid(gt[0]) % 2 == 0 and n_valid(gt[2]) % 2 == 1 and n_valid(gt[1]) == 0 and n_valid(gt[0]) > 500
        _CACHE["disp"], _CACHE["gt"] = torch.from_numpy(disp).to(DEV), torch.from_numpy(gt).to(DEV)
        for stereo in (False, True):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                _CACHE[stereo] = [ev.eval_depth(_CACHE["disp"][b:b + 1], _CACHE["gt"][b], stereo_scale=stereo) for b in range(B)]
    return _CACHE


def compare(got, ref):
    n = ref["n_valid"]
    assert got.keys() == ref.keys()
    if n == 0:
        assert got["n_valid"] == 0 and all(math.isnan(got[k]) for k in got if k != "n_valid")
        return
    for k in EXACT:
        assert got[k] == ref[k], (k, got[k], ref[k])
    tol = 2.0 * n * 2.0 ** -53
    for k in SUMMED:
        rel = abs(got[k] - ref[k]) / abs(ref[k])
        print(f"n {n} {k}: {got[k]!r} vs {ref[k]!r}, rel {rel:.2e} (bound {tol:.2e})")
        assert rel <= tol, k


@pytest.mark.parametrize("stereo", [False, True])
def test_batch_equals_the_per_image_chain(stereo):
    d = data()
    with pytest.warns(RuntimeWarning):                                          # item 1: the empty set, as eval_depth reports it
        got = ev.eval_depth_batch(d["disp"], d["gt"], stereo_scale=stereo)
    assert len(got) == B
    for b in range(B):
        compare(got[b], d[stereo][b])
    assert got[0]["n_valid"] % 2 == 0 and got[2]["n_valid"] % 2 == 1 and got[1]["n_valid"] == 0
    if stereo:
        assert got[0]["abs_rel"] != d[False][0]["abs_rel"]                      # the fixed factor was used


def _raw(disp, gt, fixed_scale=0.0, poison=False):
    y0, y1, x0, x1 = ev._garg_crop(H, W)
    nbytes = lib().fn["jp_depth_eval_batch_ws_bytes"](B, H, W)
    ws = torch.full((nbytes,), 0xFF if poison else 0, dtype=torch.uint8, device=DEV)
    sums = torch.full((B, 8), float("nan"), dtype=torch.float64, device=DEV)
    med = torch.full((B, 4), float("nan"), dtype=torch.float32, device=DEV)
    call("jp_depth_eval_batch", disp, gt, B, h, w, H, W, y0, y1, x0, x1, ev.MIN_DEPTH, float(ev.MAX_DEPTH), 0.1, 100.0, fixed_scale,
         sums, med, ws)
    return sums, med


def test_medians_and_counts_equal_the_existing_kernels_bit_for_bit():
    d = data()
    disp, gt = d["disp"], d["gt"]
    sums, med = _raw(disp, gt, poison=True)
    y0, y1, x0, x1 = ev._garg_crop(H, W)
    for b in range(B):                                                          # eval_depth's own launches, item by item
        scaled, res = torch.empty_like(disp[b:b + 1]), torch.empty((1, 1, H, W), device=DEV)
        call("jp_affine", disp[b:b + 1].contiguous(), scaled, h * w, 1.0 / 0.1 - 1.0 / 100, 1.0 / 100)
        call("jp_bilinear_fwd", scaled, res, 1, h, w, H, W)
        pred, valid = torch.empty((H, W), device=DEV), torch.empty((H, W), device=DEV, dtype=torch.uint8)
        call("jp_depth_eval_prepare", res, gt[b], pred, valid, H, W, y0, y1, x0, x1, ev.MIN_DEPTH, float(ev.MAX_DEPTH))
        mg, mp = torch.empty(2, device=DEV), torch.empty(2, device=DEV)
        call("jp_masked_median", gt[b], valid, H * W, mg)
        call("jp_masked_median", pred, valid, H * W, mp)
        s = torch.empty(8, device=DEV, dtype=torch.float64)
        call("jp_depth_errors", gt[b], pred, valid, H * W, mg, mp, 0.0, ev.MIN_DEPTH, float(ev.MAX_DEPTH), s)
        ref_med = torch.cat([mg, mp]).view(torch.int32)
        assert torch.equal(med[b].view(torch.int32), ref_med), (b, med[b], mg, mp)          # bit patterns: NaN == NaN for item 1
        assert int(mg[0]) == int(valid.sum())
        assert torch.equal(sums[b, [0, 1, 2, 7]], s[[0, 1, 2, 7]])
        n = float(s[7])
        if n:
            assert float(((sums[b, 3:7] - s[3:7]).abs() / s[3:7]).max()) <= 2.0 * n * 2.0 ** -53
        else:
            assert float(sums[b].abs().max()) == 0.0


def test_two_runs_are_bit_identical():
    d = data()
    first = _raw(d["disp"], d["gt"])
    for poison in (True, False, True):
        again = _raw(d["disp"], d["gt"], poison=poison)
        assert torch.equal(first[0].view(torch.int64), again[0].view(torch.int64))
        assert torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))


def _model(HW=256):
    opt = J.default_opt(frame_ids=[0, -1, 1], imgs_per_gpu=1, height=HW, width=HW, occ_map_size=HW // 4, type="static",
                        split="odometry")
    model = MONO.module_dict["Baseline"](opt)
    model.load_state_dict(syn.synth_state_dict(model.state_dict(), seed=3, bn_stats=True))
    return model.to(DEV).eval()


def test_evaluate_depth_lidar_equals_evaluate_depth_on_the_same_maps():
    model = _model()
    inp = syn.make_batch(1, 256, 256, [0, -1, 1], 64, (375, 1242), "odometry", seed=9)
    inp = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    Hg, Wg, n = 94, 311, 20000
    f = 180.0
    K = np.array([[f, 0, 152.4, 11.2], [0, f, 43.2, 0.05], [0, 0, 1, 0.003]])
    P = K @ np.array([[0.0, -1, 0, -0.004], [0, 0, -1, -0.076], [1, 0, 0, -0.272], [0, 0, 0, 1]])
    scans = []
    for seed in (21, 22):
        rng = np.random.default_rng(seed)
        x = rng.uniform(-5.0, 90.0, n)
        scans.append(np.stack([x, x * rng.uniform(-1.0, 1.0, n), x * rng.uniform(-0.3, 0.3, n), rng.uniform(0, 1, n)], 1)
                     .astype(np.float32))
    gts = ev.lidar_depth_maps(scans, P, (Hg, Wg)).float()
    assert int((gts[0] > 0).sum()) > 3000
    ref_err, ref_med, ref_std = evaluate_depth(model, [inp, inp], [gts[0], gts[1]])
    for batch in (8, 1):                                                        # one group of two, two groups of one
        err, med, std = evaluate_depth_lidar(model, [inp, inp], scans, (P, (Hg, Wg)), batch=batch)
        assert med == ref_med and std == ref_std
        for k in ("a1", "a2", "a3"):
            assert err[k] == ref_err[k], k
        for k in SUMMED:
            assert abs(err[k] - ref_err[k]) <= 2.0 * Hg * Wg * 2.0 ** -53 * abs(ref_err[k]), (k, err[k], ref_err[k])
    with pytest.raises(RuntimeError):
        evaluate_depth_lidar(model.train(), [inp], scans[:1], (P, (Hg, Wg)))
