"""KITTI odometry evaluation on the device (csrc/odometry.hip, core/evaluation.py::eval_odometry, apis/inference.py).

Expected values come from the reference's own toolkit (tests/golden/odometry_eval_*.npz, written by tools/make_odometry_golden.py:
kittiOdomEval, align_trajectory, umeyama_alignment, plot_kitti on the ground truth of sequences 04 and 10 and seeded perturbations of
it) and from host float64 numpy.  Where the bounds come from:

* chain: atol = 1e-9 max(1, max |t|) against the host's sequential float64 chain with np.linalg.inv.  A float64 product chain of
  4661 steps re-associated by a scan moves by about n eps 10 = 5e-12 relative; the bound is 200 x that and five orders below the
  5e-4 a transpose "inverse" of float32 rotations costs over such a sequence.
* segment table: the fixture guarantees (cond_min_dist_gap >= 1e-6 m) that no re-ordering of the float64 prefix sum can move a
  last_frame, so those are compared exactly and no row may be missing; first_frame / len / speed 1e-12; t_err/len rtol 1e-9;
  r_err/len rtol 1e-6: every segment's rotation error is >= 1e-3 rad (cond_min_rot_err), where an error of 1e-13 in the trace moves
  acos by <= 1e-10 rad = 1e-7 relative, with a decade of margin.
* moments: rtol 1e-12 of each block's largest magnitude against numpy float64.  Umeyama (R, t, c): 1e-9, on sequence 10 only --
  sequence 04 is almost a straight line (second singular value 1.5e-5 of the first), its rotation is ill-conditioned; it is used for
  the scale-only modes.  Aligned trajectories: rtol 1e-9, atol 1e-9 x the trajectory's extent.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd.apis import (chain_poses, chain_poses_device, odometry, odometry_device, evaluate_odometry,      # noqa: E402
                                 pair_transforms, pose_nets_from_checkpoint)
from jperceiver_amd.core import evaluation as ev                                                                    # noqa: E402

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def gold(seq):
    if seq not in _CACHE:
        d = dict(np.load(os.path.join(GOLD, f"odometry_eval_{seq}.npz")))
        if seq == "10":
            d.update(np.load(os.path.join(GOLD, "odometry_eval_10_aligned.npz")))
        _CACHE[seq] = d
    return _CACHE[seq]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def extent(traj):
    p = traj[:, [3, 7, 11]]
    return float(max(1.0, (p.max(0) - p.min(0)).max()))


# ------------------------------------------------------------------------------------------------------------------ chain
def _rodrigues(v):
    th = np.linalg.norm(v)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.identity(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def transforms():
    """4661 seeded float32 transforms: rotations <= 0.1 rad, translations about 1, row 3 = (0,0,0,1)"""
    if "T" not in _CACHE:
        rng = np.random.default_rng(11)
        T = np.tile(np.identity(4), (4661, 1, 1))
        for k in range(4661):
            v = rng.standard_normal(3)
            T[k, :3, :3] = _rodrigues(v / np.linalg.norm(v) * rng.uniform(1e-3, 0.1))
            T[k, :3, 3] = rng.standard_normal(3)
        _CACHE["T"] = T.astype(np.float32)
    return _CACHE["T"]


def host_chain(T, invert):
    """the sequential float64 chain of chain_poses (np.linalg.inv), or without the inverse"""
    T = np.asarray(T, dtype=np.float64)
    g = np.identity(4)
    out = [g[:3].reshape(12)]
    for k in range(T.shape[0]):
        g = g @ (np.linalg.inv(T[k]) if invert else T[k])
        out.append(g[:3].reshape(12))
    return np.stack(out)


def chain_bound(ref):
    return 1e-9 * max(1.0, float(np.abs(ref[:, [3, 7, 11]]).max()))


@pytest.mark.parametrize("invert", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1023, 1025, 4661])
def test_chain_matches_the_sequential_float64_chain(n, invert):
    T = transforms()[:n]
    ref = host_chain(T, invert)
    got = chain_poses_device(torch.from_numpy(T).to(DEV), invert=invert)
    assert got.shape == (n + 1, 12) and got.dtype == torch.float64 and got.is_cuda
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"chain n={n} invert={invert}: max err {err:.3e}, bound {chain_bound(ref):.3e}")
    assert err <= chain_bound(ref)
    if invert:
        np.testing.assert_array_equal(ref, chain_poses(T))        # the reference of this test IS the existing host function


def test_chain_uses_the_general_inverse_not_the_transpose():
    T = transforms()[:300].copy()
    T[:, 1, :3] *= np.float32(1.0 + 1e-4)                         # rotations 1e-4 off orthonormal
    ref = host_chain(T, True)
    got = chain_poses_device(torch.from_numpy(T).to(DEV)).cpu().numpy()
    err = float(np.abs(got - ref).max())
    Tt = T.astype(np.float64)
    Rt = np.transpose(Tt[:, :3, :3], (0, 2, 1))
    Tt[:, :3, 3] = -np.einsum("kij,kj->ki", Rt, Tt[:, :3, 3])
    Tt[:, :3, :3] = Rt
    wrong = float(np.abs(host_chain(Tt, False) - ref).max())
    print(f"general inverse: err {err:.3e}, bound {chain_bound(ref):.3e}; a transpose inverse would be off by {wrong:.3e}")
    assert err <= chain_bound(ref)
    assert wrong > 1e4 * chain_bound(ref)                         # the case does tell the two apart


def test_chain_known_answer_row3_ignored_and_bit_equal_runs():
    Tt = np.tile(np.identity(4, dtype=np.float32), (3, 1, 1))
    Tt[:, 0, 3] = [1.0, 2.0, 3.0]
    out = chain_poses_device(torch.from_numpy(Tt).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(out[:, 3], [0.0, -1.0, -3.0, -6.0], atol=1e-12)
    np.testing.assert_array_equal(out[:, [0, 5, 10]], np.ones((4, 3)))
    T = transforms().copy()
    a = chain_poses_device(torch.from_numpy(T).to(DEV))
    b = chain_poses_device(torch.from_numpy(T).to(DEV))
    assert torch.equal(a, b)
    T[:, 3, :] = np.float32(7.0)                                  # row 3 is not read: taken as (0,0,0,1)
    assert torch.equal(chain_poses_device(torch.from_numpy(T).to(DEV)), a)
    assert chain_poses_device(torch.empty((0, 4, 4), device=DEV)).cpu().tolist() == [[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]
    with pytest.raises(ValueError):
        chain_poses_device(torch.zeros((3, 3, 4), device=DEV))


# ------------------------------------------------------------------------------------------------------------------ segment table
def check_table(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_allclose(got[:, [0, 3, 4]], want[:, [0, 3, 4]], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[:, 2], want[:, 2], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=1e-6, atol=0)


def check_averages(got, keys, vals, present):
    assert [float(k) for k in got] == [float(k) for k in keys]
    for k, v, p in zip(got, vals, present):
        if not p:
            assert got[k] == []                                   # empty lists sit where the reference has them
        else:
            np.testing.assert_allclose(got[k][0], v[0], rtol=1e-9)
            np.testing.assert_allclose(got[k][1], v[1], rtol=1e-6)


@pytest.mark.parametrize("seq", ["04", "10"])
def test_segment_table_matches_the_toolkit(seq):
    g = gold(seq)
    assert g["cond_min_rot_err"] >= 1e-3 and g["cond_min_dist_gap"] >= 1e-6
    gt, aligned = dev(g["gt"]), dev(g["aligned_umeyama_scale"])
    table, last, dist = ev.odometry_segments(aligned, gt, g["lengths"].tolist(), int(g["step"]))
    np.testing.assert_array_equal(last, g["last_frame"])          # every (start, length), -1 included
    np.testing.assert_allclose(dist, g["dist"], rtol=1e-12, atol=1e-12)
    check_table(table, g["table"])
    # the whole path from the raw prediction: alignment on the device, then the table and the toolkit's averages
    r = ev.eval_odometry(dev(g["pred"]), gt)
    check_table(r["segments"], g["table"])
    assert r["n_segments"] == len(g["table"])
    np.testing.assert_allclose(r["t_err"], g["t_err"], rtol=1e-9)
    np.testing.assert_allclose(r["r_err"], g["r_err"], rtol=1e-6)
    check_averages(r["per_length"], g["per_length_keys"], g["per_length_vals"], g["per_length_present"])
    check_averages(r["per_speed"], g["per_speed_keys"], g["per_speed_vals"], g["per_speed_present"])
    np.testing.assert_allclose([r["distance"], r["max_speed"], r["scale"]], [g["distance"], g["max_speed"], g["umeyama_s_c"]], rtol=1e-12)
    if seq == "04":
        assert all(r["per_length"][ln] == [] for ln in (400, 500, 600, 700, 800)) and r["per_length"][300] != []
    # bit-equal runs
    t2, l2, d2 = ev.odometry_segments(aligned, gt, g["lengths"].tolist(), int(g["step"]))
    assert np.array_equal(t2, table) and np.array_equal(l2, last) and np.array_equal(d2, dist)


def host_segments(gt, pred, lengths, step):
    """calcSequenceErrors from its definition, in numpy on 4x4 matrices with a linear scan for the last frame"""
    def m4(r):
        m = np.identity(4)
        m[:3] = r.reshape(3, 4)
        return m
    pos = gt[:, [3, 7, 11]]
    dist = np.concatenate([[0.0], np.cumsum(np.sqrt(((pos[:-1] - pos[1:]) ** 2).sum(1)))])
    rows = []
    for first in range(0, len(gt), step):
        for ln in lengths:
            hit = np.nonzero(dist[first:] > dist[first] + ln)[0]
            if not len(hit):
                continue
            last = first + int(hit[0])
            dg = np.linalg.inv(m4(gt[first])) @ m4(gt[last])
            dr = np.linalg.inv(m4(pred[first])) @ m4(pred[last])
            e = np.linalg.inv(dr) @ dg
            r = np.arccos(max(min(0.5 * (np.trace(e[:3, :3]) - 1.0), 1.0), -1.0))
            rows.append([first, r / ln, np.linalg.norm(e[:3, 3]) / ln, ln, ln / (0.1 * (last - first + 1.0))])
    return np.asarray(rows).reshape(-1, 5)


def test_step_one_and_a_single_length():
    g = gold("04")
    want = host_segments(g["gt"], g["aligned_umeyama_scale"], [150.0], 1)
    table, last, _ = ev.odometry_segments(dev(g["aligned_umeyama_scale"]), dev(g["gt"]), [150.0], 1)
    assert last.shape == (271, 1) and 100 < len(want) < 271
    assert int((last >= 0).sum()) == len(want) and (last[len(want):] == -1).all()
    check_table(table, want)
    r = ev.eval_odometry(dev(g["pred"]), dev(g["gt"]), lengths=(150,), step=1)
    check_table(r["segments"], want)
    assert list(r["per_length"]) == [150] and r["n_segments"] == len(want)
    # sixteen lengths are the most one call takes
    ev.odometry_segments(dev(g["gt"]), dev(g["gt"]), [10.0 * (i + 1) for i in range(16)], 7)
    with pytest.raises(ValueError):
        ev.odometry_segments(dev(g["gt"]), dev(g["gt"]), [10.0] * 17, 7)


# ------------------------------------------------------------------------------------------------------------------ moments, Umeyama
def host_moments(x12, y12):
    x, y = x12[:, [3, 7, 11]], y12[:, [3, 7, 11]]
    n = len(x)
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    return [mx, my, np.array([(xc ** 2).sum() / n]), (yc.T @ xc / n).reshape(9), np.array([(x * y).sum()]), np.array([(x * x).sum()]),
            np.array([((x - y) ** 2).sum()])]


@pytest.mark.parametrize("seq", ["04", "10"])
def test_moments_match_numpy(seq):
    g = gold(seq)
    for x, y in ((g["pred"], g["gt"]), (g["gt"], g["aligned_umeyama_scale"]), (g["gt"][:257], g["pred"][:257]), (g["gt"][:1], g["pred"][:1])):
        got = ev.traj_moments(dev(x), dev(y))
        assert got.shape == (19,)
        o = 0
        for block in host_moments(x, y):
            np.testing.assert_allclose(got[o:o + len(block)], block, rtol=0, atol=1e-12 * max(np.abs(block).max(), 1e-300))
            o += len(block)
        assert o == 19
        assert np.array_equal(ev.traj_moments(dev(x), dev(y)), got)           # bit-equal runs


def test_umeyama_parameters_match_the_reference():
    g = gold("10")
    assert g["cond_sv_ratio"] >= 1e-3 and g["cond_sv_ratio_rebased"] >= 1e-3
    for tag, ws in (("s", True), ("n", False)):
        R, t, c = ev.umeyama_alignment(dev(g["pred"]), dev(g["gt"]), ws)
        assert R.dtype == np.float64 and R.shape == (3, 3) and t.shape == (3,)
        np.testing.assert_allclose(R, g[f"umeyama_{tag}_R"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(t, g[f"umeyama_{tag}_t"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(c, g[f"umeyama_{tag}_c"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-12)
    _, _, c = ev.umeyama_alignment(dev(gold("04")["pred"]), dev(gold("04")["gt"]), True)      # the scale is well conditioned on a line too
    np.testing.assert_allclose(c, gold("04")["umeyama_s_c"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("seq,mode", [("10", "umeyama_scale"), ("10", "scale"), ("10", "scale_7dof"), ("10", "7dof"), ("10", "6dof"),
                                      ("04", "umeyama_scale"), ("04", "scale"), ("04", "scale_7dof")])
def test_alignment_modes_match_the_reference(seq, mode):
    g = gold(seq)
    pred, gt = dev(g["pred"]), dev(g["gt"])
    got, prm = ev.align_poses(pred, gt, mode)
    want = g["aligned_" + mode]
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == want.shape
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-9, atol=1e-9 * extent(g["gt"]))
    ref = g["gt"] if mode == "umeyama_scale" else g["gt_rebased"]
    np.testing.assert_allclose(prm["reference"].cpu().numpy(), ref, rtol=1e-9, atol=1e-9 * extent(g["gt"]))
    assert torch.equal(ev.align_poses(pred, gt, mode)[0], got)                # bit-equal runs, transform kernel included
    assert torch.equal(ev.align_poses(pred, gt, "none")[0], pred)
    with pytest.raises(ValueError):
        ev.align_poses(pred, gt, "sim3")


# ------------------------------------------------------------------------------------------------------------------ properties
def test_a_perfect_prediction_has_no_error():
    g = gold("10")
    r = ev.eval_odometry(dev(g["gt"]), dev(g["gt"]))
    assert r["n_segments"] == 464
    print("pred == gt: max t_err/len %.3e, max r_err/len %.3e, ate %.3e" % (r["segments"][:, 2].max(), r["segments"][:, 1].max(), r["ate"]))
    assert r["segments"][:, 2].max() <= 1e-9 and r["segments"][:, 1].max() <= 1e-6       # acos' floor: sqrt(2 x 1e-15) / 100 m
    assert r["t_err"] <= 1e-9 and r["r_err"] <= 1e-6 and abs(r["scale"] - 1.0) <= 1e-12 and r["ate"] <= 1e-9 * extent(g["gt"])


def test_7dof_recovers_a_similarity():
    g = gold("10")
    rng = np.random.default_rng(3)
    v = rng.standard_normal(3)
    R, t, c = _rodrigues(v / np.linalg.norm(v) * 0.7), rng.standard_normal(3) * 50.0, 0.0371
    gt = g["gt"].reshape(-1, 3, 4)
    pred = np.concatenate([R @ gt[:, :, :3], (c * gt[:, :, 3] @ R.T + t)[:, :, None]], 2).reshape(-1, 12)
    r = ev.eval_odometry(dev(pred), dev(g["gt"]), align="7dof")
    print("7dof: scale rel err %.3e, ate %.3e" % (abs(r["scale"] * c - 1.0), r["ate"]))
    assert abs(r["scale"] * c - 1.0) <= 1e-10
    assert r["ate"] <= 1e-8 * extent(g["gt"])
    assert r["n_segments"] == 464 and r["t_err"] <= 1e-8


def test_the_table_does_not_depend_on_the_scale_of_the_prediction():
    g = gold("10")
    pred = g["pred"].copy()
    pred[:, [3, 7, 11]] *= 7.3
    r = ev.eval_odometry(dev(pred), dev(g["gt"]), align="umeyama_scale")
    check_table(r["segments"], g["table"])
    np.testing.assert_allclose(r["scale"] * 7.3, g["umeyama_s_c"], rtol=1e-12)


def _line(n, spacing=1.0):
    p = np.tile(np.identity(4)[:3].reshape(12), (n, 1))
    p[:, 11] = spacing * np.arange(n)
    return p


def test_edge_cases_short_unequal_and_single_pose():
    short = dev(_line(51))                                         # 50 m: shorter than every length
    with pytest.warns(RuntimeWarning):
        r = ev.eval_odometry(short, short)
    assert r["n_segments"] == 0 and np.isnan(r["t_err"]) and np.isnan(r["r_err"]) and r["segments"].shape == (0, 5)
    assert all(v == [] for v in r["per_length"].values()) and all(v == [] for v in r["per_speed"].values())
    assert r["distance"] == 50.0 and r["max_speed"] == 0.0 and r["ate"] <= 1e-12
    with pytest.raises(ValueError):
        ev.eval_odometry(dev(_line(51)), dev(_line(50)))
    with pytest.raises(ValueError):
        ev.align_poses(dev(_line(51)), dev(_line(50)), "scale")
    with pytest.raises(ValueError):
        ev.eval_odometry(short.float(), short)
    one = dev(_line(1))                                            # n = 1: nothing to align to, nothing to measure
    with pytest.warns(RuntimeWarning):
        r = ev.eval_odometry(one, one, align="none")
    assert r["n_segments"] == 0 and np.isnan(r["t_err"]) and r["distance"] == 0.0 and r["ate"] == 0.0
    assert torch.equal(ev.transform_poses(one, None, 3.0), one)
    assert ev.traj_moments(one, one)[6] == 0.0


# ------------------------------------------------------------------------------------------------------------------ pose nets
def test_odometry_device_matches_the_host_path_and_batches_agree():
    from jperceiver_amd import synthetic as syn
    from jperceiver_amd.model import MONO
    from jperceiver_amd.model.modules import PoseEncoder, PoseDecoder
    from oracle import jp_oracle as J
    opt = J.default_opt(frame_ids=[0, -1, 1], imgs_per_gpu=1, height=256, width=256, occ_map_size=64, type="static", split="odometry")
    model = MONO.module_dict["Baseline"](opt)
    model.load_state_dict(syn.synth_state_dict(model.state_dict(), seed=3, bn_stats=True))
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    enc, dec = PoseEncoder(18, None, 2), PoseDecoder(np.array([64, 64, 128, 256, 512]))
    pose_nets_from_checkpoint({"state_dict": sd, "meta": {}}, enc, dec)
    enc, dec = enc.to(DEV).eval(), dec.to(DEV).eval()
    frames = torch.rand(6, 3, 192, 640, generator=torch.Generator().manual_seed(5)).to(DEV)
    host = odometry(enc, dec, frames)                             # B = 1 pairs, numpy chain
    got = odometry_device(enc, dec, frames, batch=1)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (6, 12)
    assert float(np.abs(got.cpu().numpy() - host).max()) <= chain_bound(host)       # the per-pair kernels are the same
    T1 = pair_transforms(enc, dec, frames, batch=1)
    T4 = pair_transforms(enc, dec, frames, batch=4)               # chunks of 4 and 1
    d = float((T1 - T4).abs().max())
    print(f"B=4 against B=1 transforms: max diff {d:.3e}")
    assert tuple(T4.shape) == (5, 4, 4) and d <= 4e-5             # each is held to 2e-5 of the oracle by test_inference_gpu.py
    gt = _line(6, 60.0)                                           # made up: 60 m per frame -> the 100 m and 200 m segments of frame 0
    r = evaluate_odometry(enc, dec, frames, gt, batch=4, step=1)
    assert {"t_err", "r_err", "segments", "n_segments", "per_length", "per_speed", "distance", "max_speed", "scale", "ate",
            "poses"} <= set(r)
    assert r["n_segments"] > 0 and all(np.isfinite(r[k]) for k in ("t_err", "r_err", "distance", "max_speed", "scale", "ate"))
    assert np.isfinite(r["segments"]).all() and tuple(r["poses"].shape) == (6, 12)
    assert tuple(odometry_device(enc, dec, frames[:1]).shape) == (1, 12)
    with pytest.raises(RuntimeError):
        odometry_device(enc.train(), dec, frames)
