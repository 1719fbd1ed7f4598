#!/usr/bin/env python
"""Generate tests/golden/odometry_eval_*.npz by running the REAL reference's odometry toolkit on the CPU:
mono/tools/kitti_evaluation_toolkit.py (kittiOdomEval), mono/tools/trajectory.py (align_trajectory), mono/tools/geometry.py
(umeyama_alignment) and scripts/plot_kitti.py (the four alignment modes).  The reference is imported at generation time only; no
source of it is copied, and no test reads it.

Usage:  python tools/make_odometry_golden.py /path/to/reference/checkout

Ground truth: the reference's data files mono/datasets/gt_pose/04.txt (271 poses, 394 m, almost a straight line) and 10.txt (1201
poses, 920 m, every length of 100..800 m occurs).  Predicted trajectories: seeded perturbations of the ground truth's relative
motions (global scale 1/29.5, a per-step yaw bias of 2e-4 rad plus noise, translation noise), chained from the identity like
the output of the odometry script.

The generator ASSERTS, and stores under `cond_*`, the conditions the tolerances of tests/test_odometry_eval_gpu.py rest on:
 (a) every segment's rotation error is >= 1e-3 rad (acos is ill-conditioned near 0);
 (b) for every segment dist[last] - dist[first] - len and dist[first] + len - dist[last-1] are >= 1e-6 m (no reordering of a float64
     prefix sum can move a last_frame);
 (c) on sequence 10, where rotations of the alignment are compared, the second singular value of the covariance is >= 1e-3 of the
     first.  Sequence 04 fails this and is used for the scale-only modes and the segment table only.
Files: odometry_eval_04.npz, odometry_eval_10.npz (trajectories, tables, averages, Umeyama parameters) and
odometry_eval_10_aligned.npz (the four aligned trajectories of sequence 10), each below the size of the largest fixture so far.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
LENGTHS = [100, 200, 300, 400, 500, 600, 700, 800]
STEP = 10


def import_reference(ref):
    import importlib.util
    import matplotlib
    matplotlib.use("agg")
    sys.path.insert(0, ref)
    from mono.tools import kitti_evaluation_toolkit as kit
    from mono.tools import trajectory, geometry
    spec = importlib.util.spec_from_file_location("ref_plot_kitti", os.path.join(ref, "scripts", "plot_kitti.py"))
    pk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pk)
    return kit, trajectory, geometry, pk


def yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])


def perturbed(gt, seed):
    """gt: list of 4x4 -> predicted list of 4x4."""
    rng = np.random.default_rng(seed)
    g = np.identity(4)
    out = [g.copy()]
    for k in range(1, len(gt)):
        rel = np.linalg.inv(gt[k - 1]) @ gt[k]
        rel = rel @ yaw(2e-4 + 1e-4 * rng.standard_normal())
        rel[:3, 3] = rel[:3, 3] / 29.5 + (2e-3 / 29.5) * rng.standard_normal(3)
        g = g @ rel
        out.append(g.copy())
    return out


def flat(poses):
    return np.stack([np.asarray(p)[:3].reshape(12) for p in poses]).astype(np.float64)


def avg_dict_to_arrays(d):
    """{key: [t, r] or []} -> keys, (len, 2) array with NaN rows where the list is empty, mask of the non-empty ones"""
    keys = np.asarray(list(d.keys()), dtype=np.float64)
    present = np.asarray([v != [] for v in d.values()])
    vals = np.asarray([v if v != [] else [np.nan, np.nan] for v in d.values()], dtype=np.float64)
    return keys, vals, present


def run_plot_kitti(pk, mode, gt_file, pred_file):
    """the reference's plot_kitti() on two text files, with its plotting call replaced by a capture of the aligned poses"""
    got = {}
    pk.plot_trajectory = lambda all_poses, *a, **k: got.update(all_poses)
    opt = type("Opt", (), dict(seq="10", align=mode, type="learning", outpath="."))()
    pk.plot_kitti(opt, {"GT": [gt_file, "black"], "Ours": [pred_file, "red"]})
    order = sorted(got["Ours"].keys())
    return flat([got["Ours"][i] for i in order]), flat([got["GT"][i] for i in sorted(got["GT"].keys())])


def make(seq, seed, ref, mods, modes):
    kit, trajectory, geometry, pk = mods
    gt_file = os.path.join(ref, "mono", "datasets", "gt_pose", f"{seq}.txt")
    from mono.tools.pose_evaluation_utils import read_kitti_poses_file
    tra_gt = read_kitti_poses_file(gt_file)
    gt = [np.asarray(p, dtype=np.float64) for p in tra_gt.poses_se3]
    pred = perturbed(gt, seed)
    tra_pred = trajectory.PosePath3D(poses_se3=[p.copy() for p in pred])
    out = dict(gt=flat(gt), pred=flat(pred), lengths=np.asarray(LENGTHS, dtype=np.float64), step=np.int64(STEP))

    # ---- kittiOdomEval.eval's path (kitti_evaluation_toolkit.py:571-621)
    tra_corr, r_a, t_a, s_a = trajectory.align_trajectory(tra_pred, tra_gt, correct_only_scale=True, return_parameters=True)
    ev = kit.kittiOdomEval.__new__(kit.kittiOdomEval)
    ev.lengths, ev.num_lengths = LENGTHS, len(LENGTHS)
    poses_result, poses_gt = ev.loadPoseSe3(tra_corr), ev.loadPoseSe3(tra_gt)
    table = ev.calcSequenceErrors(poses_gt, poses_result)
    dist = ev.trajectoryDistances(poses_gt)
    last = np.asarray([[ev.lastFrameFromSegmentLength(dist, f, ln) for ln in LENGTHS] for f in range(0, len(gt), STEP)], dtype=np.int32)
    t_err, r_err = ev.computeOverallErr(table)
    out.update(aligned_umeyama_scale=flat(tra_corr.poses_se3), table=np.asarray(table, dtype=np.float64), last_frame=last,
               dist=np.asarray(dist, dtype=np.float64), t_err=np.float64(t_err), r_err=np.float64(r_err),
               distance=np.float64(ev.distance), max_speed=np.float64(ev.max_speed))
    for name, d in (("per_length", ev.computeSegmentErr(table)), ("per_speed", ev.computeSpeedErr(table))):
        k, v, p = avg_dict_to_arrays(d)
        out[name + "_keys"], out[name + "_vals"], out[name + "_present"] = k, v, p

    # ---- conditions (a) and (b)
    tab = out["table"]
    assert len(tab) == int((last >= 0).sum())
    rot = tab[:, 1] * tab[:, 3]
    out["cond_min_rot_err"] = np.float64(rot.min())
    assert rot.min() >= 1e-3, rot.min()
    d = out["dist"]
    gaps = []
    for si, f in enumerate(range(0, len(gt), STEP)):
        for li, ln in enumerate(LENGTHS):
            lf = last[si, li]
            if lf >= 0:
                gaps += [d[lf] - d[f] - ln, d[f] + ln - d[lf - 1]]
            else:
                gaps.append(d[f] + ln - d[-1])
    out["cond_min_dist_gap"] = np.float64(min(gaps))
    assert min(gaps) >= 1e-6, min(gaps)

    # ---- Umeyama parameters on the raw trajectories (geometry.py), with and without scale
    x, y = tra_pred.positions_xyz.T, tra_gt.positions_xyz.T           # as align_trajectory passes them
    for tag, ws in (("s", True), ("n", False)):
        r, t, c = geometry.umeyama_alignment(x, y, ws)
        out[f"umeyama_{tag}_R"], out[f"umeyama_{tag}_t"], out[f"umeyama_{tag}_c"] = r, t, np.float64(c)
    assert out["umeyama_s_c"] == s_a
    sv = np.linalg.svd(_cov(x, y), compute_uv=False)
    out["cond_sv_ratio"] = np.float64(sv[1] / sv[0])

    # ---- plot_kitti's modes on exact ('%.17e') text copies of the two trajectories
    aligned = {}
    with tempfile.TemporaryDirectory() as tmp:
        gf, pf = os.path.join(tmp, "gt.txt"), os.path.join(tmp, "pred.txt")
        np.savetxt(gf, out["gt"], fmt="%.17e")
        np.savetxt(pf, out["pred"], fmt="%.17e")
        assert np.array_equal(np.loadtxt(pf), out["pred"]) and np.array_equal(np.loadtxt(gf), out["gt"])
        for mode in modes:
            a, g0 = run_plot_kitti(pk, mode, gf, pf)
            aligned["aligned_" + mode] = a
            out["gt_rebased"] = g0
    if any(m in modes for m in ("7dof", "6dof")):
        x0 = aligned["aligned_scale"][:, [3, 7, 11]].T           # the re-based prediction up to a scale: the same ratio
        y0 = out["gt_rebased"][:, [3, 7, 11]].T
        sv0 = np.linalg.svd(_cov(x0, y0), compute_uv=False)
        out["cond_sv_ratio_rebased"] = np.float64(sv0[1] / sv0[0])
        assert out["cond_sv_ratio"] >= 1e-3 and out["cond_sv_ratio_rebased"] >= 1e-3, (out["cond_sv_ratio"], sv0)
    return out, aligned


def _cov(x, y):
    xc, yc = x - x.mean(1, keepdims=True), y - y.mean(1, keepdims=True)
    return yc @ xc.T / x.shape[1]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    mods = import_reference(ref)
    o4, a4 = make("04", 4, ref, mods, ("scale", "scale_7dof"))
    o10, a10 = make("10", 10, ref, mods, ("scale", "scale_7dof", "7dof", "6dof"))
    assert len(o10["table"]) == 464 and set(o10["table"][:, 3]) == set(map(float, LENGTHS))
    assert o4["table"][:, 3].max() == 300.0 and not o4["per_length_present"][3:].any()
    np.savez_compressed(os.path.join(OUT, "odometry_eval_04.npz"), **o4, **a4)
    np.savez_compressed(os.path.join(OUT, "odometry_eval_10.npz"), **o10)
    np.savez_compressed(os.path.join(OUT, "odometry_eval_10_aligned.npz"), **a10)
    for f in ("odometry_eval_04.npz", "odometry_eval_10.npz", "odometry_eval_10_aligned.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")
    for tag, o in (("04", o4), ("10", o10)):
        print(tag, "segments", len(o["table"]), "t_err %.6f r_err %.3e" % (o["t_err"], o["r_err"]), "min rot err %.3e" % o["cond_min_rot_err"],
              "min dist gap %.3e" % o["cond_min_dist_gap"], "sv ratio %.3e" % o["cond_sv_ratio"], "scale %.6f" % o["umeyama_s_c"])


if __name__ == "__main__":
    main()
