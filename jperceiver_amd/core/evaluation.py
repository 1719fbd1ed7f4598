"""Evaluation metrics with the reference's names and semantics (mono/core/evaluation/pixel_error.py:27-118,
mono/core/evaluation/eval_hooks.py:147-199), computed by GPU reductions of libjperceiver_hip.so
(csrc/evalmetrics.hip) instead of numpy on host copies:

    compute_errors(gt, pred)            abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 over two equally shaped tensors
    mean_IU(eval_segm, gt_segm)         per-class IoU list, classes = union of the labels present (pixel_error.py:82-118)
    mean_precision(eval_segm, gt_segm)  per-class precision list, classes = labels present in gt (pixel_error.py:59-79)
    eval_layout(logits, label)          the hook's per-sample layout block (eval_hooks.py:181-199): argmax + both lists
    eval_depth(disp, gt_depth)          the hook's per-sample depth block (eval_hooks.py:147-179): scaled disparity ->
                                        bilinear resize to the ground-truth size -> depth, range mask + Garg crop, median
                                        scaling (or the fixed x36 stereo scale), clamp, compute_errors -> dict incl. 'scale'
    eval_depth_batch(disp, gt_depths)   eval_depth for B samples of one ground-truth size in four launches and one device-to-host copy
                                        (jp_depth_eval_batch): exact medians, sums folded in a fixed order -> list of the same dicts
    disp_to_depth, AverageMeter         as in pixel_error.py

and the depth ground truth of the Eigen split from Velodyne scans (mono/datasets/kitti_utils.py:50-102), csrc/lidar.hip:

    lidar_depth_maps(points, P, hw)     B scans -> (B, H, W) device maps in one call: the closest return per pixel in float64, incl. the
                                        reference's shared key of pixel (r, W-1) and pixel (r+1, 0) (see csrc/lidar.hip)
    generate_depth_map(calib_dir, velo_filename, cam, vel_depth)   the reference's signature on KITTI files -> one (H, W) device map

and the KITTI odometry evaluation of mono/tools/kitti_evaluation_toolkit.py (`kittiOdomEval.eval`, the paper's t_err / r_err) with
the alignment modes of scripts/plot_kitti.py, on (n,12) float64 device trajectories (csrc/odometry.hip):

    umeyama_alignment(x, y, with_scale) (R, t, c) of Umeyama's least-squares similarity y ~ c R x + t (mono/tools/geometry.py:20-67):
                                        the moments are one device reduction, the 3x3 SVD runs on the host on 19 numbers
    align_poses(pred, gt, mode)         "umeyama_scale" (the toolkit's align_trajectory(correct_only_scale=True)), "scale",
                                        "scale_7dof", "7dof", "6dof" (plot_kitti.py:223-243, both trajectories re-based to their
                                        first pose), "none" -> (aligned trajectory, parameters)
    eval_odometry(pred, gt)             align, then calcSequenceErrors' segment table (every `step` frames x every length of
                                        100..800 m), computeOverallErr / computeSegmentErr / computeSpeedErr, plus the ATE

Segmentation inputs are 2-class maps ({0, 1}; num_class = 2 in every north-star config).  The list-length quirks of the
reference are kept: a class that occurs neither in the prediction nor in the label is simply absent from mean_IU's list.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .._lib import call, lib

MIN_DEPTH = 1e-3
MAX_DEPTH = 80


class AverageMeter(object):
    """pixel_error.py:7-24."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def disp_to_depth(disp, min_depth=0.1, max_depth=100):
    """pixel_error.py:43-48 (elementwise; works on tensors and arrays)."""
    min_disp, max_disp = 1 / max_depth, 1 / min_depth
    scaled_disp = min_disp + (max_disp - min_disp) * disp
    return scaled_disp, 1 / scaled_disp


def _dev(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("evaluation metrics run HIP kernels: pass CUDA tensors")
    return t.contiguous().float()


def _errors_from_sums(s):
    n = s[7]
    if n == 0:
        # no valid pixel (e.g. no LiDAR return inside the Garg crop): the reference's numpy path yields NaNs with a
        # RuntimeWarning (mean of an empty slice, pixel_error.py:27-40) and the evaluation carries on
        import warnings
        warnings.warn("depth metrics over an empty set of valid pixels: returning NaN", RuntimeWarning)
        return (float("nan"),) * 7
    return (s[5] / n, s[6] / n, math.sqrt(s[3] / n), math.sqrt(s[4] / n), s[0] / n, s[1] / n, s[2] / n)


def compute_errors(gt, pred):
    """pixel_error.py:27-40 on two equally shaped CUDA tensors (every element counts)."""
    gt, pred = _dev(gt).reshape(-1), _dev(pred).reshape(-1)
    assert gt.numel() == pred.numel() and gt.numel() > 0
    valid = torch.ones(gt.numel(), device=gt.device, dtype=torch.uint8)
    sums = torch.empty(8, device=gt.device, dtype=torch.float64)
    # fixed_scale 1.0 and a clamp range that never binds: the plain metric definitions
    call("jp_depth_errors", gt, pred, valid, gt.numel(), None, None, 1.0, 0.0, 3.0e38, sums)
    return _errors_from_sums(sums.cpu().tolist())


def _confusion(logits, label):
    logits, label = _dev(logits), _dev(label)
    B, C, h, w = logits.shape
    if C != 2:
        raise NotImplementedError("2-class layouts only (num_class = 2)")
    counts = torch.empty((B, 4), device=logits.device, dtype=torch.float64)
    call("jp_confusion2", logits, label.reshape(B, h * w), counts, B, h * w)
    return counts.cpu().numpy()          # [b][2*pred + true]


def _iu_from_counts(c):
    """mean_IU's list for one image from its confusion counts (pixel_error.py:82-118)."""
    n = {(p, t): c[2 * p + t] for p in (0, 1) for t in (0, 1)}
    out = []
    for k in (0, 1):
        n_eval, n_gt = n[(k, 0)] + n[(k, 1)], n[(0, k)] + n[(1, k)]
        if n_eval == 0 and n_gt == 0:
            continue                      # not in the union of classes
        if n_eval == 0 or n_gt == 0:
            out.append(0)
            continue
        out.append(n[(k, k)] / (n_gt + n_eval - n[(k, k)]))
    return out


def _prec_from_counts(c):
    """mean_precision's list for one image (pixel_error.py:59-79): classes present in gt; 0/0 -> 0."""
    n = {(p, t): c[2 * p + t] for p in (0, 1) for t in (0, 1)}
    out = []
    for k in (0, 1):
        if n[(0, k)] + n[(1, k)] == 0:
            continue
        n_eval = n[(k, 0)] + n[(k, 1)]
        out.append(0. if n_eval == 0 else n[(k, k)] / float(n_eval))
    return out


def _segm_counts(eval_segm, gt_segm):
    e, g = torch.as_tensor(eval_segm), torch.as_tensor(gt_segm)
    if e.shape != g.shape or e.dim() != 2:
        raise ValueError("DiffDim: Different dimensions of matrices!")
    e = e.cuda().float()
    logits = torch.stack([1.0 - e, e], 0).unsqueeze(0)          # argmax reproduces the given 0/1 prediction
    return _confusion(logits, g.cuda().float().reshape(1, 1, *g.shape))[0]


def mean_IU(eval_segm, gt_segm):
    return _iu_from_counts(_segm_counts(eval_segm, gt_segm))


def mean_precision(eval_segm, gt_segm):
    return _prec_from_counts(_segm_counts(eval_segm, gt_segm))


def eval_layout(logits, label):
    """eval_hooks.py:181-199 for a batch: per sample (mean_IU list, mean_precision list) of argmax(logits, 1) vs label."""
    c = _confusion(logits, label)
    return [(_iu_from_counts(ci), _prec_from_counts(ci)) for ci in c]


def eval_depth(disp, gt_depth, stereo_scale=False, min_depth=0.1, max_depth=100, mask_min=MIN_DEPTH, mask_max=MAX_DEPTH,
               stereo_factor=36.0):
    """eval_hooks.py:147-179 for one sample: disp (1,1,h,w) network output, gt_depth (H,W).  mask_min / mask_max /
    stereo_factor default to the hook's constants (1e-3, 80, 36); scripts/eval_depth_eigen.py uses (0.1, 80, 1)."""
    disp, gt = _dev(disp), _dev(gt_depth)
    assert disp.dim() == 4 and disp.shape[:2] == (1, 1) and gt.dim() == 2
    h, w = disp.shape[2:]
    H, W = gt.shape
    scaled = torch.empty_like(disp)
    # scaled_disp = min_disp + (max_disp - min_disp) * disp, then cv2.resize(INTER_LINEAR) == half-pixel bilinear
    call("jp_affine", disp, scaled, disp.numel(), 1.0 / min_depth - 1.0 / max_depth, 1.0 / max_depth)
    res = torch.empty((1, 1, H, W), device=disp.device, dtype=torch.float32)
    call("jp_bilinear_fwd", scaled, res, 1, h, w, H, W)
    crop = np.array([0.40810811 * H, 0.99189189 * H, 0.03594771 * W, 0.96405229 * W]).astype(np.int32)
    pred = torch.empty((H, W), device=disp.device, dtype=torch.float32)
    valid = torch.empty((H, W), device=disp.device, dtype=torch.uint8)
    call("jp_depth_eval_prepare", res, gt, pred, valid, H, W, int(crop[0]), int(crop[1]), int(crop[2]), int(crop[3]),
         float(mask_min), float(mask_max))
    med_g = torch.empty(2, device=disp.device, dtype=torch.float32)
    med_p = torch.empty(2, device=disp.device, dtype=torch.float32)
    call("jp_masked_median", gt, valid, H * W, med_g)
    call("jp_masked_median", pred, valid, H * W, med_p)
    sums = torch.empty(8, device=disp.device, dtype=torch.float64)
    call("jp_depth_errors", gt, pred, valid, H * W, med_g, med_p, float(stereo_factor) if stereo_scale else 0.0,
         float(mask_min), float(mask_max), sums)
    s = sums.cpu().tolist()
    mg, mp = med_g.cpu().tolist(), med_p.cpu().tolist()
    abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 = _errors_from_sums(s)
    scale = mg[1] / mp[1] if (s[7] > 0 and mp[1] != 0) else float("nan")
    return dict(abs_rel=abs_rel, sq_rel=sq_rel, rmse=rmse, rmse_log=rmse_log, a1=a1, a2=a2, a3=a3, scale=scale,
                n_valid=int(s[7]))


def _garg_crop(H, W):
    crop = np.array([0.40810811 * H, 0.99189189 * H, 0.03594771 * W, 0.96405229 * W]).astype(np.int32)
    return int(crop[0]), int(crop[1]), int(crop[2]), int(crop[3])


def eval_depth_batch(disp, gt_depths, stereo_scale=False, min_depth=0.1, max_depth=100, mask_min=MIN_DEPTH, mask_max=MAX_DEPTH,
                     stereo_factor=36.0):
    """eval_depth for a batch: disp (B,1,h,w), gt_depths (B,H,W) -> list of B dicts with eval_depth's keys.  n_valid, the medians
    (hence `scale`) and the a1 / a2 / a3 counts are those of B eval_depth calls bit for bit; the four float64 error sums are
    folded in a fixed order (bit-identical from run to run) and differ from eval_depth's atomically merged ones by reordering only."""
    disp, gt = _dev(disp), _dev(gt_depths)
    if disp.dim() != 4 or disp.shape[1] != 1 or gt.dim() != 3 or gt.shape[0] != disp.shape[0] or disp.shape[0] < 1:
        raise ValueError(f"expected disp (B,1,h,w) and gt_depths (B,H,W), got {tuple(disp.shape)} and {tuple(gt.shape)}")
    B, _, h, w = disp.shape
    H, W = gt.shape[1:]
    y0, y1, x0, x1 = _garg_crop(H, W)
    out = torch.empty(B * 10, device=disp.device, dtype=torch.float64)            # sums (B,8) | med (B,4) floats: one copy back
    sums, med = out[:B * 8], out[B * 8:].view(torch.float32)
    call("jp_depth_eval_batch", disp, gt, B, h, w, H, W, y0, y1, x0, x1, float(mask_min), float(mask_max), float(min_depth),
         float(max_depth), float(stereo_factor) if stereo_scale else 0.0, sums, med,
         _ws("jp_depth_eval_batch_ws_bytes", disp.device, B, H, W))
    host = out.cpu()
    s_all, m_all = host[:B * 8].reshape(B, 8).tolist(), host[B * 8:].view(torch.float32).reshape(B, 4).tolist()
    res = []
    for s, m in zip(s_all, m_all):
        abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 = _errors_from_sums(s)
        scale = m[1] / m[3] if (s[7] > 0 and m[3] != 0) else float("nan")
        res.append(dict(abs_rel=abs_rel, sq_rel=sq_rel, rmse=rmse, rmse_log=rmse_log, a1=a1, a2=a2, a3=a3, scale=scale,
                        n_valid=int(s[7])))
    return res


def lidar_depth_maps(points, P, hw, flip=None, vel_depth=False, dtype=torch.float64, device=None):
    """Depth ground truth of B Velodyne scans in one call (jp_lidar_depth_map; kitti_utils.py:50-102 per scan).
    points: list of B (N_b, 4) float32 arrays / tensors (x, y, z, reflectance; N_b may be 0 and may differ); P: (3,4) or (B,3,4)
    float64 velodyne -> image matrices (datasets.kitti_calib.velo_to_image); hw: (H, W) of the maps; flip: B booleans (mirror the
    finished map left-right) or None; dtype float64 or float32 (the rounded float64 map) -> (B, H, W) device tensor."""
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("dtype must be torch.float64 or torch.float32")
    B = len(points)
    if B < 1:
        raise ValueError("at least one scan")
    H, W = int(hw[0]), int(hw[1])
    scans = [p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)) for p in points]
    for p in scans:
        if p.dim() != 2 or p.shape[1] != 4 or p.dtype != torch.float32:
            raise ValueError(f"every scan must be an (N, 4) float32 array, got {tuple(p.shape)} {p.dtype}")
    if device is None:
        device = next((p.device for p in scans if p.is_cuda), torch.device("cuda"))
    counts = [int(p.shape[0]) for p in scans]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64).to(device)
    pts = torch.cat([p.to(device) for p in scans], 0).contiguous()
    if pts.shape[0] == 0:
        pts = torch.zeros((1, 4), device=device)                                  # a valid pointer; no row is read
    Pm = torch.as_tensor(np.asarray(P.cpu() if isinstance(P, torch.Tensor) else P, dtype=np.float64))
    if tuple(Pm.shape) == (3, 4):
        Pm = Pm.expand(B, 3, 4)
    if tuple(Pm.shape) != (B, 3, 4):
        raise ValueError(f"P must be (3,4) or ({B},3,4), got {tuple(Pm.shape)}")
    Pm = Pm.contiguous().to(device)
    fl = None
    if flip is not None:
        fl = torch.as_tensor(np.asarray(flip.cpu() if isinstance(flip, torch.Tensor) else flip).astype(bool).astype(np.uint8))
        if tuple(fl.shape) != (B,):
            raise ValueError(f"flip must hold {B} flags")
        fl = fl.to(device)
    out = torch.empty((B, H, W), device=device, dtype=dtype)
    call("jp_lidar_depth_map", pts, offsets, Pm, fl, B, H, W, 1 if vel_depth else 0, out if dtype == torch.float64 else None,
         out if dtype == torch.float32 else None, _ws("jp_lidar_depth_ws_bytes", device, B, H, W))
    return out


def generate_depth_map(calib_dir, velo_filename, cam=2, vel_depth=False):
    """kitti_utils.py:50-102 on KITTI files -> the (H, W) float64 map on the device."""
    from ..datasets.kitti_calib import load_velodyne_points, velo_to_image
    P, hw = velo_to_image(calib_dir, cam)
    return lidar_depth_maps([load_velodyne_points(velo_filename)], P, hw, vel_depth=vel_depth)[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# KITTI odometry evaluation (mono/tools/kitti_evaluation_toolkit.py, scripts/plot_kitti.py) on csrc/odometry.hip
ODOM_LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)
ALIGN_MODES = ("umeyama_scale", "scale", "scale_7dof", "7dof", "6dof", "none")
_I12 = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _traj(p, name="poses"):
    if not (isinstance(p, torch.Tensor) and p.is_cuda):
        raise RuntimeError(f"odometry evaluation runs HIP kernels: {name} must be a CUDA tensor")
    if p.dim() != 2 or p.shape[1] != 12 or p.shape[0] < 1 or p.dtype != torch.float64:
        raise ValueError(f"{name} must be an (n,12) float64 trajectory with n >= 1, got {tuple(p.shape)} {p.dtype}")
    return p.contiguous()


def _host_doubles(values):
    a = (ctypes.c_double * len(values))(*[float(v) for v in values])
    return a, ctypes.addressof(a)


def _ws(name, device, *args):
    nbytes = lib().fn[name](*args)
    if nbytes <= 0:
        raise RuntimeError(f"{name}{args}: {lib().last_error()}")
    return torch.empty(nbytes, device=device, dtype=torch.uint8)


def traj_moments(x, y) -> np.ndarray:
    """The 19 sums of jp_traj_moments over the positions of two equally long trajectories, as float64 numpy:
    mean_x (3), mean_y (3), sigma_x^2, cov (9, row-major), sum x.y, sum x.x, sum |x - y|^2."""
    x, y = _traj(x, "x"), _traj(y, "y")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"trajectories of different lengths: {x.shape[0]} vs {y.shape[0]}")
    n = x.shape[0]
    out = torch.empty(19, device=x.device, dtype=torch.float64)
    call("jp_traj_moments", x, y, n, out, _ws("jp_traj_moments_ws_bytes", x.device, n))
    return out.cpu().numpy()


def transform_poses(poses, A=None, scale=1.0):
    """out_k = A . [R_k | scale t_k] for an (n,12) device trajectory; A: 12 or (3,4) host numbers (None: the identity)."""
    poses = _traj(poses)
    keep, addr = _host_doubles(_I12 if A is None else np.asarray(A, dtype=np.float64).reshape(-1)[:12])
    out = torch.empty_like(poses)
    call("jp_poses_transform_f64", poses, poses.shape[0], addr, float(scale), out)
    return out


def _umeyama_from_moments(m, with_scale):
    """Umeyama 1991, eq. 34-43, from the moments: rotation U S V^T of the covariance's SVD with S = diag(1, 1, det U det V^T)
    (eq. 39, 40, 43), c = tr(D S) / sigma_x^2 (eq. 42), t = mean_y - c R mean_x (eq. 41)."""
    mean_x, mean_y, var_x, cov = m[0:3], m[3:6], m[6], m[7:16].reshape(3, 3)
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        S[2] = -1.0
    R = (U * S) @ Vt
    c = float((D * S).sum() / var_x) if with_scale else 1.0
    t = mean_y - c * (R @ mean_x)
    return R, t, c


def umeyama_alignment(x_poses, y_poses, with_scale=False):
    """(R, t, c) minimising sum |y - (c R x + t)|^2 over the positions of two (n,12) device trajectories, float64 numpy."""
    return _umeyama_from_moments(traj_moments(x_poses, y_poses), with_scale)


def _rebase(poses):
    """inv(pose_0) @ pose_k (plot_kitti.py:192-195, 218-221); the 4x4 inverse of the first pose is taken on the host."""
    g = np.identity(4)
    g[:3] = poses[0].cpu().numpy().reshape(3, 4)
    return transform_poses(poses, np.linalg.inv(g)[:3], 1.0)


def align_poses(pred, gt, mode="umeyama_scale"):
    """Align the (n,12) device trajectory `pred` to `gt` -> (aligned (n,12) device float64, parameters).  parameters: `R` (3,3),
    `t` (3), `scale` as used, and `reference`: the trajectory the aligned one is to be compared with (gt itself, or gt re-based to
    its first pose for the plot_kitti modes, which re-base both)."""
    pred, gt = _traj(pred, "pred"), _traj(gt, "gt")
    if pred.shape[0] != gt.shape[0]:
        raise ValueError(f"pred and gt must have the same number of poses, got {pred.shape[0]} and {gt.shape[0]}")
    if mode not in ALIGN_MODES:
        raise ValueError(f"align mode {mode!r}: expected one of {ALIGN_MODES}")
    R, t, c = np.identity(3), np.zeros(3), 1.0
    if mode == "none":
        return pred, dict(R=R, t=t, scale=c, reference=gt)
    if mode == "umeyama_scale":
        _, _, c = umeyama_alignment(pred, gt, True)
        return transform_poses(pred, None, c), dict(R=R, t=t, scale=c, reference=gt)
    pred0, gt0 = _rebase(pred), _rebase(gt)
    m = traj_moments(pred0, gt0)
    if mode == "scale":
        c = float(m[16] / m[17])                       # scale_lse_solver: sum(X * Y) / sum(X ** 2)
        return transform_poses(pred0, None, c), dict(R=R, t=t, scale=c, reference=gt0)
    Ru, tu, c = _umeyama_from_moments(m, mode != "6dof")
    if mode == "scale_7dof":                           # only the translations are scaled
        return transform_poses(pred0, None, c), dict(R=R, t=t, scale=c, reference=gt0)
    return transform_poses(pred0, np.concatenate([Ru, tu[:, None]], 1), c), dict(R=Ru, t=tu, scale=c, reference=gt0)


def odometry_segments(pred, gt, lengths=ODOM_LENGTHS, step=10):
    """calcSequenceErrors on two (n,12) device trajectories -> (table (m,5) float64 numpy in the reference's order, rows
    [first_frame, r_err/len, t_err/len, len, speed]; last_frame (S, nlen) int32 numpy, -1 = sequence too short; dist (n) numpy)."""
    pred, gt = _traj(pred, "pred"), _traj(gt, "gt")
    if pred.shape[0] != gt.shape[0]:
        raise ValueError(f"pred and gt must have the same number of poses, got {pred.shape[0]} and {gt.shape[0]}")
    n, nlen, step = gt.shape[0], len(lengths), int(step)
    if not 1 <= nlen <= 16:
        raise ValueError("between 1 and 16 segment lengths per call")
    if step <= 0:
        raise ValueError("step must be positive")
    S = (n + step - 1) // step
    keep, addr = _host_doubles(lengths)
    dist = torch.empty(n, device=gt.device, dtype=torch.float64)
    last = torch.empty(S * nlen, device=gt.device, dtype=torch.int32)
    table = torch.empty((S * nlen, 5), device=gt.device, dtype=torch.float64)
    call("jp_odom_segment_errors", gt, pred, n, step, addr, nlen, dist, last, table,
         _ws("jp_odom_segments_ws_bytes", gt.device, n, step, nlen))
    last = last.cpu().numpy()
    return table.cpu().numpy()[last >= 0], last.reshape(S, nlen), dist.cpu().numpy()


def _mean_tr(rows):
    return [float(np.mean(rows[:, 2])), float(np.mean(rows[:, 1]))] if len(rows) else []


def eval_odometry(pred, gt, align="umeyama_scale", lengths=ODOM_LENGTHS, step=10):
    """kittiOdomEval.eval for one sequence (kitti_evaluation_toolkit.py:554-630) on (n,12) float64 device trajectories -> dict:
    t_err, r_err     computeOverallErr: plain means of the table's t_err/len and r_err/len (printed as t_err * 100 % and
                     r_err * 180 / pi deg/m); NaN with a RuntimeWarning when no segment qualifies (the reference divides by zero)
    segments         the table, (n_segments, 5) numpy; n_segments
    per_length       computeSegmentErr: {len: [t, r] or []};  per_speed: computeSpeedErr: {2, 4, .., 24 m/s: [t, r] or []}
    distance, max_speed (m/s), scale (of the alignment), ate = sqrt(sum |x - y|^2 / n) of the aligned trajectory."""
    pred, gt = _traj(pred, "pred"), _traj(gt, "gt")
    if pred.shape[0] != gt.shape[0]:
        raise ValueError(f"pred and gt must have the same number of poses, got {pred.shape[0]} and {gt.shape[0]}")
    aligned, prm = align_poses(pred, gt, align)
    seg, last, dist = odometry_segments(aligned, gt, lengths, step)
    n = gt.shape[0]
    if len(seg):
        t_err, r_err = float(np.mean(seg[:, 2])), float(np.mean(seg[:, 1]))
    else:
        import warnings
        warnings.warn("odometry errors over an empty set of segments (trajectory shorter than every length): returning NaN",
                      RuntimeWarning)
        t_err = r_err = float("nan")
    per_length = {ln: _mean_tr(seg[seg[:, 3] == float(ln)]) for ln in lengths}
    per_speed = {s: _mean_tr(seg[np.abs(seg[:, 4] - s) < 2.0]) for s in range(2, 25, 2)}
    ate = math.sqrt(traj_moments(aligned, prm["reference"])[18] / n)
    return dict(t_err=t_err, r_err=r_err, segments=seg, n_segments=int(len(seg)), per_length=per_length, per_speed=per_speed,
                distance=float(dist[-1]), max_speed=float(seg[:, 4].max()) if len(seg) else 0.0, scale=float(prm["scale"]), ate=ate)
