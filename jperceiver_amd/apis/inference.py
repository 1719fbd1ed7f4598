"""Inference entry points with the behaviour of the reference's demo scripts, on the HIP kernels:

    evaluate_depth(model, batches, gt_depths, stereo_scale=False)
        scripts/eval_depth_eigen.py:24-113: eval-mode forward -> ("disp", 0, 0) -> disp_to_depth(0.1, 100) -> resize to the
        ground truth -> 1/disp, range mask (0.1 .. 80 m) + Garg crop, per-image median scaling (or the fixed stereo
        factor 1), clamp, the seven depth metrics; returns (mean errors, median ratio, std of ratios / median).
    evaluate_depth_lidar(model, batches, scans, calib, batch=8, stereo_scale=False)
        evaluate_depth with the ground truth built on the device from Velodyne scans (core.evaluation.lidar_depth_maps, the
        reference's generate_depth_map) and the images scored `batch` at a time (core.evaluation.eval_depth_batch); images are
        grouped by ground-truth size, which differs between KITTI drives.  Same triple.
    pose_between(pose_encoder, pose_decoder, img_a, img_b)
        the 4x4 transform `transformation_from_parameters(axisangle[:, 0], translation[:, 0])` of
        scripts/draw_odometry.py:69-71 for one pair (both images concatenated on channels, frame 0 first).
    chain_poses(transforms)
        scripts/draw_odometry.py:62-76: global_pose <- global_pose @ inv(T_k), rows 0..2 flattened -> (n+1, 12)
        (the KITTI odometry text format written by the script).
    odometry(pose_encoder, pose_decoder, frames)
        both of the above over a sequence of frames: (n, 3, H, W) -> (n, 12).
    chain_poses_device(T, invert=True)
        chain_poses on the device: (n,4,4) float32 device transforms -> (n+1, 12) float64 device poses (jp_pose_chain_f64; the
        general affine inverse, like np.linalg.inv; invert=False is eval_kitti_video.py:292's chaining).
    odometry_device(pose_encoder, pose_decoder, frames, batch=8)
        odometry() with the pairs run `batch` at a time and the chain on the device: (n,3,H,W) -> (n, 12) device float64.
    evaluate_odometry(pose_encoder, pose_decoder, frames, gt_poses, batch=8, **eval_kw)
        odometry_device + core.evaluation.eval_odometry (mono/tools/kitti_evaluation_toolkit.py: the paper's t_err / r_err).
    freeze(model_or_module) / unfreeze(module)
        frozen inference: every eval-mode `conv -> BatchNorm2d` pair below the module (the three ResNet-18 encoders, the BEV
        decoders) is folded into one convolution (jp_bn_fold_conv, once) and the residual blocks end in one relu(a + b) pass
        (jp_add_relu) -- no BatchNorm pass over any activation map.  Opt-in; every helper here and apis.Perceiver work on a
        frozen model as on any other.  Weights that change afterwards (load_state_dict, in-place edits, an optimizer step, a
        train-mode forward) are folded again by the next forward; train mode ignores the frozen state.
    read_kitti_poses(path) / write_kitti_poses(path, poses)
        the KITTI pose text file: 12 numbers per line, or 13 with a leading frame index (loadPoses); written with '%1.8e'
        like the script (draw_odometry.py:78).
The networks must already hold a checkpoint (apis.load_checkpoint; the scripts copy `PoseEncoder.*` / `PoseDecoder.*`
out of the training checkpoint's state dict, which `pose_nets_from_checkpoint` restates)."""
from __future__ import annotations

import numpy as np
import torch

from .._lib import call, lib
from ..core import evaluation as ev
from ..model import modules as _modules


def _eval(*mods):
    for m in mods:
        if m.training:
            raise RuntimeError("inference helpers expect eval-mode networks (call .eval(): BatchNorm must use running stats)")


def freeze(module):
    """Fold every eligible conv/BatchNorm2d pair of an eval-mode model (or sub-network) and attach the folded state; returns the
    same module.  The forward passes then take the frozen route while the module is in eval mode.

    Each forward re-folds the pairs whose source tensors moved, as far as the host can see it: load_state_dict, in-place
    tensor operations, optimizer steps and train-mode forwards are seen.  A write through `.data` (or by foreign code through a
    raw pointer) is NOT, exactly as for the packed-weight cache: call `jperceiver_amd.ops.weights_changed()` after one."""
    if module.training:
        raise RuntimeError("freeze expects an eval-mode model (call .eval(): BatchNorm must use running stats)")
    return _modules.freeze_module(module)


def unfreeze(module):
    """Remove the frozen state: the forward passes are the eval-mode BatchNorm route again.  Returns the module."""
    return _modules.unfreeze_module(module)


@torch.no_grad()
def evaluate_depth(model, batches, gt_depths, stereo_scale=False, min_depth=0.1, max_depth=80.0):
    """batches: iterable of input dicts with ("color_aug"|"color", 0, 0) (1,3,H,W) CUDA tensors; gt_depths: sequence of
    (h, w) arrays / tensors in metres (0 where there is no LiDAR return)."""
    _eval(model)
    errors, ratios = [], []
    for inputs, gt in zip(batches, gt_depths):
        disp = model(inputs)[("disp", 0, 0)]
        gt = torch.as_tensor(np.asarray(gt) if not isinstance(gt, torch.Tensor) else gt, dtype=torch.float32).to(disp.device)
        for b in range(disp.shape[0]):
            r = ev.eval_depth(disp[b:b + 1], gt if gt.dim() == 2 else gt[b], stereo_scale=stereo_scale, min_depth=0.1,
                              max_depth=100, mask_min=min_depth, mask_max=max_depth, stereo_factor=1.0)
            errors.append([r[k] for k in ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")])
            ratios.append(r["scale"])
    ratios = np.asarray(ratios)
    med = float(np.median(ratios))
    return dict(zip(("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"), np.asarray(errors).mean(0).tolist())), med, \
        float(np.std(ratios / med))


_ERR_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


def _calib_entry(c, cam):
    if isinstance(c, (str, bytes)) or hasattr(c, "__fspath__"):
        from ..datasets.kitti_calib import velo_to_image
        return velo_to_image(c, cam)
    P, hw = c
    return np.asarray(P, dtype=np.float64).reshape(3, 4), (int(hw[0]), int(hw[1]))


@torch.no_grad()
def evaluate_depth_lidar(model, batches, scans, calib, batch=8, stereo_scale=False, min_depth=0.1, max_depth=80.0, cam=2,
                         vel_depth=False):
    """batches: as for evaluate_depth; scans: one (N, 4) float32 Velodyne scan (array, tensor, or the path of a .bin file) per IMAGE,
    in the order the images come; calib: one entry for all images or one per image, each a calibration directory (read with
    datasets.kitti_calib.velo_to_image for camera `cam`) or a (P (3,4), (H, W)) pair.  Up to `batch` images of one ground-truth size
    are turned into depth maps by one jp_lidar_depth_map call and scored by one jp_depth_eval_batch call."""
    _eval(model)
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    scans = list(scans)
    one_calib = isinstance(calib, (str, bytes)) or hasattr(calib, "__fspath__") or (
        isinstance(calib, tuple) and len(calib) == 2 and np.ndim(calib[0]) == 2)
    cache = {}

    def calib_of(i):
        c = calib if one_calib else calib[i]
        key = c if isinstance(c, (str, bytes)) else id(c)
        if key not in cache:
            cache[key] = _calib_entry(c, cam)
        return cache[key]

    results, pending = {}, {}

    def flush(key):
        items = pending.pop(key)
        gt = ev.lidar_depth_maps([it[2] for it in items], np.stack([it[3] for it in items]), key[0], vel_depth=vel_depth,
                                 dtype=torch.float32, device=items[0][1].device)
        res = ev.eval_depth_batch(torch.cat([it[1] for it in items], 0), gt, stereo_scale=stereo_scale, min_depth=0.1, max_depth=100,
                                  mask_min=min_depth, mask_max=max_depth, stereo_factor=1.0)
        for it, r in zip(items, res):
            results[it[0]] = r

    i = 0
    for inputs in batches:
        disp = model(inputs)[("disp", 0, 0)]
        for b in range(disp.shape[0]):
            if i >= len(scans):
                raise ValueError(f"{len(scans)} scans for more images")
            pts = scans[i]
            if isinstance(pts, (str, bytes)) or hasattr(pts, "__fspath__"):
                from ..datasets.kitti_calib import load_velodyne_points
                pts = load_velodyne_points(pts)
            P, hw = calib_of(i)
            key = (hw, tuple(disp.shape[2:]))
            pending.setdefault(key, []).append((i, disp[b:b + 1], pts, P))
            if len(pending[key]) == int(batch):
                flush(key)
            i += 1
    for key in list(pending):
        flush(key)
    if not results:
        raise ValueError("no image to evaluate")
    errors = [[results[j][k] for k in _ERR_KEYS] for j in range(i)]
    ratios = np.asarray([results[j]["scale"] for j in range(i)])
    med = float(np.median(ratios))
    return dict(zip(_ERR_KEYS, np.asarray(errors).mean(0).tolist())), med, float(np.std(ratios / med))


@torch.no_grad()
def pose_between(pose_encoder, pose_decoder, img_a, img_b):
    """(B,3,H,W) x 2 -> (B,4,4): the transform the pose head predicts for the pair [img_a | img_b] (no inversion)."""
    _eval(pose_encoder, pose_decoder)
    axisangle, translation = pose_decoder(pose_encoder(torch.cat([img_a, img_b], 1).contiguous()))
    aa, tr = axisangle[:, 0].reshape(-1, 3).contiguous(), translation[:, 0].reshape(-1, 3).contiguous()
    B = aa.shape[0]
    K = torch.eye(4, device=aa.device).repeat(B, 1, 1)                 # only T is used (P = K@T is a by-product)
    T = torch.empty((B, 4, 4), device=aa.device)
    P = torch.empty((B, 3, 4), device=aa.device)
    call("jp_pose_fwd", aa, tr, K, T, P, B, 0)
    return T


def chain_poses(transforms) -> np.ndarray:
    """(n,4,4) frame-to-frame transforms -> (n+1, 12) global poses, float64 on the host like the script."""
    T = np.asarray(transforms.detach().cpu().numpy() if isinstance(transforms, torch.Tensor) else transforms, dtype=np.float64)
    g = np.identity(4)
    out = [g[0:3, :].reshape(1, 12)]
    for k in range(T.shape[0]):
        g = g @ np.linalg.inv(T[k])
        out.append(g[0:3, :].reshape(1, 12))
    return np.concatenate(out, 0)


@torch.no_grad()
def odometry(pose_encoder, pose_decoder, frames) -> np.ndarray:
    """frames (n,3,H,W) CUDA tensor (already at the pose nets' resolution) -> (n, 12) chained poses."""
    Ts = [pose_between(pose_encoder, pose_decoder, frames[k:k + 1], frames[k + 1:k + 2])[0] for k in range(frames.shape[0] - 1)]
    return chain_poses(torch.stack(Ts)) if Ts else np.identity(4)[0:3].reshape(1, 12)


def chain_poses_device(T, invert=True) -> torch.Tensor:
    """(n,4,4) float32 device transforms -> (n+1, 12) float64 device poses: G_0 = I, G_k = G_{k-1} @ inv(T_k) (or @ T_k)."""
    if not (isinstance(T, torch.Tensor) and T.is_cuda):
        raise RuntimeError("chain_poses_device runs a HIP kernel: pass a CUDA tensor (chain_poses is the host version)")
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4) or T.dtype != torch.float32:
        raise ValueError(f"expected (n,4,4) float32 transforms, got {tuple(T.shape)} {T.dtype}")
    n = T.shape[0]
    poses = torch.empty((n + 1, 12), device=T.device, dtype=torch.float64)
    if n == 0:
        poses[0] = torch.eye(4, device=T.device, dtype=torch.float64)[:3].reshape(12)
        return poses
    ws = torch.empty(lib().fn["jp_pose_chain_ws_bytes"](n), device=T.device, dtype=torch.uint8)
    call("jp_pose_chain_f64", T.contiguous(), n, 1 if invert else 0, poses, ws)
    return poses


@torch.no_grad()
def pair_transforms(pose_encoder, pose_decoder, frames, batch=8) -> torch.Tensor:
    """frames (n,3,H,W) CUDA tensor -> (n-1,4,4) float32 device transforms of the pairs [frames[k] | frames[k+1]], `batch` pairs
    per forward pass of the pose nets and per jp_pose_fwd launch."""
    _eval(pose_encoder, pose_decoder)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
        raise RuntimeError("the pose nets run HIP kernels: pass frames as a CUDA tensor")
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    n = frames.shape[0] - 1
    T = torch.empty((max(n, 0), 4, 4), device=frames.device)
    for k0 in range(0, n, int(batch)):
        k1 = min(n, k0 + int(batch))
        B = k1 - k0
        axisangle, translation = pose_decoder(pose_encoder(torch.cat([frames[k0:k1], frames[k0 + 1:k1 + 1]], 1).contiguous()))
        aa, tr = axisangle[:, 0].reshape(-1, 3).contiguous(), translation[:, 0].reshape(-1, 3).contiguous()
        K = torch.eye(4, device=aa.device).repeat(B, 1, 1)             # only T is used (P = K@T is a by-product)
        P = torch.empty((B, 3, 4), device=aa.device)
        call("jp_pose_fwd", aa, tr, K, T[k0:k1], P, B, 0)
    return T


@torch.no_grad()
def odometry_device(pose_encoder, pose_decoder, frames, batch=8) -> torch.Tensor:
    """odometry() without leaving the device: frames (n,3,H,W) -> (n, 12) float64 device poses."""
    return chain_poses_device(pair_transforms(pose_encoder, pose_decoder, frames, batch), invert=True)


def evaluate_odometry(pose_encoder, pose_decoder, frames, gt_poses, batch=8, **eval_kw):
    """odometry_device + eval_odometry against gt_poses ((n,12) array or tensor, e.g. read_kitti_poses) -> eval_odometry's dict
    plus `poses`, the predicted (n,12) device trajectory."""
    pred = odometry_device(pose_encoder, pose_decoder, frames, batch)
    gt = torch.as_tensor(np.asarray(gt_poses) if not isinstance(gt_poses, torch.Tensor) else gt_poses)
    gt = gt.to(device=pred.device, dtype=torch.float64).reshape(-1, 12)
    out = ev.eval_odometry(pred, gt, **eval_kw)
    out["poses"] = pred
    return out


def read_kitti_poses(path) -> np.ndarray:
    """KITTI pose file -> (n,12) float64; a 13-column file carries the frame index first (loadPoses), which is dropped."""
    a = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if a.shape[1] not in (12, 13):
        raise ValueError(f"{path}: expected 12 or 13 numbers per line, got {a.shape[1]}")
    return np.ascontiguousarray(a[:, -12:])


def write_kitti_poses(path, poses) -> None:
    """(n,12) poses (array or tensor) -> text, one pose per line, '%1.8e' (draw_odometry.py:78)."""
    p = poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
    np.savetxt(path, np.asarray(p, dtype=np.float64).reshape(-1, 12), delimiter=" ", fmt="%1.8e")


def pose_nets_from_checkpoint(checkpoint, pose_encoder, pose_decoder):
    """scripts/draw_odometry.py:52-56: copy `PoseEncoder.*` / `PoseDecoder.*` of a training checkpoint into the nets."""
    sd = checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint
    for prefix, net in (("PoseEncoder.", pose_encoder), ("PoseDecoder.", pose_decoder)):
        own = net.state_dict()
        missing = [n for n in own if prefix + n not in sd]
        if missing:
            raise KeyError(f"checkpoint lacks {prefix}{missing[0]} (+{len(missing) - 1} more)")
        net.load_state_dict({n: sd[prefix + n] for n in own}, strict=True)
    return pose_encoder, pose_decoder
