"""Video perception with the behaviour of the reference's demo (scripts/eval_kitti_video.py), on the device end to end:

    Perceiver(model).perceive(frames, prev)       -> Perception: raw disparity, metric depth at the output size, the
                                                     bird's-eye-view class map and the ego-motion of the pair
    Perceiver(model).perceive_video(frames)       -> VideoPerception: the same over a drive, plus the chained trajectory
    Perceiver(model).stream(src_hw)               -> PerceptionStream (apis/stream.py): raw uint8 frames one by one, state kept on the device
    colorize_disp(disp, lut, q=0.95)              -> the script's `plt.imsave(..., cmap='magma', vmax=np.percentile(disp, 95))`
    layout_rgb(layout)                            -> the script's palette image of the class map
    quantiles(x, q)                               -> np.quantile(x, q, axis=1) by exact selection on the device

The network side is `Baseline`'s eval forward and `Baseline.predict_poses`; everything after the heads (the resize to the
source size, 1/disp, the percentile, the colouring, the two-head argmax and its palette) is csrc/perception.hip -- the
script does it in host numpy on copied-back tensors, the palette step with a Python loop over the pixels (:195-218).
`perceive` enqueues work and returns device tensors; it never waits for the device."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from .._lib import call, lib

_MAX_ROWS = 64          # jp_quantiles: rows per call
_MAX_Q = 4              # ... and quantiles per call


class Perception(NamedTuple):
    disp: torch.Tensor                      # (B,1,h,w)   the network's ("disp", 0, 0) head as it is, in [0,1]
    depth: torch.Tensor                     # (B,1,OH,OW) metres
    layout: torch.Tensor                    # (B,occ,occ) uint8: 0 background, 1 road, 2 car
    cam_T_cam: Optional[torch.Tensor]       # (B,4,4) transform for frame -1, None without a predecessor


class VideoPerception(NamedTuple):
    depth: torch.Tensor                     # (n,1,OH,OW)
    layout: torch.Tensor                    # (n,occ,occ) uint8
    cam_T_cam: torch.Tensor                 # (n-1,4,4): entry k-1 belongs to frame k
    trajectory: np.ndarray                  # (n,4,4) float64 on the host: T_0 = I, T_k = T_{k-1} @ cam_T_cam_k


def _cuda_f32(x, name):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError(f"{name} must be a float32 CUDA tensor (the kernels are HIP: no CPU path)")
    return x.contiguous()


def disp_resize_depth(disp, out_size, min_depth, max_depth, want_disp=False):
    """disp (B,1,h,w) in [0,1] -> depth (B,1,OH,OW) = 1 / resize(1/max_depth + (1/min_depth - 1/max_depth) * disp), half-pixel
    bilinear, one kernel; with want_disp also the resized scaled disparity."""
    disp = _cuda_f32(disp, "disp")
    B, C, h, w = disp.shape
    if C != 1:
        raise ValueError("disp must have one channel")
    OH, OW = int(out_size[0]), int(out_size[1])
    depth = torch.empty((B, 1, OH, OW), device=disp.device, dtype=torch.float32)
    sdisp = torch.empty_like(depth) if want_disp else None
    call("jp_disp_resize_depth", disp, depth, sdisp, B, h, w, OH, OW, float(min_depth), float(max_depth))
    return (depth, sdisp) if want_disp else depth


def layout_classes(road_logits, car_logits=None, want_rgb=False):
    """(B,2,h,w) raw logits of the road head and (optionally) the car head -> (B,h,w) uint8 classes: 1 where the road head's
    channel 1 is strictly greater (np.argmax's tie rule), 2 wherever the car head's is; with want_rgb also (B,h,w,3)."""
    road = _cuda_f32(road_logits, "road_logits")
    car = None if car_logits is None else _cuda_f32(car_logits, "car_logits")
    B, C, h, w = road.shape
    if C != 2 or (car is not None and car.shape != road.shape):
        raise ValueError("layout heads must be (B,2,h,w) and of one shape")
    cls = torch.empty((B, h, w), device=road.device, dtype=torch.uint8)
    rgb = torch.empty((B, h, w, 3), device=road.device, dtype=torch.uint8) if want_rgb else None
    call("jp_layout_classes_u8", road, car, cls, rgb, B, h * w)
    return (cls, rgb) if want_rgb else cls


def _order_statistics(x, q):
    """x (rows,n) device floats, q: sequence of <= 4 values -> (device (rows,nq,2) order statistics, float64 (nq,) weights of the
    upper one) -- rows in groups of 64 per launch."""
    x = _cuda_f32(x, "x")
    if x.dim() != 2 or x.shape[1] == 0:
        raise ValueError("x must be (rows, n) with n > 0")
    q64 = np.asarray(q, dtype=np.float64).reshape(-1)
    if not 1 <= q64.size <= _MAX_Q or not np.all((q64 >= 0) & (q64 <= 1)):
        raise ValueError("1..4 quantiles in [0,1]")
    rows, n = x.shape
    # The ABI takes q as float, numpy as double, and float(0.95) * (n-1) is off by up to 0.06 at a million elements.  The rank
    # k = floor(q (n-1)) is settled here in double, and the kernel is sent the float nearest to (k + 1/2) / (n-1), which it
    # floors to the same k (checked); the interpolation weight comes from the double.
    pos = q64 * (n - 1)
    k = np.floor(pos)
    q32 = ((k + 0.5) / max(n - 1, 1)).astype(np.float32) if n > 1 else np.zeros_like(q64, dtype=np.float32)
    q32 = np.where(k >= n - 1, np.float32(1.0), q32).astype(np.float32)
    if not np.array_equal(np.minimum(np.floor(q32.astype(np.float64) * (n - 1)), n - 1), k):
        raise ValueError(f"rows of {n} elements are too long for a float quantile to address every rank")
    qc = (ctypes.c_float * q32.size)(*q32.tolist())
    out = torch.empty((rows, q32.size, 2), device=x.device, dtype=torch.float32)
    ws_bytes = lib().fn["jp_quantiles_ws_bytes"](min(rows, _MAX_ROWS))
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    for r0 in range(0, rows, _MAX_ROWS):        # one scratch for all groups: they run in order on one stream
        r1 = min(rows, r0 + _MAX_ROWS)
        call("jp_quantiles", x[r0:r1], r1 - r0, n, ctypes.addressof(qc), q32.size, out[r0:r1], ws)
    return out, pos - k


def quantiles(x, q):
    """np.quantile(x.astype(float64), q, axis=1).T (method 'linear') of a (rows,n) device tensor -> (rows,nq) float64 on the host:
    the two neighbouring order statistics by exact selection on the device, the interpolation here."""
    st, frac = _order_statistics(x, q)
    st = st.cpu().numpy().astype(np.float64)
    lo, hi = st[..., 0], st[..., 1]
    with np.errstate(invalid="ignore"):
        return np.where(frac == 0, lo, lo + (hi - lo) * frac)


def default_lut():
    """(256,3) uint8 colour table: matplotlib's magma where matplotlib imports, else a grey ramp."""
    try:
        import matplotlib
        table = matplotlib.colormaps["magma"].resampled(256)(np.arange(256), bytes=True)[:, :3]
        return torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint8))
    except Exception:
        return torch.arange(256, dtype=torch.uint8).view(256, 1).repeat(1, 3)


def colorize_disp(disp, lut, q=0.95):
    """disp (B,1,H,W) or (B,H,W) -> (B,H,W,3) uint8: per image Normalize(vmin = minimum, vmax = q-quantile) and the 256-entry
    colour table `lut` ((256,3) uint8), as plt.imsave(path, disp, cmap=..., vmax=np.percentile(disp, 100 q)) writes it."""
    disp = _cuda_f32(disp, "disp")
    if disp.dim() == 4 and disp.shape[1] == 1:
        disp = disp[:, 0]
    if disp.dim() != 3:
        raise ValueError("disp must be (B,1,H,W) or (B,H,W)")
    if not (isinstance(lut, torch.Tensor) and lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)):
        raise TypeError("lut must be a (256,3) uint8 tensor")
    B, H, W = disp.shape
    lut = lut.to(disp.device).contiguous()
    flat = disp.reshape(B, H * W)
    st, frac = _order_statistics(flat, [0.0, q])
    lo, hi = st[:, 1, 0].double(), st[:, 1, 1].double()
    vmm = torch.stack([st[:, 0, 0], (lo + (hi - lo) * float(frac[1])).float() if frac[1] != 0 else st[:, 1, 0]], 1).contiguous()
    out = torch.empty((B, H, W, 3), device=disp.device, dtype=torch.uint8)
    call("jp_colorize_u8", flat, B, H * W, vmm, lut, out)
    return out


def colorize(x, vmin_vmax, lut):
    """x (rows,n) -> (rows,n,3) uint8 with explicit per-row (vmin, vmax) ((rows,2) device floats)."""
    x = _cuda_f32(x, "x")
    rows, n = x.shape
    out = torch.empty((rows, n, 3), device=x.device, dtype=torch.uint8)
    call("jp_colorize_u8", x, rows, n, _cuda_f32(vmin_vmax, "vmin_vmax"), lut.to(x.device).contiguous(), out)
    return out


_PALETTE = ((0, 0, 0), (255, 255, 255), (0, 0, 255))       # background, road, car (eval_kitti_video.py:157-161,198-201)


def layout_rgb(layout):
    """(B,occ,occ) uint8 classes -> (B,occ,occ,3) uint8 palette image.  The class index is its own table index:
    jp_colorize_u8 with (vmin, vmax) = (0, 256) and a table that holds the palette in its first entries."""
    if not (isinstance(layout, torch.Tensor) and layout.is_cuda and layout.dtype == torch.uint8 and layout.dim() == 3):
        raise TypeError("layout must be a (B,h,w) uint8 CUDA tensor")
    B, h, w = layout.shape
    lut = torch.zeros((256, 3), dtype=torch.uint8)
    lut[:len(_PALETTE)] = torch.tensor(_PALETTE, dtype=torch.uint8)
    vmm = torch.tensor([[0.0, 256.0]], device=layout.device).repeat(B, 1)
    return colorize(layout.reshape(B, h * w).float(), vmm, lut).view(B, h, w, 3)


class Perceiver:
    """Per-frame depth, BEV layout and ego-motion from an eval-mode `Baseline` that holds a checkpoint.
    out_size: (OH, OW) of the depth maps (default: the network's resolution); min_depth / max_depth default to model.opt's.
    frozen=True: `apis.freeze(model)` first -- BatchNorm folded into the convolutions (the model stays frozen afterwards)."""

    def __init__(self, model, out_size=None, min_depth=None, max_depth=None, frozen=False):
        if model.training:
            raise RuntimeError("Perceiver expects an eval-mode model (call .eval(): BatchNorm must use running stats)")
        if frozen:
            from .inference import freeze
            freeze(model)
        self.model = model
        self.out_size = None if out_size is None else (int(out_size[0]), int(out_size[1]))
        self.min_depth = float(model.opt.min_depth if min_depth is None else min_depth)
        self.max_depth = float(model.opt.max_depth if max_depth is None else max_depth)

    @torch.no_grad()
    def perceive(self, frames, prev=None) -> Perception:
        """frames / prev: (B,3,H,W) float CUDA tensors at the network's resolution; prev[b] is the frame before frames[b]."""
        if self.model.training:
            raise RuntimeError("Perceiver expects an eval-mode model")
        frames = _cuda_f32(frames, "frames")
        out = self.model({("color_aug", 0, 0): frames})
        disp = out[("disp", 0, 0)]
        depth = disp_resize_depth(disp, self.out_size or frames.shape[2:], self.min_depth, self.max_depth)
        layout = layout_classes(out["topview"], out["topviewB"])
        T = None
        if prev is not None:
            prev = _cuda_f32(prev, "prev")
            if prev.shape != frames.shape:
                raise ValueError("prev must have the shape of frames")
            T = self.model.predict_poses({("color_aug", 0, 0): frames, ("color_aug", -1, 0): prev}, frame_ids=[0, -1])[("cam_T_cam", 0, -1)]
        return Perception(disp, depth, layout, T)

    def stream(self, src_hw, **kw):
        """A `PerceptionStream` (apis/stream.py) over this model with this Perceiver's output size and depth range: raw uint8
        camera frames of src_hw = (h, w) pushed one by one; keywords go to the session (cameras, capacity, bev_map, depth_bev, objects, ...)."""
        from .stream import PerceptionStream
        return PerceptionStream(self.model, src_hw, **{**dict(out_size=self.out_size, min_depth=self.min_depth, max_depth=self.max_depth), **kw})

    @torch.no_grad()
    def perceive_video(self, frames, batch=8) -> VideoPerception:
        """frames (n,3,H,W) in temporal order, worked off in chunks of `batch`; frame k's predecessor is frame k-1 (also across
        chunk borders), frame 0 has none."""
        frames = _cuda_f32(frames, "frames")
        n, batch = frames.shape[0], int(batch)
        if n < 1 or batch < 1:
            raise ValueError("need at least one frame and batch >= 1")
        depth, layout, poses = [], [], []
        for s in range(0, n, batch):
            e = min(n, s + batch)
            if s == 0:
                p = self.perceive(frames[0:e])
                if e > 1:           # frame 0 has no predecessor: poses of frames 1..e-1 only
                    poses.append(self.model.predict_poses({("color_aug", 0, 0): frames[1:e], ("color_aug", -1, 0): frames[0:e - 1]},
                                                          frame_ids=[0, -1])[("cam_T_cam", 0, -1)])
            else:
                p = self.perceive(frames[s:e], frames[s - 1:e - 1])
                poses.append(p.cam_T_cam)
            depth.append(p.depth)
            layout.append(p.layout)
        T = torch.cat(poses) if poses else torch.empty((0, 4, 4), device=frames.device)
        traj = np.tile(np.identity(4), (n, 1, 1))
        Th = T.cpu().numpy().astype(np.float64)
        for k in range(1, n):
            traj[k] = traj[k - 1] @ Th[k - 1]
        return VideoPerception(torch.cat(depth), torch.cat(layout), T, traj)
