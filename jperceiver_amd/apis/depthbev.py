"""Depth lifted into the layout's BEV grid, and a per-frame score of how far the depth head and the layout head agree, on the device
(csrc/depthbev.hip) -- the inverse of the training-time warp that takes the BEV distance map into the image:

    db = DepthBev(cameras=1, occ=256, K=K, src_hw=(375, 1242), depth_hw=(1024, 1024))      # K: pixel intrinsics of the camera frames
    p = Perceiver(model).perceive(frame)
    db.lift(p.depth)                                        # grid (cameras, 4, occ, occ) int32: [n, n_obst, hmin_mm, hmax_mm] per cell
    db.classes()                                            # (cameras, occ, occ) uint8: 1 ground, 2 obstacle, 255 not observed
    db.height()                                             # (cameras, occ, occ) float: highest point over the cell in metres, NaN = not observed
    agreement_scores(db.agreement(p.layout))                # road_on_ground, car_on_obstacle, observed -- plain ratios on the host

    s = PerceptionStream(model, src_hw, depth_bev=dict(K=K))   # the same per push: s.depth_bev is the live DepthBev

Conventions (the header has them in full): the cells are the layout's own -- cell (i, j) covers x in [(j - occ/2), (j + 1 - occ/2)) * 40 / occ
and forward distances [(occ - 1 - i), (occ - i)) * 40 / occ - off (off: 0.27 for KITTI, 1.9 for split == "argo").  The ground plane is
the CALLER's unless `ground` is given (below): height above ground of a camera-frame point P is h - n . P, with (n, h) = `plane`, or from `cam_height` and
`pitch_deg` (positive: the camera looks down; n = (0, cos, sin)); 1.73 m is the reference's KITTI HEIGHT_FROM_GROUND, an Argoverse
caller passes its own.  A pixel counts when its depth lies in [min_range, max_range], its height in [h_min, h_max] and it falls on the
grid; it is an obstacle point when its height exceeds obst_h.  classes(), height() and agreement() return the object's STATIC buffers
(.cls, .hgt, .agree), overwritten by the next call -- clone what has to live longer.  No method synchronises.

THE GROUND PLANE FROM DEPTH (csrc/ground.hip; opt-in: ground=True or a dict of GROUND_DEFAULTS entries).  A vehicle pitches a degree
or three under braking and over crests -- at 30 m that is 0.5 to 1.5 m of apparent height against a fixed plane, more than obst_h --
so the plane can be fitted per frame from the depth map itself, on the device, into the camera rows the lift reads:

    db = DepthBev(1, 256, K, src_hw, depth_hw, ground=True)
    db.fit_ground(p.depth, p.layout).lift(p.depth)          # one jp_ground_fit call, then the lift under the fitted plane
    g = db.ground()                                         # host: plane, height, n, rms, status, pitch_deg, roll_deg, height_ratio

`rounds` times: every pixel within `band` of the current plane (and, with use_layout, over a road cell of the layout) is quantised
to integer millimetres and summed into ten int64 moments (no atomics; the same bits whatever `parts`, the workgroups per camera),
and the least-squares plane Y = a X + b Z + c is solved in float64 in the order the header states.  The first round gates with the
constructor's plane `plane0` (track=False: every call is a function of its inputs alone) or with the plane the call before left
(track=True).  A fit is rejected -- the plane stays -- with fewer than min_points inliers (status 1), with a spread below
min_spread metres along x or z or nearly collinear points (2), or when it is not finite, tilted more than max_tilt_deg or its
height leaves [h_lo, h_hi] (3).  height_ratio = fitted / nominal camera height is the absolute-scale check of the depth head that
needs no LiDAR.  In a session, depth_bev=dict(K=..., ground=True) fits in every push, between the layout and the lift.

Not built: temporal smoothing of the plane, RANSAC, any use of the plane by `BevMap`, fusing lifted maps into a `BevMap` (its vote
kernel counts a 255 cell as seen), occlusion reasoning beyond "not observed" (the cells behind an obstacle are simply 255)."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops

_INT_MAX, _INT_MIN = 2 ** 31 - 1, -2 ** 31


def _cam_rows(cameras, K, src_hw, depth_hw, cam_height, pitch_deg, plane):
    """-> (cameras, 8) float64 numpy [fx, fy, cx, cy, nx, ny, nz, h]: K scaled from src_hw to depth_hw, the plane as given"""
    K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    if K.ndim == 2:
        K = np.broadcast_to(K, (cameras,) + K.shape)
    if K.ndim != 3 or K.shape[0] != cameras or K.shape[1:] not in ((3, 3), (4, 4)):
        raise ValueError(f"K must be (3, 3), (4, 4) or (cameras, ., .) with cameras = {cameras}, got {K.shape}")
    (h, w), (OH, OW) = src_hw, depth_hw
    rows = np.zeros((cameras, 8), dtype=np.float64)
    rows[:, 0], rows[:, 2] = K[:, 0, 0] * (OW / w), K[:, 0, 2] * (OW / w)
    rows[:, 1], rows[:, 3] = K[:, 1, 1] * (OH / h), K[:, 1, 2] * (OH / h)
    if plane is None:
        a = math.radians(float(pitch_deg))
        plane = (0.0, math.cos(a), math.sin(a), float(cam_height))
    plane = np.asarray(plane, dtype=np.float64)
    if plane.shape not in ((4,), (cameras, 4)):
        raise ValueError(f"plane must be (nx, ny, nz, h) or (cameras, 4), got {plane.shape}")
    rows[:, 4:] = plane
    if not (np.isfinite(rows).all() and (rows[:, :2] != 0).all()):
        raise ValueError("K and the plane must be finite, fx and fy non-zero")
    return rows


GROUND_DEFAULTS = dict(rounds=2, band=0.3, use_layout=True, track=False, parts=256, min_points=200, min_spread=0.5, max_tilt_deg=10.0,
                       h_lo=0.5, h_hi=4.0)
GROUND_STATUS = {-1: "no fit yet", 0: "accepted", 1: "too few points", 2: "ill-conditioned", 3: "out of bounds"}


def _ground_kw(ground):
    """None -> None (no fit); True -> the defaults; a dict -> the defaults with its entries, checked"""
    if ground is None or ground is False:
        return None
    if not (ground is True or isinstance(ground, dict)):
        raise TypeError("ground must be None, True or a dict of " + ", ".join(GROUND_DEFAULTS))
    kw = dict(GROUND_DEFAULTS)
    if ground is not True:
        unknown = sorted(set(ground) - set(kw))
        if unknown:
            raise TypeError(f"ground: unknown entries {unknown}; known: {', '.join(GROUND_DEFAULTS)}")
        kw.update(ground)
    for k in ("rounds", "parts", "min_points"):
        kw[k] = int(kw[k])
    for k in ("band", "min_spread", "max_tilt_deg", "h_lo", "h_hi"):
        kw[k] = float(kw[k])
    kw["use_layout"], kw["track"] = bool(kw["use_layout"]), bool(kw["track"])
    if kw["rounds"] < 1 or not 1 <= kw["parts"] <= 1024:
        raise ValueError("ground: rounds must be positive and parts lie in 1 .. 1024")
    if not kw["band"] > 0.0:
        raise ValueError("ground: band must be greater than zero")
    return kw


class DepthBev:
    """cameras: depth maps lifted side by side; occ: side of the grid in cells (it covers 40 m x 40 m, the layout's); K: (3, 3), (4, 4) or
    (cameras, ., .) pixel intrinsics of the camera frames of size src_hw = (h, w); depth_hw: (OH, OW) of the depth maps (default
    src_hw) -- fx, cx are scaled by OW / w and fy, cy by OH / h; cam_height, pitch_deg or plane, off, the ranges, obst_h: see the
    module docstring; min_points: points a cell needs to count as observed; obst_points: obstacle points that make it an obstacle;
    ground: None (the plane stays the constructor's: no fit, no buffers for one), True or a dict of GROUND_DEFAULTS entries
    (`fit_ground`, `ground`; module docstring).  `plane0` keeps the constructor's plane, (cameras, 4) float64 on the device."""

    def __init__(self, cameras, occ, K, src_hw, depth_hw=None, cam_height=1.73, pitch_deg=0.0, plane=None, off=0.27, min_range=1.0,
                 max_range=40.0, h_min=-1.0, h_max=3.0, obst_h=0.3, min_points=1, obst_points=2, device="cuda", ground=None):
        self.ground_kw = _ground_kw(ground)
        self.cameras, self.occ = int(cameras), int(occ)
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.depth_hw = self.src_hw if depth_hw is None else (int(depth_hw[0]), int(depth_hw[1]))
        if self.cameras < 1 or self.occ < 1 or min(self.src_hw) < 1 or min(self.depth_hw) < 1:
            raise ValueError("cameras, occ, src_hw and depth_hw must be positive")
        self.res_f = 40.0 / self.occ
        self.off, self.min_range, self.max_range = float(off), float(min_range), float(max_range)
        self.h_min, self.h_max, self.obst_h = float(h_min), float(h_max), float(obst_h)
        if not (abs(self.h_min) <= 1e6 and abs(self.h_max) <= 1e6):
            raise ValueError("|h_min| and |h_max| must not exceed 1e6 (heights are kept in int32 millimetres)")
        self.min_points, self.obst_points = int(min_points), int(obst_points)
        rows = _cam_rows(self.cameras, K, self.src_hw, self.depth_hw, cam_height, pitch_deg, plane)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("device must be a CUDA device (the kernels are HIP: no CPU path)")
        B, dev = self.cameras, self.device
        self.cam = torch.from_numpy(rows).to(dev)
        self.grid = torch.empty((B, 4, self.occ, self.occ), device=dev, dtype=torch.int32)
        self.cls = torch.empty((B, self.occ, self.occ), device=dev, dtype=torch.uint8)
        self.hgt = torch.empty((B, self.occ, self.occ), device=dev, dtype=torch.float32)
        self.agree = torch.empty((B, 2, 3), device=dev, dtype=torch.int32)
        self.plane0 = torch.from_numpy(np.ascontiguousarray(rows[:, 4:])).to(dev)          # the constructor's plane: prior, reset value
        if self.ground_kw is not None:
            if not 0.0 < self.max_range <= 1000.0:
                raise ValueError("ground: max_range must lie in (0, 1000] (points are kept in int32 millimetres)")
            self.part = torch.empty((B, self.ground_kw["parts"], 10), device=dev, dtype=torch.int64)
            self.mom = torch.empty((B, 10), device=dev, dtype=torch.int64)
            self.stat = torch.empty((B, 3), device=dev, dtype=torch.float64)
        self.reset()

    def reset(self):
        """Empties the grid ([0, 0, INT_MAX, INT_MIN] per cell) and the outputs derived from it (not observed, NaN, zero counts); with
        `ground` the plane goes back to the constructor's and the fit's outputs to "no fit yet" (status -1, n 0, rms NaN)."""
        self.grid[:, :2] = 0
        self.grid[:, 2] = _INT_MAX
        self.grid[:, 3] = _INT_MIN
        self.cls.fill_(255)
        self.hgt.fill_(float("nan"))
        self.agree.zero_()
        if self.ground_kw is not None:
            self.cam[:, 4:] = self.plane0
            self.mom.zero_()
            self.stat[:, 0], self.stat[:, 1], self.stat[:, 2] = -1.0, 0.0, float("nan")

    # ------------------------------------------------------------------------------------------ the launches
    def _lift(self, depth, accumulate):
        H, W = self.depth_hw
        ops.call("jp_depth_bev_lift", depth, self.cam, self.grid, self.cameras, H, W, self.occ, self.res_f, self.off, self.min_range,
                 self.max_range, self.h_min, self.h_max, self.obst_h, 1 if accumulate else 0)

    def _classes(self, want_height):
        ops.call("jp_depth_bev_classes", self.grid, self.cls, self.hgt if want_height else None, self.cameras, self.occ * self.occ,
                 self.min_points, self.obst_points)

    def _agree(self, layout):
        ops.call("jp_bev_agree", self.cls, layout, self.agree, self.cameras, self.occ * self.occ)

    def _fit(self, depth, layout):
        g = self.ground_kw
        H, W = self.depth_hw
        ops.call("jp_ground_fit", depth, layout if g["use_layout"] else None, None if g["track"] else self.plane0, self.cam, self.part,
                 self.mom, self.stat, self.cameras, H, W, self.occ, self.res_f, self.off, self.min_range, self.max_range, g["band"],
                 g["rounds"], g["parts"], g["min_points"], g["min_spread"], g["max_tilt_deg"], g["h_lo"], g["h_hi"])

    # ------------------------------------------------------------------------------------------ the interface
    def lift(self, depth, accumulate=False):
        """depth: (cameras, 1, OH, OW) -- or (cameras, OH, OW) -- float32 device metres.  Replaces the grid by this depth map's points,
        or adds them to it (accumulate=True: several sweeps, several cameras of one rig given the same plane).  Returns self."""
        if not (isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype == torch.float32):
            raise TypeError("depth must be a float32 CUDA tensor (the kernels are HIP: no CPU path)")
        want = (self.cameras,) + self.depth_hw
        if tuple(depth.shape) not in (want, (self.cameras, 1) + self.depth_hw):
            raise ValueError(f"depth must be (cameras, 1, OH, OW) = {(self.cameras, 1) + self.depth_hw}, got {tuple(depth.shape)}")
        self._lift(depth.contiguous(), accumulate)
        return self

    def fit_ground(self, depth, layout=None):
        """Needs `ground`.  depth as for `lift`; layout: (cameras, occ, occ) uint8 device classes, required with use_layout (only
        pixels over its road cells count).  One jp_ground_fit call: `rounds` gate-and-fit rounds, from the constructor's plane
        (track=False) or from the plane the last call left (track=True); an accepted fit replaces cam[:, 4:], which the next `lift`
        reads, a rejected one leaves the starting plane there.  Returns self; `ground()` reads the result."""
        g = getattr(self, "ground_kw", None)
        if g is None:
            raise RuntimeError("fit_ground needs DepthBev(ground=True) or ground=dict(...)")
        if not (isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype == torch.float32):
            raise TypeError("depth must be a float32 CUDA tensor (the kernels are HIP: no CPU path)")
        if tuple(depth.shape) not in ((self.cameras,) + self.depth_hw, (self.cameras, 1) + self.depth_hw):
            raise ValueError(f"depth must be (cameras, 1, OH, OW) = {(self.cameras, 1) + self.depth_hw}, got {tuple(depth.shape)}")
        if g["use_layout"]:
            if layout is None:
                raise ValueError("ground: use_layout needs the layout (pass it, or build with ground=dict(use_layout=False))")
            if not (isinstance(layout, torch.Tensor) and layout.is_cuda and layout.dtype == torch.uint8):
                raise TypeError("layout must be a uint8 CUDA tensor (the kernels are HIP: no CPU path)")
            if tuple(layout.shape) != (self.cameras, self.occ, self.occ):
                raise ValueError(f"layout must be (cameras, occ, occ) = {(self.cameras, self.occ, self.occ)}, got {tuple(layout.shape)}")
            layout = layout.contiguous()
        self._fit(depth.contiguous(), layout)
        return self

    def ground(self):
        """Host helper (it copies the plane and the status back: the one synchronising step of the fit).  -> dict of arrays, one
        entry per camera: plane (cameras, 4) [nx, ny, nz, h] as the lift will read it, height = h, n = inliers of the last round,
        rms in metres (NaN unless accepted), status (GROUND_STATUS: -1 no fit yet, 0 accepted, 1 too few points, 2 ill-conditioned,
        3 out of bounds), pitch_deg = degrees(atan2(nz, ny)) (positive: the camera looks down), roll_deg = degrees(atan2(nx, ny)),
        height_ratio = h / the constructor's h -- the absolute-scale check of the depth head."""
        if getattr(self, "ground_kw", None) is None:
            raise RuntimeError("ground needs DepthBev(ground=True) or ground=dict(...)")
        plane = self.cam[:, 4:].cpu().numpy()
        stat = self.stat.cpu().numpy()
        h0 = self.plane0[:, 3].cpu().numpy()
        return {"plane": plane, "height": plane[:, 3].copy(), "n": stat[:, 1].astype(np.int64), "rms": stat[:, 2].copy(),
                "status": stat[:, 0].astype(np.int64),
                "pitch_deg": np.degrees(np.arctan2(plane[:, 2], plane[:, 1])), "roll_deg": np.degrees(np.arctan2(plane[:, 0], plane[:, 1])),
                "height_ratio": plane[:, 3] / h0}

    def classes(self):
        """(cameras, occ, occ) uint8: 255 where n < min_points; 2 where n_obst >= obst_points; else 1 -- in this order."""
        self._classes(False)
        return self.cls

    def height(self):
        """(cameras, occ, occ) float32: the highest accepted point over the cell in metres above the plane, NaN where not observed."""
        self._classes(True)
        return self.hgt

    def agreement(self, layout):
        """layout: (cameras, occ, occ) uint8 device classes (0 background, 1 road, 2 car).  -> (cameras, 2, 3) int32 device counts:
        [l - 1][c] = cells whose lifted class is l (1 ground, 2 obstacle) and whose layout class is c; see `agreement_scores`."""
        if not (isinstance(layout, torch.Tensor) and layout.is_cuda and layout.dtype == torch.uint8):
            raise TypeError("layout must be a uint8 CUDA tensor (the kernels are HIP: no CPU path)")
        if tuple(layout.shape) != (self.cameras, self.occ, self.occ):
            raise ValueError(f"layout must be (cameras, occ, occ) = {(self.cameras, self.occ, self.occ)}, got {tuple(layout.shape)}")
        self._classes(False)
        self._agree(layout.contiguous())
        return self.agree


def agreement_scores(counts, cells=None):
    """Host helper (it copies `counts` back: the one synchronising step, the caller's choice of when).  counts: (..., 2, 3) from
    `DepthBev.agreement`, tensor or array; cells: cells per camera for `observed` (default: NaN).  -> dict of float arrays shaped
    like the leading dimensions (floats for one table), each NaN where its denominator is 0:
      road_on_ground  = ground & road / (ground & road + obstacle & road): of the road cells depth sees, the share it sees as ground
      car_on_obstacle = obstacle & car / (obstacle & car + ground & car):  of the car cells depth sees, the share where something stands
      observed        = cells counted / cells"""
    c = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.float64)
    if c.shape[-2:] != (2, 3):
        raise ValueError(f"counts must be (..., 2, 3), got {c.shape}")

    def ratio(a, b):
        with np.errstate(all="ignore"):
            r = np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)
        return float(r) if r.ndim == 0 else r

    total = c.sum((-2, -1))
    n = np.full(total.shape, 0.0 if cells is None else float(cells))
    return {"road_on_ground": ratio(c[..., 0, 1], c[..., 0, 1] + c[..., 1, 1]),
            "car_on_obstacle": ratio(c[..., 1, 2], c[..., 1, 2] + c[..., 0, 2]),
            "observed": ratio(total, n)}
