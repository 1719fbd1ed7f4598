"""World-frame BEV map: the ego-centred class maps of a drive placed in one map with the drive's float64 poses, on the device
(csrc/bevmap.hip):

    m = BevMap(cameras=1, occ=256)                          # 2048 x 2048 cells of 40 / occ metres, world (0, 0) at the centre
    v = Perceiver(model).perceive_video(frames)
    m.fuse(v.layout, v.trajectory)                          # votes [seen, road, car] per map cell, accumulated over calls
    m.classes()                                             # (cameras, Mh, Mw) uint8: 0 background, 1 road, 2 car, 255 not seen
    m.rgb(trajectory=v.trajectory)                          # palette image with the cells the camera passed through marked

    s = PerceptionStream(model, src_hw, bev_map=True)       # the same per push, behind jp_stream_traj_push: s.bev_map is the live map

Conventions (the header has them in full): world is the frame of the first camera pose (T_0 = I), +X goes to increasing columns
and +Z (forward) to decreasing rows, world (0, 0) sits at cell coordinates `origin` = (org_r, org_c).  A layout's row i ends at the
forward distance (occ - i) * 40 / occ - off of the network's own distance map (off: 0.27 for KITTI, 1.9 for split == "argo").  The BEV
plane is taken to be the camera's own x-z plane: the camera's height above the ground is not projected in.  Not built: motion gating
of a stationary car, any handling of moving vehicles (their votes smear along their path), map scrolling (a pose outside the map
simply adds nothing)."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops

_MARK = (255, 0, 0)                  # trajectory marks of BevMap.rgb


def _cuda_u8(x, name):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8):
        raise TypeError(f"{name} must be a uint8 CUDA tensor (the kernels are HIP: no CPU path)")
    return x.contiguous()


class BevMap:
    """cameras: maps kept side by side (one per camera); occ: side of the layouts in cells (they cover 40 m x 40 m);
    cells: (Mh, Mw) of the map; res: metres per map cell (default 40 / occ, the layouts' own); origin: (org_r, org_c) cell
    coordinates of world (0, 0) (default: the map centre); off, max_range: see the module docstring / jp_bev_fuse."""

    def __init__(self, cameras, occ, cells=(2048, 2048), res=None, origin=None, off=0.27, max_range=40.0, device="cuda"):
        self.cameras, self.occ = int(cameras), int(occ)
        self.cells = (int(cells[0]), int(cells[1]))
        if self.cameras < 1 or self.occ < 1 or min(self.cells) < 1:
            raise ValueError("cameras, occ and cells must be positive")
        self.res_f = 40.0 / self.occ
        self.res = self.res_f if res is None else float(res)
        if not self.res > 0:
            raise ValueError("res must be greater than zero")
        self.origin = (self.cells[0] / 2.0, self.cells[1] / 2.0) if origin is None else (float(origin[0]), float(origin[1]))
        self.off, self.max_range = float(off), float(max_range)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("device must be a CUDA device (the kernels are HIP: no CPU path)")
        self.counts = torch.zeros((self.cameras, 3) + self.cells, device=self.device, dtype=torch.int32)

    def reset(self):
        """Zeroes the counts."""
        self.counts.zero_()

    def cell_of(self, X, Z):
        """Host helper: (row, col) of the map cell that holds world (X, Z) -- jp_bev_map_mark's formula; the cell may lie off the map."""
        return (int(math.floor(self.origin[0] - float(Z) / self.res)), int(math.floor(float(X) / self.res + self.origin[1])))

    # ------------------------------------------------------------------------------------------ fusing
    def _poses(self, poses, name="poses"):
        """-> (contiguous float64 device tensor (cameras, N, stride), stride)"""
        if isinstance(poses, np.ndarray):
            if poses.dtype != np.float64:
                raise TypeError(f"{name} must be float64 (host numpy or a CUDA tensor)")
            poses = torch.from_numpy(np.ascontiguousarray(poses)).to(self.device)
        if not (isinstance(poses, torch.Tensor) and poses.is_cuda and poses.dtype == torch.float64):
            raise TypeError(f"{name} must be a float64 CUDA tensor or host numpy array (the kernels are HIP: no CPU path)")
        if poses.dim() >= 2 and tuple(poses.shape[-2:]) == (4, 4):
            poses = poses.reshape(poses.shape[:-2] + (16,))
        stride = int(poses.shape[-1]) if poses.dim() >= 1 else 0
        if stride not in (12, 16):
            raise ValueError(f"{name} must be (..., 4, 4) or (..., 12)")
        if poses.dim() == 2 and self.cameras == 1:
            poses = poses.unsqueeze(0)
        if poses.dim() != 3 or poses.shape[0] != self.cameras:
            raise ValueError(f"{name} must hold (cameras, N) = ({self.cameras}, N) poses, got {tuple(poses.shape)}")
        return poses.contiguous(), stride

    def _fuse(self, layouts, poses, stride, N):
        Mh, Mw = self.cells
        ops.call("jp_bev_fuse", layouts, poses, stride, N, self.counts, self.cameras, self.occ, self.res_f, self.off, self.max_range,
             Mh, Mw, self.res, self.origin[0], self.origin[1])

    def fuse(self, layouts, poses):
        """layouts: (cameras, N, occ, occ) -- or (N, occ, occ) for one camera -- uint8 device classes; poses: (..., 4, 4) or (..., 12)
        float64 camera-to-world transforms, on the device or as host numpy: what perceive_video returns (.layout, .trajectory) and
        what a session gives (cloned frame layouts, .trajectory()).  Adds the frames' votes to `counts`; never waits for the device."""
        layouts = _cuda_u8(layouts, "layouts")
        if layouts.dim() == 3 and self.cameras == 1:
            layouts = layouts.unsqueeze(0)
        if layouts.dim() != 4 or layouts.shape[0] != self.cameras or tuple(layouts.shape[2:]) != (self.occ, self.occ):
            raise ValueError(f"layouts must be (cameras, N, occ, occ) = ({self.cameras}, N, {self.occ}, {self.occ}), got {tuple(layouts.shape)}")
        poses, stride = self._poses(poses)
        N = int(layouts.shape[1])
        if poses.shape[1] != N:
            raise ValueError(f"{N} layouts per camera but {poses.shape[1]} poses")
        if N == 0:
            return self
        per = max(1, 65535 // self.cameras)                 # jp_bev_fuse: B * N <= 65535 per launch
        for s in range(0, N, per):
            e = min(N, s + per)
            whole = s == 0 and e == N
            self._fuse(layouts if whole else layouts[:, s:e].contiguous(), poses if whole else poses[:, s:e].contiguous(), stride, e - s)
        return self

    # ------------------------------------------------------------------------------------------ reading
    def _classes(self, min_seen, road_frac, car_frac, want_rgb):
        Mh, Mw = self.cells
        cls = torch.empty((self.cameras, Mh, Mw), device=self.device, dtype=torch.uint8)
        rgb = torch.empty((self.cameras, Mh, Mw, 3), device=self.device, dtype=torch.uint8) if want_rgb else None
        ops.call("jp_bev_map_classes", self.counts, cls, rgb, self.cameras, Mh * Mw, float(min_seen), float(road_frac), float(car_frac))
        return cls, rgb

    def classes(self, min_seen=1, road_frac=0.5, car_frac=0.5):
        """(cameras, Mh, Mw) uint8: 255 where seen < min_seen; 2 where car >= car_frac * seen; 1 where road + car >= road_frac * seen
        (a car stands on road); else 0 -- in this order."""
        return self._classes(min_seen, road_frac, car_frac, False)[0]

    def rgb(self, trajectory=None, min_seen=1, road_frac=0.5, car_frac=0.5, color=_MARK):
        """(cameras, Mh, Mw, 3) uint8: the palette of layout_rgb, (96, 96, 96) where not seen; with a trajectory ((cameras, n, 12) or
        (..., 4, 4) float64, as for `fuse`) the cells it passes through are painted `color`."""
        rgb = self._classes(min_seen, road_frac, car_frac, True)[1]
        if trajectory is not None:
            traj, stride = self._poses(trajectory, "trajectory")
            if stride == 16:
                traj = traj[..., :12].contiguous()
            n = int(traj.shape[1])
            if n > 0:
                Mh, Mw = self.cells
                packed = int(color[0]) | int(color[1]) << 8 | int(color[2]) << 16
                ops.call("jp_bev_map_mark", rgb, self.cameras, Mh, Mw, traj, n, n, self.res, self.origin[0], self.origin[1], packed)
        return rgb
