"""BEV object instances: the connected components of one class of the layout (default: car), numbered and measured on the device
(csrc/bevobj.hip) -- how many vehicles are ahead, where each one is, how large and how far:

    bo = BevObjects(cameras=1, occ=256)                     # max_objects=64, min_cells=4, conn=8, cls=2 (car; 1 = road segments)
    p = Perceiver(model).perceive(frame)
    bo.find(p.layout)                                       # one jp_bev_objects call; .labels, .count, .table are device buffers
    bo.find(p.layout, depth_bev=db)                         # ... with the lifted points and height of every object (DepthBev.grid)
    for o in bo.objects()[0]:                               # the one synchronising read: a list of dicts per camera, in id order
        o["x"], o["z"], o["range"], o["width"], o["length"], o["bearing_deg"], o["truncated"], o["height"]

    s = PerceptionStream(model, src_hw, objects=True)       # the same per push, behind jp_layout_classes_u8: s.objects is the live BevObjects

Conventions (the header has them in full): ids are canonical -- the kept components of a camera are numbered 0, 1, 2, ... in raster
order of their first cell; a component of fewer than min_cells cells (an argmax speck) is dropped before numbering and its cells get
label -1; `count` is the number of kept components even beyond max_objects (`overflowed()`), `labels` carries every id, `table`
(cameras, max_objects, 12) int32 holds FIELDS for the first max_objects.  The cells are the layout's own: cell (i, j) covers x in
[(j - occ/2), (j + 1 - occ/2)) * 40 / occ and forward distances [(occ - 1 - i), (occ - i)) * 40 / occ - off (off: 0.27 for KITTI, 1.9
for split == "argo").  `find` never synchronises and its outputs are pure functions of its inputs; .labels, .count and .table are
STATIC buffers, valid until the next `find` -- clone what has to live longer.

Tracking across frames is `BevTracker` (apis/bevtrack.py; in a session objects=dict(track=True)).

Not built: oriented boxes (width and length are those of the axis-aligned box in
the camera's own BEV frame), splitting vehicles whose cells touch, objects on the world-frame `BevMap`, any drawing of boxes."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from .._lib import lib as _jplib

_INT_MIN = -2 ** 31
FIELDS = ("cells", "r_min", "r_max", "c_min", "c_max", "sum_r", "sum_c", "first_cell", "edge_mask", "pts", "pts_obst", "hmax_mm")
OBJECTS_DEFAULTS = dict(max_objects=64, min_cells=4, conn=8, cls=2, off=0.27)


def _objects_kw(objects):
    """None -> None (no objects); True -> {}; a dict -> a copy, its keys checked (cameras, occ and device are the session's); the
    entry `track` (None, a bool or a dict of reach, min_overlap: apis/bevtrack.py) is the session's and stays in the copy"""
    if objects is None or objects is False:
        return None
    if not (objects is True or isinstance(objects, dict)):
        raise TypeError("objects must be None, True or a dict of BevObjects keyword arguments (" + ", ".join(OBJECTS_DEFAULTS) + ")")
    kw = {} if objects is True else dict(objects)
    unknown = sorted(set(kw) - set(OBJECTS_DEFAULTS) - {"track"})
    if unknown:
        raise TypeError(f"objects: unknown entries {unknown}; known: {', '.join(OBJECTS_DEFAULTS)}, track")
    if "track" in kw:
        from .bevtrack import _check as _check_track, _track_kw, TRACK_DEFAULTS
        tk = _track_kw(kw["track"])
        if tk is not None:                                              # the tracker's table is the objects': its bound on max_objects holds
            _check_track(kw.get("max_objects", OBJECTS_DEFAULTS["max_objects"]), off=kw.get("off", OBJECTS_DEFAULTS["off"]),
                         **{**TRACK_DEFAULTS, **{k: v for k, v in tk.items() if k != "filter"}})
    _check(**{**OBJECTS_DEFAULTS, **{k: v for k, v in kw.items() if k != "track"}})
    return kw


def _check(max_objects, min_cells, conn, cls, off):
    if int(max_objects) < 1 or int(min_cells) < 1:
        raise ValueError("max_objects and min_cells must be at least 1")
    if int(conn) not in (4, 8):
        raise ValueError("conn must be 4 or 8")
    if not 0 <= int(cls) <= 255:
        raise ValueError("cls must lie in 0 .. 255 (the layout holds bytes)")
    if not math.isfinite(float(off)):
        raise ValueError("off must be finite")


def object_metrics(row, occ, off=0.27, pose=None):
    """Host arithmetic of one table row (twelve integers, FIELDS) -> dict, every metric value a Python float (float64):
    x = (sum_c / cells + 0.5 - occ / 2) res_f, z = (occ - 0.5 - sum_r / cells) res_f - off (the centroid of the cell centres),
    width = (c_max - c_min + 1) res_f, length = (r_max - r_min + 1) res_f, range = (occ - 1 - r_max) res_f - off (the near edge),
    bearing_deg = degrees(atan2(x, z)), truncated = edge_mask != 0, height = hmax_mm / 1000 (None for the INT_MIN sentinel); with
    pose (the row-major 3 x 4 or 4 x 4 camera-to-world transform, 12 or 16 floats) also X_w = T[0][0] x + T[0][2] z + T[0][3],
    Z_w = T[2][0] x + T[2][2] z + T[2][3] -- the six elements jp_bev_fuse reads."""
    cells, r_min, r_max, c_min, c_max, sum_r, sum_c, first_cell, edge, pts, pts_obst, hmax = (int(v) for v in row)
    res_f = 40.0 / occ
    x = (sum_c / cells + 0.5 - occ / 2) * res_f
    z = (occ - 0.5 - sum_r / cells) * res_f - off
    out = {"cells": cells, "x": x, "z": z, "width": (c_max - c_min + 1) * res_f, "length": (r_max - r_min + 1) * res_f,
           "range": (occ - 1 - r_max) * res_f - off, "bearing_deg": math.degrees(math.atan2(x, z)), "truncated": edge != 0,
           "points": pts, "obstacle_points": pts_obst, "height": None if hmax == _INT_MIN else hmax / 1000.0}
    if pose is not None:
        T = [float(v) for v in pose]
        out["X_w"] = T[0] * x + T[2] * z + T[3]
        out["Z_w"] = T[8] * x + T[10] * z + T[11]
    return out


class BevObjects:
    """cameras: layouts labelled side by side; occ: side of the layouts in cells (<= 1024; they cover 40 m x 40 m); max_objects: rows
    of the table per camera; min_cells: cells a component needs to be kept; conn: 4 or 8; cls: the layout class that is foreground
    (2 car, 1 road); off: see the module docstring (it only enters `objects()`)."""

    def __init__(self, cameras, occ, max_objects=64, min_cells=4, conn=8, cls=2, off=0.27, device="cuda"):
        _check(max_objects, min_cells, conn, cls, off)
        self.cameras, self.occ = int(cameras), int(occ)
        if self.cameras < 1 or self.occ < 1:
            raise ValueError("cameras and occ must be positive")
        if self.occ > 1024:
            raise ValueError("occ must not exceed 1024 (sum_r is an int32)")
        self.max_objects, self.min_cells, self.conn, self.cls = int(max_objects), int(min_cells), int(conn), int(cls)
        self.off, self.res_f = float(off), 40.0 / self.occ
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("device must be a CUDA device (the kernels are HIP: no CPU path)")
        B, dev = self.cameras, self.device
        self.labels = torch.empty((B, self.occ, self.occ), device=dev, dtype=torch.int32)
        self.count = torch.empty((B,), device=dev, dtype=torch.int32)
        self.table = torch.empty((B, self.max_objects, len(FIELDS)), device=dev, dtype=torch.int32)
        self._ws = torch.empty((int(_jplib().fn["jp_bev_objects_ws_bytes"](B, self.occ)),), device=dev, dtype=torch.uint8)
        self._grid = False                                                 # whether the last find was given a grid
        self.reset()

    def reset(self):
        """No objects: labels -1, count and table zero."""
        self.labels.fill_(-1)
        self.count.zero_()
        self.table.zero_()
        self._grid = False

    def _find(self, layout, grid):
        ops.call("jp_bev_objects", layout, grid, self.labels, self.count, self.table, self._ws, self.cameras, self.occ, self.cls,
                 self.conn, self.min_cells, self.max_objects)
        self._grid = grid is not None

    def find(self, layout, depth_bev=None):
        """layout: (cameras, occ, occ) -- or (cameras, 1, occ, occ) -- uint8 device classes; depth_bev: a `DepthBev` of the same
        cameras and occ whose `.grid` (the last lift) gives every object its points and height.  Enqueues the one call; returns self."""
        if not (isinstance(layout, torch.Tensor) and layout.is_cuda and layout.dtype == torch.uint8):
            raise TypeError("layout must be a uint8 CUDA tensor (the kernels are HIP: no CPU path)")
        want = (self.cameras, self.occ, self.occ)
        if tuple(layout.shape) not in (want, (self.cameras, 1, self.occ, self.occ)):
            raise ValueError(f"layout must be (cameras, occ, occ) = {want}, got {tuple(layout.shape)}")
        grid = None
        if depth_bev is not None:
            grid = getattr(depth_bev, "grid", None)
            if not (isinstance(grid, torch.Tensor) and grid.is_cuda and grid.dtype == torch.int32):
                raise TypeError("depth_bev must be a DepthBev (its .grid an int32 CUDA tensor; the kernels are HIP: no CPU path)")
            if tuple(grid.shape) != (self.cameras, 4, self.occ, self.occ):
                raise ValueError(f"depth_bev has (cameras, occ) = ({grid.shape[0]}, {grid.shape[-1]}), this BevObjects ({self.cameras}, {self.occ})")
            grid = grid.contiguous()
        self._find(layout.contiguous(), grid)
        return self

    def overflowed(self):
        """Host helper (synchronises): per camera, whether more components were kept than the table has rows."""
        return [bool(c > self.max_objects) for c in self.count.cpu().tolist()]

    def objects(self, pose=None):
        """The one synchronising read: count and table are copied back.  -> a list per camera of dicts in id order, at most
        max_objects of them: id, cells, x, z, width, length, range, bearing_deg, truncated, points, obstacle_points, height
        (`object_metrics`; metres and degrees as float64 on the host; points, obstacle_points and height are 0, 0, None after a
        `find` without depth_bev).  pose: (cameras, 4, 4) or (cameras, 12) float64 camera-to-world, tensor or array -- the
        session's `pose` or a trajectory row: every dict also gets X_w, Z_w."""
        T = None
        if pose is not None:
            T = np.asarray(pose.detach().cpu() if isinstance(pose, torch.Tensor) else pose)
            if T.dtype != np.float64:
                raise TypeError("pose must be float64")
            if T.shape == (self.cameras, 4, 4):
                T = T.reshape(self.cameras, 16)
            if T.shape not in ((self.cameras, 12), (self.cameras, 16)):
                raise ValueError(f"pose must be (cameras, 4, 4) or (cameras, 12) with cameras = {self.cameras}, got {T.shape}")
        count = self.count.cpu().tolist()
        table = self.table.cpu().numpy()
        out = []
        for b in range(self.cameras):
            rows = []
            for i in range(min(count[b], self.max_objects)):
                rows.append({"id": i, **object_metrics(table[b, i], self.occ, self.off, None if T is None else T[b])})
            out.append(rows)
        return out
