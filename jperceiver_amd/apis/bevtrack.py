"""BEV object tracks: the objects of `BevObjects` associated from one frame to the next on the device (csrc/bevtrack.hip), with the
ego-motion taken out by the session's float64 poses -- which car is which, for how long it has been seen and how it moves:

    bo, tr = BevObjects(cameras=1, occ=256), BevTracker(cameras=1, occ=256)   # max_objects=64, reach=1, min_overlap=1
    for frame, pose in drive:                               # pose: (cameras, 4, 4) float64 camera-to-world on the device
        tr.update(bo.find(layout_of(frame)), pose)          # one jp_bev_tracks call; .tracks_i, .kin, .stats are device buffers
        for t in tr.tracks(dt=0.1)[0]:                      # the one synchronising read: a list of dicts per camera, in object-id order
            t["id"], t["track"], t["age"], t["X_w"], t["Z_w"], t["speed"]

    s = PerceptionStream(model, src_hw, objects=dict(track=True))        # the same per push, behind jp_stream_traj_push: s.tracks

Conventions (the header has them in full): every cell of a current object is carried to the world with the current pose and back into
the previous frame with the stored previous pose; the cells of the previous label map within `reach` of where it lands vote for the
pair (previous object, current object).  Pairs are matched greedily by their votes -- largest first, ties to the smaller previous
id, then the smaller current id -- until the best is below `min_overlap`.  A matched object keeps its track id and ages by one; an
unmatched one is born with the camera's next id, in object-id order; a track ends in the first frame it is not matched.  Objects
with an id at or above max_objects are not tracked.  The state of the previous frame lives in device buffers of the tracker that the
call itself rolls forward: `update` never synchronises, every call has the same arguments, and the outputs are pure functions of the
inputs and the state.  .tracks_i (cameras, max_objects, 4) int32 [track_id, age, prev_obj, overlap], .kin (cameras, max_objects, 4)
float64 [X_w, Z_w, dX_w, dZ_w] and .stats (cameras, 4) int32 [n_cur, matched, born, ended] are STATIC buffers, valid until the next
`update` -- clone what has to live longer.

Coasting a track through a missed frame, the repair of an id switch and a filter on the motion are a stage of their own behind this
one: `BevTrackFilter` (apis/bevfilter.py; in a session objects=dict(track=dict(filter=True))).

Not built: split and merge bookkeeping beyond what greedy
overlap gives (of two objects that merge, one track goes on and the other ends; of one that splits, one part keeps the id and the
other is born), association across cameras, tracks on the world-frame `BevMap`, any drawing."""
from __future__ import annotations

import math

import torch

from .. import ops
from .._lib import lib as _jplib

TRACK_DEFAULTS = dict(reach=1, min_overlap=1)


def _check(max_objects, reach, min_overlap, off):
    if not 1 <= int(max_objects) <= 256:
        raise ValueError("max_objects must lie in 1 .. 256 (the overlap matrix and the rounds of the assignment grow with its square)")
    if not 0 <= int(reach) <= 3:
        raise ValueError("reach must lie in 0 .. 3")
    if int(min_overlap) < 1:
        raise ValueError("min_overlap must be at least 1")
    if not math.isfinite(float(off)):
        raise ValueError("off must be finite")


def _track_kw(track):
    """None / False -> None (no tracking); True -> {}; a dict -> a copy, its keys (reach, min_overlap) and values checked; the entry
    `filter` (None, a bool or a dict of `BevTrackFilter` keyword arguments: apis/bevfilter.py) is the session's and stays in the copy"""
    if track is None or track is False:
        return None
    if not (track is True or isinstance(track, dict)):
        raise TypeError("track must be None, a bool or a dict of BevTracker keyword arguments (" + ", ".join(TRACK_DEFAULTS) + ")")
    kw = {} if track is True else dict(track)
    unknown = sorted(set(kw) - set(TRACK_DEFAULTS) - {"filter"})
    if unknown:
        raise TypeError(f"track: unknown entries {unknown}; known: {', '.join(TRACK_DEFAULTS)}, filter")
    if "filter" in kw:
        from .bevfilter import _filter_kw
        _filter_kw(kw["filter"])
    _check(1, off=0.0, **{**TRACK_DEFAULTS, **{k: v for k, v in kw.items() if k != "filter"}})
    return kw


class BevTracker:
    """cameras, occ, max_objects: those of the `BevObjects` it follows (occ <= 1024, max_objects <= 256); reach: half side of the
    neighbourhood of previous cells a current cell votes for (0 .. 3); min_overlap: votes a pair needs to be matched; off: see
    apis/bevobj.py (0.27 for KITTI, 1.9 for split == "argo")."""

    def __init__(self, cameras, occ, max_objects=64, reach=1, min_overlap=1, off=0.27, device="cuda"):
        _check(max_objects, reach, min_overlap, off)
        self.cameras, self.occ = int(cameras), int(occ)
        if self.cameras < 1 or self.occ < 1:
            raise ValueError("cameras and occ must be positive")
        if self.occ > 1024:
            raise ValueError("occ must not exceed 1024 (the limit of BevObjects)")
        self.max_objects, self.reach, self.min_overlap = int(max_objects), int(reach), int(min_overlap)
        self.off, self.res_f = float(off), 40.0 / self.occ
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("device must be a CUDA device (the kernels are HIP: no CPU path)")
        B, M, dev = self.cameras, self.max_objects, self.device
        self._prev_labels = torch.empty((B, self.occ, self.occ), device=dev, dtype=torch.int32)
        self._state_i = torch.empty((B, 2 + 2 * M), device=dev, dtype=torch.int32)
        self._state_d = torch.empty((B, 12 + 2 * M), device=dev, dtype=torch.float64)
        self.tracks_i = torch.empty((B, M, 4), device=dev, dtype=torch.int32)
        self.kin = torch.empty((B, M, 4), device=dev, dtype=torch.float64)
        self.stats = torch.empty((B, 4), device=dev, dtype=torch.int32)
        self._ws = torch.empty((int(_jplib().fn["jp_bev_tracks_ws_bytes"](B, self.occ, M)),), device=dev, dtype=torch.uint8)
        self.reset()

    def reset(self):
        """No history: the state is zeroed (the next update gives every object a new track, ids from 0); no tracks in the outputs."""
        for t in (self._prev_labels, self._state_i, self._state_d, self.kin, self.stats):
            t.zero_()
        self.tracks_i.copy_(torch.tensor([-1, 0, -1, 0], dtype=torch.int32, device=self.device).expand_as(self.tracks_i))

    def _update(self, labels, count, table, pose, pose_stride):
        ops.call("jp_bev_tracks", labels, count, table, pose, pose_stride, self._prev_labels, self._state_i, self._state_d, self.tracks_i,
                 self.kin, self.stats, self._ws, self.cameras, self.occ, self.max_objects, self.reach, self.min_overlap, self.off)

    def update(self, objects, pose):
        """objects: a `BevObjects` of the same cameras, occ and max_objects, after its `find`; pose: (cameras, 4, 4), (cameras, 16) or
        (cameras, 12) float64 camera-to-world on the device.  Enqueues the one call, never synchronises; returns self."""
        for n in ("labels", "count", "table"):
            t = getattr(objects, n, None)
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32):
                raise TypeError("objects must be a BevObjects (labels, count and table int32 CUDA tensors; the kernels are HIP: no CPU path)")
        got = (int(objects.labels.shape[0]), int(objects.labels.shape[-1]), int(objects.table.shape[1]))
        if got != (self.cameras, self.occ, self.max_objects):
            raise ValueError(f"objects has (cameras, occ, max_objects) = {got}, this BevTracker {(self.cameras, self.occ, self.max_objects)}")
        if not (isinstance(pose, torch.Tensor) and pose.is_cuda and pose.dtype == torch.float64):
            raise TypeError("pose must be a float64 CUDA tensor (the kernels are HIP: no CPU path)")
        if tuple(pose.shape) not in ((self.cameras, 4, 4), (self.cameras, 16), (self.cameras, 12)):
            raise ValueError(f"pose must be (cameras, 4, 4), (cameras, 16) or (cameras, 12) with cameras = {self.cameras}, got {tuple(pose.shape)}")
        self._update(objects.labels.contiguous(), objects.count.contiguous(), objects.table.contiguous(), pose.contiguous(),
                     12 if pose.shape[-1] == 12 else 16)
        return self

    def stats_host(self):
        """Host helper (synchronises): per camera a dict n_cur, matched, born, ended of the last update."""
        return [dict(zip(("n_cur", "matched", "born", "ended"), row)) for row in self.stats.cpu().tolist()]

    def tracks(self, dt=None):
        """The one synchronising read: stats, tracks_i and kin are copied back.  -> a list per camera of dicts in object-id order:
        id, track, age, prev_id (-1 for a birth), overlap, X_w, Z_w, dX_w, dZ_w (metres, float64) and speed = hypot(dX_w, dZ_w) / dt
        in metres per second with dt (the seconds between two frames), metres per frame without; None for age == 1."""
        if dt is not None and not float(dt) > 0.0:
            raise ValueError("dt must be greater than zero")
        stats, tr, kin = self.stats.cpu().tolist(), self.tracks_i.cpu().tolist(), self.kin.cpu().tolist()
        out = []
        for b in range(self.cameras):
            rows = []
            for i in range(stats[b][0]):
                (track, age, prev, ov), (X, Z, dX, dZ) = tr[b][i], kin[b][i]
                speed = None if age == 1 else math.hypot(dX, dZ) / (1.0 if dt is None else float(dt))
                rows.append({"id": i, "track": track, "age": age, "prev_id": prev, "overlap": ov, "X_w": X, "Z_w": Z, "dX_w": dX,
                             "dZ_w": dZ, "speed": speed})
            out.append(rows)
        return out
