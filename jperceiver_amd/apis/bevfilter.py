"""Filtered BEV tracks: a stage behind `BevTracker` (csrc/bevfilter.hip) that turns its frame-to-frame tracks into what a consumer
expects of a tracker -- an id that survives a missed frame and an id switch, a life cycle, and a smoothed world-frame velocity:

    bo, tr = BevObjects(cameras=1, occ=256), BevTracker(cameras=1, occ=256)
    flt = BevTrackFilter(cameras=1, occ=256)                # max_objects=64, max_tracks=128, max_coast=3, min_hits=3, gate=2 m
    for frame, pose in drive:
        flt.update(tr.update(bo.find(layout_of(frame)), pose))          # one jp_bev_track_filter call behind jp_bev_tracks
        for t in flt.tracks(dt=0.1)[0]:                     # the one synchronising read: a list of dicts per camera, in slot order
            t["track"], t["status"], t["X_w"], t["Z_w"], t["vX_w"], t["vZ_w"], t["speed"], t["heading_deg"]

    s = PerceptionStream(model, src_hw, objects=dict(track=dict(filter=True)))   # the same per push: s.track_filter

Conventions (the header has them in full).  A SLOT holds one filtered track: its persistent id (`track`, the fid), the tracker's id
it currently follows, and per world axis a constant-velocity Kalman filter on the object's centroid (position and velocity in metres
and metres per frame, a 2 x 2 covariance).  Per call: every live slot is predicted one frame ahead; an object whose tracker id a slot
follows CONTINUES it; the slots left over -- coasting ones, and those whose tracker track ended in this very frame, the id switch --
RE-ACQUIRE the unclaimed objects within `gate` metres of their predicted position, greedily, nearest first (ties to the smaller
slot, then the smaller object id); the objects still unclaimed are BORN into the slots that were free when the call began, with the
camera's next fid; slots with a measurement are updated, the others coast (status "coasting", the predicted state) for at most
`max_coast` frames and then end; a tentative slot ends at its first miss.  A track is "tentative" until it has had `min_hits`
measurements, then "confirmed".  The state lives in device buffers of the filter that the call itself rolls forward: `update` never
synchronises, every call has the same arguments, the outputs are pure functions of the inputs and the state.  .slots_i (cameras,
max_tracks, 8) int32 [fid, status, src_track, age, hits, misses, obj, 0], .slots_d (cameras, max_tracks, 10) float64 [X, Z, vX, vZ,
aX, bX, cX, aZ, bZ, cZ], .obj_slot (cameras, max_objects) int32 and .fstats (cameras, 8) int32 [live, confirmed, coasting,
continued, reacquired, born, ended, dropped] are STATIC buffers, valid until the next `update` -- clone what has to live longer.
Reset the filter whenever the tracker is reset: the tracker numbers its tracks from 0 again, and stale ids would match them.

The defaults (max_coast 3, min_hits 3, gate 2 m, meas_sigma one cell, vel_sigma0 3 m per frame, accel_sigma 0.5 m per frame^2) are
conventional tracker settings, not measurements on any data set.

Not built: Mahalanobis gating (the gate is a fixed Euclidean distance), measurement noise from the blob's size, camera-frame velocity
and time-to-collision, association across cameras, tracks on the world-frame `BevMap`, any drawing."""
from __future__ import annotations

import math

import torch

from .. import ops

FILTER_DEFAULTS = dict(max_tracks=None, max_coast=3, min_hits=3, gate=2.0, meas_sigma=None, vel_sigma0=3.0, accel_sigma=0.5)
STATUS = ("free", "tentative", "confirmed", "coasting")
FSTATS = ("live", "confirmed", "coasting", "continued", "reacquired", "born", "ended", "dropped")


def _check(max_objects, max_tracks, max_coast, min_hits, gate, meas_sigma, vel_sigma0, accel_sigma):
    """max_tracks and meas_sigma may be None (the constructor's defaults: they depend on max_objects and occ)"""
    if not 1 <= int(max_objects) <= 256:
        raise ValueError("max_objects must lie in 1 .. 256 (the limit of BevTracker, whose rows the filter reads)")
    if max_tracks is not None and not 1 <= int(max_tracks) <= 256:
        raise ValueError("max_tracks must lie in 1 .. 256 (one thread of the camera's workgroup per slot)")
    if int(max_coast) < 0:
        raise ValueError("max_coast must not be negative")
    if int(min_hits) < 1:
        raise ValueError("min_hits must be at least 1")
    for name, v in (("gate", gate), ("vel_sigma0", vel_sigma0), ("accel_sigma", accel_sigma)):
        if not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"{name} must be finite and not negative")
    if meas_sigma is not None and not (math.isfinite(float(meas_sigma)) and float(meas_sigma) > 0.0):
        raise ValueError("meas_sigma must be finite and greater than zero")


def _filter_kw(flt, max_objects=64):
    """None / False -> None (no filter); True -> {}; a dict -> a copy, its keys (FILTER_DEFAULTS) and values checked"""
    if flt is None or flt is False:
        return None
    if not (flt is True or isinstance(flt, dict)):
        raise TypeError("filter must be None, a bool or a dict of BevTrackFilter keyword arguments (" + ", ".join(FILTER_DEFAULTS) + ")")
    kw = {} if flt is True else dict(flt)
    unknown = sorted(set(kw) - set(FILTER_DEFAULTS))
    if unknown:
        raise TypeError(f"filter: unknown entries {unknown}; known: {', '.join(FILTER_DEFAULTS)}")
    _check(max_objects, **{**FILTER_DEFAULTS, **kw})
    return kw


class BevTrackFilter:
    """cameras, max_objects: those of the `BevTracker` it follows (max_objects <= 256); max_tracks: slots per camera (1 .. 256;
    None: min(256, 2 max_objects)); max_coast: frames a confirmed track is carried without a measurement; min_hits: measurements
    that confirm a track; gate: metres between a predicted position and a measurement that may re-acquire it; meas_sigma: the
    standard deviation of a centroid in metres (None: one cell, 40 / occ -- the only use of occ); vel_sigma0: the standard
    deviation of a new track's velocity in metres per frame; accel_sigma: the process noise, metres per frame^2.  The defaults
    are conventional tracker settings, not measurements."""

    def __init__(self, cameras, max_objects=64, max_tracks=None, max_coast=3, min_hits=3, gate=2.0, meas_sigma=None, vel_sigma0=3.0,
                 accel_sigma=0.5, occ=None, device="cuda"):
        _check(max_objects, max_tracks, max_coast, min_hits, gate, meas_sigma, vel_sigma0, accel_sigma)
        self.cameras, self.max_objects = int(cameras), int(max_objects)
        if self.cameras < 1:
            raise ValueError("cameras must be positive")
        if meas_sigma is None:
            if occ is None:
                raise ValueError("meas_sigma or occ is needed (meas_sigma defaults to one cell, 40 / occ)")
            if int(occ) < 1:
                raise ValueError("occ must be positive")
            meas_sigma = 40.0 / int(occ)
        self.max_tracks = min(256, 2 * self.max_objects) if max_tracks is None else int(max_tracks)
        self.max_coast, self.min_hits = int(max_coast), int(min_hits)
        self.gate, self.meas_sigma = float(gate), float(meas_sigma)
        self.vel_sigma0, self.accel_sigma = float(vel_sigma0), float(accel_sigma)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("device must be a CUDA device (the kernels are HIP: no CPU path)")
        B, M, S, dev = self.cameras, self.max_objects, self.max_tracks, self.device
        self.slots_i = torch.empty((B, S, 8), device=dev, dtype=torch.int32)
        self.slots_d = torch.empty((B, S, 10), device=dev, dtype=torch.float64)
        self._head = torch.empty((B, 2), device=dev, dtype=torch.int32)
        self.obj_slot = torch.empty((B, M), device=dev, dtype=torch.int32)
        self.fstats = torch.empty((B, 8), device=dev, dtype=torch.int32)
        self.reset()

    def reset(self):
        """No history: every slot is free and the next births take fids from 0; no tracks in the outputs.  Reset the tracker too."""
        for t in (self.slots_i, self.slots_d, self._head, self.fstats):
            t.zero_()
        self.obj_slot.fill_(-1)

    def _update(self, tracks_i, kin, stats):
        ops.call("jp_bev_track_filter", tracks_i, kin, stats, self.slots_i, self.slots_d, self._head, self.obj_slot, self.fstats,
                 self.cameras, self.max_objects, self.max_tracks, self.max_coast, self.min_hits, self.gate, self.meas_sigma,
                 self.vel_sigma0, self.accel_sigma)

    def update(self, tracker):
        """tracker: a `BevTracker` of the same cameras and max_objects, after its `update`.  Enqueues the one call, never
        synchronises; returns self."""
        want = (("tracks_i", torch.int32), ("kin", torch.float64), ("stats", torch.int32))
        for n, dt in want:
            t = getattr(tracker, n, None)
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt):
                raise TypeError("tracker must be a BevTracker (tracks_i and stats int32, kin float64 CUDA tensors; the kernels are HIP: no CPU path)")
        got = (tuple(tracker.tracks_i.shape), tuple(tracker.kin.shape), tuple(tracker.stats.shape))
        B, M = self.cameras, self.max_objects
        if got != ((B, M, 4), (B, M, 4), (B, 4)):
            raise ValueError(f"tracker has tracks_i, kin, stats of shapes {got}, this BevTrackFilter needs {((B, M, 4), (B, M, 4), (B, 4))}")
        self._update(tracker.tracks_i.contiguous(), tracker.kin.contiguous(), tracker.stats.contiguous())
        return self

    def stats_host(self):
        """Host helper (synchronises): per camera a dict live, confirmed, coasting, continued, reacquired, born, ended, dropped of
        the last update."""
        return [dict(zip(FSTATS, row)) for row in self.fstats.cpu().tolist()]

    def tracks(self, dt=None):
        """The one synchronising read: slots_i and slots_d are copied back.  -> a list per camera of dicts for the live slots in
        slot order: track (the fid), status ("tentative" | "confirmed" | "coasting"), age, hits, misses, id (the current object
        id, -1 while coasting), X_w, Z_w (metres, float64), vX_w, vZ_w and speed = hypot(vX_w, vZ_w) in metres per second with dt
        (the seconds between two frames), per frame without, heading_deg = degrees(atan2(vX_w, vZ_w)) (0: along world +Z), and
        X_sigma, Z_sigma, the filter's own standard deviations of the position in metres."""
        if dt is not None and not float(dt) > 0.0:
            raise ValueError("dt must be greater than zero")
        si, sd = self.slots_i.cpu().tolist(), self.slots_d.cpu().tolist()
        per = 1.0 if dt is None else float(dt)
        out = []
        for b in range(self.cameras):
            rows = []
            for (fid, status, _, age, hits, misses, obj, _), d in zip(si[b], sd[b]):
                if not 1 <= status <= 3:
                    continue
                vX, vZ = d[2] / per, d[3] / per
                rows.append({"track": fid, "status": STATUS[status], "age": age, "hits": hits, "misses": misses, "id": obj, "X_w": d[0],
                             "Z_w": d[1], "vX_w": vX, "vZ_w": vZ, "speed": math.hypot(vX, vZ), "heading_deg": math.degrees(math.atan2(vX, vZ)),
                             "X_sigma": math.sqrt(max(d[4], 0.0)), "Z_sigma": math.sqrt(max(d[7], 0.0))})
            out.append(rows)
        return out
