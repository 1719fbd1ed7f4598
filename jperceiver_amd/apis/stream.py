"""Streaming perception: one object that takes raw camera frames one by one and answers with depth, the bird's-eye-view class
map, the ego-motion of the frame and the running trajectory -- what the reference's demo (scripts/eval_kitti_video.py:
`transform()`, `predict()` and the chaining at :281-292) does per frame with host numpy, a kept `prev` image and a kept global
pose, here on the device end to end:

    s = PerceptionStream(model, src_hw=(375, 1242))        # or Perceiver(model).stream((375, 1242))
    for frame in camera:                                    # (cameras, h, w, 3) uint8, host or device
        f = s.push(frame)                                   # StreamFrame(index, disp, depth, layout, cam_T_cam, pose)
    s.trajectory()                                          # (cameras, n, 12) float64, rows 0..2 of every global pose

What one push runs, on the current stream:  DevicePreprocessor.resize_u8 (the Pillow-exact Lanczos resize + ToTensor)  ->  the
model's eval forward (frozen by default, apis.freeze; Baseline.eval_branch: without the Softmax2d maps and the published extras
nothing here reads)  ->  jp_stream_pose_pair (the frame resized to 192 x 640, paired with its predecessor out of a two-slot ring;
with itself for the first frame, as the demo does)  ->  PoseEncoder, PoseDecoder, jp_pose_fwd(invert)  ->  disp_resize_depth,
layout_classes  ->  jp_stream_traj_push (T_k = T_{k-1} @ cam_T_cam_k in float64, T_0 = I).  "Previous frame" and "trajectory
row k" are decided by a frame counter in DEVICE memory: every launch of a push has the same arguments for every frame, nothing is
copied back, and the host never reads the counter (it mirrors the count).  `push` never synchronises.  Against
Perceiver.perceive(cur, prev) the previous frame is resized for the pose nets once instead of twice, and the results are the same
bits.  Weights that change between pushes are picked up as by any eval forward (the frozen state's and the pack registry's host
checks run in every push).

THE RETURNED TENSORS ARE THE SESSION'S STATIC OUTPUT BUFFERS: they are valid until the next `push` (or `reset`), which
overwrites them in place -- clone what has to live longer.

Frames in pinned host memory are copied without blocking: the caller must leave that buffer untouched until the copy has run
(an event recorded after `push`, or any later synchronisation, tells).

bev_map=True (or a dict of BevMap keyword arguments): every push ends with one more launch, jp_bev_fuse, which votes the frame's
layout into a world-frame map with the pose jp_stream_traj_push has just finished (apis/bevmap.py).  `s.bev_map` is the live `BevMap`
-- it accumulates, it is not a per-frame static buffer -- and exists after the first push, which tells the layouts' size.  The
default (None) adds nothing to a push.

depth_bev=dict(K=..., ...) (keyword arguments of `DepthBev`, apis/depthbev.py; K, the pixel intrinsics of the camera frames, is
required): every push enqueues three more launches with the same arguments for every frame -- jp_depth_bev_lift (its fill
included) behind jp_disp_resize_depth, jp_depth_bev_classes behind jp_layout_classes_u8 and jp_bev_agree after that.
`s.depth_bev` is the live `DepthBev`; its `.grid`, `.cls` and `.agree` are static buffers with the lifetime of the other
outputs.  `off` defaults from model.opt.split, `occ` is model.opt.occ_map_size, the depth maps are `out_size`.  The default
(None) adds nothing to a push.

depth_bev=dict(K=..., ground=True) (or ground=dict(...), the `ground` argument of `DepthBev`): the ground plane is fitted from
every frame's depth (and, with use_layout, the road cells of its layout) before the lift measures heights against it.  The order
of a push becomes jp_layout_classes_u8 -> jp_ground_fit -> jp_depth_bev_lift -> jp_depth_bev_classes -> jp_bev_agree: the lift
moves behind the layout, in this kind of session only, and every launch still has fixed arguments (the plane travels in device
memory).  `s.depth_bev.ground()` reads the live plane, its status and the height ratio (the one synchronising step).

objects=True (or a dict of `BevObjects` keyword arguments: max_objects, min_cells, conn, cls, off; apis/bevobj.py): the layout part
of every push ends with one jp_bev_objects call -- the connected components of the car cells, numbered and measured -- behind
jp_layout_classes_u8, and in a depth_bev session behind the lift, whose grid it is given (points and height per object).
`s.objects` is the live `BevObjects`; its `.labels`, `.count` and `.table` are static buffers with the lifetime of the other
outputs, `s.objects.objects(pose=frame.pose)` is the synchronising read.  `off` defaults from model.opt.split.  The default (None)
adds nothing to a push.

objects=dict(track=True) (or track=dict(reach=..., min_overlap=...), next to the other entries; apis/bevtrack.py): the pose part of
every push ends with one jp_bev_tracks call behind jp_stream_traj_push -- it reads the pose that launch has just finished, and the
labels and table jp_bev_objects left earlier on the same stream -- which gives every object a track id that lasts while the object
stays in view, its age and its world-frame displacement.  `s.tracks` is the live `BevTracker`; `.tracks_i`, `.kin` and `.stats` are
static buffers with the lifetime of the other outputs, `s.tracks.tracks(dt)` is the synchronising read.  Without `track` a push is
what it was.

objects=dict(track=dict(filter=True)) (or filter=dict(max_tracks, max_coast, min_hits, gate, meas_sigma, vel_sigma0, accel_sigma), next
to reach and min_overlap; apis/bevfilter.py): every push then ends its pose part with one jp_bev_track_filter call directly behind
jp_bev_tracks -- persistent ids that coast through missed frames, a life cycle and a filtered world-frame velocity per track.
`s.track_filter` is the live `BevTrackFilter` (None otherwise); `.slots_i`, `.slots_d`, `.obj_slot` and `.fstats` are static buffers,
`s.track_filter.tracks(dt)` is the synchronising read; `reset()` resets it with the tracker.  Without `filter` a push is what it was."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .. import ops
from ..datasets.preprocess import DevicePreprocessor
from ..ops import Var

_PH, _PW = 192, 640          # the pose nets' input (net.py:632)


class StreamFrame(NamedTuple):
    index: int                              # 0 for the first frame after construction / reset()
    disp: torch.Tensor                      # (cameras,1,h,w)   the network's ("disp", 0, 0) head, in [0,1]
    depth: torch.Tensor                     # (cameras,1,OH,OW) metres
    layout: torch.Tensor                    # (cameras,occ,occ) uint8: 0 background, 1 road, 2 car
    cam_T_cam: Optional[torch.Tensor]       # (cameras,4,4) transform for frame -1; None for index 0
    pose: torch.Tensor                      # (cameras,4,4) float64 global pose: I for index 0, then pose @ cam_T_cam


class PerceptionStream:
    """See the module docstring.  model: an eval-mode `Baseline` on the GPU that holds a checkpoint; src_hw: (h, w) of the camera
    frames; out_size: (OH, OW) of the depth maps (default: the network's resolution); min_depth / max_depth default to
    model.opt's; capacity: trajectory rows kept per camera (later frames still update `pose`); bev_map: None, True or a dict of
    `BevMap` keyword arguments (`off` defaults from model.opt.split, `occ` is the layouts'); depth_bev: None or a dict of
    `DepthBev` keyword arguments with at least K (`off` defaults from model.opt.split; cameras, occ, src_hw, depth_hw and device
    are the session's); objects: None, True or a dict of `BevObjects` keyword arguments (`off` defaults from model.opt.split;
    cameras, occ and device are the session's) and, optionally, track: True or a dict of `BevTracker`'s reach and min_overlap and, optionally,
    filter: True or a dict of `BevTrackFilter` keyword arguments."""

    def __init__(self, model, src_hw, cameras=1, out_size=None, min_depth=None, max_depth=None, capacity=4096, frozen=True,
                 bev_map=None, depth_bev=None, objects=None):
        if not (bev_map is None or bev_map is True or isinstance(bev_map, dict)):
            raise TypeError("bev_map must be None, True or a dict of BevMap keyword arguments")
        if not (depth_bev is None or isinstance(depth_bev, dict)):
            raise TypeError("depth_bev must be None or a dict of DepthBev keyword arguments (K is required)")
        if depth_bev is not None and "K" not in depth_bev:
            raise ValueError("depth_bev needs K, the pixel intrinsics of the camera frames")
        if depth_bev is not None and depth_bev.get("ground") is not None:
            from .depthbev import _ground_kw
            _ground_kw(depth_bev["ground"])                           # a malformed `ground` is refused before anything else is looked at
        if objects is not None:
            from .bevobj import _objects_kw
            objects = _objects_kw(objects)                            # ... and so is a malformed `objects`, its `track` included
        if model.training:
            raise RuntimeError("PerceptionStream expects an eval-mode model (call .eval(): BatchNorm must use running stats)")
        p = next(model.parameters())
        if not p.is_cuda:
            raise RuntimeError("PerceptionStream runs HIP kernels: move the model to the GPU first (there is no CPU path)")
        h, w = int(src_hw[0]), int(src_hw[1])
        self.cameras, self.capacity = int(cameras), int(capacity)
        if h < 1 or w < 1 or self.cameras < 1 or self.capacity < 1:
            raise ValueError("src_hw, cameras and capacity must be positive")
        if frozen:
            from .inference import freeze
            freeze(model)
        self.model, self.dev, self.src_hw = model, p.device, (h, w)
        self.net_hw = (int(model.opt.height), int(model.opt.width))
        self.out_size = self.net_hw if out_size is None else (int(out_size[0]), int(out_size[1]))
        self.min_depth = float(model.opt.min_depth if min_depth is None else min_depth)
        self.max_depth = float(model.opt.max_depth if max_depth is None else max_depth)
        B, dev = self.cameras, self.dev
        self._pre = DevicePreprocessor(self.net_hw[0], self.net_hw[1], dev)
        self._in = torch.zeros((B, h, w, 3), device=dev, dtype=torch.uint8)
        self._ring = torch.zeros((2, B, 3, _PH, _PW), device=dev)
        self._count = torch.zeros(1, device=dev, dtype=torch.int32)
        self._pose = torch.zeros((B, 16), device=dev, dtype=torch.float64)
        self._traj = torch.zeros((B, self.capacity, 12), device=dev, dtype=torch.float64)
        self._T = torch.zeros((B, 4, 4), device=dev)
        self._K = torch.eye(4, device=dev).repeat(B, 1, 1)            # only T is read (P = K @ T is jp_pose_fwd's by-product)
        self._P = torch.empty((B, 3, 4), device=dev)
        self._depth = torch.empty((B, 1) + self.out_size, device=dev)
        self._disp = self._layout = None                              # shaped by the first pass
        self._n = 0
        self._bev_kw = None if bev_map is None else dict(bev_map if isinstance(bev_map, dict) else {})
        if self._bev_kw is not None:
            self._bev_kw.setdefault("off", 1.9 if getattr(model.opt, "split", None) == "argo" else 0.27)
        self.bev_map = None                                           # the live BevMap: made by the first push of a bev_map session
        self.depth_bev = None                                         # the live DepthBev of a depth_bev session
        if depth_bev is not None:
            from .depthbev import DepthBev
            kw = {"off": 1.9 if getattr(model.opt, "split", None) == "argo" else 0.27, **depth_bev}
            kw.update(cameras=B, occ=int(model.opt.occ_map_size), src_hw=self.src_hw, depth_hw=self.out_size, device=dev)
            self.depth_bev = DepthBev(**kw)
        self.objects = None                                           # the live BevObjects of an objects session
        self.tracks = None                                            # the live BevTracker of an objects session with `track`
        self.track_filter = None                                      # the live BevTrackFilter of a `track` session with `filter`
        if objects is not None:
            from .bevobj import BevObjects
            from .bevtrack import BevTracker, _track_kw
            kw = {"off": 1.9 if getattr(model.opt, "split", None) == "argo" else 0.27, **objects}
            track = _track_kw(kw.pop("track", None))
            self.objects = BevObjects(B, int(model.opt.occ_map_size), device=dev, **kw)
            if track is not None:
                from .bevfilter import BevTrackFilter, _filter_kw
                flt = _filter_kw(track.pop("filter", None), self.objects.max_objects)
                self.tracks = BevTracker(B, self.objects.occ, max_objects=self.objects.max_objects, off=self.objects.off, device=dev, **track)
                if flt is not None:
                    self.track_filter = BevTrackFilter(B, max_objects=self.objects.max_objects, occ=self.objects.occ, device=dev, **flt)

    # ---------------------------------------------------------------------------------------- state
    def reset(self):
        """Forget the stream: the next frame is frame 0 again (paired with itself, pose = I, trajectory row 0)."""
        for t in (self._count, self._ring, self._pose, self._traj, self._T):
            t.zero_()
        if self.bev_map is not None:
            self.bev_map.reset()
        if self.depth_bev is not None:
            self.depth_bev.reset()
        if self.objects is not None:
            self.objects.reset()
        if self.tracks is not None:
            self.tracks.reset()
        if self.track_filter is not None:                             # with the tracker: its ids start from 0 again
            self.track_filter.reset()
        self._n = 0

    def trajectory(self):
        """(cameras, n, 12) float64 device tensor, a copy: rows 0..2 of the global pose of every frame pushed so far (at most
        `capacity` of them), T_0 = I and T_k = T_{k-1} @ cam_T_cam_k."""
        return self._traj[:, :min(self._n, self.capacity)].clone()

    def _check_frames(self, frames):
        if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8):
            raise TypeError("frames must be a uint8 tensor (raw camera frames; the session resizes and scales them itself)")
        want = (self.cameras,) + self.src_hw + (3,)
        if tuple(frames.shape) != want:
            raise ValueError(f"frames must have shape (cameras, h, w, 3) = {want}, got {tuple(frames.shape)}")
        if frames.is_cuda and frames.device != self.dev:
            raise ValueError(f"frames live on {frames.device}, the session on {self.dev}")

    # ---------------------------------------------------------------------------------------- one frame
    def _body(self):
        """The launches of one push, on the current stream."""
        m, B, dev = self.model, self.cameras, self.dev
        H, W = self.net_hw
        img = self._pre.resize_u8(self._in, H, W)
        x = Var(img)
        feats = m.eval_branch("depth_encoder", x)
        disp = m.eval_branch("depth_decoder", feats)
        if self._disp is None:
            self._disp = torch.empty_like(disp)
        h, w = disp.shape[2:]
        ops.call("jp_axpby", disp, None, self._disp, disp.numel(), 1.0, 0.0)
        ops.call("jp_disp_resize_depth", self._disp, self._depth, None, B, h, w, self.out_size[0], self.out_size[1],
                 self.min_depth, self.max_depth)
        db = self.depth_bev
        fit = db is not None and db.ground_kw is not None              # a ground session: the lift waits for the fit, the fit for the layout
        if db is not None and not fit:
            db._lift(self._depth, False)
        road, car = m.eval_branch("layout_heads", m.eval_branch("layout_encoder", x), feats[-1])
        h, w = road.shape[2:]
        if self._layout is None:
            self._layout = torch.empty((B, h, w), device=dev, dtype=torch.uint8)
        ops.call("jp_layout_classes_u8", road, car, self._layout, None, B, h * w)
        if db is not None:
            if (h, w) != (db.occ, db.occ):
                raise ValueError(f"depth_bev: the layouts are {h} x {w}, model.opt.occ_map_size says {db.occ}")
            if fit:
                db._fit(self._depth, self._layout)
                db._lift(self._depth, False)
            db._classes(False)
            db._agree(self._layout)
        if self.objects is not None:
            if (h, w) != (self.objects.occ, self.objects.occ):
                raise ValueError(f"objects: the layouts are {h} x {w}, model.opt.occ_map_size says {self.objects.occ}")
            self.objects._find(self._layout, None if db is None else db.grid)      # behind the layout, and behind the lift
        pair = torch.empty((B, 6, _PH, _PW), device=dev)
        # (no magnitude slot: the pose encoder normalises the pair into a new tensor first (ops.affine), and the stem convolution
        # reduces the magnitude of THAT input itself where its kernel reads one -- nothing reads max |pair|)
        ops.call("jp_stream_pose_pair", img, self._ring, self._count, pair, None, B, H, W)
        aa, tr = m.eval_branch("pose", Var(pair))
        ops.call("jp_pose_fwd", aa.t, tr.t, self._K, self._T, self._P, B, 1)
        ops.call("jp_stream_traj_push", self._T, self._pose, self._traj, self._count, B, self.capacity)
        if self.tracks is not None:                                   # behind traj_push (the pose) and behind jp_bev_objects (labels, table)
            self.tracks._update(self.objects.labels, self.objects.count, self.objects.table, self._pose, 16)
            if self.track_filter is not None:                         # directly behind jp_bev_tracks: it reads tracks_i, kin and stats
                self.track_filter._update(self.tracks.tracks_i, self.tracks.kin, self.tracks.stats)
        if self._bev_kw is not None:
            if self.bev_map is None:
                if h != w:
                    raise ValueError(f"bev_map needs square layouts, the model's are {h} x {w}")
                from .bevmap import BevMap
                self.bev_map = BevMap(B, h, **{**self._bev_kw, "device": dev})
            self.bev_map._fuse(self._layout, self._pose, 16, 1)       # behind traj_push: the pose it reads is finished

    @torch.no_grad()
    def push(self, frames_u8) -> StreamFrame:
        """frames_u8: (cameras, h, w, 3) uint8, on the session's device or on the host (pinned host memory is copied without
        blocking and must stay untouched until that copy has run).  Enqueues the frame's work and returns the static output
        buffers; never waits for the device."""
        if self.model.training:
            raise RuntimeError("PerceptionStream expects an eval-mode model")
        self._check_frames(frames_u8)
        with torch.cuda.device(self.dev):
            self._in.copy_(frames_u8, non_blocking=True)
            ops.PackRegistry.of(self.dev).refresh_all()
            self._body()
        k = self._n
        self._n += 1
        return StreamFrame(k, self._disp, self._depth, self._layout, self._T if k > 0 else None, self._pose.view(-1, 4, 4))
