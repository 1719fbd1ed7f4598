#!/usr/bin/env python
"""Measure the streaming perception session (apis.PerceptionStream) against what a user of the per-frame API does without it
and write profiles/stream_inference.md.

    python tools/stream_bench.py [--out profiles/stream_inference.md] [--hw 1024] [--src 375 1242] [--cameras 1 4]
                                 [--frames 30] [--warmup 3]
    python tools/stream_bench.py --profile [--cameras 1]      # the kernel profile, in a run of its own (prints, writes nothing)

Shape: hw x hw network (default 1024, the project's), uint8 camera frames of 375 x 1242 in pinned host memory, synthetic
weights whose BatchNorm statistics are not the identity, one model per camera count shared by both routes.  Routes, alternated
frame by frame within one process, each keeping its own stream state:
  E   the per-frame API: upload, DevicePreprocessor.resize_u8, Perceiver(frozen=True).perceive(cur, prev), then the demo's
      host chain -- the frame's cam_T_cam copied to the host and T_k = T_{k-1} @ cam_T_cam_k in numpy
  S   PerceptionStream.push
Per-frame latency: host clock around the route's push plus a synchronise; `warmup` frames, then `frames` timed ones; median
(min .. max).  Launch counts: C-ABI entry-point calls of one steady-state frame.  Output check: the largest differences between
S and E over the timed frames' last four.  Nothing here is a threshold; the note records the numbers, also where S is slower.
Needs a GPU: there is no CPU path to fall back to."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jperceiver_amd.apis import Perceiver, PerceptionStream                                   # noqa: E402
from jperceiver_amd.datasets.preprocess import DevicePreprocessor                             # noqa: E402
from tools.frozen_bench import build_model, counted_calls, profiled                           # noqa: E402


class EagerRoute:
    """the per-frame API, frame by frame"""

    def __init__(self, model, hw, cams):
        self.per = Perceiver(model, frozen=True)
        self.pre = DevicePreprocessor(hw, hw, torch.device("cuda"))
        self.hw, self.cams = hw, cams
        self.reset()

    def reset(self):
        self.prev, self.pose = None, np.tile(np.identity(4), (self.cams, 1, 1))

    def push(self, frame_host):
        cur = self.pre.resize_u8(frame_host.cuda(non_blocking=True), self.hw, self.hw)
        p = self.per.perceive(cur, self.prev)
        if p.cam_T_cam is not None:
            self.pose = self.pose @ p.cam_T_cam.cpu().numpy().astype(np.float64)
        self.prev = cur
        return p


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def pose_of(route):
    return route.pose if isinstance(route, EagerRoute) else route._pose.cpu().numpy().reshape(-1, 4, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_inference.md"))
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--src", type=int, nargs=2, default=[375, 1242])
    ap.add_argument("--cameras", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_bench: no GPU")
    h, w = opt.src
    if opt.profile:
        c = opt.cameras[0]
        s = PerceptionStream(build_model(opt.hw, c), (h, w), cameras=c)
        fr = torch.randint(0, 256, (4, c, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).pin_memory()
        for k in range(3):
            s.push(fr[k])
        torch.cuda.synchronize()
        prof = profiled(lambda: s.push(fr[3]))
        print(f"kernel profile of one session frame ({c} camera(s), {opt.hw}x{opt.hw}; the profile records the convolution dispatches "
              "and jp_add_relu): " + "; ".join(f"{k}: {n} launches, {ms:.3f} ms" for k, (n, ms) in sorted(prof.items())))
        return
    n_all = opt.warmup + opt.frames
    lines = ["# Streaming perception: raw frames in, depth / BEV / pose / trajectory out, no host round trip", "",
             f"Written by `tools/stream_bench.py` on {torch.cuda.get_device_name(0)}; {opt.hw}x{opt.hw} network, uint8 frames of {h}x{w} in "
             f"pinned host memory, synthetic weights (BatchNorm statistics not the identity).  Routes: E = upload, `resize_u8`, "
             "`Perceiver(frozen=True).perceive(cur, prev)`, host chain of the pose (the per-frame API); S = `PerceptionStream.push`.  "
             f"Latency: host clock around one push + synchronise, {opt.warmup} warm-up frames, then {opt.frames} timed frames, the routes "
             "alternated frame by frame; median (min .. max).  Calls: C-ABI entry-point calls of one steady-state frame.  Differences: "
             "largest over the last four timed frames, S against E (disp and pose absolute, depth relative, BEV classes as a share of "
             "the pixels).", ""]
    for c in opt.cameras:
        model = build_model(opt.hw, c)
        g = torch.Generator().manual_seed(100 + c)
        frames = torch.randint(0, 256, (n_all, c, h, w, 3), dtype=torch.uint8, generator=g).pin_memory()
        routes = {"E": EagerRoute(model, opt.hw, c), "S": PerceptionStream(model, (h, w), cameras=c)}
        times = {k: [] for k in routes}
        diffs = {k: dict(disp=0.0, depth=0.0, layout=0.0, T=0.0) for k in routes if k != "E"}
        for i in range(n_all):
            outs = {}
            for k, r in routes.items():
                ms, out = wall_ms(lambda r=r: r.push(frames[i]))
                if i >= opt.warmup:
                    times[k].append(ms)
                outs[k] = out
            if i >= n_all - 4:
                e = outs["E"]
                for k in diffs:
                    o, d = outs[k], diffs[k]
                    d["disp"] = max(d["disp"], float((o.disp - e.disp).abs().max()))
                    d["depth"] = max(d["depth"], float(((o.depth - e.depth).abs() / e.depth).max()))
                    d["layout"] = max(d["layout"], float((o.layout != e.layout).float().mean()))
                    d["T"] = max(d["T"], float((o.cam_T_cam - e.cam_T_cam).abs().max()))
        torch.cuda.synchronize()
        dpose = {k: float(np.abs(pose_of(routes[k]) - pose_of(routes["E"])).max()) for k in diffs}
        ncalls = {}
        for k, r in routes.items():
            with counted_calls() as cc:
                r.push(frames[n_all - 1])
            torch.cuda.synchronize()
            ncalls[k] = len(cc.names)
        e_lo, e_hi = min(times["E"]), max(times["E"])
        lines += [f"## {c} camera(s)", "",
                  "| route | ms per frame | vs E (median) | below E's band | C-ABI calls per frame | disp | depth (rel) | BEV classes | cam_T_cam | pose after "
                  f"{n_all} frames |", "|---|---|---|---|---|---|---|---|---|---|"]
        me = statistics.median(times["E"])
        for k in routes:
            t = times[k]
            m = statistics.median(t)
            row = f"| {k} | {m:.3f} ({min(t):.3f} .. {max(t):.3f}) | {m / me:.3f} | "
            row += "- | " if k == "E" else ("yes | " if max(t) < e_lo else ("median only | " if m < e_lo else "no | "))
            row += f"{ncalls[k]} | "
            row += "- | - | - | - | - |" if k == "E" else (f"{diffs[k]['disp']:.2e} | {diffs[k]['depth']:.2e} | {diffs[k]['layout']:.4%} | "
                                                            f"{diffs[k]['T']:.2e} | {dpose[k]:.2e} |")
            lines.append(row)
        lines += ["", f"E's band: {e_lo:.3f} .. {e_hi:.3f} ms.", ""]
        print("\n".join(lines[-10:]), flush=True)
        del routes, model
        import gc
        gc.collect()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
