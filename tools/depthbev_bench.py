#!/usr/bin/env python
"""Measure the depth-to-BEV lift (csrc/depthbev.hip, apis.DepthBev, PerceptionStream(depth_bev=...)) and write profiles/depth_bev.md.

    python tools/depthbev_bench.py [--out profiles/depth_bev.md] [--hw 1024] [--src 375 1242] [--frames 30] [--warmup 3]
                                   [--launches 200] [--rounds 7] [--no-session]

Shape: depth maps of hw x hw (default 1024, the project's), a grid of occ = hw / 4 = 256 cells a side, one camera.
  1. jp_depth_bev_lift as the session calls it (accumulate = 0: the fill launch is part of the call), in both forms of the kernel
     -- JP_DEPTH_BEV_RUNS=0: per-lane atomics, =1: wave-level run aggregation; the library reads the switch at every call -- on two
     scenes: a synthetic road (flat ground below the horizon, sky above, a few boxes standing on the ground) and uniform random
     depth, the worst case for run aggregation (no two neighbouring lanes share a cell).  Device events around `launches`
     back-to-back launches, the two forms alternated round by round, `rounds` rounds, median (min .. max) per call; bytes / time
     against the 4 bytes per pixel the pass has to read.  The atomics each form issues are COUNTED from the scene, by the torch
     restatement of the kernel's keys below: per-lane = 3 per accepted pixel + 1 per obstacle point; runs = 3 per run of equal
     keys inside a 64-lane wave + 1 per run that holds an obstacle point.  The two forms' grids are compared bit for bit.
  2. a session with and without depth_bev on the same model and frames, alternated frame by frame within one process: host clock
     around one push + synchronise, median (min .. max) per frame; C-ABI calls of one steady-state frame.
Nothing here is a threshold.  The default form is the faster one on the road scene; the file records the numbers and names it.
Needs a GPU: there is no CPU path to fall back to; a number that was not taken reads "not measured"."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jperceiver_amd.apis import DepthBev, PerceptionStream                                     # noqa: E402

SWITCH = "JP_DEPTH_BEV_RUNS"
FORMS = (("0", "per-lane atomics"), ("1", "run aggregation"))


def road_scene(hw, fx, cy, h):
    """(1,1,hw,hw) float32: ground plane depth h fy / (v - cy) below the horizon, +Inf (rejected) above, three boxes on the ground"""
    v = torch.arange(hw, dtype=torch.float64)[:, None].expand(hw, hw)
    d = torch.where(v > cy, h * fx / (v - cy).clamp(min=1e-9), torch.full_like(v, float("inf")))
    for z, u0, u1, top in ((8.0, 0.10, 0.27, 1.6), (14.0, 0.55, 0.68, 1.5), (25.0, 0.40, 0.50, 2.8)):
        v0 = int(cy - (top - h) * fx / z)                    # image row of the box's top edge
        box = d[max(v0, 0):, int(u0 * hw):int(u1 * hw)]
        box.copy_(box.clamp(max=z))
    return d.float()[None, None].contiguous()


def random_scene(hw, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 39.0 * torch.rand((1, 1, hw, hw), generator=g)).contiguous()


def count_atomics(depth, db):
    """-> dict: pixels, accepted, atomics issued by each form -- the kernel's keys restated in torch float64 on the device"""
    H, W = db.depth_hw
    c = db.cam[0]
    d = depth.reshape(H, W).double()
    u = torch.arange(W, device=d.device, dtype=torch.float64)[None, :]
    v = torch.arange(H, device=d.device, dtype=torch.float64)[:, None]
    X = (u - c[2]) / c[0] * d
    Y = (v - c[3]) / c[1] * d
    hgt = c[7] - ((c[4] * X + c[5] * Y) + c[6] * d)
    uu = X / db.res_f + 0.5 * db.occ
    vv = (d + db.off) / db.res_f
    ok = (d >= db.min_range) & (d <= db.max_range) & (hgt >= db.h_min) & (hgt <= db.h_max) & (uu >= 0) & (uu < db.occ) & (vv >= 0) & (vv < db.occ)
    key = torch.where(ok, (db.occ - 1 - vv.clamp(0, db.occ).floor()) * db.occ + uu.clamp(0, db.occ).floor(), torch.full_like(d, -1.0)).long()
    key, ob = key.reshape(-1), (ok & (hgt > db.obst_h)).reshape(-1)
    idx = torch.arange(key.numel(), device=key.device)
    head = torch.ones_like(ob)
    head[1:] = key[1:] != key[:-1]
    head |= (idx & 63) == 0                                   # a run ends with its wave
    run = torch.cumsum(head.long(), 0) - 1
    runs = int((head & (key >= 0)).sum())
    ob_runs = int((torch.zeros(int(run[-1]) + 1, device=key.device, dtype=torch.long).scatter_add_(0, run, ob.long()) > 0).sum())
    acc = int(ok.sum())
    return {"pixels": key.numel(), "accepted": acc, "0": 3 * acc + int(ob.sum()), "1": 3 * runs + ob_runs}


def time_lift(db, depth, launches, rounds):
    """-> ({form: [microseconds per call, one per round]}, grids bit-equal)"""
    grids = {}
    for f, _ in FORMS:                                        # warm-up: code objects, clocks
        os.environ[SWITCH] = f
        for _ in range(20):
            db.lift(depth)
        grids[f] = db.grid.clone()
    torch.cuda.synchronize()
    out = {f: [] for f, _ in FORMS}
    for _ in range(rounds):
        for f, _ in FORMS:
            os.environ[SWITCH] = f
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                db.lift(depth)
            e1.record()
            torch.cuda.synchronize()
            out[f].append(e0.elapsed_time(e1) * 1e3 / launches)
    os.environ.pop(SWITCH, None)
    return out, torch.equal(grids["0"], grids["1"])


def fmt(t, nd=2):
    return f"{statistics.median(t):.{nd}f} ({min(t):.{nd}f} .. {max(t):.{nd}f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bev.md"))
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--src", type=int, nargs=2, default=[375, 1242])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-session", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depthbev_bench: no GPU")
    hw, occ = opt.hw, opt.hw // 4
    fx, cx, cy, h = 0.6 * hw, 0.5 * hw, 0.4 * hw, 1.73
    K = np.array([[fx, 0.0, cx], [0.0, fx, cy], [0.0, 0.0, 1.0]])
    db = DepthBev(1, occ, K, (hw, hw), cam_height=h)
    scenes = (("road", road_scene(hw, fx, cy, h).cuda()), ("uniform random", random_scene(hw, 5).cuda()))
    nbytes = 4 * hw * hw
    lines = ["# Depth lifted into the layout's BEV grid: the two forms of jp_depth_bev_lift, and a session with it", "",
             f"Written by `tools/depthbev_bench.py` on {torch.cuda.get_device_name(0)}; depth maps of {hw} x {hw}, grid of {occ} x {occ} cells "
             f"of {40.0 / occ} m, one camera (fx = fy = {fx}, cx = {cx}, cy = {cy}, level, {h} m above the ground).", "",
             "## jp_depth_bev_lift (accumulate = 0: the session's call, the fill launch included)", "",
             f"Device events around {opt.launches} back-to-back calls, the two forms alternated round by round, {opt.rounds} rounds, median "
             f"(min .. max) per call.  GB/s: the {nbytes} bytes of depth the pass reads over the median time.  Atomics: counted from the "
             "scene (per-lane: 3 per accepted pixel + 1 per obstacle point; runs: 3 per run of equal cells inside a wave + 1 per run "
             "with an obstacle point), per pixel of the image.", "",
             "| scene | pixels accepted | form | us per call | GB/s | atomics per pixel | grids bit-equal |", "|---|---|---|---|---|---|---|"]
    road_med = {}
    for name, depth in scenes:
        cnt = count_atomics(depth, db)
        t, same = time_lift(db, depth, opt.launches, opt.rounds)
        for f, label in FORMS:
            med = statistics.median(t[f])
            if name == "road":
                road_med[f] = med
            lines.append(f"| {name} | {cnt['accepted']} of {cnt['pixels']} | {label} ({SWITCH}={f}) | {fmt(t[f])} | {nbytes / (med * 1e-6) / 1e9:.1f} | "
                         f"{cnt[f] / cnt['pixels']:.4f} | {same} |")
    best = min(road_med, key=road_med.get)
    lines += ["", f"Faster on the road scene: **{dict(FORMS)[best]}** ({SWITCH}={best}), {road_med[best]:.2f} us against "
              f"{road_med['1' if best == '0' else '0']:.2f} us -- the form to ship as the default; {SWITCH}={'1' if best == '0' else '0'} selects the other.", ""]
    print("\n".join(lines[-9:]), flush=True)

    if not opt.no_session:
        from tools.frozen_bench import build_model, counted_calls
        from tools.stream_bench import wall_ms
        sh, sw = opt.src
        model = build_model(hw, 1)
        n_all = opt.warmup + opt.frames
        g = torch.Generator().manual_seed(101)
        frames = torch.randint(0, 256, (n_all, 1, sh, sw, 3), dtype=torch.uint8, generator=g).pin_memory()
        Ks = np.array([[0.58 * sw, 0.0, 0.5 * sw], [0.0, 1.92 * sh, 0.46 * sh], [0.0, 0.0, 1.0]])         # KITTI-like
        # (synthetic weights: the depths are no street scene -- fractions of a metre -- so the ranges are opened until points are accepted)
        wide = dict(K=Ks, min_range=0.01, max_range=100.0, h_min=-50.0, h_max=50.0)
        routes = {"without": PerceptionStream(model, (sh, sw)), "with": PerceptionStream(model, (sh, sw), depth_bev=wide)}
        times = {k: [] for k in routes}
        for i in range(n_all):
            for k, r in routes.items():
                ms, _ = wall_ms(lambda r=r: r.push(frames[i]))
                if i >= opt.warmup:
                    times[k].append(ms)
        ncalls = {}
        for k, r in routes.items():
            with counted_calls() as cc:
                r.push(frames[n_all - 1])
            torch.cuda.synchronize()
            ncalls[k] = len(cc.names)
        same = all(torch.equal(getattr(routes["with"], a), getattr(routes["without"], a)) for a in ("_disp", "_depth", "_layout", "_pose", "_traj"))
        pts = int(routes["with"].depth_bev.grid[:, 0].sum())
        lo, hi = min(times["without"]), max(times["without"])
        mw = statistics.median(times["with"])
        lines += ["## A session with and without depth_bev", "",
                  f"uint8 frames of {sh}x{sw} in pinned host memory, synthetic weights, the default form of the lift; host clock around one push "
                  f"+ synchronise, {opt.warmup} warm-up frames, then {opt.frames} timed frames, the two sessions alternated frame by frame; "
                  "median (min .. max).", "", "| session | ms per frame | C-ABI calls per frame |", "|---|---|---|"]
        for k in routes:
            lines.append(f"| {k} depth_bev | {fmt(times[k], 4)} | {ncalls[k]} |")
        lines += ["", f"Without-lift band: {lo:.4f} .. {hi:.4f} ms; the with-lift median {mw:.4f} ms lies "
                  f"{'inside' if lo <= mw <= hi else 'OUTSIDE'} it (difference of the medians: {mw - statistics.median(times['without']):+.4f} ms).  "
                  f"Outputs, pose and trajectory of the two sessions after {n_all + 1} frames bit-equal: {same}; points accepted in the last "
                  f"frame: {pts} of {hw * hw} (synthetic weights: the depths are fractions of a metre, the session's ranges are opened to "
                  "1 cm .. 100 m and +-50 m of height so that they count; they pile onto a few cells).", ""]
        print("\n".join(lines[-8:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
