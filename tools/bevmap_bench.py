#!/usr/bin/env python
"""Measure the world-frame BEV map (csrc/bevmap.hip, apis.BevMap, PerceptionStream(bev_map=...)) and write profiles/bev_map.md.

    python tools/bevmap_bench.py [--out profiles/bev_map.md] [--hw 1024] [--src 375 1242] [--cells 2048 2048] [--frames 30]
                                 [--warmup 3] [--launches 200] [--rounds 7]

Shape: hw x hw network (default 1024, the project's: layouts of occ = hw / 4 = 256 cells), a map of 2048 x 2048 cells of
40 / occ = 0.15625 m, one camera.
  1. jp_bev_fuse alone (N = 1, the session's launch): device events around `launches` back-to-back launches on seeded random
     layouts and poses that stay on the map, `rounds` rounds, median (min .. max) per launch; against the bytes the launch must
     move -- window cells x (1 B gathered + 3 x 4 B read + 3 x 4 B written), an upper bound since only the cells a frame hits are
     touched -- as bytes / time.  A launch this short is bounded by launch overhead, not bandwidth: the rate is what it is.
  2. a session with and without the map on the same model and frames, alternated frame by frame within one process (as
     tools/stream_bench.py alternates its routes): host clock around one push + synchronise, median (min .. max) per frame,
     and whether the with-map median lies inside the without-map band; C-ABI calls of one steady-state frame.
Nothing here is a threshold.  Needs a GPU: there is no CPU path to fall back to; a number that was not taken reads "not measured"."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jperceiver_amd.apis import BevMap, PerceptionStream                                      # noqa: E402
from tools.frozen_bench import build_model, counted_calls                                     # noqa: E402
from tools.stream_bench import wall_ms                                                        # noqa: E402


def window_cells(occ, res_f, res):
    """side of the square window one frame's launch visits (csrc/bevmap.hip)"""
    return int(math.ceil(occ * res_f * math.sqrt(2.0) / res) + 3)


def fuse_bytes(occ, res_f, res):
    w = window_cells(occ, res_f, res)
    return w * w * (1 + 3 * 4 + 3 * 4)


def drive_poses(n, seed):
    """(n, 16) float64: a seeded drive that stays within 60 m of the start, yaw anywhere, pitch and roll <= 0.05 rad"""
    rng = np.random.default_rng(seed)
    out = np.tile(np.identity(4), (n, 1, 1))
    for k in range(n):
        yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)
        cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
        out[k, :3, :3] = Ry @ Rx @ Rz
        out[k, 0, 3], out[k, 2, 3] = rng.uniform(-60, 60), rng.uniform(-60, 60)
    return out.reshape(n, 16)


def time_fuse(occ, cells, launches, rounds):
    """-> list of ms per launch, one per round (device events around `launches` launches)"""
    m = BevMap(1, occ, cells=cells)
    g = torch.Generator().manual_seed(7)
    lay = torch.randint(0, 3, (launches, 1, occ, occ), dtype=torch.uint8, generator=g).cuda()
    poses = torch.from_numpy(drive_poses(launches, 11)).cuda()
    for k in range(min(launches, 20)):                       # warm-up: code object, clocks
        m._fuse(lay[k], poses[k], 16, 1)
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(launches):
            m._fuse(lay[k], poses[k], 16, 1)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / launches)
    assert int(m.counts[:, 0].sum()) > 0
    return out


def fmt(t):
    return f"{statistics.median(t):.4f} ({min(t):.4f} .. {max(t):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_map.md"))
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--src", type=int, nargs=2, default=[375, 1242])
    ap.add_argument("--cells", type=int, nargs=2, default=[2048, 2048])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bevmap_bench: no GPU")
    h, w = opt.src
    occ, cells = opt.hw // 4, tuple(opt.cells)
    res_f = res = 40.0 / occ
    win, nbytes = window_cells(occ, res_f, res), fuse_bytes(occ, res_f, res)
    lines = ["# World-frame BEV map: the stream's layouts voted into one map on the device", "",
             f"Written by `tools/bevmap_bench.py` on {torch.cuda.get_device_name(0)}; {opt.hw}x{opt.hw} network (layouts of {occ} x {occ} "
             f"cells), map of {cells[0]} x {cells[1]} cells of {res} m, one camera.", "",
             "## jp_bev_fuse (N = 1, the session's launch)", "",
             f"Device events around {opt.launches} back-to-back launches (seeded random layouts, poses on the map), {opt.rounds} rounds, "
             "median (min .. max) per launch.  Bytes: window cells x (1 B gathered + 3 x 4 B read + 3 x 4 B written) -- an upper bound, "
             "only the cells a frame hits (at most half the window) are touched.", ""]
    t = time_fuse(occ, cells, opt.launches, opt.rounds)
    med = statistics.median(t)
    lines += ["| window | bytes per launch | ms per launch | bytes / time (median) |", "|---|---|---|---|",
              f"| {win} x {win} cells | {nbytes} ({nbytes / 2 ** 20:.2f} MiB) | {fmt(t)} | {nbytes / (med * 1e-3) / 1e9:.1f} GB/s |", "",
              "Back-to-back launches of this size measure the launch rate as much as the kernel: the figure is a time per enqueued "
              "launch, not a share of the memory bandwidth.", ""]
    print("\n".join(lines[-6:]), flush=True)

    model = build_model(opt.hw, 1)
    n_all = opt.warmup + opt.frames
    g = torch.Generator().manual_seed(101)
    frames = torch.randint(0, 256, (n_all, 1, h, w, 3), dtype=torch.uint8, generator=g).pin_memory()
    routes = {"without": PerceptionStream(model, (h, w)), "with": PerceptionStream(model, (h, w), bev_map=dict(cells=cells))}
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
    seen = int(routes["with"].bev_map.counts[:, 0].sum())
    lo, hi = min(times["without"]), max(times["without"])
    mw = statistics.median(times["with"])
    lines += ["## A session with and without the map", "",
              f"uint8 frames of {h}x{w} in pinned host memory, synthetic weights; host clock around one push + synchronise, {opt.warmup} "
              f"warm-up frames, then {opt.frames} timed frames, the two sessions alternated frame by frame; median (min .. max).", "",
              "| session | ms per frame | C-ABI calls per frame |", "|---|---|---|"]
    for k in routes:
        lines.append(f"| {k} the map | {fmt(times[k])} | {ncalls[k]} |")
    lines += ["", f"Without-map band: {lo:.4f} .. {hi:.4f} ms; the with-map median {mw:.4f} ms lies "
              f"{'inside' if lo <= mw <= hi else 'OUTSIDE'} it (difference of the medians: {mw - statistics.median(times['without']):+.4f} ms).  "
              f"Outputs, pose and trajectory of the two sessions after {n_all + 1} frames bit-equal: {same}; map cells seen: {seen}.", ""]
    print("\n".join(lines[-8:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
