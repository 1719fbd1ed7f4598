#!/usr/bin/env python
"""Measure the BEV object instances (csrc/bevobj.hip, apis.BevObjects, PerceptionStream(objects=...)) and write profiles/bev_objects.md.

    python tools/bevobj_bench.py [--out profiles/bev_objects.md] [--occ 256] [--launches 200] [--rounds 7] [--frames 30] [--warmup 3]
                                 [--hw 1024] [--src 375 1242] [--no-session] [--stats NAME=DIR ...]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/bevobj_bench.py --trace NAME [--cameras 1]

Shape: layouts of occ x occ (default 256, the project's at 1024 x 1024), 1 and 4 cameras.
  1. one `BevObjects.find` (the one jp_bev_objects call: five launches) on
       road / car  : the BEV labels of jperceiver_amd/synthetic.py make_batch -- a road blob of about a third of the cells with two
                     vehicle boxes -- labelled for the car class (the default), 8-connected;
       road / road : the same maps labelled for the road class: one large component;
       percolation : a random map with 0.59 of the cells foreground, 4-connected -- near the site-percolation threshold, the
                     longest union chains a map of this size can hold;
     each without a grid, the first also with one.  Device events around `launches` back-to-back calls, `rounds` rounds, the cases
     alternated round by round; median (min .. max) per call, next to the lift's time (profiles/depth_bev.md) and to the time of one
     pass over the maps at the HBM rate.
  2. --stats NAME=DIR: the kernel times of a rocprofv3 --kernel-trace run of `--trace NAME` (a run of its own, the profiler slows
     the host), which say which phase dominates.
  3. a session with and without `objects` on the same model and frames, alternated frame by frame within one process: host clock
     around one push + synchronise, median (min .. max) per frame; C-ABI calls of one steady-state frame.
Nothing here is a threshold.  Needs a GPU: there is no CPU path to fall back to; a number that was not taken reads "not measured"."""
import argparse
import glob
import os
import re
import sqlite3
import statistics
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jperceiver_amd import synthetic as syn                                                     # noqa: E402
from jperceiver_amd.apis import BevObjects, PerceptionStream                                    # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X peak
LIFT_US = 15.0                    # jp_depth_bev_lift on the road scene, profiles/depth_bev.md
PHASES = ("bevobj_init_kernel", "bevobj_unite_kernel", "bevobj_flatten_kernel", "bevobj_number_kernel", "bevobj_emit_kernel")


def road_layouts(B, occ):
    """(B, occ, occ) uint8: 0 background, 1 road, 2 vehicle -- the BEV labels of the synthetic batch"""
    inp = syn.make_batch(B, 64, 64, frame_ids=(0,), occ=occ, seed=9)
    road, veh = inp[("bothS", 0, 0)][:, 0].numpy(), inp[("bothD", 0, 0)][:, 0].numpy()
    return np.where(veh > 0, 2, np.where(road > 0, 1, 0)).astype(np.uint8)


def percolation_layouts(B, occ, density=0.59):
    rng = np.random.default_rng(59)
    return np.where(rng.random((B, occ, occ)) < density, 2, 0).astype(np.uint8)


def random_grid(B, occ):
    rng = np.random.default_rng(4)
    n = rng.integers(0, 6, size=(B, occ, occ)) * (rng.random((B, occ, occ)) < 0.5)
    hmax = rng.integers(-900, 3000, size=(B, occ, occ))
    return np.stack([n, n // 2, hmax - 100, hmax], axis=1).astype(np.int32)


def cases(B, occ):
    """name -> (BevObjects, layout, depth_bev or None)"""
    road = torch.from_numpy(road_layouts(B, occ)).cuda()
    perc = torch.from_numpy(percolation_layouts(B, occ)).cuda()
    grid = types.SimpleNamespace(grid=torch.from_numpy(random_grid(B, occ)).cuda())
    return {"road / car": (BevObjects(B, occ), road, None),
            "road / car, with a grid": (BevObjects(B, occ), road, grid),
            "road / road": (BevObjects(B, occ, cls=1), road, None),
            "percolation": (BevObjects(B, occ, conn=4), perc, None)}


def time_finds(cs, launches, rounds):
    for bo, lay, g in cs.values():
        for _ in range(20):
            bo.find(lay, depth_bev=g)
    torch.cuda.synchronize()
    out = {k: [] for k in cs}
    for _ in range(rounds):
        for k, (bo, lay, g) in cs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                bo.find(lay, depth_bev=g)
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    return out


def fmt(t, nd=2):
    return f"{statistics.median(t):.{nd}f} ({min(t):.{nd}f} .. {max(t):.{nd}f})"


def kernel_stats(d):
    """{kernel name: (calls, average us)} of the bevobj kernels in the rocpd database of a rocprofv3 output directory"""
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
        try:
            rows = sqlite3.connect(f).execute("select name, count(*), avg(duration) from kernels group by name").fetchall()
        except sqlite3.Error:
            continue
        for name, n, avg in rows:
            name = re.sub(r"\(anonymous namespace\)::", "", name)
            for p in PHASES:
                if name.startswith(p):
                    out[p] = (int(n), float(avg) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_objects.md"))
    ap.add_argument("--occ", type=int, default=256)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--src", type=int, nargs=2, default=[375, 1242])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-session", action="store_true")
    ap.add_argument("--trace", default=None, help="only run `launches` finds of this case (for a profiler run) and exit")
    ap.add_argument("--cameras", type=int, default=1)
    ap.add_argument("--stats", nargs="*", default=[], help="CASE=DIR: rocprofv3 output directories of --trace runs")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bevobj_bench: no GPU")
    occ = opt.occ
    if opt.trace is not None:
        bo, lay, g = cases(opt.cameras, occ)[opt.trace]
        for _ in range(opt.launches):
            bo.find(lay, depth_bev=g)
        torch.cuda.synchronize()
        print(f"traced {opt.launches} finds of '{opt.trace}', {opt.cameras} camera(s): kept {bo.count.cpu().tolist()}")
        return

    lines = ["# BEV object instances: jp_bev_objects, and a session with it", "",
             f"Written by `tools/bevobj_bench.py` on {torch.cuda.get_device_name(0)}; layouts of {occ} x {occ} cells of {40.0 / occ} m.", "",
             "## One `BevObjects.find` (one jp_bev_objects call: five launches)", "",
             f"Device events around {opt.launches} back-to-back calls, the cases alternated round by round, {opt.rounds} rounds, median "
             "(min .. max) per call.  Defaults unless the case says otherwise: max_objects 64, min_cells 4, conn 8, cls 2.  `pass`: the "
             f"time of one pass over the maps at the HBM peak of {HBM_BYTES_PER_S / 1e12:.0f} TB/s -- 1 byte of layout read and 4 bytes of labels written "
             "per cell, 16 more bytes read per cell with a grid.  The maps are far too small for that bound to bind: the call's time is "
             f"launch and dependency latency of five short kernels.  The lift next to it (profiles/depth_bev.md): {LIFT_US:.0f} us.", "",
             "| case | cameras | kept components | us per call | x the lift | pass at the HBM rate, us |", "|---|---|---|---|---|---|"]
    med = {}
    for B in (1, 4):
        cs = cases(B, occ)
        t = time_finds(cs, opt.launches, opt.rounds)
        for k, (bo, lay, g) in cs.items():
            m = statistics.median(t[k])
            med[(k, B)] = m
            nbytes = B * occ * occ * (5 + (16 if g is not None else 0))
            label = k + (", conn 4" if k == "percolation" else "") + (", cls 1" if k == "road / road" else "")
            lines.append(f"| {label} | {B} | {bo.count.cpu().tolist()} | {fmt(t[k])} | {m / LIFT_US:.2f} | {nbytes / HBM_BYTES_PER_S * 1e6:.3f} |")
    print("\n".join(lines[-10:]), flush=True)

    lines += ["", "## The five kernels (rocprofv3 --kernel-trace, a run of its own per case)", ""]
    got = False
    for item in opt.stats:
        name, d = item.split("=", 1)
        st = kernel_stats(d)
        if not st:
            lines += [f"{name}: not measured (no kernel statistics under the directory given).", ""]
            continue
        got = True
        tot = sum(a for _, a in st.values())
        top = max(st, key=lambda p: st[p][1])
        lines += [f"{name}:", "", "| kernel | calls | average us | share |", "|---|---|---|---|"]
        lines += [f"| `{p}` | {st[p][0]} | {st[p][1]:.2f} | {100 * st[p][1] / tot:.0f} % |" for p in PHASES if p in st]
        lines += ["", f"Sum of the averages {tot:.2f} us; the largest is `{top}`.", ""]
    if not got and not opt.stats:
        lines += ["not measured (no --stats directory was given).", ""]

    if not opt.no_session:
        from tools.frozen_bench import build_model, counted_calls
        from tools.stream_bench import wall_ms
        sh, sw = opt.src
        model = build_model(opt.hw, 1)
        n_all = opt.warmup + opt.frames
        g = torch.Generator().manual_seed(101)
        frames = torch.randint(0, 256, (n_all, 1, sh, sw, 3), dtype=torch.uint8, generator=g).pin_memory()
        routes = {"without": PerceptionStream(model, (sh, sw)), "with": PerceptionStream(model, (sh, sw), objects=True)}
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
        kept = routes["with"].objects.count.cpu().tolist()
        cars = int((routes["with"]._layout == 2).sum())
        lo, hi = min(times["without"]), max(times["without"])
        mw, mo = statistics.median(times["with"]), statistics.median(times["without"])
        lines += ["## A session with and without objects", "",
                  f"uint8 frames of {sh}x{sw} in pinned host memory, synthetic weights, network {opt.hw} x {opt.hw}; host clock around one push + "
                  f"synchronise, {opt.warmup} warm-up frames, then {opt.frames} timed frames, the two sessions alternated frame by frame; median "
                  "(min .. max).", "", "| session | ms per frame | C-ABI calls per frame |", "|---|---|---|"]
        for k in routes:
            lines.append(f"| {k} objects | {fmt(times[k], 4)} | {ncalls[k]} |")
        lines += ["", f"Plain-session band: {lo:.4f} .. {hi:.4f} ms; the median with objects, {mw:.4f} ms, lies "
                  f"{'inside' if lo <= mw <= hi else 'OUTSIDE'} it (difference of the medians: {mw - mo:+.4f} ms).  Outputs, pose and "
                  f"trajectory of the two sessions after {n_all + 1} frames bit-equal: {same}; the last layout holds {cars} car cells in "
                  f"{kept} kept components (synthetic weights: no street scene).", ""]
        print("\n".join(lines[-8:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
