#!/usr/bin/env python
"""Measure the BEV object tracks (csrc/bevtrack.hip, apis.BevTracker, PerceptionStream(objects=dict(track=True))) and write
profiles/bev_tracks.md.

    python tools/bevtrack_bench.py [--out profiles/bev_tracks.md] [--occ 256] [--launches 200] [--rounds 7] [--frames 30] [--warmup 3]
                                   [--hw 1024] [--src 375 1242] [--no-session]

Shape: layouts of occ x occ (default 256, the project's at 1024 x 1024), max_objects 64, 1 and 4 cameras.
  1. one `BevTracker.update` (the one jp_bev_tracks call: four launches) on two scenes, each a pair of frames the tracker is fed in
     turn, so that every timed call has a previous frame to match against:
       road        : the synthetic road scene of tools/bevobj_bench.py (two vehicle boxes), and the same scene two rows nearer and
                     one column to the right under the pose of a camera that drove 2 cells forward and 1 cell to the left -- the
                     known ego-motion: every object is matched and its world displacement is zero;
       percolation : a random map with 0.59 of the cells foreground, 4-connected (hundreds of components, the first 64 tracked),
                     and the same map shifted, identity poses: the most votes a map of this size gives;
     in the three forms of the vote (JP_BEV_TRACKS_VOTE: 0 an atomic per vote, 1 wave-local runs, 2 runs into an LDS tile of the
     matrix), with `jp_bev_objects` on the same layouts timed beside it in the same process.  Device events around `launches`
     back-to-back calls, `rounds` rounds, the cases alternated round by round; median (min .. max) per call.
  2. a plain session, an objects=True session and an objects=dict(track=True) session on the same model and frames, alternated
     frame by frame within one process: host clock around one push + synchronise, median (min .. max) per frame; C-ABI calls of
     one steady-state frame.
Nothing here is a threshold.  Needs a GPU: there is no CPU path to fall back to; a number that was not taken reads "not measured"."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jperceiver_amd.apis import BevObjects, BevTracker, PerceptionStream                        # noqa: E402
from tools.bevobj_bench import fmt, percolation_layouts, road_layouts                            # noqa: E402

VOTES = {"0": "an atomic per vote", "1": "wave-local runs", "2": "runs into an LDS tile (default)"}


def shifted(m, di, dj):
    """(B, occ, occ) moved by di rows and dj columns, background where the map enters"""
    occ = m.shape[-1]
    out = np.zeros_like(m)
    out[:, max(di, 0):occ + min(di, 0), max(dj, 0):occ + min(dj, 0)] = m[:, max(-di, 0):occ + min(-di, 0), max(-dj, 0):occ + min(-dj, 0)]
    return out


def scenes(B, occ):
    """name -> [(BevObjects after find, layout, pose)] x 2: the pair of frames the tracker is fed in turn"""
    res_f = 40.0 / occ
    eye = torch.eye(4, dtype=torch.float64, device="cuda").repeat(B, 1, 1)
    moved = eye.clone()
    moved[:, 0, 3], moved[:, 2, 3] = -res_f, 2.0 * res_f             # the camera drove 2 cells forward and 1 to the left
    road, perc = road_layouts(B, occ), percolation_layouts(B, occ)
    out = {}
    for name, maps, poses, kw in (("road", (road, shifted(road, 2, 1)), (eye, moved), {}),
                                  ("percolation", (perc, shifted(perc, 1, -1)), (eye, eye), dict(conn=4))):
        pair = []
        for m, T in zip(maps, poses):
            lay = torch.from_numpy(m).cuda()
            pair.append((BevObjects(B, occ, **kw).find(lay), lay, T))
        out[name] = pair
    return out


def time_calls(cases, launches, rounds):
    """cases: name -> (callable that enqueues one call, environment value of JP_BEV_TRACKS_VOTE or None)"""
    for fn, env in cases.values():
        _setenv(env)
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (fn, env) in cases.items():
            _setenv(env)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    _setenv(None)
    return out


def _setenv(v):
    if v is None:
        os.environ.pop("JP_BEV_TRACKS_VOTE", None)
    else:
        os.environ["JP_BEV_TRACKS_VOTE"] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_tracks.md"))
    ap.add_argument("--occ", type=int, default=256)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--src", type=int, nargs=2, default=[375, 1242])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-session", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bevtrack_bench: no GPU")
    occ = opt.occ
    lines = ["# BEV object tracks: jp_bev_tracks, and a session with it", "",
             f"Written by `tools/bevtrack_bench.py` on {torch.cuda.get_device_name(0)}; layouts of {occ} x {occ} cells of {40.0 / occ} m, "
             "max_objects 64, reach 1, min_overlap 1.", "",
             "## One `BevTracker.update` (one jp_bev_tracks call: four launches), and `jp_bev_objects` beside it", "",
             f"Device events around {opt.launches} back-to-back calls, the cases alternated round by round, {opt.rounds} rounds, median "
             "(min .. max) per call.  The tracker is fed the two frames of a scene in turn, so every timed call matches against a "
             "previous frame.  `matched` is what the last call of the default form reported per camera, next to the tracked objects.", "",
             "| scene | cameras | tracked objects | matched | form of the vote | us per update | jp_bev_objects, us | update / objects |",
             "|---|---|---|---|---|---|---|---|"]
    for B in (1, 4):
        for name, pair in scenes(B, occ).items():
            cases, trackers = {}, {}
            for v in VOTES:
                tr = trackers[v] = BevTracker(B, occ)
                flip = [0]

                def step(tr=tr, flip=flip):
                    bo, _, T = pair[flip[0]]
                    flip[0] ^= 1
                    tr.update(bo, T)
                cases[v] = (step, v)
            probe = BevObjects(B, occ, **({"conn": 4} if name == "percolation" else {}))
            cases["objects"] = (lambda probe=probe: probe.find(pair[0][1]), None)
            t = time_calls(cases, opt.launches, opt.rounds)
            st = trackers["2"].stats.cpu().tolist()
            same = all(torch.equal(trackers["2"].tracks_i, trackers[v].tracks_i) and torch.equal(trackers["2"].kin, trackers[v].kin) for v in VOTES)
            mo = statistics.median(t["objects"])
            for v, what in VOTES.items():
                lines.append(f"| {name} | {B} | {[r[0] for r in st]} | {[r[1] for r in st]} | {v}: {what} | {fmt(t[v])} | {fmt(t['objects'])} | "
                             f"{statistics.median(t[v]) / mo:.2f} |")
            if name == "road":
                d = float(trackers["2"].kin[:, :, 2:].abs().max())
                lines.append(f"| | | | | the three forms give the same tracks and kin: {same}; largest world displacement of a matched object: {d:.3g} m | | | |")
            else:
                lines.append(f"| | | | | the three forms give the same tracks and kin: {same} | | | |")
    print("\n".join(lines[-20:]), flush=True)

    if not opt.no_session:
        from tools.frozen_bench import build_model, counted_calls
        from tools.stream_bench import wall_ms
        sh, sw = opt.src
        model = build_model(opt.hw, 1)
        n_all = opt.warmup + opt.frames
        g = torch.Generator().manual_seed(101)
        frames = torch.randint(0, 256, (n_all, 1, sh, sw, 3), dtype=torch.uint8, generator=g).pin_memory()
        routes = {"plain": PerceptionStream(model, (sh, sw)), "objects=True": PerceptionStream(model, (sh, sw), objects=True),
                  "objects=dict(track=True)": PerceptionStream(model, (sh, sw), objects=dict(track=True))}
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
        tracked = routes["objects=dict(track=True)"]
        same = all(torch.equal(getattr(tracked, a), getattr(routes["plain"], a)) for a in ("_disp", "_depth", "_layout", "_pose", "_traj"))
        st = tracked.tracks.stats_host()
        lines += ["", "## A plain session, one with objects, one with objects and tracks", "",
                  f"uint8 frames of {sh}x{sw} in pinned host memory, synthetic weights, network {opt.hw} x {opt.hw}; host clock around one push + "
                  f"synchronise, {opt.warmup} warm-up frames, then {opt.frames} timed frames, the three sessions alternated frame by frame; median "
                  "(min .. max).", "", "| session | ms per frame | C-ABI calls per frame |", "|---|---|---|"]
        for k in routes:
            lines.append(f"| {k} | {fmt(times[k], 4)} | {ncalls[k]} |")
        mt = statistics.median(times["objects=dict(track=True)"])
        for k in ("plain", "objects=True"):
            lo, hi, m = min(times[k]), max(times[k]), statistics.median(times[k])
            lines += ["", f"Band of the {k} session: {lo:.4f} .. {hi:.4f} ms; the median with tracks, {mt:.4f} ms, lies "
                      f"{'inside' if lo <= mt <= hi else 'OUTSIDE'} it (difference of the medians: {mt - m:+.4f} ms)."]
        lines += ["", f"Outputs, pose and trajectory of the tracked and the plain session after {n_all + 1} frames bit-equal: {same}; the last frame's "
                  f"tracker statistics: {st} (synthetic weights: no street scene).", ""]
        print("\n".join(lines[-12:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
