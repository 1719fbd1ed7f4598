#!/usr/bin/env python
"""Measure the filtered BEV tracks (csrc/bevfilter.hip, apis.BevTrackFilter, PerceptionStream(objects=dict(track=dict(filter=True))))
and write profiles/bev_track_filter.md.

    python tools/bevfilter_bench.py [--out profiles/bev_track_filter.md] [--occ 256] [--launches 200] [--rounds 7] [--frames 30]
                                    [--warmup 3] [--hw 1024] [--src 375 1242] [--no-session]

Shape: layouts of occ x occ (default 256, the project's at 1024 x 1024), max_objects 64, max_tracks 128, 1 and 4 cameras.
  1. one `BevTrackFilter.update` (the one jp_bev_track_filter call: one launch) behind the tracker on the two scenes of
     tools/bevtrack_bench.py -- the road scene (two vehicle boxes under a known ego-motion) and the random map whose first 64
     components are tracked -- with `BevTracker.update` alone and the pair of calls timed beside it in the same process.  The tracker
     is fed the two frames of a scene in turn; the filter alone is timed on the tracker's outputs of the last of them (every slot
     continues).  Device events around `launches` back-to-back calls, `rounds` rounds, the cases alternated round by round.
  2. id switches on the road scene: the scene stands still for `--frames` frames and one vehicle is blanked for one, and for two,
     frames out of every five; counted are the ids that vehicle is given over the run, by the tracker alone and by the filter.
  3. an objects=dict(track=True) session and an objects=dict(track=dict(filter=True)) session on the same model and frames,
     alternated frame by frame within one process: host clock around one push + synchronise, median (min .. max) per frame.
Nothing here is a threshold.  Needs a GPU: there is no CPU path to fall back to; a number that was not taken reads "not measured"."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jperceiver_amd.apis import BevObjects, BevTracker, BevTrackFilter, PerceptionStream       # noqa: E402
from tools.bevobj_bench import fmt, road_layouts                                                # noqa: E402
from tools.bevtrack_bench import scenes, time_calls                                             # noqa: E402


def id_switches(occ, frames, blank):
    """the road scene standing still, its object 0 blanked in the frames k with k % 5 in `blank` -> (frames it was seen in, ids the
    tracker gave it, ids the filter gave it)"""
    lay = torch.from_numpy(road_layouts(1, occ)).cuda()
    bo, tr, flt = BevObjects(1, occ), BevTracker(1, occ), BevTrackFilter(1, occ=occ)
    first = bo.find(lay).labels.clone()
    if int(bo.count[0]) < 1:
        return {}, {}
    cell = int(bo.table[0, 0, 7])                                       # first_cell of object 0
    gone = torch.where(first == 0, torch.zeros_like(lay), lay)
    eye = torch.eye(4, dtype=torch.float64, device="cuda").repeat(1, 1, 1)
    t_ids, f_ids = {}, {}                                               # frame -> id, the frames the vehicle is seen in
    for k in range(frames):
        flt.update(tr.update(bo.find(gone if k % 5 in blank else lay), eye))
        obj = int(bo.labels.view(-1)[cell])
        if obj < 0:
            continue
        t_ids[k] = int(tr.tracks_i[0, obj, 0])
        slot = int(flt.obj_slot[0, obj])
        f_ids[k] = int(flt.slots_i[0, slot, 0]) if slot >= 0 else -1
    return t_ids, f_ids


def switches(ids):
    """frame -> id  ->  the frames in which the id differs from the one of the frame it was last seen in"""
    ks = sorted(ids)
    return [k for prev, k in zip(ks, ks[1:]) if ids[k] != ids[prev]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_track_filter.md"))
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
        sys.exit("bevfilter_bench: no GPU")
    occ = opt.occ
    lines = ["# Filtered BEV tracks: jp_bev_track_filter, and a session with it", "",
             f"Written by `tools/bevfilter_bench.py` on {torch.cuda.get_device_name(0)}; layouts of {occ} x {occ} cells of {40.0 / occ} m, "
             "max_objects 64, max_tracks 128, max_coast 3, min_hits 3, gate 2 m (the defaults: conventional settings, not tuned).", "",
             "## One `BevTrackFilter.update` (one jp_bev_track_filter call: one launch), and `BevTracker.update` beside it", "",
             f"Device events around {opt.launches} back-to-back calls, the cases alternated round by round, {opt.rounds} rounds, median "
             "(min .. max) per call.  `tracker` and `tracker + filter` are fed the two frames of a scene in turn; `filter` is the one call "
             "alone on the tracker's outputs of the last frame.  `live` is what the filter of the pair reported per camera after the last "
             "call.", "",
             "| scene | cameras | tracked objects | live slots | filter, us | tracker, us | tracker + filter, us | the pair - the tracker, us |",
             "|---|---|---|---|---|---|---|---|"]
    for B in (1, 4):
        for name, pair in scenes(B, occ).items():
            tr_alone, tr_pair, flt_pair, flt_alone = BevTracker(B, occ), BevTracker(B, occ), BevTrackFilter(B, occ=occ), BevTrackFilter(B, occ=occ)
            flips = {"t": 0, "p": 0}

            def tracker():
                bo, _, T = pair[flips["t"]]
                flips["t"] ^= 1
                tr_alone.update(bo, T)

            def both():
                bo, _, T = pair[flips["p"]]
                flips["p"] ^= 1
                flt_pair.update(tr_pair.update(bo, T))

            held = BevTracker(B, occ)
            for bo, _, T in pair:
                held.update(bo, T)
            cases = {"filter": (lambda: flt_alone.update(held), None), "tracker": (tracker, None), "pair": (both, None)}
            t = time_calls(cases, opt.launches, opt.rounds)
            n_cur = [r[0] for r in tr_pair.stats.cpu().tolist()]
            live = [r[0] for r in flt_pair.fstats.cpu().tolist()]
            d = statistics.median(t["pair"]) - statistics.median(t["tracker"])
            lines.append(f"| {name} | {B} | {n_cur} | {live} | {fmt(t['filter'])} | {fmt(t['tracker'])} | {fmt(t['pair'])} | {d:+.2f} |")
    print("\n".join(lines[-6:]), flush=True)

    lines += ["", "## Id switches on the road scene when one vehicle flickers", "",
              f"The road scene stands still for {opt.frames} frames (identity poses); its object 0 is removed from the layout in one, and in "
              "two, frames out of every five (frames 2, 7, 12, ... and 2, 3, 7, 8, ...).  An id switch is a frame in which the vehicle "
              "carries another id than in the frame it was last seen in.  Tracker: `tracks_i[..., 0]`; filter: the fid of the slot `obj_slot` "
              "names.  With min_hits 3 the first blank meets a track of two measurements, still tentative, and a tentative track ends at "
              "its first miss: a switch of the filter in the first frame after that blank is this rule, not a failure to coast.", "",
              "| blanked frames out of five | frames seen | id switches, tracker alone | in frames | id switches, filter | in frames |",
              "|---|---|---|---|---|---|"]
    for blank in ((), (2,), (2, 3)):
        t_ids, f_ids = id_switches(occ, opt.frames, blank)
        st, sf = switches(t_ids), switches(f_ids)
        lines.append(f"| {len(blank)} | {len(t_ids)} | {len(st)} | {st} | {len(sf)} | {sf} |" if t_ids else f"| {len(blank)} | not measured (no object) | | | | |")
    print("\n".join(lines[-5:]), flush=True)

    if not opt.no_session:
        from tools.frozen_bench import build_model, counted_calls
        from tools.stream_bench import wall_ms
        sh, sw = opt.src
        model = build_model(opt.hw, 1)
        n_all = opt.warmup + opt.frames
        g = torch.Generator().manual_seed(101)
        frames = torch.randint(0, 256, (n_all, 1, sh, sw, 3), dtype=torch.uint8, generator=g).pin_memory()
        k_t, k_f = "objects=dict(track=True)", "objects=dict(track=dict(filter=True))"
        routes = {k_t: PerceptionStream(model, (sh, sw), objects=dict(track=True)),
                  k_f: PerceptionStream(model, (sh, sw), objects=dict(track=dict(filter=True)))}
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
        a, b = routes[k_t], routes[k_f]
        same = all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("_disp", "_depth", "_layout", "_pose", "_traj")) and all(
            torch.equal(getattr(a.tracks, n), getattr(b.tracks, n)) for n in ("tracks_i", "kin", "stats"))
        lines += ["", "## A session with tracks, and one with tracks and the filter", "",
                  f"uint8 frames of {sh}x{sw} in pinned host memory, synthetic weights, network {opt.hw} x {opt.hw}; host clock around one push + "
                  f"synchronise, {opt.warmup} warm-up frames, then {opt.frames} timed frames, the two sessions alternated frame by frame; median "
                  "(min .. max).  The track=True session runs exactly the calls it ran before the filter existed.", "",
                  "| session | ms per frame | C-ABI calls per frame |", "|---|---|---|"]
        for k in routes:
            lines.append(f"| {k} | {fmt(times[k], 4)} | {ncalls[k]} |")
        lo, hi, m, mf = min(times[k_t]), max(times[k_t]), statistics.median(times[k_t]), statistics.median(times[k_f])
        lines += ["", f"Band of the track=True session: {lo:.4f} .. {hi:.4f} ms; the median with the filter, {mf:.4f} ms, lies "
                  f"{'inside' if lo <= mf <= hi else 'OUTSIDE'} it (difference of the medians: {mf - m:+.4f} ms).",
                  "", f"Outputs, pose, trajectory and tracker buffers of the two sessions after {n_all + 1} frames bit-equal: {same}; the last frame's "
                  f"filter statistics: {b.track_filter.stats_host()} (synthetic weights: no street scene).", ""]
        print("\n".join(lines[-10:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
