#!/usr/bin/env python
"""Time the odometry evaluation path on the GPU and write profiles/odometry_eval.md.

    python tools/odometry_bench.py [--out profiles/odometry_eval.md] [--n 4661] [--frames 64]

What is measured (nothing here is a threshold; the file records the numbers):
 * every entry point of csrc/odometry.hip at n poses (default 4661, the longest KITTI sequence): device events around a window of
   back-to-back calls on one stream, after a warm-up; median and range of the per-call time over several windows.  An entry point's
   time includes all of its launches (3 for the chain, 4 for the segment table, 3 for the moments).
 * eval_odometry(pred, gt) at the same n: host clock around the call, which ends in device-to-host copies (a synchronise).
 * odometry_device(batch=8) against the existing odometry() (B = 1 pairs, numpy chain) on `frames` frames at 192x640, synthetic
   weights: host clock around each call + synchronise, the two alternated.
Needs a GPU: there is no CPU path to fall back to."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jperceiver_amd._lib import call, lib                                                   # noqa: E402
from jperceiver_amd.core import evaluation as ev                                            # noqa: E402
from jperceiver_amd.apis import odometry, odometry_device, chain_poses_device               # noqa: E402


def event_time_us(fn, calls, windows, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        per_call.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(per_call), min(per_call), max(per_call)


def wall_time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def synthetic_sequence(n, seed=0):
    """a car-like float32 transform sequence: ~1 m forward per frame, small rotations"""
    rng = np.random.default_rng(seed)
    T = np.tile(np.identity(4, dtype=np.float32), (n, 1, 1))
    a = rng.normal(0.0, 0.01, n)
    T[:, 0, 0], T[:, 0, 2], T[:, 2, 0], T[:, 2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    T[:, :3, 3] = rng.normal([0.0, 0.0, -1.0], 0.05, (n, 3))
    return torch.from_numpy(T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odometry_eval.md"))
    ap.add_argument("--n", type=int, default=4661)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("odometry_bench: no GPU")
    dev = "cuda"
    n = opt.n
    T = synthetic_sequence(n - 1).to(dev)
    gt = chain_poses_device(T)
    Tp = T.clone()                                                 # the prediction: noisy translations, 1/29.5 of the scale
    Tp[:, :3, 3] += 0.02 * torch.randn((n - 1, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    pred = ev.transform_poses(chain_poses_device(Tp), None, 1 / 29.5)
    rows = []

    ws = torch.empty(lib().fn["jp_pose_chain_ws_bytes"](n - 1), device=dev, dtype=torch.uint8)
    poses = torch.empty((n, 12), device=dev, dtype=torch.float64)
    rows.append(("jp_pose_chain_f64 (n-1 transforms, invert)", event_time_us(
        lambda: call("jp_pose_chain_f64", T, n - 1, 1, poses, ws), opt.calls, opt.windows, 20)))
    lengths = (ctypes.c_double * 8)(*[float(x) for x in ev.ODOM_LENGTHS])
    S = (n + 9) // 10
    dist = torch.empty(n, device=dev, dtype=torch.float64)
    last = torch.empty(S * 8, device=dev, dtype=torch.int32)
    table = torch.empty((S * 8, 5), device=dev, dtype=torch.float64)
    ws2 = torch.empty(lib().fn["jp_odom_segments_ws_bytes"](n, 10, 8), device=dev, dtype=torch.uint8)
    rows.append(("jp_odom_segment_errors (step 10, 8 lengths)", event_time_us(
        lambda: call("jp_odom_segment_errors", gt, pred, n, 10, ctypes.addressof(lengths), 8, dist, last, table, ws2),
        opt.calls, opt.windows, 20)))
    out19 = torch.empty(19, device=dev, dtype=torch.float64)
    ws3 = torch.empty(lib().fn["jp_traj_moments_ws_bytes"](n), device=dev, dtype=torch.uint8)
    rows.append(("jp_traj_moments", event_time_us(lambda: call("jp_traj_moments", pred, gt, n, out19, ws3), opt.calls, opt.windows, 20)))
    A = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    outp = torch.empty_like(pred)
    rows.append(("jp_poses_transform_f64", event_time_us(
        lambda: call("jp_poses_transform_f64", pred, n, ctypes.addressof(A), 29.5, outp), opt.calls, opt.windows, 20)))

    res = ev.eval_odometry(pred, gt)
    e2e = wall_time_ms(lambda: ev.eval_odometry(pred, gt), 30, 5)

    # pose nets: synthetic weights, eval mode
    from jperceiver_amd import synthetic as syn
    from jperceiver_amd.model.modules import PoseEncoder, PoseDecoder
    enc, dec = PoseEncoder(18, None, 2), PoseDecoder(np.array([64, 64, 128, 256, 512]))
    enc.load_state_dict(syn.synth_state_dict(enc.state_dict(), seed=3, bn_stats=True))
    dec.load_state_dict(syn.synth_state_dict(dec.state_dict(), seed=4, bn_stats=True))
    enc, dec = enc.to(dev).eval(), dec.to(dev).eval()
    frames = torch.rand(opt.frames, 3, 192, 640, generator=torch.Generator().manual_seed(5)).to(dev)
    odometry(enc, dec, frames)
    odometry_device(enc, dec, frames, batch=8)
    torch.cuda.synchronize()
    tb, t1 = [], []
    for _ in range(5):                                              # alternated: the host is shared
        for f, acc in ((lambda: odometry_device(enc, dec, frames, batch=8), tb), (lambda: odometry(enc, dec, frames), t1)):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
    diff = float(np.abs(odometry_device(enc, dec, frames, batch=8).cpu().numpy() - odometry(enc, dec, frames)).max())

    name = torch.cuda.get_device_name(0)
    L = ["# Odometry evaluation: measured times", "",
         f"Box: {name}, torch {torch.__version__}, HIP {torch.version.hip}; written by `tools/odometry_bench.py`.", "",
         "Protocol: one process, one stream, profiler off.  Entry points: device events around a window of "
         f"{opt.calls} back-to-back calls after 20 warm-up calls; {opt.windows} windows; the per-call time is the window over the "
         "number of calls (launch overhead that the queue does not hide is part of it).  End-to-end figures: host clock around "
         "the call plus a device synchronise, after warm-up.  No threshold is attached to any of these numbers.", "",
         f"## Entry points of csrc/odometry.hip at n = {n} poses", "",
         "| entry point | launches | median us / call | min | max |", "|---|---|---|---|---|"]
    launches = {0: 3, 1: 4, 2: 3, 3: 1}
    for i, (nm, (med, lo, hi)) in enumerate(rows):
        L.append(f"| {nm} | {launches[i]} | {med:.1f} | {lo:.1f} | {hi:.1f} |")
    L += ["", f"## eval_odometry(pred, gt) at n = {n}", "",
          f"Wall time, 30 calls after 5 warm-up calls: median {e2e[0]:.2f} ms (min {e2e[1]:.2f}, max {e2e[2]:.2f}); "
          f"{res['n_segments']} segments over {res['distance']:.0f} m.  The call makes two moments reductions, one transform and one "
          "segment table, and copies the table, the distances and 19 + 19 numbers back; most of it is host work (allocation, "
          "ctypes calls, the numpy averages) and the synchronising copies.", "",
          f"## Pose nets: {opt.frames} frames at 192x640, synthetic weights", "",
          "| path | median ms | min | max | ms / pair (median) |", "|---|---|---|---|---|",
          f"| odometry_device(batch=8): 8 pairs per forward pass, chain on the device | {statistics.median(tb):.1f} | {min(tb):.1f} | "
          f"{max(tb):.1f} | {statistics.median(tb) / (opt.frames - 1):.2f} |",
          f"| odometry(): one pair per forward pass, numpy chain | {statistics.median(t1):.1f} | {min(t1):.1f} | {max(t1):.1f} | "
          f"{statistics.median(t1) / (opt.frames - 1):.2f} |", "",
          f"Five alternated runs of each after one warm-up run.  Largest difference between the two trajectories: {diff:.2e} "
          "(the B = 8 and B = 1 convolutions take different kernels; tests/test_odometry_eval_gpu.py holds each transform to 4e-5).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    main()
