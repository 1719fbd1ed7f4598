#!/usr/bin/env python
"""Time the LiDAR depth ground truth and the batched depth scorer at KITTI size (profiles/lidar_depth_eval.md).

    python tools/lidar_depth_bench.py [--repeats 30] [--warmup 5] [--batch 8] [--points 120000]

Prints one JSON line:
  lidar_depth_maps_ms       one lidar_depth_maps call on `batch` seeded scans of `points` points at 375 x 1242 (scans already on the
                            device: the upload of the file contents is the caller's)
  lidar_kernels_ms          the jp_lidar_depth_map call alone, on prepared device buffers
  eval_depth_batch_ms       one eval_depth_batch call on `batch` images (disp 192 x 640, ground truth 375 x 1242)
  eval_depth_loop_ms        `batch` eval_depth calls, the loop of apis.evaluate_depth, on the same inputs
  per_image_speedup         eval_depth_loop_ms / eval_depth_batch_ms
Every figure is the median of `repeats` host-clock windows that start after and end with a synchronise of the device, after `warmup`
untimed runs; the two scorers alternate inside one loop, so drift of the machine hits both.  The outputs of the two scorers on
these inputs are compared before anything is timed.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jperceiver_amd._lib import call, lib                                       # noqa: E402
from jperceiver_amd.core import evaluation as ev                                # noqa: E402

H, W, h, w = 375, 1242, 192, 640


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=120000)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    dev = torch.device("cuda")
    B, n = a.batch, a.points
    K = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
    P = K @ np.array([[0.0, -1, 0, -0.004], [0, 0, -1, -0.076], [1, 0, 0, -0.272], [0, 0, 0, 1]])
    scans = []
    for b in range(B):
        rng = np.random.default_rng(100 + b)
        x = rng.uniform(-5.0, 80.0, n)
        pts = np.stack([x, x * rng.uniform(-1.0, 1.0, n), x * rng.uniform(-0.3, 0.3, n), rng.uniform(0, 1, n)], 1)
        scans.append(torch.from_numpy(pts.astype(np.float32)).to(dev))
    gt = ev.lidar_depth_maps(scans, P, (H, W), dtype=torch.float32)
    disp = torch.rand((B, 1, h, w), generator=torch.Generator().manual_seed(0)).to(dev)

    # prepared buffers for the bare entry point
    pts_all = torch.cat(scans, 0).contiguous()
    offsets = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    Pd = torch.from_numpy(np.broadcast_to(P, (B, 3, 4)).copy()).to(dev)
    out32 = torch.empty((B, H, W), device=dev)
    ws = torch.empty(lib().fn["jp_lidar_depth_ws_bytes"](B, H, W), dtype=torch.uint8, device=dev)

    def lidar_api():
        ev.lidar_depth_maps(scans, P, (H, W), dtype=torch.float32)

    def lidar_bare():
        call("jp_lidar_depth_map", pts_all, offsets, Pd, None, B, H, W, 0, None, out32, ws)

    def batch():
        return ev.eval_depth_batch(disp, gt)

    def loop():
        return [ev.eval_depth(disp[b:b + 1], gt[b]) for b in range(B)]

    warnings.simplefilter("ignore", RuntimeWarning)
    rb, rl = batch(), loop()
    for x, y in zip(rb, rl):                                    # faster and different is not faster
        assert x["n_valid"] == y["n_valid"] and x["scale"] == y["scale"] and x["a1"] == y["a1"], (x, y)
        assert abs(x["abs_rel"] - y["abs_rel"]) <= 2.0 * x["n_valid"] * 2.0 ** -53 * abs(y["abs_rel"]), (x, y)
    fns = dict(lidar_depth_maps_ms=lidar_api, lidar_kernels_ms=lidar_bare, eval_depth_batch_ms=batch, eval_depth_loop_ms=loop)
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    times = {k: [] for k in fns}
    for _ in range(a.repeats):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    res = {k: round(statistics.median(v), 4) for k, v in times.items()}
    res.update({k.replace("_ms", "_min_ms"): round(min(v), 4) for k, v in times.items()})
    res["per_image_speedup"] = round(res["eval_depth_loop_ms"] / res["eval_depth_batch_ms"], 2)
    res.update(batch=B, points=n, gt_hw=[H, W], disp_hw=[h, w], repeats=a.repeats, warmup=a.warmup,
               n_valid=[r["n_valid"] for r in rb], nonzero_gt=int((gt != 0).sum()) // B, device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
