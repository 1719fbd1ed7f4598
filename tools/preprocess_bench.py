#!/usr/bin/env python
"""Time one batch of device-side preprocessing (jperceiver_amd.datasets.DevicePreprocessor) with and without the on-device flip
and the batched ColorJitter, in ONE process, alternating the variants.

Shape (KITTI raw through the 1024 x 1024 recipe): B = 8 items, 3 frames, raw 375 x 1242 -> full 375 x 1242 -> 1024 x 1024, two
BEV labels 512 x 512 -> 256 x 256; every item augmented (the worst case for the per-op jitter).

  per_op          what the pipeline did before it had a flip: do_color_aug=True, one jp_color_jitter_op chain per (item, frame)
  flip+batched    do_color_aug=True, do_flip=True, batched=True

and, to tell the two changes apart, `flip` (do_flip=True, per-op jitter) and `batched` (no flip, batched jitter).

Times are device events around `--iters` back-to-back calls (the host enqueues ahead, so a window holds the device time or the
host's launch time, whichever is longer -- which is what a training loop sees); `--rounds` windows per variant, alternated;
median / min / max are reported.  Launches are counted, not timed: library launches from the entry points called (a contrast
op of jp_color_jitter_op is a memset + two kernels, jp_color_jitter_batched two kernels, everything else one), plus the torch
operations of the call (one clone per frame, the uploads of the flag and parameter tables).  Needs a GPU; there is no fallback.

    python tools/preprocess_bench.py [--iters 100] [--rounds 7] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from jperceiver_amd import synthetic as syn  # noqa: E402
from jperceiver_amd.datasets import DevicePreprocessor  # noqa: E402
from jperceiver_amd.datasets import preprocess as pp  # noqa: E402

B, FR, RAW, FULL, NET, LABEL = 8, [0, -1, 1], (375, 1242), (375, 1242), (1024, 1024), 512
VARIANTS = {
    "per_op": dict(do_flip=False, batched=False),
    "flip+batched": dict(do_flip=True, batched=True),
    "flip": dict(do_flip=True, batched=False),
    "batched": dict(do_flip=False, batched=True),
}


def make_raw(dev):
    raw = {("color", f, -1): (torch.from_numpy(syn.hash_uniform(1, ("raw", f), (B,) + RAW + (3,))) * 256).to(torch.uint8).to(dev)
           for f in FR}
    for name in ("bothS", "bothD"):
        raw[(name, 0, 0)] = ((torch.from_numpy(syn.hash_uniform(1, name, (B, LABEL, LABEL))) > 0.55) * 255).to(torch.uint8).to(dev)
    return raw


class LaunchCounter:
    """counts what one __call__ enqueues: wraps the ctypes dispatcher of the preprocessing module"""

    def __init__(self):
        self.lib = self.calls = 0
        self._real = pp.call

    def __enter__(self):
        def call(name, *a):
            self.calls += 1
            if name == "jp_color_jitter_op":
                self.lib += 3 if a[4] == 1 else 1          # contrast: memset + gray sum + apply
            elif name == "jp_color_jitter_batched":
                self.lib += 2
            else:
                self.lib += 1
            return self._real(name, *a)
        pp.call = call
        return self

    def __exit__(self, *exc):
        pp.call = self._real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench: no GPU (this tool measures; it has no CPU path)")
    dev = torch.device("cuda", 0)
    pre = DevicePreprocessor(NET[0], NET[1], dev)
    raw = make_raw(dev)

    def run(name, seed=0):
        return pre(raw, FR, FULL, do_color_aug=True, generator=torch.Generator().manual_seed(seed), **VARIANTS[name])

    res = {k: {} for k in VARIANTS}
    for name in VARIANTS:                                    # launches of one call
        with LaunchCounter() as lc:
            run(name)
        v = VARIANTS[name]
        torch_ops = len(FR) + int(v["do_flip"]) + int(v["batched"])        # clones + table uploads
        res[name].update(entry_point_calls=lc.calls, library_launches=lc.lib, torch_ops=torch_ops, launches=lc.lib + torch_ops)
    # same draws, same inputs: how far the batched jitter is from the per-op one (the gray mean is summed in another order)
    a, b = run("per_op", 1), run("batched", 1)
    diff = max(float((a[k] - b[k]).abs().max()) for k in a if k[0] == "color_aug")
    fa, fb = run("flip", 1), run("flip+batched", 1)
    diff_f = max(float((fa[k] - fb[k]).abs().max()) for k in fa if k[0] == "color_aug")
    flipped_ok = torch.equal(fa[("color", 0, -1)], a[("color", 0, -1)].flip(-1))        # no resize at this shape: a pure mirror
    del a, b, fa, fb
    for name in VARIANTS:
        for _ in range(args.warmup):
            run(name)
    torch.cuda.synchronize()
    times = {k: [] for k in VARIANTS}
    for _ in range(args.rounds):
        for name in VARIANTS:                                # alternate the variants inside every round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.iters):
                run(name, i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    for name, t in times.items():
        res[name].update(ms_median=statistics.median(t), ms_min=min(t), ms_max=max(t))
    out = dict(tool="preprocess_bench", device=torch.cuda.get_device_name(0), B=B, frames=len(FR), raw=RAW, full=FULL, net=NET,
               label=LABEL, iters=args.iters, rounds=args.rounds, variants=res, batched_vs_per_op_max_abs_diff=diff,
               flip_batched_vs_flip_per_op_max_abs_diff=diff_f, flip_mirrors_full_frame=flipped_ok)
    print("| variant | ms / batch (median) | min | max | launches | of which library |")
    print("|---|---|---|---|---|---|")
    for name, r in res.items():
        print(f"| {name} | {r['ms_median']:.3f} | {r['ms_min']:.3f} | {r['ms_max']:.3f} | {r['launches']} | {r['library_launches']} |")
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
