#!/usr/bin/env python
"""Measure frozen inference (apis.freeze: eval BatchNorm folded into the convolutions, jp_add_relu) against the eval route it
replaces and write profiles/frozen_inference.md.

    python tools/frozen_bench.py [--out profiles/frozen_inference.md] [--hw 1024] [--batches 1 8] [--reps 7]

What is measured (nothing here is a threshold; the file records the numbers, also where frozen is slower):
 * Perceiver.perceive_video on synthetic frames at hw x hw (default 1024, the project's shape), 2 * batch frames per call, eager
   and frozen on two models that hold the same synthetic checkpoint: host clock around the call, which ends in a device-to-host
   copy of the poses, plus a synchronise; 3 warm-up calls each, then `reps` timed calls each, the two alternated; median and
   range of the time per frame.
 * entry-point calls per frame of one steady-state call, counted where the Python layers hand over to the C ABI (one call is
   one launch for the element-wise kernels and BatchNorm, up to a few for a convolution).
 * from the library's own profile (jp_profile_*: HIP events around each launch, on its stream), in a run of its own: launches
   and summed milliseconds of jp_bn_eval_fwd and jp_add_relu, and the number of convolution dispatches.
 * not measured here: the block-level errors against float64 and the full-model figures.  The test suite prints those; the
   sections of the note that hold them (from "Block-level error" on) are kept as they are when the note is rewritten.
Needs a GPU: there is no CPU path to fall back to."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jperceiver_amd import _lib, synthetic as syn                                           # noqa: E402
from jperceiver_amd.apis import Perceiver                                                   # noqa: E402
from jperceiver_amd.model import MONO                                                       # noqa: E402
from oracle import jp_oracle as J                                                           # noqa: E402


def build_model(hw, batch):
    opt = J.default_opt(frame_ids=[0, -1, 1], imgs_per_gpu=batch, height=hw, width=hw, occ_map_size=hw // 4, type="static",
                        split="odometry")
    model = MONO.module_dict["Baseline"](opt)
    model.load_state_dict(syn.synth_state_dict(model.state_dict(), seed=3, bn_stats=True))
    return model.cuda().eval()


def frames(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, hw, hw, generator=g).cuda()


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


class counted_calls:
    """Count the C-ABI calls of every jperceiver_amd module that took `call` from _lib by name."""

    def __enter__(self):
        self.names, orig = [], _lib.call

        def counting(name, *a):
            self.names.append(name)
            return orig(name, *a)

        self.patched = [m for n, m in list(sys.modules.items()) if n.startswith("jperceiver_amd") and getattr(m, "call", None) is orig]
        for m in self.patched:
            m.call = counting
        self.orig = orig
        return self

    def __exit__(self, *a):
        for m in self.patched:
            m.call = self.orig


def profiled(fn, cap=8192):
    L = _lib.lib()
    if L.fn["jp_profile_begin"](cap) != 0:
        raise RuntimeError(L.last_error())
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        n = L.fn["jp_profile_end"]()
    if n >= cap:
        raise RuntimeError("profile buffer too small")
    buf, fl, ms = ctypes.create_string_buffer(512), ctypes.c_double(), ctypes.c_float()
    out = {}
    for i in range(n):
        rc = L.fn["jp_profile_get"](i, ctypes.cast(buf, ctypes.c_void_p), 512, ctypes.cast(ctypes.pointer(fl), ctypes.c_void_p),
                                    ctypes.cast(ctypes.pointer(ms), ctypes.c_void_p))
        if rc != 0:
            raise RuntimeError(L.last_error())
        tag = buf.value.decode()
        tag = tag if tag in ("jp_bn_eval_fwd", "jp_add_relu") else "convolution dispatches"
        c, t = out.get(tag, (0, 0.0))
        out[tag] = (c + 1, t + ms.value)
    return out


KEPT = "## Block-level error against float64"


def kept_sections(path):
    """The part of the note that this tool does not measure -- the figures that the test suite prints (`pytest -s
    tests/test_frozen_blocks_gpu.py tests/test_frozen_model_gpu.py`), copied in by hand: everything from the block-error heading
    on stays as it is when the note is rewritten."""
    if os.path.exists(path):
        old = open(path).read()
        if KEPT in old:
            return old[old.index(KEPT):].rstrip("\n").split("\n")
    return [KEPT + " (tests/test_frozen_blocks_gpu.py)", "", "Not recorded yet: run the test with `-s` and copy the four rows it prints.", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_inference.md"))
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frozen_bench: no GPU")
    lines = ["# Frozen inference: eval BatchNorm folded into the convolutions, fused add + ReLU", "",
             f"Written by `tools/frozen_bench.py` on {torch.cuda.get_device_name(0)}; `Perceiver.perceive_video` at "
             f"{opt.hw}x{opt.hw}, synthetic frames and weights (BatchNorm statistics not the identity), 2 x batch frames per call.  "
             f"Time per frame: host clock around the call + synchronise, {opt.warmup} warm-up calls, then {opt.reps} timed calls per "
             "route, the two routes alternated; median (min .. max).  Calls per frame: C-ABI entry-point calls of one steady-state "
             "call / frames.  Kernel rows: the library's HIP-event profile (`jp_profile_*`) of one call, in a run of its own "
             "(launches and summed milliseconds per call, i.e. for 2 x batch frames and the pose pairs that go with them).", ""]
    eager, frozen = build_model(opt.hw, max(opt.batches)), build_model(opt.hw, max(opt.batches))
    pe, pf = Perceiver(eager), Perceiver(frozen, frozen=True)
    for b in opt.batches:
        n = 2 * b
        fr = frames(n, opt.hw, seed=100 + b)
        routes = (("eager", lambda: pe.perceive_video(fr, batch=b)), ("frozen", lambda: pf.perceive_video(fr, batch=b)))
        for _ in range(opt.warmup):
            for _, fn in routes:
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in routes}
        for _ in range(opt.reps):
            for k, fn in routes:
                times[k].append(wall_ms(fn) / n)
        ncalls, prof = {}, {}
        for k, fn in routes:
            with counted_calls() as c:
                fn()
            torch.cuda.synchronize()
            ncalls[k] = c.names
        for k, fn in routes:
            prof[k] = profiled(fn)
        ve, vf = routes[0][1](), routes[1][1]()
        dT = float((ve.cam_T_cam - vf.cam_T_cam).abs().max())
        dD = float(((ve.depth - vf.depth).abs() / ve.depth).max())
        dL = float((ve.layout != vf.layout).float().mean())
        lines += [f"## batch {b} ({n} frames per call)", "",
                  "| route | ms per frame | C-ABI calls per frame | jp_bn_eval_fwd launches / ms | jp_add_relu launches / ms | convolution dispatches / ms |",
                  "|---|---|---|---|---|---|"]
        for k, _ in routes:
            t = times[k]
            p = prof[k]
            cell = lambda tag: "{} / {:.3f}".format(*p[tag]) if tag in p else "0 / 0"          # noqa: E731
            lines.append(f"| {k} | {statistics.median(t):.3f} ({min(t):.3f} .. {max(t):.3f}) | {len(ncalls[k]) / n:.1f} "
                         f"({ncalls[k].count('jp_bn_eval_fwd')} jp_bn_eval_fwd, {ncalls[k].count('jp_add_relu')} jp_add_relu, "
                         f"{ncalls[k].count('jp_amax_into')} jp_amax_into per call) | {cell('jp_bn_eval_fwd')} | {cell('jp_add_relu')} | "
                         f"{cell('convolution dispatches')} |")
        me, mf = statistics.median(times["eager"]), statistics.median(times["frozen"])
        lines += ["", f"frozen / eager time per frame: {mf / me:.3f} ({'frozen is SLOWER' if mf > me else 'frozen is faster'}); "
                      f"outputs of the two routes on these frames: poses differ by {dT:.2e}, depth by {dD:.2e} relative, "
                      f"{dL:.4%} of the BEV classes.", ""]
        print("\n".join(lines[-8:]), flush=True)
    lines += kept_sections(opt.out) + [""]
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
