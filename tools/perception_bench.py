#!/usr/bin/env python
"""Time the four kernels of csrc/perception.hip at the demo's largest shape (network 1024^2 -> frames of 2056 x 2464, B = 8) next
to the three-kernel path jp_disp_resize_depth replaces, and write the table of profiles/perception_kernels.md.

    python tools/perception_bench.py [--reps 30] [--out profiles/perception_kernels.md]

HIP-event medians of warm launches; bytes are the compulsory traffic computed from the shapes (every input read once per pass
over it, every output written once), GB/s = those bytes over the median time."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jperceiver_amd._lib import call                                                        # noqa: E402
from jperceiver_amd.apis import perception as pc                                            # noqa: E402


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--net", type=int, default=1024)
    ap.add_argument("--size", type=int, nargs=2, default=(2056, 2464))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perception_bench needs the GPU: a timing taken anywhere else says nothing")
    B, hw, (OH, OW) = a.batch, a.net, a.size
    dev, occ = "cuda", a.net // 4
    g = torch.Generator(device=dev).manual_seed(0)
    disp = torch.rand((B, 1, hw, hw), device=dev, generator=g)
    dmin, dmax = 0.1, 100.0
    f4 = 4
    n_in, n_out = B * hw * hw, B * OH * OW
    rows = []

    depth, sdisp = pc.disp_resize_depth(disp, (OH, OW), dmin, dmax, want_disp=True)
    rows.append(("jp_disp_resize_depth (depth only)", (n_in + n_out) * f4,
                 timed(lambda: pc.disp_resize_depth(disp, (OH, OW), dmin, dmax), a.reps)))
    rows.append(("jp_disp_resize_depth (+ disp_out)", (n_in + 2 * n_out) * f4,
                 timed(lambda: pc.disp_resize_depth(disp, (OH, OW), dmin, dmax, want_disp=True), a.reps)))

    scaled, res, old = torch.empty_like(disp), torch.empty_like(depth), torch.empty_like(depth)

    def three_kernels():
        call("jp_affine", disp, scaled, disp.numel(), 1.0 / dmin - 1.0 / dmax, 1.0 / dmax)
        call("jp_bilinear_fwd", scaled, res, B, hw, hw, OH, OW)
        torch.reciprocal(res, out=old)
    rows.append(("before: jp_affine -> jp_bilinear_fwd -> 1/x", (2 * n_in + n_in + n_out + 2 * n_out) * f4, timed(three_kernels, a.reps)))

    flat = sdisp.view(B, OH * OW)
    rows.append(("jp_quantiles (q = 0, 0.95; 4 passes)", 4 * n_out * f4, timed(lambda: pc._order_statistics(flat, [0.0, 0.95]), a.reps)))
    rows.append(("jp_quantiles (q = 0, 0.5, 0.95, 1)", 4 * n_out * f4,
                 timed(lambda: pc._order_statistics(flat, [0.0, 0.5, 0.95, 1.0]), a.reps)))
    st, _ = pc._order_statistics(flat, [0.0, 0.95])
    vmm = torch.stack([st[:, 0, 0], st[:, 1, 0]], 1).contiguous()
    lut = pc.default_lut().to(dev)
    rows.append(("jp_colorize_u8", n_out * (f4 + 3), timed(lambda: pc.colorize(flat, vmm, lut), a.reps)))
    rows.append(("colorize_disp (quantiles + colorize)", n_out * (5 * f4 + 3), timed(lambda: pc.colorize_disp(sdisp, lut), a.reps)))
    road, car = torch.randn((B, 2, occ, occ), device=dev, generator=g), torch.randn((B, 2, occ, occ), device=dev, generator=g)
    npx = B * occ * occ
    rows.append(("jp_layout_classes_u8 (cls only)", npx * (4 * f4 + 1), timed(lambda: pc.layout_classes(road, car), a.reps)))
    rows.append(("jp_layout_classes_u8 (+ rgb)", npx * (4 * f4 + 4), timed(lambda: pc.layout_classes(road, car, want_rgb=True), a.reps)))

    # the timed calls include the output allocation from torch's caching allocator (host side, overlapped with the launches)
    same = bool(torch.equal(old, depth))
    lines = ["# Perception post-processing kernels on the MI355X", "",
             f"`python tools/perception_bench.py --reps {a.reps}`: network {hw}x{hw}, frames {OH}x{OW}, B = {B}, BEV {occ}x{occ}; "
             f"{torch.cuda.get_device_name(0)}.  HIP-event medians of {a.reps} warm launches (5 un-timed ones first); bytes = "
             "compulsory traffic from the shapes (inputs read once per pass, outputs written once); GB/s = bytes / median.", "",
             "| kernel | MB moved | median ms | min | max | GB/s |", "|---|---:|---:|---:|---:|---:|"]
    for name, nbytes, (med, lo, hi) in rows:
        lines.append(f"| {name} | {nbytes / 1e6:.1f} | {med:.4f} | {lo:.4f} | {hi:.4f} | {nbytes / 1e6 / med:.0f} |")
    lines += ["", f"Depth of the one-pass kernel bit-equal to the three-kernel path on this input: {same}.", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
