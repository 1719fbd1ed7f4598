#!/usr/bin/env python
"""bench.py — JPerceiver `Baseline` train-step throughput on N MI355X of one node.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A "step" = one full training iteration of the reference hot loop on one synthetic batch that is already
resident in HBM: batch_processor (forward + all losses, incl. generating the CGT scale label) ->
DistOptimizerHook.after_train_iter (zero_grad, backward with the overlapped gradient all-reduce over RCCL,
deterministic global norm, clip 35 + Adam).  Workload at every N (weak scaling): configs[1] of BASELINE.json,
cfg_kitti_baseline_odometry_boundary_ce_iou_1024_20 — 1024x1024 (the size every reference config uses),
frames [0,-1,1], type static, loss_sum 3, occ 256, fp32, 8 images per GPU.

Rank 0 prints ONE JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step = milliseconds per timed step, ...).
A plain run sets up, warms up, times the K steps and prints it; the objects below are null there.  --full adds them (each
can still be left out with its --no-* option):
  roofline     — the BY-TIME DOMINANT kernel of one instrumented step: every implicit-GEMM dispatch is bracketed by HIP
                 events inside the library, on the stream it is launched on (jp_profile_*); dominant = the kernel
                 instantiation with the largest summed duration.
                 A kernel is priced on the pipe it runs on: EXECUTED MFMA FLOPs / time against 2.5 PFLOP/s (dense bf16) for the
                 split-product patch kernels (P9S / W9S / P9US ...: 3 fp16 products per fp32 product since round 5, 6 bf16 products in a
                 -DJP_NS=3 build; the dense 16-bit MFMA peak is the same for both), against 157.3 TFLOP/s for
                 the exact-fp32 MFMA kernels.  Step-level figures ride along: step_fp32_equiv_tflops = 1.63 TFLOP*B / t_step,
                 achieved_hbm = (9.7 GB*B + 2.3 GB) / t_step, and per-pipe aggregates of all igemm kernels.
  families     — per-kernel-family time / rate table of that step (the whole table is also written to the file named by
                 $JP_BENCH_TABLE).
  cpu_baseline — the oracle (PyTorch-CPU port of the reference step) timed on this host's cores at B=1, SAME flags as
                 the GPU workload (static, 3 frames, loss_sum 3, 1024^2).
  secondary    — clearly labelled, NOT the headline: the shape-agnostic depth/pose/CGT/photometric sub-path at
                 BASELINE.json's 1024(W)x320(H) with the (square-only) layout branch disabled.
  exact_build  — the same workload on the -DJP_NS=3 build of the library (exact_build_figure).

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step computed as DIR/<name>.npy (dump_outputs).
"""
import argparse
import collections
import ctypes
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ARITHMETIC = {
    2: "fp32 in / out / accumulate everywhere; the patch convolutions form each fp32 product as 3 fp16-MFMA products a0 b0 + a0 b1 + a1 b0 of "
       "two-way fp16 splits of both operands, each operand tensor scaled by the power of two that puts its largest magnitude into [2^14, 2^15) "
       "(igemm_p9s.h:jp_split2h, scale.hip): operands carried to 2^-23 relative for elements within 2^-17 of their tensor's largest, 2^-40 of "
       "that largest below; the term left out is <= 2^-22 |a b|.  Measured error vs float64: 0.62-1.00 x the exact-fp32 MFMA kernels' on 48 "
       "layer x pass cases (profiles/r05_fp16x2_accuracy_vs_f64.md; tests/test_split_accuracy_gpu.py holds <= 1.25 x; tools/split_study.py: "
       "the split error is 3-4 x below the fp32 accumulation's own rounding). "
       "Inf / NaN / |x| >= 2^100 inputs: NaN in the outputs that read them.  A -DJP_NS=3 build keeps the exact 3-way bf16 splits (6 products); "
       "JP_P9S=0 JP_W9S=0 JP_P9US=0 selects the exact-fp32 MFMA kernels",
    3: "fp32 in / out / accumulate everywhere; the patch convolutions form each fp32 product as 6 bf16-MFMA "
       "products of exact 3-way bf16 operand splits (igemm_p9s.h): error vs float64 <= the fp32 FMA chain's "
       "(tests/test_split_accuracy_gpu.py) on FINITE inputs (an Inf input yields NaN where fp32 arithmetic yields Inf: "
       "Inf - bf16(Inf), and Inf x a zero residual split); JP_P9S=0 JP_W9S=0 JP_P9US=0 selects the exact-fp32 MFMA kernels",
}


def _scheme():
    """2: the library forms fp32 products from two fp16 splits per operand (3 matrix products), 3: three bf16 splits (6 products)."""
    from jperceiver_amd import ops
    return ops.split_scheme()


SIX_TAGS = ("p1l_tag",)       # split kernels that still run the six-product bf16 scheme


def _products(tag):
    return 6.0 if (_scheme() == 3 or any(k in tag for k in SIX_TAGS)) else 3.0


PEAK_FP32_TF, PEAK_BF16_TF, PEAK_HBM_TBS = 157.3, 2500.0, 8.0     # dense fp32-MFMA / dense bf16-MFMA TFLOP/s, HBM TB/s (MI355X_MICROARCH.md)
SPLIT_TAGS = ("p1l_tag", "p9sm_tag", "p9sw_tag", "p9s_tag", "w9s_tag", "p9us2_tag", "w1s_tag", "p9sd_tag", "w4s_tag", "p9s2d_tag", "p9s2f_tag", "w9s2_tag", "p9sx2_tag", "p7s_tag")     # kernels on the bf16 pipe: 6 bf16 MFMA products per fp32 product (igemm_p9s.h)

# BASELINE.json `configs`, in order.  Per-GPU batch = BASELINE.json's figure (the reference's files carry IMGS_PER_GPU = 1/3/3/3/1
# for a 24 GB card; /root/reference/config/<name>.py:3-6 give frames / size, :19 the type, :47-55 loss_sum / split).  The
# headline (default, --config 1) is configs[1]; the others are selectable so that every config's own workload can be timed
# at any N:  python bench.py --config 3 --gpus 8
CONFIGS = [
    dict(name="cfg_kitti_baseline_odometry_boundary_ce_iou_1024_20_B1", B=1, frames=[0, -1], type="static", split="odometry",
         loss_sum=3, full_hw=(375, 1242), gpus=1),
    dict(name="cfg_kitti_baseline_odometry_boundary_ce_iou_1024_20", B=8, frames=[0, -1, 1], type="static", split="odometry",
         loss_sum=3, full_hw=(375, 1242), gpus=1),
    dict(name="cfg_kitti_baseline_kitti_odom_4gpus", B=12, frames=[0, -1, 1], type="static", split="odometry",
         loss_sum=1, full_hw=(375, 1242), gpus=4),
    dict(name="cfg_kitti_baseline_kitti_odom_8pugsB24_lr1e-4_ce_eigen", B=24, frames=[0, -1, 1], type="static_eigen", split="eigen",
         loss_sum=0, full_hw=(375, 1242), gpus=8),
    dict(name="cfg_kitti_baseline_argo_both_boundary_ce_iou_1024_20_B1", B=1, frames=[0, -1], type="Argo_both", split="argo",
         loss_sum=3, full_hw=(2056, 2464), gpus=8, extra=dict(loss_weightS=20, loss2_weightS=20)),
]


def make_opt(B, H, W=None, frames=(0, -1, 1), ty="static", split="odometry", **kw):
    W = H if W is None else W
    o = dict(name="Baseline", depth_num_layers=18, pose_num_layers=18, frame_ids=list(frames), imgs_per_gpu=B,
             height=H, width=W, scales=[0, 1, 2, 3], min_depth=0.1, max_depth=100.0,
             depth_pretrained_path=None, pose_pretrained_path=None, automask=True, disp_norm=True,
             smoothness_weight=1e-3, scale_weight=0.1, dynamic_weight=15.0, static_weight=5.0,
             occ_map_size=256 if H != W else H // 4, num_class=2, loss_type="iou", loss_weight=20, loss2_type="boundary",
             loss2_weight=20, type=ty, loss_sum=3, split=split)
    o.update(kw)
    return o


def cpu_baseline(HW, cfg, seconds_budget=30.0):
    """Oracle (port of the reference CPU path) on this host: B=1, the GPU workload's own flags (type, loss_sum, split,
    frames, full-resolution frame; label generated by the oracle), 1 warm-up + timed steps."""
    frames = cfg["frames"]
    from oracle import jp_oracle as J
    from jperceiver_amd import synthetic as syn
    # threads = cores this process may actually run on (cgroup/affinity aware), capped: oneDNN oversubscription
    # on a 2-socket box is catastrophically slow
    try:
        ncores = len(os.sched_getaffinity(0))
    except AttributeError:
        ncores = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(ncores, 32)))
    optd = make_opt(1, HW, HW, frames, cfg["type"], cfg["split"], loss_sum=cfg["loss_sum"], **cfg.get("extra", {}))
    opt = J.default_opt(**{k: v for k, v in optd.items() if k != "name"})
    shapes = J.state_shapes(opt.occ_map_size)
    tmpl = {n: torch.empty(s, dtype=torch.long if n.endswith("num_batches_tracked") else torch.float32)
            for n, s in shapes.items()}
    P, Bf = J.make_params(shapes, syn.synth_state_dict(tmpl, seed=0))
    inp = syn.make_batch(1, HW, HW, frames, HW // 4, cfg["full_hw"], cfg["split"], seed=11)
    st = {}
    times = []
    t_begin = time.perf_counter()
    for it in range(8):
        for p in P.values():
            p.grad = None
        t0 = time.perf_counter()
        label = J.make_scale_label(opt, inp)
        out, L = J.forward(P, Bf, opt, inp, True, None, None, label)
        J.total_loss(L).backward()
        J.adam_step(P, st)
        dt = time.perf_counter() - t0
        if it > 0:
            times.append(dt)
        if it >= 2 and time.perf_counter() - t_begin > seconds_budget:
            break
    ms = sum(times) / len(times)
    return dict(value=round(1.0 / ms, 4), unit="images/s", cores=torch.get_num_threads(), kind="port",
                sample=f"{len(times)} timed oracle steps (+1 warm-up), B=1, {HW}x{HW}, {len(frames)} frames, type {cfg['type']}, "
                       f"loss_sum {cfg['loss_sum']} (the GPU workload's flags), {ms:.2f} s/step")


def build_runner(optd, dev, world, rank, batch_kw, step_graph=False):
    from jperceiver_amd import synthetic as syn
    from jperceiver_amd.model import MONO
    from jperceiver_amd.apis import batch_processor, build_optimizer, Runner, DataParallelShell, change_input_variable
    from jperceiver_amd.core import DistOptimizerHook
    model = MONO.module_dict["Baseline"](optd)
    model.load_state_dict(syn.synth_state_dict(model.state_dict(), seed=0))
    model = model.to(dev).train()
    optim = build_optimizer(model, dict(type="Adam", lr=1e-4, weight_decay=0))
    wrapped = DataParallelShell(model) if world > 1 else model
    hook = DistOptimizerHook(grad_clip=dict(max_norm=35, norm_type=2))
    runner = Runner(wrapped, batch_processor, optim, hook, step_graph=step_graph)
    # per-rank shard of the synthetic "dataset"; resident in HBM before timing starts
    batch = syn.make_batch(rank=rank, **batch_kw)
    batch = change_input_variable(batch, device=dev, opt=model.opt)
    torch.cuda.synchronize()
    return runner, batch


PREWARM = 0 if os.environ.get("JP_PMC_CALIB") else int(os.environ.get("JP_BENCH_PREWARM", "30"))     # (counter passes: every launch is replayed)


def timed_steps(runner, batch, steps, warmup, world, dev, log, calibrate=None, prewarm=0):
    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Pre-warm (reported as `prewarm_steps`): a process that is the FIRST on a cold box needs a few seconds of load before the step
    # time settles (measured: 63.9 ms for 20 steps after 5 warm-up steps as the first process on a box, 62.7 after 40, 62.4 / 62.3 for
    # the next processes after 5 -- profiles/r06_bench_repeat_head.log).  These untimed steps come BEFORE the W warm-up steps the
    # caller asked for; the timed region is unchanged.  A fixed count: every rank must issue the same number of exchanges.
    for _ in range(prewarm):
        runner.train_iter(batch)
    if prewarm:
        torch.cuda.synchronize()
    for i in range(warmup):
        t_w = time.perf_counter()
        runner.train_iter(batch)
        torch.cuda.synchronize()
        log(f"warm-up step {i}: {(time.perf_counter() - t_w) * 1e3:.1f} ms")
    if calibrate is not None:
        # --graph auto: the captured replay wins on a slow host and loses on a fast one; time a few
        # un-timed steps each way and keep the faster issue mode for the timed region
        for mode in (True, False):
            runner.step_graph = mode
            runner.train_iter(batch)
            torch.cuda.synchronize()
            t_c = time.perf_counter()
            for _ in range(5):
                runner.train_iter(batch)
            torch.cuda.synchronize()
            calibrate["graph_ms" if mode else "eager_ms"] = round((time.perf_counter() - t_c) / 5 * 1e3, 3)
        runner.step_graph = calibrate["graph_ms"] < calibrate["eager_ms"]
        calibrate["chosen"] = "graph" if runner.step_graph else "eager"
        log(f"--graph auto: {calibrate}")
    sync()
    if world > 1:
        runner.hook.exposed_events = []
    t0 = time.perf_counter()
    for _ in range(steps):
        out = runner.train_iter(batch)
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0           # this rank's own clock (before the closing barrier)
    sync()
    dt = time.perf_counter() - t0
    multi = None
    if world > 1:
        ev = runner.hook.exposed_events or []
        runner.hook.exposed_events = None
        exposed = sum(a.elapsed_time(b) for a, b in ev) / max(1, len(ev))
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
        mine = torch.tensor([dt_own / steps * 1e3, exposed], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        multi = {"backend": dist.get_backend(), "ms_per_step_per_rank": [round(float(e[0]), 3) for e in every],
                 "allreduce_exposed_ms_per_rank": [round(float(e[1]), 3) for e in every],
                 "allreduce_exposed_ms": round(max(float(e[1]) for e in every), 3),
                 "allreduce_bytes_per_step": int(runner.optimizer.arena.live_numel) * 4,
                 "note": "exposed = time the compute stream waits for the bucketed SUM all-reduce after the backward's last "
                         "kernel (core/dist_utils.py); DESIGN.md section 6 estimates 0.35-2.4 ms on xGMI"}
    return dt, out, multi


DUMP_SAMPLE = 4 << 20      # elements kept of a flat vector longer than this (a fixed, seeded sample of its positions)


def dump_outputs(path, runner, out, log):
    """--dump-outputs: what the last timed step handed its caller, as DIR/<name>.npy --
      loss.npy                the summed loss (float64, shape (1,));
      log_vars.<term>.npy     every logged loss term (float64, shape (1,));
      params.npy / grads.npy  all parameters after the step's clip + Adam update and the step's gradients, flattened in
                              state_dict order (float32); longer than DUMP_SAMPLE elements: the positions np.unique of
                              default_rng(0).integers(0, n, DUMP_SAMPLE) -- the same positions for the same model;
      buffers.npy             the BatchNorm running statistics, flattened in state_dict order (float32).
    Inputs, weights and the step's random draws are seeded, so the same arguments give the same inputs in every run."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    model = getattr(runner.model, "module", runner.model)
    loss = out["loss"]
    files = {"loss": np.array([float(loss.detach() if torch.is_tensor(loss) else loss)], dtype=np.float64)}
    for k, v in out["log_vars"].items():
        if k != "loss":       # ('min_reconstruct_loss', 0) -> log_vars.min_reconstruct_loss_0
            files["log_vars." + re.sub(r"[^A-Za-z0-9.-]+", "_", str(k)).strip("_")] = np.array([float(v)], dtype=np.float64)
    named = dict(model.named_parameters())
    sd = model.state_dict()
    pn = [n for n in sd if n in named]
    bn = [n for n in sd if n not in named and sd[n].is_floating_point()]

    def flat(ts, name):
        v = torch.cat([t.detach().reshape(-1).float() for t in ts])
        if v.numel() > DUMP_SAMPLE:
            idx = np.unique(np.random.default_rng(0).integers(0, v.numel(), DUMP_SAMPLE))
            v = v[torch.from_numpy(idx).to(v.device)]
        files[name] = v.cpu().numpy().astype(np.float32)

    flat([sd[n] for n in pn], "params")
    flat([named[n].grad if named[n].grad is not None else torch.zeros_like(named[n]) for n in pn], "grads")
    if bn:
        flat([sd[n] for n in bn], "buffers")
    for name, a in files.items():
        np.save(os.path.join(path, name + ".npy"), a)
    log(f"--dump-outputs: {len(files)} arrays, {sum(a.nbytes for a in files.values()) / 1e6:.1f} MB -> {path}")


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _self_launch(args_list, n):
    """`python bench.py --gpus N` with no rendezvous in the environment (the form of the driver's N=1 command and of the
    reference's one-line launch, /root/reference/readme.md:87, run.py:1-6): start the N ranks ourselves, one process per
    GPU, under torch.distributed.run on 127.0.0.1; rank 0's single JSON line passes through on stdout."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + args_list
    print(f"[bench] launching {n} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=1, choices=range(len(CONFIGS)),
                    help="index into BASELINE.json `configs` (default 1 = the headline workload)")
    ap.add_argument("--batch", type=int, default=None, help="images per GPU (default: the config's, BASELINE.json)")
    ap.add_argument("--hw", type=int, default=1024)
    ap.add_argument("--graph", choices=("auto", "on", "off"), default="auto",
                    help="replay the whole iteration from one captured hipGraph (apis.trainer.CapturedStep); auto = for "
                         "single-process runs with <= 2 images per GPU, time both issue modes in the warm-up and keep the faster")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure the roofline / family table, the secondary 1024x320 workload, the CPU "
                         "baseline and the -DJP_NS=3 build (off: a plain run only times the headline workload)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (loss terms, parameters, gradients, BatchNorm buffers) "
                         "to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true")
    ap.add_argument("--no-exact-build", action="store_true",
                    help="skip timing the -DJP_NS=3 build of the library (csrc/libjperceiver_hip_ns3.so: exact three-way bf16 splits, six products)")
    ap.add_argument("--secondary-only", action="store_true",
                    help="time only the labelled 1024(W)x320(H) secondary workload (for rocprofv3 passes over that shape) and print its block")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_self_launch(sys.argv[1:], args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > torch.cuda.device_count():
        # several ranks time-slicing one GPU (only the 1-GPU gloo smoke test of the N>1 code path does this): the pose
        # branch's side stream turns into cross-process queue ping-pong there, so keep the step single-stream
        os.environ["JP_POSE_STREAM"] = "0"
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local % torch.cuda.device_count())
        # "nccl" == RCCL over xGMI.  JP_DIST_BACKEND=gloo lets the N>1 code path be exercised on a 1-GPU box.
        dist.init_process_group(os.environ.get("JP_DIST_BACKEND", "nccl"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: either launch with torch.distributed.run "
                         f"--nproc-per-node {args.gpus}, or run `python bench.py --gpus {args.gpus}` without WORLD_SIZE set")
    dev = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(dev)

    from jperceiver_amd import _lib

    def log(msg):
        if rank == 0:
            print(f"[bench] {msg}", file=sys.stderr, flush=True)

    cfg = CONFIGS[args.config]
    B, HW, frames = (args.batch or cfg["B"]), args.hw, cfg["frames"]
    if args.secondary_only:
        print(json.dumps({"secondary": secondary_figure(dev, B, log, steps=args.steps, warmup=args.warmup)}), flush=True)
        return
    optd = make_opt(B, HW, HW, frames, cfg["type"], cfg["split"], loss_sum=cfg["loss_sum"], **cfg.get("extra", {}))
    # more than one rank: only on request (--graph on: graph A | eager exchange | graph B, apis/trainer.py); `auto` calibrates per
    # process, and the ranks must not choose differently
    use_graph = args.graph == "on" or (world == 1 and args.graph == "auto" and B <= 2)
    runner, batch = build_runner(optd, dev, world, rank,
                                 dict(B=B, height=HW, width=HW, frame_ids=frames, occ=HW // 4, full_hw=cfg["full_hw"],
                                      split=cfg["split"], seed=1), step_graph=use_graph)
    if use_graph and args.warmup < 3:
        log("note: the captured step needs 2 eager iterations + the capture itself: --warmup < 3 puts them inside the timed region")
    calib = {} if (use_graph and args.graph == "auto") else None
    dt, out, multi = timed_steps(runner, batch, args.steps, args.warmup, world, dev, log, calibrate=calib, prewarm=PREWARM)
    use_graph = bool(runner.step_graph)
    ms = dt / args.steps * 1e3
    value = B * world * args.steps / dt
    log(f"{args.steps} timed steps: {ms:.1f} ms/step, {value:.2f} images/s")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, runner, out, log)
    if os.environ.get("JP_PMC_CALIB") and rank == 0:
        # known-byte streaming copy (4 B/lane loads and stores, the igemm gather's access width) so that the
        # FETCH_SIZE / WRITE_SIZE counters of a rocprofv3 --pmc pass can be calibrated (MI355X_MICROARCH.md §HBM)
        n = 1 << 28
        a, b = torch.empty(n, device=dev), torch.empty(n, device=dev)
        for _ in range(3):
            _lib.call("jp_axpby", a, None, b, n, 1.0, 0.0)
        torch.cuda.synchronize()
        del a, b
    roof, fam, cpu, sec = None, None, None, None
    if args.full and not args.no_roofline:
        # every rank runs the instrumented step (it contains the gradient all-reduce); rank 0 reports
        runner.step_graph = False          # the instrumented step is issued launch by launch (HIP events around each)
        roof, fam = measure_roofline(runner, batch, B, ms * 1e-3, rank)
        log(f"roofline: {json.dumps(roof)}")
    if world > 1:
        dist.barrier()
    del runner, batch
    torch.cuda.empty_cache()
    if args.full and rank == 0 and world == 1 and not args.no_secondary and args.config == 1:
        sec = secondary_figure(dev, B, log)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        log("timing the CPU baseline (oracle) ...")
        cpu = cpu_baseline(HW, cfg)
    exact = None
    if args.full and rank == 0 and world == 1 and not args.no_exact_build and not os.environ.get("JP_LIB_PATH"):
        exact = exact_build_figure(args, log)
    if rank == 0:
        line = {
            "metric": f"train images/sec (full train step, synthetic {len(frames)}-frame batches)", "value": round(value, 3),
            "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "prewarm_steps": PREWARM,       # untimed steps before the W warm-up steps (cold-box settling, see timed_steps)
            "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "arithmetic": ARITHMETIC[_scheme()],
            "workload_note": "random-init network: its disparity is pixel noise, so the CGT warp kernels' gathers are L2-miss-bound here "
                             "(cgt_warp_bwd: 6.3 x its algorithmic bytes, 2.3 x / 1.3 x slower than on a smooth disparity, DESIGN 4.5); "
                             "the photometric family is overstated by ~1 ms per step against a trained network",
            "config": {"workload": f"{cfg['name']}: {HW}x{HW}, frames {frames}, {B} images/GPU, type {cfg['type']}, "
                                   f"loss_sum {cfg['loss_sum']}, occ {HW // 4}, full-res frame {cfg['full_hw'][0]}x{cfg['full_hw'][1]}",
                       "config_index": args.config, "global_batch": B * world,
                       "parallelism": f"dp{world}", "loss": float(out["log_vars"]["loss"]),
                       "step_graph": bool(use_graph), "step_graph_calibration": calib},
            "roofline": roof, "cpu_baseline": cpu, "families": fam, "secondary": sec, "exact_build": exact,
        }
        if multi is not None:
            line["multi_gpu"] = multi
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


def exact_build_figure(args, log, steps=5, warmup=2):
    """The SAME workload on the -DJP_NS=3 build of the same tree (make ns3: every fp32 product of the patch kernels = 6 bf16 products
    of exact three-way operand splits, no per-tensor operand scales -- the arithmetic of rounds 3-4), so that the driver's
    record carries both arithmetics: `value` above is the default build's three fp16 products of power-of-two-scaled two-way splits
    (DESIGN 4.6b).  Timed in a child process (the library is chosen at load time, JP_LIB_PATH)."""
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jperceiver_amd", "csrc", "libjperceiver_hip_ns3.so")
    if not os.path.exists(so):
        return {"skipped": "csrc/libjperceiver_hip_ns3.so not built (make -C jperceiver_amd/csrc ns3)"}
    cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--warmup", str(warmup), "--config", str(args.config),
           "--hw", str(args.hw), "--graph", args.graph, "--no-cpu-baseline", "--no-roofline", "--no-secondary", "--no-exact-build"]
    if args.batch:
        cmd += ["--batch", str(args.batch)]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, JP_LIB_PATH=so), capture_output=True, text=True, timeout=600)
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        res = {"arithmetic": line["arithmetic"], "library": "csrc/libjperceiver_hip_ns3.so (-DJP_NS=3)", "value": line["value"],
               "unit": "images/s", "ms_per_step": line["ms_per_step"], "steps": steps, "warmup": warmup, "loss": line["config"]["loss"]}
        log(f"exact build (-DJP_NS=3): {res['value']} images/s ({res['ms_per_step']} ms/step)")
        return res
    except Exception as e:     # the headline must not depend on the second library
        return {"error": repr(e)}


def secondary_figure(dev, B, log, steps=6, warmup=2):
    """BASELINE.json names "1024x320"; the reference itself cannot run non-square inputs (CVP / CCT need square maps,
    SURVEY.md §0).  Secondary, clearly labelled: the shape-agnostic sub-path (depth encoder/decoder, pose networks,
    CGT warp, photometric + SSIM + automask, smoothness, CGT scale label + loss, backward, clip + Adam) at
    H=320, W=1024 with the layout branch disabled.  Parity at this shape: tests/test_subpath_320x1024_gpu.py (the reference's
    own modules at 320x1024 -> tests/golden/subpath_320x1024_b2.npz, and this exact workload against the oracle)."""
    try:
        frames = [0, -1, 1]
        optd = make_opt(B, 320, 1024, frames, layout_branch=False)
        # 921 launches of ~28 us per step: on a box with a slow host this workload is launch-bound (258 vs 304 images/s measured on
        # two boxes of the pool with the same tree), so -- like the one-image configs -- both issue modes are timed in the warm-up
        # and the faster one is kept (the captured hipGraph replays the same kernels, bit for bit: tests/test_step_graph_gpu.py)
        runner, batch = build_runner(optd, dev, 1, 0, dict(B=B, height=320, width=1024, frame_ids=frames, occ=256,
                                                           full_hw=(375, 1242), split="odometry", seed=1), step_graph=True)
        calib = {}
        dt, out, _ = timed_steps(runner, batch, steps, max(warmup, 3), 1, dev, lambda m: None, calibrate=calib)
        ms = dt / steps * 1e3
        res = {"workload": f"SECONDARY (not the headline): 1024(W)x320(H), frames {frames}, {B} images/GPU, "
                           "depth + pose + CGT warp + photometric/SSIM/automask + smoothness + scale losses, backward, "
                           "clip + Adam; BEV-layout branch disabled (the reference's CVP/CCT need square inputs)",
               "parity": "tests/test_subpath_320x1024_gpu.py (reference-generated fixture at 320x1024 + oracle on this workload)",
               "value": round(B * steps / dt, 3), "unit": "images/s", "ms_per_step": round(ms, 3), "steps": steps,
               "warmup": max(warmup, 3), "loss": float(out["log_vars"]["loss"]), "step_graph": bool(runner.step_graph),
               "step_graph_calibration": calib}
        log(f"secondary figure: {res['value']} images/s ({res['ms_per_step']} ms/step) at 1024x320 without the layout branch")
        return res
    except Exception as e:     # the headline must not depend on the secondary figure
        log(f"secondary figure failed: {e!r}")
        return {"workload": "SECONDARY 1024x320 sub-path", "error": repr(e)}


# ------------------------------------------------------------------------------------------------- instrumented step
def _conv_shape(name, a):
    """-> (kind, algorithmic FLOPs, algorithmic bytes) of one conv entry-point call (ABI argument order)."""
    if name == "jp_conv2d_fwd_src3":
        cin, N, H, W, Cout, KH, s, p = a[1] + a[4] + a[7], a[12], a[13], a[14], a[15], a[16], a[17], a[18]
        kind = "fwd"
    elif name == "jp_conv2d_dgrad":
        N, cin, H, W, Cout, KH, s, p = a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]
        kind = "dgrad"
    elif name == "jp_conv2d_dgrad_src3":
        cin = sum(c for d, c in ((a[2], a[3]), (a[6], a[7]), (a[10], a[11])) if d is not None)
        N, H, W, Cout, KH, s, p = a[14], a[15], a[16], a[17], a[18], a[19], a[20]
        kind = "dgrad"
    elif name == "jp_conv2d_wgrad_src3":
        cin, N, H, W, Cout, KH, s, p = a[1] + a[4] + a[7], a[11], a[12], a[13], a[14], a[15], a[16], a[17]
        kind = "wgrad"
    else:
        return None
    OH, OW = (H + 2 * p - KH) // s + 1, (W + 2 * p - KH) // s + 1
    fl = 2.0 * N * OH * OW * Cout * cin * KH * KH
    by = 4.0 * (N * cin * H * W + N * Cout * OH * OW + Cout * cin * KH * KH)
    return kind, fl, by


def _hbm_bytes(name, a):
    """Algorithmic HBM bytes of one call of an HBM-bound entry point (every tensor the op must read or write, once per
    pass the algorithm needs; ABI argument order, include/jperceiver_hip.h) -- None for entry points not modelled."""
    try:
        if name == "jp_bn_train_fwd":            # pass 1 reads x (statistics), pass 2 reads x (+ residual), writes y
            E = a[10] * a[11] * a[12]
            return 4.0 * E * (3 + (a[3] is not None))
        if name == "jp_bn_train_bwd":            # reduce: dy, x (+ y for the ReLU mask); apply: the same + dx (+ dres)
            E = a[12] * a[13] * a[14]
            r = 1 if a[15] else 0
            return 4.0 * E * (2 * (2 + r) + 1 + (a[8] is not None))
        if name == "jp_maxpool_fwd":
            NC, H, W, k, s_, p_ = a[3:9]
            OH, OW = (H + 2 * p_ - k) // s_ + 1, (W + 2 * p_ - k) // s_ + 1
            return NC * (4.0 * H * W + 5.0 * OH * OW)
        if name == "jp_maxpool_bwd":
            NC, H, W, k, s_, p_ = a[4:10]
            OH, OW = (H + 2 * p_ - k) // s_ + 1, (W + 2 * p_ - k) // s_ + 1
            return NC * (5.0 * OH * OW + 4.0 * H * W * (1 + (a[3] is not None)))
        if name == "jp_cgt_warp_fwd":            # disparity (source scale), colour gather, pred
            B, H, W = a[7:10]
            return 4.0 * B * (a[1] * a[2] + 6 * H * W)
        if name == "jp_cgt_warp_bwd":            # dpred, disparity, colour gather, ddisp_up
            B, H, W = a[9:12]
            return 4.0 * B * (a[2] * a[3] + 7 * H * W)
        if name == "jp_ssim_l1_fwd":
            return 4.0 * a[3] * a[4] * a[5] * 7
        if name == "jp_ssim_l1_bwd":             # pred, target, min index (int64), gout, dpred
            return a[7] * a[8] * a[9] * (12.0 + 12 + 8 + 4 + 12)
        if name == "jp_adam_clip_step":
            return 28.0 * a[4]
        if name == "jp_sum_n":
            return 4.0 * a[6] * (1 + sum(x is not None for x in a[:5]))
        if name == "jp_axpby":
            return 4.0 * a[3] * (2 + (a[1] is not None))
        if name == "jp_act_bwd":
            return 12.0 * a[3]
        if name == "jp_upsample2x_fwd":
            return 4.0 * a[2] * a[3] * a[4] * a[5] * 5
        if name == "jp_upsample2x_bwd":
            return 4.0 * a[2] * a[3] * a[4] * a[5] * 5
    except (TypeError, IndexError):
        return None
    return None


_FAMILY = [("jp_bn_", "batchnorm"), ("jp_maxpool", "pool"), ("jp_cgt_warp", "photometric"), ("jp_ssim", "photometric"),
           ("jp_minreproj", "photometric"), ("jp_pose", "photometric"), ("jp_smooth", "losses"), ("jp_scale_loss", "losses"),
           ("jp_layout", "losses"), ("jp_sdf", "losses"), ("jp_l1", "losses"), ("jp_adam", "optimizer"),
           ("jp_grad_sumsq", "optimizer"), ("jp_sum_doubles", "optimizer"), ("jp_pack_replay", "weight pack"),
           ("jp_conv2d_", "conv")]


def _kernel_name(tag):
    """launch helper's __PRETTY_FUNCTION__ -> the kernel's name as rocprofv3 prints it."""
    m = re.search(r"\[(.*)\]\s*$", tag)
    if not m:
        return tag
    parts, depth, cur = [], 0, ""
    for ch in m.group(1):
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    parts.append(cur.strip())
    kv = dict(p.split(" = ", 1) for p in parts if " = " in p)
    kv = {k: v.replace("(anonymous namespace)::", "") for k, v in kv.items()}
    if "p9sw_tag" in tag:
        taps = kv.get("TAPS", "1")
        return f"jp_igemm_p9s_wide_kernel<{kv['WM']}, {kv['WN']}, {kv['REFLECT']}, {kv['REV']}, {kv['E']}, {taps}, {1 if taps == '9' else 2}>"
    if "p9sm_tag" in tag:
        return f"jp_igemm_p9sm_kernel<{kv['WM']}, {kv['WN']}, {kv['REFLECT']}, {kv['REV']}, {kv['E']}, {kv['TAPS']}>"
    if "p9s_tag" in tag:
        taps = kv.get("TAPS", "9")
        return f"jp_igemm_p9s_kernel<{kv['WM']}, {kv['WN']}, 2, {kv['REFLECT']}, {kv['REV']}, {kv['E']}, {taps}, {1 if taps == '9' else 2}>"
    if "p9_tag" in tag:
        taps = kv.get("TAPS", "9")          # rocprofv3 prints the defaulted TAPS / CPB arguments too: 9, 1 (3x3) or 1, 2 (1x1)
        return f"jp_igemm_p9_kernel<{kv['WM']}, {kv['WN']}, {kv['REFLECT']}, {kv['REV']}, {kv['E']}, {taps}, {2 if taps == '1' else 1}>"
    if "w9s2_tag" in tag:
        return f"jp_wgrad_w9s2_kernel<{kv['KG']}>"
    if "w1s_tag" in tag:
        return "jp_wgrad_w1s_kernel"
    if "w1_tag" in tag:
        return "jp_wgrad_w1_kernel"
    if "w7_tag" in tag:
        return f"jp_wgrad_w7_kernel<{kv['CIN']}>"
    if "p7s_tag" in tag:
        return f"jp_igemm_p7s_kernel<{kv['CIN']}, {kv['E']}>"
    if "p9sx2_tag" in tag:
        return f"jp_igemm_p9s_x2_kernel<{kv['WM']}, {kv['WN']}, 2, {kv['E']}>"
    if "p9s2f_tag" in tag:
        return f"jp_igemm_p9s2f_kernel<{kv['E']}>"
    if "p9s2d_tag" in tag:
        return f"jp_igemm_p9s2d_kernel<{kv['WM']}, {kv['WN']}, 2, {kv['E']}>"
    if "w4s_tag" in tag:
        return f"jp_wgrad_w4s_kernel<{kv['TR']}>"
    if "p9sd_tag" in tag:
        return f"jp_igemm_p9sd_kernel<{kv['E']}>"
    if "p1l_tag" in tag:
        return f"jp_conv1x1_p1l_kernel<{kv['E']}>"
    if "p9us2_tag" in tag:
        return f"jp_igemm_p9us2_kernel<{kv['E']}>"
    if "p9u_tag" in tag:
        return f"jp_igemm_p9u_kernel<{kv['E']}>"
    if "w9s_tag" in tag:
        return f"jp_wgrad_w9s_kernel<{kv['TR']}, {kv['REFLECT']}, {kv.get('KG', '1')}, {kv.get('NCB', '2')}>"
    if "w9_tag" in tag:
        return f"jp_wgrad_w9_kernel<{kv['MW']}, 2, {kv['KG']}, {kv['REFLECT']}>"
    if "launch_r3" in tag:
        return f"jp_igemm_r3_kernel<{kv['WM']}, {kv['WN']}, 32, {kv['A']}, {kv['B']}, {kv['E']}>"
    return f"jp_igemm_kernel<{kv['WM']}, {kv['WN']}, 32, {kv['A']}, {kv['B']}, {kv['E']}, false, {kv['IL']}>"


def measure_roofline(runner, batch, B, t_step, rank):
    from jperceiver_amd import _lib, ops, ops_loss, runtime
    from jperceiver_amd.model import net as netmod, modules as mods, losses as lossmod
    from jperceiver_amd.core import dist_utils
    L = _lib.lib()
    orig = _lib.call
    calls = []          # (name, e0, e1, rec_lo, rec_hi, conv-shape or None)
    call_args = []

    def timed_call(name, *a):
        st = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lo = L.fn["jp_profile_count"]()
        e0.record(st)
        orig(name, *a)
        e1.record(st)
        calls.append((name, e0, e1, lo, L.fn["jp_profile_count"](), _conv_shape(name, a)))
        call_args.append(a)

    patched = [m for m in (_lib, ops, ops_loss, runtime, netmod, mods, lossmod, dist_utils) if getattr(m, "call", None) is orig]
    # The instrumented step runs SINGLE-STREAM: with the side stream active an event pair also brackets the time a
    # kernel waits for (or shares the CUs with) the other stream's kernels, which is not that kernel's duration.
    side_was, wg_was = netmod._POSE_STREAM, ops._WG_ON
    began = False
    netmod._POSE_STREAM = False
    ops._WG_ON = False            # parameter-gradient kernels on the main stream too (no companion streams)
    try:
        # one un-timed step in the same single-stream mode first: its allocation pattern differs from the overlapped steps',
        # and a kernel that is the first to touch freshly mapped scratch pays the page faults (a 75 us launch measured 2.9 ms)
        runner.train_iter(batch)
        torch.cuda.synchronize()
        if L.fn["jp_profile_begin"](8192) != 0:
            raise RuntimeError(L.last_error())
        began = True
        for m in patched:
            m.call = timed_call
        runner.train_iter(batch)
        torch.cuda.synchronize()
    finally:
        netmod._POSE_STREAM = side_was
        ops._WG_ON = wg_was
        for m in patched:
            m.call = orig
        nrec = L.fn["jp_profile_end"]() if began else 0
    # ---- per igemm dispatch: tag, executed FLOPs (2*M*N*K of the GEMM), HIP-event milliseconds
    buf, fl, msv = ctypes.create_string_buffer(512), ctypes.c_double(), ctypes.c_float()
    recs = []
    for i in range(nrec):
        rc = L.fn["jp_profile_get"](i, ctypes.cast(buf, ctypes.c_void_p), 512, ctypes.cast(ctypes.pointer(fl), ctypes.c_void_p),
                                    ctypes.cast(ctypes.pointer(msv), ctypes.c_void_p))
        if rc != 0:
            raise RuntimeError(L.last_error())
        tag = buf.value.decode()
        split = any(k in tag for k in SPLIT_TAGS)
        # [tag, executed MFMA FLOPs, ms, algorithmic FLOPs, algorithmic bytes, fp32-equivalent executed FLOPs]
        recs.append([tag, fl.value, msv.value, 0.0, 0.0, fl.value / _products(tag) if split else fl.value])
    fam = collections.OrderedDict()
    by_name = {}
    conv_alg = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}
    for name, e0, e1, lo, hi, shp in calls:
        t = e0.elapsed_time(e1)
        bn_ = by_name.setdefault(name, [0, 0.0])
        bn_[0] += 1
        bn_[1] += t
        f = next((fam_name for pre, fam_name in _FAMILY if name.startswith(pre)), "elementwise / other")
        if shp is not None:
            f = "conv " + shp[0]
            conv_alg[shp[0]] += shp[1]
            sub = recs[lo:hi]
            if sub:
                # The layer's algorithmic work goes to its main kernel(s); border / fold passes get none.  Plain GEMM
                # kernels are credited what they execute (2*M*N*K, never more than the layer's nominal FLOPs); only the
                # parity-class kernels (pre-summed weight slots: fewer executed than nominal FLOPs) get the remainder.
                # (r[5] = executed FLOPs in fp32 products: a split-bf16 kernel issues 6 bf16 MFMA FLOPs per fp32 FLOP)
                big = max(r[5] for r in sub)
                main = [r for r in sub if r[5] >= 0.1 * big]
                par = [r for r in main if re.search(r"FwdBP|WgradBP|DgradUPB|DgradS2B|p9u_tag|p9us2_tag|p9sd_tag|w4s_tag", r[0]) and "p9_tag" not in r[0]]
                plain = [r for r in main if r not in par]
                left = shp[1]
                tot_plain = sum(r[5] for r in plain)
                for r in plain:
                    a = r[5] if (par or tot_plain <= shp[1]) else shp[1] * r[5] / tot_plain
                    a = min(a, left)
                    r[3] += a
                    left -= a
                tot_par = sum(r[5] for r in par)
                for r in par:
                    r[3] += max(left, 0.0) * r[5] / tot_par
                tot = sum(r[5] for r in main)
                for r in main:
                    r[4] += shp[2] * r[5] / tot
        d = fam.setdefault(f, {"calls": 0, "ms": 0.0})
        d["calls"] += 1
        d["ms"] += t
    kern = {}
    for tag, flx, msx, alg, byt, _f32 in recs:
        k = kern.setdefault(tag, {"launches": 0, "ms": 0.0, "executed_flop": 0.0, "algorithmic_flop": 0.0, "alg_bytes": 0.0})
        k["launches"] += 1
        k["ms"] += msx
        k["executed_flop"] += flx
        k["algorithmic_flop"] += alg
        k["alg_bytes"] += byt
    # by-time dominant kernel among those that carry layer work (border / fold passes are credited no FLOPs: on tiny smoke
    # configurations such a latency-bound pass can be the longest single instantiation)
    cand = {t: k for t, k in kern.items() if k["algorithmic_flop"] > 0} or kern
    dom_tag, dom = max(cand.items(), key=lambda kv: kv[1]["ms"])
    ig_ms = sum(k["ms"] for k in kern.values())
    ig_alg = sum(k["algorithmic_flop"] for k in kern.values())
    # the dominant kernel is priced on the pipe it runs on: EXECUTED MFMA FLOPs / time against that pipe's dense peak -- bf16
    # (2.5 PF) for the split-product kernels, fp32 (157.3 TF) for the exact-fp32 ones; parity-class kernels execute fewer
    # FLOPs than the layer's nominal count and are priced on what they execute, so nothing can exceed its peak
    dom_split = any(k in dom_tag for k in SPLIT_TAGS)
    peak = PEAK_BF16_TF if dom_split else PEAK_FP32_TF
    ach = dom["executed_flop"] / (dom["ms"] * 1e-3) / 1e12
    name = _kernel_name(dom_tag)
    ms_split = sum(k["ms"] for t, k in kern.items() if any(x in t for x in SPLIT_TAGS))
    ex_split = sum(k["executed_flop"] for t, k in kern.items() if any(x in t for x in SPLIT_TAGS))
    ms_f32 = sum(k["ms"] for t, k in kern.items() if not any(x in t for x in SPLIT_TAGS))
    ex_f32 = sum(k["executed_flop"] for t, k in kern.items() if not any(x in t for x in SPLIT_TAGS))
    traffic = None
    try:    # HBM/fabric bytes per launch of this kernel from the committed rocprofv3 --pmc passes (tools/pmc_traffic.py)
        import glob
        f = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))[-1]
        j = json.load(open(f))
        # rocprofv3 prints default template arguments too: compare without the closing '>'
        if j.get("kernel", "").replace(" ", "").startswith(name.replace(" ", "").rstrip(">")):
            traffic = round(j["traffic_bytes_per_launch"])
    except Exception:
        pass
    conv_total = sum(conv_alg.values())
    bf16_frac = ex_split / max(ms_split, 1e-9) / 1e9 / PEAK_BF16_TF
    f32_frac = ex_f32 / max(ms_f32, 1e-9) / 1e9 / PEAK_FP32_TF
    hbm_ms = sum(v["ms"] for k, v in fam.items() if not k.startswith("conv "))
    # the step against the bound that binds it now: every fp32 convolution FLOP of the step (1.63 TFLOP per
    # image-step) costs 6 bf16-MFMA FLOPs when formed from exact operand splits, priced at the 2.5 PF dense bf16 peak
    NP = 3 if _scheme() == 2 else 6
    step_bound = 1.63e12 * B * NP / t_step / (PEAK_BF16_TF * 1e12)
    # key order: the driver's parser keeps a bounded set of scalars -- the step-level figures come right after `frac`
    roof = {"bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(ach / peak, 4), "traffic": traffic,
            "step_bf16_bound_frac": round(step_bound, 4), "products_per_fp32_product": NP,
            # rounds 3-5a priced the step against SIX products per fp32 product (31.3 ms at B = 8): the same step on that scale
            "step_six_product_bound_frac": round(1.63e12 * B * 6 / t_step / (PEAK_BF16_TF * 1e12), 4),
            "bf16_pipe_frac": round(bf16_frac, 4), "fp32_pipe_frac": round(f32_frac, 4),
            "fp32_pipe_ms": round(ms_f32, 2), "bf16_pipe_ms": round(ms_split, 2), "hbm_kernels_ms": round(hbm_ms, 2),
            "kernel": name + " — by-time dominant igemm instantiation of the step",
            "pipe": (("fp16 MFMA (dense 16-bit peak 2.5 PF), fp32 products as 3 fp16 products of 2-way splits of power-of-two-scaled operands "
                      "(fp32 in/out/accumulate)" if _products(dom_tag) == 3.0 else
                      "bf16 MFMA, fp32 products as 6 bf16 products of 3-way operand splits (fp32 in/out/accumulate)") if dom_split
                     else "fp32 MFMA (exact)"),
            "launches": dom["launches"], "avg_launch_ms": round(dom["ms"] / dom["launches"], 4),
            "total_ms_per_step": round(dom["ms"], 3),
            "avg_launch_gflop": round(dom["algorithmic_flop"] / dom["launches"] / 1e9, 2),
            "executed_tflops": round(ach, 2),
            # the same kernel in fp32 FLOPs of the layer it computes (what an fp32-MFMA kernel would be priced on)
            "algorithmic_fp32_tflops": round(dom["algorithmic_flop"] / (dom["ms"] * 1e-3) / 1e12, 2),
            "algorithmic_bytes_per_launch": round(dom["alg_bytes"] / dom["launches"]),
            "step_fp32_equiv_tflops": round(1.63e12 * B / t_step / 1e12, 2),
            "step_conv_tflop_counted": round(conv_total / 1e12, 3),
            "achieved_hbm_tbs": round((9.7e9 * B + 2.3e9) / t_step / 1e12, 3),
            "achieved_hbm_frac": round((9.7e9 * B + 2.3e9) / t_step / (PEAK_HBM_TBS * 1e12), 4),
            # all implicit-GEMM kernels of the step, per pipe: executed MFMA TFLOP/s against that pipe's dense peak
            "igemm_ms_per_step": round(ig_ms, 2), "igemm_fp32_equiv_tflops": round(ig_alg / (ig_ms * 1e-3) / 1e12, 2),
            "bf16_pipe_executed_tflops": round(ex_split / max(ms_split, 1e-9) / 1e9, 1),
            "fp32_pipe_executed_tflops": round(ex_f32 / max(ms_f32, 1e-9) / 1e9, 1)}
    table = {"step_ms_timed": round(t_step * 1e3, 2),
             "entry_points": {k: {"calls": v[0], "ms": round(v[1], 3)} for k, v in sorted(by_name.items(), key=lambda kv: -kv[1][1])},
             "families": {k: {"calls": v["calls"], "ms": round(v["ms"], 3)} for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])},
             "conv_algorithmic_tflop": {k: round(v / 1e12, 3) for k, v in conv_alg.items()},
             "igemm_kernels": [{"kernel": _kernel_name(t), "launches": k["launches"], "ms": round(k["ms"], 3),
                                "algorithmic_tflops": round(k["algorithmic_flop"] / max(k["ms"], 1e-9) / 1e9, 1),
                                "executed_tflops": round(k["executed_flop"] / max(k["ms"], 1e-9) / 1e9, 1)}
                               for t, k in sorted(kern.items(), key=lambda kv: -kv[1]["ms"])[:24]]}
    if os.environ.get("JP_BENCH_DUMP"):          # raw records for offline checks of the tables below
        json.dump({"recs": [[_kernel_name(r[0]), r[1], r[2]] for r in recs],
                   "calls": [[c[0], c[1].elapsed_time(c[2]), c[3], c[4],
                              [x for x in a if isinstance(x, int) and not isinstance(x, bool) and abs(x) < (1 << 28)]]
                             for c, a in zip(calls, call_args)]}, open(os.environ["JP_BENCH_DUMP"], "w"))
    # every conv entry-point call of the step: integer arguments (ABI order), event ms, the kernels it launched
    layers = collections.OrderedDict()
    for (name, e0, e1, lo, hi, shp), args in zip(calls, call_args):
        if shp is None:
            continue
        key = (name, tuple(x for x in args if isinstance(x, int) and not isinstance(x, bool) and abs(x) < (1 << 20)),
               tuple(_kernel_name(r[0]) for r in recs[lo:hi]))
        d = layers.setdefault(key, {"calls": 0, "ms": 0.0, "kernel_ms": [0.0] * (hi - lo)})
        d["calls"] += 1
        d["ms"] += e0.elapsed_time(e1)
        d["kernel_ms"] = [x + r[2] for x, r in zip(d["kernel_ms"], recs[lo:hi])]
    table["conv_calls"] = [{"entry": k[0], "ints": list(k[1]), "calls": v["calls"], "ms": round(v["ms"], 3),
                            "kernels": [f"{n} {m:.3f}" for n, m in zip(k[2], v["kernel_ms"])]}
                           for k, v in sorted(layers.items(), key=lambda kv: -kv[1]["ms"])]
    # HBM-bound entry points: algorithmic bytes against the event time of the same (single-stream) step
    hb, hb_shape = {}, {}
    for (name, e0, e1, lo, hi, shp), args in zip(calls, call_args):
        by = _hbm_bytes(name, args)
        if by is None:
            continue
        ints = tuple(x for x in args if isinstance(x, int) and not isinstance(x, bool) and abs(x) < (1 << 28))
        for d in (hb.setdefault(name, [0, 0.0, 0.0]), hb_shape.setdefault((name, ints), [0, 0.0, 0.0])):
            d[0] += 1
            d[1] += e0.elapsed_time(e1)
            d[2] += by
    table["hbm_calls"] = [{"entry": k[0], "ints": list(k[1]), "calls": v[0], "ms": round(v[1], 3),
                           "algorithmic_TBps": round(v[2] / max(v[1], 1e-9) / 1e9, 2)}
                          for k, v in sorted(hb_shape.items(), key=lambda kv: -kv[1][1])[:40]]
    table["hbm_entry_points"] = [{"entry": k, "calls": v[0], "ms": round(v[1], 3), "algorithmic_GB": round(v[2] / 1e9, 3),
                                  "algorithmic_TBps": round(v[2] / max(v[1], 1e-9) / 1e9, 2)}
                                 for k, v in sorted(hb.items(), key=lambda kv: -kv[1][1])]
    for k, v in table["families"].items():
        if k.startswith("conv ") and v["ms"] > 0:
            v["algorithmic_tflops"] = round(conv_alg[k[5:]] / (v["ms"] * 1e-3) / 1e12, 1)
    if rank == 0:
        path = os.environ.get("JP_BENCH_TABLE")
        if path is None and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
            path = os.path.join(ROOT, "gpurun_out", "bench_families.json")
        if path:
            try:
                json.dump({"roofline": roof, **table}, open(path, "w"), indent=1)
            except OSError:
                pass
    fam_short = {k: v["ms"] for k, v in table["families"].items()}
    return roof, fam_short


if __name__ == "__main__":
    main()
