"""Two data-parallel ranks on ONE MI355X (backend gloo, both processes on cuda:0) through the real product path:
`Runner.train_iter` -> `batch_processor` -> `DistOptimizerHook.after_train_iter` with the flat-arena `FlatAdam`,
i.e. the tape-driven overlapped bucket all-reduce, the two-phase deterministic global norm and the fused clip+Adam
with grad_scale = 1/world (mono/core/utils/dist_utils.py:12-60, mono/apis/trainer.py:167).

Checked per rank:  the arena holds g_0 + g_1 after the exchange (each rank's local gradients are measured in a
separate, hook-free backward on the same inputs);  the parameters after the step equal the oracle's reference-ordered
clip+Adam applied to the exchanged arena / world, i.e. the MEAN gradient (<= 1e-6);  both replicas end bit-identical (SHA-1 of the parameter arena);
the dead tail is untouched.  (The 8-GPU RCCL run itself belongs to the driver; the rendezvous here is 127.0.0.1.)"""
import hashlib
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, ty, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
        torch.cuda.set_device(0)
        from jperceiver_amd import synthetic as syn
        from jperceiver_amd.model import MONO
        from jperceiver_amd.apis import batch_processor, build_optimizer, Runner, DataParallelShell, init_dist
        from jperceiver_amd.core import DistOptimizerHook
        from oracle import jp_oracle as J
        init_dist("pytorch", backend="gloo")
        HW, B, FR = 256, 1, [0, -1, 1]
        opt = J.default_opt(frame_ids=FR, imgs_per_gpu=B, height=HW, width=HW, occ_map_size=HW // 4, type=ty,
                            split="odometry")
        model = MONO.module_dict["Baseline"](opt)
        # rank 1 starts from different weights: the wrap-time broadcast must make the replicas identical
        model.load_state_dict(syn.synth_state_dict(model.state_dict(), seed=rank))
        model = model.cuda().train()
        optim = build_optimizer(model, dict(type="Adam", lr=1e-4, weight_decay=0))
        shell = DataParallelShell(model)
        runner = Runner(shell, batch_processor, optim, DistOptimizerHook(grad_clip=dict(max_norm=35, norm_type=2),
                                                                         bucket_size_mb=16))

        def batch():
            d = syn.make_batch(B, HW, HW, FR, HW // 4, (94, 311), "odometry", seed=31, rank=rank)
            m = syn.make_dropout_masks(B, HW, HW, seed=31, rank=rank)
            d[("dropout_mask", 0)], d[("dropout_mask", 1)] = m
            for s, per in enumerate(syn.make_automask_noise(B, HW, HW, 4, 2, seed=31, rank=rank)):
                for j, nz in enumerate(per):
                    d[("automask_noise", s, j)] = nz
            return d

        a = optim.arena
        p_before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
        # (1) local gradients, no exchange
        optim.zero_grad()
        out = batch_processor(shell, batch(), True)
        out["loss"].backward()
        torch.cuda.synchronize()
        g_local = a.grads.detach().cpu().clone()
        # (2) the real step
        runner.train_iter(batch())
        torch.cuda.synchronize()
        g_sum = a.grads.detach().cpu().clone()
        both = [torch.zeros_like(g_local) for _ in range(world)]
        dist.all_gather(both, g_local)
        expect = both[0] + both[1]
        live = a.live_numel
        err_sum = float((g_sum[:live] - expect[:live]).norm() / expect[:live].norm())
        tail_untouched = bool(torch.equal(g_sum[live:], g_local[live:]))
        # (3) oracle clip+Adam on the mean gradient = the exchanged arena / world.  (The arena of THIS step, not
        # g_local's sum: Adam's first update is lr*g/(|g|+1e-8), so the ~1e-6 relative run-to-run noise of two separate
        # backward passes would move weights whose gradient is ~1e-8 by a good fraction of lr.)
        P = {}
        for n, p, o, k in a.entries[:a.n_live_entries]:
            t = p_before[n].clone().requires_grad_(True)
            t.grad = (g_sum[o:o + k] / world).view(t.shape).clone()
            P[n] = t
        norm_ref = J.adam_step(P, {}, lr=1e-4, max_norm=35.0)
        worst = max(float((p.detach().cpu() - P[n].detach()).abs().max()) for n, p in model.named_parameters() if n in P)
        dead_moved = max([float((p.detach().cpu() - p_before[n]).abs().max()) for n, p in model.named_parameters() if n not in P] or [0.0])
        norm_hip = float(a.normsq.sqrt()) / world          # the kernel scales the norm of the SUM by grad_scale
        digest = hashlib.sha1(a.params.detach().cpu().numpy().tobytes()).hexdigest()
        first_w = float(p_before["DepthEncoder.encoder.conv1.weight"].reshape(-1)[0])
        q.put((rank, err_sum, tail_untouched, worst, dead_moved, abs(norm_hip - norm_ref) / norm_ref, digest, first_w, None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:      # surface worker failures in the parent's assertion message
        import traceback
        q.put((rank, None, None, None, None, None, None, None, traceback.format_exc() + repr(e)))


@pytest.mark.parametrize("ty", ["static", "Argo_both"])
def test_two_ranks_overlapped_exchange_and_adam(ty):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, ty, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in procs)
    for p in procs:
        p.join(60)
    for r in res:
        assert r[8] is None, f"rank {r[0]} failed:\n{r[8]}"
    for rank, err_sum, tail_ok, worst, dead_moved, norm_err, digest, first_w, _ in res:
        assert err_sum < 2e-5, f"rank {rank}: arena after the exchange differs from g0+g1 by {err_sum}"
        assert tail_ok, f"rank {rank}: the dead tail of the gradient arena was touched by the all-reduce"
        assert worst <= 1e-6, f"rank {rank}: parameters differ from clip+Adam on the mean gradient by {worst}"
        assert dead_moved == 0.0
        assert norm_err < 1e-5
    assert res[0][6] == res[1][6], "replicas diverged after one step"
    assert res[0][7] == res[1][7], "rank 0's parameters were not broadcast at wrap time"


def test_bench_two_rank_code_path_on_one_gpu():
    """bench.py's N>1 path (torch.distributed.run, one rank per process, barrier + max-over-ranks timing, the
    instrumented roofline step with the overlapped exchange) exercised with JP_DIST_BACKEND=gloo on a 1-GPU box."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, JP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", JP_BENCH_PREWARM="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "1", "--hw", "256", "--full", "--no-cpu-baseline", "--no-secondary"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 2 and j["scaling"] == "weak" and j["value"] > 0
    # (two processes time-slice one GPU here and the maps are 256x256: a kernel's HIP-event time can be mostly waiting for
    # the other rank, so the fraction may round to 0.0 -- only its range is checked on this smoke configuration)
    assert j["roofline"]["bound"] == "mfma" and 0 <= j["roofline"]["frac"] < 1 and j["roofline"]["launches"] >= 1
    assert any(k in j["roofline"]["kernel"] for k in ("jp_igemm", "jp_wgrad"))
    assert j["roofline"]["step_fp32_equiv_tflops"] > 0 and j["families"]


# ------------------------------------------------------------------------------------------- RCCL itself (1 rank)
def _rccl_worker(port, q):
    """One rank, backend "nccl" (= RCCL): a real step through `_Exchange.launch` / `finish` -- communicator creation,
    async work handles launched from the tape's streams, `work.wait()` as a stream dependency, allocator stream
    bookkeeping on the arena slices (gloo has none of these semantics)."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        torch.cuda.set_device(0)
        from jperceiver_amd import synthetic as syn
        from jperceiver_amd.model import MONO
        from jperceiver_amd.apis import batch_processor, build_optimizer, Runner, DataParallelShell, init_dist
        from jperceiver_amd.core import DistOptimizerHook
        from jperceiver_amd.core import dist_utils
        from oracle import jp_oracle as J
        init_dist("pytorch", backend="nccl")
        assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
        HW, B, FR = 256, 2, [0, -1, 1]
        opt = J.default_opt(frame_ids=FR, imgs_per_gpu=B, height=HW, width=HW, occ_map_size=HW // 4, type="static", split="odometry")
        d = syn.make_batch(B, HW, HW, FR, HW // 4, (94, 311), "odometry", seed=41)
        m = syn.make_dropout_masks(B, HW, HW, seed=41)
        d[("dropout_mask", 0)], d[("dropout_mask", 1)] = m
        for s, per in enumerate(syn.make_automask_noise(B, HW, HW, 4, 2, seed=41)):
            for j, nz in enumerate(per):
                d[("automask_noise", s, j)] = nz

        def fresh(force):
            model = MONO.module_dict["Baseline"](opt)
            model.load_state_dict(syn.synth_state_dict(model.state_dict(), seed=0))
            model = model.cuda().train()
            optim = build_optimizer(model, dict(type="Adam", lr=1e-4, weight_decay=0))
            shell = DataParallelShell(model)
            hook = DistOptimizerHook(grad_clip=dict(max_norm=35, norm_type=2), bucket_size_mb=4, force_exchange=force)
            return model, optim, Runner(shell, batch_processor, optim, hook)

        def sha(t):
            return hashlib.sha1(t.detach().cpu().numpy().tobytes()).hexdigest()

        # (a) two plain world-1 steps from identical weights: is the step itself bit-reproducible run to run?
        digests = []
        for _ in range(2):
            model, optim, runner = fresh(False)
            runner.train_iter({k: v.clone() for k, v in d.items()})
            torch.cuda.synchronize()
            digests.append((sha(optim.arena.grads), sha(optim.arena.params)))
            p_plain, g_plain = optim.arena.params.detach().cpu().clone(), optim.arena.grads.detach().cpu().clone()
        deterministic = digests[0] == digests[1]
        # (b) the same step with every bucket pushed through RCCL.  Each bucket is snapshotted on the launching stream
        # right before its all-reduce is enqueued: with one rank SUM is the identity, so after finish() the arena must
        # equal the snapshots BIT FOR BIT (a collective that ran before the producing kernels finished, or a wait that did
        # not order the norm / Adam kernels behind it, shows up here or in the parameter comparison below)
        model, optim, runner = fresh(True)
        snaps, launches = [], []
        orig_launch = dist_utils._Exchange.launch

        def spy(self, seg):
            if seg not in self.done and seg in self.arena.segments:
                off, n = self.arena.segments[seg]
                snaps.append((off, n, self.arena.grads[off:off + n].clone()))
                launches.append((seg, torch.cuda.current_stream().cuda_stream))
            return orig_launch(self, seg)
        dist_utils._Exchange.launch = spy
        try:
            runner.train_iter({k: v.clone() for k, v in d.items()})
        finally:
            dist_utils._Exchange.launch = orig_launch
        torch.cuda.synchronize()
        a = optim.arena
        ident = all(torch.equal(a.grads[o:o + n], t) for o, n, t in snaps)
        covered = sorted((o, n) for o, n, _ in snaps) == sorted(a.segments.values())
        g_x, p_x = a.grads.detach().cpu(), a.params.detach().cpu()
        same_as_plain = bool(torch.equal(g_x, g_plain) and torch.equal(p_x, p_plain))
        close_to_plain = float((p_x - p_plain).abs().max())
        # oracle clip+Adam on the exchanged arena (grad_scale = 1/1)
        p0 = syn.synth_state_dict(model.state_dict(), seed=0)
        P = {}
        for n, p, o, k in a.entries[:a.n_live_entries]:
            t = p0[n].clone().requires_grad_(True)
            t.grad = g_x[o:o + k].view(t.shape).clone()
            P[n] = t
        J.adam_step(P, {}, lr=1e-4, max_norm=35.0)
        worst = max(float((p.detach().cpu() - P[n].detach()).abs().max()) for n, p in model.named_parameters() if n in P)
        q.put(dict(ident=ident, covered=covered, deterministic=deterministic, same_as_plain=same_as_plain,
                   close_to_plain=close_to_plain, worst=worst, n_buckets=len(snaps), streams=len({s for _, s in launches}),
                   segs=[s for s, _ in launches], err=None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        import traceback
        q.put(dict(err=traceback.format_exc() + repr(e)))


def test_rccl_single_rank_exchange():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(port, q))
    p.start()
    r = q.get(timeout=900)
    p.join(60)
    assert r["err"] is None, r["err"]
    assert r["covered"] and r["n_buckets"] == 6, r          # every arena segment went through RCCL exactly once
    # launched from the tape as each segment's backward is ENQUEUED (the side stream's heads / layout encoder / pose nodes
    # are enqueued before the depth decoder's); the depth encoder's remainder is the last thing the backward finishes
    assert set(r["segs"]) == {"DepthDecoder", "heads", "LayoutEncoder", "Pose", "DepthEncoder.l4", "DepthEncoder.lo"}
    assert r["segs"][-1] == "DepthEncoder.lo" and r["streams"] >= 2, r
    assert r["ident"], "a bucket changed under a 1-rank SUM all-reduce: the collective raced its producer kernels"
    assert r["worst"] <= 1e-6, f"parameters after the RCCL step differ from clip+Adam on the exchanged arena by {r['worst']}"
    if r["deterministic"]:
        assert r["same_as_plain"], "the step through RCCL is not bit-identical to the plain world-1 step"
    else:   # atomics in a backward kernel: the step is not bit-reproducible run to run, compare at rounding level
        assert r["close_to_plain"] <= 2.5e-4, r             # lr-sized moves: |dp| <= ~2 lr for sign flips of ~0 gradients


def test_bench_self_launch_two_ranks():
    """`python bench.py --gpus 2` with NO rendezvous in the environment (the form of the driver's command): bench.py starts
    its own ranks under torch.distributed.run and rank 0 still prints exactly one JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(JP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", JP_BENCH_PREWARM="2")      # (the pre-warm loop on two ranks)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", "2",
           "--batch", "1", "--hw", "256", "--no-cpu-baseline", "--no-secondary", "--no-roofline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 2 and j["config"]["config_index"] == 2
    assert "cfg_kitti_baseline_kitti_odom_4gpus" in j["config"]["workload"] and "loss_sum 1" in j["config"]["workload"]


def test_bench_two_gpus_rccl():
    """`bench.py --gpus 2 --config 1` on backend nccl (= RCCL), one rank per GPU -- the form of the
    driver's scaling run.  Needs two devices: skipped (not failed) on the 1-GPU boxes of the build pool."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (RCCL with N > 1 ranks)")
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", JP_BENCH_PREWARM="0")
    env.pop("JP_DIST_BACKEND", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--config", "1",
           "--no-cpu-baseline", "--no-secondary", "--no-roofline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 16 and j["scaling"] == "weak"
    assert j["multi_gpu"]["backend"] == "nccl" and len(j["multi_gpu"]["ms_per_step_per_rank"]) == 2
    assert j["multi_gpu"]["allreduce_exposed_ms"] >= 0.0


class _SynthSet(torch.utils.data.Dataset):
    """4 synthetic odometry items in the layout `mono_dataset.__getitem__` returns (no batch axis)"""

    def __init__(self, hw, frames):
        import numpy as np
        self.hw, self.frames = hw, frames
        self.flag = np.zeros(4, dtype=np.int64)

    def __len__(self):
        return 4

    def __getitem__(self, i):
        from jperceiver_amd import synthetic as syn
        d = syn.make_batch(1, self.hw, self.hw, self.frames, self.hw // 4, (94, 311), "odometry", seed=70 + i)
        return {k: v[0] for k, v in d.items()}


def test_train_mono_two_epochs_single_rank(tmp_path):
    """`train_mono(model, dataset_train, dataset_val, cfg, args, distributed, validate, logger)`
    (mono/apis/trainer.py:59-73) end to end on the device: GroupSampler loader -> DeviceLoader -> the HIP step -> clip+Adam,
    step-LR, the epoch checkpoint; then `resume_from` continues where the file says."""
    from jperceiver_amd import synthetic as syn
    from jperceiver_amd.model import MONO
    from jperceiver_amd.apis import train_mono
    from oracle import jp_oracle as J
    HW, FR = 256, [0, -1, 1]
    opt = J.default_opt(frame_ids=FR, imgs_per_gpu=2, height=HW, width=HW, occ_map_size=HW // 4, type="static", split="odometry")

    class Cfg(dict):
        __getattr__ = dict.get
    cfg = Cfg(imgs_per_gpu=2, workers_per_gpu=0, gpus=[0], optimizer=dict(type="Adam", lr=1e-4, weight_decay=0),
              optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)), work_dir=str(tmp_path), total_epochs=2,
              lr_config=dict(policy="step", step=[1], gamma=0.5), checkpoint_config=dict(interval=2, save_optimizer=False),
              workflow=[("train", 1)], log_level="INFO")
    model = MONO.module_dict["Baseline"](opt)
    model.load_state_dict(syn.synth_state_dict(model.state_dict(), seed=0))
    w0 = model.DepthDecoder.iconv3.conv.weight.detach().clone()
    runner = train_mono(model, _SynthSet(HW, FR), None, cfg, None, distributed=False, validate=False)
    assert runner.epoch == 2 and runner.iter == 4 and runner.current_lr()[0] == pytest.approx(5e-5)
    lv = runner.outputs["log_vars"]
    assert all(v == v and abs(v) < 1e6 for v in lv.values()) and "loss" in lv        # (the boundary term makes the total negative)
    w1 = runner.model.module.DepthDecoder.iconv3.conv.weight.detach().cpu()
    moved = (w1 - w0).abs().max()
    assert 1e-5 < float(moved) < 1e-3                          # 2 steps at 1e-4 + 2 at 5e-5: |dw| <= 3e-4 per weight
    assert sorted(os.listdir(tmp_path)) == ["epoch_2.pth", "latest.pth"]          # mmcv's `latest.pth` link beside the epoch file
    m2 = MONO.module_dict["Baseline"](opt)
    r2 = train_mono(m2, _SynthSet(HW, FR), None, Cfg(cfg, resume_from=str(tmp_path / "epoch_2.pth"), total_epochs=2,
                                                     work_dir=str(tmp_path / "r")), None)
    assert r2.epoch == 2 and r2.iter == 4                      # nothing left to train; weights are the file's
    assert torch.equal(r2.model.module.DepthDecoder.iconv3.conv.weight.detach().cpu(), w1)
