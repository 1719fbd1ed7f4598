"""The two per-frame kernels of the streaming session (csrc/stream.hip) against what they replace.

jp_stream_pose_pair, B = 2, frames of 3 x 40 x 56 (upscaling, odd sizes) and 3 x 256 x 256 (the session's shape in the tests;
both run more than one workgroup and the grid-stride loop more than once), three consecutive pushes with a hand-advanced
counter: `pair` is bit-equal to cat([bilinear_resize(prev), bilinear_resize(cur)]) of ops.bilinear_resize (jp_bilinear_fwd),
the first push pairs the frame with itself, the ring slot of parity n & 1 is the one written (the other keeps its bits), the
magnitude slot holds pair.abs().max(), and the counter is left alone.

jp_stream_traj_push, B = 2, capacity = 4, 6 pushes of seeded transforms (rotation < 0.1 rad, |t| <= 1): pose and trajectory are
bit-equal to a numpy float64 chain written with the kernel's explicit sum order ((a0 b0 + a1 b1) + a2 b2) + a3 b3; rows beyond
the capacity are not written (the trajectory buffer sits inside a guarded allocation) while pose and count go on; count == 0
yields the identity whatever T holds (it holds NaN here); and against plain `numpy @` the difference is <= 1e-12 absolute --
4-term float64 dot products with sum |a||b| <= 11 give at most 5e-15 per step, and 6 steps with bounded amplification (the
factors are rigid motions) stay below 1e-12.  B = 18 runs the kernel's second pass over the cameras (16 per pass)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                     # noqa: E402
from jperceiver_amd.ops import Var                 # noqa: E402

DEV = "cuda"
PH, PW = 192, 640


def chain_step(P, T):
    """P (B,4,4) float64 poses, T (B,4,4) float32 transforms -> P @ double(T), every element ((a0 b0 + a1 b1) + a2 b2) + a3 b3
    with each numpy operation rounding once: the order of jp_stream_traj_push."""
    P, T = np.asarray(P, dtype=np.float64), np.asarray(T, dtype=np.float32).astype(np.float64)
    a, b = P[:, :, None, :], np.swapaxes(T, 1, 2)[:, None, :, :]          # a[b,i,1,k], b[b,1,j,k] = T[b,k,j]
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def seeded_transforms(n, B, seed):
    """(n,B,4,4) float32 rigid motions: rotation angle < 0.1 rad about a random axis, |t_i| <= 1."""
    rng = np.random.default_rng(seed)
    out = np.tile(np.identity(4), (n, B, 1, 1))
    for k in range(n):
        for b in range(B):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            th = rng.uniform(0.01, 0.1)
            Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            out[k, b, :3, :3] = np.identity(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
            out[k, b, :3, 3] = rng.uniform(-1, 1, 3)
    return out.astype(np.float32)


@pytest.mark.parametrize("hw", [(40, 56), (256, 256)])
def test_pose_pair_is_the_bilinear_resize_of_the_frame_and_its_predecessor(hw):
    B, (H, W) = 2, hw
    g = torch.Generator().manual_seed(7 + H)
    frames = (torch.rand(3, B, 3, H, W, generator=g) * 2 - 0.5).to(DEV)          # (negative values too: the magnitude is of |pair|)
    ring = torch.full((2, B, 3, PH, PW), -3.0, device=DEV)
    count = torch.zeros(1, device=DEV, dtype=torch.int32)
    prev = None
    for n in range(3):
        count.fill_(n)                                                            # hand-advanced: the kernel only reads it
        pair = torch.full((B, 6, PH, PW), -5.0, device=DEV)
        slot = torch.zeros(ops._slot_floats(), device=DEV)
        before = ring.clone()
        ops.call("jp_stream_pose_pair", frames[n], ring, count, pair, slot, B, H, W)
        cur = ops.bilinear_resize(Var(frames[n]), PH, PW).t
        want = torch.cat([cur if n == 0 else prev, cur], 1)
        assert torch.equal(pair, want), n
        if n == 0:
            assert torch.equal(pair[:, 0:3], pair[:, 3:6])                        # the first frame is paired with itself
        assert torch.equal(ring[n & 1], cur), n
        assert torch.equal(ring[(n & 1) ^ 1], before[(n & 1) ^ 1]), n             # the other slot keeps its bits
        assert float(slot.max()) == float(pair.abs().max()), n
        assert int(count.item()) == n
        prev = cur
    # no magnitude slot: the same pair
    pair2 = torch.empty_like(pair)
    ops.call("jp_stream_pose_pair", frames[2], ring, count, pair2, None, B, H, W)
    assert torch.equal(pair2, pair)


def _guarded_traj(B, cap):
    """a (B,cap,12) trajectory in the middle of a larger allocation filled with a sentinel"""
    G = 64
    store = torch.full((G + B * cap * 12 + G,), -7.0, device=DEV, dtype=torch.float64)
    return store, store[G:G + B * cap * 12].view(B, cap, 12), G


def test_traj_push_chains_in_float64_with_the_documented_sum_order():
    B, cap, N = 2, 4, 6
    Ts = seeded_transforms(N, B, seed=11)
    Ts[0] = np.nan                                                                # count == 0: T is not read
    store, traj, G = _guarded_traj(B, cap)
    pose = torch.full((B, 16), 9.0, device=DEV, dtype=torch.float64)
    count = torch.zeros(1, device=DEV, dtype=torch.int32)
    ref = np.tile(np.identity(4), (B, 1, 1))
    plain = ref.copy()
    rows = []
    for k in range(N):
        ops.call("jp_stream_traj_push", torch.from_numpy(Ts[k]).to(DEV), pose, traj, count, B, cap)
        if k > 0:
            ref = chain_step(ref, Ts[k])
            plain = plain @ Ts[k].astype(np.float64)
        rows.append(ref[:, :3, :].reshape(B, 12).copy())
        assert int(count.item()) == k + 1
        got = pose.cpu().numpy().reshape(B, 4, 4)
        assert np.array_equal(got, ref), k                                         # bit for bit, beyond the capacity too
        if k == 0:
            assert np.array_equal(got, np.tile(np.identity(4), (B, 1, 1)))
    want = np.stack(rows[:cap], 1)                                                 # (B,cap,12): frames 0..cap-1 only
    assert np.array_equal(traj.cpu().numpy(), want)
    s = store.cpu().numpy()
    assert np.all(s[:G] == -7.0) and np.all(s[G + B * cap * 12:] == -7.0)          # nothing outside the trajectory was written
    d = float(np.abs(pose.cpu().numpy().reshape(B, 4, 4) - plain).max())
    print(f"explicit-order chain vs numpy @ after {N} pushes: {d:.3e}")
    assert d <= 1e-12


def test_traj_push_walks_more_cameras_than_one_pass_holds():
    B, cap = 18, 3
    Ts = seeded_transforms(3, B, seed=12)
    store, traj, G = _guarded_traj(B, cap)
    pose = torch.zeros((B, 16), device=DEV, dtype=torch.float64)
    count = torch.zeros(1, device=DEV, dtype=torch.int32)
    ref = np.tile(np.identity(4), (B, 1, 1))
    rows = []
    for k in range(3):
        ops.call("jp_stream_traj_push", torch.from_numpy(Ts[k]).to(DEV), pose, traj, count, B, cap)
        if k > 0:
            ref = chain_step(ref, Ts[k])
        rows.append(ref[:, :3, :].reshape(B, 12).copy())
    assert int(count.item()) == 3
    assert np.array_equal(pose.cpu().numpy().reshape(B, 4, 4), ref)
    assert np.array_equal(traj.cpu().numpy(), np.stack(rows, 1))
    s = store.cpu().numpy()
    assert np.all(s[:G] == -7.0) and np.all(s[G + B * cap * 12:] == -7.0)
