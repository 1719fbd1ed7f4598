"""The streaming perception session (apis.PerceptionStream) at 256^2 on the synthetic checkpoint of the other eval-mode tests
(tests/test_inference_gpu._model), five uint8 frames of 94 x 311 per camera cut from tests/test_perception_gpu._frames
patterns, cameras 1 and 2.  The module shares one model, the frames and the reference chain; every test builds a session of its
own, so a failure points at the session and not at what an earlier test did to it.

* precondition (asserted): two eager Perceiver(frozen=True).perceive passes on the same pair give the same bits at this shape,
  for one camera and for two -- every bit-equality below rests on it.
* the session gives, for every frame k, the bits of DevicePreprocessor.resize_u8 followed by perceive(frame_k, frame_{k-1}):
  disp, depth, layout and cam_T_cam (None for frame 0); its trajectory equals the explicit-order float64 chain of those
  cam_T_cam bit for bit (tests/test_stream_kernels_gpu.chain_step) and the `T_{k-1} @ cam_T_cam_k` chaining of perceive_video
  within 1e-12 (the bound derived in tests/test_stream_kernels_gpu.py).  With one camera that is
  Perceiver.perceive_video(batch=1) itself; with two cameras the pose nets of the session run at batch 2, which perceive_video
  cannot be asked to do for a temporal sequence, so there its chaining (numpy @ from the identity) is applied to the reference
  cam_T_cam.
* launches of a steady-state push, counted at ops.call: the two new entry points once each, no jp_bn_eval_fwd (frozen), no
  Softmax2d map and no jp_bilinear_fwd, where the resize_u8 + perceive(cur, prev) it replaces issues four and two.
* a second session on the same model, used in between, does not disturb the first.
* reset(): pushing the same frames again reproduces the first run's bits.
* static buffers: the tensors returned for frame k+1 are the storage returned for frame k, overwritten.
* changed weights: after an in-place edit of BatchNorm running means and a load_state_dict on one convolution (the edits of
  tests/test_frozen_model_gpu.py::test_changed_weights_are_folded_again) the next push matches a fresh eager perceive on the
  changed model, differs from the pre-change output of the same frames by more than 10 x the README bar, and the trajectory
  continues from the pose it had."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd.apis import Perceiver, PerceptionStream                        # noqa: E402
from jperceiver_amd.datasets.preprocess import DevicePreprocessor                  # noqa: E402
from tests.test_frozen_model_gpu import _count                                     # noqa: E402
from tests.test_inference_gpu import _model                                        # noqa: E402
from tests.test_perception_gpu import _frames                                      # noqa: E402
from tests.test_stream_kernels_gpu import chain_step                               # noqa: E402

DEV = "cuda"
HW, SRC, NF = 256, (94, 311), 5
REL_BAR = 1e-3                              # README parity paragraph
FIELDS = ("disp", "depth", "layout", "cam_T_cam")


def _u8_frames(cams):
    """(NF, cams, 94, 311, 3) uint8 on the device: frame k of camera c is pattern k * cams + c"""
    f = _frames(NF * cams, SRC[1], seed=41 + cams)[:, :, :SRC[0], :]                # (n,3,94,311) in [0,1]
    return (f * 255).round().to(torch.uint8).permute(0, 2, 3, 1).reshape(NF, cams, SRC[0], SRC[1], 3).contiguous().to(DEV)


def _clone(fr):
    out = {k: (None if getattr(fr, k) is None else getattr(fr, k).clone()) for k in FIELDS + ("pose",) if hasattr(fr, k)}
    out["index"] = getattr(fr, "index", None)
    return out


def _run(s, frames):
    out = [_clone(s.push(frames[k])) for k in range(frames.shape[0])]
    torch.cuda.synchronize()
    return out


def _assert_same(a, b, what):
    for k in FIELDS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert torch.equal(a[k], b[k]), (what, k, float((a[k].float() - b[k].float()).abs().max()))


class _World:
    """what the tests share and leave unchanged: one model, the frames, the reference chain per camera count"""

    def __init__(self):
        self.opt, self.model = _model(HW=HW, B=2)
        self.per = Perceiver(self.model, frozen=True)
        self.pre = DevicePreprocessor(HW, HW, torch.device(DEV))
        self.frames = {c: _u8_frames(c) for c in (1, 2)}
        self.ref, self.repeat_equal = {}, {}
        for c in (1, 2):
            self.ref[c], self.repeat_equal[c] = self.reference(c)

    def resized(self, c, k):
        return self.pre.resize_u8(self.frames[c][k], HW, HW)

    def perceive(self, c, k):
        p = self.per.perceive(self.resized(c, k), self.resized(c, k - 1) if k > 0 else None)
        return _clone(p)

    def reference(self, c):
        ref = [self.perceive(c, k) for k in range(NF)]
        again = self.perceive(c, 2)
        torch.cuda.synchronize()
        return ref, all(torch.equal(ref[2][k], again[k]) for k in FIELDS)

    def session(self, c):
        return PerceptionStream(self.model, SRC, cameras=c)


@pytest.fixture(scope="module")
def world():
    return _World()


@pytest.mark.parametrize("cams", [1, 2])
def test_precondition_two_eager_passes_give_the_same_bits(world, cams):
    assert world.repeat_equal[cams]


@pytest.mark.parametrize("cams", [1, 2])
def test_session_equals_the_reference_chain(world, cams):
    ref = world.ref[cams]
    s = world.session(cams)
    got = _run(s, world.frames[cams])
    assert [g["index"] for g in got] == list(range(NF))
    assert got[0]["cam_T_cam"] is None and ref[0]["cam_T_cam"] is None
    for k in range(NF):
        _assert_same(got[k], ref[k], f"frame {k}")
    # the trajectory: the explicit-order chain of the reference transforms, bit for bit
    P = np.tile(np.identity(4), (cams, 1, 1))
    plain = P.copy()
    rows = [P[:, :3].reshape(cams, 12).copy()]
    assert np.array_equal(got[0]["pose"].cpu().numpy(), P)
    for k in range(1, NF):
        T = ref[k]["cam_T_cam"].cpu().numpy()
        P = chain_step(P, T)
        plain = plain @ T.astype(np.float64)                    # perceive_video's chaining
        rows.append(P[:, :3].reshape(cams, 12).copy())
        assert np.array_equal(got[k]["pose"].cpu().numpy(), P), k
    traj = s.trajectory().cpu().numpy()
    assert traj.shape == (cams, NF, 12) and traj.dtype == np.float64
    assert np.array_equal(traj, np.stack(rows, 1))
    d = float(np.abs(P - plain).max())
    print(f"{cams} camera(s): explicit-order chain vs numpy @ over {NF} frames: {d:.3e}")
    assert d <= 1e-12
    if cams == 1:
        seq = torch.cat([world.resized(1, k) for k in range(NF)])
        v = world.per.perceive_video(seq, batch=1)
        assert torch.equal(v.cam_T_cam, torch.cat([ref[k]["cam_T_cam"] for k in range(1, NF)]))
        dv = float(np.abs(v.trajectory[:, :3].reshape(NF, 12) - traj[0]).max())
        print(f"session trajectory vs perceive_video's: {dv:.3e}")
        assert dv <= 1e-12


def test_launches_of_a_steady_state_push(world, monkeypatch):
    fr = world.frames[2]
    s = world.session(2)
    s.push(fr[0])
    s.push(fr[1])
    cs = _count(monkeypatch, lambda: s.push(fr[2]))
    cur, prev = world.resized(2, 2), world.resized(2, 1)
    ce = _count(monkeypatch, lambda: (world.pre.resize_u8(fr[2], HW, HW), world.per.perceive(cur, prev)))
    print(f"launches per frame: session {len(cs)}, resize_u8 + perceive(cur, prev) {len(ce)}")
    assert cs.count("jp_stream_pose_pair") == 1 and cs.count("jp_stream_traj_push") == 1
    assert cs.count("jp_bn_eval_fwd") == 0 and cs.count("jp_bn_fold_conv") == 0 and cs.count("jp_softmax_c2") == 0
    assert ce.count("jp_bilinear_fwd") == 2 and cs.count("jp_bilinear_fwd") == 0
    assert ce.count("jp_softmax_c2") == 4
    torch.cuda.synchronize()


def test_two_sessions_on_one_model_do_not_disturb_each_other(world):
    a, b = world.session(2), world.session(2)
    fr, ref = world.frames[2], world.ref[2]
    for k in range(NF):
        ga = _clone(a.push(fr[k]))
        gb = _clone(b.push(fr[NF - 1 - k]))                       # the other session sees the frames in reverse
        _assert_same(ga, ref[k], f"frame {k}")
        assert gb["index"] == k
    r = world.session(2)
    rev = _run(r, fr.flip(0))
    assert torch.equal(gb["cam_T_cam"], rev[NF - 1]["cam_T_cam"]) and torch.equal(gb["pose"], rev[NF - 1]["pose"])
    assert torch.equal(b.trajectory(), r.trajectory())


def test_reset_reproduces_the_first_run(world):
    s = world.session(2)
    first = _run(s, world.frames[2])
    t1 = s.trajectory()
    s.reset()
    assert s.trajectory().shape == (2, 0, 12)
    second = _run(s, world.frames[2])
    for k in range(NF):
        assert second[k]["index"] == k
        _assert_same(second[k], first[k], f"frame {k}")
        assert torch.equal(second[k]["pose"], first[k]["pose"])
    assert torch.equal(s.trajectory(), t1)


def test_outputs_are_static_buffers_overwritten_by_the_next_push(world):
    s = world.session(2)
    fr = world.frames[2]
    s.push(fr[0])
    a = s.push(fr[1])
    kept = _clone(a)
    b = s.push(fr[2])
    torch.cuda.synchronize()
    assert (a.index, b.index) == (1, 2)
    for k in FIELDS + ("pose",):
        ta, tb = getattr(a, k), getattr(b, k)
        assert ta.data_ptr() == tb.data_ptr() and ta.untyped_storage().data_ptr() == tb.untyped_storage().data_ptr(), k
        assert torch.equal(ta, tb), k                               # frame 1's tensors now hold frame 2's results
    assert not torch.equal(kept["disp"], b.disp) and not torch.equal(kept["cam_T_cam"], b.cam_T_cam)
    _assert_same(kept, world.ref[2][1], "frame 1")
    _assert_same(_clone(b), world.ref[2][2], "frame 2")


def test_changed_weights_reach_the_next_push(world):
    m, fr = world.model, world.frames[2]
    s = world.session(2)
    for k in range(3):
        s.push(fr[k])
    pose2, traj2 = s._pose.clone().view(-1, 4, 4), s.trajectory()
    snap = {k: v.detach().clone() for k, v in m.state_dict().items()}
    try:
        bn = m.LayoutDecoder.decoder[1]
        bn.running_mean.add_(0.5 * bn.running_var.sqrt())                       # in place
        bn2 = m.DepthEncoder.encoder.layer4[1].bn2
        bn2.running_mean.mul_(-1.0).sub_(0.25)
        conv = m.DepthEncoder.encoder.layer1[0].conv1
        conv.load_state_dict({"weight": conv.weight.detach().flip(0).clone() * 1.25})      # a sub-module's own load_state_dict
        got = _clone(s.push(fr[3]))
        s.push(fr[4])
        traj = s.trajectory()
        fresh = world.perceive(2, 3)                                            # eager, on the changed model
        torch.cuda.synchronize()
        _assert_same(got, fresh, "after the change")
        before = world.ref[2][3]
        moved = float((got["disp"] - before["disp"]).abs().max() / before["disp"].abs().max())
        flipped = float((got["layout"] != before["layout"]).float().mean())
        print(f"disp moved by {moved:.3e} (relative) with the weights, {flipped:.2%} of the class map changed")
        assert moved > 10 * REL_BAR
        # the trajectory goes on from the pose it had
        want = chain_step(pose2.cpu().numpy(), got["cam_T_cam"].cpu().numpy())
        assert np.array_equal(got["pose"].cpu().numpy(), want)
        assert torch.equal(traj[:, :3], traj2) and traj.shape[1] == 5
    finally:
        m.load_state_dict(snap)
    # everything is back: a new session gives the reference bits again
    back = _run(world.session(2), fr[:2])
    _assert_same(back[1], world.ref[2][1], "restored")
