"""Frozen inference on the full model (apis.freeze / Perceiver(frozen=True)) at 256^2, B = 2 -- the shape of the other eval-mode
tests (tests/test_inference_gpu.py, tests/test_perception_gpu.py), with their synthetic checkpoint whose BatchNorm running
statistics and affine maps are not the identity (synthetic.synth_state_dict(bn_stats=True)).

* parity: Perceiver(frozen=True) against Perceiver(frozen=False) on the same frames within the README's bars -- pose transform
  <= 1e-4, disparity and both layout heads' logits <= 1e-3 of each tensor's largest magnitude.  The BEV class map may differ
  only where the eager path's two logits are closer than that bar, and on fewer than 0.5 % of the pixels.  That this cap cannot
  hide a failure is checked on the CPU oracle (oracle.jp_oracle.forward, eval mode, the same weights and frames): at least
  99.5 % of the pixels of either head lie OUTSIDE the ambiguity band, so a route that got the layout wrong would flip far more
  pixels than the cap admits, and outside the band.
* launches, counted at ops.call: a frozen forward issues no jp_bn_eval_fwd (every BatchNorm of the model sits behind a
  convolution) and exactly one jp_add_relu per BasicBlock; the eager forward issues no jp_add_relu; unfreeze restores the eager
  pattern.
* staleness: a running_mean overwritten in place and a convolution weight replaced through load_state_dict after freezing are
  picked up by the next frozen forward (it matches a fresh eager forward and differs from the frozen output before the change).
* modes: a train-mode forward on a frozen model is bit-equal to a never-frozen model's (same seed and inputs, 256^2, B = 1:
  the step shape of tests/test_step_graph_gpu.py); the running statistics it rewrote reach the next frozen eval forward; freeze
  on a train-mode model raises."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops, synthetic as syn                                              # noqa: E402
from jperceiver_amd.apis import Perceiver, freeze, unfreeze, change_input_variable            # noqa: E402
from jperceiver_amd.model import MONO, modules as M                                           # noqa: E402
from oracle import jp_oracle as J                                                             # noqa: E402
from tests.test_inference_gpu import _model                                                   # noqa: E402
from tests.test_perception_gpu import _frames                                                 # noqa: E402

DEV = "cuda"
POSE_BAR, REL_BAR = 1e-4, 1e-3            # README parity paragraph
HEADS = ("topview", "topviewB")
N_BLOCKS = 8                              # BasicBlocks of one ResNet-18


def _heads(model, per, cur, prev):
    """everything the parity bars speak about, from one model: the Perceiver's outputs and the raw layout logits"""
    p = per.perceive(cur, prev)
    with torch.no_grad():
        out = model({("color_aug", 0, 0): cur})
    torch.cuda.synchronize()
    return dict(disp=p.disp.clone(), depth=p.depth.clone(), layout=p.layout.clone(), T=p.cam_T_cam.clone(),
                **{h: out[h].clone() for h in HEADS}, fwd_disp=out[("disp", 0, 0)].clone())


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _assert_parity(fz, eg, what):
    dT = float((fz["T"] - eg["T"]).abs().max())
    rel = {k: _rel(fz[k], eg[k]) for k in ("disp", "fwd_disp") + HEADS}
    share = float((fz["layout"] != eg["layout"]).float().mean())
    print(f"{what}: pose {dT:.3e}; " + ", ".join(f"{k} {v:.3e}" for k, v in rel.items()) + f"; class map differs on {share:.4%}")
    assert dT <= POSE_BAR, (what, dT)
    for k, v in rel.items():
        assert v <= REL_BAR, (what, k, v)
    assert torch.equal(fz["disp"], fz["fwd_disp"])
    # a class may flip only where the eager logits of a head are closer than the bar (relative to that head's largest logit)
    flips = torch.zeros_like(eg["layout"], dtype=torch.bool)
    for h in HEADS:
        e, f = eg[h], fz[h]
        band = (e[:, 1] - e[:, 0]).abs() < REL_BAR * e.abs().max()
        flip = (e[:, 1] > e[:, 0]) != (f[:, 1] > f[:, 0])
        assert not bool((flip & ~band).any()), (what, h, "a class flipped outside the ambiguity band")
        flips |= flip
    assert not bool(((fz["layout"] != eg["layout"]) & ~flips).any())
    assert share < 0.005, (what, share)
    return rel


@pytest.fixture(scope="module")
def pair():
    """(eager model, frozen model, frames): two copies of one checkpoint"""
    opt, eager = _model(HW=256, B=2)
    _, frozen = _model(HW=256, B=2)
    fr = _frames(3, 256, seed=33)
    return opt, eager, frozen, fr


def test_frozen_perceiver_matches_the_eager_one(pair):
    opt, eager, frozen, fr = pair
    # the CPU oracle on the same weights and frames: >= 99.5 % of the pixels of either head are outside the ambiguity band
    sd = {k: v.detach().cpu() for k, v in eager.state_dict().items()}
    P, Bf = J.make_params({k: tuple(v.shape) for k, v in sd.items()}, sd)
    with torch.no_grad():
        oo = J.forward(P, Bf, opt, {("color_aug", 0, 0): fr[1:3]}, training=False)
    for h in HEADS:
        lg = oo[h]
        clear = float(((lg[:, 1] - lg[:, 0]).abs() >= REL_BAR * lg.abs().max()).float().mean())
        print(f"oracle {h}: {clear:.4%} of the pixels outside the ambiguity band, classes {np.unique(lg.argmax(1).numpy()).tolist()}")
        assert clear >= 0.995, (h, clear)
    fr = fr.to(DEV)
    pe = Perceiver(eager)
    assert not M.is_frozen(eager)
    pf = Perceiver(frozen, frozen=True)
    assert M.is_frozen(frozen) and not M.is_frozen(eager)
    eg, fz = _heads(eager, pe, fr[1:3], fr[0:2]), _heads(frozen, pf, fr[1:3], fr[0:2])
    _assert_parity(fz, eg, "frozen vs eager")
    # and against the oracle itself, like the eager route (the README's bars are bars against the reference restatement)
    for h in HEADS:
        assert _rel(fz[h].cpu(), oo[h]) <= REL_BAR, h
    assert _rel(fz["disp"].cpu(), oo[("disp", 0, 0)]) <= REL_BAR
    # a second frozen pass gives the same bits: nothing is re-folded, nothing depends on the launch order
    fz2 = _heads(frozen, pf, fr[1:3], fr[0:2])
    for k in fz:
        assert torch.equal(fz[k], fz2[k]), k
    # the video entry point works on a frozen model as on any other
    ve, vf = pe.perceive_video(fr, batch=2), pf.perceive_video(fr, batch=2)
    assert float((ve.cam_T_cam - vf.cam_T_cam).abs().max()) <= POSE_BAR
    assert float(((ve.depth - vf.depth).abs() / ve.depth).max()) <= REL_BAR


def _count(monkeypatch, fn):
    calls = []
    real = ops.call
    with monkeypatch.context() as mp:
        mp.setattr(ops, "call", lambda n, *a: (calls.append(n), real(n, *a))[1])
        fn()
    # (jp_pack_replay is the pack registry's refresh: it fires in the pass after the set of packed layers of ANY model on the
    # device grew, frozen or not -- plumbing that is no part of a route's pattern)
    return [c for c in calls if c != "jp_pack_replay"]


def test_launch_pattern_of_the_frozen_route(pair, monkeypatch):
    opt, eager, frozen, fr = pair
    fr = fr.to(DEV)
    freeze(frozen)

    def run(model):
        def go():
            with torch.no_grad():
                model({("color_aug", 0, 0): fr[1:3]})
            model.predict_poses({("color_aug", 0, 0): fr[1:3], ("color_aug", -1, 0): fr[0:2]}, frame_ids=[0, -1])
        return go

    for _ in range(2):                                         # (packs and folds are made: the counted passes are steady-state ones)
        run(frozen)()
        run(eager)()
    ce, cf = _count(monkeypatch, run(eager)), _count(monkeypatch, run(frozen))
    n_bn = sum(isinstance(m, torch.nn.BatchNorm2d) for n, m in eager.named_modules()
               if n.split(".")[0] in ("DepthEncoder", "LayoutEncoder", "PoseEncoder", "LayoutDecoder", "LayoutTransformDecoder",
                                      "LayoutDecoderB", "LayoutTransformDecoderB"))
    print(f"launches per forward + pose pass: eager {len(ce)} (jp_bn_eval_fwd {ce.count('jp_bn_eval_fwd')}), "
          f"frozen {len(cf)} (jp_add_relu {cf.count('jp_add_relu')})")
    assert ce.count("jp_bn_eval_fwd") == n_bn == 100 and ce.count("jp_add_relu") == 0
    assert cf.count("jp_bn_eval_fwd") == 0 and cf.count("jp_bn_fold_conv") == 0
    assert cf.count("jp_add_relu") == 3 * N_BLOCKS               # depth, layout and pose encoder: one per BasicBlock
    assert len(cf) < len(ce) - n_bn + 3 * N_BLOCKS + 1           # and nothing else took the BatchNorm passes' place
    # unfreeze: the eager pattern again, call for call
    unfreeze(frozen)
    assert not M.is_frozen(frozen)
    assert _count(monkeypatch, run(frozen)) == ce
    freeze(frozen)                                               # (folds on attach)
    assert _count(monkeypatch, run(frozen)) == cf


def test_changed_weights_are_folded_again(pair):
    opt, eager, frozen, fr = pair
    fr = fr.to(DEV)
    pe, pf = Perceiver(eager), Perceiver(frozen, frozen=True)
    before = _heads(frozen, pf, fr[1:3], fr[0:2])
    snap = {k: v.detach().clone() for k, v in eager.state_dict().items()}
    try:
        for m in (eager, frozen):
            bn = m.LayoutDecoder.decoder[1]
            bn.running_mean.add_(0.5 * bn.running_var.sqrt())                       # in place
            bn2 = m.DepthEncoder.encoder.layer4[1].bn2
            bn2.running_mean.mul_(-1.0).sub_(0.25)
            conv = m.DepthEncoder.encoder.layer1[0].conv1
            conv.load_state_dict({"weight": conv.weight.detach().flip(0).clone() * 1.25})      # a sub-module's own load_state_dict
        after_f, after_e = _heads(frozen, pf, fr[1:3], fr[0:2]), _heads(eager, pe, fr[1:3], fr[0:2])
        _assert_parity(after_f, after_e, "after the change")
        moved = {k: _rel(after_f[k], before[k]) for k in ("disp", "topview")}
        print(f"frozen output moved by {moved} (relative) with the weights")
        assert moved["disp"] > 10 * REL_BAR and moved["topview"] > 10 * REL_BAR
    finally:
        for m in (eager, frozen):
            m.load_state_dict(snap)
    # Baseline.load_state_dict put everything back: the frozen model follows (the pack epoch moved)
    back = _heads(frozen, pf, fr[1:3], fr[0:2])
    for k in back:
        assert torch.equal(back[k], before[k]), k


def test_train_mode_ignores_the_frozen_state():
    HW, B, FR = 256, 1, [0, -1, 1]
    opt = J.default_opt(frame_ids=FR, imgs_per_gpu=B, height=HW, width=HW, occ_map_size=HW // 4, type="static", split="odometry",
                        loss_weightS=20, loss2_weightS=20)
    models = []
    for _ in range(2):
        m = MONO.module_dict["Baseline"](opt)
        m.load_state_dict(syn.synth_state_dict(m.state_dict(), seed=0, bn_stats=True))
        models.append(m.to(DEV))
    plain, frozen = models
    with pytest.raises(RuntimeError, match="eval-mode"):
        freeze(frozen)                                            # (a fresh module is in train mode)
    freeze(frozen.eval())
    x = _frames(1, HW, seed=5).to(DEV)
    with torch.no_grad():
        frozen({("color_aug", 0, 0): x})                          # folded and packed: the state is live when train mode starts
    batch = syn.make_batch(B, HW, HW, FR, HW // 4, (94, 311), "odometry", seed=81)
    res = []
    for m in (plain, frozen):
        m.train()
        ops.manual_seed(11)
        data = change_input_variable({k: v.clone() for k, v in batch.items()}, opt=opt)
        out, losses = m(data)
        torch.cuda.synchronize()
        res.append((out, losses._lv.vals.clone()))
    (o0, l0), (o1, l1) = res
    assert torch.equal(l0, l1), "loss terms differ between a frozen and a never-frozen model in train mode"
    assert o0.keys() == o1.keys()
    for k in o0:
        if torch.is_tensor(o0[k]):
            assert torch.equal(o0[k], o1[k]), k
    for (n0, b0), (n1, b1) in zip(plain.named_buffers(), frozen.named_buffers()):
        assert n0 == n1 and torch.equal(b0, b1), n0               # the running statistics took the same update
    # ... which the frozen state must see once the model is back in eval mode (kernels rewrote the buffers: no version bump)
    with torch.no_grad():
        oe, of = plain.eval()({("color_aug", 0, 0): x}), frozen.eval()({("color_aug", 0, 0): x})
    assert M.is_frozen(frozen) and not M.is_frozen(plain)
    for k in (("disp", 0, 0),) + HEADS:
        assert _rel(of[k], oe[k]) <= REL_BAR, k
