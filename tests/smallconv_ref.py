"""FLOAT64 reference of the direct small-channel convolutions (jperceiver_amd/csrc/conv_small.hip, conv_c16.hip), on the CPU, written
from the definition and not from the kernels:

    y = act(bias + Conv3x3(pad(cat_s(up2x?(x_s)))))        stride 1, pad 1, reflection or zero padding

The logical input is BUILT (logical_input): every half-resolution segment is repeated 2 x 2 (nearest), the segments are concatenated
along the channels, and the border is gathered by reflected indices or filled with zeros.  The convolution is the sum over the nine
taps of a channel contraction of the shifted input (correlate), in float64; the three gradients come from float64 autograd of that
graph.  Next to every result stands its TERM SUM  S = sum_k |a_k| |b_k|  (+ |bias| for the forward), from the same graph on absolute
values (tests/test_split_accuracy_gpu.py does the same for the engine): every error is |got - ref64| / S per element, maximised over
the tensor, so an element that is small because its terms cancel is still held to the size of its own terms, and a channel scaled by
2^-10 is not hidden behind one scaled by 2^10.

Activations.  The backward is a convolution backward of the pre-activation gradient g = dy act'(pre):
  sigmoid   the output is compared with sigmoid(pre64) against S / 4 (|sigmoid'| <= 1 / 4) and g = dy y64 (1 - y64);
  ReLU, leaky ReLU  the gate of the reference is pre64 > 0, except where |pre64| < (forward bar) S: there the evaluation under test
            decides (y > 0), and upstream() counts the elements it decided (`amb`) and the unambiguous gates that differ (`wrong`);
  bias      db = sum g, with S = sum |g|.

Two fp32 yardsticks, evaluated on the CPU and judged by the same metric (evaluate()):
  aten32    F.conv2d, the activation and autograd in float32 on the built input;
  chain32   ONE sequential chain per result element, acc = fl32(fl64(a) fl64(b) + fl64(acc)) (an fmaf: the product of two floats is
            exact in double), vectorised over the elements and looped over the terms -- forward: channel, then tap; input gradient:
            output channel, then tap, then the logical positions that read the stored element (2 x 2 of an upsampled one, the reflected
            twins); weight and bias gradient: image, then pixel in row-major order.  A kernel's wave and workgroup trees are shorter
            than a single chain, which is the least favourable order an fp32 evaluation can take.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3
SLOPE = 0.01

# srcs: ((channels, stored at half resolution?), ...); H, W: the logical (= output) size
Case = namedtuple("Case", "name family N srcs H W Cout reflect bias act scaled")
Inputs = namedtuple("Inputs", "xs w b dy")
Forward = namedtuple("Forward", "pre S")                      # float64: pre-activation, its term sum (with |bias|)
Backward = namedtuple("Backward", "dxs S_dxs dw S_dw db S_db")
Upstream = namedtuple("Upstream", "g amb wrong")


def cin(case):
    return sum(c for c, _ in case.srcs)


# --------------------------------------------------------------------------------------------------- the definition, any dtype
def upsample2x(t):
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3)


def reflect_index(n):
    """logical index read by the padded positions 0 .. n + 1 (nn.ReflectionPad2d(1): -1 -> 1, n -> n - 2)"""
    return torch.tensor([1] + list(range(n)) + [n - 2], dtype=torch.long)


def logical_input(xs, case):
    """(N, Cin, H + 2, W + 2): upsample, concatenate, pad"""
    cat = torch.cat([upsample2x(x) if up else x for x, (_, up) in zip(xs, case.srcs)], 1)
    assert tuple(cat.shape) == (case.N, cin(case), case.H, case.W)
    if case.reflect:
        return cat[:, :, reflect_index(case.H)][:, :, :, reflect_index(case.W)]
    out = cat.new_zeros(case.N, cin(case), case.H + 2, case.W + 2)
    out[:, :, 1:-1, 1:-1] = cat
    return out


def correlate(xp, w):
    """sum over the taps (ty, tx) and channels c of w[o, c, ty, tx] xp[n, c, y + ty, x + tx]"""
    H, W = xp.shape[2] - 2, xp.shape[3] - 2
    out = None
    for ty in range(3):
        for tx in range(3):
            t = torch.einsum("oc,nchw->nohw", w[:, :, ty, tx], xp[:, :, ty:ty + H, tx:tx + W])
            out = t if out is None else out + t
    return out


def activation(pre, act):
    if act == ACT_SIGMOID:
        return torch.sigmoid(pre)
    if act == ACT_RELU:
        return torch.where(pre > 0, pre, torch.zeros_like(pre))
    if act == ACT_LEAKY:
        return torch.where(pre > 0, pre, SLOPE * pre)
    return pre


# --------------------------------------------------------------------------------------------------- float64 reference
def forward(inp, case):
    with torch.no_grad():
        xs, w = [x.double() for x in inp.xs], inp.w.double()
        pre = correlate(logical_input(xs, case), w)
        S = correlate(logical_input([x.abs() for x in xs], case), w.abs())
        if inp.b is not None:
            pre = pre + inp.b.double().view(1, -1, 1, 1)
            S = S + inp.b.double().abs().view(1, -1, 1, 1)
    return Forward(pre, S)


def _grads(xs, w, g, case, want_dx):
    xs = [x.clone().requires_grad_(want_dx) for x in xs]
    w = w.clone().requires_grad_(True)
    correlate(logical_input(xs, case), w).backward(g)
    return [x.grad for x in xs], w.grad


def backward(inp, case, g, want_dx=True):
    """g: float64 gradient of the pre-activation -> the three gradients and their term sums"""
    xs, w = [x.double() for x in inp.xs], inp.w.double()
    dxs, dw = _grads(xs, w, g, case, want_dx)
    S_dxs, S_dw = _grads([x.abs() for x in xs], w.abs(), g.abs(), case, want_dx)
    return Backward(dxs, S_dxs, dw, S_dw, g.sum((0, 2, 3)), g.abs().sum((0, 2, 3)))


def ambiguous(fwd, case, fwd_bar):
    """elements whose ReLU gate an fp32 evaluation inside the forward bar may decide either way"""
    if case.act not in (ACT_RELU, ACT_LEAKY):
        return torch.zeros_like(fwd.pre, dtype=torch.bool)
    return fwd.pre.abs() < fwd_bar * fwd.S


def upstream(inp, case, fwd, y_got, fwd_bar):
    """gradient of the pre-activation for the reference backward; y_got decides the ambiguous gates"""
    dy = inp.dy.double()
    if case.act == ACT_SIGMOID:
        y = torch.sigmoid(fwd.pre)
        return Upstream(dy * y * (1 - y), 0, 0)
    if case.act == ACT_NONE:
        return Upstream(dy, 0, 0)
    amb, ref_gate, got_gate = ambiguous(fwd, case, fwd_bar), fwd.pre > 0, y_got > 0
    gate = torch.where(amb, got_gate, ref_gate)
    wrong = int((~amb & (got_gate != ref_gate)).sum())
    slope = 0.0 if case.act == ACT_RELU else SLOPE
    return Upstream(dy * torch.where(gate, 1.0, slope).double(), int(amb.sum()), wrong)


def worst(got, ref, S):
    """max |got - ref| / S; a sum with no term at all (S == 0: the taps of a one-row map that read only padding) must be exactly 0"""
    e = (got.double() - ref).abs()
    inf = torch.full_like(e, float("inf"))
    return float(torch.where(S > 0, e / S.clamp_min(1e-300), torch.where(e > 0, inf, torch.zeros_like(e))).max())


def forward_error(case, fwd, y_got):
    if case.act == ACT_SIGMOID:
        return worst(y_got, torch.sigmoid(fwd.pre), fwd.S / 4)
    return worst(y_got, activation(fwd.pre, case.act), fwd.S)


def evaluate(inp, case, fwd, got, fwd_bar):
    """got: dict(y, dxs, dw, db) of an fp32 evaluation (a yardstick or the device) -> ({quantity: error}, Upstream)"""
    up = upstream(inp, case, fwd, got["y"], fwd_bar)
    bwd = backward(inp, case, up.g)
    figs = {"fwd": forward_error(case, fwd, got["y"]),
            "dx": max(worst(d, r, s) for d, r, s in zip(got["dxs"], bwd.dxs, bwd.S_dxs)),
            "dw": worst(got["dw"], bwd.dw, bwd.S_dw)}
    if inp.b is not None:
        figs["db"] = worst(got["db"], bwd.db, bwd.S_db)
    return figs, up


# --------------------------------------------------------------------------------------------------- yardstick 1: ATen float32
def aten32(inp, case):
    """on ONE thread: how ATen splits a sum over its threads must not move the committed figures from machine to machine"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        xs = [x.clone().requires_grad_(True) for x in inp.xs]
        w = inp.w.clone().requires_grad_(True)
        b = inp.b.clone().requires_grad_(True) if inp.b is not None else None
        pre = F.conv2d(logical_input(xs, case), w, b)
        y = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_LEAKY: lambda t: F.leaky_relu(t, SLOPE), ACT_SIGMOID: torch.sigmoid}[case.act](pre)
        y.backward(inp.dy)
    finally:
        torch.set_num_threads(threads)
    return dict(y=y.detach(), dxs=[x.grad for x in xs], dw=w.grad, db=b.grad if b is not None else None)


# --------------------------------------------------------------------------------------------------- yardstick 2: one fp32 chain
def _fma(a64, b64, acc32):
    return (a64 * b64 + acc32.double()).float()


def _chain_forward(inp, case):
    xp = logical_input(inp.xs, case)
    w = inp.w.double()
    acc = torch.zeros(case.N, case.Cout, case.H, case.W)
    for c in range(cin(case)):
        for t in range(9):
            ty, tx = divmod(t, 3)
            acc = _fma(w[:, c, ty, tx].view(1, -1, 1, 1), xp[:, c:c + 1, ty:ty + case.H, tx:tx + case.W].double(), acc)
    if inp.b is not None:
        acc = (acc.double() + inp.b.double().view(1, -1, 1, 1)).float()
    return acc


def _readers(case, up):
    """the padded logical positions that read each stored element of a segment, by rank: [(padded flat index, stored flat index)...]"""
    def line(n):
        src = reflect_index(n).numpy() if case.reflect else np.array([-1] + list(range(n)) + [-1])
        return np.where(src >= 0, src >> up, -1)
    rows, cols = line(case.H), line(case.W)
    ws = case.W >> up
    stored = np.where((rows[:, None] >= 0) & (cols[None, :] >= 0), rows[:, None] * ws + cols[None, :], -1).reshape(-1)
    padded = np.nonzero(stored >= 0)[0]
    stored = stored[padded]
    order = np.argsort(stored, kind="stable")
    padded, stored = padded[order], stored[order]
    rank = np.arange(len(stored)) - np.searchsorted(stored, stored, side="left")
    return [(padded[rank == r], stored[rank == r]) for r in range(int(rank.max()) + 1)]


def _chain_dgrad(inp, case, g):
    """g: float32 gradient of the pre-activation"""
    N, H, W = case.N, case.H, case.W
    gflat = g.double().reshape(N, case.Cout, H * W)
    w = inp.w.double()
    out, c0 = [], 0
    for (C, up), x in zip(case.srcs, inp.xs):
        acc = torch.zeros(N, C, x.shape[2] * x.shape[3])
        plan = []
        for t in range(9):
            ty, tx = divmod(t, 3)
            for padded, stored in _readers(case, up):
                oy, ox = padded // (W + 2) - ty, padded % (W + 2) - tx
                ok = (oy >= 0) & (oy < H) & (ox >= 0) & (ox < W)
                if ok.any():
                    plan.append((t, torch.from_numpy((oy * W + ox)[ok]), torch.from_numpy(stored[ok])))
        for co in range(case.Cout):
            for t, pix, stored in plan:
                acc[:, :, stored] = _fma(gflat[:, co, pix].unsqueeze(1), w[co, c0:c0 + C, t // 3, t % 3].view(1, -1, 1), acc[:, :, stored])
        out.append(acc.view_as(x))
        c0 += C
    return out


def _chain_wgrad(inp, case, g):
    """-> dw (Cout, Cin, 3, 3), db (Cout): image, then pixel in row-major order; the bias rides along as a column of ones"""
    N, H, W, Ci = case.N, case.H, case.W, cin(case)
    xp = logical_input(inp.xs, case).numpy()
    g64 = g.double().numpy().reshape(N, case.Cout, H * W)
    acc32 = np.zeros((case.Cout, Ci * 9 + 1), np.float32)
    acc64, buf = np.zeros_like(acc32, dtype=np.float64), np.zeros_like(acc32, dtype=np.float64)
    for n in range(N):
        cols = np.ones((H * W, Ci * 9 + 1))
        for t in range(9):
            ty, tx = divmod(t, 3)
            cols[:, t:Ci * 9:9] = xp[n, :, ty:ty + H, tx:tx + W].reshape(Ci, H * W).T
        gn = np.ascontiguousarray(g64[n].T)[:, :, None]           # (HW, Cout, 1)
        cols = cols[:, None, :]
        for p in range(H * W):
            np.multiply(gn[p], cols[p], out=buf)
            np.add(buf, acc64, out=buf)
            acc32[...] = buf
            acc64[...] = acc32
    dw = torch.from_numpy(acc32[:, :Ci * 9].reshape(case.Cout, Ci, 3, 3).copy())
    return dw, torch.from_numpy(acc32[:, -1].copy())


def chain32(inp, case):
    pre = _chain_forward(inp, case)
    y = activation(pre, case.act)
    if case.act == ACT_SIGMOID:
        g = inp.dy * y * (1 - y)
    elif case.act in (ACT_RELU, ACT_LEAKY):
        g = inp.dy * torch.where(y > 0, 1.0, 0.0 if case.act == ACT_RELU else SLOPE)
    else:
        g = inp.dy
    dw, db = _chain_wgrad(inp, case, g)
    return dict(y=y, dxs=_chain_dgrad(inp, case, g), dw=dw, db=db if inp.b is not None else None)


# --------------------------------------------------------------------------------------------------- independent gather evaluation
def gather_forward(xs, w, case):
    """The same convolution WITHOUT building the logical input: every tap gathers the stored element by index arithmetic
    ((reflected or masked logical index) >> up), float64, differentiable (the backward of an index gather is the transposed gather)."""
    def line(n, t):
        i = torch.arange(n) - 1 + t
        if case.reflect:
            i = torch.where(i < 0, -i, torch.where(i >= n, 2 * n - 2 - i, i))
            return i, torch.ones(n, dtype=torch.bool)
        ok = (i >= 0) & (i < n)
        return i.clamp(0, n - 1), ok
    out, c0 = 0, 0
    for (C, up), x in zip(case.srcs, xs):
        for ty in range(3):
            iy, oky = line(case.H, ty)
            for tx in range(3):
                ix, okx = line(case.W, tx)
                v = x[:, :, iy >> up][:, :, :, ix >> up] * (oky[:, None] & okx[None, :]).to(x.dtype)
                out = out + torch.einsum("oc,nchw->nohw", w[:, c0:c0 + C, ty, tx], v)
        c0 += C
    return out


def up_head_gather_forward(x, w, case):
    """Disparity head by parity classes: output pixel (2i + a, 2j + b) reads the edge-clamped 2 x 2 patch rows i - 1 + a + r, columns
    j - 1 + b + s of the half-resolution x with the 16 (class, slot) sums of the taps: rows {0}, {1, 2} for a = 0 and {0, 1}, {2}
    for a = 1 (the reflection of the upsampled map is an edge clamp of the stored one)."""
    taps = {(0, 0): [0], (0, 1): [1, 2], (1, 0): [0, 1], (1, 1): [2]}
    N, C, h, wd = x.shape
    y = x.new_zeros(N, 1, 2 * h, 2 * wd)
    for a in range(2):
        for b in range(2):
            acc = 0
            for r in range(2):
                rows = (torch.arange(h) - 1 + a + r).clamp(0, h - 1)
                for s in range(2):
                    cols = (torch.arange(wd) - 1 + b + s).clamp(0, wd - 1)
                    wq = sum(w[0, :, ty, tx] for ty in taps[(a, r)] for tx in taps[(b, s)])
                    acc = acc + torch.einsum("c,nchw->nhw", wq, x[:, :, rows][:, :, :, cols])
            y[:, 0, a::2, b::2] = acc
    return y
