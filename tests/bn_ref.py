"""Float64 references of the BatchNorm kernels (test infrastructure, not part of the product).

Plain torch restatements of what jperceiver_amd/csrc/bn.hip computes, written from the formulas of train-mode BatchNorm2d and not by
calling F.batch_norm: two-pass variance, biased for the normalisation and unbiased (n / (n - 1)) into running_var, the momentum
update applied n_updates times, the optional residual add and ReLU, the fused ReLU + MaxPool2d(3, 2, 1) of the ResNet stem tail with
the first maximum in row-major window order, eval mode, and the per-channel sum.  Every function works in the dtype of its inputs on
the CPU; fed float64 it is the referee of tests/test_bn_f64_gpu.py.  tests/test_bn_ref_cpu.py holds it to F.batch_norm,
F.max_pool2d(return_indices=True) and float64 autograd.

The backward functions take the ReLU gate (and the pooled argmax byte) as ARGUMENTS: the caller decides which decisions are the
reference's own and which are ambiguous in fp32 (tests/bn_cases.py).
"""
from collections import namedtuple

import torch

BnFwd = namedtuple("BnFwd", "y mean var invstd rm rv pre terms")
BnBwd = namedtuple("BnBwd", "dx dres dgamma dbeta abs_dgamma abs_dbeta")
PoolFwd = namedtuple("PoolFwd", "pooled idx bn cand")


def _c(v):
    return v.view(1, -1, 1, 1)


def momentum_update(r, new, momentum, n_updates):
    for _ in range(n_updates):
        r = (1 - momentum) * r + momentum * new
    return r


def bn_train_fwd(x, gamma, beta, residual=None, relu=False, eps=1e-5, momentum=0.1, n_updates=1, rm=None, rv=None):
    """x (N, C, H, W).  -> y, batch mean, biased variance, invstd, the running statistics after n_updates momentum updates (None
    without running statistics), the pre-activation (before the ReLU) and `terms` = |x sc| + |sh| + |residual| with
    sc = invstd gamma, sh = beta - mean sc: the magnitudes an fp32 evaluation of the pre-activation combines"""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.sum((0, 2, 3)) / n
    var = ((x - _c(mean)) ** 2).sum((0, 2, 3)) / n
    invstd = 1 / torch.sqrt(var + eps)
    sc = invstd * gamma
    sh = beta - mean * sc
    pre = (x - _c(mean)) * _c(sc) + _c(beta)
    terms = (x * _c(sc)).abs() + _c(sh).abs()
    if residual is not None:
        pre = pre + residual
        terms = terms + residual.abs()
    y = torch.clamp(pre, min=0) if relu else pre
    unbiased = var * n / (n - 1) if n > 1 else var
    rm2 = momentum_update(rm, mean, momentum, n_updates) if rm is not None else None
    rv2 = momentum_update(rv, unbiased, momentum, n_updates) if rv is not None else None
    return BnFwd(y, mean, var, invstd, rm2, rv2, pre, terms)


def bn_train_bwd(dy, x, mean, invstd, gamma, gate=None):
    """dyr = dy * gate (gate: bool, None = no ReLU);  dbeta = sum dyr;  dgamma = sum dyr xhat;
    dx = gamma invstd (dyr - dbeta / n - xhat dgamma / n);  dres = dyr.  abs_*: the sums of the magnitudes of the terms."""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    dyr = dy if gate is None else dy * gate.to(dy.dtype)
    xhat = (x - _c(mean)) * _c(invstd)
    dbeta = dyr.sum((0, 2, 3))
    dgamma = (dyr * xhat).sum((0, 2, 3))
    dx = _c(gamma * invstd) * (dyr - _c(dbeta) / n - xhat * _c(dgamma) / n)
    return BnBwd(dx, dyr, dgamma, dbeta, (dyr * xhat).abs().sum((0, 2, 3)), dyr.abs().sum((0, 2, 3)))


def pool_candidates(a):
    """a (N, C, H, W), H and W even -> (9, N, C, H/2, W/2): the 3x3 window of every pooled element of MaxPool2d(3, 2, 1) in the order
    ky * 3 + kx, -inf outside the map"""
    N, C, H, W = a.shape
    OH, OW = H // 2, W // 2
    p = torch.full((N, C, H + 2, W + 2), float("-inf"), dtype=a.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = a
    return torch.stack([p[:, :, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] for ky in range(3) for kx in range(3)], 0)


def first_max(cand):
    """(9, ...) -> the maximum and the index of its FIRST occurrence in window order (a later equal candidate does not take over)"""
    best, idx = cand[0].clone(), torch.zeros(cand.shape[1:], dtype=torch.uint8)
    for k in range(1, cand.shape[0]):
        take = cand[k] > best
        best = torch.where(take, cand[k], best)
        idx = torch.where(take, torch.full_like(idx, k), idx)
    return best, idx


def bn_relu_pool_fwd(x, gamma, beta, eps=1e-5, momentum=0.1, n_updates=1, rm=None, rv=None):
    """maxpool(3, 2, 1)(relu(bn(x))) -> pooled map, argmax byte ky * 3 + kx (first maximum), the BnFwd of the normalisation and the
    nine candidates of every window"""
    bn = bn_train_fwd(x, gamma, beta, None, True, eps, momentum, n_updates, rm, rv)
    cand = pool_candidates(bn.y)
    pooled, idx = first_max(cand)
    return PoolFwd(pooled, idx, bn, cand)


def argmax_position(idx, H, W):
    """argmax byte (N, C, OH, OW) -> flat position iy * W + ix of the selected input element inside its (H, W) plane"""
    OH, OW = idx.shape[2:]
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    k = idx.long()
    return (2 * oy - 1 + k // 3) * W + (2 * ox - 1 + k % 3)


def scatter_pooled(dpool, idx, H, W):
    """the max-pool backward: every pooled gradient goes to the input element its argmax byte names"""
    N, C = dpool.shape[:2]
    pos = argmax_position(idx, H, W).reshape(N, C, -1)
    out = torch.zeros(N, C, H * W, dtype=dpool.dtype)
    out.scatter_add_(2, pos, dpool.reshape(N, C, -1))
    return out.view(N, C, H, W)


def bn_relu_pool_bwd(dpool, idx, x, mean, invstd, gamma, gate):
    """gradient of bn_relu_pool_fwd: dpool scattered through idx, then bn_train_bwd with the ReLU gate (N, C, H, W) over the statistics
    of the WHOLE map (count N H W)"""
    H, W = x.shape[2:]
    return bn_train_bwd(scatter_pooled(dpool, idx, H, W), x, mean, invstd, gamma, gate)


def bn_eval_fwd(x, gamma, beta, rm, rv, residual=None, relu=False, eps=1e-5):
    pre = (x - _c(rm)) * _c(gamma / torch.sqrt(rv + eps)) + _c(beta)
    if residual is not None:
        pre = pre + residual
    return torch.clamp(pre, min=0) if relu else pre


def channel_sum(x):
    return x.sum((0, 2, 3))


# ------------------------------------------------------------------------------------------- groups
def grouped_fwd(fn, groups, x, gamma, beta, rm, rv, residual=None, **kw):
    """`groups` independent forward passes stacked along N: fn (bn_train_fwd or bn_relu_pool_fwd) per slice, the running statistics
    updated group by group, in order.  -> the per-group results and the running statistics after the last group"""
    Ng = x.shape[0] // groups
    outs = []
    for g in range(groups):
        sl = slice(g * Ng, (g + 1) * Ng)
        if fn is bn_train_fwd:
            o = fn(x[sl], gamma, beta, residual[sl] if residual is not None else None, rm=rm, rv=rv, **kw)
            rm, rv = o.rm, o.rv
        else:
            o = fn(x[sl], gamma, beta, rm=rm, rv=rv, **kw)
            rm, rv = o.bn.rm, o.bn.rv
        outs.append(o)
    return outs, rm, rv
