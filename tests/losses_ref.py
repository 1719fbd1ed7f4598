"""Dtype-generic references of the loss kernels (test infrastructure, not part of the product).

Plain torch restatements of what jperceiver_amd/csrc/losses.hip and the min-reprojection reduction of photometric.hip compute, written
from the formulas of the losses and not from the kernels.  Every function works in the dtype of its inputs on the CPU: fed float64
leaves it is the referee of tests/test_losses_f64_gpu.py under autograd; tests/test_losses_ref_cpu.py holds it to oracle/jp_oracle.py
evaluated in float64 at 1e-12.  The signed distance is an integer min-plus transform and does not go through scipy.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------- smoothness
# The five stencils of the edge-aware smoothness term as (row offset, column offset, coefficient) taps; a stencil exists where all its
# taps lie inside the image.  dxy (the x difference of the y difference) equals dyx and is counted twice by the loss.
STENCILS = {
    "dx": ((0, 0, -1.0), (0, 1, 1.0)),
    "dy": ((0, 0, -1.0), (1, 0, 1.0)),
    "dxx": ((0, 0, 1.0), (0, 1, -2.0), (0, 2, 1.0)),
    "dyy": ((0, 0, 1.0), (1, 0, -2.0), (2, 0, 1.0)),
    "dxy": ((0, 0, 1.0), (0, 1, -1.0), (1, 0, -1.0), (1, 1, 1.0)),
}
STENCIL_COUNT = {"dx": 1, "dy": 1, "dxx": 1, "dyy": 1, "dxy": 2}
Smooth = namedtuple("Smooth", "loss stencils")


def stencil(t, taps):
    """t (..., h, w) -> sum_k coef_k * t[y + oy_k, x + ox_k] over the positions where every tap is inside"""
    h, w = t.shape[-2:]
    my, mx = max(o[0] for o in taps), max(o[1] for o in taps)
    return sum(c * t[..., oy:h - my + oy, ox:w - mx + ox] for oy, ox, c in taps)


def smooth(disp, img, weight):
    """disp (B,1,h,w), img (B,3,h,w) at the disparity's resolution -> weight * sum_kinds mean(|S(d / (mean d + 1e-7))| *
    exp(-0.5 * mean_c |S(img)|)) and the stencil values of the normalised disparity per kind (detached)."""
    dn = disp / (disp.mean((2, 3), keepdim=True) + 1e-7)
    loss, vals = 0, {}
    for kind, taps in STENCILS.items():
        s = stencil(dn, taps)
        e = torch.exp(-0.5 * stencil(img, taps).abs().mean(1, True))
        loss = loss + STENCIL_COUNT[kind] * (s.abs() * e).mean()
        vals[kind] = s.detach()
    return Smooth(loss * weight, vals)


def stencil_reach(ind, kind, h, w):
    """ind: bool map over the positions of a kind's stencils -> bool (..., h, w): the pixels that some marked stencil reads"""
    taps = STENCILS[kind]
    my, mx = max(o[0] for o in taps), max(o[1] for o in taps)
    out = torch.zeros(ind.shape[:-2] + (h, w), dtype=torch.bool)
    for oy, ox, _ in taps:
        out[..., oy:h - my + oy, ox:w - mx + ox] |= ind
    return out


# ------------------------------------------------------------------------------------------- scale loss
Scale = namedtuple("Scale", "loss pred valid")


def scale(disp, label, weight, min_depth, max_depth, crop=None):
    """disp (B,1,hs,ws) -> depth 1 / (1/max + (1/min - 1/max) disp) -> bilinear resize (align_corners=False) to the label's size ->
    clamp [1e-3, 80] -> weight * mean over {label > 0 inside crop} of |gt - pred| / gt.  crop = (y0, y1, x0, x1), half-open.
    Returns the loss (NaN when no pixel is valid), the resized depth BEFORE the clamp (detached) and the valid mask."""
    min_disp, max_disp = 1 / max_depth, 1 / min_depth
    depth = 1 / (min_disp + (max_disp - min_disp) * disp)
    pred = F.interpolate(depth, label.shape[2:], mode="bilinear", align_corners=False)
    valid = label > 0
    if crop is not None:
        inside = torch.zeros_like(valid)
        inside[:, :, crop[0]:crop[1], crop[2]:crop[3]] = True
        valid = valid & inside
    gt = label[valid]
    pr = torch.clamp(pred, 1e-3, 80)[valid]
    return Scale(weight * ((gt - pr).abs() / gt).mean(), pred.detach(), valid)


def resize_reach(ind, hs, ws):
    """ind (B,1,FH,FW) bool over label pixels -> (B,1,hs,ws) bool: the source pixels a marked label pixel interpolates from with a
    non-zero weight (the bilinear weights are non-negative, so backpropagating the indicator cannot cancel)."""
    x = torch.zeros(ind.shape[0], 1, hs, ws, dtype=torch.float64, requires_grad=True)
    (F.interpolate(x, ind.shape[2:], mode="bilinear", align_corners=False) * ind.double()).sum().backward()
    return x.grad > 0


# ------------------------------------------------------------------------------------------- layout loss
REGION = {"iou": (1.0, 1.0, 1.0), "dice": (2.0, 1.0, 1.0), "tversky": (1.0, 0.3, 0.7)}      # (a, alpha, beta) of the overlap score
FOCAL_ALPHA, FOCAL_GAMMA, FOCAL_SMOOTH = 0.25, 2.0, 1e-5


def region(logits, gt, kind):
    """logits (B,2,h,w), gt (B,h,w) long.  iou / dice / tversky: -mean_{b,c} (a tp + 1) / (a tp + alpha fp + beta fn + 1) with
    tp = sum p oh, fp = sum p (1 - oh), fn = sum (1 - p) oh per image and class.  focal: mean over pixels of
    -alpha_t (1 - pt)^gamma log(pt), pt = sum_c clamp(oh_c, smooth, 1 - smooth) p_c + smooth, alpha = (0.25, 0.75)."""
    p = F.softmax(logits, 1)
    oh = torch.stack([gt == 0, gt == 1], 1).to(logits.dtype)
    if kind == "focal":
        pt = (oh.clamp(FOCAL_SMOOTH, 1 - FOCAL_SMOOTH) * p).sum(1) + FOCAL_SMOOTH
        al = torch.where(gt == 0, FOCAL_ALPHA, 1 - FOCAL_ALPHA)
        return (-al * (1 - pt) ** FOCAL_GAMMA * pt.log()).mean()
    a, alpha, beta = REGION[kind]
    tp, fp, fn = (p * oh).sum((2, 3)), (p * (1 - oh)).sum((2, 3)), ((1 - p) * oh).sum((2, 3))
    return -((a * tp + 1) / (a * tp + alpha * fp + beta * fn + 1)).mean()


def weighted_ce(logits, gt, w0, w1):
    """sum_p w[gt_p] * -log softmax(logits)_p[gt_p] / sum_p w[gt_p]"""
    logp = F.log_softmax(logits, 1).gather(1, gt.unsqueeze(1)).squeeze(1)
    wt = torch.where(gt == 0, w0, w1).to(logits.dtype)
    return -(wt * logp).sum() / wt.sum()


def layout(logits, label, sdf, w0, w1, lw, cew, l2w, kind):
    """lw * region + cew * CE(w0, w1) + l2w * mean(p1 * sdf); label (B,1,h,w) {0,1}, sdf (B,h,w) or None"""
    gt = label.squeeze(1).long()
    out = lw * region(logits, gt, kind) + cew * weighted_ce(logits, gt, w0, w1)
    if sdf is not None:
        out = out + l2w * (F.softmax(logits, 1)[:, 1] * sdf).mean()
    return out


# ------------------------------------------------------------------------------------------- L1, row sum, min-reprojection
def l1(a, b):
    return (a - b).abs().mean()


def exact_sum(x):
    """the exactly rounded sum of a 1-d tensor as a python float"""
    return math.fsum(x.double().tolist())


MinReproj = namedtuple("MinReproj", "argmin total sum_abs margin fma_slack")


def min_reprojection(cands, noises, tie_partner=None):
    """cands: 1..4 fp32 tensors (n,), noises: fp32 tensors for the first len(noises) candidates.  The candidate values are formed in
    fp32 as the ABI states them, c_j + noise_j * 1e-5f with the product rounded before the sum; the argmin takes the first of equal
    values; the sum of the minima is exact.  margin: per pixel, the gap between the minimum and the nearest other candidate, leaving
    out the candidate tie_partner[i] (-1: none) that was made bit-equal on purpose.  fma_slack: sum over the winners of the difference
    between that value and c + noise * 1e-5f rounded once (a fused multiply-add), which a compiler may choose at either identity
    candidate; it is far below the margin, so the argmin is the same."""
    k = torch.tensor(1e-5, dtype=torch.float32)
    vals, alts = [], []
    for j, c in enumerate(cands):
        if j < len(noises):
            vals.append(c + noises[j] * k)
            alts.append((c.double() + noises[j].double() * k.double()).float())
        else:
            vals.append(c)
            alts.append(c)
    cat = torch.stack(vals, 0).double()
    m, arg = torch.min(cat, 0)
    other = cat.clone()
    other.scatter_(0, arg.unsqueeze(0), float("inf"))
    if tie_partner is not None:
        has = tie_partner >= 0
        other[tie_partner.clamp(min=0)[has], torch.nonzero(has).squeeze(1)] = float("inf")
    margin = other.amin(0) - m if len(cands) > 1 else torch.full_like(m, float("inf"))
    alt = torch.stack(alts, 0).double().gather(0, arg.unsqueeze(0)).squeeze(0)
    return MinReproj(arg, exact_sum(m), exact_sum(m.abs()), margin, exact_sum((alt - m).abs()))


# ------------------------------------------------------------------------------------------- exact signed distance
_FAR = 1 << 40


def _column_distance(want):
    """want (h,w) bool -> (h,w) int64: distance along the column to the nearest True pixel, _FAR where the column has none"""
    h = want.shape[0]
    ys = torch.arange(h)
    d = (ys.view(h, 1, 1) - ys.view(1, h, 1)).abs().expand(h, h, want.shape[1])
    return torch.where(want.unsqueeze(0), d, torch.tensor(_FAR)).amin(1)


def squared_distance(want):
    """want (h,w) bool -> (h,w) int64: squared Euclidean distance to the nearest True pixel (>= _FAR where there is none): a column
    pass, then per row min_x' (x - x')^2 + G[y, x']^2"""
    h, w = want.shape
    g = _column_distance(want)
    g2 = torch.where(g >= _FAR, torch.tensor(_FAR), g * g)
    xs = torch.arange(w)
    dx2 = (xs.view(w, 1) - xs.view(1, w)) ** 2
    out = torch.empty(h, w, dtype=torch.int64)
    for y0 in range(0, h, 32):
        out[y0:y0 + 32] = (dx2.unsqueeze(0) + g2[y0:y0 + 32].unsqueeze(1)).amin(2)
    return out


def inner_boundary(fg):
    """foreground pixels with a 4-neighbour of the other colour; the image border is no neighbour"""
    diff = torch.zeros_like(fg)
    diff[:-1] |= fg[:-1] != fg[1:]
    diff[1:] |= fg[1:] != fg[:-1]
    diff[:, :-1] |= fg[:, :-1] != fg[:, 1:]
    diff[:, 1:] |= fg[:, 1:] != fg[:, :-1]
    return diff & fg


SignedDistance = namedtuple("SignedDistance", "sdf d2 sign")


def signed_distance(label):
    """label (B,1,h,w) {0,1} -> per image: d2 (B,h,w) int64, the squared distance of a pixel to the nearest pixel of the other colour;
    sign -1 on foreground, +1 on background, 0 on the 4-connected inner boundary; sdf = sign * sqrt(d2) in float64.  An image without
    foreground is all zero (d2 = 0, sign = 0).  An image without background measures to the phantom site (-1, 0), as the Euclidean
    distance transform of an all-ones array does: d2 = (y + 1)^2 + x^2."""
    B, _, h, w = label.shape
    d2 = torch.zeros(B, h, w, dtype=torch.int64)
    sign = torch.zeros(B, h, w, dtype=torch.int64)
    for b in range(B):
        fg = label[b, 0] > 0.5
        if not bool(fg.any()):
            continue
        if bool(fg.all()):
            ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
            d2[b] = (ys + 1) ** 2 + xs ** 2
        else:
            d2[b] = torch.where(fg, squared_distance(~fg), squared_distance(fg))
        sign[b] = torch.where(fg, -1, 1) * (~inner_boundary(fg)).long()
    return SignedDistance(sign.double() * d2.double().sqrt(), d2, sign)
