"""Cases, seeded inputs, exclusion masks, input conditions and error metrics shared by tests/test_photometric_ref_cpu.py (which checks
every condition on the float64 reference without a GPU) and tests/test_photometric_f64_gpu.py (which runs the kernels).  Everything
here is CPU-only torch; nothing imports the HIP library."""
import math

import torch
import torch.nn.functional as F

from oracle import jp_oracle as J
from tests import photometric_ref as R

F64 = torch.float64
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0
LATTICE_DELTA = 3e-3          # per-pixel / per-go exclusion band around the bilinear lattice lines and the two clip borders
CLAMP_DELTA = 1e-5            # exclusion band of the SSIM clamp
MASK_CAP = 0.02               # either mask may leave out at most this share of a case


# ------------------------------------------------------------------------------------------- metrics
def err_abs(got, ref, keep=None):
    e = (got.detach().double() - ref.detach().double()).abs()
    return float(e[keep].max()) if keep is not None else float(e.max())


def err_rms(got, ref, keep=None):
    """max |err| / rms(reference) over the kept elements (per-pixel gradients)"""
    g, r = got.detach().double(), ref.detach().double()
    if keep is not None:
        g, r = g[keep], r[keep]
    return float((g - r).abs().max() / r.pow(2).mean().sqrt())


def err_max(got, ref):
    """max |err| / max |reference| (aggregated gradients, loss values)"""
    g, r = got.detach().double(), ref.detach().double()
    return float((g - r).abs().max() / r.abs().max())


def round_up_1sig(v):
    """v rounded up to one significant digit"""
    e = math.floor(math.log10(v))
    m = math.ceil(v / 10 ** e - 1e-9)
    return float(f"{m}e{e}") if m < 10 else float(f"1e{e + 1}")


# ------------------------------------------------------------------------------------------- bars
# Largest error of the project's fp32 CPU oracle (oracle/jp_oracle.py + ATen, float32) against the float64 reference over all cases of
# a quantity: same inputs, masks and metric as the GPU assertions (tests/test_photometric_ref_cpu.py recomputes them).
ORACLE_ERR = {
    "pose_T": 1.88e-7,         # max |err|, cam_T_cam
    "pose_P": 1.72e-7,         # max |err| / max |ref|, P = K T
    "pose_grad": 1.47e-5,      # max |err| / max |ref|, d_axisangle / d_translation of the pose alone (the |axisangle| = 1e-3 row)
    "warp_pred": 6.76e-5,      # max |err|, unmasked pixels
    "warp_ddisp_up": 2.56e-4,  # max |err| / rms(ref), unmasked pixels
    "warp_dP": 9.74e-6,        # max |err| / max |ref|
    "ssim_fwd": 2.48e-5,       # max |err|, unmasked windows
    "ssim_bwd": 6.23e-4,       # max |err| / rms(ref)
    "comp_loss": 1.36e-7,      # |err| / |ref|
    "comp_ddisp": 4.62e-5,     # max |err| / max |ref|
    "comp_daa": 5.96e-6,
    "comp_dtr": 4.25e-6,
}
# The bar of a quantity is 8 x that error rounded up to one significant digit: the kernels evaluate the same fp32 formulas in another
# order (P = K T pre-multiplied, contracted FMAs, rsqrt and a reciprocal), so a few times the oracle's error is expected and an order of
# magnitude more is not; a real defect (a shifted texel, a wrong clip mask, a dropped add, a wrong candidate) is 1e-2 or more.
BARS = {k: round_up_1sig(8 * v) for k, v in ORACLE_ERR.items()}
# Three bars are TIGHTER than the rule gives:
#  - warp_ddisp_up, ssim_bwd: the rule gives 3e-3 and 5e-3, but every gradient bar has to sit at least 20 x under the former 2e-2
#    of test_cgt_warp_and_pose.  That leaves 3.9 x and 1.6 x the oracle's own error: its SSIM gradient is limited by the variance
#    cancellation E[x^2] - mu^2 against C2 = 9e-4 in the flat and saturated rectangles.
#  - pose_grad: jp_pose_bwd is evaluated in double from fp32 inputs, so unlike the fp32 oracle (1.5e-5 off at |axisangle| = 1e-3,
#    the cancellation the kernel was moved to double for) it owes nothing but the final rounding of its fp32 outputs, 2^-24 of an
#    element's own magnitude, plus a few double ulps through 1 - cos(th) and the th > 0 quotient: 5 x 2^-24 = 3e-7.
BARS["warp_ddisp_up"] = 1e-3
BARS["ssim_bwd"] = 1e-3
BARS["pose_grad"] = 3e-7
BAR_EXCEPTIONS = ("warp_ddisp_up", "ssim_bwd", "pose_grad")


# ------------------------------------------------------------------------------------------- geometry
def intrinsics(B, H, W):
    K = torch.tensor([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]).repeat(B, 1, 1)
    return K, torch.linalg.pinv(K)


# ------------------------------------------------------------------------------------------- (a) pose
POSE_ANGLES = (0.0, 1e-6, 1e-3, 3e-2, 0.3, 3.1)


def pose_inputs(seed=11):
    """B = 6: one launch holds |axisangle| = 0, 1e-6, 1e-3, 3e-2, 0.3, 3.1, each with a random direction."""
    B = len(POSE_ANGLES)
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(B, 3, generator=g, dtype=F64)
    aa = (d / d.norm(dim=1, keepdim=True) * torch.tensor(POSE_ANGLES, dtype=F64).view(B, 1)).float()
    tr = ((torch.rand(B, 3, generator=g) - 0.5) * 0.2)
    K, _ = intrinsics(B, 24, 80)
    dP = torch.randn(B, 12, generator=g, dtype=F64)
    return aa, tr, K, dP


def pose_reference(aa, tr, K, dP, invert, dtype=F64):
    """-> T, P, d_axisangle, d_translation in `dtype` (autograd of the restatement under the upstream dP)"""
    a, t = aa.detach().to(dtype).clone().requires_grad_(True), tr.detach().to(dtype).clone().requires_grad_(True)
    T, P = R.pose(a, t, K.to(dtype), invert)
    (P * dP.to(dtype).view(-1, 3, 4)).sum().backward()
    return T.detach(), P.detach(), a.grad, t.grad


# ------------------------------------------------------------------------------------------- (b) warp
# name: (B, H, W, hs, ws)
WARP_SHAPES = {
    "24x300": (3, 24, 300, 6, 75),     # second forward column block, ragged; 4 backward workgroups, last one ragged
    "40x72": (2, 40, 72, 5, 9),        # coarse source map (ratio 8): the upsampling source coordinate clamps at every edge
    "33x70": (2, 33, 70, 33, 70),      # ratio 1; H % 4 != 0: ragged last forward row band
    "9x260": (1, 9, 260, 3, 65),       # one row band of a second column block; H*W not a multiple of 256
}
# (shape, regime) -> committed seed: the first seed from 0 on whose float64 reference meets every condition of warp_conditions
WARP_SEEDS = {("24x300", "gentle"): 0, ("24x300", "wild"): 2, ("24x300", "behind"): 0,
              ("40x72", "gentle"): 0, ("40x72", "wild"): 12, ("40x72", "behind"): 3,
              ("33x70", "gentle"): 0, ("33x70", "wild"): 12, ("33x70", "behind"): 0,
              ("9x260", "gentle"): 0, ("9x260", "wild"): 56, ("9x260", "behind"): 0}
TWO_FRAME_CASE = ("24x300", "gentle")    # two source frames (frame 0 and 1 of the same seed) into one ddisp_up
WARP_CASES = [(s, r) for s in WARP_SHAPES for r in ("gentle", "wild", "behind")]
# No |z + 1e-7| below this in any case.  fp32 forms z as a four-term sum of magnitude <= 1, so it carries ~1e-7 of absolute error; a
# coordinate inside the image (|ix| <= 300) then moves by 300 * 1e-7 / |z| <= 1e-3, inside the lattice band, and the sign of z is
# never in doubt.  A random disparity field crosses z = 0 continuously, so the behind-the-camera regime is built from two depth bands.
Z_FLOOR = 0.03


def warp_inputs(shape, regime, seed, frame=0):
    """Seeded inputs of one source frame.  `frame` > 0 draws another pose / colour / upstream gradient for the same disparity."""
    B, H, W, hs, ws = WARP_SHAPES[shape]
    K, invK = intrinsics(B, H, W)
    g = torch.Generator().manual_seed(1000 * seed + 17)
    u = torch.rand(B, 1, hs, ws, generator=g)
    disp = 0.005 + 0.045 * u if regime == "gentle" else 0.2 + 0.5 * u
    if regime == "behind":
        # two depth bands, far (disp 0.02 .. 0.05: depth 2 .. 4.8) and, in one random column interval per image, near (disp 0.6 .. 0.7:
        # depth ~0.15); the camera steps back by ~0.5, which leaves the near band behind it.  The bilinear ramp between the bands crosses
        # z = 0 within one source cell; the seed decides whether a pixel of the ramp lands inside Z_FLOOR.
        lo = (torch.rand(B, generator=g) * 0.5 * ws).long()
        wid = (ws * (0.3 + 0.2 * torch.rand(B, generator=g))).long().clamp(min=1)
        cols = torch.arange(ws).view(1, ws)
        near = ((cols >= lo.view(B, 1)) & (cols < (lo + wid).view(B, 1))).view(B, 1, 1, ws)
        disp = torch.where(near, 0.6 + 0.1 * u, 0.02 + 0.03 * u)
    g = torch.Generator().manual_seed(1000 * seed + 100 + frame)
    aa = (torch.rand(B, 3, generator=g) - 0.5) * 0.06
    tr = (torch.rand(B, 3, generator=g) - 0.5) * 0.2
    if regime == "behind":
        tr[:, 2] = -0.5 + 0.06 * (torch.rand(B, generator=g) - 0.5)
    col = torch.rand(B, 3, H, W, generator=g)
    go = torch.randn(B, 3, H, W, generator=g)
    # the kernel is handed this fp32 P; the reference starts from the same numbers
    P = R.pose(aa.double(), tr.double(), K.double(), bool(frame % 2))[1].float()
    return dict(B=B, H=H, W=W, hs=hs, ws=ws, disp=disp, invK=invK, P=P, color=col, go=go)


def lattice_mask(ix, iy, H, W, delta):
    """True where a sampling coordinate lies within delta of an integer in [0, size-1] (the clip borders 0 and size-1 included)"""
    def near(c, n):
        return (c - c.round().clamp(0, n - 1)).abs() < delta
    return near(ix, W) | near(iy, H)


def warp_forward(inp, dtype=F64):
    """forward of the restatement with fresh leaves -> (WarpOut, disp leaf, P leaf)"""
    d = inp["disp"].to(dtype).clone().requires_grad_(True)
    P = inp["P"].to(dtype).clone().requires_grad_(True)
    w = R.warp(d, inp["invK"].to(dtype), P, inp["color"].to(dtype), inp["H"], inp["W"], MIN_DEPTH, MAX_DEPTH)
    return w, d, P


def warp_reference(inp, dtype=F64, mask=None):
    """-> dict(pred, ix, iy, z, mask, go, ddisp_up, dP, ddisp).  The lattice mask comes from this evaluation unless one is given (the
    fp32 twin is handed the float64 mask); the upstream gradient is zeroed under it."""
    w, d, P = warp_forward(inp, dtype)
    if mask is None:
        mask = lattice_mask(w.ix, w.iy, inp["H"], inp["W"], LATTICE_DELTA)
    go = inp["go"] * (~mask).unsqueeze(1)
    (w.pred * go.to(dtype)).sum().backward()
    return dict(pred=w.pred.detach(), ix=w.ix, iy=w.iy, z=w.z, mask=mask, go=go, ddisp_up=w.disp_up.grad, dP=P.grad.reshape(-1, 12),
                ddisp=d.grad)


def warp_oracle_fp32(inp, mask):
    """The project's fp32 CPU oracle (oracle/jp_oracle.py + ATen) on the same inputs and masked upstream gradient.  P enters as
    K = identity, T = [P; 0 0 0 1], so that the gradient of T's first three rows is dP."""
    B, H, W = inp["B"], inp["H"], inp["W"]
    d = inp["disp"].clone().requires_grad_(True)
    T = torch.cat([inp["P"], torch.tensor([0, 0, 0, 1.0]).expand(B, 1, 4)], 1).requires_grad_(True)
    d_up = F.interpolate(d, [H, W], mode="bilinear", align_corners=False)
    d_up.retain_grad()
    _, depth = J.disp_to_depth(d_up, MIN_DEPTH, MAX_DEPTH)
    grid = J.project(J.backproject(depth, inp["invK"]), torch.eye(4).repeat(B, 1, 1), T, H, W)
    pr = F.grid_sample(inp["color"], grid, mode="bilinear", padding_mode="border", align_corners=False)
    go = inp["go"] * (~mask).unsqueeze(1)
    (pr * go).sum().backward()
    return dict(pred=pr.detach(), ddisp_up=d_up.grad, dP=T.grad[:, :3].reshape(B, 12), ddisp=d.grad)


def warp_conditions(regime, ref, H, W):
    """-> list of failed conditions (empty: the case is admissible), from the float64 reference alone"""
    ix, iy, z = ref["ix"], ref["iy"], ref["z"]
    bad = []
    if not (torch.isfinite(ix).all() and torch.isfinite(iy).all()):
        bad.append("non-finite coordinate")
    share = float(ref["mask"].double().mean())
    if share > MASK_CAP:
        bad.append(f"lattice mask {share:.4f} > {MASK_CAP}")
    zmin = float((z + 1e-7).abs().min())
    if zmin < Z_FLOOR:
        bad.append(f"|z| {zmin:.2e} < {Z_FLOOR}")
    inx, iny = (ix > 0) & (ix < W - 1), (iy > 0) & (iy < H - 1)
    if regime == "gentle":
        s = float((inx & iny).double().mean())
        if s < 0.5:
            bad.append(f"unclipped share {s:.3f} < 0.5")
    if regime == "wild":
        for nm, m in (("left", ix <= 0), ("right", ix >= W - 1), ("top", iy <= 0), ("bottom", iy >= H - 1)):
            s = float(m.double().mean())
            if s < 0.05:
                bad.append(f"{nm} border share {s:.3f} < 0.05")
    if regime == "behind":
        s = float((z <= 0).double().mean())
        if s < 0.10:
            bad.append(f"z <= 0 share {s:.3f} < 0.10")
    return bad


def find_warp_seed(shape, regime, limit=2000):
    _, H, W, _, _ = WARP_SHAPES[shape]
    for seed in range(limit):
        inp = warp_inputs(shape, regime, seed)
        with torch.no_grad():
            w = R.warp(inp["disp"].double(), inp["invK"].double(), inp["P"].double(), inp["color"].double(), H, W, MIN_DEPTH, MAX_DEPTH)
        ref = dict(ix=w.ix, iy=w.iy, z=w.z, mask=lattice_mask(w.ix, w.iy, H, W, LATTICE_DELTA))
        if not warp_conditions(regime, ref, H, W):
            return seed
    raise RuntimeError(f"no admissible seed for {shape} {regime}")


# ------------------------------------------------------------------------------------------- (c) SSIM + L1
SSIM_SHAPES = [(2, 2), (2, 3), (3, 2), (3, 3), (4, 62), (5, 63), (8, 64), (9, 65), (17, 124), (3, 125), (6, 257), (12, 300)]
SSIM_GOUT, SSIM_GSCALE = 0.37, 0.61
SSIM_MASKED_INDEX = 7          # min_index written at clamp-masked windows: matches no candidate, on the device and in the reference


def _erode(m, r):
    """m (B,H,W) bool -> True where every in-image pixel within Chebyshev distance r is True"""
    return F.max_pool2d((~m).float().unsqueeze(1), 2 * r + 1, 1, r).squeeze(1) == 0


def ssim_inputs(H, W, seed=5):
    """x, y as test_ssim_l1_fwd_bwd draws them (y = 0.7 x + 0.3 r) plus a constant-colour rectangle in both images, a rectangle where
    pred == target bit for bit and a rectangle saturated at 1.0 in pred only.  Images of 2 or 3 rows and columns cannot hold
    rectangles: there B = 4 and images 1, 2, 3 are entirely constant / equal / saturated.  -> x, y, index map, equal-rectangle mask"""
    tiny = H <= 3 and W <= 3
    B = 4 if tiny else 2
    g = torch.Generator().manual_seed(seed + 131 * H + W)
    x = torch.rand(B, 3, H, W, generator=g)
    y = 0.7 * x + 0.3 * torch.rand(B, 3, H, W, generator=g)
    cx, cy = torch.rand(3, generator=g).view(3, 1, 1), torch.rand(3, generator=g).view(3, 1, 1)
    eq = torch.zeros(B, H, W, dtype=torch.bool)
    if tiny:
        x[1], y[1] = cx.expand(3, H, W), cy.expand(3, H, W)
        eq[2] = True
        x[3] = 1.0
    else:
        r0, r1, c0, c1 = H // 4, H // 4 + max(1, H // 2), W // 8, W // 8 + W // 4
        x[0, :, r0:r1, c0:c1], y[0, :, r0:r1, c0:c1] = cx, cy
        eq[1, :, W // 2:W // 2 + max(6, W // 4)] = True
        eq[0, H // 2:, W - max(6, W // 5):] = True
        x[1, :, H // 2:, :W // 4] = 1.0
    y = torch.where(eq.unsqueeze(1), x, y)
    idx = (torch.rand(B, H, W, generator=g) * 4).long()
    return x, y, idx, eq


def ssim_reference(x, y, dtype=F64):
    """forward of the restatement -> (x leaf, loss map (B,1,H,W) with graph, pre-clamp SSIM (B,3,H,W))"""
    xr = x.to(dtype).clone().requires_grad_(True)
    lr, pre = R.reprojection(xr, y.to(dtype))
    return xr, lr, pre


def ssim_masks(pre, eq):
    """-> (masked windows (B,H,W), exact-zero windows, asserted equal-rectangle pixels).  A window is masked when any channel's float64
    pre-clamp value is within CLAMP_DELTA of 0 or 1 -- except the windows whose whole 3x3 support lies in the pred == target
    rectangle: their value is exactly 0 and so is their derivative on either side of the clamp gate."""
    near = ((pre.abs() < CLAMP_DELTA) | ((pre - 1).abs() < CLAMP_DELTA)).any(1)
    exact0 = _erode(eq, 1)
    return near & ~exact0, exact0, _erode(eq, 2)


def ssim_grad(xr, lr, weight):
    """d sum(weight * loss map) / d pred with the graph kept for the next candidate"""
    g, = torch.autograd.grad((lr * weight.to(lr.dtype).unsqueeze(1)).sum(), xr, retain_graph=True)
    return g


def ssim_weights(idx, masked):
    """-> (index map with masked windows disabled, [(cand or None, per-window weight (B,H,W), pixels to compare (B,H,W))...]).  With an
    index the masked windows get weight 0 on both sides and every pixel is compared; without one (NULL min_index) every window
    weighs in, and the pixels a masked window reaches (its 3x3 support) are left out."""
    idm = torch.where(masked, torch.full_like(idx, SSIM_MASKED_INDEX), idx)
    s = SSIM_GOUT * SSIM_GSCALE
    every = torch.ones_like(masked)
    runs = [(c, (idm == c).double() * s, every) for c in range(4)]
    runs.append((None, torch.full(idx.shape, s, dtype=F64), _erode(~masked, 1)))
    return idm, runs


# ------------------------------------------------------------------------------------------- (d) the composite
COMP_B, COMP_H, COMP_W = 2, 16, 24
COMP_SCALES = [(16, 24), (8, 12), (4, 6)]
COMP_GOUT = (0.8, 1.3, 0.6)              # upstream gradients of the three loss slots (non-unit)
COMP_INVERT = (True, False)              # frame -1, frame +1
COMP_LATTICE, COMP_MARGIN, COMP_WIN = 1e-3, 1e-5, 0.02
COMP_SEED = 1                            # first seed from 0 on that meets composite_conditions (find_composite_seed)


def composite_inputs(seed):
    """Two source frames, three disparity scales, two identity candidates with noise.  Here no upstream gradient can be masked per
    pixel, so the inputs are safe by construction.  The reference maps pixel u to ix = u * W / (W - 1) - 0.5 (it normalises by W - 1
    and grid_sample un-normalises by W), so even a still camera sweeps a whole lattice cell across the image: the integer pixels then
    sit at multiples of 1 / (W - 1) with the nearest 1 / (2 (W - 1)) = 0.022 (x) and 0.033 (y) from a lattice line.  The motion keeps
    the per-pixel variation of the shift under that: pose-network-sized rotations (|axisangle| ~ 4e-3, the regime jp_pose_bwd's
    double arithmetic exists for), focal length 4 W, depths 2.9 .. 3.1, translations of ~2e-3.  The seed is searched until the common
    shift lands every coordinate at least COMP_LATTICE from a lattice line (composite_conditions)."""
    B, H, W = COMP_B, COMP_H, COMP_W
    g = torch.Generator().manual_seed(7000 + seed)
    f = 4.0 * W
    K = torch.tensor([[f, 0, 0.5 * W, 0], [0, f, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]).repeat(B, 1, 1)
    invK = torch.linalg.pinv(K)
    disps = [(1 / (2.9 + 0.2 * torch.rand(B, 1, h, w, generator=g)) - 0.01) / 9.99 for h, w in COMP_SCALES]
    aas, trs = [], []
    for j in range(2):
        aas.append((torch.rand(B, 3, generator=g) - 0.5) * torch.tensor([6e-3, 6e-3, 4e-4]))
        trs.append((torch.rand(B, 3, generator=g) - 0.5) * torch.tensor([4e-3, 4e-3, 1e-3]))
    target = torch.rand(B, 3, H, W, generator=g)
    colors = [torch.rand(B, 3, H, W, generator=g) for _ in range(2)]
    noises = [[torch.randn(B, 1, H, W, generator=g) for _ in range(2)] for _ in COMP_SCALES]
    return dict(K=K, invK=invK, disps=disps, aas=aas, trs=trs, target=target, colors=colors, noises=noises)


def composite_reference(inp, dtype=F64):
    """-> dict(loss [3], argmin [3], margin [3], ddisp [3], daa [2], dtr [2], outs [3 MinReproj]) from the restatement in `dtype`"""
    c = lambda t: t.to(dtype)
    H, W = COMP_H, COMP_W
    aas = [c(a).clone().requires_grad_(True) for a in inp["aas"]]
    trs = [c(t).clone().requires_grad_(True) for t in inp["trs"]]
    disps = [c(d).clone().requires_grad_(True) for d in inp["disps"]]
    Ps = [R.pose(a, t, c(inp["K"]), inv)[1] for a, t, inv in zip(aas, trs, COMP_INVERT)]
    target, colors = c(inp["target"]), [c(x) for x in inp["colors"]]
    idl = [R.reprojection(x, target)[0] for x in colors]
    outs = [R.min_reprojection(d, c(inp["invK"]), Ps, colors, target, idl, [c(n) for n in nz], H, W, MIN_DEPTH, MAX_DEPTH,
                               len(COMP_SCALES)) for d, nz in zip(disps, inp["noises"])]
    sum(o.loss * g for o, g in zip(outs, COMP_GOUT)).backward()
    return dict(loss=[o.loss.detach() for o in outs], argmin=[o.argmin for o in outs], margin=[o.margin for o in outs],
                ddisp=[d.grad for d in disps], daa=[a.grad for a in aas], dtr=[t.grad for t in trs], outs=outs)


def composite_oracle_fp32(inp):
    """the same composite from oracle/jp_oracle.py's fp32 pieces"""
    B, H, W = COMP_B, COMP_H, COMP_W
    aas = [a.clone().requires_grad_(True) for a in inp["aas"]]
    trs = [t.clone().requires_grad_(True) for t in inp["trs"]]
    disps = [d.clone().requires_grad_(True) for d in inp["disps"]]
    Ts = [J.transformation_from_parameters(a.view(B, 1, 3), t.view(B, 1, 3), inv) for a, t, inv in zip(aas, trs, COMP_INVERT)]
    idl = [J.reprojection_loss(x, inp["target"]) for x in inp["colors"]]
    loss, arg = [], []
    for d, nz in zip(disps, inp["noises"]):
        d_up = F.interpolate(d, [H, W], mode="bilinear", align_corners=False)
        _, depth = J.disp_to_depth(d_up, MIN_DEPTH, MAX_DEPTH)
        cands = [i + n * 1e-5 for i, n in zip(idl, nz)]
        for T, col in zip(Ts, inp["colors"]):
            grid = J.project(J.backproject(depth, inp["invK"]), inp["K"], T, H, W)
            pr = F.grid_sample(col, grid, mode="bilinear", padding_mode="border", align_corners=False)
            cands.append(J.reprojection_loss(pr, inp["target"]))
        m, a = torch.min(torch.cat(cands, 1), dim=1)
        loss.append(m.mean() / len(COMP_SCALES))
        arg.append(a)
    sum(l * g for l, g in zip(loss, COMP_GOUT)).backward()
    return dict(loss=[l.detach() for l in loss], argmin=arg, ddisp=[d.grad for d in disps], daa=[a.grad for a in aas],
                dtr=[t.grad for t in trs])


def composite_conditions(ref):
    """-> list of failed conditions, all with cap 0, from the float64 reference alone"""
    H, W = COMP_H, COMP_W
    bad = []
    for s, o in enumerate(ref["outs"]):
        for j, w in enumerate(o.warps):
            if bool(lattice_mask(w.ix, w.iy, H, W, COMP_LATTICE).any()):
                bad.append(f"scale {s} frame {j}: coordinate within {COMP_LATTICE} of a lattice line")
            if float((w.z + 1e-7).abs().min()) < Z_FLOOR:
                bad.append(f"scale {s} frame {j}: |z| below {Z_FLOOR}")
        if float(o.margin.min()) < COMP_MARGIN:
            bad.append(f"scale {s}: argmin margin {float(o.margin.min()):.2e}")
        for j, pre in enumerate(o.pre):
            if bool(((pre.abs() < CLAMP_DELTA) | ((pre - 1).abs() < CLAMP_DELTA)).any()):
                bad.append(f"scale {s} frame {j}: SSIM within {CLAMP_DELTA} of the clamp")
        share = torch.bincount(o.argmin.flatten(), minlength=4).double() / o.argmin.numel()
        if float(share.min()) < COMP_WIN:
            bad.append(f"scale {s}: candidate shares {share.tolist()}")
    return bad


def find_composite_seed(limit=20000):
    for seed in range(limit):
        if not composite_conditions(composite_reference(composite_inputs(seed))):
            return seed
    raise RuntimeError("no admissible composite seed")
