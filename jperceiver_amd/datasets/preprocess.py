"""Device-side `MonoDataset.preprocess` (mono/datasets/mono_dataset.py:126-171,417-431): the raw uint8 frames of a batch
are uploaded once (pinned, asynchronous — datasets/loader.py) and resized / converted / augmented by HIP kernels
(csrc/preprocess.hip) instead of PIL + torchvision on 24 host workers per GPU.

  resize          transforms.Resize((H, W), Image.ANTIALIAS): Pillow's 8-bit Lanczos resampler, bit-exact (the
                  fixed-point coefficient tables are built here exactly like libImaging/Resample.c builds them)
  to_tensor       HWC uint8 -> CHW float32 / 255
  ColorJitter     brightness / contrast / saturation (0.8, 1.2), hue (-0.1, 0.1), random order.  Decided PER ITEM
                  (`do_color_aug = random.random() > 0.5`, mono_dataset.py:202); the parameters are drawn PER FRAME:
                  the reference hands `preprocess` a `transforms.ColorJitter` object (its `get_params` line is commented
                  out, mono_dataset.py:338-339) and such an object re-draws order + factors on every call, i.e. for
                  every frame of the item (mono_dataset.py:153-156).  `jitter="per_item"` gives what the docstring there
                  intends (one draw shared by an item's frames).  Applied in torchvision's float-tensor arithmetic (the
                  reference applies it to the 8-bit PIL image: values differ by <= ~1/255 rounding)
  process_topview luma, binarise, NEAREST resize to H/4
  flip            `do_flip = random.random() > 0.5` PER ITEM (mono_dataset.py:203): every getter applies
                  `transpose(pil.FLIP_LEFT_RIGHT)` to the raw image / BEV label before any resize.  Here a per-item flag
                  table on the device makes the first kernel that touches a raw frame or label read it mirrored
                  (jp_resample_h_u8_flip / jp_u8_to_tensor_flip / jp_topview_u8_flip); calibration is NOT adjusted, as in
                  the reference
  batched jitter  `batched=True`: the jitter of a whole batch in one jp_color_jitter_batched call per frame id (a
                  per-image parameter table on the device, two launches, the gray mean folded in a fixed order: the
                  same bits run to run) instead of up to six launches per augmented (item, frame)
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .._lib import call, lib

PRECISION_BITS = 32 - 8 - 2


def _lanczos(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    m = (x >= -3.0) & (x < 3.0)

    def sinc(v):
        r = np.ones_like(v)
        nz = v != 0.0
        pv = v[nz] * math.pi
        r[nz] = np.sin(pv) / pv
        return r
    out[m] = sinc(x[m]) * sinc(x[m] / 3.0)
    return out


def pil_resample_tables(in_size: int, out_size: int):
    """precompute_coeffs + normalize_coeffs_8bpc of Pillow's Resample.c for the Lanczos filter (support 3):
    -> bounds (out, 2) int32 {first tap, tap count}, kk (out, ksize) int32, ksize."""
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size      # box = (0, 0, in, in) held as C floats
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _lanczos((np.arange(xmax) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in w:                       # sequential sum, like the C loop
            ww += v
        if ww != 0.0:
            w = w / ww
        fx = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS))
        kk[xx, :xmax] = np.trunc(fx).astype(np.int32)          # (int) cast truncates toward zero
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


class ColorJitterParams:
    """torchvision.transforms.ColorJitter.get_params: a random order of the four ops and one factor each."""

    def __init__(self, brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=(-0.1, 0.1), generator=None):
        self.order = torch.randperm(4, generator=generator).tolist()
        u = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi, generator=generator))
        self.factors = [u(*brightness), u(*contrast), u(*saturation), u(*hue)]     # indexed by op id 0..3


CJ_RECORD_WORDS = 9            # jp_color_jitter_batched: n_ops, order[4], factor[4] (float bits) as int32


def color_jitter_table(params_list) -> np.ndarray:
    """The parameter table of jp_color_jitter_batched: (len(params_list), 9) int32, one record per image -- n_ops, the op ids in
    the order they are applied, and each op's factor (float bits).  An entry is a ColorJitterParams or None (n_ops = 0: the
    image is left untouched)."""
    tab = np.zeros((len(params_list), CJ_RECORD_WORDS), np.int32)
    fac = tab[:, 5:].view(np.float32)
    for i, p in enumerate(params_list):
        if p is None:
            continue
        order = [int(op) for op in p.order]
        if len(order) > 4 or any(op < 0 or op > 3 for op in order) or order.count(1) > 1:
            raise ValueError(f"ColorJitter order {order}: at most four ops with ids 0..3, contrast (1) at most once")
        tab[i, 0] = len(order)
        tab[i, 1:1 + len(order)] = order
        fac[i, :len(order)] = [float(p.factors[op]) for op in order]
    return tab


def _per_item(what, N, name, generator):
    """None -> one coin per item from the generator; a bool -> every item; a sequence -> per item (nothing is drawn)."""
    if what is None:
        return (torch.rand(N, generator=generator) > 0.5).tolist()
    if isinstance(what, (bool, int)):
        return [bool(what)] * N
    flags = [bool(c) for c in what]
    if len(flags) != N:
        raise ValueError(f"{name} has {len(flags)} entries for {N} items")
    return flags


def draw_augmentation(N, frame_ids, do_color_aug=None, do_flip=False, generator=None, jitter="per_frame"):
    """Every random decision of one batch, on the host, in the documented order -> (coins, flips, params).
    Draw order (generator): the N colour coins (do_color_aug is None), then the N flip coins (do_flip is None), then the
    jitter parameters per augmented item and per frame (`jitter="per_item"`: once per item).  Anything given explicitly
    consumes nothing, so do_flip=False draws exactly what the pipeline drew before it knew about flips.
    coins / flips: N bools; params: {(item, frame): ColorJitterParams} for the augmented items."""
    if jitter not in ("per_frame", "per_item"):
        raise ValueError(f"jitter={jitter!r}")
    coins = _per_item(do_color_aug, N, "do_color_aug", generator)
    flips = _per_item(do_flip, N, "do_flip", generator)
    params = {}                      # (item, frame) -> ColorJitterParams
    for i, c in enumerate(coins):
        if not c:
            continue
        shared = ColorJitterParams(generator=generator) if jitter == "per_item" else None
        for f in frame_ids:
            params[(i, f)] = shared if shared is not None else ColorJitterParams(generator=generator)
    return coins, flips, params


class DevicePreprocessor:
    """Preprocess one uploaded batch.  Tables are cached per (in, out) size; everything runs on the caller's stream."""

    def __init__(self, height, width, device):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.h, self.w, self.dev = height, width, dev
        self._tab = {}

    def _tables(self, n_in, n_out):
        key = (n_in, n_out)
        if key not in self._tab:
            b, k, ks = pil_resample_tables(n_in, n_out)
            self._tab[key] = (torch.from_numpy(b).to(self.dev), torch.from_numpy(k).to(self.dev), ks)
        return self._tab[key]

    def resize_u8(self, frames: torch.Tensor, OH: int, OW: int, want_u8=False, flip=None):
        """frames (N, H, W, C) uint8 on the device -> float (N, C, OH, OW) in [0, 1] (and the uint8 HWC image).
        flip: (N,) uint8 on the device, non-zero = resize the left-right mirrored frame (None: the plain kernels)."""
        N, H, W, C = frames.shape
        frames = frames.contiguous()
        if flip is not None:
            return self._resize_u8_flip(frames, OH, OW, want_u8, self._flags(flip, N))
        if (H, W) == (OH, OW):
            out = torch.empty((N, C, OH, OW), device=self.dev, dtype=torch.float32)
            call("jp_u8_to_tensor", frames, out, N, H, W, C)
            return (out, frames) if want_u8 else out
        bh, kh, ksh = self._tables(W, OW)
        bv, kv, ksv = self._tables(H, OH)
        tmp = torch.empty((N, H, OW, C), device=self.dev, dtype=torch.uint8)
        if W != OW:
            call("jp_resample_h_u8", frames, tmp, bh, kh, N * H, W, OW, C, ksh)
        else:
            tmp = frames
        out = torch.empty((N, C, OH, OW), device=self.dev, dtype=torch.float32)
        o8 = torch.empty((N, OH, OW, C), device=self.dev, dtype=torch.uint8) if want_u8 else None
        if H != OH:
            call("jp_resample_v_u8", tmp, o8, out, bv, kv, N, H, OH, OW, C, ksv)
        else:
            call("jp_u8_to_tensor", tmp, out, N, OH, OW, C)
            o8 = tmp
        return (out, o8) if want_u8 else out

    def _flags(self, flip, N):
        if not torch.is_tensor(flip) or flip.dtype != torch.uint8 or flip.shape != (N,):
            raise ValueError(f"flip must be a uint8 tensor of {N} flags on the device")
        return flip.contiguous()

    def _resize_u8_flip(self, frames, OH, OW, want_u8, flip):
        """resize_u8 of the frames mirrored where `flip` says so: the mirror is folded into the first pass that reads them."""
        N, H, W, C = frames.shape
        out = torch.empty((N, C, OH, OW), device=self.dev, dtype=torch.float32)
        if W == OW and H == OH:
            o8 = torch.empty((N, OH, OW, C), device=self.dev, dtype=torch.uint8) if want_u8 else None
            call("jp_u8_to_tensor_flip", frames, out, o8, flip, N, H, W, C)
            return (out, o8) if want_u8 else out
        tmp = torch.empty((N, H, OW, C), device=self.dev, dtype=torch.uint8)
        if W != OW:
            bh, kh, ksh = self._tables(W, OW)
            call("jp_resample_h_u8_flip", frames, tmp, bh, kh, flip, N, H, W, OW, C, ksh)
        else:
            call("jp_u8_to_tensor_flip", frames, None, tmp, flip, N, H, W, C)
        if H != OH:
            bv, kv, ksv = self._tables(H, OH)
            o8 = torch.empty((N, OH, OW, C), device=self.dev, dtype=torch.uint8) if want_u8 else None
            call("jp_resample_v_u8", tmp, o8, out, bv, kv, N, H, OH, OW, C, ksv)
        else:
            call("jp_u8_to_tensor", tmp, out, N, OH, OW, C)
            o8 = tmp
        return (out, o8) if want_u8 else out

    def color_jitter_(self, x: torch.Tensor, params: ColorJitterParams):
        """in place on (N, 3, H, W) floats; the SAME parameters for every image of the call."""
        N, C, H, W = x.shape
        assert C == 3 and x.is_contiguous()
        sums = torch.empty(N, device=x.device, dtype=torch.float64)
        for op in params.order:
            call("jp_color_jitter_op", x, sums, N, H * W, int(op), float(params.factors[op]))
        return x

    def color_jitter_batched_(self, x: torch.Tensor, params_list, table=None):
        """in place on (N, 3, H, W) floats, one jp_color_jitter_batched call: params_list[i] is image i's ColorJitterParams, or
        None for an image that is left untouched.  table: the (N, 9) int32 device copy of color_jitter_table(params_list) when
        the caller already uploaded it."""
        N, C, H, W = x.shape
        assert C == 3 and x.is_contiguous()
        if table is None:
            if len(params_list) != N:
                raise ValueError(f"{len(params_list)} parameter entries for {N} images")
            table = torch.from_numpy(color_jitter_table(params_list)).to(x.device)
        ws = torch.empty(lib().fn["jp_color_jitter_batched_ws_doubles"](N, H * W), device=x.device, dtype=torch.float64)
        call("jp_color_jitter_batched", x, table, ws, N, H * W)
        return x

    def topview(self, label_u8: torch.Tensor, size: int, both=False, flip=None):
        """process_topview / process_topview_both: (N, h, w[, C]) uint8 -> (N, 1, size, size) float {0, 1}.
        flip: (N,) uint8 on the device, non-zero = the label is mirrored left-right first (None: the plain kernel)."""
        if label_u8.dim() == 3:
            label_u8 = label_u8.unsqueeze(-1)
        N, h, w, C = label_u8.shape
        out = torch.empty((N, 1, size, size), device=self.dev, dtype=torch.float32)
        if flip is None:
            call("jp_topview_u8", label_u8.contiguous(), out, N, h, w, C, size, int(both))
        else:
            call("jp_topview_u8_flip", label_u8.contiguous(), out, self._flags(flip, N), N, h, w, C, size, int(both))
        return out

    def __call__(self, raw: dict, frame_ids, full_hw, do_color_aug=None, generator=None, jitter="per_frame", do_flip=False,
                 batched=False):
        """raw: {("color", f, -1): (N, h, w, 3) uint8, ("bothS"|"bothD"|"both_dynamic", 0, 0): uint8 labels, calibration
        tensors ...} already on the device -> the input dict Baseline.forward expects.
        do_color_aug: None -> one coin per ITEM (mono_dataset.py:202); a bool -> every item; a sequence -> per item.
        do_flip: the same three forms for the horizontal flip (mono_dataset.py:203); the default False flips nothing and draws
        nothing.  A flipped item has every ("color", f, -1) frame mirrored at raw resolution, before any resize, so its
        ("color", 0, -1), every ("color", f, 0) / ("color_aug", f, 0) and its bothS / bothD / both_dynamic labels are mirrored.
        Calibration (K, inv_K, odometry_K, Tr_cam2_velo, ...) and every other tensor pass through UNTOUCHED: the reference does
        not adjust them on a flip either (mono_dataset.py:203-345), so do not "fix" that here.  The flags are kept as
        self.last_flip.
        jitter: "per_frame" (the reference's actual behaviour: every frame of an augmented item gets its own draw) or
        "per_item" (one draw shared by the item's frames).
        batched: apply the jitter of the whole batch with one color_jitter_batched_ call per frame id (same draws; the gray
        mean is summed in another order, so augmented images may differ from batched=False in the last bits).
        Draw order (generator): the N colour coins, then the N flip coins (only for do_flip=None), then per item, per frame
        (draw_augmentation)."""
        out = {}
        FH, FW = full_hw
        N = raw[("color", frame_ids[0], -1)].shape[0]
        coins, flips, params = draw_augmentation(N, frame_ids, do_color_aug, do_flip, generator, jitter)
        self.last_jitter = params        # for loggers / tests
        self.last_flip = flips
        flip = torch.tensor(flips, dtype=torch.uint8).to(self.dev, non_blocking=True) if any(flips) else None
        tables = None
        if batched and any(coins):       # one upload for all frames: (frames, N, 9)
            tables = torch.from_numpy(np.stack([color_jitter_table([params.get((i, f)) for i in range(N)])
                                                for f in frame_ids])).to(self.dev, non_blocking=True)
        for j, f in enumerate(frame_ids):
            full, full8 = self.resize_u8(raw[("color", f, -1)], FH, FW, want_u8=True, flip=flip)   # resize_full, then resize from it
            if f == 0:
                out[("color", 0, -1)] = full
            img = self.resize_u8(full8, self.h, self.w)
            out[("color", f, 0)] = img
            aug = img.clone() if any(coins) else img
            if tables is not None:
                self.color_jitter_batched_(aug, None, table=tables[j])
            else:
                for i, c in enumerate(coins):
                    if c:
                        self.color_jitter_(aug[i:i + 1], params[(i, f)])
            out[("color_aug", f, 0)] = aug
        for k, v in raw.items():
            if k[0] in ("bothS", "bothD"):
                out[k] = self.topview(v, self.h // 4, flip=flip)
            elif k[0] == "both_dynamic":
                out[k] = self.topview(v, self.h // 4, both=True, flip=flip)
            elif k[0] != "color":
                out[k] = v.float() if torch.is_tensor(v) and v.dtype != torch.float32 else v
        return out
