"""Training-branch colour augmentation: host sampler + device op (``zp_augment``, csrc/zp_crop.hip).

The reference's ``apply_augmentation`` (bop_dataset_pytorch.py:349-355) runs, for 80 % of the
samples, the imgaug chain of ``GDR_Net_Augmentation.build_augmentations``
(GDR_Net_Augmentation.py:161-178), ``Sequential(random_order=False)``:

    Sometimes(0.3, SaltAndPepper(0.05))                    if use_peper_salt
    Sometimes(0.2, MotionBlur(k=5))                        if use_motion_blur
    Sometimes(0.4, CoarseDropout(p=0.1, size_percent=0.05))
    Sometimes(0.5, GaussianBlur(np.random.rand()))         sigma: one draw per sample
    Sometimes(0.5, Add((-20, 20), per_channel=0.3))
    Sometimes(0.4, Invert(0.20, per_channel=True))
    Sometimes(0.5, Multiply((0.7, 1.4), per_channel=0.8))
    Sometimes(0.5, Multiply((0.7, 1.4)))
    Sometimes(0.5, LinearContrast((0.5, 2.0), per_channel=0.3))

Here every random choice is sampled on the host by ``AugmentSampler`` (plain numpy, one
``np.random.Generator``) and handed to the device as small per-crop descriptors: a position-hash
seed and threshold (salt and pepper), two 5 x 5 Q16 integer stencils (motion blur, Gaussian blur),
a low-resolution keep-mask (coarse dropout) and one composed u8 LUT per channel (the five
point-wise stages).  The device then does exact integer pixel work only, so a batch is
bit-reproducible from its descriptors.

PARITY UNPINNED: imgaug 0.4.0 and OpenCV 4.x are absent here, so nothing below is checked against
the libraries themselves.  The distributions restate imgaug's parameters (ranges, per_channel
probabilities, the u8 LUT formulas, MotionBlur's direction ramp rotated bilinearly, the 5-tap
Gaussian kernel for sigma < 1, SaltAndPepper's Beta(0.5, 0.5) replacement values); the random
streams differ (imgaug draws per pixel from its own generators, the device hashes the position),
and the blurs are Q16 integer stencils rather than OpenCV's float / fixed-point filters.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L

AUG_SP, AUG_STENCIL_A, AUG_DROPOUT, AUG_STENCIL_B, AUG_LUT = 1, 2, 4, 8, 16  # include/zp.h
DESC_DTYPE = np.dtype([("flags", "<u4"), ("sp_seed", "<u4"), ("sp_thresh", "<u4"), ("kA", "<i4", (25,)),
                       ("kB", "<i4", (25,))])  # = zp_aug_desc
SP_P = 0.05
CHAIN_P = 0.8  # color_aug_prob (bop_dataset_pytorch.py:351)


def beta_table():
    """u8 [256]: the quantiles (k + 0.5) / 256 of Beta(0.5, 0.5) * 255, SaltAndPepper's replacement
    values (the arcsine law's inverse CDF is sin^2(pi u / 2))."""
    k = np.arange(256, dtype=np.float64)
    return np.rint(255.0 * np.sin(np.pi * (k + 0.5) / 512.0) ** 2).astype(np.uint8)


# ---- point-wise stages as u8 LUTs [3][256]; every parameter is per channel ([3]) ----------------
_I = np.arange(256, dtype=np.float64)


def lut_add(v):
    return np.clip(_I[None, :] + np.asarray(v, np.float64).reshape(3, 1), 0, 255).astype(np.uint8)


def lut_invert(on):
    on = np.asarray(on, bool).reshape(3, 1)
    return np.where(on, 255 - _I[None, :], _I[None, :]).astype(np.uint8)


def lut_multiply(m):
    return np.clip(np.rint(_I[None, :] * np.asarray(m, np.float64).reshape(3, 1)), 0, 255).astype(np.uint8)


def lut_contrast(alpha):
    t = 127.0 + np.asarray(alpha, np.float64).reshape(3, 1) * (_I[None, :] - 127.0)
    return np.clip(t, 0, 255).astype(np.uint8)  # truncated


def compose_luts(luts):
    """LUTs applied in list order: out[c][i] = l_n[c][... l_1[c][l_0[c][i]]]."""
    out = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    rows = np.arange(3)[:, None]
    for l in luts:
        out = np.asarray(l, np.uint8)[rows, out]
    return out


# ---- stencils -------------------------------------------------------------------------------
def identity_kernel():
    k = np.zeros((5, 5), np.int32)
    k[2, 2] = 65536
    return k


def gaussian_taps(sigma):
    """Q8 1-D taps [5]: exp(-x^2 / 2 sigma^2) normalised, the outer pairs rounded to nearest, the
    centre taking the remainder (sum 256)."""
    x = np.arange(-2, 3, dtype=np.float64)
    w = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    w /= w.sum()
    o2, o1 = int(np.rint(256.0 * w[0])), int(np.rint(256.0 * w[1]))
    return np.array([o2, o1, 256 - 2 * (o1 + o2), o1, o2], np.int32)


def gaussian_kernel(sigma):
    t = gaussian_taps(sigma)
    return np.outer(t, t).astype(np.int32)


def motion_kernel(angle, direction):
    """MotionBlur(k=5, angle, direction, order=1): the centre column carries
    linspace(d, 1 - d, 5) with d = (clip(direction, -1, 1) + 1) / 2, as a u8 image; it is rotated by
    ``angle`` degrees about the centre with bilinear sampling (zero outside) and normalised, then
    quantised to Q16 by largest remainder (sum exactly 65536)."""
    d = (float(np.clip(direction, -1.0, 1.0)) + 1.0) / 2.0
    m = np.zeros((5, 5), np.float64)
    m[:, 2] = (np.linspace(d, 1.0 - d, 5) * 255.0).astype(np.uint8)
    th = np.deg2rad(float(angle))
    c, s = np.cos(th), np.sin(th)
    yy, xx = np.mgrid[0:5, 0:5].astype(np.float64) - 2.0
    sx, sy = c * xx + s * yy + 2.0, -s * xx + c * yy + 2.0  # inverse map: output -> source
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    pad = np.zeros((9, 9), np.float64)  # source with a zero frame: taps out to [-2, 6] read 0
    pad[2:7, 2:7] = m
    xi = np.clip(x0.astype(np.int64) + 2, 0, 7)
    yi = np.clip(y0.astype(np.int64) + 2, 0, 7)
    r = (pad[yi, xi] * (1 - fx) * (1 - fy) + pad[yi, xi + 1] * fx * (1 - fy) +
         pad[yi + 1, xi] * (1 - fx) * fy + pad[yi + 1, xi + 1] * fx * fy)
    r = np.clip(np.rint(r), 0, 255) / 255.0
    return quantise_q16(r / r.sum())


def quantise_q16(w):
    """Non-negative weights summing to 1 -> int32 summing to exactly 65536 (largest remainder)."""
    t = np.asarray(w, np.float64) * 65536.0
    q = np.floor(t).astype(np.int64)
    rest = int(65536 - q.sum())
    order = np.argsort(-(t - q).ravel(), kind="stable")[:rest]
    q.ravel()[order] += 1
    return q.astype(np.int32)


@dataclass
class AugBatch:
    """Descriptors of one batch for ``zp_augment``."""
    flags: np.ndarray      # u32 [B]
    sp_seed: np.ndarray    # u32 [B]
    sp_thresh: np.ndarray  # u32 [B]
    kA: np.ndarray         # i32 [B, 5, 5] (motion blur)
    kB: np.ndarray         # i32 [B, 5, 5] (Gaussian blur)
    masks: np.ndarray      # u8 [B, mh, mw], 1 = keep
    luts: np.ndarray       # u8 [B, 3, 256]
    beta_tab: np.ndarray   # u8 [256]
    params: list = field(default_factory=list)  # the sampled choices per crop (for inspection and tests)

    def desc(self):
        d = np.zeros(len(self.flags), DESC_DTYPE)
        d["flags"], d["sp_seed"], d["sp_thresh"] = self.flags, self.sp_seed, self.sp_thresh
        d["kA"] = self.kA.reshape(-1, 25)
        d["kB"] = self.kB.reshape(-1, 25)
        return d


def empty_batch(B, H, W, mh=None, mw=None):
    """flags = 0 for every crop, every descriptor at its identity."""
    mh = max(int(0.05 * H), 3) if mh is None else mh
    mw = max(int(0.05 * W), 3) if mw is None else mw
    return AugBatch(np.zeros(B, np.uint32), np.zeros(B, np.uint32), np.zeros(B, np.uint32),
                    np.tile(identity_kernel(), (B, 1, 1)), np.tile(identity_kernel(), (B, 1, 1)),
                    np.ones((B, mh, mw), np.uint8), np.tile(np.arange(256, dtype=np.uint8), (B, 3, 1)), beta_table(),
                    [dict(chain=False) for _ in range(B)])


class AugmentSampler:
    """Samples the chain above.  ``use_peper_salt`` / ``use_motion_blur`` as the reference's configs
    spell them (all train with both on)."""

    def __init__(self, use_peper_salt=True, use_motion_blur=True, rng: np.random.Generator | None = None):
        self.use_peper_salt, self.use_motion_blur = bool(use_peper_salt), bool(use_motion_blur)
        self.rng = rng if rng is not None else np.random.default_rng()

    def _per_channel(self, p, draw):
        """imgaug's per_channel=p: with probability p one draw per channel, else one shared draw."""
        pc = bool(self.rng.random() < p)
        return pc, (np.array([draw() for _ in range(3)]) if pc else np.repeat(draw(), 3))

    def sample(self, B, H, W):
        r = self.rng
        out = empty_batch(B, H, W)
        mh, mw = out.masks.shape[1:]
        for b in range(B):
            p = out.params[b]
            if not r.random() < CHAIN_P:
                continue
            p["chain"] = True
            flags = 0
            p["sp"] = self.use_peper_salt and bool(r.random() < 0.3)
            if p["sp"]:
                flags |= AUG_SP
                out.sp_seed[b] = r.integers(0, 1 << 32, dtype=np.uint64)
                out.sp_thresh[b] = int(SP_P * 2 ** 32)
            p["motion"] = self.use_motion_blur and bool(r.random() < 0.2)
            if p["motion"]:
                flags |= AUG_STENCIL_A
                p["angle"], p["direction"] = float(r.uniform(0.0, 360.0)), float(r.uniform(-1.0, 1.0))
                out.kA[b] = motion_kernel(p["angle"], p["direction"])
            p["dropout"] = bool(r.random() < 0.4)
            if p["dropout"]:
                flags |= AUG_DROPOUT
                out.masks[b] = r.random((mh, mw)) >= 0.1  # drop ~ Bernoulli(0.1)
            p["sigma"] = float(r.random())  # GaussianBlur(np.random.rand()): drawn when the chain is built
            p["gauss"] = bool(r.random() < 0.5)
            if p["gauss"] and p["sigma"] >= 1e-3:  # imgaug skips a blur below 1e-3
                flags |= AUG_STENCIL_B
                out.kB[b] = gaussian_kernel(p["sigma"])
            luts = []
            p["add"] = bool(r.random() < 0.5)
            if p["add"]:
                p["add_pc"], p["add_v"] = self._per_channel(0.3, lambda: int(r.integers(-20, 21)))
                luts.append(lut_add(p["add_v"]))
            p["invert"] = bool(r.random() < 0.4)
            if p["invert"]:
                p["invert_on"] = r.random(3) < 0.2
                luts.append(lut_invert(p["invert_on"]))
            p["mul"] = bool(r.random() < 0.5)
            if p["mul"]:
                p["mul_pc"], p["mul_m"] = self._per_channel(0.8, lambda: float(r.uniform(0.7, 1.4)))
                luts.append(lut_multiply(p["mul_m"]))
            p["mul2"] = bool(r.random() < 0.5)
            if p["mul2"]:
                p["mul2_m"] = float(r.uniform(0.7, 1.4))
                luts.append(lut_multiply(np.repeat(p["mul2_m"], 3)))
            p["contrast"] = bool(r.random() < 0.5)
            if p["contrast"]:
                p["contrast_pc"], p["alpha"] = self._per_channel(0.3, lambda: float(r.uniform(0.5, 2.0)))
                luts.append(lut_contrast(p["alpha"]))
            if luts:
                flags |= AUG_LUT
                out.luts[b] = compose_luts(luts)
            out.flags[b] = flags
        return out


def _pack(batch: AugBatch):
    """One host buffer for one H2D copy: (bytes, offsets of desc, masks, luts, beta_tab), 16-byte aligned."""
    parts = [batch.desc().view(np.uint8).ravel(), np.ascontiguousarray(batch.masks, np.uint8).ravel(),
             np.ascontiguousarray(batch.luts, np.uint8).ravel(), np.ascontiguousarray(batch.beta_tab, np.uint8).ravel()]
    offs, n = [], 0
    for a in parts:
        offs.append(n)
        n += (a.size + 15) // 16 * 16
    buf = np.zeros(n, np.uint8)
    for o, a in zip(offs, parts):
        buf[o:o + a.size] = a
    return buf, offs


def augment_images(images, img_index, batch: AugBatch, bbox=None, out=None, method=L.ZP_CROP_SQUARE):
    """``zp_augment_m``: images u8 [N, H, W, 3] (BGR, device), img_index int [B] (host or device int32),
    bbox None or int32 [B, 4] (host or device) -> u8 [B, H, W, 3].  With ``bbox`` only the tiles
    meeting each crop's copied region are written; the rest of ``out`` keeps its contents
    (uninitialised when ``out`` is not given).  ``method`` (``ZP_CROP_SQUARE`` / ``ZP_CROP_RECT``) is
    the crop method that will read ``bbox``: the squared box or the box clipped to the image."""
    if not (isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and images.is_cuda and images.dim() == 4
            and images.shape[3] == 3):
        raise ValueError("images: expected a uint8 CUDA tensor [N, H, W, 3]")
    images = images.contiguous()
    N, H, W, _ = images.shape
    dev = images.device
    B = len(batch.flags)
    if isinstance(img_index, torch.Tensor) and img_index.is_cuda:
        ii = img_index.to(torch.int32).contiguous()
    else:
        idx = np.asarray(img_index, dtype=np.int64).reshape(-1)
        if len(idx) == 0 or idx.min() < 0 or idx.max() >= N:
            raise ValueError("img_index out of range")
        ii = torch.from_numpy(idx.astype(np.int32)).to(dev)
    if ii.numel() != B:
        raise ValueError("img_index and the descriptors disagree on the batch size")
    mh, mw = batch.masks.shape[1:]
    if batch.masks.shape[0] != B or batch.luts.shape != (B, 3, 256) or batch.kA.shape != (B, 5, 5) or \
            batch.kB.shape != (B, 5, 5) or batch.beta_tab.shape != (256,):
        raise ValueError("descriptor arrays do not match the batch")
    bb = None
    if bbox is not None:
        bb = bbox if isinstance(bbox, torch.Tensor) and bbox.is_cuda else torch.as_tensor(np.asarray(bbox)).to(dev)
        bb = bb.to(torch.int32).reshape(B, 4).contiguous()
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    elif not (out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, H, W, 3)):
        raise ValueError("out: expected a contiguous uint8 CUDA tensor [B, H, W, 3]")
    buf, offs = _pack(batch)
    dbuf = torch.from_numpy(buf).to(dev)
    base = dbuf.data_ptr()
    L.call("zp_augment_m", images.data_ptr(), N, H, W, ii.data_ptr(), base + offs[0], base + offs[1], mh, mw,
           base + offs[2], base + offs[3], L.ptr(bb), B, out.data_ptr(), int(method), L.stream_ptr())
    dbuf.record_stream(torch.cuda.current_stream(dev))
    return out
