"""numpy restatement of zp_mask_bbox and zp_composite (include/zp.h): the executable definition of
their semantics -- replace_bg / get_bg_image of GDR_Net_Augmentation.py:78-153 with OpenCV's
fixed-point INTER_LINEAR for u8 (the arithmetic of oracle/crop_ref.py, here with the sampling scale
1 / f that cv2.resize uses when it is given fx = fy = f).  Integer steps are exact and the few real
steps are single IEEE operations in the device code's order (csrc/zp_shade.hip), so the kernels must
reproduce the outputs bit for bit.  Reads nothing outside the repository.
"""
from __future__ import annotations

import numpy as np


def mask_bbox(mask):
    """mask u8 [B, H, W] -> i32 [B, 4] = (r1, c1, r2, c2), inclusive; an empty mask gives (0, 0, -1, -1)."""
    out = np.zeros((len(mask), 4), np.int32)
    for b, m in enumerate(np.asarray(mask)):
        ys, xs = np.nonzero(m)
        out[b] = (ys.min(), xs.min(), ys.max(), xs.max()) if len(ys) else (0, 0, -1, -1)
    return out


def _cut(a, b, u):
    """int(a + (b - a) u), kept inside [0, 65536]."""
    v = np.float64(a) + (np.float64(b) - np.float64(a)) * np.float64(u)
    if not v >= 0:
        return 0
    return 65536 if v > 65536 else int(v)


def truncate(mask, bbox, rnd, u):
    """One mask u8 [H, W] -> bool [H, W] after replace_bg's truncation (:128-149)."""
    m = np.asarray(mask) != 0
    r1, c1, r2, c2 = (int(v) for v in bbox)
    if r2 < 0 or c2 < 0 or rnd < 0:
        return m
    m = m.copy()
    mid_r, mid_c = 0.5 * float(r1 + r2), 0.5 * float(c1 + c2)
    if rnd < 0.2:
        m[:_cut(r1, mid_r, u), :] = False
    elif rnd < 0.4:
        m[_cut(mid_r, r2, u):, :] = False
    elif rnd < 0.6:
        m[:, :_cut(c1, mid_c, u)] = False
    elif rnd < 0.8:
        m[:, _cut(mid_c, c2, u):] = False
    return m


def lin_taps(d, n, scale):
    """INTER_LINEAR taps of d destination samples over n source samples at the given sampling scale:
    (s0, s1 int64 [d], a int64 [d, 2])."""
    i = np.arange(d, dtype=np.float64)
    f = ((i + 0.5) * np.float64(scale) - 0.5).astype(np.float32)
    fl = np.floor(f)
    lo, hi = fl < 0, fl >= np.float32(n - 1)
    s0 = np.where(lo, 0, np.where(hi, n - 1, fl)).astype(np.int64)
    fr = np.where(lo | hi, np.float32(0), f - fl).astype(np.float32)
    a0 = np.rint((np.float32(1) - fr) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(fr * np.float32(2048)).astype(np.int64)
    return s0, np.minimum(s0 + 1, n - 1), np.stack([a0, a1], 1)


def resize_linear_u8(src, ow, oh, f):
    """cv2.resize(src, None, fx=f, fy=f, interpolation=cv2.INTER_LINEAR) for u8 [h, w, C], whose
    dsize is (ow, oh) = rint(size * f)."""
    h, w = src.shape[:2]
    if (ow, oh) == (w, h):
        return src.copy()
    r = src.astype(np.int64)
    scale = 1.0 / np.float64(f)
    if abs(scale - 2.0) < np.finfo(np.float64).eps:  # INTER_AREA fast path
        out = np.zeros((oh, ow) + src.shape[2:], np.uint8)
        for y in range(oh):
            for x in range(ow):
                if 2 * y >= h or 2 * x >= w:
                    continue
                blk = r[2 * y:2 * y + 2, 2 * x:2 * x + 2].reshape(-1, *src.shape[2:])
                s = blk.sum(0)
                if len(blk) == 4:
                    out[y, x] = (s + 2) >> 2
                elif len(blk) == 1:
                    out[y, x] = s
                else:  # two samples: half to even
                    hv = s >> 1
                    out[y, x] = hv + ((s & 1) & (hv & 1))
        return out
    xs0, xs1, xa = lin_taps(ow, w, scale)
    ys0, ys1, ya = lin_taps(oh, h, scale)
    hz = r[:, xs0] * xa[:, 0][None, :, None] + r[:, xs1] * xa[:, 1][None, :, None]
    v = (((hz[ys0] >> 4) * ya[:, 0][:, None, None]) >> 16) + (((hz[ys1] >> 4) * ya[:, 1][:, None, None]) >> 16)
    return np.clip((v + 2) >> 2, 0, 255).astype(np.uint8)


def background(bg, geo, f, H, W):
    """get_bg_image after the read: the top-left crop of bg u8 [Hb, Wb, 3], resized, pasted at the
    top-left of a zero H x W image; what falls outside is dropped."""
    cw, ch, ow, oh = (int(v) for v in geo)
    res = resize_linear_u8(bg[:ch, :cw], ow, oh, f)
    out = np.zeros((H, W, 3), np.uint8)
    out[:min(oh, H), :min(ow, W)] = res[:H, :W]
    return out


def composite(fg, mask, bgs, bg_index, bg_geo, bg_f, trunc):
    """fg u8 [B, H, W, 3], mask u8 [B, H, W], bgs u8 [n_bg, Hb, Wb, 3], bg_index [B], bg_geo [B, 4],
    bg_f [B], trunc [B, 2] -> (image u8 [B, H, W, 3], truncated mask u8 [B, H, W] of 255 / 0)."""
    B, H, W = mask.shape
    bbox = mask_bbox(mask)
    img, mo = np.empty_like(fg), np.empty((B, H, W), np.uint8)
    for b in range(B):
        m = truncate(mask[b], bbox[b], trunc[b][0], trunc[b][1])
        bgi = background(bgs[int(bg_index[b])], bg_geo[b], bg_f[b], H, W)
        img[b] = np.where(m[..., None], fg[b], bgi)
        mo[b] = np.where(m, 255, 0)
    return img, mo
