"""Reference of zp_pack_weight / zp_pack_weight_multi (include/zp.h), stated from the header alone.

The map:  dst[r][t * cstride + c] = src[r][c][ky[t]][kx[t]]        (transposed == 0, src [d0 = rows][d1 = chans])
                                  = src[c][r][ky[t]][kx[t]]        (transposed == 1, src [d0 = chans][d1 = rows])
for r < rows, t < ntaps, c < chans; every other element of dst [rows_pad][k_pad] is zero.

The stored forms (zp.h ZP_F32 .. ZP_F32H2, csrc/zp_common.h):
  ZP_F32    the f32 itself
  ZP_BF16   round to nearest even onto bf16
  ZP_F16    IEEE fp16, round to nearest even (65520 and above become infinity)
  ZP_F32X3  three bf16 planes: hi = bf16(v), mid = bf16(v - hi), lo = bf16((v - hi) - mid), the differences
            in f32; v == hi + mid + lo exactly for finite v (-0 joins to +0); a non-finite v keeps mid = lo = 0
  ZP_F32H2  two fp16 planes: hi = fp16(v), lo = fp16((v - hi) * 2^11), the difference and the product in f32;
            v ~ hi + lo * 2^-11 to 2^-23 |v| for |v| >= 2^-13, 2^-36 absolute below; lo = 0 when hi is
            not finite.  A finite WEIGHT with |w| >= 31.984375 (= 65504 / 2^11) is out of range for the conv
            that consumes it: packing one raises the range flag (zp_split_range_flag).  Padding is zero and
            cannot raise it; no other type raises it.
Planes are [NPL][rows_pad][k_pad] words, plane p one plane size after plane p - 1."""
from __future__ import annotations

import numpy as np

F32, BF16, F16, X3, H2 = 0, 1, 2, 3, 4       # include/zp.h ZP_F32 .. ZP_F32H2
DTYPES = {"f32": F32, "bf16": BF16, "f16": F16, "x3": X3, "h2": H2}
H2_WEIGHT_LIMIT = np.float32(31.984375)


def bf16_bits(v):
    """f32 -> bf16 words, round to nearest even (finite values and infinities)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(w):
    return (np.asarray(w, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f16_bits(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float32).astype(np.float16).view(np.uint16)


def f16_value(w):
    return np.asarray(w, np.uint16).view(np.float16).astype(np.float32)


def split3(v):
    """[3][...] bf16 words of ZP_F32X3"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        h = bf16_bits(v)
        r1 = v - bf16_value(h)
        m = bf16_bits(r1)
        lo = bf16_bits(r1 - bf16_value(m))
    fin = np.isfinite(v)
    return np.stack([h, np.where(fin, m, 0).astype(np.uint16), np.where(fin, lo, 0).astype(np.uint16)])


def join3(w):
    p = bf16_value(w)
    return (p[0] + p[1]) + p[2]


def split2(v):
    """[2][...] fp16 words of ZP_F32H2"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        h = f16_bits(v)
        hv = f16_value(h)
        lo = f16_bits((v - hv) * np.float32(2048.0))
    return np.stack([h, np.where(np.isfinite(hv), lo, 0).astype(np.uint16)])


def join2(w):
    """fma(lo, 2^-11, hi): both terms and their sum are exact in f64, so one rounding"""
    hi, lo = f16_value(w[0]).astype(np.float64), f16_value(w[1]).astype(np.float64)
    return (lo * 2.0 ** -11 + hi).astype(np.float32)


def h2_weight_out_of_range(v):
    a = np.abs(np.asarray(v, np.float32))
    return np.isfinite(a) & (a >= H2_WEIGHT_LIMIT)


def pack(src, transposed, taps, cstride, rows_pad, k_pad):
    """dst [rows_pad][k_pad] f32 of the map above.  src [d0][d1][kh][kw]; taps [(ky, kx)]"""
    src = np.asarray(src, np.float32)
    d0, d1, kh, kw = src.shape
    rows, chans = (d1, d0) if transposed else (d0, d1)
    assert cstride >= chans and rows_pad >= rows and len(taps) * cstride <= k_pad
    dst = np.zeros((rows_pad, k_pad), np.float32)
    for r in range(rows):
        for t, (ky, kx) in enumerate(taps):
            assert 0 <= ky < kh and 0 <= kx < kw
            dst[r, t * cstride:t * cstride + chans] = src[:, r, ky, kx] if transposed else src[r, :, ky, kx]
    return dst


def store(dst, dtype):
    """the words dst is stored as: uint32 [R][K] (ZP_F32), uint16 [R][K] (16-bit types), uint16 [NPL][R][K]"""
    dst = np.asarray(dst, np.float32)
    if dtype == F32:
        return dst.view(np.uint32).copy()
    if dtype == BF16:
        return bf16_bits(dst)
    if dtype == F16:
        return f16_bits(dst)
    return split3(dst) if dtype == X3 else split2(dst)


def raises_flag(dst, dtype):
    """does packing dst (the f32 matrix of pack()) in `dtype` raise the range flag"""
    return bool(dtype == H2 and h2_weight_out_of_range(dst).any())
