"""Reference of zp_maxpool3s2 / zp_maxpool3s2_bwd (include/zp.h; csrc/zp_pool.hip): the 3x3, stride 2,
padding 1 max pool of an NHWC tensor, by torch's CPU rule.

forward   per window the maximum by `v > max || isnan(v)` over the in-bounds taps in (ky, kx) order, the
          maximum starting at -inf and the index at the window's first in-bounds tap.  So the first of equal
          values wins (+0 and -0 are equal), a NaN takes over and only a later NaN replaces it, and a window
          of -inf alone keeps -inf and points to its first in-bounds tap.
backward  dx[index] receives each window's dy, added in f32 in (oy, ox) order starting from zero, then the
          existing dx when accumulating; one rounding to the storage type at the end.

Values are f32 arrays holding values of the storage type; tests/test_pool_ref_host.py holds both functions
to F.max_pool2d and its backward."""
from __future__ import annotations

import numpy as np


def out_size(n):
    return (n - 1) // 2 + 1


def forward(x):
    """x [B][IH][IW][C] f32 -> (y [B][OH][OW][C] f32, index [B][OH][OW][C] = iy * IW + ix of the winner)"""
    x = np.asarray(x, np.float32)
    B, IH, IW, C = x.shape
    OH, OW = out_size(IH), out_size(IW)
    oy, ox = np.meshgrid(np.arange(OH), np.arange(OW), indexing="ij")
    m = np.full((B, OH, OW, C), -np.inf, np.float32)
    first = np.maximum(oy * 2 - 1, 0) * IW + np.maximum(ox * 2 - 1, 0)
    idx = np.broadcast_to(first[None, :, :, None], m.shape).astype(np.int64).copy()
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy * 2 - 1 + ky, ox * 2 - 1 + kx
            ok = (iy >= 0) & (iy < IH) & (ix >= 0) & (ix < IW)
            v = x[:, np.clip(iy, 0, IH - 1), np.clip(ix, 0, IW - 1)]
            with np.errstate(invalid="ignore"):
                take = ok[None, :, :, None] & ((v > m) | np.isnan(v))
            m = np.where(take, v, m)
            idx = np.where(take, (iy * IW + ix)[None, :, :, None], idx)
    return m, idx


def backward(x, dy, dx=None):
    """the f32 sums before the store's rounding: [B][IH][IW][C].  dx: the existing values when accumulating"""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    B, IH, IW, C = x.shape
    _, idx = forward(x)
    OH, OW = idx.shape[1:3]
    acc = np.zeros((B, IH * IW, C), np.float32)
    b, c = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        for oy in range(OH):
            for ox in range(OW):
                acc[b, idx[:, oy, ox, :], c] += dy[:, oy, ox, :]  # (b, c) pairs are distinct: no lost update
        if dx is not None:
            acc = acc + np.asarray(dx, np.float32).reshape(B, IH * IW, C)
    return acc.reshape(B, IH, IW, C)


def edge_input(B, IH, IW, C, seed):
    """x [B][IH][IW][C] f32, every value on the bf16 and fp16 grids: small rounded integers (ties in most
    windows); channel 0 all zeros of alternating sign; a lone NaN; a NaN with a larger value after it; +inf;
    windows of -inf alone at the corner and (where the extents allow) in the interior"""
    rng = np.random.default_rng(seed)
    x = np.round(rng.standard_normal((B, IH, IW, C)) * 3).astype(np.float32)
    sign = (np.add.outer(np.arange(IH), np.arange(IW)) + seed) % 2
    x[..., 0] = np.where(sign, np.float32(0.0), np.float32(-0.0))[None]
    if C > 1:
        x[0, IH // 2, IW // 2, 1] = np.nan                      # alone
        x[B - 1, 0, 0, C - 1] = np.nan                          # then a larger value in the same windows
        x[B - 1, min(1, IH - 1), min(1, IW - 1), C - 1] = 100.0
        x[0, IH - 1, IW - 1, 2 % C] = np.inf
    if C > 3:
        x[:, :2, :2, 3] = -np.inf                               # window (0, 0) holds nothing else
        if IH >= 5 and IW >= 5:
            x[:, 1:4, 1:4, C - 2] = -np.inf                     # window (1, 1): rows and columns 1..3
        x[B - 1, :, :, C - 3] = -np.inf                         # every window of this channel
    return x
