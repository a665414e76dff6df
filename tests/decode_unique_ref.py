"""Numpy oracle of the unique 2D-3D correspondences (``zp_decode_unique``, ``Decoder(unique=True)``),
written from the rule, shared by tests/test_decode_unique_host.py and tests/test_gpu_decode_unique.py.

Per crop: the mask pixels are visited in row-major order and grouped by class id; groups keep the
order of their first pixel.  A group's 2D point is (sum x / n, sum y / n): the sums are exact
integers and each quotient is one correctly rounded f64 division.  The crop -> image map is
``int(w / S * mean_x + x0)``: an f64 division, a multiply, an add (each rounded on its own, no FMA)
and a truncation toward zero.  The 3D point is the LUT row of the id; a row with a NaN gives
(0, 0, 0) (the device's rule, as in the non-unique decode; the reference would pass the NaN on).
"""
from collections import namedtuple

import numpy as np

Unique = namedtuple("Unique", "count xy xyz mult mean ids_order")


def make_lut(n, nan_rows=()):
    """LUT by formula, f64 [n, 3]: row i = (i, 2 i + 0.5, -i / 3); nan_rows are set to NaN."""
    i = np.arange(n, dtype=np.float64)
    lut = np.stack([i, 2.0 * i + 0.5, -i / 3.0], 1)
    for r in nan_rows:
        lut[r] = np.nan
    return lut


def coarsen_lut(lut, ignore_bit):
    """generate_new_dict.py:4-33 as zp_lut_coarsen does it: f64 mean of the 2^k children (summed in
    order), then the cast to f32 the device LUT holds.  ignore_bit 0 is the plain cast, except that the
    sum's start at +0.0 turns a -0.0 entry (make_lut's row 0) into +0.0, as on the device."""
    lut = np.asarray(lut, np.float64)
    nch = 1 << ignore_bit
    s = np.zeros((lut.shape[0] // nch, 3))
    for c in range(nch):
        s = s + lut[c::nch]
    return (s / nch).astype(np.float32)


def group(mask, ids):
    """-> (ids in first-appearance order, n, sum x, sum y) as Python-int exact values"""
    H, W = mask.shape
    order, acc = [], {}
    for y in range(H):
        for x in range(W):
            if not mask[y, x]:
                continue
            k = int(ids[y, x])
            a = acc.get(k)
            if a is None:
                acc[k] = [1, x, y]
                order.append(k)
            else:
                a[0] += 1
                a[1] += x
                a[2] += y
    return order, [acc[k][0] for k in order], [acc[k][1] for k in order], [acc[k][2] for k in order]


def map_to_original(mean, bbox, bbox_size):
    """mapping_pixel_position_to_original_position on f64 points [n, 2] -> int64 [n, 2]"""
    mean = np.asarray(mean, np.float64).reshape(-1, 2)
    rx = np.float64(bbox[2]) / np.float64(bbox_size)
    ry = np.float64(bbox[3]) / np.float64(bbox_size)
    x = (rx * mean[:, 0]) + np.float64(bbox[0])  # numpy: two rounded operations
    y = (ry * mean[:, 1]) + np.float64(bbox[1])
    return np.stack([np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)], 1)


def unique_crop(mask, ids, lut, bbox, bbox_size, nan_to_zero=True):
    """mask bool [H, W], ids int [H, W], lut [n, 3] (any float dtype; rows are returned in it) ->
    Unique(count, xy int64 [n, 2], xyz [n, 3], mult int64 [n], mean f64 [n, 2], ids_order)"""
    order, n, sx, sy = group(np.asarray(mask, bool), np.asarray(ids))
    cnt = len(order)
    nn = np.asarray(n, np.float64)
    mean = np.stack([np.asarray(sx, np.float64) / nn, np.asarray(sy, np.float64) / nn], 1).reshape(cnt, 2)
    lut = np.asarray(lut)
    xyz = lut[np.asarray(order, np.int64)].reshape(cnt, 3).copy()
    if nan_to_zero:
        xyz[np.isnan(xyz).any(1)] = 0
    return Unique(cnt, map_to_original(mean, bbox, bbox_size), xyz, np.asarray(n, np.int64), mean,
                  np.asarray(order, np.int64))


def bits_to_logits(ids, nbits, rng=None):
    """ids [.., H, W] -> code logits f32 [.., nbits, H, W] (channel 0 = MSB) of magnitude 1 (or
    random in [0.5, 2) with rng), positive where the bit is set"""
    ids = np.asarray(ids, np.int64)
    bits = (ids[..., None, :, :] >> (nbits - 1 - np.arange(nbits))[:, None, None]) & 1
    mag = np.ones(bits.shape, np.float32) if rng is None else rng.uniform(0.5, 2.0, bits.shape).astype(np.float32)
    return np.where(bits > 0, mag, -mag).astype(np.float32)


def digits_to_logits(ids, steps, d, rng=None):
    """ids [.., H, W] -> d-ary code logits f32 [.., steps * d, H, W]: the digit's class has the
    largest logit of its step (digit_i = (id // d^(steps-1-i)) % d)"""
    ids = np.asarray(ids, np.int64)
    lead = ids.shape[:-2]
    H, W = ids.shape[-2:]
    out = (-np.ones(lead + (steps, d, H, W), np.float32) if rng is None
           else rng.uniform(-2.0, -0.5, lead + (steps, d, H, W)).astype(np.float32))
    for i in range(steps):
        dg = (ids // d ** (steps - 1 - i)) % d
        np.put_along_axis(out[..., i, :, :, :], dg[..., None, :, :], np.float32(1.0), axis=-3)
    return out.reshape(lead + (steps * d, H, W))


def mask_to_logits(mask):
    return np.where(np.asarray(mask, bool), np.float32(1.0), np.float32(-1.0)).astype(np.float32)[..., None, :, :]


# ---- the shared cases: name -> (mask bool [H, W], ids int [H, W] < 65536, bbox, bbox_size) ----------
# A group of 7 pixels with sum x = sum y = 216 under a 119-wide box at bbox_size 36, and one of 3
# pixels with sum x = 101 under a 108-wide box, found by a search on the CPU: fl(fl(w / 36) * fl(s / n))
# is an integer after the add of -100, while the exact product lies just below it -- a contracted FMA
# gives the integer below (and so does s * fl(1 / 7) for the 7-group).
NEAR7 = dict(xs=(35, 35, 34, 33, 30, 29, 20), ys=(20, 29, 30, 33, 34, 35, 35), bbox=(-100, -100, 119, 119), bbox_size=36,
             id=40001)
NEAR3 = dict(xs=(35, 34, 32), ys=(3, 17, 38), bbox=(-100, 7, 108, 53), bbox_size=36, id=40002)


def _plant(mask, ids, spec):
    for x, y in zip(spec["xs"], spec["ys"]):
        mask[y, x] = True
        ids[y, x] = spec["id"]


def cases():
    rng = np.random.default_rng(20261020)
    out = {}
    # two tiles, HW % 4 == 0; class 5 starts in tile 0 (pixel 3) and has its other pixels in tile 1
    H, W = 40, 36
    mask = rng.random((H, W)) < 0.7
    ids = rng.integers(100, 300, (H, W))
    for p in (3, 1030, 1100, 1439):
        mask.flat[p], ids.flat[p] = True, 5
    out["two_tiles"] = (mask, ids, (13, 7, 37, 53), 128)
    # 1073 pixels: the scalar tail path, two tiles
    H, W = 37, 29
    out["tail"] = (rng.random((H, W)) < 0.6, rng.integers(0, 60, (H, W)) * 1000, (-100, 50, 300, 250), 37)
    out["single_tile"] = (rng.random((8, 8)) < 0.8, rng.integers(0, 12, (8, 8)) + 65524, (5, 5, 64, 64), 8)
    H, W = 40, 36
    out["empty"] = (np.zeros((H, W), bool), rng.integers(0, 65536, (H, W)), (13, 7, 37, 53), 128)
    out["one_class"] = (np.ones((H, W), bool), np.full((H, W), 777), (13, 7, 37, 53), 128)
    out["distinct"] = (rng.random((H, W)) < 0.8, rng.permutation(65536)[:H * W].reshape(H, W), (13, 7, 37, 53), 128)
    # groups of 3 and 7 pixels (non-terminating means) and the two near-integer groups
    mask = np.zeros((H, W), bool)
    ids = np.zeros((H, W), np.int64)
    free = rng.permutation(H * W)
    k = 0
    for g in range(60):
        n = 3 if g % 2 else 7
        mask.flat[free[k:k + n]], ids.flat[free[k:k + n]] = True, 1000 + g
        k += n
    m7, i7 = mask.copy(), ids.copy()
    _plant(m7, i7, NEAR7)
    out["near7"] = (m7, i7, NEAR7["bbox"], NEAR7["bbox_size"])
    m3, i3 = mask.copy(), ids.copy()
    _plant(m3, i3, NEAR3)
    out["near3"] = (m3, i3, NEAR3["bbox"], NEAR3["bbox_size"])
    # 16 ids that agree in their low 12 bits, and 16 more that agree in their high bits
    pool = np.concatenate([np.arange(16) * 4096, np.arange(16) + 4096])
    out["table_stress"] = (rng.random((H, W)) < 0.9, pool[rng.integers(0, 32, (H, W))], (13, 7, 37, 53), 128)
    # exactly 5 and exactly 6 classes over more than 100 pixels
    for n in (5, 6):
        mask = rng.random((H, W)) < 0.5
        out[f"classes{n}"] = (mask, (np.arange(n) * 9973 + 17)[rng.integers(0, n, (H, W))], (260, 180, 128, 128), 128)
    return out


LUT_CLASSES = 65536
