"""The decode's crop -> image map where a fused multiply-add would change it, on the device: full
decode (``zp_decode``, ``zp_decode_radix``) and ``Decoder(unique=True)`` at a ``bbox_size`` that is no
power of two and a negative box origin, so ``w / S * px`` is inexact and ``+ x0`` lands on an integer.
Expected values are numpy's ``(np.float64(w) / S * px + x0).astype(int)`` (a division, a multiply and
an add, each rounded) and tests/decode_unique_ref.py; every comparison is exact.

Shapes: 96 x 96 and 100 x 100 (9 and 10 tiles of 1024 pixels, the last one partial, HW % 4 == 0: the
16-byte path and the prefix over earlier tiles) and 33 x 31 (1023 pixels: the scalar path).  Crop 0 of
every call has every pixel on but one whole tile (where there are several) and one single pixel; crop 1
has a random mask and another box."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import decode_unique_ref as ref

pytestmark = pytest.mark.gpu

THR = np.float32(8.940696716308594e-08)
#        H    W   bbox_size  boxes of crop 0 and crop 1            px of crop 0 that separates fused from two-step
SHAPES = {"s96": (96, 96, 96, ((-1, -1, 4, 4), (7, -3, 50, 61)), 48),
          "s100": (100, 100, 100, ((-5, -5, 5, 5), (-20, 11, 333, 77)), 60),
          "tail": (33, 31, 37, ((-100, 50, 300, 250), (3, 4, 5, 6)), None)}
CODES = {"binary": (2, 3), "radix4": (4, 2)}  # class_base, steps
NAN_ROW = 5


def _map(w, S, p, x0):
    """numpy's own: f64 division, multiply, add, truncation"""
    return (np.float64(w) / S * p + x0).astype(int)


def _fused(w, S, p, x0):
    """what a contracted multiply-add truncates: the exact product of the rounded ratio, plus x0"""
    return math.trunc(Fraction(float(np.float64(w) / S)) * int(p) + x0)


def _masks(H, W, rng):
    m0 = np.ones(H * W, bool)
    if H * W > 2048:
        m0[1024:2048] = False  # one whole tile
    m0[H * W // 2 + 7] = False
    return np.stack([m0.reshape(H, W), rng.random((H, W)) < 0.6])


@pytest.fixture(scope="module")
def cases():
    """(shape, code) -> inputs and expected rows, computed once on the host"""
    out = {}
    for si, (sname, (H, W, S, boxes, sep)) in enumerate(SHAPES.items()):
        rng = np.random.default_rng(20261021 + si)
        masks = _masks(H, W, rng)
        if sep is not None:
            # not vacuous: a masked pixel of crop 0 whose fused value differs from the expected one
            x0, _, w, _ = boxes[0]
            ys, xs = np.nonzero(masks[0])
            diff = [int(p) for p in np.unique(xs) if _fused(w, S, p, x0) != int(_map(w, S, np.float64(p), x0))]
            assert sep in diff, (sname, diff)
        for cname, (d, steps) in CODES.items():
            if d == 2:
                logits = rng.standard_normal((2, steps, H, W)).astype(np.float32)
                digits = (logits > THR).astype(np.int64)
            else:
                logits = rng.standard_normal((2, steps * d, H, W)).astype(np.float32)
                digits = logits.reshape(2, steps, d, H, W).argmax(2)
            ids = np.zeros((2, H, W), np.int64)
            for i in range(steps):
                ids = ids * d + digits[:, i]
            lut = ref.make_lut(d ** steps, nan_rows=(NAN_ROW,))
            lut32 = ref.coarsen_lut(lut, 0)
            rows = []
            for b in range(2):
                ys, xs = np.nonzero(masks[b])
                x0, y0, w, h = boxes[b]
                xy = np.stack([_map(w, S, xs.astype(np.float64), x0), _map(h, S, ys.astype(np.float64), y0)], 1)
                xyz = lut32[ids[b][ys, xs]].copy()
                xyz[np.isnan(xyz).any(1)] = 0
                rows.append((xy, xyz))
            assert (ids[0][masks[0]] == NAN_ROW).any()
            out[sname, cname] = dict(masks=masks, logits=logits, ids=ids, lut=lut, lut32=lut32, rows=rows, d=d,
                                     boxes=np.asarray(boxes), S=S)
    return out


def _decoder(c):
    from zebrapose_amd.decode import Decoder
    return Decoder(c["lut"], device="cuda", class_base=c["d"])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("code", tuple(CODES))
@pytest.mark.parametrize("shape", tuple(SHAPES))
def test_full_decode(gpu, cases, shape, code):
    c = cases[shape, code]
    counts, xy, xyz, ids = _decoder(c)(_dev(ref.mask_to_logits(c["masks"])), _dev(c["logits"]), c["boxes"],
                                       bbox_size=c["S"], return_ids=True)
    np.testing.assert_array_equal(ids.cpu().numpy(), c["ids"])
    np.testing.assert_array_equal(counts.cpu().numpy(), c["masks"].reshape(2, -1).sum(1))
    for b, (want_xy, want_xyz) in enumerate(c["rows"]):
        n = len(want_xy)
        np.testing.assert_array_equal(xy[b, :n].cpu().numpy(), want_xy)
        assert xyz[b, :n].cpu().numpy().tobytes() == want_xyz.tobytes()


@pytest.mark.parametrize("code", tuple(CODES))
@pytest.mark.parametrize("shape", tuple(SHAPES))
def test_unique_decode(gpu, cases, shape, code):
    c = cases[shape, code]
    u = _decoder(c).unique(_dev(ref.mask_to_logits(c["masks"])), _dev(c["logits"]), c["boxes"], bbox_size=c["S"])
    np.testing.assert_array_equal(u.ids.cpu().numpy(), c["ids"])
    for b in range(2):
        want = ref.unique_crop(c["masks"][b], c["ids"][b], c["lut32"], c["boxes"][b], c["S"])
        n = int(u.counts[b])
        assert n == want.count
        np.testing.assert_array_equal(u.xy[b, :n].cpu().numpy(), want.xy)
        assert u.xyz[b, :n].cpu().numpy().tobytes() == want.xyz.tobytes()
        np.testing.assert_array_equal(u.mult[b, :n].cpu().numpy(), want.mult)
        assert u.mean_xy[b, :n].cpu().numpy().tobytes() == np.ascontiguousarray(want.mean).tobytes()
