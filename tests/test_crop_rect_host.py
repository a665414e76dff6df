"""The rectangular crop (``resize_method = crop_resize``) without a GPU: the numpy restatement
tests/crop_rect_ref.py tied to the pinned square oracle (oracle/crop_ref.py) where the two must
agree, its fast-path rules, CropPipeline's host box arithmetic under ``"crop_resize"`` and the
refusals (an unknown crop method at the C entry points, the warp-affine method in Python)."""
import ctypes

import numpy as np
import pytest

from oracle import crop_ref as C
from tests import crop_rect_ref as R

H, W, S = 48, 64, 16


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    gt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = rng.integers(0, 2, (H, W), dtype=np.uint8) * 255
    ent = rng.integers(0, 256, (H, W), dtype=np.uint8)
    return img, gt, mask, ent


def _unnorm(x):
    """Normalised f32 [3, S, S] -> the u8 crop [S, S, 3] it was made from."""
    v = np.rint((x.transpose(1, 2, 0) * C.STD + C.MEAN) * 255)
    return v.astype(np.uint8)


def test_same_size_is_the_slice(scene):
    img, gt, mask, ent = scene
    box = [9, 7, S, S]
    x = R.crop_image_rect(img, box, S)
    want = ((img[7:7 + S, 9:9 + S].astype(np.float32) / np.float32(255) - C.MEAN) / C.STD).transpose(2, 0, 1)
    np.testing.assert_array_equal(x, want.astype(np.float32))
    np.testing.assert_array_equal(_unnorm(x), img[7:7 + S, 9:9 + S])
    code, m, e = R.crop_gt_rect(gt, mask, ent, box, S, 16)
    g = gt[7:7 + S, 9:9 + S].astype(np.int64)
    np.testing.assert_array_equal(code[15], g[:, :, 2] & 1)
    np.testing.assert_array_equal(code[0], (g[:, :, 1] >> 7) & 1)
    np.testing.assert_array_equal(m, (mask[7:7 + S, 9:9 + S] / 255.).astype(np.float32))
    np.testing.assert_array_equal(e, (ent[7:7 + S, 9:9 + S] / 255.).astype(np.float32))


@pytest.mark.parametrize("side", [5, 37, 2 * S], ids=["upscale", "fractional_downscale", "exact_2x"])
def test_square_box_inside_matches_square_oracle(scene, side):
    """bw == bh inside the image: square_roi's int() truncation lands on the slice itself, so the two
    restatements must agree bit for bit, image and GT (the GT also at its own exact 2x, S = side / 2
    where that is whole)."""
    img, gt, mask, ent = scene
    box = [6, 4, side, side]
    np.testing.assert_array_equal(C.square_roi(img, box), img[4:4 + side, 6:6 + side])
    np.testing.assert_array_equal(R.crop_image_rect(img, box, S), C.crop_image(img, box, S))
    for Sg in (8, S):
        for got, want in zip(R.crop_gt_rect(gt, mask, ent, box, Sg, 16), C.crop_gt(gt, mask, ent, box, Sg, 16)):
            np.testing.assert_array_equal(got, want)


def _two_pass(roi, S):
    """The general INTER_LINEAR path pixel by pixel (the test's own loops over _lin_taps)."""
    sh, sw = roi.shape[:2]
    xs0, xs1, xa, xedge = C._lin_taps(S, sw)
    ys0, ys1, ya, _ = C._lin_taps(S, sh)
    out = np.zeros((S, S, roi.shape[2]), np.uint8)
    for dy in range(S):
        for dx in range(S):
            for c in range(roi.shape[2]):
                h = []
                for sy in (ys0[dy], ys1[dy]):
                    p0, p1 = int(roi[sy, xs0[dx], c]), int(roi[sy, xs1[dx], c])
                    h.append(p0 * 2048 if xedge[dx] else p0 * int(xa[dx, 0]) + p1 * int(xa[dx, 1]))
                r = (((h[0] >> 4) * int(ya[dy, 0])) >> 16) + (((h[1] >> 4) * int(ya[dy, 1])) >> 16)
                out[dy, dx, c] = min(255, max(0, (r + 2) >> 2))
    return out


def _box_filter(roi):
    r = roi.astype(np.int64)
    return ((r[0::2, 0::2] + r[0::2, 1::2] + r[1::2, 0::2] + r[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def test_box_filter_needs_both_axes_at_2x(scene):
    img = scene[0]
    both = img[5:5 + 2 * S, 3:3 + 2 * S]
    np.testing.assert_array_equal(R.resize_linear_u8(both, S), _box_filter(both))
    for roi in (img[5:5 + 2 * S - 1, 3:3 + 2 * S], img[5:5 + 2 * S, 3:3 + 2 * S - 1]):  # 2S x (2S - 1) both ways
        got = R.resize_linear_u8(roi, S)
        np.testing.assert_array_equal(got, _two_pass(roi, S))
        assert (got != _box_filter(both)).any()
    # and the crop takes the same route
    np.testing.assert_array_equal(_unnorm(R.crop_image_rect(img, [3, 5, 2 * S, 2 * S - 1], S)),
                                  _two_pass(img[5:5 + 2 * S - 1, 3:3 + 2 * S], S))


def test_identity_in_x_only_has_unit_taps(scene):
    img = scene[0]
    roi = img[2:42, 11:11 + S]  # sw == S, sh == 40: the general path with x coefficients (2048, 0)
    _, _, xa, _ = C._lin_taps(S, S)
    assert (xa[:, 0] == 2048).all() and (xa[:, 1] == 0).all()
    np.testing.assert_array_equal(R.resize_linear_u8(roi, S), _two_pass(roi, S))


def test_empty_slices_are_the_zero_crop(scene):
    img, gt, mask, ent = scene
    for box in ([70, 10, 20, 20], [-30, 5, 20, 20], [5, 50, 9, 9], [10, 10, 0, 12], [10, 10, 12, 0], [-1, -1, -1, -1]):
        assert R.rect_region(box, H, W) is None
        assert not R.crop_image_rect(img, box, S).any()
        assert not any(a.any() for a in R.crop_gt_rect(gt, mask, ent, box, 8, 16))
    assert R.rect_region([-5, 40, 30, 30], H, W) == (0, 40, 25, 48)


def test_pipeline_boxes_under_crop_resize():
    from zebrapose_amd.crop import CropPipeline, aug_Bbox, get_final_Bbox, padding_Bbox
    cp = CropPipeline(S, 8, resize_method="crop_resize")
    raw = np.array([[10, 12, 30, 14], [-8, -6, 30, 20], [50, 30, 30, 40], [-1, -1, -1, -1], [200, 10, 20, 20],
                    [-90, 5, 20, 20], [10, 10, 0, 5]])
    pad, fin = cp.boxes(raw, W, H)
    assert pad.dtype == np.int32 and fin.dtype == np.int64
    for i, bb in enumerate(raw):
        if i >= 3:  # no detection, wholly outside (right, left), zero width: handled like the -1 box
            assert not pad[i].any() and not fin[i].any(), i
            continue
        p = padding_Bbox(bb, 1.5)
        np.testing.assert_array_equal(pad[i], p)
        np.testing.assert_array_equal(fin[i], get_final_Bbox(p, "crop_resize", W, H))
        x1, y1, x2, y2 = R.rect_region(p, H, W)
        np.testing.assert_array_equal(fin[i], [x1, y1, x2 - x1, y2 - y1])
    assert (fin[1][:2] == 0).all() and fin[2][0] + fin[2][2] == W and fin[2][1] + fin[2][3] == H  # clipped
    # training branch: the jittered boxes, drawn from the generator in order
    tr = raw[[0, 1, 2, 4]]
    aug, fin = cp.train_boxes(tr, W, H, np.random.default_rng(7))
    rng = np.random.default_rng(7)
    for i, bb in enumerate(tr):
        a = aug_Bbox(bb, 1.5, rng)
        if R.rect_region(a, H, W) is None:
            assert i == 3 and not aug[i].any() and not fin[i].any()
            continue
        np.testing.assert_array_equal(aug[i], a)
        np.testing.assert_array_equal(fin[i], get_final_Bbox(a, "crop_resize", W, H))
    assert not aug[3].any()
    # the default method keeps the squared final box
    pad0, fin0 = CropPipeline(S, 8).boxes(raw[:1], W, H)
    np.testing.assert_array_equal(fin0[0], get_final_Bbox(pad0[0], "crop_square_resize", W, H))
    assert fin0[0][2] == fin0[0][3]


def test_resize_method_refusals():
    from zebrapose_amd.crop import CropPipeline
    assert CropPipeline().resize_method == "crop_square_resize"
    assert CropPipeline(resize_method="crop_resize").resize_method == "crop_resize"
    with pytest.raises(NotImplementedError, match="crop_resize_by_warp_affine"):
        CropPipeline(resize_method="crop_resize_by_warp_affine")
    with pytest.raises(NotImplementedError):
        CropPipeline(resize_method="crop_round_resize")


def test_unknown_crop_method_is_refused_without_gpu():
    """The method check runs on the host before any launch (no GPU needed)."""
    from zebrapose_amd import _lib
    assert (_lib.ZP_CROP_SQUARE, _lib.ZP_CROP_RECT) == (0, 1)
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)
    for method in (2, -1, 7):
        rc = _lib.lib.zp_crop_image_m(p, 1, 4, 4, p, p, 1, 4, p, method, None)
        assert rc == 1 and b"zp_crop_image_m" in _lib.lib.zp_last_error() and b"method" in _lib.lib.zp_last_error()
        rc = _lib.lib.zp_crop_gt_m(p, p, p, 1, 4, 4, p, p, 1, 4, 16, p, p, p, method, None)
        assert rc == 1 and b"zp_crop_gt_m" in _lib.lib.zp_last_error() and b"method" in _lib.lib.zp_last_error()
        rc = _lib.lib.zp_augment_m(p, 1, 8, 8, p, p, p, 3, 3, p, p, p, 1, p, method, None)
        assert rc == 1 and b"zp_augment_m" in _lib.lib.zp_last_error() and b"method" in _lib.lib.zp_last_error()
