"""The rectangular crop (``resize_method = crop_resize``: zp_crop_image_m / zp_crop_gt_m / zp_augment_m
with ZP_CROP_RECT, through CropPipeline(resize_method="crop_resize")) against the numpy restatement
tests/crop_rect_ref.py, bit-exact throughout: wide and tall boxes, boxes clipped at every border,
every route of the resize (copy, 2 x 2 box filter, the general two-pass path where only one axis is
at 2x or at 1x), one-pixel-wide ROIs, an upscale, empty ROIs, d-ary digits, a realistic size, the
training branch, and the crop -> decode round trip.  The square path is pinned unchanged beside it.
Parity against OpenCV itself is unpinned (cv2 absent; tests/crop_rect_ref.py's header)."""
import numpy as np
import pytest
import torch

from oracle import crop_ref as C
from tests import aug_ref as A
from tests import crop_rect_ref as R

pytestmark = pytest.mark.gpu

H, W, S_IMG, S_GT = 48, 64, 16, 8
BOXES = {
    "wide": [10, 12, 40, 14], "tall": [20, 3, 11, 41],
    "clip_left": [-7, 10, 25, 20], "clip_top": [12, -9, 30, 22], "clip_right": [50, 8, 30, 25],
    "clip_bottom": [9, 30, 22, 40], "clip_left_top": [-5, -6, 30, 28], "clip_right_bottom": [45, 35, 40, 40],
    "whole_image": [-3, -3, 80, 60],
    "copy_16x16": [7, 9, 16, 16], "box_32x32": [3, 5, 32, 32], "no_box_32x31": [3, 5, 32, 31],
    "no_box_31x32": [3, 5, 31, 32], "identity_x_16x40": [11, 2, 16, 40],
    "roi_1x9": [30, 20, 1, 9], "roi_9x1": [30, 20, 9, 1], "roi_1x1": [63, 47, 5, 5], "upscale_5x7": [40, 30, 5, 7],
    "gt_copy_8x8": [5, 5, 8, 8], "gt_2x_8x16": [5, 5, 8, 16],
    "outside_right": [70, 10, 20, 20], "outside_left": [-30, 5, 20, 20], "outside_below": [5, 48, 9, 9],
    "zero_width": [10, 10, 0, 12], "zero_height": [10, 10, 12, 0], "no_detection": [-1, -1, -1, -1],
}
EMPTY = ("outside_right", "outside_left", "outside_below", "zero_width", "zero_height", "no_detection")


def _stacks(seed, N, h, w):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (N, h, w, 3), dtype=np.uint8)
    gts = rng.integers(0, 256, (N, h, w, 3), dtype=np.uint8)
    masks = rng.integers(0, 2, (N, h, w), dtype=np.uint8) * 255
    ent = rng.integers(0, 256, (N, h, w), dtype=np.uint8)
    return imgs, gts, masks, ent


@pytest.fixture(scope="module")
def scene():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    host = _stacks(17, 2, H, W)
    return host, [torch.from_numpy(a).cuda() for a in host]


def _check(out, host, idx, boxes, S_img, S_gt, L=16):
    imgs, gts, masks, ent = host
    x, code, m, e = (out[k].cpu().numpy() for k in ("x", "code", "mask", "entire_mask"))
    for b, bb in enumerate(boxes):
        i = idx[b]
        np.testing.assert_array_equal(x[b], R.crop_image_rect(imgs[i], bb, S_img), err_msg=f"image crop {b} {bb}")
        rc, rm, re = R.crop_gt_rect(gts[i], masks[i], ent[i], bb, S_gt, L)
        np.testing.assert_array_equal(code[b], rc, err_msg=f"code {b} {bb}")
        np.testing.assert_array_equal(m[b], rm, err_msg=f"mask {b} {bb}")
        np.testing.assert_array_equal(e[b], re, err_msg=f"entire {b} {bb}")
    return x, code, m, e


@pytest.mark.parametrize("name", list(BOXES))
def test_rect_crop_matches_restatement(gpu, scene, name):
    from zebrapose_amd.crop import CropPipeline
    host, dev = scene
    bb = np.array([BOXES[name]], np.int32)
    reg = R.rect_region(bb[0], H, W)
    assert (reg is None) == (name in EMPTY)
    cp = CropPipeline(S_IMG, S_GT, resize_method="crop_resize")
    x, code, m, e = _check(cp(dev[0], [1], bb, dev[1], dev[2], dev[3]), host, [1], bb, S_IMG, S_GT)
    if reg is None:
        assert not x.any() and not code.any() and not m.any() and not e.any()
    else:
        assert x.std() > 0.1  # a crop of noise, not a constant
        if name.endswith(("32x31", "31x32")):  # and not the box filter's result
            sq = C.cv_resize_linear_u8(host[0][1][5:37, 3:35], S_IMG)
            assert (x[0] != ((sq.astype(np.float32) / np.float32(255) - C.MEAN) / C.STD).transpose(2, 0, 1)).any()


def test_realistic_size_mixed_boxes(gpu):
    from zebrapose_amd.crop import CropPipeline
    host = _stacks(23, 2, 480, 640)
    dev = [torch.from_numpy(a).cuda() for a in host]
    bb = np.array([[100, 80, 200, 150], [-40, 300, 300, 260], [128, 64, 512, 256], [500, -20, 180, 333]], np.int32)
    idx = [1, 0, 1, 1]
    cp = CropPipeline(resize_method="crop_resize")
    out = cp(dev[0], idx, bb, dev[1], dev[2], dev[3])
    assert out["x"].shape == (4, 3, 256, 256) and out["code"].shape == (4, 16, 128, 128)
    _check(out, host, idx, bb, 256, 128)


@pytest.mark.parametrize("base", [4, 256])
def test_dary_digits_through_rect_crop(gpu, scene, base):
    from zebrapose_amd.crop import CropPipeline
    host, dev = scene
    names = ["wide", "clip_left_top", "upscale_5x7", "outside_right"]
    bb = np.array([BOXES[n] for n in names], np.int32)
    idx = [0, 1, 1, 0]
    cp = CropPipeline(S_IMG, S_GT, class_base=base, resize_method="crop_resize")
    code = cp(dev[0], idx, bb, dev[1])["code"].cpu().numpy()
    s = base.bit_length() - 1
    n = 16 // s
    assert code.shape == (4, n, S_GT, S_GT)
    for b in range(4):
        cid = R.crop_ids_rect(host[1][idx[b]], bb[b], S_GT) & 0xFFFF
        want = np.stack([(cid >> (s * (n - 1 - i))) & (base - 1) for i in range(n)]).astype(np.uint8)
        np.testing.assert_array_equal(code[b], want, err_msg=names[b])
    assert code[:3].max() > base // 2 and not code[3].any()


def _raw_crops(dev, idx, bb, method):
    """The C entry points called directly: method None = the old functions without the argument."""
    from zebrapose_amd import _lib as L
    B = len(idx)
    ii = torch.tensor(idx, dtype=torch.int32, device="cuda")
    bd = torch.from_numpy(np.asarray(bb, np.int32)).cuda()
    # prefilled with a value no crop produces, so a pixel left unwritten shows
    x = torch.full((B, 3, S_IMG, S_IMG), 77.0, dtype=torch.float32, device="cuda")
    code = torch.full((B, 16, S_GT, S_GT), 9, dtype=torch.uint8, device="cuda")
    m = torch.full((B, S_GT, S_GT), 77.0, dtype=torch.float32, device="cuda")
    e = torch.full((B, S_GT, S_GT), 77.0, dtype=torch.float32, device="cuda")
    N = dev[0].shape[0]
    tail = () if method is None else (method,)
    sfx = "" if method is None else "_m"
    L.call("zp_crop_image" + sfx, dev[0].data_ptr(), N, H, W, ii.data_ptr(), bd.data_ptr(), B, S_IMG, x.data_ptr(),
           *tail, L.stream_ptr())
    L.call("zp_crop_gt" + sfx, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), N, H, W, ii.data_ptr(),
           bd.data_ptr(), B, S_GT, 16, code.data_ptr(), m.data_ptr(), e.data_ptr(), *tail, L.stream_ptr())
    return [t.cpu().numpy() for t in (x, code, m, e)]


def test_square_path_unchanged(gpu, scene):
    from zebrapose_amd import _lib as L
    from zebrapose_amd.crop import CropPipeline
    host, dev = scene
    names = list(BOXES)
    bb = np.array([BOXES[n] for n in names], np.int32)
    idx = [i % 2 for i in range(len(bb))]
    old = _raw_crops(dev, idx, bb, None)
    new = _raw_crops(dev, idx, bb, L.ZP_CROP_SQUARE)
    for a, b in zip(old, new):
        np.testing.assert_array_equal(a, b)
    out = CropPipeline(S_IMG, S_GT)(dev[0], idx, bb, dev[1], dev[2], dev[3])
    pipe = [out[k].cpu().numpy() for k in ("x", "code", "mask", "entire_mask")]
    for a, b in zip(old, pipe):
        np.testing.assert_array_equal(a, b)
    for n in ("wide", "clip_left_top", "clip_right_bottom"):  # and both equal the pinned square oracle
        b = names.index(n)
        i = idx[b]
        np.testing.assert_array_equal(old[0][b], C.crop_image(host[0][i], bb[b], S_IMG), err_msg=n)
        for got, want in zip((old[1][b], old[2][b], old[3][b]),
                             C.crop_gt(host[1][i], host[2][i], host[3][i], bb[b], S_GT, 16)):
            np.testing.assert_array_equal(got, want, err_msg=n)
    # the rectangular method through the raw entry points is the pipeline's
    rect = _raw_crops(dev, idx, bb, L.ZP_CROP_RECT)
    _check(dict(zip(("x", "code", "mask", "entire_mask"), [torch.from_numpy(a) for a in rect])), host, idx, bb,
           S_IMG, S_GT)
    assert (rect[0] != old[0]).any()


def test_train_batch_under_crop_resize(gpu):
    from zebrapose_amd import _lib as L
    from zebrapose_amd.augment import AugmentSampler, augment_images
    from zebrapose_amd.crop import CropPipeline, aug_Bbox, get_final_Bbox
    h, w = 72, 100  # 3 x 4 tiles of 32, the last row and column partial
    host = _stacks(29, 2, h, w)
    dev = [torch.from_numpy(a).cuda() for a in host]
    raw = np.array([[10, 8, 40, 30], [-5, 30, 30, 50], [60, -4, 50, 40], [70, 50, 28, 20], [30, 20, 12, 31],
                    [300, 10, 20, 20]])
    B = len(raw)
    idx = np.arange(B) % 2
    cp = CropPipeline(S_IMG, S_GT, resize_method="crop_resize")
    seen = 0
    for seed in (2, 6):
        out = cp.train_batch(dev[0], idx, raw, dev[1], dev[2], dev[3], AugmentSampler(True, True,
                                                                                     np.random.default_rng(seed)))
        boxes, batch = out["boxes"], out["aug"]
        rng = np.random.default_rng(seed)  # the boxes are drawn first, from the sampler's generator
        for i in range(B):
            want = aug_Bbox(raw[i], 1.5, rng)
            if i == B - 1:  # wholly outside: clipped to nothing, handled like a missing detection
                assert R.rect_region(want, h, w) is None
                assert not boxes[i].any() and not out["final_boxes"][i].any()
                continue
            np.testing.assert_array_equal(boxes[i], want)
            np.testing.assert_array_equal(out["final_boxes"][i], get_final_Bbox(want, "crop_resize", w, h))
            x1, y1, x2, y2 = R.rect_region(want, h, w)
            np.testing.assert_array_equal(out["final_boxes"][i], [x1, y1, x2 - x1, y2 - y1])
        seen |= int(np.bitwise_or.reduce(batch.flags))
        ref = A.aug_ref_batch(host[0], idx, batch)
        x, code, m, e = (out[k].cpu().numpy() for k in ("x", "code", "mask", "entire_mask"))
        for i in range(B):
            np.testing.assert_array_equal(x[i], R.crop_image_rect(ref[i], boxes[i], S_IMG), err_msg=f"x {i}")
            rc, rm, re = R.crop_gt_rect(host[1][idx[i]], host[2][idx[i]], host[3][idx[i]], boxes[i], S_GT, 16)
            np.testing.assert_array_equal(code[i], rc)
            np.testing.assert_array_equal(m[i], rm)
            np.testing.assert_array_equal(e[i], re)
        assert not x[B - 1].any()
        # the augmentation's box form alone: the tiles meeting the clipped box and nothing else
        pre = torch.full((B, h, w, 3), 7, dtype=torch.uint8, device="cuda")
        augment_images(dev[0], idx, batch, bbox=boxes, out=pre, method=L.ZP_CROP_RECT)
        pre = pre.cpu().numpy()
        for i in range(B):
            t = R.tile_mask(boxes[i], h, w)
            assert (pre[i][~t] == 7).all(), f"crop {i} {boxes[i]}: written outside its tiles"
            np.testing.assert_array_equal(pre[i][t], ref[i][t], err_msg=f"crop {i} {boxes[i]}")
            if i < B - 1:
                assert t.any() and not t.all()
        assert not R.tile_mask(boxes[B - 1], h, w).any()
    assert seen == 31, f"stages met: {seen:05b}"


def test_crop_then_decode_returns_to_the_source_pixel(gpu):
    """GT colour = the pixel's own position (id = y W + x < 2^16).  Cropping with a clipped non-square
    box and decoding the code planes with the returned final box must bring every crop pixel back to
    the source pixel it sampled: the crop reads x1 + min(floor(dx (1 / (S / sw))), sw - 1), the decode
    returns trunc(x1 + dx (sw / S)); dx sw / S < sw, both floors of values that differ by rounding
    only, so |difference| < 1 per axis -- a derived bound, not a measured one.  (The two roundings part
    first at an ROI side of 186, where 1 / (S / sw) falls an ulp short of sw / S and cv2's nearest index
    is one lower at a few dx; no side of a 48 x 64 image reaches that.)"""
    from zebrapose_amd.crop import CropPipeline
    from zebrapose_amd.decode import Decoder
    yy, xx = np.mgrid[0:H, 0:W]
    ids = yy * W + xx
    gt = np.stack([np.zeros_like(ids), ids >> 8, ids & 255], axis=2).astype(np.uint8)[None]
    img = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
    cp = CropPipeline(S_IMG, S_GT, resize_method="crop_resize")
    raw = np.array([[40, -10, 30, 35], [3, 20, 37, 11]])  # padded: clipped at the top right / at the left, both oblong
    pad, fin = cp.boxes(raw, W, H)
    assert fin[0][2] != fin[0][3] and fin[0][1] == 0 and fin[0][0] + fin[0][2] == W
    out = cp(img, [0, 0], pad, torch.from_numpy(gt).cuda())
    logits = (out["code"].float() * 2 - 1) * 20
    mask_logits = torch.full((2, 1, S_GT, S_GT), 20.0, device="cuda")
    dec = Decoder(np.zeros((65536, 3)), device="cuda")
    counts, xy, _, got = dec(mask_logits, logits, fin, bbox_size=S_GT, return_ids=True)
    assert counts.cpu().tolist() == [S_GT * S_GT] * 2
    got = got.cpu().numpy()
    xy = xy.cpu().numpy().reshape(2, S_GT, S_GT, 2)
    for b in range(2):
        np.testing.assert_array_equal(got[b], R.crop_ids_rect(gt[0], pad[b], S_GT))
        src_x, src_y = got[b] % W, got[b] // W
        x1, y1, x2, y2 = R.rect_region(pad[b], H, W)
        assert src_x.min() == x1 and src_y.min() == y1 and src_x.max() < x2 and src_y.max() < y2
        assert np.abs(xy[b, :, :, 0] - src_x).max() < 1 and np.abs(xy[b, :, :, 1] - src_y).max() < 1
