"""zp_mask_bbox, zp_composite and SyntheticBatcher against their numpy restatements
(tests/synth_ref.py, tests/shade_ref.py): every byte compared, no tolerance."""
import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests import shade_ref as SR
from tests import synth_ref as YR
from tests.test_gpu_render import rot_xyz

pytestmark = pytest.mark.gpu

H, W = 24, 40


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_mask_bbox(gpu):
    from zebrapose_amd.synth import mask_bbox
    m = np.zeros((5, H, W), np.uint8)
    m[1, 7, 33] = 1                       # a single pixel, any nonzero value
    m[2] = 255                            # full
    m[3, 3, 20] = m[3, 20, 2] = m[3, 11, 39] = m[3, 23, 17] = 255  # ragged: each bound from another pixel
    m[4, 0, 0] = m[4, 23, 39] = 9
    got = mask_bbox(cuda(m)).cpu().numpy()
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, [[0, 0, -1, -1], [7, 33, 7, 33], [0, 0, 23, 39], [3, 2, 23, 39], [0, 0, 23, 39]])
    np.testing.assert_array_equal(got, YR.mask_bbox(m))
    big = np.zeros((2, 61, 67), np.uint8)  # more pixels than one pass of the block
    big[0, 50:60, 3:66] = 1
    big[1, 60, 66] = 1
    np.testing.assert_array_equal(mask_bbox(cuda(big)).cpu().numpy(), YR.mask_bbox(big))


def blob_masks(B, seed):
    """An ellipse per sample; the last one empty."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((B, H, W), np.uint8)
    for b in range(B - 1):
        cy, cx, ry, rx = r.uniform(9, 14), r.uniform(15, 25), r.uniform(5, 9), r.uniform(7, 14)
        m[b] = np.where(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1, 255, 0)
    return m


# one sample per truncation mode, truncation off, and (the last) an empty mask under a truncating draw
TRUNC = np.array([[0.1, 0.37], [0.3, 0.81], [0.5, 0.5], [0.7, 0.123], [0.9, 0.4], [-1.0, 0.6], [0.15, 0.7]])


@pytest.mark.parametrize("bg_hw", [(30, 50), (50, 30), (48, 80), (24, 40), (31, 47)],
                         ids=["wide", "tall", "twice", "same", "odd"])
def test_composite(gpu, bg_hw):
    from zebrapose_amd.synth import bg_geometry, composite
    B = len(TRUNC)
    r = np.random.default_rng(sum(bg_hw))
    fg = r.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    mask = blob_masks(B, 5)
    assert not mask[-1].any() and all(mask[b].any() for b in range(B - 1))
    bgs = r.integers(0, 256, (3,) + bg_hw + (3,)).astype(np.uint8)
    idx = np.array([0, 1, 2, 0, 1, 2, 1])
    cw, ch, ow, oh, f = bg_geometry(bg_hw[0], bg_hw[1], H, W)
    ref_img, ref_mask = YR.composite(fg, mask, bgs, idx, np.tile([cw, ch, ow, oh], (B, 1)), np.full(B, f), TRUNC)
    img, mo = composite(cuda(fg), cuda(mask), cuda(bgs), idx, TRUNC)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mo.cpu().numpy(), ref_mask)
    np.testing.assert_array_equal(img.cpu().numpy(), ref_img)
    # the modes did what they say: 0-3 cut something off, 4 and 5 nothing, the empty mask shows background only
    kept = [(ref_mask[b] != 0).sum() / max((mask[b] != 0).sum(), 1) for b in range(B)]
    assert all(0 < k < 1 for k in kept[:4]) and kept[4] == 1 and kept[5] == 1 and not ref_mask[6].any()
    np.testing.assert_array_equal(ref_img[6], YR.background(bgs[1], (cw, ch, ow, oh), f, H, W))


def test_composite_geometry_beyond_the_image(gpu):
    """A caller's geometry whose resized background is larger than the image: the excess is dropped;
    one that does not fit the stack shows a zero background."""
    from zebrapose_amd import _lib as L
    r = np.random.default_rng(9)
    B = 4
    fg = r.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    mask = blob_masks(B + 1, 6)[:B]
    bgs = r.integers(0, 256, (1, 30, 50, 3)).astype(np.uint8)
    # larger than the image; smaller; a crop wider than the stack; a 2x reduction of odd sides, whose last
    # row and column of 2 x 2 blocks are cut by the crop
    geo = np.array([[50, 30, 45, 27], [50, 30, 20, 12], [51, 30, 40, 24], [49, 29, 25, 15]], np.int32)
    fs = np.array([0.9, 0.4, 0.8, 0.5])
    trunc = np.full((B, 2), -1.0)
    d = [cuda(a) for a in (fg, mask, bgs, np.zeros(B, np.int32), geo, fs, trunc)]
    bbox = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    out, mo = torch.empty_like(d[0]), torch.empty_like(d[1])
    st = L.stream_ptr()
    L.call("zp_mask_bbox", d[1].data_ptr(), B, H, W, bbox.data_ptr(), st)
    L.call("zp_composite", d[0].data_ptr(), d[1].data_ptr(), bbox.data_ptr(), B, H, W, d[2].data_ptr(), 1, 30, 50,
           d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), out.data_ptr(), mo.data_ptr(), st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b in (0, 1, 3):
        bgi = YR.background(bgs[0], geo[b], fs[b], H, W)
        np.testing.assert_array_equal(got[b], np.where((mask[b] != 0)[..., None], fg[b], bgi))
    np.testing.assert_array_equal(got[2], np.where((mask[2] != 0)[..., None], fg[2], 0))
    np.testing.assert_array_equal(mo.cpu().numpy(), np.where(mask != 0, 255, 0))


def test_synthetic_batcher_feeds_train_batch(gpu):
    from zebrapose_amd.augment import AugmentSampler
    from zebrapose_amd.crop import CropPipeline
    from zebrapose_amd.render import MeshRenderer, face_bgr_from_ids
    from zebrapose_amd.synth import SyntheticBatcher, bg_geometry
    v, f = RR.icosphere(2)
    rgb = np.random.default_rng(1).integers(0, 256, (len(v), 3)).astype(np.uint8)
    ids = 777 + np.arange(len(f))
    Hh, Ww = 48, 64
    bgs = np.random.default_rng(2).integers(0, 256, (2, 60, 100, 3)).astype(np.uint8)
    sb = SyntheticBatcher(MeshRenderer(v, f, colors=rgb, normals=v), MeshRenderer.from_class_ids(v, f, ids), bgs,
                          rng=np.random.default_rng(3))
    R = np.stack([rot_xyz(0.9, -0.3, 0.5), rot_xyz(-0.2, 1.1, 0.0)]).reshape(2, 9)
    t = np.array([[0.1, -0.1, 3.0], [-0.3, 0.2, 2.4]])
    K = np.array([[55.0, 55.0, 32.0, 24.0], [50.0, 58.0, 30.0, 26.0]])
    draws = sb.sample(2)
    draws["trunc"][:, 0] = [0.1, 0.7]  # one cut above, one on the right
    dev = sb(R, t, K, Hh, Ww, draws=draws)
    torch.cuda.synchronize()
    # the same batch built on the host
    light = np.concatenate([draws["light"], draws["phong"]], 1)
    ref = SR.render_shaded(v, f, v, rgb, R, t, K, light, Hh, Ww)
    gt = RR.render(v, f, face_bgr_from_ids(ids), R, t, K, Hh, Ww)["color"]
    geo = bg_geometry(60, 100, Hh, Ww)
    img, mo = YR.composite(ref["shaded"], ref["mask"], bgs, draws["bg_index"], np.tile(geo[:4], (2, 1)), np.full(2, geo[4]),
                           draws["trunc"])
    bb = YR.mask_bbox(mo).astype(np.int64)
    raw = np.stack([bb[:, 1], bb[:, 0], bb[:, 3] - bb[:, 1] + 1, bb[:, 2] - bb[:, 0] + 1], 1)
    assert (mo != 0).sum() > 300 and ((mo != 0) != (ref["mask"] != 0)).any() and (raw[:, 2:] > 5).all()
    for k, a in (("images", img), ("gt_images", gt), ("masks", mo), ("entire_masks", ref["mask"])):
        np.testing.assert_array_equal(dev[k].cpu().numpy(), a, err_msg=k)
    np.testing.assert_array_equal(dev["raw_boxes"], raw)
    cp = CropPipeline()
    a = cp.train_batch(dev["images"], dev["img_index"], dev["raw_boxes"], dev["gt_images"], dev["masks"],
                       dev["entire_masks"], AugmentSampler(rng=np.random.default_rng(4)))
    b = cp.train_batch(cuda(img), np.arange(2), raw, cuda(gt), cuda(mo), cuda(ref["mask"]),
                       AugmentSampler(rng=np.random.default_rng(4)))
    torch.cuda.synchronize()
    for k in ("x", "code", "mask", "entire_mask"):
        np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=k)
    np.testing.assert_array_equal(a["final_boxes"], b["final_boxes"])
    assert a["code"].any() and a["mask"].any()
