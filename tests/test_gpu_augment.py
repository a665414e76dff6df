"""zp_augment (zebrapose_amd.augment.augment_images, CropPipeline.train_batch) against the numpy
oracle tests/aug_ref.py, bit-exact: every stage alone and all five together on small odd-sized
images (single, partial and several 32 x 32 tiles), the bbox form on 480 x 640 images with boxes
on every border, the copy, the salt-and-pepper statistics, refused arguments, and the training
step fed from train_batch.  Stencil A is an asymmetric ramp, so a fused tile that mirrors its
stage-0 halo instead of evaluating stage 1-2 at the mirrored in-image pixel fails."""
import numpy as np
import pytest
import torch

from oracle import crop_ref as C
from tests import aug_ref as R
from tests.test_gpu_crop import BOXES

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 37), (31, 65), (33, 32), (45, 70)]
STAGES = {"sp": R.SP, "stencil_a": R.STENCIL_A, "dropout": R.DROPOUT, "stencil_b": R.STENCIL_B, "lut": R.LUT,
          "all": 31}
# boxes of test_gpu_crop.py that touch or cross the left/top, right/bottom, all four, left+right, top+right
# borders, one inside, one tiny, plus the zero box
BORDER_BOXES = [BOXES[1], BOXES[2], BOXES[6], BOXES[7], BOXES[9], BOXES[0], BOXES[11], [0, 0, 0, 0]]


def _q16(w):
    """Largest-remainder quantisation to sum 65536 (the test's own)."""
    t = np.asarray(w, np.float64) / np.sum(w) * 65536
    q = np.floor(t).astype(np.int64)
    for i in np.argsort(-(t - q).ravel())[:65536 - q.sum()]:
        q.ravel()[i] += 1
    assert q.sum() == 65536
    return q.astype(np.int32)


def _ramp_kernel(rng):
    """A diagonal ramp plus small random weights everywhere: no symmetry of any kind."""
    w = rng.random((5, 5)) * 0.2
    w[np.arange(5), np.arange(5)] += np.arange(1, 6)
    return _q16(w)


def _batch(rng, B, H, W, flags, mh=None, mw=None, sp_p=0.05):
    """Hand-built descriptors with every stage's data non-trivial, whatever the flags."""
    from zebrapose_amd.augment import empty_batch
    b = empty_batch(B, H, W, mh, mw)
    b.flags[:] = flags
    b.sp_seed[:] = rng.integers(0, 1 << 32, B, dtype=np.uint64)
    b.sp_thresh[:] = int(sp_p * 2 ** 32)
    for i in range(B):
        b.kA[i] = _ramp_kernel(rng)
        g = rng.random(5) + 0.1
        b.kB[i] = _q16(np.outer(g, g[::-1] + rng.random(5)))
        b.luts[i] = np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8)
    b.masks[:] = rng.random(b.masks.shape) >= 0.4
    b.beta_tab = R.beta_tab()
    return b


@pytest.mark.parametrize("stage", list(STAGES))
def test_stages_match_oracle_on_small_images(gpu, stage):
    from zebrapose_amd.augment import augment_images
    rng = np.random.default_rng(list(STAGES).index(stage))
    for H, W in SIZES:
        imgs = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        idx = rng.integers(0, 3, 4)
        mh, mw = ((5, 7) if (H, W) == (45, 70) else (H, W) if (H, W) == (9, 37) else (None, None))
        b = _batch(rng, 4, H, W, STAGES[stage], mh, mw, sp_p=0.3)
        out = augment_images(torch.from_numpy(imgs).cuda(), idx, b).cpu().numpy()
        ref = R.aug_ref_batch(imgs, idx, b)
        np.testing.assert_array_equal(out, ref, err_msg=f"{stage} {H}x{W}")
        assert stage == "stencil_a" or stage == "stencil_b" or (out != imgs[idx]).any()


def test_mixed_flags_per_crop(gpu):
    from zebrapose_amd.augment import augment_images
    rng = np.random.default_rng(11)
    H, W = 45, 70
    imgs = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    b = _batch(rng, 8, H, W, 0, sp_p=0.2)
    b.flags[:] = [0, 31, 6, 10, 12, 3, 17, 14]
    idx = rng.integers(0, 2, 8)
    out = augment_images(torch.from_numpy(imgs).cuda(), idx, b).cpu().numpy()
    np.testing.assert_array_equal(out, R.aug_ref_batch(imgs, idx, b))


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(5)
    N, H, W = 3, 480, 640
    imgs = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    gts = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    masks = rng.integers(0, 2, (N, H, W), dtype=np.uint8) * 255
    ent = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
    return imgs, gts, masks, ent


def _region(box, H, W):
    """crop_square_resize's copied image region (oracle/crop_ref.py square_roi): y0, y1, x0, x1."""
    x1, y1, bw, bh = box[0], box[1], max(box[2], 0), max(box[3], 0)
    x2, y2 = x1 + bw, y1 + bh
    cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    if bh > bw:
        x1, x2 = cx - bh / 2, cx + bh / 2
    else:
        y1, y2 = cy - bw / 2, cy + bw / 2
    x1, y1, x2, y2 = int(x1), int(y1), int(x2), int(y2)
    return max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)


def test_bbox_form_writes_each_copied_region(gpu, scene):
    from zebrapose_amd.augment import augment_images
    imgs = scene[0]
    N, H, W = imgs.shape[:3]
    rng = np.random.default_rng(21)
    bb = np.array(BORDER_BOXES, np.int32)
    B = len(bb)
    idx = rng.integers(0, N, B)
    b = _batch(rng, B, H, W, 31)
    ref = R.aug_ref_batch(imgs, idx, b)
    out = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    augment_images(torch.from_numpy(imgs).cuda(), idx, b, bbox=bb, out=out)
    out = out.cpu().numpy()
    for i in range(B):
        y0, y1, x0, x1 = _region(bb[i], H, W)
        if bb[i][2] <= 0 and bb[i][3] <= 0:
            assert (out[i] == 7).all(), "a zero box writes nothing"
            continue
        assert y1 > y0 and x1 > x0
        np.testing.assert_array_equal(out[i, y0:y1, x0:x1], ref[i, y0:y1, x0:x1], err_msg=f"crop {i} {bb[i]}")
        # whatever else was written is the oracle's value too; tiles a whole tile away are untouched
        wrote = (out[i] != 7).any(axis=2)
        np.testing.assert_array_equal(out[i][wrote], ref[i][wrote])
        far = np.ones((H, W), bool)
        far[max(y0 - 32, 0):y1 + 32, max(x0 - 32, 0):x1 + 32] = False
        assert (out[i][far] == 7).all()


def test_train_batch_matches_oracle(gpu, scene):
    from zebrapose_amd.augment import AugmentSampler
    from zebrapose_amd.crop import CropPipeline, aug_Bbox, get_final_Bbox
    imgs, gts, masks, ent = scene
    N, H, W = imgs.shape[:3]
    raw = np.array(BORDER_BOXES)
    B = len(raw)
    idx = np.arange(B) % N
    cp = CropPipeline()
    dev = [torch.from_numpy(a).cuda() for a in (imgs, gts, masks, ent)]
    seen = 0
    for seed in (2, 6):  # two draws of the chain whose flags, between them, switch every stage on
        sampler = AugmentSampler(True, True, np.random.default_rng(seed))
        out = cp.train_batch(dev[0], idx, raw, dev[1], dev[2], dev[3], sampler)
        boxes, batch = out["boxes"], out["aug"]
        rng = np.random.default_rng(seed)  # the boxes are drawn first, from the sampler's generator
        for i in range(B):
            want = aug_Bbox(raw[i], 1.5, rng)
            np.testing.assert_array_equal(boxes[i], want)
            np.testing.assert_array_equal(out["final_boxes"][i], get_final_Bbox(want, "crop_square_resize", W, H))
        seen |= int(np.bitwise_or.reduce(batch.flags))
        x, code, m, e = (out[k].cpu().numpy() for k in ("x", "code", "mask", "entire_mask"))
        ref = R.aug_ref_batch(imgs, idx, batch)
        for i in range(B):
            np.testing.assert_array_equal(x[i], C.crop_image(ref[i], boxes[i]), err_msg=f"x {i} {boxes[i]}")
            rc, rm, re = C.crop_gt(gts[idx[i]], masks[idx[i]], ent[idx[i]], boxes[i])
            np.testing.assert_array_equal(code[i], rc)
            np.testing.assert_array_equal(m[i], rm)
            np.testing.assert_array_equal(e[i], re)
        assert not x[B - 1].any()  # the zero box stays the all-zero dummy crop
    assert seen == 31, f"stages met: {seen:05b}"


def test_copy_and_reproducibility(gpu):
    from zebrapose_amd.augment import augment_images, empty_batch
    rng = np.random.default_rng(4)
    H, W = 45, 70
    imgs = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    d = torch.from_numpy(imgs).cuda()
    idx = np.array([2, 0, 1, 1])
    out = augment_images(d, idx, empty_batch(4, H, W)).cpu().numpy()
    np.testing.assert_array_equal(out, imgs[idx])
    b = _batch(rng, 4, H, W, 0)  # flags 0 ignore every descriptor
    np.testing.assert_array_equal(augment_images(d, idx, b).cpu().numpy(), imgs[idx])
    b.flags[:] = 31
    r1 = augment_images(d, idx, b).cpu().numpy()
    r2 = augment_images(d, idx, b).cpu().numpy()
    np.testing.assert_array_equal(r1, r2)
    assert (r1 != imgs[idx]).any()


def test_salt_and_pepper_statistics(gpu):
    from zebrapose_amd.augment import augment_images, empty_batch
    rng = np.random.default_rng(9)
    H = W = 128
    img = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    img[..., 1] = img[..., 0] ^ 0xFF  # no source pixel has equal channels
    B = 5
    b = empty_batch(B, H, W)
    b.flags[:] = R.SP
    b.sp_seed[:] = rng.integers(0, 1 << 32, B, dtype=np.uint64)
    b.sp_thresh[:] = int(0.05 * 2 ** 32)
    out = augment_images(torch.from_numpy(img).cuda(), np.zeros(B, np.int64), b).cpu().numpy()
    tab = R.beta_tab()
    assert tab[0] == 0 and tab[255] == 255 and tab[127] in (126, 127) and (np.diff(tab.astype(int)) >= 0).all()
    for i in range(B):
        hit = (out[i] != img[0]).any(axis=2)
        frac = hit.mean()
        print(f"seed {int(b.sp_seed[i])}: replaced {frac:.4f}")
        assert 0.043 <= frac <= 0.057, frac
        px = out[i][hit]
        assert (px[:, 0] == px[:, 1]).all() and (px[:, 0] == px[:, 2]).all() and np.isin(px[:, 0], tab).all()
        np.testing.assert_array_equal(out[i][~hit], img[0][~hit])
    assert len({out[i].tobytes() for i in range(B)}) == B  # the seed moves the pattern


def test_bad_arguments_are_refused(gpu):
    from zebrapose_amd import _lib as L
    from zebrapose_amd.augment import _pack, empty_batch
    H = W = 16
    img = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((1, H, W, 3), 9, dtype=torch.uint8, device="cuda")
    ii = torch.zeros(1, dtype=torch.int32, device="cuda")
    buf, offs = _pack(empty_batch(1, H, W))
    d = torch.from_numpy(buf).cuda()
    p = [d.data_ptr() + o for o in offs]

    def call(**kw):
        a = dict(imgs=img.data_ptr(), n=1, H=H, W=W, ii=ii.data_ptr(), desc=p[0], masks=p[1], mh=3, mw=3, luts=p[2],
                 beta=p[3], B=1, out=out.data_ptr())
        a.update(kw)
        L.call("zp_augment", a["imgs"], a["n"], a["H"], a["W"], a["ii"], a["desc"], a["masks"], a["mh"], a["mw"],
               a["luts"], a["beta"], None, a["B"], a["out"], L.stream_ptr())

    for kw, word in ((dict(H=7), "H, W >= 8"), (dict(W=4), "H, W >= 8"), (dict(mh=0), "dropout mask"),
                     (dict(mw=0), "dropout mask"), (dict(mh=H + 1), "dropout mask"), (dict(mw=W + 1), "dropout mask"),
                     (dict(imgs=None), "null"), (dict(ii=None), "null"), (dict(desc=None), "null"),
                     (dict(masks=None), "null"), (dict(luts=None), "null"), (dict(beta=None), "null"),
                     (dict(out=None), "null"), (dict(B=0), "bad"), (dict(n=0), "bad"),
                     (dict(H=1024, W=1024, n=(1 << 40) // (1024 * 1024 * 3) + 1), "too large")):
        with pytest.raises(L.ZPError, match=word):
            call(**kw)
    torch.cuda.synchronize()
    assert (out == 9).all()
    call()  # and the same call with nothing wrong goes through
    assert not out.cpu().numpy().any()


def test_train_batch_feeds_a_training_step(gpu):
    from zebrapose_amd.augment import AugmentSampler
    from zebrapose_amd.crop import CropPipeline
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeNet_Deeplab
    from zebrapose_amd.train import TrainStep
    g = torch.Generator().manual_seed(0)
    N, H, W = 2, 480, 640
    imgs = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    gts = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    mk = (torch.randint(0, 2, (N, H, W), dtype=torch.uint8, generator=g) * 255).cuda()
    out = CropPipeline().train_batch(imgs, [0, 1], [[100, 100, 180, 160], [400, 300, 200, 150]], gts, mk, mk,
                                     AugmentSampler(True, True, np.random.default_rng(0)))
    assert out["x"].shape == (2, 3, 256, 256) and out["code"].shape == (2, 16, 128, 128)
    assert out["final_boxes"].shape == (2, 4)
    net = BinaryCodeNet_Deeplab(34, 16, 2, concat=True, output_kernel_size=1, precision="bf16").cuda().train()
    loss = TrainStep(net, learning_rate=2e-4)(out["x"], out["code"], out["mask"])[0]
    assert np.isfinite(float(loss))
