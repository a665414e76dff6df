"""zp_scene_compose against its numpy definition (tests/scene_ref.py), every output compared bit for
bit, and the Python layers above it (scene_compose, SceneBatcher, CropPipeline's gt_index) on two
tiny meshes."""
import numpy as np
import pytest
import torch

from tests import scene_ref as SR

pytestmark = pytest.mark.gpu

OUTS = ("image", "fg", "scene", "instance", "mask_visib", "info")
# scalar path (W % 4 != 0), the same with more than one block, vector path, the same with a partly
# filled last item row, and with more than one block
SHAPES = [(5, 7), (33, 35), (8, 12), (33, 64), (40, 108)]
LAYOUTS = {"one": ([0], 1), "five": ([2, 0, 2, 0, 2], 3)}  # unsorted; image 1 of "five" has no instance


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_case(H, W, idx, seed):
    """depth f32 [B, H, W] and shaded u8 [B, H, W, 3]: positive values with about half the pixels 0, exact
    two- and three-way ties, one instance wholly behind another, and the special values."""
    r = np.random.default_rng(seed)
    B = len(idx)
    depth = r.uniform(0.5, 4.0, (B, H, W)).astype(np.float32)
    depth[r.random((B, H, W)) < 0.5] = 0.0
    flat = depth.reshape(B, -1)
    n = H * W
    special = np.array([0.0, -1.0, np.nan, np.inf, 1e-45], np.float32)
    for b in range(B):
        flat[b, r.permutation(n)[:10]] = np.tile(special, 2)
    if B == 5:  # image 2 holds 0, 2, 4 and image 0 holds 1, 3
        p = r.permutation(n)
        flat[0, p[:4]] = flat[2, p[:4]] = flat[4, p[:4]] = 1.25       # three tie: 0 wins
        flat[0, p[4:8]] = 0.0
        flat[2, p[4:8]] = flat[4, p[4:8]] = 0.75                      # two tie with nothing before them: 2 wins
        flat[0, p[8]], flat[2, p[8]], flat[4, p[8]] = 0.0, np.inf, np.inf    # a tie at infinity
        flat[0, p[9]], flat[2, p[9]], flat[4, p[9]] = np.nan, 2.0, -1.0      # NaN is no surface
        flat[0, p[10]], flat[2, p[10]], flat[4, p[10]] = 1e-45, 0.5, 0.5     # the subnormal is the nearest
        flat[1] = r.uniform(0.5, 2.0, n).astype(np.float32)           # 1 covers the image ...
        flat[3] = np.where(flat[3] > 0, flat[1] + np.float32(1.0), 0)  # ... and 3 lies wholly behind it
    shaded = r.integers(1, 256, (B, H, W, 3)).astype(np.uint8)
    return depth, shaded


def run(depth, idx, n_img, shaded=None, outputs=None):
    from zebrapose_amd.synth import scene_compose
    o = scene_compose(cuda(depth), np.asarray(idx), n_img, None if shaded is None else cuda(shaded), outputs)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_kernel_equals_the_definition(gpu, hw, layout):
    from zebrapose_amd.gtinfo import scene_depth
    from zebrapose_amd.synth import mask_bbox
    idx, n_img = LAYOUTS[layout]
    depth, shaded = make_case(*hw, idx, seed=hw[0] * 1000 + hw[1] + len(idx))
    ref = SR.scene_compose(depth, idx, n_img, shaded)
    got = run(depth, idx, n_img, shaded)
    for k in OUTS:
        assert same_bits(got[k], ref[k]), k
    for k, v in SR.host_fields(ref["info"]).items():
        assert same_bits(got[k], v), k
    # the case holds what it is meant to hold
    if layout == "five":
        assert ref["info"][3, 0] > 0 and ref["info"][3].tolist()[1:] == [0, 0, 0, -1, -1] and not ref["mask_visib"][3].any()
        assert (ref["instance"][1] == -1).all() and not ref["image"][1].any() and not ref["fg"][1].any()
        assert sorted(np.unique(ref["instance"]).tolist()) == [-1, 0, 1, 2, 4]
    assert np.isinf(ref["scene"]).any() and (ref["scene"] == np.float32(1e-45)).any() and not np.isnan(ref["scene"]).any()
    # cross-checks against what the library already had
    scene, inst = scene_depth(cuda(depth), np.asarray(idx), n_img)
    assert same_bits(scene.cpu().numpy(), got["scene"]) and same_bits(inst.cpu().numpy(), got["instance"])
    assert same_bits(mask_bbox(cuda(got["mask_visib"])).cpu().numpy(), got["info"][:, 2:])
    assert np.array_equal((got["mask_visib"] == 255).sum((1, 2)), got["info"][:, 1])
    assert np.isin(got["mask_visib"], (0, 255)).all()
    for n in range(n_img):  # the visible masks of an image: pairwise disjoint, their union the foreground
        members = [b for b in range(len(idx)) if idx[b] == n]
        cover = sum((got["mask_visib"][b] > 0).astype(np.int32) for b in members) if members else np.zeros(hw, np.int32)
        assert cover.max() <= 1 and np.array_equal(cover * 255, got["fg"][n])
    # the same input again: the same bytes
    again = run(depth, idx, n_img, shaded)
    for k in OUTS:
        assert same_bits(again[k], got[k]), k


@pytest.mark.parametrize("hw", [(5, 7), (8, 12)], ids=["scalar", "vector"])
def test_each_output_may_be_left_out(gpu, hw):
    idx, n_img = LAYOUTS["five"]
    depth, shaded = make_case(*hw, idx, seed=11)
    ref = SR.scene_compose(depth, idx, n_img, shaded)
    got = run(depth, idx, n_img, None)  # no shaded: every output but image
    assert "image" not in got
    for k in OUTS[1:]:
        assert same_bits(got[k], ref[k]), k
    for drop in OUTS:
        keep = tuple(k for k in OUTS if k != drop)
        got = run(depth, idx, n_img, shaded, keep)
        assert drop not in got and ("bbox_visib" in got) == (drop != "info")
        for k in keep:
            assert same_bits(got[k], ref[k]), (drop, k)
    for only in OUTS:
        got = run(depth, idx, n_img, shaded, (only,))
        assert same_bits(got[only], ref[only]), only


def test_an_instance_of_no_image(gpu):
    """img_index outside [0, n_img): never an index (the kernels compare it with the image numbers and
    test its range before anything else), an empty visible mask, px_all counted, the others undisturbed."""
    H, W = 8, 12
    idx = [0, 7, 1, -1]
    depth, shaded = make_case(H, W, idx, seed=3)
    depth[1] = np.where(depth[1] > 0, np.float32(0.25), 0)  # nearer than everything, were it in an image
    ref = SR.scene_compose(depth, idx, 2, shaded)
    got = run(depth, idx, 2, shaded)
    for k in OUTS:
        assert same_bits(got[k], ref[k]), k
    for b in (1, 3):
        n_all = int((depth[b] > 0).sum())
        assert n_all > 0 and got["info"][b].tolist() == [n_all, 0, 0, 0, -1, -1] and not got["mask_visib"][b].any()
        assert got["bbox_visib"][b].tolist() == [0, 0, 0, 0] and got["visib_fract"][b] == 0.0
    alone = run(depth[[0, 2]], [0, 1], 2, shaded[[0, 2]])
    for k in ("image", "fg", "scene"):
        assert same_bits(alone[k], got[k]), k
    assert same_bits(alone["mask_visib"], got["mask_visib"][[0, 2]]) and same_bits(alone["info"], got["info"][[0, 2]])
    assert np.array_equal(np.where(got["instance"] == 2, 1, got["instance"]), alone["instance"])
    # the mask of an instance of no image is cleared whatever it held, also alone and on the scalar path
    for hw in ((8, 12), (5, 7)):
        d = np.ones((1,) + hw, np.float32)
        o = run(d, [4], 2, None, ("mask_visib", "info", "fg"))
        assert not o["mask_visib"].any() and not o["fg"].any() and o["info"].tolist() == [[hw[0] * hw[1], 0, 0, 0, -1, -1]]


# ---- the Python layers, on two quads -------------------------------------------------------------------

HQ, WQ = 24, 32
KQ = [20.0, 20.0, 16.0, 12.0]


def quad_renderers(same_codes):
    """obj_id -> (shaded renderer, code renderer) of two two-triangle quads with vertex colours and normals
    facing the camera; object 2's code renderer is its shaded one when ``same_codes``."""
    from zebrapose_amd.render import MeshRenderer
    f = np.array([[0, 1, 2], [0, 2, 3]])
    nrm = np.tile([0.0, 0.0, -1.0], (4, 1))
    rs, rc = {}, {}
    for oid, half in ((1, 0.5), (2, 0.4)):
        v = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float64)
        rgb = np.random.default_rng(oid).integers(60, 256, (4, 3)).astype(np.uint8)
        rs[oid] = MeshRenderer(v, f, colors=rgb, normals=nrm)
        rc[oid] = rs[oid] if same_codes and oid == 2 else MeshRenderer.from_class_ids(v, f, [300 * oid, 300 * oid + 7])
    return rs, rc


def backgrounds():
    return np.random.default_rng(5).integers(0, 256, (3, 30, 50, 3)).astype(np.uint8)


def host(o, k):
    return o[k].cpu().numpy() if isinstance(o[k], torch.Tensor) else np.asarray(o[k])


@pytest.mark.parametrize("same_codes", [False, True], ids=["two_renderers", "one_renderer"])
def test_one_instance_per_image_equals_the_synthetic_batcher(gpu, same_codes):
    from zebrapose_amd.synth import SceneBatcher, SyntheticBatcher
    rs, rc = quad_renderers(same_codes)
    bgs = backgrounds()
    sb = SceneBatcher(rs, rc, bgs, rng=np.random.default_rng(8))
    obj = [2, 1, 2]
    R = np.tile(np.eye(3), (3, 1, 1))
    t = np.array([[0.1, 0.0, 2.0], [-0.2, 0.1, 2.5], [0.3, -0.1, 1.7]])
    draws = sb.sample(3)
    out = sb(obj, np.array([1, 0, 2]), R, t, KQ, HQ, WQ, draws=draws)  # instance b is alone in its image
    torch.cuda.synchronize()
    assert out["kept"].tolist() == [0, 1, 2] and out["img_index"].tolist() == [1, 0, 2]
    assert out["gt_index"].tolist() == [0, 1, 2] and out["visib_fract"].tolist() == [1.0] * 3
    for b, (oid, n) in enumerate(zip(obj, (1, 0, 2))):
        one = SyntheticBatcher(rs[oid], rc[oid], bgs, truncate_fg=False)
        d = {"light": draws["light"][n:n + 1], "phong": draws["phong"][n:n + 1], "bg_index": draws["bg_index"][n:n + 1],
             "trunc": np.full((1, 2), -1.0)}
        want = one(R[b:b + 1], t[b:b + 1], KQ, HQ, WQ, draws=d)
        torch.cuda.synchronize()
        assert same_bits(host(out, "images")[n], host(want, "images")[0]), b
        for k in ("gt_images", "masks", "entire_masks"):
            assert same_bits(host(out, k)[b], host(want, k)[0]), (b, k)
        assert same_bits(out["raw_boxes"][b], want["raw_boxes"][0]) and host(want, "masks").any()
        assert host(want, "gt_images").any()


def test_a_near_quad_hides_half_of_a_far_one(gpu):
    from zebrapose_amd.synth import SceneBatcher, composite
    rs, rc = quad_renderers(False)
    bgs = backgrounds()
    sb = SceneBatcher(rs, rc, bgs, rng=np.random.default_rng(9))
    # instance 0: the far quad (object 1, 1 wide, at z = 2); instance 1: the near one, 10 % nearer, over its right half
    obj, ii = [1, 2], np.array([0, 0])
    R = np.tile(np.eye(3), (2, 1, 1))
    t = np.array([[-0.1, 0.0, 2.0], [0.3, 0.0, 1.8]])
    draws = sb.sample(1)
    out = sb(obj, ii, R, t, KQ, HQ, WQ, draws=draws)
    torch.cuda.synchronize()
    masks, entire, images = host(out, "masks") > 0, host(out, "entire_masks") > 0, host(out, "images")
    far, near = entire[0], entire[1]
    assert out["kept"].tolist() == [0, 1] and (far & near).sum() > 20 and (far & ~near).sum() > 20
    assert np.array_equal(masks[1], near) and np.array_equal(masks[0], far & ~near)
    inst = host(out, "instance")[0]
    assert np.array_equal(inst == 1, near) and np.array_equal(inst == 0, far & ~near) and np.array_equal(inst < 0, ~(far | near))
    shaded = [rs[o].render_shaded(R[b:b + 1], t[b:b + 1], KQ, HQ, WQ, light=draws["light"], phong=draws["phong"],
                                  outputs=("shaded",))["shaded"][0].cpu().numpy() for b, o in enumerate(obj)]
    assert np.array_equal(images[0][near], shaded[1][near]) and np.array_equal(images[0][masks[0]], shaded[0][masks[0]])
    assert (shaded[1][far & near] != shaded[0][far & near]).any()
    empty = torch.zeros((1, HQ, WQ, 3), dtype=torch.uint8, device="cuda")
    bg = composite(empty, empty[..., 0].contiguous(), cuda(bgs), draws["bg_index"], np.full((1, 2), -1.0))[0][0].cpu().numpy()
    assert np.array_equal(images[0][~(far | near)], bg[~(far | near)]) and bg.any()
    fract = (far & ~near).sum() / far.sum()
    assert 0.3 < fract < 0.7 and out["visib_fract"].tolist() == [fract, 1.0]
    ys, xs = np.nonzero(masks[0])
    assert out["raw_boxes"][0].tolist() == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
    # a bound above the far one's fraction drops it; as a non-target it still occludes nothing of the near one
    out2 = sb(obj, ii, R, t, KQ, HQ, WQ, draws=draws, min_visib_fract=fract + 1e-6)
    assert out2["kept"].tolist() == [1] and out2["img_index"].tolist() == [0] and out2["gt_index"].tolist() == [0]
    assert same_bits(host(out2, "masks")[0], host(out, "masks")[1]) and same_bits(host(out2, "images"), images)
    assert same_bits(host(out2, "gt_images")[0], host(out, "gt_images")[1]) and host(out2, "gt_images").shape[0] == 1
    out3 = sb(obj, ii, R, t, KQ, HQ, WQ, draws=draws, targets=[0], min_visib_fract=fract)
    assert out3["kept"].tolist() == [0] and same_bits(host(out3, "masks")[0], host(out, "masks")[0])
    assert same_bits(host(out3, "gt_images")[0], host(out, "gt_images")[0]) and same_bits(host(out3, "images"), images)


def crop_inputs():
    r = np.random.default_rng(21)
    H, W = 40, 56
    images = r.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    gt = r.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    masks = np.where(r.random((3, H, W)) < 0.5, 255, 0).astype(np.uint8)
    entire = np.where(r.random((3, H, W)) < 0.7, 255, 0).astype(np.uint8)
    img_index, gt_index = np.array([1, 0, 1, 1]), np.array([2, 0, 1, 2])
    raw = np.array([[5, 4, 30, 20], [20, 10, 25, 28], [-4, 12, 30, 30], [8, 8, 12, 16]])
    return images, gt, masks, entire, img_index, gt_index, raw


@pytest.mark.parametrize("method", ["crop_square_resize", "crop_resize"])
def test_crops_from_per_instance_stacks(gpu, method):
    """gt_index on per-instance stacks against the same data expanded to image-aligned stacks through the
    call as it was."""
    from zebrapose_amd.augment import AugmentSampler
    from zebrapose_amd.crop import CropPipeline
    images, gt, masks, entire, ii, gi, raw = crop_inputs()
    cp = CropPipeline(crop_size_img=32, crop_size_gt=16, resize_method=method)
    boxes, _ = cp.boxes(raw, 56, 40)
    a = cp(cuda(images), ii, boxes, cuda(gt), cuda(masks), cuda(entire), gt_index=gi)
    b = cp(cuda(images[ii]), np.arange(4), boxes, cuda(gt[gi]), cuda(masks[gi]), cuda(entire[gi]))
    torch.cuda.synchronize()
    for k in ("x", "code", "mask", "entire_mask"):
        assert same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    assert a["code"].any() and a["mask"].any() and not same_bits(a["code"][0].cpu().numpy(), a["code"][1].cpu().numpy())
    a = cp.train_batch(cuda(images), ii, raw, cuda(gt), cuda(masks), cuda(entire),
                       AugmentSampler(rng=np.random.default_rng(4)), gt_index=gi)
    b = cp.train_batch(cuda(images[ii]), np.arange(4), raw, cuda(gt[gi]), cuda(masks[gi]), cuda(entire[gi]),
                       AugmentSampler(rng=np.random.default_rng(4)))
    torch.cuda.synchronize()
    for k in ("x", "code", "mask", "entire_mask"):
        assert same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    assert np.array_equal(a["final_boxes"], b["final_boxes"]) and np.array_equal(a["boxes"], b["boxes"])
    # image-aligned stacks: None, the argument left out, and the image index spelt out are one thing
    al = [cuda(gt[:2]), cuda(masks[:2]), cuda(entire[:2])]
    outs = [cp(cuda(images), ii, boxes, *al), cp(cuda(images), ii, boxes, *al, gt_index=None),
            cp(cuda(images), ii, boxes, *al, gt_index=ii), cp(cuda(images), ii, boxes, *al, gt_index=torch.from_numpy(ii))]
    for o in outs[1:]:
        for k in ("x", "code", "mask", "entire_mask"):
            assert same_bits(o[k].cpu().numpy(), outs[0][k].cpu().numpy()), k
    # only a mask stack, of its own length
    m = cp(cuda(images), ii, boxes, masks=cuda(masks), gt_index=gi)
    assert m["code"] is None and same_bits(m["mask"].cpu().numpy(), a_mask(cp, images, ii, boxes, masks, gi))


def a_mask(cp, images, ii, boxes, masks, gi):
    return cp(cuda(images[ii]), np.arange(len(ii)), boxes, masks=cuda(masks[gi]))["mask"].cpu().numpy()


def test_gt_index_refusals(gpu):
    from zebrapose_amd.crop import CropPipeline
    images, gt, masks, entire, ii, gi, raw = crop_inputs()
    cp = CropPipeline(crop_size_img=32, crop_size_gt=16)
    boxes, _ = cp.boxes(raw, 56, 40)
    im, g, m, e = cuda(images), cuda(gt), cuda(masks), cuda(entire)
    for bad in (dict(gt_index=[0, 1, 2, 3]), dict(gt_index=[0, 1, -1, 2]), dict(gt_index=[0, 1, 2]),
                dict(gt_index=[0.0, 1.0, 2.0, 1.0]), dict(gt_index=[[0, 1, 2, 1]]), dict(masks=m[:2]),
                dict(entire_masks=e[:, :, :-1].contiguous()), dict(gt_images=None, masks=None, entire_masks=None)):
        with pytest.raises(ValueError):
            cp(**dict(dict(images=im, img_index=ii, boxes=boxes, gt_images=g, masks=m, entire_masks=e, gt_index=gi), **bad))
            pytest.fail(f"{list(bad)} was accepted")
    with pytest.raises(ValueError, match="GT images / masks must match the image stack"):
        cp(im, ii, boxes, g, m, e)  # per-instance stacks without gt_index: refused as ever


def test_scene_batcher_feeds_train_batch_and_the_net(gpu):
    """The seam only: a scene batch through train_batch into one forward of the binary net at batch 2."""
    from zebrapose_amd.augment import AugmentSampler
    from zebrapose_amd.crop import CropPipeline
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeNet_Deeplab
    from zebrapose_amd.synth import SceneBatcher
    rs, rc = quad_renderers(True)
    sb = SceneBatcher(rs, rc, backgrounds(), rng=np.random.default_rng(2))
    R = np.tile(np.eye(3), (3, 1, 1))
    t = np.array([[-0.1, 0.0, 2.0], [0.3, 0.0, 1.8], [0.0, 0.1, 2.2]])
    out = sb([1, 2, 2], np.array([0, 0, 1]), R, t, KQ, HQ, WQ, targets=[0, 2])
    assert out["kept"].tolist() == [0, 2] and out["img_index"].tolist() == [0, 1]
    cp = CropPipeline(crop_size_img=64, crop_size_gt=32)
    tb = cp.train_batch(out["images"], out["img_index"], out["raw_boxes"], out["gt_images"], out["masks"],
                        out["entire_masks"], AugmentSampler(rng=np.random.default_rng(4)), gt_index=out["gt_index"])
    assert tuple(tb["x"].shape) == (2, 3, 64, 64) and tuple(tb["code"].shape) == (2, 16, 32, 32)
    assert tb["mask"].any() and tb["code"].any() and (tb["entire_mask"] >= tb["mask"]).all()
    net = BinaryCodeNet_Deeplab(34, 16, 2, concat=True, output_kernel_size=1, precision="fp32").cuda().eval()
    with torch.no_grad():
        m, c = net(tb["x"])
    torch.cuda.synchronize()
    assert m.shape[0] == 2 and c.shape[0] == 2 and bool(torch.isfinite(m).all()) and bool(torch.isfinite(c).all())
