"""zp_render through zebrapose_amd.render.MeshRenderer against its numpy restatement
(tests/render_ref.py): colour, mask, face index and the bits of depth are compared exactly -- no
tolerance and no pixels left out.  Meshes are built here: an icosphere by subdivision and a
two-colour quad whose diagonal passes through sample points."""
import itertools

import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests.test_render_host import EYE, K1, QUAD, T0, quad_variants

pytestmark = pytest.mark.gpu

ALL = ("color", "depth", "mask", "face")


def dev_render(mr, R, t, K, H, W, z_near=1e-6, outputs=ALL):
    out = mr.render(R, t, K, H, W, z_near=z_near, outputs=outputs)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(dev, ref, what=""):
    for k in dev:
        a, b = dev[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if k == "depth":
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what}: {k} differs at {len(bad)} places, first {bad[0]}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}"


def both(verts, faces, face_bgr, R, t, K, H, W, z_near=1e-6, what=""):
    """Render on the device and with the reference; compare everything; return the two dicts."""
    from zebrapose_amd.render import MeshRenderer
    mr = MeshRenderer(verts, faces, face_colors=np.asarray(face_bgr, np.uint8))
    dev = dev_render(mr, R, t, K, H, W, z_near)
    ref = RR.render(verts, faces, face_bgr, R, t, K, H, W, z_near)
    assert_same(dev, ref, what)
    return dev, ref


def rot_xyz(a, b, c):
    def r(axis, th):
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        S = np.eye(3)
        S[i, i], S[i, j], S[j, i], S[j, j] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
        return S
    return r(0, a) @ r(1, b) @ r(2, c)


def face_colours(nf, seed=0):
    """Distinct random colours, none black."""
    ids = np.random.default_rng(seed).permutation(1 << 24)[:nf] | 1
    return np.stack([ids >> 16, (ids >> 8) & 255, ids & 255], 1).astype(np.uint8)


@pytest.fixture(scope="module")
def ico4():
    v, f = RR.icosphere(4)
    assert len(f) == 5120
    return v, f, face_colours(len(f))


@pytest.fixture(scope="module")
def ico3():
    v, f = RR.icosphere(3)
    return v, f, face_colours(len(f), 1)


# ---- 1. one triangle far larger than the image: the list path and the clip -----------------------------

@pytest.mark.parametrize("xy", [
    [[-1000, -1000], [3000, -1000], [-1000, 3000]],
    # projections beyond the +-2^28 saturation: snapped to (S, S), (-S, S), (S, -S), interior x + y > 0
    [[1e7, 1e7], [-1e7, 1e7], [1e7, -1e7]]], ids=["plain", "saturated"])
def test_triangle_covering_the_image(gpu, xy):
    v = np.concatenate([np.array(xy, np.float32), np.ones((3, 1), np.float32)], 1)
    K = np.array([[10.0, 10.0, 8.0, 6.0]])
    for f in ([[0, 1, 2]], [[0, 2, 1]]):
        assert RR.box_samples(v, f, EYE[0], T0[0], K[0], 12, 16)[0] == 16 * 12
        dev, _ = both(v, np.array(f, np.int32), [[7, 8, 9]], EYE, T0, K, 12, 16, what=f"cover {xy[0]} {f}")
        assert (dev["mask"] == 255).all() and (dev["color"] == [7, 8, 9]).all() and (dev["face"] == 0).all()
        assert (dev["depth"] == 1.0).all()


# ---- 2. shared edge --------------------------------------------------------------------------------

def test_shared_edge_quad(gpu):
    expect = np.zeros((16, 16), bool)
    expect[2:12, 2:12] = True
    for faces, colors, tag in quad_variants():
        dev, _ = both(QUAD, faces, colors, EYE, T0, K1, 16, 16, what=f"quad {tag}")
        np.testing.assert_array_equal(dev["mask"][0] == 255, expect)
        d = np.arange(2, 12)
        assert (dev["face"][0][d, d] >= 0).all()  # every sample on the diagonal has exactly one owner


# ---- 3. order invariance ----------------------------------------------------------------------------

def test_order_invariance(gpu, ico3):
    v = np.array([[1.5, 1.5, 2], [9.5, 1.5, 2], [1.5, 9.5, 2], [0.75, 0.75, 1], [4.75, 0.75, 1], [0.75, 4.75, 1]],
                 np.float32)
    K2 = np.array([[2.0, 2.0, 0.0, 0.0]])
    col = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    # two coincident triangles of different colour: the lower index, whichever colour it carries
    for order in ([0, 1], [1, 0]):
        dev, _ = both(v, np.array([[0, 1, 2], [1, 2, 0]], np.int32), col[order], EYE, T0, K2, 12, 12, what="coincident")
        fg = dev["mask"][0] == 255
        assert fg.sum() > 10 and (dev["face"][0][fg] == 0).all() and (dev["color"][0][fg] == col[order][0]).all()
    # near and far with the same image, in both orders: the near one
    for order in ([0, 1], [1, 0]):
        f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)[order]
        dev, _ = both(v, f, col[order], EYE, T0, K2, 12, 12, what="near/far")
        fg = dev["mask"][0] == 255
        assert (dev["color"][0][fg] == col[1]).all() and (dev["depth"][0][fg] == 1.0).all()
    # a random permutation of an icosphere's faces
    sv, sf, sc = ico3
    R, t, K = rot_xyz(0.3, -0.5, 0.2).reshape(1, 9), np.array([[0.1, -0.05, 3.0]]), np.array([[70.0, 75.0, 31.5, 22.0]])
    a, _ = both(sv, sf, sc, R, t, K, 48, 64, what="sphere")
    perm = np.random.default_rng(5).permutation(len(sf))
    b, _ = both(sv, sf[perm], sc[perm], R, t, K, 48, 64, what="sphere permuted")
    assert (a["mask"] == 255).sum() > 500
    np.testing.assert_array_equal(a["color"], b["color"])
    np.testing.assert_array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
    np.testing.assert_array_equal(perm[b["face"][b["face"] >= 0]], a["face"][a["face"] >= 0])


# ---- 4. icosphere, 5120 faces -------------------------------------------------------------------------

SPHERE_CASES = {
    # name: (H, W, t, K, check on the per-face box sample counts)
    "far_subpixel": (48, 64, [0.2, -0.1, 50.0], [500.0, 500.0, 32.0, 24.0], lambda n: n.max() <= 16 and (n > 0).sum() > 1000),
    "close_list": (120, 160, [0.05, 0.02, 2.0], [400.0, 400.0, 80.0, 60.0], lambda n: (n > 16).sum() > 100),
    "off_screen": (48, 64, [0.0, 0.0, 10.0], [360.0, 360.0, 32.0, 24.0], lambda n: (n > 0).sum() > 500),
    "odd_size": (29, 37, [0.3, 0.1, 20.0], [240.0, 250.0, 17.3, 14.0], lambda n: (n > 0).sum() > 1000),
}


@pytest.mark.parametrize("name", list(SPHERE_CASES))
def test_icosphere(gpu, ico4, name):
    v, f, c = ico4
    H, W, t, K, path_ok = SPHERE_CASES[name]
    R = rot_xyz(0.7, 0.2, -0.4).reshape(1, 9)
    t, K = np.array([t]), np.array([K])
    n = RR.box_samples(v, f, R[0], t[0], K[0], H, W)
    assert path_ok(n), (name, n.max(), (n > 16).sum(), (n > 0).sum())
    dev, _ = both(v, f, c, R, t, K, H, W, what=name)
    fg = dev["mask"][0] == 255
    if name == "far_subpixel":
        assert 200 < fg.sum() < 500      # a disc of radius ~10 px
    if name == "close_list":
        assert fg.all()                   # the sphere fills the image; its faces span 10-30 px
        span = np.sqrt(np.bincount(dev["face"][0].ravel()).max())
        assert 10 <= span <= 30, span
    if name == "off_screen":              # radius ~40 px around the centre of 64 x 48: cut on all four sides
        assert fg[0].any() and fg[-1].any() and fg[:, 0].any() and fg[:, -1].any() and not fg.all()
    if name == "odd_size":
        assert 300 < fg.sum() < H * W and not (fg[0].any() or fg[-1].any())


# ---- 5. discards ---------------------------------------------------------------------------------------

def test_discards(gpu, ico3):
    v = np.array([[1.5, 1.5, 1], [9.5, 1.5, 1], [1.5, 9.5, 1], [3, 3, 0.25], [5.5, 5.5, 1]], np.float32)
    col = [[1, 1, 1]]
    dev, _ = both(v, np.array([[0, 1, 2]], np.int32), col, EYE, T0, K1, 12, 12, z_near=0.5, what="kept")
    assert dev["mask"].any()
    for f in ([[0, 1, 3]], [[0, 4, 0]], [[2, 4, 1]]):  # a vertex behind z_near; zero area, twice
        dev, _ = both(v, np.array(f, np.int32), col, EYE, T0, K1, 12, 12, z_near=0.5, what=f"discard {f}")
        assert not dev["mask"].any() and not dev["color"].any() and not dev["depth"].any() and (dev["face"] == -1).all()
    # one discarded and one kept triangle in one mesh: the kept one is untouched
    dev, _ = both(v, np.array([[0, 1, 3], [0, 1, 2]], np.int32), [[1, 1, 1], [2, 2, 2]], EYE, T0, K1, 12, 12, z_near=0.5)
    assert (dev["face"][dev["mask"] == 255] == 1).all() and dev["mask"].any()
    # a mesh wholly behind the camera
    sv, sf, sc = ico3
    dev, _ = both(sv, sf, sc, EYE, np.array([[0.0, 0.0, -5.0]]), np.array([[100.0, 100.0, 16.0, 12.0]]), 24, 32, what="behind")
    assert not dev["mask"].any() and not dev["color"].any() and not dev["depth"].any() and (dev["face"] == -1).all()


# ---- 6. batching, reproducibility, streams --------------------------------------------------------------

def test_batching_and_streams(gpu, ico3):
    from zebrapose_amd.render import MeshRenderer
    v, f, c = ico3
    R = np.stack([rot_xyz(0.1, 0.2, 0.3), rot_xyz(-1.0, 0.5, 2.0), rot_xyz(2.0, -0.7, 0.0)]).reshape(3, 9)
    t = np.array([[0.0, 0.0, 4.0], [0.5, -0.3, 2.5], [-1.5, 0.4, 6.0]])
    K = np.array([[60.0, 60.0, 20.0, 15.0], [45.0, 50.0, 18.5, 16.25], [110.0, 100.0, 25.0, 12.0]])
    H, W = 30, 40
    mr = MeshRenderer(v, f, face_colors=c)
    full = dev_render(mr, R, t, K, H, W)
    assert_same(full, RR.render(v, f, c, R, t, K, H, W), "batch of 3")
    assert all((full["mask"][b] == 255).sum() > 50 for b in range(3))
    for b in range(3):
        one = dev_render(mr, R[b:b + 1], t[b:b + 1], K[b:b + 1], H, W)
        assert_same(one, {k: a[b:b + 1] for k, a in full.items()}, f"item {b} alone")
    assert_same(dev_render(mr, R, t, K, H, W), full, "second run")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = mr.render(R, t, K, H, W, outputs=ALL)
    side.synchronize()
    assert_same({k: a.cpu().numpy() for k, a in out.items()}, full, "side stream")
    # one K row (or a 3 x 3 camera matrix) serves the whole batch
    Km = np.array([[60.0, 0, 20.0], [0, 60.0, 15.0], [0, 0, 1]])
    assert_same(dev_render(mr, R, t, Km, H, W), dev_render(mr, R, t, np.repeat(K[:1], 3, 0), H, W), "shared K")


# ---- 7. NULL outputs ---------------------------------------------------------------------------------

def test_every_subset_of_outputs(gpu, ico3):
    from zebrapose_amd.render import MeshRenderer
    v, f, c = ico3
    R, t, K = rot_xyz(0.4, 0.1, 0.9).reshape(1, 9), np.array([[0.2, 0.1, 3.0]]), np.array([[50.0, 50.0, 16.0, 12.0]])
    mr = MeshRenderer(v, f, face_colors=c)
    full = dev_render(mr, R, t, K, 24, 32)
    for n in range(1, 4):
        for sub in itertools.combinations(ALL, n):
            part = dev_render(mr, R, t, K, 24, 32, outputs=sub)
            assert set(part) == set(sub)
            assert_same(part, full, f"outputs {sub}")
    # a mesh without colours renders everything but colour
    bare = MeshRenderer(v, f)
    assert_same(dev_render(bare, R, t, K, 24, 32, outputs=("depth", "mask", "face")), full, "no colours")
    with pytest.raises(ValueError):
        bare.render(R, t, K, 24, 32)
    with pytest.raises(ValueError):
        mr.render(R, t[:0], K, 24, 32)


# ---- 8 and 9. meaning, independent of render_ref; into the crop pipeline ------------------------------------

ID0 = 777  # ids ID0 .. ID0 + nf - 1: none is 0 (black is the background), all below 2^16


@pytest.fixture(scope="module")
def id_render(ico3):
    from zebrapose_amd.render import MeshRenderer
    v, f, _ = ico3
    ids = ID0 + np.arange(len(f))
    R = np.stack([rot_xyz(0.9, -0.3, 0.5), rot_xyz(-0.2, 1.1, 0.0)]).reshape(2, 9)
    t = np.array([[0.1, -0.1, 3.0], [-0.6, 0.3, 2.2]])
    K = np.array([[150.0, 150.0, 64.0, 64.0], [140.0, 160.0, 60.0, 70.0]])
    mr = MeshRenderer.from_class_ids(v, f, ids)
    out = mr.render(R, t, K, 128, 128, outputs=ALL)
    torch.cuda.synchronize()
    return v, f, ids, R, t, K, out


def test_rendered_ids_name_the_face_under_the_pixel(gpu, id_render):
    v, f, ids, R, t, K, out = id_render
    color, depth, mask = (out[k].cpu().numpy() for k in ("color", "depth", "mask"))
    np.testing.assert_array_equal(mask, np.where(depth > 0, 255, 0).astype(np.uint8))
    v64 = v.astype(np.float64)
    for b in range(2):
        Rm = R[b].reshape(3, 3)
        cam = v64 @ Rm.T + t[b]
        uv = np.stack([K[b, 0] * cam[:, 0] / cam[:, 2] + K[b, 2], K[b, 1] * cam[:, 1] / cam[:, 2] + K[b, 3]], 1)
        ctr = v64[f].mean(1) @ Rm.T + t[b]
        cuv = np.stack([K[b, 0] * ctr[:, 0] / ctr[:, 2] + K[b, 2], K[b, 1] * ctr[:, 1] / ctr[:, 2] + K[b, 3]], 1)
        ext = uv[f].max(1) - uv[f].min(1)  # [nf, 2]: the face's projected extent
        ys, xs = np.nonzero(mask[b])
        assert len(ys) > 3000
        px = color[b, ys, xs].astype(np.int64)
        face = ((px[:, 0] << 16) | (px[:, 1] << 8) | px[:, 2]) - ID0
        assert face.min() >= 0 and face.max() < len(f)
        centre = np.stack([xs + 0.5, ys + 0.5], 1)
        assert (np.abs(cuv[face] - centre) <= ext[face] + 1.0).all()
        # the depth is the visible (front) surface's: within the face's own Z range, rounding aside
        z = cam[:, 2][f]
        assert (depth[b, ys, xs] >= z.min(1)[face] * (1 - 1e-6)).all() and (depth[b, ys, xs] <= z.max(1)[face] * (1 + 1e-6)).all()
        assert (ctr[face, 2] < t[b, 2]).all()  # front half of the sphere


def test_rendered_stacks_feed_the_crop_pipeline(gpu, id_render):
    from zebrapose_amd.crop import CropPipeline
    v, f, ids, R, t, K, out = id_render
    ref = RR.render(v, f, np.stack([ids >> 16, (ids >> 8) & 255, ids & 255], 1).astype(np.uint8), R, t, K, 128, 128)
    assert out["color"].dtype == torch.uint8 and tuple(out["color"].shape) == (2, 128, 128, 3)
    assert out["mask"].dtype == torch.uint8 and tuple(out["mask"].shape) == (2, 128, 128)
    cp = CropPipeline()
    images = torch.zeros((2, 128, 128, 3), dtype=torch.uint8, device="cuda")
    idx = [0, 1, 0, 1]
    boxes = np.array([[0, 0, 128, 128], [0, 0, 128, 128], [30, 20, 70, 90], [-10, 40, 100, 60]], np.int32)
    a = cp(images, idx, boxes, gt_images=out["color"], entire_masks=out["mask"])
    b = cp(images, idx, boxes, gt_images=torch.from_numpy(ref["color"]).cuda(), entire_masks=torch.from_numpy(ref["mask"]).cuda())
    torch.cuda.synchronize()
    for k in ("code", "entire_mask"):
        np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=k)
    # crops 0 and 1 copy the 128 x 128 render: the 16 planes of a foreground pixel spell its face's id
    code = a["code"].cpu().numpy().astype(np.int64)
    face = out["face"].cpu().numpy()
    for i in range(2):
        spelled = sum(code[i, k] << (15 - k) for k in range(16))
        fg = face[i] >= 0
        assert fg.sum() > 3000
        np.testing.assert_array_equal(spelled[fg], ids[face[i][fg]])
        assert (spelled[~fg] == 0).all()
        np.testing.assert_array_equal(a["entire_mask"][i].cpu().numpy(), fg.astype(np.float32))
