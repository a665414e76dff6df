"""zp_render_shaded through MeshRenderer.render_shaded against its numpy restatement
(tests/shade_ref.py): every byte of the shaded image and of the common outputs, and the bits of
depth, are compared exactly -- no tolerance and no pixels left out -- and the common outputs against
MeshRenderer.render at the same poses."""
import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests import shade_ref as SR
from tests.test_gpu_render import assert_same, rot_xyz
from tests.test_render_host import EYE, K1, QUAD, T0, quad_variants

pytestmark = pytest.mark.gpu

ALL = ("shaded", "color", "depth", "mask", "face")


def dev_shaded(mr, R, t, K, H, W, light, z_near=1e-6, outputs=ALL):
    light = np.asarray(light, np.float64).reshape(-1, 6)
    out = mr.render_shaded(R, t, K, H, W, light=light[:, :3], phong=light[:, 3:], z_near=z_near, outputs=outputs)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def both(v, f, n, rgb, face_bgr, R, t, K, light, H, W, z_near=1e-6, what=""):
    from zebrapose_amd.render import MeshRenderer
    mr = MeshRenderer(v, f, colors=rgb, normals=n) if face_bgr is None else None
    if mr is None:
        mr = MeshRenderer(v, f, face_colors=np.asarray(face_bgr, np.uint8), normals=n)
        mr.vert_rgb = torch.from_numpy(np.ascontiguousarray(rgb)).to(mr.device)
    fb = mr.face_bgr.cpu().numpy()
    dev = dev_shaded(mr, R, t, K, H, W, light, z_near)
    ref = SR.render_shaded(v, f, n, rgb, R, t, K, light, H, W, z_near, face_bgr=fb)
    assert_same(dev, ref, what)
    plain = mr.render(R, t, K, H, W, z_near=z_near, outputs=("color", "depth", "mask", "face"))
    torch.cuda.synchronize()
    assert_same({k: a.cpu().numpy() for k, a in plain.items()}, dev, what + " vs render")
    return dev, mr


@pytest.fixture(scope="module")
def ico2():
    v, f = RR.icosphere(2)
    assert len(f) == 320
    rgb = np.random.default_rng(11).integers(0, 256, (len(v), 3)).astype(np.uint8)
    return v, f, v.copy(), rgb


POSES = dict(
    R=np.stack([rot_xyz(0.1, 0.2, 0.3), rot_xyz(-1.0, 0.5, 2.0), rot_xyz(2.0, -0.7, 0.0)]).reshape(3, 9),
    t=np.array([[0.0, 0.0, 4.0], [0.5, -0.3, 2.5], [-1.5, 0.4, 6.0]]),
    K=np.array([[90.0, 90.0, 32.0, 24.0], [45.0, 50.0, 30.5, 20.25], [160.0, 150.0, 60.0, 20.0]]),
    light=np.array([[400.0, 400.0, -400.0, 0.4, 0.8, 0.3], [-3.0, 1.0, 1.5, 0.35, 0.87, 0.22],
                    [0.2, -5.0, 9.0, 0.5, 0.71, 0.39]]))


def test_icosphere_batch(gpu, ico2):
    v, f, n, rgb = ico2
    p = POSES
    dev, _ = both(v, f, n, rgb, None, p["R"], p["t"], p["K"], p["light"], 48, 64, what="ico2")
    for b in range(3):
        fg = dev["mask"][b] == 255
        assert fg.sum() > 150 and dev["shaded"][b][fg].any() and not dev["shaded"][b][~fg].any()
    assert len(np.unique(dev["shaded"].reshape(-1, 3), axis=0)) > 500  # shaded, not flat


def test_quad_diagonal_follows_the_top_left_winner(gpu):
    rgb = np.array([[200, 10, 10], [10, 200, 10], [10, 10, 200], [200, 200, 10]], np.uint8)
    n = np.tile(np.array([[0, 0, -1]], np.float32), (4, 1))
    light = np.array([[3.0, 2.0, -4.0, 0.4, 0.8, 0.3]])
    for faces, colors, tag in quad_variants():
        dev, _ = both(QUAD, faces, n, rgb, colors, EYE, T0, K1, light, 16, 16, what=f"quad {tag}")
        d = np.arange(2, 12)
        assert (dev["face"][0][d, d] >= 0).all() and dev["shaded"][0][d, d].any(axis=1).all()


def test_back_face_shows_ambient_only(gpu):
    v = np.array([[1.5, 1.5, 2], [9.5, 1.5, 2], [1.5, 9.5, 2]], np.float32)
    rgb = np.array([[255, 128, 64], [255, 128, 64], [255, 128, 64]], np.uint8)
    K2 = np.array([[2.0, 2.0, 0.0, 0.0]])
    # behind the camera, on the axis.  No specular weight: the reference's specular term is not gated by
    # the diffuse one (Rv . Vd can be positive on a back face), so "ambient only" is a statement about d
    light = np.array([[0.0, 0.0, -10.0, 0.4, 0.8, 0.0]])
    for nz, lit in ((-1.0, True), (1.0, False)):  # facing the light and the camera; facing away
        n = np.tile(np.array([[0, 0, nz]], np.float32), (3, 1))
        both(v, np.array([[0, 1, 2]], np.int32), n, rgb, None, EYE, T0, K2, light + [0, 0, 0, 0, 0, 0.3], 12, 12,
             what=f"nz {nz} with specular")
        dev, _ = both(v, np.array([[0, 1, 2]], np.int32), n, rgb, None, EYE, T0, K2, light, 12, 12, what=f"nz {nz}")
        fg = dev["mask"][0] == 255
        assert fg.sum() > 10
        amb = np.rint(255 * (0.4 * (rgb[0][::-1] / 255.0))).astype(np.uint8)
        if lit:
            assert (dev["shaded"][0][fg].astype(int) > amb.astype(int)).all()
        else:
            assert (dev["shaded"][0][fg] == amb).all()


def test_one_zero_normal_vertex(gpu, ico2):
    v, f, n, rgb = ico2
    n = n.copy()
    n[:12] = 0  # the icosahedron's own vertices, spread over the sphere: the faces around each interpolate from a zero corner
    both(v, f, n, rgb, None, POSES["R"][:1], POSES["t"][:1], POSES["K"][:1], POSES["light"][:1], 48, 64, what="zero normal")
    both(v, f, np.zeros_like(n), rgb, None, POSES["R"][:1], POSES["t"][:1], POSES["K"][:1], POSES["light"][:1], 48, 64,
         what="all zero normals")


def test_triangle_behind_z_near_beside_a_visible_one(gpu):
    v = np.array([[1.5, 1.5, 1], [9.5, 1.5, 1], [1.5, 9.5, 1], [3, 3, 0.25], [9.5, 9.5, 1.5]], np.float32)
    rgb = np.random.default_rng(2).integers(0, 256, (5, 3)).astype(np.uint8)
    n = np.tile(np.array([[0.3, 0.1, -1]], np.float32), (5, 1))
    light = np.array([[2.0, -1.0, -3.0, 0.4, 0.8, 0.3]])
    dev, _ = both(v, np.array([[0, 1, 3], [0, 1, 2], [4, 1, 2]], np.int32), n, rgb, None, EYE, T0, K1, light, 12, 12,
                  z_near=0.5, what="z_near")
    fg = dev["mask"][0] == 255
    assert fg.any() and (dev["face"][0][fg] >= 1).all()


def test_shaded_alone_and_twice(gpu, ico2):
    v, f, n, rgb = ico2
    from zebrapose_amd.render import MeshRenderer
    mr = MeshRenderer(v, f, colors=rgb, normals=n)
    p = POSES
    full = dev_shaded(mr, p["R"], p["t"], p["K"], 48, 64, p["light"])
    one = dev_shaded(mr, p["R"][1:2], p["t"][1:2], p["K"][1:2], 48, 64, p["light"][1:2], outputs=("shaded",))
    assert set(one) == {"shaded"}
    np.testing.assert_array_equal(one["shaded"][0], full["shaded"][1])
    again = dev_shaded(mr, p["R"], p["t"], p["K"], 48, 64, p["light"])
    assert_same(again, full, "second run")
    # the default light is the reference's (400, 400, 400) of GL's eye frame
    dflt = mr.render_shaded(p["R"], p["t"], p["K"], 48, 64)
    torch.cuda.synchronize()
    assert set(dflt) == {"shaded", "mask"}
    ref = SR.render_shaded(v, f, n, rgb, p["R"], p["t"], p["K"], np.tile([400.0, 400.0, -400.0, 0.4, 0.8, 0.3], (3, 1)), 48, 64)
    np.testing.assert_array_equal(dflt["shaded"].cpu().numpy(), ref["shaded"])
    bare = MeshRenderer(v, f, colors=rgb)
    with pytest.raises(ValueError):
        bare.render_shaded(p["R"], p["t"], p["K"], 48, 64)
