"""Host side of the shaded renderer and the compositor: sanity of the numpy restatements
(tests/shade_ref.py, tests/synth_ref.py) that pin the kernels, bg_geometry on a hand-worked table,
read_ply's normals and vertex_normals.  No GPU."""
import os
import struct

import numpy as np
import pytest

from oracle import crop_ref
from tests import render_ref as RR
from tests import shade_ref as SR
from tests import synth_ref as YR

K = np.array([[40.0, 40.0, 16.0, 12.0]])
R0 = np.eye(3).reshape(1, 9)
T3 = np.array([[0.0, 0.0, 3.0]])


def sphere(seed=0):
    v, f = RR.icosphere(1)
    rgb = np.random.default_rng(seed).integers(1, 256, (len(v), 3)).astype(np.uint8)
    return v, f, v.copy(), rgb


# ---- shade_ref ---------------------------------------------------------------------------------

def test_ambient_only_is_the_interpolated_colour():
    v, f, n, rgb = sphere()
    rgb[:] = rgb[0]  # one colour: interpolation returns it up to rounding, so the byte is rint(255 ka c)
    light = np.array([[400.0, 400.0, -400.0, 0.4, 0.0, 0.0]])  # 0.4 c is never a half: no ties
    out = SR.render_shaded(v, f, n, rgb, R0, T3, K, light, 24, 32)
    fg = out["mask"][0] == 255
    assert fg.sum() > 100 and not out["shaded"][0][~fg].any()
    expect = np.rint(255.0 * (0.4 * (rgb[0].astype(np.float64) / 255.0)))[::-1].astype(np.uint8)
    assert (out["shaded"][0][fg] == expect).all()


def test_zero_normals_give_ambient_only():
    v, f, n, rgb = sphere(1)
    light = np.array([[1.0, -2.0, 0.5, 0.4, 0.8, 0.3]])
    full = SR.render_shaded(v, f, n, rgb, R0, T3, K, light, 24, 32)["shaded"]
    flat = SR.render_shaded(v, f, np.zeros_like(n), rgb, R0, T3, K, light, 24, 32)["shaded"]
    amb = SR.render_shaded(v, f, n, rgb, R0, T3, K, light * [1, 1, 1, 1, 0, 0], 24, 32)["shaded"]
    np.testing.assert_array_equal(flat, amb)
    assert (full != amb).any()


def test_light_on_a_vertex_gives_no_nan():
    v, f, n, rgb = sphere(2)
    P = v[f[0, 0]].astype(np.float64) + T3[0]  # R = I: the vertex's camera-space position, exactly
    light = np.array([[P[0], P[1], P[2], 0.4, 0.8, 0.3]])
    _, _, Lv = SR.vertex_attributes(v, n, R0[0], T3[0], light[0])
    assert np.isfinite(Lv).all() and not Lv[f[0, 0]].any()
    with np.errstate(invalid="raise"):
        out = SR.render_shaded(v, f, n, rgb, R0, T3, K, light, 24, 32)
    assert out["shaded"][0][out["mask"][0] == 255].any()


def test_lit_side_is_brighter():
    """Meaning, independent of the formulas: a grey sphere lit from the left is brighter on its left."""
    v, f, n, _ = sphere()
    rgb = np.full((len(v), 3), 128, np.uint8)
    light = np.array([[-50.0, 0.0, 3.0, 0.2, 0.8, 0.0]])
    sh = SR.render_shaded(v, f, n, rgb, R0, T3, K, light, 24, 32)["shaded"][0].astype(np.int64)
    assert sh[12, 6, 0] > sh[12, 25, 0] and sh[12, 25, 0] == round(255 * 0.2 * (128 / 255))


# ---- bg_geometry ---------------------------------------------------------------------------------

@pytest.mark.parametrize("args, expect", [
    # image 24 x 40, H / W = 0.6.  Wide background, the image's own orientation (first branch of
    # get_bg_image): ceil(30 / 0.6) = 50 columns kept; f = 24 / 30; 50 f = 40 does not pass max_size
    ((30, 50, 24, 40), (50, 30, 40, 24, 24 / 30)),
    # tall background under a wide image (the other branch): ceil(30 * 0.6) = 18 rows; f = 24 / 18
    ((50, 30, 24, 40), (30, 18, 40, 24, 24 / 18)),
    # exactly 2x: the whole 48 x 80 background, f = 1/2
    ((48, 80, 24, 40), (80, 48, 40, 24, 0.5)),
    # max_size: ceil(4 / 0.6) = 7 columns; f = 24 / 4 = 6 gives round(42) > 40, so f = 40 / 7 and the
    # short side comes to rint(4 * 40 / 7 = 22.86) = 23 rows: a row short of the image
    ((4, 7, 24, 40), (7, 4, 40, 23, 40 / 7)),
    # a tall image, 40 x 24 (H / W = 5/3): wide background, ceil(30 / (5/3)) = 18 columns
    ((30, 50, 40, 24), (18, 30, 24, 40, 24 / 18)),
    # a tall background that is not tall enough: ceil(30 * 5/3) = 50 rows asked, 40 there are; f = 24 / 30
    ((40, 30, 40, 24), (30, 40, 24, 32, 0.8)),
    # same size: a copy
    ((24, 40, 24, 40), (40, 24, 40, 24, 1.0)),
])
def test_bg_geometry_table(args, expect):
    from zebrapose_amd.synth import bg_geometry
    got = bg_geometry(*args)
    assert got[:4] == expect[:4] and got[4] == expect[4], (args, got)


def test_bg_geometry_never_exceeds_the_image_itself():
    """The crop takes the image's orientation, its short side comes to min(H, W) and the max_size rule
    bounds the long one, so bg_geometry's own output fits the image; zp_composite's rule for a
    resized side beyond the image (dropped) is reached by a caller's geometry, below."""
    from zebrapose_amd.synth import bg_geometry
    r = np.random.default_rng(0)
    for bh, bw, H, W in r.integers(1, 700, (4000, 4)):
        try:
            cw, ch, ow, oh, f = bg_geometry(bh, bw, H, W)
        except ValueError:
            continue
        assert ow <= W and oh <= H and cw <= bw and ch <= bh


def test_background_beyond_the_image_is_dropped():
    bg = np.random.default_rng(3).integers(0, 256, (30, 50, 3)).astype(np.uint8)
    f = 0.9  # out 45 x 27 over an image of 40 x 24
    full = YR.resize_linear_u8(bg, 45, 27, f)
    got = YR.background(bg, (50, 30, 45, 27), f, 24, 40)
    np.testing.assert_array_equal(got, full[:24, :40])
    short = YR.background(bg, (50, 30, 20, 12), 0.4, 24, 40)  # and one that falls short: zeros beyond
    assert not short[12:].any() and not short[:, 20:].any() and short[:12, :20].any()


# ---- synth_ref's resize against the crop oracle's ----------------------------------------------------

@pytest.mark.parametrize("n, d", [(30, 24), (18, 24), (48, 24), (24, 24), (7, 40), (50, 16), (31, 17), (17, 31)])
def test_resize_matches_the_crop_oracle(n, d):
    """Square inputs, where cv_resize_linear_u8 applies: its scale is 1 / (d / n), ours 1 / f; they are
    compared wherever the two are the same number."""
    f = d / n
    assert 1.0 / f == 1.0 / (d / n)
    roi = np.random.default_rng(n * 100 + d).integers(0, 256, (n, n, 3)).astype(np.uint8)
    np.testing.assert_array_equal(YR.resize_linear_u8(roi, d, d, f), crop_ref.cv_resize_linear_u8(roi, d))


def test_area_path_on_an_odd_side():
    src = np.array([[[10], [20], [31]], [[30], [40], [50]], [[1], [2], [4]]], np.uint8)  # 3 x 3, f = 1/2 -> 2 x 2
    out = YR.resize_linear_u8(src, 2, 2, 0.5)[..., 0]
    # full block (10 + 20 + 30 + 40 + 2) >> 2; right column 31, 50: 40.5 -> 40; bottom row 1, 2: 1.5 -> 2; corner 4
    np.testing.assert_array_equal(out, [[25, 40], [2, 4]])


def test_truncation_modes():
    m = np.zeros((24, 40), np.uint8)
    m[4:20, 10:31] = 255  # rows 4..19, columns 10..30
    bb = YR.mask_bbox(m[None])[0]
    assert tuple(bb) == (4, 10, 19, 30)
    keep = lambda rnd, u: YR.truncate(m, bb, rnd, u)
    assert keep(0.1, 0.5)[:, 15].nonzero()[0].min() == int(4 + (11.5 - 4) * 0.5)       # rows below 7 cleared
    assert keep(0.3, 0.5)[:, 15].nonzero()[0].max() == int(11.5 + (19 - 11.5) * 0.5) - 1
    assert keep(0.5, 0.5)[10].nonzero()[0].min() == int(10 + (20.0 - 10) * 0.5)
    assert keep(0.7, 0.5)[10].nonzero()[0].max() == int(20.0 + (30 - 20.0) * 0.5) - 1
    for rnd in (0.8, 0.95, -1.0):
        np.testing.assert_array_equal(keep(rnd, 0.5), m != 0)
    e = np.zeros((24, 40), np.uint8)
    assert tuple(YR.mask_bbox(e[None])[0]) == (0, 0, -1, -1) and not YR.truncate(e, (0, 0, -1, -1), 0.1, 0.5).any()


# ---- read_ply normals, vertex_normals ---------------------------------------------------------------

PV = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], np.float32)
PN = np.array([[0, 0, -1], [1, 0, 0], [0, 1, 0], [0.6, 0, 0.8]], np.float32)
PC = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [250, 251, 252]], np.uint8)
PF = np.array([[0, 1, 2], [0, 1, 3]], np.int32)


def _write(path, binary, with_normals):
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", f"element vertex {len(PV)}",
            "property float x", "property float y", "property float z"]
    if with_normals:
        head += ["property float nx", "property float ny", "property float nz"]
    head += ["property uchar red", "property uchar green", "property uchar blue", f"element face {len(PF)}",
             "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        for i in range(len(PV)):
            vals = list(PV[i]) + (list(PN[i]) if with_normals else [])
            if binary:
                fh.write(struct.pack(f"<{len(vals)}f3B", *vals, *PC[i]))
            else:
                fh.write((" ".join(repr(float(x)) for x in vals) + " " + " ".join(str(int(c)) for c in PC[i]) + "\n").encode())
        for f in PF:
            fh.write(struct.pack("<B3i", 3, *f) if binary else ("3 " + " ".join(str(int(i)) for i in f) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True], ids=["ascii", "binary"])
def test_read_ply_normals(tmp_path, binary):
    from zebrapose_amd.render import read_ply
    p = os.path.join(tmp_path, "n.ply")
    _write(p, binary, True)
    m = read_ply(p, normals=True)
    assert m["normals"].dtype == np.float32
    np.testing.assert_array_equal(m["normals"], PN)
    np.testing.assert_array_equal(m["vertices"], PV)
    np.testing.assert_array_equal(m["colors"], PC)
    np.testing.assert_array_equal(m["faces"], PF)
    assert sorted(read_ply(p)) == ["colors", "faces", "vertices"]  # the default call returns what it always did
    _write(p, binary, False)
    assert read_ply(p, normals=True)["normals"] is None and sorted(read_ply(p)) == ["colors", "faces", "vertices"]


def test_vertex_normals_of_an_icosphere():
    from zebrapose_amd.render import vertex_normals
    # the icosahedron (level 0): every vertex has five-fold symmetry, so its area-weighted normal is
    # radial exactly; a subdivided sphere's vertices are not that symmetric (level 3 is 1e-2 off radial)
    v, f = RR.icosphere(0)
    n = vertex_normals(v, f)
    assert n.dtype == np.float32 and n.shape == v.shape
    u = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(n - u).max() < 1e-6
    v3, f3 = RR.icosphere(3)  # outward everywhere on the finer sphere, unit length
    n3 = vertex_normals(v3, f3).astype(np.float64)
    assert ((n3 * v3).sum(1) > 0.99).all() and np.abs(np.linalg.norm(n3, axis=1) - 1).max() < 1e-6
    # a vertex no face uses keeps a zero normal
    n2 = vertex_normals(np.concatenate([v, [[5, 5, 5]]]), f)
    assert not n2[-1].any()
