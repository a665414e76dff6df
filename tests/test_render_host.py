"""Host side of the GT renderer (no GPU): the numpy restatement tests/render_ref.py obeys the
properties zp_render's contract names (shared edges covered exactly once, nearest wins, ties to the
lowest face), read_ply round-trips, modified_gt_for_symmetry picks the symmetric pose nearest the
identity, and zp_render's argument checks fail cleanly before any device call."""
import ctypes
import itertools
import os
import struct

import numpy as np
import pytest

from tests import render_ref as RR

# Z = 1, fx = fy = 1, cx = cy = 0: u = x, v = y exactly, so half-integer vertices snap exactly
EYE = np.eye(3).reshape(1, 9)
T0 = np.zeros((1, 3))
K1 = np.array([[1.0, 1.0, 0.0, 0.0]])

# a quad whose diagonal (2.5, 2.5) - (12.5, 12.5) passes through the sample points (i + 1/2, i + 1/2)
QUAD = np.array([[2.5, 2.5, 1], [12.5, 2.5, 1], [12.5, 12.5, 1], [2.5, 12.5, 1]], np.float32)
QUAD_TRIS = [(0, 1, 2), (0, 2, 3)]


def quad_variants():
    """Both windings of each triangle and both face orders."""
    for flip0, flip1, swap in itertools.product((0, 1), (0, 1), (0, 1)):
        tris = [QUAD_TRIS[0][::-1] if flip0 else QUAD_TRIS[0], QUAD_TRIS[1][::-1] if flip1 else QUAD_TRIS[1]]
        colors = [[10, 20, 30], [40, 50, 60]]
        if swap:
            tris, colors = tris[::-1], colors[::-1]
        yield np.array(tris, np.int32), np.array(colors, np.uint8), (flip0, flip1, swap)


def test_ref_shared_edge_covered_exactly_once():
    expect = np.zeros((16, 16), bool)
    expect[2:12, 2:12] = True  # samples 2.5 .. 11.5; those at 12.5 lie on the right / bottom edges
    for faces, colors, tag in quad_variants():
        both = RR.render(QUAD, faces, colors, EYE, T0, K1, 16, 16)
        np.testing.assert_array_equal(both["mask"][0] == 255, expect, err_msg=str(tag))
        a = RR.render(QUAD, faces[:1], colors[:1], EYE, T0, K1, 16, 16)["mask"][0] == 255
        b = RR.render(QUAD, faces[1:], colors[1:], EYE, T0, K1, 16, 16)["mask"][0] == 255
        assert not (a & b).any(), f"{tag}: a sample on the diagonal is covered twice"
        np.testing.assert_array_equal(a | b, expect, err_msg=f"{tag}: a sample on the diagonal is not covered")
        d = np.arange(2, 12)
        assert (a[d, d] ^ b[d, d]).all()
        # the colour of each pixel is its owner's
        own = np.where(a[..., None], colors[0], np.where(b[..., None], colors[1], 0))
        np.testing.assert_array_equal(both["color"][0], own)


def test_ref_depth_and_ties():
    v = np.array([[1.5, 1.5, 2], [9.5, 1.5, 2], [1.5, 9.5, 2],     # far, Z = 2
                  [0.75, 0.75, 1], [4.75, 0.75, 1], [0.75, 4.75, 1]], np.float32)  # near, Z = 1: same image
    col = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    for order in ([0, 1], [1, 0]):
        f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)[order]
        o = RR.render(v, f, col[order], EYE, T0, np.array([[2.0, 2.0, 0.0, 0.0]]), 12, 12)
        fg = o["mask"][0] == 255
        assert fg.sum() > 10
        assert (o["depth"][0][fg] == 1.0).all() and (o["depth"][0][~fg] == 0).all()
        assert (o["color"][0][fg] == col[1]).all()
        assert (o["face"][0][fg] == order.index(1)).all() and (o["face"][0][~fg] == -1).all()
    # coincident triangles: the lower face index
    f = np.array([[0, 1, 2], [0, 1, 2], [1, 2, 0]], np.int32)
    o = RR.render(v, f, np.array([[9, 9, 9], [7, 7, 7], [5, 5, 5]], np.uint8), EYE, T0, K1, 12, 12)
    fg = o["mask"][0] == 255
    assert fg.any() and (o["face"][0][fg] == 0).all() and (o["color"][0][fg] == 9).all()
    assert (o["depth"][0][fg] == 2.0).all()


def test_ref_discards():
    v = np.array([[1.5, 1.5, 1], [9.5, 1.5, 1], [1.5, 9.5, 1], [3, 3, 0.25], [5.5, 5.5, 1]], np.float32)
    col = np.array([[1, 1, 1]], np.uint8)
    assert RR.render(v, [[0, 1, 2]], col, EYE, T0, K1, 12, 12)["mask"].any()
    for f in ([[0, 1, 3]], [[0, 4, 0]], [[2, 4, 1]], [[0, 1, 7]]):  # behind z_near, zero area (twice), bad index
        assert not RR.render(v, f, col, EYE, T0, K1, 12, 12, z_near=0.5)["mask"].any(), f


# ---- read_ply -------------------------------------------------------------------------------------

MESH_V = np.array([[0, 0, 0], [1.5, 0, 0.25], [0, -2, 1e-3], [3, 4, 5]], np.float32)
MESH_C = np.array([[255, 0, 1], [2, 3, 4], [5, 6, 7], [8, 9, 250]], np.uint8)
MESH_F = np.array([[0, 1, 2], [2, 1, 3]], np.int32)


def _write_ply(path, binary, faces=MESH_F, colors=True, double=False, extra=False):
    ft = "double" if double else "float"
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "comment written by the test",
            f"element vertex {len(MESH_V)}", f"property {ft} x", f"property {ft} y", f"property {ft} z"]
    if extra:
        head += ["property float nx"]
    if colors:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        for i, p in enumerate(MESH_V):
            c = MESH_C[i]
            if binary:
                fh.write(struct.pack("<3d" if double else "<3f", *p))
                if extra:
                    fh.write(struct.pack("<f", 0.5))
                if colors:
                    fh.write(struct.pack("<3B", *c))
            else:
                vals = [repr(float(x)) for x in p] + (["0.5"] if extra else []) + ([str(int(x)) for x in c] if colors else [])
                fh.write((" ".join(vals) + "\n").encode())
        for f in faces:
            if binary:
                fh.write(struct.pack(f"<B{len(f)}i", len(f), *f))
            else:
                fh.write((" ".join(str(int(x)) for x in [len(f), *f]) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("double,extra,colors", [(False, False, True), (True, True, True), (False, False, False)])
def test_read_ply_round_trip(tmp_path, binary, double, extra, colors):
    from zebrapose_amd.render import read_ply
    p = os.path.join(tmp_path, "m.ply")
    _write_ply(p, binary, colors=colors, double=double, extra=extra)
    m = read_ply(p)
    assert m["vertices"].dtype == np.float32 and m["faces"].dtype == np.int32
    np.testing.assert_array_equal(m["vertices"], MESH_V)
    np.testing.assert_array_equal(m["faces"], MESH_F)
    if colors:
        assert m["colors"].dtype == np.uint8
        np.testing.assert_array_equal(m["colors"], MESH_C)
    else:
        assert m["colors"] is None


@pytest.mark.parametrize("binary", [False, True])
def test_read_ply_rejects_quads_and_other_files(tmp_path, binary):
    from zebrapose_amd.render import read_ply
    p = os.path.join(tmp_path, "q.ply")
    _write_ply(p, binary, faces=[[0, 1, 2, 3]])
    with pytest.raises(ValueError, match="triangles"):
        read_ply(p)
    _write_ply(p, binary, faces=[[0, 1, 2], [0, 1, 2, 3]])
    with pytest.raises(ValueError, match="triangles"):
        read_ply(p)
    _write_ply(p, binary, faces=[[0, 1, 9]])
    with pytest.raises(ValueError, match="index"):
        read_ply(p)
    with open(p, "wb") as fh:
        fh.write(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="format"):
        read_ply(p)
    with open(p, "wb") as fh:
        fh.write(b"solid stl\n")
    with pytest.raises(ValueError, match="PLY"):
        read_ply(p)


# ---- modified_gt_for_symmetry -------------------------------------------------------------------

def _rot(axis, th):
    c, s = np.cos(th), np.sin(th)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    S = np.eye(3)
    S[i, i], S[i, j], S[j, i], S[j, j] = c, -s, s, c
    return S


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _sym4(S, s):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = S, s
    return m.reshape(-1).tolist()


def _fro(R):
    return np.linalg.norm(R - np.eye(3))


POSES = [(_random_rotation(np.random.default_rng(s)), np.random.default_rng(100 + s).standard_normal(3) * 50)
         for s in range(12)]
# discrete symmetries with translations (an object whose symmetry axis misses the model origin)
DISC = [(_rot(2, np.pi), np.array([4.0, -2.0, 0.0])), (_rot(0, np.pi), np.array([0.0, 1.0, 6.0])),
        (_rot(2, np.pi) @ _rot(0, np.pi), np.array([4.0, -3.0, -6.0]))]


def test_symmetry_discrete_is_group_member_and_minimal():
    from zebrapose_amd.render import modified_gt_for_symmetry
    info = {"symmetries_discrete": [_sym4(S, s) for S, s in DISC]}
    members = [(np.eye(3), np.zeros(3))] + DISC
    picked = set()
    for R, t in POSES:
        R2, t2 = modified_gt_for_symmetry(R, t, info)
        hit = [k for k, (S, s) in enumerate(members)
               if np.allclose(R2, R @ S, atol=1e-12) and np.allclose(t2, R @ s + t, atol=1e-9)]
        assert len(hit) == 1, "the result is not the input composed with one listed symmetry"
        picked.add(hit[0])
        assert all(_fro(R2) <= _fro(R @ S) for S, _ in members)
    assert len(picked) > 1  # the poses exercise more than the identity
    # column-vector translations keep their shape (the reference passes cam_t_m2c as [3, 1])
    R2, t2 = modified_gt_for_symmetry(POSES[0][0], POSES[0][1].reshape(3, 1), info)
    assert t2.shape == (3, 1)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_symmetry_continuous_is_axis_rotation_and_minimal(axis):
    from zebrapose_amd.render import modified_gt_for_symmetry
    ax = [0, 0, 0]
    ax[axis] = 1
    info = {"symmetries_continuous": [{"axis": ax, "offset": [0, 0, 0]}]}
    n = 3600
    h = 2 * np.pi / n
    # The sampling step's effect on the norm.  With S(th) the rotation by th about the axis a and (i, j)
    # the other two axes, n(th)^2 = ||R S(th) - I||_F^2 = 6 - 2 tr(R S(th)) = 6 - 2 (R_aa + A cos(th - th*)).
    # tr(R S) lies in [-1, 3] for every th, so R_aa + A <= 3 and R_aa - A >= -1, hence A <= 2.  At distance d
    # from the optimum th*: n(th)^2 - n(th*)^2 = 2 A (1 - cos d) <= A d^2 <= 2 d^2, so
    # n(th) <= sqrt(n(th*)^2 + 2 d^2) <= n(th*) + sqrt(2) d.  Some sample lies within d = h / 2 of th*, so
    # the best sample is above the true minimum by at most sqrt(2) h / 2.  The result, being the exact
    # minimiser over the axis rotations, exceeds no sample (up to rounding, 1e-12) and undercuts the best
    # sample by no more than that margin.
    margin = np.sqrt(2) * h / 2
    for R, t in POSES:
        R2, t2 = modified_gt_for_symmetry(R, t, info)
        np.testing.assert_array_equal(np.asarray(t2), t)  # zero offset: the translation stays
        S = R.T @ R2                                      # the group element applied
        assert np.allclose(S @ S.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(S) - 1) < 1e-12
        e = np.zeros(3)
        e[axis] = 1
        assert np.allclose(S @ e, e, atol=1e-12), "not a rotation about the symmetry axis"
        samples = np.array([_fro(R @ _rot(axis, k * h)) for k in range(n)])
        assert _fro(R2) <= samples.min() + 1e-12
        assert _fro(R2) >= samples.min() - margin - 1e-12


def test_symmetry_continuous_z_with_discrete():
    from zebrapose_amd.render import modified_gt_for_symmetry
    flip = (_rot(0, np.pi), np.array([0.0, 0.0, 10.0]))  # a cylinder's end-over-end flip about an offset centre
    info = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}],
            "symmetries_discrete": [_sym4(*flip)]}
    n = 3600
    h = 2 * np.pi / n
    used = set()
    for R, t in POSES:
        R2, t2 = modified_gt_for_symmetry(R, t, info)
        # group membership: (identity or the flip) followed by a rotation about z
        ok = []
        for k, (S, s) in enumerate([(np.eye(3), np.zeros(3)), flip]):
            Z = (R @ S).T @ R2
            if np.allclose(Z @ [0, 0, 1], [0, 0, 1], atol=1e-12) and np.allclose(Z @ Z.T, np.eye(3), atol=1e-12) \
                    and np.allclose(t2, R @ s + t, atol=1e-9):
                ok.append(k)
        assert len(ok) == 1
        used.add(ok[0])
        best = min(_fro(R @ S @ _rot(2, k * h)) for S, _ in [(np.eye(3), None), flip] for k in range(n))
        assert _fro(R2) <= best + 1e-12
    assert used == {0, 1}


def test_symmetry_none_and_unsupported():
    from zebrapose_amd.render import modified_gt_for_symmetry
    R, t = POSES[3]
    R2, t2 = modified_gt_for_symmetry(R, t, {"diameter": 100.0})
    np.testing.assert_array_equal(R2, R)
    np.testing.assert_array_equal(t2, t)
    with pytest.raises(NotImplementedError):
        modified_gt_for_symmetry(R, t, {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 1]}]})
    with pytest.raises(NotImplementedError):
        modified_gt_for_symmetry(R, t, {"symmetries_continuous": [{"axis": [1, 0, 0], "offset": [0, 0, 0]}],
                                        "symmetries_discrete": [_sym4(*DISC[0])]})


def test_face_colours_from_ids_and_vertex_colours():
    from zebrapose_amd.render import face_bgr_from_ids
    fb = face_bgr_from_ids([0, 1, 0x1234, 0xABCDEF])
    np.testing.assert_array_equal(fb, [[0, 0, 0], [0, 0, 1], [0, 0x12, 0x34], [0xAB, 0xCD, 0xEF]])
    ids = (fb[:, 0].astype(int) << 16) | (fb[:, 1].astype(int) << 8) | fb[:, 2]  # zp_crop_gt's reading
    np.testing.assert_array_equal(ids, [0, 1, 0x1234, 0xABCDEF])
    with pytest.raises(ValueError):
        face_bgr_from_ids([1 << 24])


# ---- zp_render argument checks (no device call is reached) ---------------------------------------------

def test_zp_render_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    lib = _lib.lib
    assert lib.zp_render_ws_bytes(2, 100, 50, 48, 64) >= 2 * 48 * 64 * 8 + 2 * 100 * 16 + 2 * 50 * 4
    assert lib.zp_render_ws_bytes(0, 100, 50, 48, 64) == -1 and lib.zp_render_ws_bytes(1, 1, 1, 1 << 16, 1 << 16) == -1
    buf = (ctypes.c_double * 64)()  # stands in for every pointer: the checks fail before any of them is used
    p = ctypes.addressof(buf)
    good = dict(B=1, verts=p, nv=3, faces=p, nf=1, face_bgr=p, R=p, t=p, K=p, H=8, W=8, z_near=0.1, color=p, depth=p,
                mask=p, face_out=p, ws=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.zp_render(*[a[k] for k in good])

    for bad, word in [(dict(B=0), b"B 0"), (dict(nv=0), b"nv 0"), (dict(nf=-1), b"nf -1"), (dict(H=0), b"H 0"),
                      (dict(W=0), b"W 0"), (dict(H=1 << 20), b"range"), (dict(z_near=0.0), b"z_near"),
                      (dict(z_near=float("nan")), b"z_near"), (dict(verts=None), b"NULL"), (dict(faces=None), b"NULL"),
                      (dict(R=None), b"NULL"), (dict(t=None), b"NULL"), (dict(K=None), b"NULL"), (dict(ws=None), b"NULL"),
                      (dict(face_bgr=None), b"face_bgr")]:
        assert call(**bad) == 1, bad
        assert word in lib.zp_last_error(), (bad, lib.zp_last_error())
    # no output asked for: nothing to do, and nothing is launched
    assert call(color=None, depth=None, mask=None, face_out=None) == 0
