"""Host side of the mesh coder (no GPU): the numpy restatement tests/meshcode_ref.py obeys the
properties zp_mesh_code's contract names (balanced children, prefix ids, the face rule, the ordered
LUT means, separated blobs, identical points), the LUT / PLY writers round-trip through
read_lut_file / read_ply, and zp_mesh_code's argument checks fail cleanly before any device call."""
import ctypes

import numpy as np
import pytest

from tests import meshcode_ref as MR


def check_invariants(verts, faces, bits, res):
    nv = len(verts)
    levels = res["levels"]
    prev = np.zeros(nv, np.int64)
    for l, gid in enumerate(levels):
        assert np.array_equal(gid >> 1, prev), f"level {l}: ids are no prefixes"
        n_parent = np.bincount(prev, minlength=1 << l)
        n_child = np.bincount(gid, minlength=2 << l).reshape(-1, 2)
        assert np.array_equal(np.sort(n_child, axis=1), np.stack([n_parent // 2, (n_parent + 1) // 2], 1)), f"level {l}"
        prev = gid
    leaf = np.bincount(res["vertex_ids"], minlength=1 << bits)
    assert leaf.min() >= nv >> bits and leaf.max() <= -(-nv >> bits)
    assert np.array_equal(res["vertex_ids"], levels[-1])
    # the LUT: ordered f64 mean per class, NaN exactly where no face has the class
    fid, lut = res["face_ids"], res["lut"]
    assert np.array_equal(fid, MR.face_ids_from(res["vertex_ids"], faces))
    present = np.zeros(1 << bits, bool)
    present[fid] = True
    assert np.array_equal(np.isnan(lut).any(1), ~present) and np.array_equal(np.isnan(lut).all(1), ~present)
    v64 = verts.astype(np.float64)
    for c in np.flatnonzero(present)[:: max(1, int(present.sum()) // 40)]:
        s = np.zeros(3)
        fs = np.flatnonzero(fid == c)
        for f in fs:
            for j in range(3):
                s = s + v64[faces[f, j]]
        assert np.array_equal(lut[c], s / float(3 * len(fs))), c


@pytest.fixture(scope="module")
def sphere9():
    v, f = MR.icosphere(3)
    assert len(v) == 642
    return v, f, MR.encode(v, f, 9, return_levels=True)


def test_ref_invariants_icosphere(sphere9):
    v, f, res = sphere9
    check_invariants(v, f, 9, res)


def test_ref_invariants_lattice_with_ties():
    v, f = MR.lattice()
    check_invariants(v, f, 6, MR.encode(v, f, 6, return_levels=True))


def test_ref_same_seed_same_result_other_seed_same_invariants(sphere9):
    v, f, res = sphere9
    again = MR.encode(v, f, 9)
    for k in ("vertex_ids", "face_ids"):
        assert np.array_equal(res[k], again[k])
    assert np.array_equal(res["lut"].view(np.int64), again["lut"].view(np.int64))
    other = MR.encode(v, f, 9, seed=7, return_levels=True)
    assert not np.array_equal(MR.sample_draws(0, 3, 9), MR.sample_draws(7, 3, 9))
    check_invariants(v, f, 9, other)


def test_ref_face_rule_table():
    vid = np.array([5, 5, 5, 6, 7, 8])
    faces = np.array([[0, 1, 2],   # all equal -> i0
                      [0, 1, 3],   # i0 == i1 -> i0
                      [0, 3, 1],   # i0 == i2 -> i0
                      [3, 0, 1],   # i1 == i2 -> i1
                      [3, 4, 5]])  # all differ -> i0
    assert MR.face_ids_from(vid, faces).tolist() == [5, 5, 5, 5, 6]


@pytest.mark.parametrize("count", [2, 4])
def test_ref_blobs_are_separated_by_the_leading_bits(count):
    v, f, blob = MR.blobs(count)
    bits = 3
    res = MR.encode(v, f, bits)
    lead = res["vertex_ids"] >> (bits - (1 if count == 2 else 2))
    for b in range(count):
        assert len(np.unique(lead[blob == b])) == 1
    assert len(np.unique(lead)) == count


def test_ref_identical_points_split_by_the_tie_rule():
    v, f = MR.duplicate_mesh()
    res = MR.encode(v, f, 7, return_levels=True)
    check_invariants(v, f, 7, res)
    # the 64 copies end in leaves of one or two vertices like everything else
    assert np.bincount(res["vertex_ids"][:64], minlength=128).max() <= 2
    # a group of identical points alone: c0 == c1, class 1 stays empty, the first n // 2 by index keep class 0
    pts = np.zeros((6, 3), np.int64)
    lv = MR.split_levels(pts, 1, MR.sample_draws(0, 3, 1), 10, 0)
    assert lv[0].tolist() == [0, 0, 0, 1, 1, 1]
    lv = MR.split_levels(np.zeros((5, 3), np.int64), 1, MR.sample_draws(0, 3, 1), 10, 0)
    assert lv[0].tolist() == [0, 0, 1, 1, 1]


def test_grid_and_eps_match_the_package():
    from zebrapose_amd import meshcode as MC
    rng = np.random.default_rng(1)
    for scale in (1e-3, 1.0, 77.7, 5e4, 2.0 ** 19 - 1, 2.0 ** 19):
        v = (rng.uniform(-1, 1, (50, 3)) * scale).astype(np.float32)
        k = MR.grid_log2(v)
        assert MC.grid_log2(v) == k
        q = np.abs(np.rint(np.ldexp(v.astype(np.float64), k))).max()
        assert q <= MR.SAT and np.abs(np.rint(np.ldexp(v.astype(np.float64), k + 1))).max() > MR.SAT
        for eps in (0.0, 1.0, 0.3, 1e30):
            assert MC.eps_to_grid(eps, k) == MR.eps2_q(eps, k)
    assert MR.eps2_q(1.0, 3) == 64 and MR.eps2_q(0.3, 0) == 0 and MR.eps2_q(1.5, 1) == 9


# ---- writers ---------------------------------------------------------------------------------

def as_mesh_code(v, f, bits, res):
    import torch
    from zebrapose_amd.meshcode import MeshCode
    return MeshCode(v, f, bits, torch.from_numpy(res["vertex_ids"]), torch.from_numpy(res["face_ids"]),
                    torch.from_numpy(res["lut"]), MR.sample_draws(0, 3, bits))


def test_write_lut_file_round_trip(tmp_path):
    from zebrapose_amd.decode import read_lut_file
    v, f = MR.icosphere(2)
    v = v * np.float32(61.7)
    res = MR.encode(v, f[: len(f) // 2], 7)  # half the faces: some classes stay empty
    assert np.isnan(res["lut"]).any()
    p = str(tmp_path / "Class_CorresPoint000001.txt")
    as_mesh_code(v, f[: len(f) // 2], 7, res).write_lut_file(p)
    total, divide, iters, lut = read_lut_file(p)
    assert (total, divide, iters) == (128.0, 2.0, 7.0)
    nan = np.isnan(res["lut"])
    assert np.array_equal(np.isnan(lut), nan)
    want = np.array([[float("%g" % x) for x in row] for row in res["lut"]])
    assert np.array_equal(lut[~nan], want[~nan])
    with open(p) as fh:  # the reference's loader splits every line on single spaces into four fields
        lines = fh.read().split("\n")
    assert lines[0] == "128 2 7" and lines[-1] == "" and all(len(l.split(" ")) == 4 for l in lines[1:-1])
    assert len(lines) == 130


def test_write_ply_round_trip(tmp_path):
    from zebrapose_amd.render import face_bgr_from_ids, read_ply
    v, f = MR.icosphere(2)
    v = np.concatenate([v, np.array([[9, 9, 9]], np.float32)])  # one vertex no face uses
    res = MR.encode(v, f, 6)
    p = str(tmp_path / "obj_000001.ply")
    as_mesh_code(v, f, 6, res).write_ply(p)
    ply = read_ply(p)
    assert ply["faces"].shape == f.shape
    assert len(ply["vertices"]) == len(v) + 3 * len(f) - 162  # every use after a vertex's first is a duplicate
    assert np.array_equal(ply["vertices"][ply["faces"]], v[f])
    want = face_bgr_from_ids(res["face_ids"])[:, ::-1]
    for j in range(3):  # all three vertices carry the face's colour
        assert np.array_equal(ply["colors"][ply["faces"][:, j]], want)
    assert np.array_equal(np.sort(ply["faces"].reshape(-1)), np.sort(np.unique(ply["faces"])))  # no vertex shared
    assert np.array_equal(ply["vertices"][: len(v)], v)


# ---- C ABI and encode_mesh argument checks (no device) ------------------------------------------

def test_zp_mesh_code_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    lib = _lib.lib
    assert lib.zp_mesh_code_ws_bytes(642, 1280, 9) >= 642 * (16 + 4 * 5 + 8 * 2) + 1280 * 8
    assert lib.zp_mesh_code_ws_bytes(1 << 21, 1 << 22, 16) > 0
    for nv, nf, bits in [(511, 100, 9), (642, 0, 9), (642, 100, 0), (1 << 17, 100, 17), ((1 << 21) + 1, 100, 4),
                         (-1, 100, 1), (642, -5, 3)]:
        assert lib.zp_mesh_code_ws_bytes(nv, nf, bits) == -1, (nv, nf, bits)
    buf = (ctypes.c_double * 64)()  # stands in for every pointer: the checks fail before any of them is used
    p = ctypes.addressof(buf)
    good = dict(verts=p, nv=642, faces=p, nf=1280, bits=9, attempts=3, iterations=10, grid_log2=18, eps2_q=1 << 36,
                draws=p, vertex_ids=p, face_ids=p, lut=p, ws=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.zp_mesh_code(*[a[k] for k in good])

    cases = [(dict(bits=0), b"bits 0"), (dict(bits=17), b"bits 17"), (dict(nv=511), b"nv 511"), (dict(nv=0), b"nv 0"),
             (dict(nv=(1 << 21) + 1), b"range"), (dict(nf=0), b"range"), (dict(nf=-3), b"range"),
             (dict(attempts=0), b"attempts 0"), (dict(iterations=0), b"iterations 0"), (dict(iterations=-2), b"iterations"),
             (dict(grid_log2=41), b"grid_log2 41"), (dict(grid_log2=-41), b"grid_log2 -41"), (dict(eps2_q=-1), b"eps2_q")]
    cases += [({k: None}, b"NULL") for k in ("verts", "faces", "draws", "vertex_ids", "face_ids", "lut", "ws")]
    for bad, word in cases:
        assert call(**bad) == 1, bad
        assert word in lib.zp_last_error(), (bad, lib.zp_last_error())


def test_encode_mesh_refuses_bad_meshes_on_the_host():
    from zebrapose_amd.meshcode import encode_mesh
    v, f = MR.icosphere(1)  # 42 vertices
    with pytest.raises(ValueError, match="cannot fill"):
        encode_mesh(v, f, bits=6, device="cpu")
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[5, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            encode_mesh(w, f, bits=3, device="cpu")
    g = f.copy()
    g[3, 2] = 42
    with pytest.raises(ValueError, match="outside"):
        encode_mesh(v, g, bits=3, device="cpu")
    g[3, 2] = -1
    with pytest.raises(ValueError, match="outside"):
        encode_mesh(v, g, bits=3, device="cpu")
    with pytest.raises(ValueError, match="faces"):
        encode_mesh(v, f.astype(np.float32), bits=3, device="cpu")
    with pytest.raises(ValueError, match="faces"):
        encode_mesh(v, f[:, :2], bits=3, device="cpu")
    with pytest.raises(ValueError, match="bits"):
        encode_mesh(v, f, bits=17, device="cpu")
