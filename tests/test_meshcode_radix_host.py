"""Host side of the d-ary mesh coder (no GPU): the numpy restatement tests/meshcode_radix_ref.py
obeys what zp_mesh_code_radix's contract names (children of floor / ceil size at every level, ids that
fold the digits MSB first, the face rule, NaN LUT rows, separated blobs for every seed tried, identical
points), a d-ary MeshCode writes the "N d levels" LUT header and builds a d-ary Decoder, and the
argument checks of encode_mesh_radix and of the C entry fail cleanly before any device call."""
import ctypes

import numpy as np
import pytest

from tests import meshcode_radix_ref as RR
from tests import meshcode_ref as MR


def check_invariants(verts, faces, d, levels, res):
    nv = len(verts)
    prev = np.zeros(nv, np.int64)
    folded = np.zeros(nv, np.int64)
    for l, gid in enumerate(res["levels"]):
        assert np.array_equal(gid // d, prev), f"level {l}: a child is not d * parent + digit"
        n_parent = np.bincount(prev, minlength=d ** l)
        n_child = np.bincount(gid, minlength=d ** (l + 1)).reshape(-1, d)
        lo, hi = n_parent // d, -(-n_parent // d)
        assert ((n_child == lo[:, None]) | (n_child == hi[:, None])).all(), f"level {l}: unbalanced"
        folded += (gid % d) * d ** (levels - 1 - l)
        prev = gid
    assert np.array_equal(res["vertex_ids"], folded)  # sum_l digit_l * d^(levels - 1 - l)
    C = d ** levels
    leaf = np.bincount(res["vertex_ids"], minlength=C)
    assert len(leaf) == C and leaf.min() >= nv // C and leaf.max() <= -(-nv // C)
    fid, lut = res["face_ids"], res["lut"]
    assert lut.shape == (C, 3) and np.array_equal(fid, MR.face_ids_from(res["vertex_ids"], faces))
    present = np.zeros(C, bool)
    present[fid] = True
    assert np.array_equal(np.isnan(lut).any(1), ~present) and np.array_equal(np.isnan(lut).all(1), ~present)
    assert np.array_equal(lut[~present].view(np.int64), np.full((int((~present).sum()), 3), 0x7FF8000000000000))
    v64 = verts.astype(np.float64)
    for c in np.flatnonzero(present)[:: max(1, int(present.sum()) // 40)]:
        s = np.zeros(3)
        fs = np.flatnonzero(fid == c)
        for f in fs:
            for j in range(3):
                s = s + v64[faces[f, j]]
        assert np.array_equal(lut[c], s / float(3 * len(fs))), c


@pytest.mark.parametrize("mesh,d,levels", [("icosphere", 4, 3), ("lattice", 16, 2), ("random1027", 4, 5),
                                           ("random300", 256, 1), ("random1000", 16, 2)])
def test_ref_invariants(mesh, d, levels):
    v, f = {"icosphere": lambda: MR.icosphere(3), "lattice": MR.lattice, "random1027": lambda: MR.random_points(1027, 3),
            "random300": lambda: MR.random_points(300, 4), "random1000": lambda: MR.random_points(1000, 5)}[mesh]()
    check_invariants(v, f, d, levels, RR.encode(v, f, d, levels, return_levels=True))


def test_ref_half_the_faces_leave_nan_rows():
    v, f = MR.icosphere(2)
    res = RR.encode(v, f[: len(f) // 2], 4, 3, return_levels=True)
    assert np.isnan(res["lut"]).any()
    check_invariants(v, f[: len(f) // 2], 4, 3, res)


def test_ref_same_seed_same_result_other_seed_other_draws():
    v, f = MR.icosphere(3)
    a, b = RR.encode(v, f, 4, 3), RR.encode(v, f, 4, 3)
    for k in ("vertex_ids", "face_ids"):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(a["lut"].view(np.int64), b["lut"].view(np.int64))
    assert RR.sample_draws(0, 3, 4, 3).shape == (3, 21) and RR.sample_draws(0, 3, 256, 2).shape == (3, 257)
    assert not np.array_equal(RR.sample_draws(0, 3, 4, 3), RR.sample_draws(7, 3, 4, 3))
    check_invariants(v, f, 4, 3, RR.encode(v, f, 4, 3, seed=7, return_levels=True))


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("count", [4, 16])
def test_ref_blobs_are_recovered_up_to_a_permutation_of_digits(count, seed):
    v, f, blob = MR.blobs(count)
    vid = RR.encode(v, f, count, 1, seed=seed)["vertex_ids"]
    digit_of_blob = [np.unique(vid[blob == b]) for b in range(count)]
    assert all(len(u) == 1 for u in digit_of_blob)
    assert sorted(int(u[0]) for u in digit_of_blob) == list(range(count))


def test_ref_identical_points_split_by_the_tie_rules():
    v, f = MR.duplicate_mesh()
    res = RR.encode(v, f, 4, 2, return_levels=True)
    check_invariants(v, f, 4, 2, res)
    # a group of identical points alone: every seed is its lowest vertex, classes 1 .. d - 1 stay empty in
    # Lloyd, all scores are 0, and the peel hands out floor(|U_j| / (d - j)) vertices in index order
    lv = RR.split_levels(np.zeros((10, 3), np.int64), 4, 1, RR.sample_draws(0, 3, 4, 1), 10, 0)
    assert lv[0].tolist() == [0, 0, 1, 1, 2, 2, 2, 3, 3, 3]
    lv = RR.split_levels(np.zeros((4, 3), np.int64), 4, 1, RR.sample_draws(0, 3, 4, 1), 10, 0)
    assert lv[0].tolist() == [0, 1, 2, 3]


def test_ref_peel_on_a_line():
    """Eight points on a line, d = 4, one level, worked by hand.  Draw 0 gives seed 0 at x = 0; the
    farthest-point seeds are 70, then 30 (30 and 40 tie at min d^2 900: lower index), then 50.  Lloyd
    labels {0, 10}, {60, 70}, {20, 30, 40}, {50} (40 ties between centres 30 and 50, 60 between 70 and
    50: lowest class), moves the centres to 5, 65, 30, 50 and stops after the second step."""
    q = np.array([[x, 0, 0] for x in (0, 10, 20, 30, 40, 50, 60, 70)], np.int64)
    lv = RR.split_levels(q, 4, 1, np.zeros((1, 1), np.uint32), 10, 0)
    # the peel, quotas 2, 2, 2: D_0 - min(D_1, D_2, D_3) is lowest at 0 (-875) and 10 (-375); of the rest
    # D_1 - min(D_2, D_3) at 70 (-375) and 60 (-75); D_2 - D_3 at 20 (-800) and 30 (-400); 40, 50 are left
    assert np.bincount(lv[0], minlength=4).tolist() == [2, 2, 2, 2]
    assert lv[0][0] == lv[0][1] == 0 and lv[0][6] == lv[0][7] == 1
    assert lv[0][2] == lv[0][3] == 2 and lv[0][4] == lv[0][5] == 3


# ---- MeshCode of a d-ary code (no device) ------------------------------------------------------

def as_mesh_code(v, f, d, levels, res):
    import torch
    from zebrapose_amd.meshcode import MeshCode
    return MeshCode(v, f, (d.bit_length() - 1) * levels, torch.from_numpy(res["vertex_ids"]),
                    torch.from_numpy(res["face_ids"]), torch.from_numpy(res["lut"]), RR.sample_draws(0, 3, d, levels),
                    divide=d, levels=levels)


def test_write_lut_file_header_and_round_trip(tmp_path):
    from zebrapose_amd.decode import read_lut_file
    v, f = MR.icosphere(2)
    res = RR.encode(v * np.float32(61.7), f[: len(f) // 2], 4, 3)
    assert np.isnan(res["lut"]).any()
    p = str(tmp_path / "Class_CorresPoint000001.txt")
    mc = as_mesh_code(v * np.float32(61.7), f[: len(f) // 2], 4, 3, res)
    assert (mc.divide, mc.levels, mc.bits) == (4, 3, 6)
    mc.write_lut_file(p)
    total, divide, iters, lut = read_lut_file(p)
    assert (total, divide, iters) == (64.0, 4.0, 3.0)
    nan = np.isnan(res["lut"])
    assert np.array_equal(np.isnan(lut), nan)
    want = np.array([[float("%g" % x) for x in row] for row in res["lut"]])
    assert np.array_equal(lut[~nan], want[~nan])
    with open(p) as fh:
        assert fh.readline() == "64 4 3\n"


def test_binary_mesh_code_keeps_its_header_and_fields(tmp_path):
    import torch
    from zebrapose_amd.meshcode import MeshCode
    v, f = MR.icosphere(2)
    res = MR.encode(v, f, 5)
    mc = MeshCode(v, f, 5, torch.from_numpy(res["vertex_ids"]), torch.from_numpy(res["face_ids"]),
                  torch.from_numpy(res["lut"]), MR.sample_draws(0, 3, 5))
    assert (mc.divide, mc.levels, mc.bits) == (2, 5, 5)
    p = str(tmp_path / "lut.txt")
    mc.write_lut_file(p)
    with open(p) as fh:
        assert fh.readline() == "32 2 5\n"


def test_radix_mesh_code_refuses_ignore_bit():
    v, f = MR.icosphere(2)
    mc = as_mesh_code(v, f, 4, 2, RR.encode(v, f, 4, 2))
    with pytest.raises(ValueError, match="ignore_bit"):
        mc.decoder(ignore_bit=1, device="cpu")


# ---- C ABI and encode_mesh_radix argument checks (no device) ---------------------------------------

def test_zp_mesh_code_radix_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    lib = _lib.lib
    assert lib.zp_mesh_code_radix_ws_bytes(642, 1280, 4, 3) >= 642 * (16 + 4 * 6 + 8 * 2) + 1280 * 8
    # sensible at the largest problem: well under a gigabyte, no nv * d table
    assert 0 < lib.zp_mesh_code_radix_ws_bytes(1 << 21, 1 << 22, 256, 2) < 1 << 30
    assert lib.zp_mesh_code_radix_ws_bytes(1 << 21, 1 << 22, 4, 8) > 0
    for nv, nf, d, levels in [(63, 100, 4, 3), (642, 0, 4, 3), (642, 100, 4, 0), (642, 100, 2, 3), (642, 100, 3, 2),
                              (70000, 100, 512, 1), (1 << 20, 100, 4, 9), (1 << 20, 100, 256, 3),
                              ((1 << 21) + 1, 100, 4, 2), (-1, 100, 4, 1), (642, -5, 4, 2)]:
        assert lib.zp_mesh_code_radix_ws_bytes(nv, nf, d, levels) == -1, (nv, nf, d, levels)
    buf = (ctypes.c_double * 64)()  # stands in for every pointer: the checks fail before any of them is used
    p = ctypes.addressof(buf)
    good = dict(verts=p, nv=642, faces=p, nf=1280, divide=4, levels=3, attempts=3, iterations=10, grid_log2=18,
                eps2_q=1 << 36, draws=p, vertex_ids=p, face_ids=p, lut=p, ws=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.zp_mesh_code_radix(*[a[k] for k in good])

    cases = [(dict(divide=2), b"zp_mesh_code"), (dict(divide=3), b"divide 3"), (dict(divide=512), b"divide 512"),
             (dict(divide=0), b"divide 0"), (dict(levels=0), b"levels 0"), (dict(levels=9, nv=1 << 20), b"levels 9"),
             (dict(divide=256, levels=3, nv=1 << 20), b"levels 3"), (dict(nv=63), b"nv 63"), (dict(nv=0), b"nv 0"),
             (dict(nv=(1 << 21) + 1), b"range"), (dict(nf=0), b"range"), (dict(nf=-3), b"range"),
             (dict(attempts=0), b"attempts 0"), (dict(iterations=0), b"iterations 0"),
             (dict(grid_log2=41), b"grid_log2 41"), (dict(grid_log2=-41), b"grid_log2 -41"), (dict(eps2_q=-1), b"eps2_q")]
    cases += [({k: None}, b"NULL") for k in ("verts", "faces", "draws", "vertex_ids", "face_ids", "lut", "ws")]
    for bad, word in cases:
        assert call(**bad) == 1, bad
        assert word in lib.zp_last_error(), (bad, lib.zp_last_error())
    assert b"zp_mesh_code_radix" in lib.zp_last_error()


def test_encode_mesh_radix_refuses_bad_input_on_the_host():
    from zebrapose_amd.meshcode import encode_mesh_radix
    v, f = MR.icosphere(1)  # 42 vertices
    with pytest.raises(ValueError, match="encode_mesh"):
        encode_mesh_radix(v, f, 2, 3, device="cpu")
    for d in (3, 512, 0, -4):
        with pytest.raises(ValueError, match="power of two"):
            encode_mesh_radix(v, f, d, 1, device="cpu")
    for d, levels in ((4, 0), (4, 9), (16, 5), (256, 3)):
        with pytest.raises(ValueError, match="levels"):
            encode_mesh_radix(v, f, d, levels, device="cpu")
    with pytest.raises(ValueError, match="cannot fill"):
        encode_mesh_radix(v, f, 4, 3, device="cpu")
    with pytest.raises(ValueError, match="attempts"):
        encode_mesh_radix(v, f, 4, 2, attempts=0, device="cpu")
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[5, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            encode_mesh_radix(w, f, 4, 2, device="cpu")
    g = f.copy()
    g[3, 2] = 42
    with pytest.raises(ValueError, match="outside"):
        encode_mesh_radix(v, g, 4, 2, device="cpu")
    with pytest.raises(ValueError, match="faces"):
        encode_mesh_radix(v, f.astype(np.float32), 4, 2, device="cpu")
    with pytest.raises(ValueError, match="faces"):
        encode_mesh_radix(v, f[:, :2], 4, 2, device="cpu")
