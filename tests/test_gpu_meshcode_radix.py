"""zp_mesh_code_radix through zebrapose_amd.meshcode.encode_mesh_radix against its numpy restatement
(tests/meshcode_radix_ref.py): vertex ids, face ids and the bits of the LUT are compared exactly.
The cases are the smallest shapes at which the kernels can still go wrong: exact ties in labels,
scores and seeds, last levels with one vertex per class, group sizes no multiple of d, mixed quotas
of one and two, groups of identical points, and the two full-depth codes of 65536 classes.  Then the
chain raw mesh -> d-ary codes -> renderer -> GT digit planes -> Decoder(class_base=d)."""
import numpy as np
import pytest
import torch

from tests import meshcode_radix_ref as RR
from tests import meshcode_ref as MR

pytestmark = pytest.mark.gpu


def dev_encode(v, f, d, levels, **kw):
    from zebrapose_amd.meshcode import encode_mesh_radix
    mc = encode_mesh_radix(v, f, d, levels, **kw)
    torch.cuda.synchronize()
    return mc


def assert_same(mc, ref, what=""):
    for k in ("vertex_ids", "face_ids"):
        a, b = getattr(mc, k).cpu().numpy(), ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{what}: {k} differs at {len(bad)} of {len(a)} places, first {bad[0]}: {a[bad[0]]} vs {b[bad[0]]}"
    a, b = mc.lut.cpu().numpy().view(np.int64), ref["lut"].view(np.int64)
    assert a.shape == b.shape
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{what}: lut differs at {len(bad)} places, first {bad[0]}"


def both(v, f, d, levels, what, **kw):
    mc = dev_encode(v, f, d, levels, **kw)
    assert_same(mc, RR.encode(v, f, d, levels, **kw), what)
    return mc


@pytest.fixture(scope="module")
def sphere3():
    v, f = MR.icosphere(3)
    return v * np.float32(40), f


@pytest.mark.parametrize("d,levels", [(4, 3), (16, 2)])
def test_integer_lattice_ties(d, levels):
    v, f = MR.lattice()
    both(v, f, d, levels, f"lattice / {d}^{levels}")


@pytest.mark.parametrize("n,d,levels", [(16, 4, 2), (256, 256, 1), (1000, 16, 2), (300, 256, 1), (1027, 4, 5)])
def test_random_points(n, d, levels):
    v, f = MR.random_points(n, seed=n)
    both(v, f, d, levels, f"random {n} / {d}^{levels}")


def test_duplicate_points_coincident_seeds_and_empty_classes():
    v, f = MR.duplicate_mesh()
    mc = both(v, f, 4, 2, "duplicates / 4^2")
    leaf = np.bincount(mc.vertex_ids.cpu().numpy(), minlength=16)
    assert leaf.min() >= len(v) // 16 and leaf.max() <= -(-len(v) // 16)


@pytest.mark.parametrize("d,levels", [(4, 8), (256, 2)])
def test_full_depth_65536_classes(d, levels):
    v, f = MR.random_points(70000, seed=70000)
    mc = both(v, f, d, levels, f"random 70000 / {d}^{levels}")
    assert tuple(mc.lut.shape) == (65536, 3)


def test_icosphere_one_and_three_attempts(sphere3):
    both(*sphere3, 4, 3, "attempts 1", attempts=1)
    both(*sphere3, 4, 3, "attempts 3", attempts=3)


def test_huge_eps_stops_every_group_after_its_first_step(sphere3):
    both(*sphere3, 4, 3, "eps 1e30", eps=1e30)
    both(*sphere3, 4, 3, "eps 1e30, other seed", eps=1e30, seed=11)


def test_two_runs_are_bitwise_equal(sphere3):
    a, b = dev_encode(*sphere3, 16, 2), dev_encode(*sphere3, 16, 2)
    assert torch.equal(a.vertex_ids, b.vertex_ids) and torch.equal(a.face_ids, b.face_ids)
    assert torch.equal(a.lut.view(torch.int64), b.lut.view(torch.int64))


def test_chain_encode_render_gt_digits_decode(sphere3):
    from zebrapose_amd import _lib as L
    d, levels = 4, 3
    v, f = sphere3
    mc = dev_encode(v, f, d, levels)
    assert (mc.divide, mc.levels, mc.bits) == (d, levels, 6)
    H = W = 64
    out = mc.renderer().render(np.eye(3).reshape(1, 9), np.array([[0.0, 0.0, 200.0]]),
                               np.array([[120.0, 120.0, 32.0, 32.0]]), H, W, outputs=("color", "face", "mask"))
    torch.cuda.synchronize()
    color, face = out["color"].cpu().numpy()[0].astype(np.int64), out["face"].cpu().numpy()[0]
    covered = face >= 0
    assert covered.sum() > 1000 and np.array_equal(covered, out["mask"].cpu().numpy()[0] > 0)
    fid = mc.face_ids.cpu().numpy()
    ids = (color[..., 0] << 16) | (color[..., 1] << 8) | color[..., 2]  # the GT id image
    # GT digit planes (zp_pack_digits over the id's bit planes, MSB first), folded back
    planes = np.stack([(ids >> (mc.bits - 1 - j)) & 1 for j in range(mc.bits)]).astype(np.uint8)[None]
    bt = torch.from_numpy(planes).cuda()
    digits = torch.empty((1, levels, H, W), dtype=torch.uint8, device="cuda")
    L.call("zp_pack_digits", bt.data_ptr(), 1, mc.bits, H, W, 2, digits.data_ptr(), L.stream_ptr())
    dg = digits.cpu().numpy()[0].astype(np.int64)
    assert dg.max() < d
    folded = sum(dg[i] * d ** (levels - 1 - i) for i in range(levels))
    assert np.array_equal(folded[covered], fid[face[covered]])
    # logits one-hot in those digits -> Decoder(class_base=d) returns the LUT rows of the ids
    dec = mc.decoder()
    assert dec.class_base == d and dec.steps == levels and tuple(dec.lut.shape) == (1, d ** levels, 3)
    code = np.full((1, levels * d, H, W), -5.0, np.float32)
    for i in range(levels):
        np.put_along_axis(code[0, i * d:(i + 1) * d], dg[i][None], 5.0, axis=0)
    mask = np.where(covered, 5.0, -5.0).astype(np.float32)[None, None]
    counts, xy, xyz = dec(torch.from_numpy(mask).cuda(), torch.from_numpy(code).cuda(), np.array([[0, 0, W, H]]),
                          bbox_size=W)
    torch.cuda.synchronize()
    lut = mc.lut.cpu().numpy()
    want = lut[fid[face[covered]]].astype(np.float32)  # row-major over the mask
    assert not np.isnan(want).any() and int(counts[0]) == int(covered.sum())
    assert np.array_equal(xyz.cpu().numpy()[0, : len(want)], want)


def test_files_round_trip(sphere3, tmp_path):
    from zebrapose_amd.decode import read_lut_file
    from zebrapose_amd.render import read_ply
    mc = dev_encode(*sphere3, 4, 3)
    p = str(tmp_path / "Class_CorresPoint000001.txt")
    mc.write_lut_file(p)
    total, divide, iters, lut = read_lut_file(p)
    assert (total, divide, iters) == (64, 4, 3)
    ref = mc.lut.cpu().numpy()
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(lut), nan)
    assert np.array_equal(lut[~nan], np.array([[float("%g" % x) for x in row] for row in ref])[~nan])
    q = str(tmp_path / "obj_000001.ply")
    mc.write_ply(q)
    ply = read_ply(q)
    assert np.array_equal(ply["vertices"][ply["faces"]], sphere3[0][sphere3[1]])
