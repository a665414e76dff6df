"""zp_mesh_code through zebrapose_amd.meshcode.encode_mesh against its numpy restatement
(tests/meshcode_ref.py): vertex ids, face ids and the bits of the LUT are compared exactly.  The
cases are the smallest shapes at which the kernels can still go wrong: leaves of one or two
vertices, odd group sizes, many groups inside one wave, exact ties, identical points, and one
large shallow case in which whole waves sit inside one group."""
import numpy as np
import pytest
import torch

from tests import meshcode_ref as MR

pytestmark = pytest.mark.gpu


def dev_encode(v, f, bits, **kw):
    from zebrapose_amd.meshcode import encode_mesh
    mc = encode_mesh(v, f, bits=bits, **kw)
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


def both(v, f, bits, what, **kw):
    mc = dev_encode(v, f, bits, **kw)
    assert_same(mc, MR.encode(v, f, bits, **kw), what)
    return mc


@pytest.fixture(scope="module")
def sphere3():
    v, f = MR.icosphere(3)
    return v * np.float32(40), f


def test_icosphere_642_at_9_bits(sphere3):
    both(*sphere3, 9, "icosphere 642 / 9")


def test_icosphere_10242_at_13_bits():
    v, f = MR.icosphere(5)
    assert len(v) == 10242
    both(v * np.float32(75.5), f, 13, "icosphere 10242 / 13")


@pytest.mark.parametrize("n,bits", [(1024, 10), (1025, 10), (1000, 5)])
def test_random_points(n, bits):
    v, f = MR.random_points(n, seed=n)
    both(v, f, bits, f"random {n} / {bits}")


def test_integer_lattice_ties():
    v, f = MR.lattice()
    both(v, f, 6, "lattice / 6")
    both(v, f, 10, "lattice / 10")


def test_duplicate_points_empty_class():
    v, f = MR.duplicate_mesh()
    both(v, f, 7, "duplicates / 7")


def test_large_shallow_many_workgroups_per_group():
    v, f = MR.random_points((1 << 17) + 3, seed=5)
    both(v, f[:3000], 4, "random 2^17 + 3 / 4")


def test_single_step_and_no_early_stop(sphere3):
    both(*sphere3, 9, "attempts 1, iterations 1", attempts=1, iterations=1)
    both(*sphere3, 9, "eps 0", eps=0.0)


def test_huge_eps_stops_every_group_after_its_first_step(sphere3):
    both(*sphere3, 9, "eps 1e30", eps=1e30)
    both(*sphere3, 9, "other seed", seed=11)


def test_two_runs_are_bitwise_equal(sphere3):
    a, b = dev_encode(*sphere3, 9), dev_encode(*sphere3, 9)
    assert torch.equal(a.vertex_ids, b.vertex_ids) and torch.equal(a.face_ids, b.face_ids)
    assert torch.equal(a.lut.view(torch.int64), b.lut.view(torch.int64))


def test_non_default_stream_equals_default_stream(sphere3):
    a = dev_encode(*sphere3, 9)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = dev_encode(*sphere3, 9)
    assert torch.equal(a.vertex_ids, b.vertex_ids) and torch.equal(a.face_ids, b.face_ids)
    assert torch.equal(a.lut.view(torch.int64), b.lut.view(torch.int64))


def test_end_to_end_encode_render_read_back(sphere3):
    from zebrapose_amd.render import face_bgr_from_ids
    v, f = sphere3
    mc = dev_encode(v, f, 9)
    out = mc.renderer().render(np.eye(3).reshape(1, 9), np.array([[0.0, 0.0, 200.0]]),
                               np.array([[120.0, 120.0, 32.0, 32.0]]), 64, 64, outputs=("color", "face"))
    torch.cuda.synchronize()
    color, face = out["color"].cpu().numpy()[0], out["face"].cpu().numpy()[0]
    covered = face >= 0
    assert covered.sum() > 1000
    fid = mc.face_ids.cpu().numpy()
    assert np.array_equal(color[covered], face_bgr_from_ids(fid)[face[covered]])
    c = color[covered].astype(np.int64)
    ids = (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    assert np.array_equal(ids, fid[face[covered]])
    lut = mc.lut.cpu().numpy()
    assert not np.isnan(lut[ids]).any()
    dec = mc.decoder()
    assert dec.bits == 9 and tuple(dec.lut.shape) == (1, 512, 3)
