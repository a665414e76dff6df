"""zp_mesh_subdivide and its drivers (zebrapose_amd.meshcode.subdivide_midpoint / upsample_mesh) against
the numpy restatement tests/subdiv_ref.py: vertices, faces, parents, counts and the longest edge are
compared bit for bit.  The cases are the smallest at which the kernels can still go wrong: boundary
edges, every rotation of the 1- and 2-split templates, the diagonal rule both ways and at a tie, budgets
that cut through ties, non-manifold and degenerate faces, meshes of one slot short of, exactly and one
slot past a workgroup, and two meshes of several workgroups."""
import numpy as np
import pytest
import torch

from tests import meshcode_ref as MR
from tests import subdiv_ref as SR

pytestmark = pytest.mark.gpu

FILL = -7


def dev_pass(v, f, abs2=0.0, rel2=0.0, max_split=SR.NO_BUDGET, cap_v=None, cap_f=None, check=True):
    """One zp_mesh_subdivide call through the C ABI -> the dict subdiv_ref.subdivide_pass returns, plus the
    untrimmed output buffers (prefilled with FILL) under "raw"."""
    from zebrapose_amd import _lib as L
    v = np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(f, np.int32).reshape(-1, 3))
    nv, nf = len(v), len(f)
    cap_v = nv + min(max_split, 3 * nf) if cap_v is None else cap_v
    cap_f = 4 * nf if cap_f is None else cap_f
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    ov = torch.full((max(cap_v, 1), 3), float(FILL), dtype=torch.float32, device="cuda")
    of = torch.full((max(cap_f, 1), 3), FILL, dtype=torch.int32, device="cuda")
    par = torch.full((max(cap_v, 1), 2), FILL, dtype=torch.int32, device="cuda")
    counts = torch.full((4,), FILL, dtype=torch.int64, device="cuda")
    mx = torch.full((1,), float(FILL), dtype=torch.float64, device="cuda")
    ws = torch.empty(L.lib.zp_mesh_subdivide_ws_bytes(nv, nf), dtype=torch.uint8, device="cuda")
    L.call("zp_mesh_subdivide", vd.data_ptr(), nv, fd.data_ptr(), nf, float(abs2), float(rel2), int(max_split),
           ov.data_ptr(), cap_v, of.data_ptr(), cap_f, par.data_ptr(), counts.data_ptr(), mx.data_ptr(), ws.data_ptr(),
           L.stream_ptr())
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    raw = (ov.cpu().numpy(), of.cpu().numpy(), par.cpu().numpy())
    res = {"counts": c, "max_len2": mx.cpu().numpy()[0], "raw": raw}
    if c[2] <= cap_v and c[3] <= cap_f:
        res.update(vertices=raw[0][:c[2]], faces=raw[1][:c[3]], parents=raw[2][:c[2]])
        if check:  # nothing beyond the counted rows is touched
            assert (raw[0][c[2]:] == FILL).all() and (raw[1][c[3]:] == FILL).all() and (raw[2][c[2]:] == FILL).all()
    return res


def assert_same(dev, ref, what=""):
    assert np.array_equal(dev["counts"], ref["counts"]), (what, dev["counts"], ref["counts"])
    assert np.float64(dev["max_len2"]).view(np.int64) == np.float64(ref["max_len2"]).view(np.int64), what
    for k, bits in (("vertices", np.int32), ("faces", np.int32), ("parents", np.int32)):
        a, b = dev[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.shape, b.shape)
        bad = np.argwhere(a.view(bits) != b.view(bits))
        assert len(bad) == 0, f"{what}: {k} differs at {len(bad)} places, first {bad[0]}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}"


def both(v, f, what="", **kw):
    dev, ref = dev_pass(v, f, **kw), SR.subdivide_pass(v, f, **kw)
    assert_same(dev, ref, what)
    return ref


def sweep(v, f, what):
    """Full split, the relative threshold, and budgets below the number of qualifying edges."""
    full = both(v, f, what + " full")
    rel = both(v, f, what + " rel", rel2=0.25)
    for n in sorted({1, int(rel["counts"][1]) // 2, int(rel["counts"][1]) - 1} - {0}):
        r = both(v, f, f"{what} rel budget {n}", rel2=0.25, max_split=n)
        assert r["counts"][1] == min(n, rel["counts"][1])
    both(v, f, what + " budget 3", max_split=3)
    return full


SCALENE = np.array([(0, 0, 0), (7, 0, 0), (2, 4, 1)], np.float32)  # len2 49, 42, 21


def test_single_triangle_all_boundary_edges():
    r = sweep(SCALENE, [(0, 1, 2)], "triangle")
    assert np.array_equal(r["counts"], [3, 3, 6, 4])


def test_tetrahedron():
    r = sweep(*SR.tetrahedron(), "tetrahedron")
    assert np.array_equal(r["counts"], [6, 6, 10, 16]) and SR.is_closed_manifold(r["faces"])


def test_box():
    v, f = SR.box()
    r = sweep(v, f, "box")
    assert np.array_equal(r["counts"], [18, 18, 26, 48])
    r = both(v, f, "box long edges", abs2=10.5 ** 2)
    assert SR.is_closed_manifold(r["faces"]) and 0 < r["counts"][1] < 18


@pytest.mark.parametrize("n", [255, 256, 257])
def test_strip_across_workgroup_boundaries(n):
    v, f = SR.strip(n)
    assert len(f) == n
    sweep(v, f, f"strip {n}")


@pytest.mark.parametrize("level,nv", [(3, 642), (4, 2562)])
def test_anisotropic_icosphere_several_workgroups(level, nv):
    v, f = MR.icosphere(level)
    assert len(v) == nv
    v = v * np.array([1.0, 0.37, 2.9], np.float32)
    full = sweep(v, f, f"icosphere {nv}")
    assert SR.is_closed_manifold(full["faces"]) and full["counts"][2] == 4 * nv - 6
    r = both(v, f, f"icosphere {nv} threshold", abs2=float(np.float64(np.median(SR.len2(v[f[:, 0]], v[f[:, 1]])))))
    assert SR.is_closed_manifold(r["faces"]) and 0 < r["counts"][1] < r["counts"][0]


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_one_and_two_split_faces_in_every_rotation(rot):
    face = [tuple(np.roll([0, 1, 2], -rot))]
    r = both(SCALENE, face, f"1 split, rotation {rot}", abs2=45.0)
    assert np.array_equal(r["counts"], [3, 1, 4, 2])
    r = both(SCALENE, face, f"2 split, rotation {rot}", abs2=30.0)
    assert np.array_equal(r["counts"], [3, 2, 5, 3])
    # the same through the budget, and with the reversed orientation
    both(SCALENE, face, f"1 split by budget, rotation {rot}", max_split=1)
    both(SCALENE, face, f"2 split by budget, rotation {rot}", max_split=2)
    back = [tuple(np.roll([2, 1, 0], -rot))]
    both(SCALENE, back, f"1 split reversed, rotation {rot}", abs2=45.0)
    both(SCALENE, back, f"2 split reversed, rotation {rot}", abs2=30.0)


def _has_edge(faces, a, b):
    f = np.asarray(faces)
    return any(((f[:, j] == a) & (f[:, (j + 1) % 3] == b)).any() or ((f[:, j] == b) & (f[:, (j + 1) % 3] == a)).any()
               for j in range(3))


def test_two_split_diagonal_both_ways_and_at_a_tie():
    """Integer coordinates, so every len2 is exact.  A right-isoceles triangle's hypotenuse is its longest
    edge and always splits before a leg, so the quad's two diagonals can only differ there (the budget of 2
    takes the hypotenuse and the leg of the lower key); the exact tie needs both legs split and the base
    not, which a tall isoceles triangle gives."""
    # right angle at index 1, unsplit leg (1, 2): the quad is (2, m02, m01, 1) up to rotation
    v = np.array([(0, 4, 0), (0, 0, 0), (4, 0, 0)], np.float32)
    r = both(v, [(2, 0, 1)], "right-isoceles, diagonal from the midpoint", max_split=2)
    assert np.array_equal(r["parents"][3:], [(0, 1), (0, 2)])  # m01 = 3 (leg), m02 = 4 (hypotenuse)
    assert _has_edge(r["faces"], 4, 1) and not _has_edge(r["faces"], 2, 3)  # len2 8 against 20
    for face in [(0, 1, 2), (1, 2, 0), (1, 0, 2)]:
        both(v, [face], f"right-isoceles {face}", max_split=2)
    # the other leg split: right angle at index 0, hypotenuse (1, 2), legs (0, 1) and (0, 2)
    v = np.array([(0, 0, 0), (0, 4, 0), (4, 0, 0)], np.float32)
    r = both(v, [(0, 1, 2)], "right-isoceles, the other way", max_split=2)
    assert np.array_equal(r["parents"][3:], [(0, 1), (1, 2)])
    both(v, [(2, 1, 0)], "right-isoceles, the other way, reversed", max_split=2)
    # tall isoceles: legs (0, 1) and (1, 2) of len2 68 split, the base (2, 0) of len2 16 does not
    v = np.array([(-2, 0, 0), (0, 8, 0), (2, 0, 0)], np.float32)
    r = both(v, [(0, 1, 2)], "tie", abs2=20.0)
    assert np.array_equal(r["faces"], [(3, 1, 4), (0, 3, 4), (0, 4, 2)])  # 25 against 25: the second template
    v[0, 0] = -4  # len2(m01, v2) = 32 < len2(v0, m12) = 41
    r = both(v, [(0, 1, 2)], "first diagonal", abs2=40.0)
    assert np.array_equal(r["faces"], [(3, 1, 4), (0, 3, 2), (3, 4, 2)])
    v[0, 0], v[2, 0] = -2, 4  # and 41 against 32
    r = both(v, [(0, 1, 2)], "second diagonal", abs2=40.0)
    assert np.array_equal(r["faces"], [(3, 1, 4), (0, 3, 4), (0, 4, 2)])


@pytest.mark.parametrize("budget", [1, 5, 11])
def test_budget_through_ties_on_a_unit_cube(budget):
    v, f = SR.box(1.0, 1.0, 1.0)  # 12 axis edges of len2 1, 6 face diagonals of len2 2
    r = both(v, f, f"cube budget {budget}", max_split=budget)
    assert r["counts"][1] == budget and r["counts"][0] == 18
    l2 = SR.len2(v[r["parents"][8:, 0]], v[r["parents"][8:, 1]])
    assert (l2 == 2.0).sum() == min(budget, 6) and (l2 == 1.0).sum() == max(budget - 6, 0)
    keys = (r["parents"][8:, 0].astype(np.int64) << 32) | r["parents"][8:, 1]
    assert (np.diff(keys) > 0).all()
    r = both(v, f, f"cube axis edges only, budget {budget}", abs2=0.5, rel2=0.0, max_split=budget)
    both(v, f, f"cube rel, budget {budget}", rel2=0.75, max_split=budget)  # only the diagonals qualify


def test_edge_shared_by_three_faces():
    v = np.array([(0, 0, 0), (4, 0, 0), (2, 3, 0), (2, -3, 1), (2, 0, 3)], np.float32)
    f = [(0, 1, 2), (1, 0, 3), (0, 1, 4)]
    r = sweep(v, f, "three faces on one edge")
    assert np.array_equal(r["counts"], [7, 7, 12, 12])
    r = both(v, f, "only the shared edge", abs2=15.5)
    assert np.array_equal(r["counts"], [7, 1, 6, 6])


def test_face_with_a_repeated_index():
    v = np.array([(0, 0, 0), (4, 0, 0), (2, 3, 0), (1, 1, 1)], np.float32)
    f = [(0, 1, 2), (0, 0, 1), (2, 1, 2), (3, 3, 3), (1, 3, 1)]
    r = sweep(v, f, "repeated index")
    assert r["counts"][1] == 4  # (0,1) (0,2) (1,2) (1,3); the zero-length edges never split
    both(np.zeros((3, 3), np.float32), [(0, 1, 2)], "all edges of length 0")
    both(np.zeros((3, 3), np.float32), [(0, 1, 2)], "all edges of length 0, rel", rel2=0.25, max_split=2)


def test_vertex_no_face_uses_and_out_of_range_indices():
    v, f = SR.box()
    v = np.concatenate([v[:3], [(9, 9, 9)], v[3:], [(-5, 0, 2)]]).astype(np.float32)
    f = np.where(f >= 3, f + 1, f).astype(np.int32)
    r = sweep(v, f, "unused vertices")
    assert np.array_equal(r["vertices"][:10], v) and not (r["faces"] == 3).any() and not (r["faces"] == 9).any()
    g = f.copy()
    g[0, 0], g[5, 2] = -3, 1000  # read as 0 and 9
    sweep(v, g, "clamped indices")


def test_threshold_above_the_longest_edge_changes_nothing():
    v, f = SR.box()
    r = both(v, f, "high threshold", abs2=10101.0)
    assert np.array_equal(r["counts"], [18, 0, 8, 12])
    assert np.array_equal(r["vertices"], v) and np.array_equal(r["faces"], f) and r["max_len2"] == 10100.0
    both(v, f, "threshold at the longest edge", abs2=10100.0)
    r = both(v, f, "just below", abs2=10099.5)
    assert r["counts"][1] == 2
    r = both(v, f, "budget 0", max_split=0)
    assert np.array_equal(r["counts"], [18, 0, 8, 12])


def test_capacity_one_too_small_leaves_the_outputs_untouched():
    v, f = SR.box()
    ref = SR.subdivide_pass(v, f, rel2=0.25)
    nvo, nfo = int(ref["counts"][2]), int(ref["counts"][3])
    assert_same(dev_pass(v, f, rel2=0.25, cap_v=nvo, cap_f=nfo), ref, "exact capacity")
    for cap_v, cap_f in [(nvo - 1, nfo), (nvo, nfo - 1), (0, 0), (nvo - 1, nfo - 1)]:
        d = dev_pass(v, f, rel2=0.25, cap_v=cap_v, cap_f=cap_f)
        assert np.array_equal(d["counts"], ref["counts"]) and d["max_len2"] == ref["max_len2"]
        assert "vertices" not in d and all((a == FILL).all() for a in d["raw"]), (cap_v, cap_f)


@pytest.fixture(scope="module")
def sphere3():
    v, f = MR.icosphere(3)
    return v * np.array([1.0, 0.37, 2.9], np.float32), f


def test_two_runs_are_bitwise_equal(sphere3):
    a, b = dev_pass(*sphere3, rel2=0.25, max_split=700), dev_pass(*sphere3, rel2=0.25, max_split=700)
    assert_same(a, b, "two runs")


def test_non_default_stream_equals_default_stream(sphere3):
    a = dev_pass(*sphere3, rel2=0.25, max_split=700)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = dev_pass(*sphere3, rel2=0.25, max_split=700)
    assert_same(a, b, "streams")


def assert_mesh_same(m, ref, what):
    for k in ("vertices", "faces", "parents"):
        a, b = getattr(m, k), ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (what, k)
    assert m.pass_sizes == ref["pass_sizes"], what


def test_drivers_match_the_reference(sphere3):
    from zebrapose_amd.meshcode import subdivide_midpoint, upsample_mesh
    v, f = SR.box()
    assert_mesh_same(subdivide_midpoint(v, f, iterations=2, threshold=10.5),
                     SR.subdivide_midpoint(v, f, iterations=2, threshold=10.5), "midpoint 2 x 10.5")
    assert_mesh_same(subdivide_midpoint(*sphere3), SR.subdivide_midpoint(*sphere3), "midpoint sphere")
    m = upsample_mesh(v, f, min_vertices=1025)
    assert_mesh_same(m, SR.upsample_mesh(v, f, min_vertices=1025), "upsample box 1025")
    assert len(m.pass_sizes) == 6 and len(m.vertices) == 1025 and SR.is_closed_manifold(m.faces)
    m = upsample_mesh(v, f, min_vertices=8)
    assert m.pass_sizes == [] and np.array_equal(m.vertices, v) and np.array_equal(m.faces, f)
    assert np.array_equal(m.parents, np.stack([np.arange(8)] * 2, 1)) and m.parents.dtype == np.int32
    m = subdivide_midpoint(v, f, iterations=0)
    assert m.pass_sizes == [] and np.array_equal(m.faces, f)
    with pytest.raises(ValueError, match="max_passes"):
        upsample_mesh(v, f, min_vertices=1025, max_passes=2)
    with pytest.raises(ValueError, match="length 0"):
        upsample_mesh(np.zeros((3, 3), np.float32), [(0, 1, 2)], min_vertices=4)
    with pytest.raises(ValueError, match="2\\^21"):
        upsample_mesh(v, f, min_vertices=(1 << 21) + 1)


def test_lift_of_the_positions_reproduces_the_vertices(sphere3):
    from zebrapose_amd.meshcode import subdivide_midpoint, upsample_mesh
    v, f = sphere3
    m = subdivide_midpoint(v, f)
    lifted = m.lift(v)
    assert lifted.dtype == np.float64 and np.array_equal(lifted.astype(np.float32).view(np.int32), m.vertices.view(np.int32))
    m = upsample_mesh(*SR.box(), min_vertices=100)
    rgb = np.arange(24, dtype=np.float64).reshape(8, 3)
    assert np.array_equal(m.lift(rgb), SR.lift(rgb, m.parents, 8, m.pass_sizes)) and len(m.lift(rgb)) == 100
    with pytest.raises(ValueError, match="rows"):
        m.lift(rgb[:5])


def _render_read_back(mc, classes):
    from zebrapose_amd.render import face_bgr_from_ids
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
    assert tuple(mc.decoder().lut.shape) == (1, classes, 3)


def test_end_to_end_icosahedron_upsampled_coded_rendered():
    from zebrapose_amd.meshcode import encode_mesh, encode_mesh_radix
    v, f = MR.icosphere(0)
    v = v * np.float32(40)
    assert len(v) == 12
    with pytest.raises(ValueError, match="12 vertices cannot fill 2\\^10 classes"):
        encode_mesh(v, f, bits=10)
    mc = encode_mesh(v, f, bits=10, upsample=True)
    torch.cuda.synchronize()
    ref = SR.upsample_mesh(v, f, min_vertices=1025)
    assert len(mc.vertices) == 1025 and np.array_equal(mc.vertices.view(np.int32), ref["vertices"].view(np.int32))
    assert np.array_equal(mc.faces, ref["faces"]) and SR.is_closed_manifold(mc.faces)
    assert np.bincount(mc.vertex_ids.cpu().numpy(), minlength=1024).min() >= 1
    assert mc.decoder().bits == 10
    _render_read_back(mc, 1024)
    with pytest.raises(ValueError, match="cannot fill"):
        encode_mesh_radix(v, f, divide=4, levels=4)
    mc = encode_mesh_radix(v, f, divide=4, levels=4, upsample=True)
    torch.cuda.synchronize()
    assert len(mc.vertices) == 257 and mc.divide == 4 and mc.levels == 4
    assert np.bincount(mc.vertex_ids.cpu().numpy(), minlength=256).min() >= 1
    _render_read_back(mc, 256)
