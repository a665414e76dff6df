"""Host side of the mesh upsampling (no GPU): the numpy restatement tests/subdiv_ref.py keeps the
properties zp_mesh_subdivide's contract implies (closed meshes stay closed with no T-junction, the
surface is unchanged, the budget lands exactly on the target, the longest edge never grows), and the
library's argument checks fail cleanly before any device call."""
import ctypes

import numpy as np
import pytest

from tests import subdiv_ref as SR


def test_tetrahedron_full_split():
    v, f = SR.tetrahedron()
    before = SR.area(v, f)
    r = SR.subdivide_pass(v, f)
    assert r["vertices"].shape == (10, 3) and r["faces"].shape == (16, 3)
    assert np.array_equal(r["counts"], [6, 6, 10, 16])
    assert SR.is_closed_manifold(r["faces"])
    assert before == 13.856406460551018 and SR.area(r["vertices"], r["faces"]) == 13.856406460551018
    assert np.array_equal(r["parents"][:4], np.stack([np.arange(4)] * 2, 1))
    assert np.array_equal(r["parents"][4:], [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)])
    assert np.array_equal(r["vertices"][4], [1, 0, 0]) and r["max_len2"] == 8.0


@pytest.fixture(scope="module")
def box_runs():
    v, f = SR.box()
    assert len(v) == 8 and len(f) == 12 and SR.is_closed_manifold(f)
    return v, f, {n: SR.upsample_mesh(v, f, min_vertices=n) for n in (9, 100, 1025, 4097)}


@pytest.mark.parametrize("target,passes", [(9, 1), (100, 3), (1025, 6), (4097, 7)])
def test_box_upsampled_to_a_target(box_runs, target, passes):
    v, f, runs = box_runs
    r = runs[target]
    assert len(r["pass_sizes"]) == passes
    assert len(r["vertices"]) == target == r["pass_sizes"][-1]
    assert SR.is_closed_manifold(r["faces"])
    assert len(r["vertices"]) - len(r["faces"]) / 2 == 2
    a0, a1 = SR.area(v, f), SR.area(r["vertices"], r["faces"])
    assert abs(a1 - a0) <= 1e-9 * a0
    longest = r["max_len2"] + [SR.longest_edge2(r["vertices"], r["faces"])]
    assert all(b <= a for a, b in zip(longest, longest[1:])), longest
    assert np.array_equal(r["vertices"][:8], v)


def test_upsample_leaves_a_large_enough_mesh_alone_and_refuses_a_point():
    v, f = SR.box()
    r = SR.upsample_mesh(v, f, min_vertices=8)
    assert r["pass_sizes"] == [] and r["vertices"] is not None and np.array_equal(r["faces"], f)
    with pytest.raises(ValueError, match="split nothing"):
        SR.upsample_mesh(np.zeros((3, 3), np.float32), [(0, 1, 2)], min_vertices=5)
    with pytest.raises(ValueError, match="max_passes"):
        SR.upsample_mesh(v, f, min_vertices=4097, max_passes=3)


def test_threshold_and_lift():
    v, f = SR.box()
    r = SR.subdivide_midpoint(v, f, iterations=2, threshold=10.5)  # past the 10 x 1 faces' diagonal
    assert SR.is_closed_manifold(r["faces"])
    assert len(r["pass_sizes"]) == 2 and r["pass_sizes"][-1] == len(r["vertices"])
    one = SR.subdivide_midpoint(v, f)
    lifted = SR.lift(v, one["parents"], len(v), one["pass_sizes"])
    assert np.array_equal(lifted.astype(np.float32), one["vertices"])
    none = SR.subdivide_pass(v, f, abs2=1e9)
    assert np.array_equal(none["counts"], [18, 0, 8, 12]) and np.array_equal(none["faces"], f)


def test_zp_mesh_subdivide_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    lib = _lib.lib
    assert lib.zp_mesh_subdivide_ws_bytes(0, 1) == -1
    for nv, nf in [(1, 0), (-3, 4), ((1 << 21) + 1, 4), (8, (1 << 24) + 1)]:
        assert lib.zp_mesh_subdivide_ws_bytes(nv, nf) == -1, (nv, nf)
    assert lib.zp_mesh_subdivide_ws_bytes(8, 12) >= 36 * (8 * 4 + 4 * 5) + 12 * 8
    assert lib.zp_mesh_subdivide_ws_bytes(1 << 21, 1 << 24) > 0
    buf = (ctypes.c_double * 64)()  # stands in for every pointer: the checks fail before any of them is used
    p = ctypes.addressof(buf)
    good = dict(verts=p, nv=8, faces=p, nf=12, abs2=0.0, rel2=0.25, max_split=5, out_verts=p, cap_v=13, out_faces=p,
                cap_f=48, parents=p, counts=p, max_len2=p, ws=p, stream=None)
    cases = [(dict(rel2=1.0), b"rel2"), (dict(rel2=-0.5), b"rel2"), (dict(rel2=float("nan")), b"rel2"),
             (dict(abs2=-1.0), b"abs2"), (dict(max_split=-1), b"max_split"), (dict(nv=0), b"nv"),
             (dict(nf=(1 << 24) + 1), b"nf"), (dict(cap_v=-1), b"cap_v"), (dict(verts=None), b"NULL"),
             (dict(counts=None), b"NULL"), (dict(max_len2=None), b"NULL"), (dict(ws=None), b"NULL"),
             (dict(parents=None), b"NULL")]
    for bad, word in cases:
        rc = lib.zp_mesh_subdivide(*{**good, **bad}.values())
        assert rc == 1, bad
        assert word in lib.zp_last_error(), (bad, lib.zp_last_error())
