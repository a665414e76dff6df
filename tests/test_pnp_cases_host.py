"""Preconditions of tests/test_gpu_pnp_edges.py, checked on the oracle alone (oracle/pnp_ref.py,
numpy f64): a badly built input fails here, on the CPU, before any device run.  No GPU needed."""
import warnings

import numpy as np
import pytest

from oracle import pnp_ref
from tests import pnp_cases as C

# (c) what the oracle makes of each degenerate case: does it solve it (pnp_cases.oracle_solves:
# success, finite, and the same answer again under a 1e-13 perturbation), and does the final EPnP
# over its inlier set pass the conditioning guard (pnp_cases.well_posed).  The device is compared
# with the oracle where "solved", with the truth where "well_posed" too; elsewhere only the
# invariants apply.
#   identical: every hypothesis is 0 / 0, RANSAC finds no model
#   collinear: RANSAC returns a pose with a handful of inliers, but the rotation about the line
#              is free and the 1e-13 perturbation turns it by tens of degrees
ORACLE_TABLE = {
    "slab": {"solved": True, "well_posed": True},
    "planar": {"solved": True, "well_posed": True},
    "coarse_lut": {"solved": True, "well_posed": True},
    "small_far": {"solved": True, "well_posed": True},
    "off_centre": {"solved": True, "well_posed": True},
    "identical": {"solved": False, "well_posed": False},
    "collinear": {"solved": False, "well_posed": False},
}


def test_builders_are_deterministic_and_typed():
    for make in (C.degenerate_cases, lambda: {i: s for i, (s, _) in enumerate(C.exact_cases(True))}):
        a, b = make(), make()
        assert list(a) == list(b)
        for k in a:
            pw, uv, R, t = a[k]
            assert pw.dtype == np.float32 and uv.dtype == np.int32 and pw.shape == (len(uv), 3) and uv.shape[1] == 2
            assert np.array_equal(pw, b[k][0]) and np.array_equal(uv, b[k][1])
            assert np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0 and t[2] > 0


def test_shapes_are_what_they_claim():
    rng = np.random.default_rng(3)
    pw = C.cube(rng, 500)[0]
    assert np.abs(pw).max() < 62 and np.abs(pw).max() > 50
    pw = C.slab(rng, 500)[0]
    assert np.abs(pw[:, 2]).max() <= 0.5 and np.abs(pw[:, 2]).max() > 0.3 and np.abs(pw[:, :2]).max() > 50
    pw = C.planar(rng, 500)[0]
    assert np.all(pw[:, 2] == 0.0) and np.abs(pw[:, :2]).max() > 50
    pw, uv, _, _ = C.coarse_lut(rng)
    assert len(pw) == 4000 and len(np.unique(pw, axis=0)) == 64 and len(np.unique(uv, axis=0)) <= 64
    pw, uv, _, _ = C.coarse_lut_spread(rng)
    assert len(pw) == 4000 and len(np.unique(pw, axis=0)) == 64 and len(np.unique(uv, axis=0)) > 2000
    pw, _, _, t = C.small_far(rng, 500)
    assert np.abs(pw).max() < 7 and t[2] == 1500.0
    uv = C.off_centre(rng, 500)[1]
    assert (uv < 0).any(axis=1).mean() > 0.25 and uv.min() > -150
    pw = C.identical(rng)[0]
    assert len(pw) == 50 and len(np.unique(pw, axis=0)) == 1
    pw = C.collinear(rng)[0].astype(np.float64)
    assert len(pw) == 50 and np.linalg.matrix_rank(pw) == 1 and np.all(np.cross(pw, pw[np.abs(pw[:, 0]).argmax()]) == 0)


@pytest.mark.parametrize("per_crop_K", [False, True])
def test_exact_scenes_hit_their_pixels_and_are_well_posed(per_crop_K):
    """(a): the only noise is the f32 rounding of pw; the final EPnP is well conditioned; at the
    1e4 px threshold the oracle's RANSAC keeps all n points, so the refine runs over all of them."""
    cases = C.exact_cases(per_crop_K)
    assert [len(s[0]) for s, _ in cases] == list(C.EXACT_SIZES)
    if per_crop_K:
        Ks = np.stack([K for _, K in cases])
        for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)):
            r = Ks[:, i, j] / C.K0[i, j]
            assert r.min() >= 0.8 and r.max() <= 1.2 and r.max() - r.min() > 0.1
    for (pw, uv, R, t), K in cases:
        n = len(pw)
        assert np.abs(C.project(pw, R, t, K)[0] - uv).max() < 1e-3, n
        assert np.float32(C.EXACT_THRESHOLD ** 2) == 1e8  # thr^2 is an exact f32
        assert C.well_posed(pw, uv, K), n
        ref = pnp_ref.solve_pnp_ransac(pw, uv.astype(np.float32), K, reprojection_error=C.EXACT_THRESHOLD)
        assert ref["success"] and ref["inliers"] == n, n
        Rr, tr = pnp_ref.epnp(pw, uv.astype(np.float32), K)
        assert C.rot_angle_deg(Rr, R) < 1e-3 and np.linalg.norm(tr - t) < 1e-5 * np.linalg.norm(t), n


def test_degenerate_cases_against_the_oracle_table():
    """(c): the oracle raises on none of the cases, and solves / finds well-posed exactly the ones
    ORACLE_TABLE says; where both, the oracle itself returns the true pose to half the device's
    bound (0.25 degree, 0.5 %)."""
    cases = C.degenerate_cases()
    assert set(cases) == set(ORACLE_TABLE)
    for name, (pw, uv, R, t) in cases.items():
        assert len(pw) <= 2000
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # 0 / 0 in the degenerate hypotheses
            ref, solved = C.oracle_solves(pw, uv)
            assert solved == ORACLE_TABLE[name]["solved"], name
            wp = bool(ref["success"]) and C.well_posed(*[a[C.oracle_inliers(ref, pw, uv, C.K0)] for a in (pw, uv)], C.K0)
        assert wp == ORACLE_TABLE[name]["well_posed"], name
        if solved and wp:
            assert C.rot_angle_deg(ref["R"], R) < 0.25 and np.linalg.norm(ref["t"] - t) < 5e-3 * np.linalg.norm(t), name


def test_iteration_scene_is_settled_in_the_first_chunk():
    """(d): at 32, 33 and 1000 iterations the oracle holds the scene's consensus (about half of
    the 800 points, the true pose to 0.25 degree); one iteration finds nothing"""
    pw, uv, R, t = C.iteration_scene()
    assert len(pw) == 800
    assert not pnp_ref.solve_pnp_ransac(pw, uv.astype(np.float32), C.K0, iterations=1)["success"]
    for it in (32, 33, 1000):
        ref = pnp_ref.solve_pnp_ransac(pw, uv.astype(np.float32), C.K0, iterations=it)
        assert ref["success"] and ref["inliers"] > 350 and ref["best"] < 32 + (it == 1000) * 1000, it
        assert C.rot_angle_deg(ref["R"], R) < 0.25 and np.linalg.norm(ref["t"] - t) < 5e-3 * np.linalg.norm(t), it


def test_oracle_epnp_carries_nan_without_raising():
    """one repeated 3D point, an exactly planar set and a collinear set: epnp() returns (NaN where
    the C++ would), it does not raise"""
    cases = C.degenerate_cases()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name in ("identical", "planar", "collinear"):
            pw, uv, _, _ = cases[name]
            R, t = pnp_ref.epnp(pw[:50], uv[:50].astype(np.float32), C.K0)
            assert R.shape == (3, 3) and t.shape == (3,)
            if name == "identical":
                assert not np.all(np.isfinite(R))
