"""Preconditions of tests/icp_cases.py, checked on the oracle (tests/icp_ref.py) alone, so that no
check of tests/test_gpu_icp_edges.py can pass vacuously: every degenerate case has the rank it is
built for (the oracle's singular values of H), the reflection case a best orthogonal fit of
determinant -1, every loop-exit case its iteration count, every boundary case its side, and every
neighbour that is compared exactly a relative margin of 1e-9.

The oracle needed one change for these inputs: draw_indices() cast NaN and negative products to
int64 (undefined, and a negative index wraps); it now gives the index the contract's "floor(draw *
count) as an index below count" implies for any draw.  numpy's SVD returns finite, orthonormal
factors on every H here (H = 0 included): nothing else had to be carried."""
import numpy as np
import pytest

from tests import icp_cases as C
from tests import icp_ref as IR

MARGIN = 1e-9


def _svd_fit(w):
    """(U V^T's determinant before the fix, the oracle's own R of the first fit)"""
    U, _, Vt = np.linalg.svd(w["H"])
    return np.linalg.det(Vt.T @ U.T), IR.best_fit_transform(w["A"], w["B"][w["nn"]])[1]


def test_draw_indices_at_the_ends():
    one = 1.0 - 2.0 ** -53
    d = [0.0, one, 1.0, 1.5, 1e300, np.inf, -1e-300, -0.5, -np.inf, -0.0, np.nan, 0.5]
    assert IR.draw_indices(d, 19).tolist() == [0, 18, 18, 18, 18, 18, 0, 0, 0, 0, 0, 9]
    assert IR.draw_indices(d, 1).tolist() == [0] * 12
    assert one * 19.0 < 19.0  # the largest draw below 1 stays below count: no count rounds it up
    u = np.random.default_rng(0).random(1000)
    assert np.array_equal(IR.draw_indices(u, 77), np.floor(u * 77).astype(np.int64))
    w = C.run(C.draw_ends())
    assert w["status"] == 0 and w["n"] == 16 and w["iterations"] == 1 and w["margins"][0] >= MARGIN
    c = C.draw_ends()
    assert np.array_equal(w["A"], c["src"][[0, 18, 18, 18, 18, 18, 0, 0, 0, 0, 0, 9, 1, 0, 18, 18]])
    assert np.array_equal(w["B"], c["dst"][IR.draw_indices(c["ud"], 21)]) and np.isfinite(w["T"]).all()


@pytest.mark.parametrize("name", sorted(C.fit_cases()))
def test_fit_cases_have_the_intended_conditioning(name):
    c, target = C.fit_cases()[name]
    w = C.run(c)
    S = w["S"]
    assert w["status"] == 0 and w["n"] == 200 and w["iterations"] == 1 and w["margins"][0] >= MARGIN
    if target is not None:
        assert target / 2 <= S[1] / S[0] <= 2 * target, S
    else:
        assert S[1] >= 0.1 * S[0]
    if "planar" in name:
        assert S[2] <= 1e-9 * S[1]
    elif "needle" in name:
        assert S[2] >= 0.5 * S[1]
    else:
        assert 1e-3 * S[1] <= S[2] <= 0.6 * S[1]
    det, R = _svd_fit(w)
    assert det > 0 or "planar" in name  # no reflection (a plane's third pair has no sign of its own)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14


@pytest.mark.parametrize("name", sorted(C.degenerate_cases()))
def test_degenerate_cases_have_the_intended_rank(name):
    c, rank = C.degenerate_cases()[name]
    w = C.run(c)
    S = w["S"]
    assert w["status"] == 0 and w["iterations"] == 1 and w["margins"][0] >= MARGIN
    assert np.isfinite(w["T"]).all() and np.isfinite(w["R"]).all() and np.isfinite(w["t"]).all()
    if rank == 0:
        assert not w["H"].any() and not S.any()
    elif rank == 1:
        assert S[0] > 0 and S[1] <= 1e-14 * S[0]
        if name == "collinear_exact":  # integers: H = 80 d d'^T, every entry exact
            assert np.array_equal(w["H"], 80.0 * np.outer([1.0, 2.0, 2.0], [2.0, -1.0, 2.0]))
    else:
        assert S[2] > 1e-7 * S[0] and S[2] < 0.9 * S[1]  # full rank, the flipped pair distinct from the second
    det, R = _svd_fit(w)
    if name.startswith("mirrored"):
        assert det < 0  # the best orthogonal fit is a reflection ...
        assert np.array_equal(w["B"][w["nn"]][:, 1] - w["B"][w["nn"]][:, 1].min(), w["A"][:, 1] - w["A"][:, 1].min())
    # ... and the oracle's fix returns a rotation on every one of them
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14


@pytest.mark.parametrize("n,N", C.SIZE_PAIRS)
def test_sizes(n, N):
    w = C.run(C.sized(n, N))
    assert w["status"] == 0 and w["n"] == n and len(w["nn"]) == n and w["margins"][0] >= MARGIN
    if n >= 63:
        assert w["S"][2] > 0.05 * w["S"][0]
    else:
        assert np.linalg.matrix_rank(w["H"], tol=1e-12 * max(np.abs(w["H"]).max(), 1e-300)) == n - 1


@pytest.mark.parametrize("name", sorted(C.loop_cases()))
def test_loop_exits(name):
    c, its = C.loop_cases()[name]
    w = C.run(c)
    assert w["status"] == 0 and min(w["margins"]) >= MARGIN
    assert c["N"] <= 256 and c["kw"].get("max_iterations", 200) <= 1000
    if its is None:
        assert 3 < w["iterations"] < 200
    else:
        assert w["iterations"] == its
    if name == "subset":
        assert w["mean_error"] == 0.0 and w["n"] == 40
    if name == "tolerance_0":  # it would have stopped long before under the default tolerance
        assert C.run(c, tolerance=5e-7)["iterations"] < 20


def test_status_boundaries():
    for c, status in C.fraction_cases():
        ns, nd, frac = len(c["src"]), len(c["dst"]), c["kw"]["min_fraction"]
        w = C.run(c)
        assert w["status"] == status, c["name"]
        assert (float(nd) < float(ns) * frac) == (status == 2)
        if status == 0:
            assert min(w["margins"]) >= MARGIN and w["n"] == nd
            # every point's neighbour is its own image, so the fit of these few points is unique
            # (one point: H = 0 and the identity on both sides) and the loops walk the same pairs
            assert np.array_equal(w["nn"], np.arange(nd))
            assert nd == 1 or w["S"][2] >= 1e-3 * w["S"][0], w["S"]
    assert 80 * 0.0625 == 5.0 and 7 * 0.5 == 3.5
    theta, cases = C.angle_cases()
    assert np.deg2rad(5) < theta < np.deg2rad(12)
    for c, status in cases:
        w = C.run(c)
        assert w["status"] == status and min(w["margins"]) >= MARGIN
        assert (IR.rotation_angle(w["T"]) > c["kw"]["angle_limit"]) == (status == 3)
        assert abs(c["kw"]["angle_limit"] / theta - 1) >= 0.9e-6  # 1e6 times the solvers' 1e-12
    for src, dst, status in [(*C.neighbours()[0], 1), (*C.neighbours()[1], 2)]:
        assert IR.icp_pose(src, dst, np.full(128, 0.5), np.full(128, 0.5), C.R0, C.T0)["status"] == status


def test_depth_cases():
    d = C.depth_cases()
    w = IR.depth_points(d["special_values"]["depth"][0], d["special_values"]["K"][0])
    assert w["count"] == 5 and np.isfinite(w["pts"]).all()  # two denormals, 500, near the largest f32, 1
    assert w["pts"][:, 2].tolist() == [float(np.float32(1e-45)), 500.0, float(np.float32(1.1e-38)), float(np.float32(3.4e38)), 1.0]
    t = d["tiles"]["depth"]
    assert [IR.depth_points(t[b], d["tiles"]["K"][b])["count"] for b in range(3)][1:] == [1024, 3072]
    assert (t[0, :16] > 0).all() and not t[0, 16:32].any() and 0 < (t[0, 32:] > 0).sum() < 1024
    assert all(IR.depth_points(t[b], d["tiles"]["K"][b])["count"] > d["tiles_cap"]["cap"] for b in range(3))
    f = d["filter_on_the_radius"]
    full = IR.depth_points(f["depth"][0], f["K"][0])["pts"]
    assert np.array_equal(full, np.round(full))  # integers: every squared distance is exact
    d2 = ((full - f["filt"][0, :3]) ** 2).sum(1)
    assert (d2 == 25.0).sum() == 4 and (d2 < 25.0).sum() == 22
    w = IR.depth_points(f["depth"][0], f["K"][0], filt=f["filt"][0], factor=f["factor"])
    assert w["count"] == 22 and w["edge"] == 0.0
    z = d["filter_factor_0"]
    assert IR.depth_points(z["depth"][0], z["K"][0], filt=z["filt"][0], factor=0.0)["count"] == 0
    for name, c in d.items():
        if not c["exact"] and c["filt"] is not None:
            for b in range(len(c["depth"])):
                assert IR.depth_points(c["depth"][b], c["K"][b], c["cap"], c["filt"][b], c["factor"])["edge"] >= MARGIN
