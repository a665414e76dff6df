"""The ICP oracle (tests/icp_ref.py) on the CPU: against what the reference's own rgbd_to_point_cloud,
best_fit_transform and icp returned for the inputs stored beside the results in tests/golden/icp.npz
(tools/capture_icp_fixture.py), on a noiseless cloud with a known motion, and on the mode and status
rules; and the host-side argument checks of zp_depth_points / zp_icp, which need no GPU.

Tolerances: back-projection is the same single f64 operations, equal bits.  A fit differs from the
reference's only in BLAS's order of summation, 1e-12.  The loop: with every neighbour decided by a
relative margin of at least 1e-9 (asserted) both sides walk the same correspondences, and T to 1e-9."""
import ctypes

import numpy as np
import pytest

from tests import icp_ref as IR
from tests import refine_ref as RF

MODES = {"full": IR.FULL, "depth_only": IR.DEPTH_ONLY, "no_depth": IR.NO_DEPTH}


@pytest.fixture(scope="module")
def fx(golden):
    return golden("icp.npz")


def _k4(K):
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])


def test_back_projection_bits(fx):
    got = IR.depth_points(fx["depth"], _k4(fx["K"]))
    assert got["count"] == len(fx["cloud"]) > 100
    assert np.array_equal(got["pts"].view(np.uint64), np.ascontiguousarray(fx["cloud"]).view(np.uint64))
    c = fx["cloud"].mean(0)
    assert np.abs(got["stats"][:3] - c).max() <= 1e-12 * np.abs(c).max()
    assert abs(got["stats"][3] - np.linalg.norm(fx["cloud"] - c, axis=1).max()) <= 1e-12 * np.abs(c).max()


def test_depth_rule_and_filter():
    d = np.zeros((5, 7), np.float32)
    d[1, 2], d[2, 3], d[3, 1], d[4, 6], d[0, 0] = 500, np.nan, -3, np.inf, 700
    K = [100.0, 90.0, 3.0, 2.0]
    got = IR.depth_points(d, K)
    assert got["count"] == 2 and got["pts"][:, 2].tolist() == [700.0, 500.0]  # row-major: (0, 0) first
    assert IR.depth_points(d, K, cap=1)["count"] == 2 and len(IR.depth_points(d, K, cap=1)["pts"]) == 1
    near = IR.depth_points(d, K, filt=[-5.0, -5.0, 500.0, 10.0], factor=2.0)
    assert near["count"] == 1 and near["pts"][0, 2] == 500.0 and near["edge"] > 1e-9
    none = IR.depth_points(np.zeros((3, 3)), K)
    assert none["count"] == 0 and not none["stats"].any()


@pytest.mark.parametrize("name", sorted(MODES))
def test_best_fit_transform_against_the_reference(fx, name):
    dist, idx, margin = IR.nearest(fx["A"], fx["B"])
    assert margin >= 1e-9 and np.array_equal(idx, fx["nn0"])
    T, R, t, _, _ = IR.best_fit_transform(fx["A"], fx["B"][idx], MODES[name])
    scale = np.abs(fx[f"fit_{name}_T"]).max()
    assert np.abs(T - fx[f"fit_{name}_T"]).max() <= 1e-12 * scale
    assert np.abs(R - fx[f"fit_{name}_R"]).max() <= 1e-12 and np.abs(t - fx[f"fit_{name}_t"]).max() <= 1e-12 * scale


@pytest.mark.parametrize("name", sorted(MODES))
def test_icp_against_the_reference(fx, name):
    r = IR.icp(fx["A"], fx["B"], 200, 5e-7, MODES[name])
    assert min(r["margins"]) >= 1e-9, min(r["margins"])
    assert r["iterations"] == int(fx[f"icp_{name}_i"]) + 1
    assert np.abs(r["T"] - fx[f"icp_{name}_T"]).max() <= 1e-9 * np.abs(fx[f"icp_{name}_T"]).max()
    assert abs(r["mean_error"] - fx[f"icp_{name}_dist"].mean()) <= 1e-9


def cloud(seed, n, spread=(40.0, 30.0, 20.0)):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)) * np.array(spread) + np.array([3.0, -4.0, 600.0])


def moved(A, axis, deg, shift):
    c = A.mean(0)
    R = RF.rodrigues(axis, np.deg2rad(deg))
    return (A - c) @ R.T + c + np.asarray(shift, np.float64), R, c


def test_oracle_recovers_a_known_motion():
    """Noiseless, a motion well inside the basin: every point ends on its own image and T is the motion."""
    A = cloud(1, 150)
    B, R, c = moved(A, [0.2, 0.9, -0.3], 2.0, [0.8, -0.5, 0.6])
    perm = np.random.default_rng(2).permutation(len(A))
    r = IR.icp(A, B[perm], 200, 1e-12)
    assert np.array_equal(perm[r["nn"]], np.arange(len(A)))
    assert r["mean_error"] < 1e-9
    assert np.abs(r["T"][:3, :3] - R).max() < 1e-10
    assert np.abs(r["T"][:3, :3] @ A.T + r["T"][:3, 3:] - B.T).max() < 1e-9


def test_modes_and_statuses():
    A = cloud(3, 80)
    B, _, _ = moved(A, [0.1, 0.2, 0.9], 3.0, [1.0, 0.5, -2.0])
    R0, t0 = RF.rodrigues([1, 2, 3], 0.4), np.array([1.0, 2.0, 500.0])
    u = (np.arange(80) + 0.5) / 80  # draw i picks point i
    full = IR.icp_pose(A, B, u, u, R0, t0)
    assert full["status"] == 0 and full["n"] == 80 and full["iterations"] >= 2
    assert np.abs(full["R"].T @ full["R"] - np.eye(3)).max() < 1e-12
    only = IR.icp_pose(A, B, u, u, R0, t0, mode=IR.DEPTH_ONLY)
    assert only["status"] == 0 and np.array_equal(only["T"][:3, :3], np.eye(3))
    flat = IR.icp_pose(A, B, u, u, R0, t0, mode=IR.NO_DEPTH)
    assert flat["status"] == 0 and flat["T"][2, 3] == 0.0
    # the subsample: n = min(n_src, n_dst, N), draws -> indices with replacement
    few = IR.icp_pose(A, B[:50], u, u[::-1], R0, t0, N=64)
    assert few["n"] == 50 and np.array_equal(few["A"], A[IR.draw_indices(u[:50], 80)])
    assert np.array_equal(few["B"], B[IR.draw_indices(u[::-1][:50], 50)])
    # statuses: the pose goes through untouched
    big, _, _ = moved(A, [0, 0, 1], 30.0, [0, 0, 0])
    far = IR.icp_pose(A, big, u, u, R0, t0, mode=IR.NO_DEPTH)
    assert far["status"] == 3 and IR.rotation_angle(far["T"]) > IR.ANGLE_LIMIT
    assert np.array_equal(far["R"], R0) and np.array_equal(far["t"], t0)
    assert IR.icp_pose(A, big, u, u, R0, t0)["status"] == 0  # the limit belongs to no_depth alone
    assert IR.icp_pose(np.zeros((0, 3)), B, u, u, R0, t0)["status"] == 1
    assert IR.icp_pose(A, B[:3], u, u, R0, t0)["status"] == 2 and IR.icp_pose(A, B[:4], u, u, R0, t0)["status"] == 0
    assert abs(IR.rotation_angle(np.eye(4))) == 0.0
    T30 = np.eye(4)
    T30[:3, :3] = RF.rodrigues([0.3, -0.2, 0.9], np.deg2rad(30.0))
    assert abs(IR.rotation_angle(T30) - np.deg2rad(30.0)) < 1e-14


def _err():
    from zebrapose_amd import _lib as L
    return L.lib.zp_last_error().decode()


def test_ws_bytes_reject_bad_sizes():
    from zebrapose_amd import _lib as L
    dp, ic = L.lib.zp_depth_points_ws_bytes, L.lib.zp_icp_ws_bytes
    assert dp(1, 480, 640, 480 * 640) >= 0 and dp(32, 480, 640, 480 * 640) >= 0 and ic(1, 3000) >= 0 and ic(32, 4096) >= 0
    for bad in [(0, 4, 4, 16), (1, 0, 4, 16), (1, 4, 0, 16), (1, 4, 4, 0), (70000, 4, 4, 16), (1, 1 << 15, 4, 16),
                (1, 8192, 8192, 16), (1, 4, 4, (1 << 24) + 1), (1024, 4, 4, 1 << 20)]:
        assert dp(*bad) == -1, bad
    for bad in [(0, 100), (1, 0), (1, 4097), (-1, 100), (70000, 100)]:
        assert ic(*bad) == -1, bad


def test_entry_points_reject_bad_arguments():
    """Every check comes before the first device call: rc 1, zp_last_error names the function, and the
    stand-in pointers are never read."""
    from zebrapose_amd import _lib as L
    P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(16)]

    def icp(B=2, N=100, src=P[0], ns=P[1], scap=10, dst=P[2], nd=P[3], dcap=10, ds=P[4], dd=P[5], iters=200, tol=5e-7,
            mode=0, frac=0.05, ang=0.35, R=P[6], t=P[7], Ro=P[8], to=P[9], st=P[10], it=P[11], err=P[12]):
        return L.lib.zp_icp(B, N, src, ns, scap, dst, nd, dcap, ds, dd, iters, tol, mode, frac, ang, R, t, Ro, to, st, it,
                            err, None, None, None, None)

    for kw in [dict(B=0), dict(N=0), dict(N=4097), dict(iters=0), dict(tol=float("nan")), dict(mode=3), dict(mode=-1),
               dict(scap=0), dict(dcap=0), dict(frac=-1.0), dict(frac=float("inf")), dict(ang=float("nan")),
               dict(src=None), dict(nd=None), dict(ds=None), dict(dd=None), dict(R=None), dict(Ro=None), dict(st=None),
               dict(it=None), dict(err=None), dict(Ro=P[6]), dict(to=P[7])]:
        assert icp(**kw) == 1, kw
        assert _err().startswith("zp_icp:"), (kw, _err())

    def dpts(B=2, H=8, W=8, depth=P[0], K=P[1], cap=64, filt=None, factor=2.0, counts=P[2], pts=P[3], stats=None):
        return L.lib.zp_depth_points(B, H, W, depth, K, cap, filt, factor, counts, pts, stats, None, None)

    for kw in [dict(B=0), dict(H=0), dict(W=0), dict(cap=0), dict(depth=None), dict(K=None), dict(counts=None),
               dict(pts=None), dict(filt=P[4], factor=float("nan")), dict(filt=P[4], factor=-1.0),
               dict(filt=P[4], stats=P[4])]:
        assert dpts(**kw) == 1, kw
        assert _err().startswith("zp_depth_points:"), (kw, _err())
