"""zp_pnp_lo at its edges, against tests/pnp_lo_ref.py: the block reduction's sizes (one step from a
perturbed pose: Hb within the worst-case summation bound, the pose within 64 cond 2^-52, inliers
exact), the statuses and their bit-for-bit copy-through beside a neighbour that is still refined,
degenerate geometry, and the argument checks (those run without a GPU)."""
import ctypes

import numpy as np
import pytest

from tests import pnp_cases as PC
from tests import pnp_lo_cases as C
from tests import pnp_lo_ref as LO


@pytest.mark.gpu
def test_reduction_edges(gpu):
    from tests.test_gpu_pnp_lo import run_lo
    cases, refs = C.edge_cases(), C.edge_refs()
    assert tuple(len(c[0][0]) for c in cases) == PC.EXACT_SIZES
    counts, xy, xyz = PC.batch([c[0] for c in cases], HW=PC.EXACT_HW, garbage_tail=True)
    R0, t0 = np.stack([c[2] for c in cases]), np.stack([c[3] for c in cases])
    got = run_lo(gpu, counts, xy, xyz, [c[1] for c in cases], R0, t0, reproj_err=C.EDGE_THR, rounds=1, steps=1)
    for b, ref in enumerate(refs):
        n = int(counts[b])
        assert got["status"][b] == 0 and got["inliers"][b] == ref["inliers"], n
        assert np.array_equal(got["trace"][b], ref["trace"]), n
        err = np.abs(got["Hb"][b] - ref["Hb"])
        assert np.all(err <= C.hb_bound(ref, n)), (n, (err / np.maximum(C.hb_bound(ref, n), 1e-300)).max())
        tol = C.step_tol(ref)
        dR, dt = np.abs(got["R"][b].reshape(3, 3) - ref["R"]).max(), np.abs(got["t"][b] - ref["t"]).max()
        print(f"n {n}: |dR| {dR:.3g}, |dt| {dt:.3g} / {np.abs(ref['t']).max():.4g}, tol {tol:.3g}")
        assert dR <= tol and dt <= tol * np.abs(ref["t"]).max(), (n, tol)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.gpu
def test_statuses_copy_the_pose_through(gpu):
    from tests.test_gpu_pnp_lo import run_lo
    sc = C.noisy_scene(300, 31)
    R, t, _ = C.ransac_pose(300, 31)
    nan_R = R.copy()
    nan_R[2, 0] = np.nan
    far = t + np.array([0.0, 0.0, 5000.0])
    five = (sc[0][:5], sc[1][:5])
    #        scene  pose         active status
    rows = [(sc, (R, t), 0, 1), (five, (R, t), 1, 1), (sc, (nan_R, t), 1, 1), (sc, (R, far), 1, 2), (sc, (R, t), 1, 0)]
    counts, xy, xyz = PC.batch([r[0] for r in rows], HW=333, garbage_tail=True)
    Rin, tin = np.stack([r[1][0] for r in rows]), np.stack([r[1][1] for r in rows])
    got = run_lo(gpu, counts, xy, xyz, [C.K0] * len(rows), Rin, tin, active=[r[2] for r in rows])
    assert got["status"].tolist() == [r[3] for r in rows]
    for b, (scene, pose, act, status) in enumerate(rows[:4]):
        assert np.array_equal(_bits(got["R"][b]), _bits(pose[0]).reshape(9)), b
        assert np.array_equal(_bits(got["t"][b]), _bits(pose[1])), b
        assert got["cost"][b] == 0 and np.all(got["Hb"][b] == 0)
        ref = LO.refine(scene[0], scene[1], C.K0, pose[0], pose[1], active=bool(act))
        assert ref["status"] == status and got["inliers"][b] == ref["inliers"]
        assert np.array_equal(got["trace"][b], ref["trace"])
    assert got["inliers"][:3].tolist() == [0, 0, 0] and 0 <= got["inliers"][3] < 6
    # the neighbour is refined as if alone
    ref = C.noisy_ref(300, 31)[0][0]
    assert np.array_equal(got["trace"][4], ref["trace"]) and got["inliers"][4] == ref["inliers"]
    alone = run_lo(gpu, *PC.batch([sc], HW=333), [C.K0], R[None], t[None])
    for key in got:
        assert np.asarray(got[key][4]).tobytes() == np.asarray(alone[key][0]).tobytes(), key


@pytest.mark.gpu
def test_degenerate_geometry(gpu):
    from tests.test_gpu_pnp_lo import run_lo
    behind, Rb, tb = C.behind_scene()
    ident = PC.identical(np.random.default_rng(7710), 50)
    coll = PC.collinear(np.random.default_rng(7711), 50)
    rows = [(ident, ident[2], ident[3]), (coll, coll[2], coll[3]), (behind, Rb, tb)]
    counts, xy, xyz = PC.batch([r[0] for r in rows], HW=400, garbage_tail=True)
    got = run_lo(gpu, counts, xy, xyz, [C.K0] * 3, np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]))
    Zb = LO.project(behind[0].astype(np.float64), behind[1].astype(np.float64), Rb, tb, LO.kvec(C.K0))[2]
    assert 150 <= int((Zb <= 0).sum()) <= 250
    for b, (sc, R0, t0) in enumerate(rows):
        ref = LO.refine(sc[0], sc[1], C.K0, R0, t0)
        assert ref["status"] in (0, 2) and got["status"][b] == ref["status"], b
        for key in ("R", "t", "cost", "Hb"):
            assert np.all(np.isfinite(got[key][b])), (b, key)
        Rg, tg = got["R"][b].reshape(3, 3), got["t"][b]
        m0, m1 = LO.truncated_cost(sc[0], sc[1], R0, t0, C.K0), LO.truncated_cost(sc[0], sc[1], Rg, tg, C.K0)
        assert m1 <= m0 * (1 + len(sc[0]) * 2.0 ** -50), (b, m0, m1)
        mask, _ = LO.select(sc[0].astype(np.float64), sc[1].astype(np.float64), Rg, tg, LO.kvec(C.K0), C.THR ** 2)
        Z = LO.project(sc[0].astype(np.float64), sc[1].astype(np.float64), Rg, tg, LO.kvec(C.K0))[2]
        assert got["inliers"][b] == (int(mask.sum()) if ref["status"] == 0 else ref["inliers"]) and not np.any(mask & (Z <= 0))
        assert got["inliers"][b] <= int((Z > 0).sum())


def test_argument_checks_without_gpu():
    """every bad call is ZP_ERR_ARG with a message, before any device call"""
    from zebrapose_amd import _lib as L
    lib = L.lib
    assert lib.zp_pnp_lo_ws_bytes(0, 16) == -1 and lib.zp_pnp_lo_ws_bytes(4, 0) == -1
    assert lib.zp_pnp_lo_ws_bytes(65536, 16) == -1 and lib.zp_pnp_lo_ws_bytes(1, (1 << 24) + 1) == -1
    assert lib.zp_pnp_lo_ws_bytes(32, 16384) >= 32 * 16384 // 8
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    q = p + 256

    def call(rounds=4, steps=10, err=2.0, status=p, R_out=q, B=1, HW=16):
        return lib.zp_pnp_lo(B, HW, p, p, p, p, p, p, None, err, rounds, steps, R_out, q, p, p, status, None, None, p, None)

    for kw, word in ((dict(rounds=0), b"rounds"), (dict(rounds=65), b"rounds"), (dict(steps=65), b"steps"),
                     (dict(steps=0), b"steps"), (dict(err=0.0), b"reproj_err"), (dict(err=float("inf")), b"reproj_err"),
                     (dict(err=float("nan")), b"reproj_err"), (dict(status=None), b"NULL"), (dict(R_out=p), b"in place"),
                     (dict(B=0), b"sizes"), (dict(HW=(1 << 24) + 1), b"sizes")):
        assert call(**kw) == 1, kw
        assert word in lib.zp_last_error(), (kw, lib.zp_last_error())
