"""The PnP local optimisation without a GPU: the properties of tests/pnp_lo_ref.py (the executable
definition of zp_pnp_lo), the preconditions the device tests rest on, checked on the reference alone,
and the device code's host build (tools/pnp_lo_host_check.hip: csrc/zp_pnp_lo.hip's per-point math and
its loop on the CPU, serial sums) against the reference.

Preconditions.  The device tests compare `trace` exactly, so every decision of the reference on their
scenes has to stand clear of rounding:
  * no point with |r2 - thr^2| <= 1e-6 thr^2 at any selection;
  * no accept / reject decision with |C' - C| <= 1e-9 C.  One kind of decision cannot meet this band:
    the accepted step that ends an LM run has C - C' <= 1e-10 C by the stopping rule itself, and every
    LM run that converges inside `steps` iterations ends with one (all 24 runs of the 8 scenes here do;
    the decreases before it shrink by 1e-2 .. 1e-6 per step).  For those steps the decrease must lie in
    [1e-12 C, 0.9e-10 C]: 1e-12 is above 2 n 2^-53 = 3.4e-13, the worst-case relative rounding of the two
    sums C and C' at n = 1500 in any order, so no summation order turns the acceptance into a rejection,
    and 0.9e-10 keeps the same distance from the stopping rule's own threshold.  Every other decision
    keeps the 1e-9 band.
  * the whole-loop pose bound is 16 x the reference's own spread over three summation orders.  Three
    runs that happen to agree to the bit would give a bound of zero, below the resolution of f64 itself:
    the spread must reach one ulp, 2^-53 for R (entries in [1/2, 1)) and the spacing of the largest |t|.
The seeds in pnp_lo_cases.NOISY are fixed so that all eight scenes qualify; none is skipped."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import pnp_lo_cases as C
from tests import pnp_lo_ref as LO
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pnp_lo") / "pnp_lo_host_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950",
                    os.path.join(ROOT, "tools", "pnp_lo_host_check.hip"), "-o", str(exe)], check=True,
                   capture_output=True)
    return str(exe)


def run_host(exe, tmp_path, pw, uv, K, R, t, reproj_err=2.0, rounds=4, steps=10):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    n = len(pw)
    with open(fin, "wb") as f:
        f.write(struct.pack("iiii", n, rounds, steps, 0))
        f.write(struct.pack("d", reproj_err))
        f.write(LO.kvec(K).tobytes())
        f.write(np.ascontiguousarray(R, np.float64).tobytes())
        f.write(np.ascontiguousarray(t, np.float64).tobytes())
        f.write(np.ascontiguousarray(pw, np.float32).tobytes())
        f.write(np.ascontiguousarray(uv, np.int32).tobytes())
    subprocess.run([exe, str(fin), str(fout)], check=True, capture_output=True)
    raw = open(fout, "rb").read()
    d = np.frombuffer(raw[:41 * 8], np.float64)
    i = np.frombuffer(raw[41 * 8:], np.int32)
    assert len(i) == 2 + 2 * rounds
    return {"R": d[:9].reshape(3, 3), "t": d[9:12], "cost": d[12], "Hb": d[13:41], "inliers": int(i[0]),
            "status": int(i[1]), "trace": i[2:].reshape(rounds, 2)}


def _count(pw, uv, R, t, thr=C.THR):
    return int(LO.select(pw.astype(np.float64), uv.astype(np.float64), R, t, LO.kvec(C.K0), thr * thr)[0].sum())


@pytest.mark.parametrize("n,seed", C.NOISY)
def test_reference_lowers_truncated_cost_and_keeps_consensus(n, seed):
    pw, uv, _, _ = C.noisy_scene(n, seed)
    R, t, _ = C.ransac_pose(n, seed)
    ref = C.noisy_ref(n, seed)[0][0]
    assert ref["status"] == 0
    m0, m1 = LO.truncated_cost(pw, uv, R, t, C.K0), LO.truncated_cost(pw, uv, ref["R"], ref["t"], C.K0)
    i0 = _count(pw, uv, R, t)
    print(f"n {n} seed {seed}: M {m0:.6f} -> {m1:.6f}, f64 inliers {i0} -> {ref['inliers']}, trace {ref['trace'].tolist()}")
    assert m1 < m0
    assert ref["inliers"] >= i0
    assert ref["inliers"] == _count(pw, uv, ref["R"], ref["t"])
    Rm = ref["R"]
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1) < 1e-12


@pytest.mark.parametrize("n,seed", C.NOISY)
def test_preconditions_of_the_exact_trace_comparisons(n, seed):
    runs, tolR, tolt = C.noisy_ref(n, seed)
    assert tolR >= 16 * 2.0 ** -53 and tolt >= 16 * np.spacing(np.abs(runs[0]["t"]).max())
    for ref in runs:  # the scene and its two permutations: the decisions are those of one problem
        sel, dec, last = C.margins(ref)
        print(f"n {n} seed {seed}: selection margin {sel:.3g}, decision margin {dec:.3g}, ending decreases "
              f"{[float(f'{d:.3g}') for d in last]}")
        assert sel > 1e-6
        assert dec > 1e-9
        assert all(1e-12 <= d <= 0.9e-10 for d in last)
        assert np.array_equal(ref["trace"], runs[0]["trace"]) and ref["inliers"] == runs[0]["inliers"]


def test_preconditions_of_the_edge_cases():
    """every size has a set to step on, the outliers are outside it, and no point sits on the threshold
    under the start pose or the stepped one (inliers are compared exactly)"""
    thr2 = C.EDGE_THR ** 2
    for (sc, K, R0, t0), ref in zip(C.edge_cases(), C.edge_refs()):
        n = len(sc[0])
        assert ref["status"] == 0 and ref["trace"][0, 1] == 1 and 6 <= ref["trace"][0, 0] <= n
        if n >= 255:
            assert ref["trace"][0, 0] < n
        _, r2 = LO.select(sc[0].astype(np.float64), sc[1].astype(np.float64), ref["R"], ref["t"], LO.kvec(K), thr2)
        for v in (ref["r2_rounds"][0], r2):
            assert np.abs(v - thr2).min() > 1e-6 * thr2
        assert np.all(np.isfinite(ref["theta0"]))


@pytest.mark.parametrize("n,seed", C.NOISY)
def test_host_program_whole_loop(host_check, tmp_path, n, seed):
    pw, uv, _, _ = C.noisy_scene(n, seed)
    R, t, _ = C.ransac_pose(n, seed)
    runs, tolR, tolt = C.noisy_ref(n, seed)
    ref = runs[0]
    got = run_host(host_check, tmp_path, pw, uv, C.K0, R, t)
    assert got["status"] == 0 and got["inliers"] == ref["inliers"]
    assert np.array_equal(got["trace"], ref["trace"]), (got["trace"], ref["trace"])
    assert np.all(np.abs(got["Hb"] - ref["Hb"]) <= C.hb_bound(ref, n))
    dR, dt = np.abs(got["R"] - ref["R"]).max(), np.abs(got["t"] - ref["t"]).max()
    print(f"n {n} seed {seed}: |dR| {dR:.3g} (bound {tolR:.3g}), |dt| {dt:.3g} (bound {tolt:.3g})")
    assert dR <= tolR and dt <= tolt
    assert abs(got["cost"] - ref["cost"]) <= 1e-9 * ref["cost"]


def test_host_program_single_step_at_the_reduction_edges(host_check, tmp_path):
    for (sc, K, R0, t0), ref in zip(C.edge_cases(), C.edge_refs()):
        n = len(sc[0])
        got = run_host(host_check, tmp_path, sc[0], sc[1], K, R0, t0, reproj_err=C.EDGE_THR, rounds=1, steps=1)
        assert got["status"] == 0 and got["inliers"] == ref["inliers"], n
        assert np.array_equal(got["trace"], ref["trace"])
        assert np.all(np.abs(got["Hb"] - ref["Hb"]) <= C.hb_bound(ref, n)), n
        tol = C.step_tol(ref)
        assert np.abs(got["R"] - ref["R"]).max() <= tol, (n, tol)
        assert np.abs(got["t"] - ref["t"]).max() <= tol * np.abs(ref["t"]).max(), (n, tol)


def test_host_program_copies_through(host_check, tmp_path):
    pw, uv, _, _ = C.noisy_scene(300, 31)
    R, t, _ = C.ransac_pose(300, 31)
    far = t + np.array([0.0, 0.0, 5000.0])
    bad = R.copy()
    bad[1, 1] = np.nan
    for args, status in (((pw[:5], uv[:5], C.K0, R, t), 1), ((pw, uv, C.K0, bad, t), 1), ((pw, uv, C.K0, R, far), 2)):
        got = run_host(host_check, tmp_path, *args)
        ref = LO.refine(*args)
        assert got["status"] == status == ref["status"]
        assert np.array_equal(got["R"].view(np.int64), np.asarray(args[3]).view(np.int64))
        assert np.array_equal(got["t"].view(np.int64), np.asarray(args[4]).view(np.int64))
        assert got["cost"] == 0 and got["inliers"] == ref["inliers"] and np.array_equal(got["trace"], ref["trace"])


def test_degenerate_geometry_on_the_reference_and_the_host_program(host_check, tmp_path):
    from tests import pnp_cases as PC
    (behind, Rb, tb) = C.behind_scene()
    cases = [(PC.identical(np.random.default_rng(7710), 50),) * 2, (PC.collinear(np.random.default_rng(7711), 50),) * 2]
    cases = [(sc, sc[2], sc[3]) for sc, _ in cases] + [(behind, Rb, tb)]
    for sc, R0, t0 in cases:
        ref = LO.refine(sc[0], sc[1], C.K0, R0, t0)
        got = run_host(host_check, tmp_path, sc[0], sc[1], C.K0, R0, t0)
        assert ref["status"] in (0, 2) and got["status"] == ref["status"]
        assert np.all(np.isfinite(got["R"])) and np.all(np.isfinite(got["t"])) and np.isfinite(got["cost"])
        m0, m1 = LO.truncated_cost(sc[0], sc[1], R0, t0, C.K0), LO.truncated_cost(sc[0], sc[1], got["R"], got["t"], C.K0)
        assert m1 <= m0 * (1 + len(sc[0]) * 2.0 ** -50)
        Z = LO.project(sc[0].astype(np.float64), sc[1].astype(np.float64), got["R"], got["t"], LO.kvec(C.K0))[2]
        assert got["inliers"] <= int((Z > 0).sum())
