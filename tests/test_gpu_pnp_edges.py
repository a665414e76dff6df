"""The device RANSAC-EPnP (zp_pnp_ransac) at its edges, against oracle/pnp_ref.py (numpy f64):
the code that exists only on the device -- the block-parallel Jacobi, the null-space pick and the
four block-reduced passes of k_pnp_refine -- held to 1e-9 at the reduction boundaries; crops that
do not depend on their neighbours, their slot in the batch, the rows past counts[b] or HW; flat,
duplicated and degenerate geometry; the iteration-count edges.  The inputs come from
tests/pnp_cases.py; tests/test_pnp_cases_host.py checks their preconditions on the oracle alone.
"""
import warnings

import numpy as np
import pytest
import torch

from oracle import pnp_ref
from tests import pnp_cases as C
from tests.test_gpu_pnp import K, _scene
from tests.test_pnp_cases_host import ORACLE_TABLE

pytestmark = pytest.mark.gpu


def _run(scenes, HW, Ks=None, garbage_tail=False, **kw):
    from zebrapose_amd.pnp import PnP
    counts, xy, xyz = (torch.from_numpy(a).cuda() for a in C.batch(scenes, HW, garbage_tail))
    return [v.cpu() for v in PnP(**kw)(counts, xy, xyz, K if Ks is None else Ks)]


@pytest.mark.parametrize("per_crop_K", [False, True])
def test_final_epnp_is_exact_at_the_reduction_edges(gpu, per_crop_K):
    """(a) At a 1e4 px threshold every point is an inlier of the first valid hypothesis and the
    scan stops there, so the refine runs over all n points: n at and around one wave (64), one
    pass of the block (256) and two, and deep into the stride-256 loop.  The result is the
    oracle's EPnP of the same n points to the 1e-9 the serial host build is held to."""
    cases = C.exact_cases(per_crop_K)
    Ks = np.stack([k for _, k in cases]) if per_crop_K else None
    R, t, ok, inl = _run([s for s, _ in cases], C.EXACT_HW, Ks, reprojection_error=C.EXACT_THRESHOLD)
    R, t = R.numpy(), t.numpy()
    fails = []
    for b, ((pw, uv, _, _), Kb) in enumerate(cases):
        n = len(pw)
        Rr, tr = pnp_ref.epnp(pw, uv.astype(np.float32), Kb)
        dR, dt = np.abs(R[b] - Rr).max(), np.abs(t[b] - tr).max() / np.abs(tr).max()
        print(f"n={n}: ok {bool(ok[b])} inliers {int(inl[b])} max|dR| {dR:.2e} max|dt|/max|t| {dt:.2e}")
        if not (bool(ok[b]) and int(inl[b]) == n):
            fails.append((n, "inliers", int(inl[b])))
            continue
        try:
            np.testing.assert_allclose(R[b], Rr, rtol=0, atol=1e-9)
            np.testing.assert_allclose(t[b], tr, rtol=1e-9, atol=1e-9 * np.abs(tr).max())
        except AssertionError as e:
            fails.append((n, str(e)))
    assert not fails, fails


# (b) the realistic scenes of test_gpu_pnp: early stop, no stop, tiny sets, below the minimum, empty
_B_SIZES = [(3000, 0.3), (800, 0.5), (40, 0.1), (6, 0.0), (5, 0.0), (0, 0.0)]
_B_HW = 3000
_cache = {}


def _b_scenes():
    if "scenes" not in _cache:
        rng = np.random.default_rng(5)
        _cache["scenes"] = [_scene(rng, n, f) for n, f in _B_SIZES]
    return _cache["scenes"]


def _b_alone():
    """each crop on its own, B = 1: computed once, never modified"""
    if "alone" not in _cache:
        _cache["alone"] = [_run([s], _B_HW) for s in _b_scenes()]
    return _cache["alone"]


def _assert_slots_equal_alone(res, order):
    alone = _b_alone()
    for slot, k in enumerate(order):
        for name, a, r in zip(("R", "t", "ok", "inl"), alone[k], res):
            assert torch.equal(a[0], r[slot]), (name, slot, k)


def test_crop_is_independent_of_batch_and_slot(gpu):
    """B = 65 and B = 130 put the 64-thread block edge of k_pnp_subsets / k_pnp_select inside the
    batch; every slot returns, bit for bit, what its crop returns alone -- in either order"""
    scenes = _b_scenes()
    assert bool(_b_alone()[0][2][0]) and bool(_b_alone()[1][2][0]) and not bool(_b_alone()[5][2][0])
    order = [i % len(scenes) for i in range(65)]
    _assert_slots_equal_alone(_run([scenes[k] for k in order], _B_HW), order)
    order = [i % len(scenes) for i in range(130)][::-1]
    _assert_slots_equal_alone(_run([scenes[k] for k in order], _B_HW), order)


def test_rows_past_counts_and_HW_do_not_matter(gpu):
    """NaN / INT32_MIN / INT32_MAX instead of zeros past counts[b], HW 4097 instead of 3000, and
    the same call again: all bit for bit the crops' own results"""
    scenes = _b_scenes()
    order = [i % len(scenes) for i in range(65)]
    batch = [scenes[k] for k in order]
    _assert_slots_equal_alone(_run(batch, _B_HW, garbage_tail=True), order)
    wide = _run(batch, 4097)
    _assert_slots_equal_alone(wide, order)
    for a, b in zip(wide, _run(batch, 4097)):
        assert torch.equal(a, b)


def _invariants(name, n, R, t, ok, inl):
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(t)), name
    assert 0 <= inl <= n, (name, inl)
    if ok:
        assert np.abs(R.T @ R - np.eye(3)).sum(1).max() <= 1e-9, name
        assert abs(np.linalg.det(R) - 1) <= 1e-9 and inl >= 5, (name, inl)
    else:
        assert not R.any() and not t.any() and inl == 0, name


def _agrees_with_oracle(name, n, R, t, ok, inl, ref):
    assert ok, name
    assert abs(inl - ref["inliers"]) <= max(2, 0.02 * n), (name, inl, ref["inliers"])
    dang = C.rot_angle_deg(R, ref["R"])
    assert dang < 0.1, (name, dang)
    assert np.linalg.norm(t - ref["t"]) < 1e-2 * np.linalg.norm(ref["t"]), (name, t, ref["t"])


def test_degenerate_geometry(gpu):
    """(c) thin, exactly planar (the pseudo-inverse branch of epnp_control), heavily duplicated,
    tiny-and-far and off-image objects, one repeated 3D point, collinear points: finite outputs, a
    proper rotation or an all-zero failure; the oracle's pose where the oracle solves the case,
    the true pose where its final EPnP is well conditioned too (ORACLE_TABLE)."""
    cases = C.degenerate_cases()
    R, t, ok, inl = (v.numpy() for v in _run(list(cases.values()), 2000))
    for b, (name, (pw, uv, Rt, tt)) in enumerate(cases.items()):
        n = len(pw)
        print(f"{name}: ok {bool(ok[b])} inliers {int(inl[b])} of {n}")
        _invariants(name, n, R[b], t[b], bool(ok[b]), int(inl[b]))
        if not ORACLE_TABLE[name]["solved"]:
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ref = pnp_ref.solve_pnp_ransac(pw, uv.astype(np.float32), K)
        _agrees_with_oracle(name, n, R[b], t[b], bool(ok[b]), int(inl[b]), ref)
        if ORACLE_TABLE[name]["well_posed"]:
            ang = C.rot_angle_deg(R[b], Rt)
            assert ang < 0.5 and np.linalg.norm(t[b] - tt) < 0.01 * np.linalg.norm(tt), (name, ang, t[b], tt)


def test_coarse_lut_with_spread_pixels_keeps_the_invariants(gpu):
    """64 distinct 3D points shared by 4000 pixels spread over each point's footprint, plain and
    with 30 % outliers: whatever RANSAC makes of one point seen at many pixels, the outputs are
    finite and a reported pose is a rotation.  No pose is compared: this data fixes it only to
    degrees (pnp_cases.coarse_lut)."""
    rng = np.random.default_rng(31)
    scenes = [C.coarse_lut_spread(rng), C.add_outliers(rng, C.coarse_lut_spread(rng), 0.3)]
    R, t, ok, inl = (v.numpy() for v in _run(scenes, 4000))
    for b in range(2):
        print(f"spread coarse LUT {b}: ok {bool(ok[b])} inliers {int(inl[b])} of 4000")
        _invariants(b, 4000, R[b], t[b], bool(ok[b]), int(inl[b]))


@pytest.mark.parametrize("iterations", [1, 32, 33, 1000])
def test_iteration_count_edges(gpu, monkeypatch, iterations):
    """(d) one hypothesis, the last of the first chunk, the first of the second, and far more than
    the scan needs: the oracle's result at the same count; at 1000 also the one-chunk schedule's,
    bit for bit"""
    pw, uv, _, _ = scene = C.iteration_scene()
    res = _run([scene], 800, iterations=iterations)
    R, t, ok, inl = (v.numpy()[0] for v in res)
    _invariants(iterations, 800, R, t, bool(ok), int(inl))
    ref = pnp_ref.solve_pnp_ransac(pw, uv.astype(np.float32), K, iterations=iterations)
    print(f"iterations={iterations}: device ok {bool(ok)} inliers {int(inl)}; oracle {ref['success']} {ref.get('inliers')}")
    # at 1 iteration the oracle finds no model (test_pnp_cases_host pins it): a device that ran
    # more hypotheses than asked would find the consensus and fail here
    assert bool(ok) == bool(ref["success"]), iterations
    if ref["success"]:
        _agrees_with_oracle(iterations, 800, R, t, bool(ok), int(inl), ref)
    if iterations == 1000:
        monkeypatch.setenv("ZP_PNP_FIRST", "0")
        for a, b in zip(res, _run([scene], 800, iterations=iterations)):
            assert torch.equal(a, b)
