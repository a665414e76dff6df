"""Host side of the BOP pose errors (no GPU): tests/bop_ref.py's visibility masks equal the
reference's lib/pysixd/visibility.py where that tree exists, symmetry_transformations follows
misc.get_symmetry_transformations' rule, zp_pose_error_sym / zp_vsd refuse bad arguments before any
device call, and bop_recall averages as BOP does."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from tests import bop_ref as BR
from tests.conftest import GOLDEN

# the reference tree as oracle/capture_fixtures.py finds it (absent on most machines: the test skips)
REF_VISIBILITY = os.path.join(os.environ.get("ZP_REFERENCE", "/root/reference/zebrapose"), "lib", "pysixd",
                              "visibility.py")

INFOS = {
    "none": {"diameter": 100.0},
    "disc2": {"symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1],
                                      [1, 0, 0, 2.5, 0, -1, 0, 0, 0, 0, -1, -4.0, 0, 0, 0, 1]]},
    "cont": {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [3.0, -2.0, 7.0]}]},
    "both": {"symmetries_discrete": [[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 10.0, 0, 0, 0, 1]],
             "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0.0, 0.0, 0.0]}]},
}


def test_visibility_masks_equal_the_reference():
    if not os.path.exists(REF_VISIBILITY):
        pytest.skip("no reference tree")
    spec = importlib.util.spec_from_file_location("ref_visibility", REF_VISIBILITY)
    V = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V)
    rng = np.random.default_rng(3)
    shape = (37, 53)
    scene = rng.uniform(400, 1200, shape)
    d_test = scene + rng.choice([-40.0, -15.0, -5.0, 5.0, 15.0, 40.0], shape) + rng.uniform(-1, 1, shape)
    d_test[rng.random(shape) < 0.2] = 0
    d_gt = np.where(rng.random(shape) < 0.6, scene, 0.0)
    d_est = np.where(rng.random(shape) < 0.6, scene + rng.choice([-20.0, 0.0, 3.0, 15.0], shape), 0.0)
    for delta in (15.0, 15, 0.0, 7.5):
        vg, ve = BR.vsd_masks(d_est, d_gt, d_test, delta)
        want_g = V.estimate_visib_mask_gt(d_test, d_gt, delta, visib_mode="bop19")
        want_e = V.estimate_visib_mask_est(d_test, d_est, want_g, delta, visib_mode="bop19")
        assert np.array_equal(vg, want_g) and np.array_equal(ve, want_e)
        assert vg.any() and ve.any() and not vg.all() and (ve & ~vg).any() and (vg & ~ve).any()


@pytest.mark.parametrize("name,count", [("none", 1), ("disc2", 3), ("cont", 314), ("both", 628)])
def test_symmetry_transformations(name, count):
    from zebrapose_amd.metric import symmetry_transformations
    info = INFOS[name]
    R, t = symmetry_transformations(info, 0.01)
    assert R.shape == (count, 3, 3) and t.shape == (count, 3) and R.dtype == np.float64 and t.dtype == np.float64
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    assert np.abs(np.linalg.det(R) - 1).max() < 1e-12
    assert np.array_equal(R[0], np.eye(3)) == (name in ("none", "disc2"))
    wR, wt = BR.symmetry_set(info, 0.01)
    assert np.abs(R - wR).max() < 1e-12 and np.abs(t - wt).max() < 1e-12
    if name == "disc2":
        for k, m in enumerate(info["symmetries_discrete"]):
            m = np.reshape(m, (4, 4)).astype(np.float64)
            assert np.array_equal(R[1 + k], m[:3, :3]) and np.array_equal(t[1 + k], m[:3, 3])
    if name == "cont":  # step i turns by 2 pi i / 315 about the axis through the offset, which stays fixed
        off = np.array(info["symmetries_continuous"][0]["offset"])
        assert np.abs(R @ off + t - off).max() < 1e-12
        a = 2 * np.pi * 5 / 315
        assert np.allclose(R[4], [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], atol=1e-14)
    if name == "both":  # discrete outermost: the first 314 are the continuous steps alone
        cR, ct = symmetry_transformations({"symmetries_continuous": info["symmetries_continuous"]}, 0.01)
        assert np.array_equal(R[:314], cR) and np.array_equal(t[:314], ct)
        m = np.reshape(info["symmetries_discrete"][0], (4, 4)).astype(np.float64)
        assert np.abs(R[314:] - cR @ m[:3, :3]).max() < 1e-15
        assert np.abs(t[314:] - (cR @ m[:3, 3] + ct)).max() < 1e-12
    # a coarser step: ceil(pi / 0.5) = 7 steps per turn -> 6 non-zero ones
    if name == "cont":
        assert symmetry_transformations(info, 0.5)[0].shape[0] == 6


def test_symmetry_transformations_match_the_reference_fixture():
    from zebrapose_amd.metric import symmetry_transformations
    path = os.path.join(GOLDEN, "bop_errors.npz")
    with np.load(path, allow_pickle=False) as z:
        f = {k: z[k] for k in z.files}
    for name, info in INFOS.items():
        R, t = symmetry_transformations(info, 0.01)
        assert R.shape == f[f"sym_{name}_R"].shape
        assert np.abs(R - f[f"sym_{name}_R"]).max() < 1e-12 and np.abs(t - f[f"sym_{name}_t"]).max() < 1e-12


def test_pose_error_sym_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    lib = _lib.lib
    assert lib.zp_pose_error_sym_ws_bytes(32, 20000, 314, 2) >= 32 * 314 * 8
    assert lib.zp_pose_error_sym_ws_bytes(1, 1, 1, 3) >= 8
    assert lib.zp_pose_error_sym_ws_bytes(5, 5000, 4096, 2) > 0
    for B, n, S, mode in [(0, 10, 1, 2), (-1, 10, 1, 2), (1, 0, 1, 2), (1, 10, 0, 2), (1, 10, 4097, 2), (1, 10, -1, 3),
                          (1, 10, 1, 0), (1, 10, 1, 4)]:
        assert lib.zp_pose_error_sym_ws_bytes(B, n, S, mode) == -1, (B, n, S, mode)
    buf = (ctypes.c_double * 64)()  # stands in for every pointer: the checks fail before any of them is used
    p = ctypes.addressof(buf)
    good = dict(B=2, pts=p, n=10, R_est=p, t_est=p, R_gt=p, t_gt=p, K=p, sym_R=p, sym_t=p, S=3, mode=2, out=p, ws=p,
                stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.zp_pose_error_sym(*[a[k] for k in good])

    cases = [(dict(S=0), b"S 0"), (dict(S=4097), b"S 4097"), (dict(S=-2), b"S -2"), (dict(B=0), b"B 0"),
             (dict(n=0), b"n 0"), (dict(n=-7), b"n -7"), (dict(mode=1), b"mode 1"), (dict(mode=4), b"mode 4"),
             (dict(mode=3, K=None), b"NULL K")]
    cases += [({k: None}, b"NULL") for k in ("pts", "R_est", "t_est", "R_gt", "t_gt", "sym_R", "sym_t", "out", "ws")]
    for bad, word in cases:
        assert call(**bad) == 1, bad
        assert word in lib.zp_last_error(), (bad, lib.zp_last_error())


def test_vsd_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    lib = _lib.lib
    assert lib.zp_vsd_ws_bytes(32, 480, 640, 10) > 0 and lib.zp_vsd_ws_bytes(1, 1, 1, 32) > 0
    for B, H, W, ntau in [(0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 4, 4, 33), (1, -4, 4, 1),
                          (1, 65536, 32768, 1), (65536, 4, 4, 1)]:
        assert lib.zp_vsd_ws_bytes(B, H, W, ntau) == -1, (B, H, W, ntau)
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    taus = (ctypes.c_double * 32)(*([0.1] * 32))
    good = dict(B=2, depth_est=p, depth_gt=p, depth_test=p, n_test=2, test_index=p, H=4, W=4, K=p, delta=15.0,
                taus=taus, ntau=10, diameter=p, out=p, counts=p, ws=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.zp_vsd(*[a[k] for k in good])

    cases = [(dict(ntau=0), b"ntau 0"), (dict(ntau=33), b"ntau 33"), (dict(H=0), b"0 x 4"), (dict(W=0), b"4 x 0"),
             (dict(W=-1), b"4 x -1"), (dict(B=0), b"B 0"), (dict(n_test=0), b"n_test 0"),
             (dict(n_test=1, test_index=None), b"n_test 1")]
    cases += [({k: None}, b"NULL") for k in ("depth_est", "depth_gt", "depth_test", "K", "taus", "out", "ws")]
    for bad, word in cases:
        assert call(**bad) == 1, bad
        assert word in lib.zp_last_error(), (bad, lib.zp_last_error())


def test_bop_recall_on_a_hand_made_vector():
    import torch
    from zebrapose_amd.metric import BOP19_TAUS, BOP19_THRESHOLDS, BOP19_VSD_DELTA, bop_recall
    errors = [0.01, 0.07, 0.12, 0.26, 0.9]
    # below 0.05: 1 of 5; below 0.1: 2; below 0.15 .. 0.25: 3; below 0.3 .. 0.5: 4
    want = (1 + 2 + 3 * 3 + 4 * 5) / (5 * 10)
    assert abs(bop_recall(errors, BOP19_THRESHOLDS) - want) < 1e-15
    assert abs(bop_recall(torch.tensor(errors, dtype=torch.float64), BOP19_THRESHOLDS) - want) < 1e-15
    assert bop_recall([0.3], [0.3]) == 0.0 and bop_recall([0.3], [0.31]) == 1.0  # strictly below
    # VSD: errors [N, ntau], every tau against every threshold
    e = np.array([[0.0, 1.0], [0.2, 0.4]])
    assert abs(bop_recall(e, [0.3, 0.5]) - (1 + 1 + 1 + 2) / 8) < 1e-15
    assert BOP19_VSD_DELTA == 15.0 and len(BOP19_TAUS) == 10 and len(BOP19_THRESHOLDS) == 10
    assert np.array_equal(BOP19_TAUS, np.arange(0.05, 0.51, 0.05))
