"""Model info without a GPU: tests/modelinfo_ref.py against what the reference's calc_pts_diameter
returned (tests/golden/model_info.npz, tools/capture_modelinfo_fixtures.py), metric.add_scores /
auc_posecnn on CPU tensors against what test.py's own score tail made of the same errors, and
zp_model_info's host-side argument checks.

CLOUDS and score_cases build the inputs; the capture tool imports them, and the golden file stores
what they returned at capture time, which is what the tests read.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import modelinfo_ref as MR

SIZES = (1, 2, 3, 255, 256, 257, 1000, 2049)
FRACTIONS = (0.1, 0.05, 0.02)


def CLOUDS():
    out = {f"{kind}_{n}": MR.cloud(kind, n) for kind in ("uniform", "mixed") for n in SIZES}
    a = np.float32(37.5)
    out["cube8"] = np.array([[sx * a, sy * a, sz * a] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    out["same300"] = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (300, 1))
    return out


def score_cases():
    """name -> (errors mm f64 [N], success bool [N], diameter)."""
    rng = np.random.default_rng(465)
    d = 102.5
    rand = rng.gamma(2.0, 12.0, 300)
    rand[::17] = rng.uniform(100, 400, len(rand[::17]))
    mixed = rng.gamma(2.0, 8.0, 40)
    mixed[[3, 11, 30]] = np.nan
    ok = np.ones(40, bool)
    ok[[0, 11, 25]] = False
    cases = {
        "all_above": (np.array([100.5, 250.0, 1e4, 101.0]), None, d),          # nothing <= 0.1 m: NaN
        "one": (np.array([7.25]), None, d),
        "ties": (np.array([5.0, 5.0, 5.0, 12.0, 12.0, 0.0, 0.0, 40.0, 40.0, 99.0]), None, d),
        # exactly on d * 0.1, d * 0.05, d * 0.02, on 10, 20 .. 100 and on 0.1 m: strict <
        "thresholds": (np.array([d * 0.1, d * 0.05, d * 0.02, 10.0, 20.0, 30.0, 50.0, 100.0, 9.999999, 2.0499999, 2.05]),
                       None, d),
        "nan_failed": (mixed, ok, 64.0),
        "random": (rand, None, 87.3),
    }
    return {k: (np.asarray(e, np.float64), np.ones(len(e), bool) if s is None else s, float(dd))
            for k, (e, s, dd) in cases.items()}


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def G(golden):
    return golden("model_info.npz")


def test_inputs_are_the_recorded_ones(G):
    for name, pts in CLOUDS().items():
        assert np.array_equal(pts.view(np.int32), G[f"cloud_{name}"].view(np.int32)), name
    for name, (e, s, d) in score_cases().items():
        assert np.array_equal(bits(e), bits(G[f"score_{name}_errors"])) and np.array_equal(s, G[f"score_{name}_success"])
        assert d == float(G[f"score_{name}_diameter"])


@pytest.mark.parametrize("name", sorted(CLOUDS()))
def test_ref_reproduces_reference_diameter_bitwise(G, name):
    pts = G[f"cloud_{name}"]
    r = MR.model_info_ref(pts)
    assert bits(r["diameter"]) == bits(G[f"diameter_{name}"]), (name, r["diameter"], float(G[f"diameter_{name}"]))
    i, j = r["pair"]
    assert 0 <= i <= j < len(pts)
    p = pts.astype(np.float64)
    dx, dy, dz = p[i] - p[j]
    assert bits((dx * dx + dy * dy) + dz * dz) == bits(r["d2max"])
    assert np.array_equal(bits(r["min"]), bits(p.min(0))) and np.array_equal(bits(r["size"]), bits(np.ptp(p, axis=0)))


def test_ref_ties_and_degenerate_clouds(G):
    assert MR.model_info_ref(G["cloud_cube8"])["pair"] == (0, 7)
    r = MR.model_info_ref(G["cloud_same300"])
    assert r["diameter"] == 0.0 and r["pair"] == (0, 0)
    r = MR.model_info_ref(G["cloud_uniform_1"])
    assert r["diameter"] == 0.0 and r["pair"] == (0, 0) and np.all(r["size"] == 0.0)


def test_mixed_cloud_has_inexact_products(G):
    """On the recorded data: some dx dx of the mixed-magnitude cloud does not fit f64, so a fused
    multiply-add in d2 would round differently; the exact product is formed in Python integers."""
    assert MR.dx2_inexact(G["cloud_mixed_257"])
    x = G["cloud_mixed_257"][:, 0].astype(np.float64)
    found = False
    for i in range(0, 40):
        for j in range(i + 1, 40):
            dx = float(x[i] - x[j])
            m, e = math.frexp(dx)
            q = int(m * (1 << 53))
            assert math.ldexp(q, e - 53) == dx
            p = dx * dx
            pm, pe = math.frexp(p)
            # p == q^2 2^(2 (e - 53)) exactly?  Compare as integers at the finer of the two scales.
            lhs, ls = int(pm * (1 << 53)), pe - 53
            rhs, rs = q * q, 2 * (e - 53)
            s = min(ls, rs)
            found |= (lhs << (ls - s)) != (rhs << (rs - s))
    assert found


@pytest.mark.parametrize("name", sorted(score_cases()))
def test_scores_match_reference_on_cpu(G, name):
    import torch
    from zebrapose_amd import metric as M
    e, s, d = G[f"score_{name}_errors"], G[f"score_{name}_success"], float(G[f"score_{name}_diameter"])
    got = M.add_scores(torch.from_numpy(e), d, success=torch.from_numpy(s), fractions=FRACTIONS)
    assert set(got) == {"pass", "auc_steps", "auc_posecnn", "mean_error"}
    assert all(isinstance(v, float) for v in got["pass"] + [got["auc_steps"], got["auc_posecnn"], got["mean_error"]])
    assert got["pass"] == [float(v) for v in G[f"score_{name}_pass"]]
    assert got["auc_steps"] == float(G[f"score_{name}_auc_steps"])
    want = float(G[f"score_{name}_auc_posecnn"])
    if math.isnan(want):
        assert math.isnan(got["auc_posecnn"])
    else:
        assert abs(got["auc_posecnn"] - want) <= 1e-9 * max(1.0, abs(want))
    want = float(G[f"score_{name}_mean_error"])
    assert abs(got["mean_error"] - want) <= 1e-9 * max(1.0, abs(want))
    # the stand-alone function, on the errors as test.py:522 passes them
    clean = np.where(np.isnan(e) | ~s, 10000.0, e) / 1000.0
    a = M.auc_posecnn(clean)
    want = float(G[f"score_{name}_auc_posecnn"])
    assert (math.isnan(a) and math.isnan(want)) or abs(a - want) <= 1e-9 * max(1.0, abs(want))
    # and the numpy restatement agrees with the reference too
    ref = MR.add_scores_ref(e, d, s, FRACTIONS)
    assert ref["pass"] == got["pass"] and ref["auc_steps"] == got["auc_steps"]
    assert (math.isnan(ref["auc_posecnn"]) and math.isnan(want)) or abs(ref["auc_posecnn"] - want) <= 1e-9 * max(1.0, abs(want))


def test_score_cases_cover_the_edges(G):
    assert math.isnan(float(G["score_all_above_auc_posecnn"]))
    assert len(G["score_one_errors"]) == 1 and len(G["score_random_errors"]) >= 200
    e = G["score_ties_errors"]
    assert len(np.unique(e)) < len(e)
    e, d = G["score_thresholds_errors"], float(G["score_thresholds_diameter"])
    assert all(np.any(e == d * f) for f in FRACTIONS) and np.any(e == 10.0) and np.any(e == 100.0)
    assert np.isnan(G["score_nan_failed_errors"]).any() and not G["score_nan_failed_success"].all()


def test_add_scores_defaults_and_bad_input():
    from zebrapose_amd import metric as M
    got = M.add_scores([1.0, 7.0, float("nan")], 100.0)   # thresholds 10, 5, 2 mm; the NaN counts as 10000
    assert got["pass"] == [2 / 3, 1 / 3, 1 / 3] and got["auc_steps"] == float(np.mean(np.array([10, 10, 0]) / 10))
    with pytest.raises(ValueError):
        M.add_scores([], 100.0)
    with pytest.raises(ValueError):
        M.add_scores([1.0, 2.0], 100.0, success=[True])
    assert math.isnan(M.auc_posecnn([]))


def test_host_side_validation_without_gpu():
    """zp_model_info refuses bad arguments on the host before any launch (no GPU needed)."""
    from zebrapose_amd import _lib
    lib = _lib.lib
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    assert lib.zp_model_info_ws_bytes(0) == -1 and lib.zp_model_info_ws_bytes(-5) == -1
    assert lib.zp_model_info_ws_bytes((2 ** 31 - 1024) // 3 + 1) == -1
    small, big = lib.zp_model_info_ws_bytes(1), lib.zp_model_info_ws_bytes(700_000_000)
    assert 0 < small <= big <= 1 << 20          # a few thousand partials, whatever n is
    for args, word in (((p, 0, p, p, p, p, None), b"n 0"),
                       ((p, 4, None, p, p, p, None), b"NULL"),
                       ((p, 4, p, p, None, p, None), b"NULL"),
                       ((None, 4, p, p, p, p, None), b"NULL"),
                       ((p, 4, p, p, p, None, None), b"NULL"),
                       ((p, (2 ** 31 - 1024) // 3 + 1, p, p, p, p, None), b"outside")):
        assert lib.zp_model_info(*args) == 1
        assert word in lib.zp_last_error(), (args, lib.zp_last_error())
