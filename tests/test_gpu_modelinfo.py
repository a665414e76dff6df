"""zp_model_info through zebrapose_amd.modelinfo against its numpy restatement (tests/modelinfo_ref.py)
and, where the golden file has the cloud, against what the reference's calc_pts_diameter returned:
the diameter, d2max and the six box values are compared as bits, the pair exactly.

The kernel's tile is 256 x 256, so the sizes are 1, 2, 3 (a few threads), 255 / 256 / 257 (T - 1, T,
T + 1), 1000 and 2049 (several tiles, a partial last one).  Its grid is 1024 workgroups; 2049 points
are 45 tiles, so one more size, 11265 points = 1035 tiles, makes some workgroups walk a second tile.
"""
import functools
import json
import math

import numpy as np
import pytest
import torch

from tests import meshcode_ref as MESH
from tests import modelinfo_ref as MR
from tests.test_modelinfo_host import FRACTIONS, SIZES, bits

pytestmark = pytest.mark.gpu

KEYS = ("diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z")


@functools.lru_cache(maxsize=None)
def ref_of(kind, n):
    pts = MR.cloud(kind, n)
    return pts, MR.model_info_ref(pts)  # computed once; the tests leave both unchanged


def run(pts, dev):
    """-> (model_info dict, d2max, pair) from one call of the C entry point's wrapper."""
    from zebrapose_amd import modelinfo as MI
    out, pair = MI._run(pts, dev)
    info = MI.model_info(pts, device=dev)
    d, pair2 = MI.model_diameter(pts, return_pair=True, device=dev)
    assert pair2 == pair and bits(d) == bits(info["diameter"]) == bits(math.sqrt(out[7]))
    return info, out[7], pair


def assert_matches(info, d2max, pair, ref, what):
    assert list(info) == list(KEYS) and all(type(v) is float for v in info.values()), what
    assert bits(d2max) == bits(ref["d2max"]), (what, d2max, ref["d2max"])
    assert bits(info["diameter"]) == bits(ref["diameter"]), (what, info["diameter"], ref["diameter"])
    assert pair == ref["pair"], (what, pair, ref["pair"])
    for a, ax in enumerate("xyz"):
        assert bits(info[f"min_{ax}"]) == bits(ref["min"][a]) and bits(info[f"size_{ax}"]) == bits(ref["size"][a]), (what, ax)


@pytest.mark.parametrize("kind", ("uniform", "mixed"))
@pytest.mark.parametrize("n", SIZES)
def test_sizes_bitwise(gpu, golden, n, kind):
    pts, ref = ref_of(kind, n)
    G = golden("model_info.npz")
    assert np.array_equal(pts, G[f"cloud_{kind}_{n}"])
    info, d2max, pair = run(pts, gpu)
    assert_matches(info, d2max, pair, ref, f"{kind} {n}")
    assert bits(info["diameter"]) == bits(G[f"diameter_{kind}_{n}"])


def test_more_tiles_than_the_grid(gpu):
    pts, ref = ref_of("uniform", 11265)
    assert_matches(*run(pts, gpu), ref, "uniform 11265")


@pytest.mark.parametrize("where", ((10, 200), (300, 400), (100, 400), (0, 599), (598, 599)),
                         ids=("diagonal0", "diagonal1", "offdiagonal", "first_last", "partial_tile"))
def test_placement_of_the_maximum(gpu, where):
    pts = np.random.default_rng(600).uniform(-10, 10, (600, 3)).astype(np.float32)
    pts[where[0]] = (-900.5, 3.25, 1.0)
    pts[where[1]] = (870.25, -2.5, 0.5)
    info, d2max, pair = run(pts, gpu)
    assert pair == where
    assert_matches(info, d2max, pair, MR.model_info_ref(pts), str(where))


def test_cube_corners_tie(gpu, golden):
    pts = golden("model_info.npz")["cloud_cube8"]
    info, d2max, pair = run(pts, gpu)
    assert pair == (0, 7)
    assert_matches(info, d2max, pair, MR.model_info_ref(pts), "cube")
    assert bits(info["diameter"]) == bits(golden("model_info.npz")["diameter_cube8"])


def test_duplicated_extremes_lowest_pair_wins(gpu):
    pts = np.random.default_rng(7).uniform(-10, 10, (700, 3)).astype(np.float32)
    pts[5] = pts[300] = pts[620] = (-500.0, 1.0, 2.0)
    pts[9] = pts[450] = pts[699] = (400.0, -3.0, 0.25)
    info, d2max, pair = run(pts, gpu)
    assert pair == (5, 9)
    assert_matches(info, d2max, pair, MR.model_info_ref(pts), "duplicates")


def test_identical_points(gpu, golden):
    pts = golden("model_info.npz")["cloud_same300"]
    info, d2max, pair = run(pts, gpu)
    assert info["diameter"] == 0.0 and d2max == 0.0 and pair == (0, 0)
    assert info["size_x"] == info["size_y"] == info["size_z"] == 0.0 and info["min_y"] == -2.25
    one, _, pair = run(pts[:1], gpu)
    assert one["diameter"] == 0.0 and pair == (0, 0)


def test_reproducible_and_order_independent(gpu):
    pts, ref = ref_of("mixed", 1000)
    a, b = run(pts, gpu), run(pts, gpu)
    assert a == b
    perm = np.random.default_rng(3).permutation(len(pts))
    info, d2max, pair = run(np.ascontiguousarray(pts[perm]), gpu)
    assert bits(info["diameter"]) == bits(a[0]["diameter"]) and bits(d2max) == bits(a[1])
    assert info == a[0]
    p = pts.astype(np.float64)
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if int((np.triu(d2) == ref["d2max"]).sum()) == 1:  # the maximum is unique: the pair maps back
        assert tuple(sorted((int(perm[pair[0]]), int(perm[pair[1]])))) == ref["pair"]


def test_rejections_and_conversions(gpu):
    from zebrapose_amd import modelinfo as MI
    pts, ref = ref_of("uniform", 257)
    for bad in (np.nan, np.inf, -np.inf):
        p = pts.copy()
        p[200, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            MI.model_diameter(p, device=gpu)
        with pytest.raises(ValueError, match="finite"):
            MI.model_info(torch.from_numpy(p).to(gpu))
    p64 = pts.astype(np.float64)
    assert bits(MI.model_diameter(p64, device=gpu)) == bits(ref["diameter"])
    assert bits(MI.calc_pts_diameter(p64)) == bits(ref["diameter"])
    assert bits(MI.model_diameter(torch.from_numpy(p64).to(gpu))) == bits(ref["diameter"])
    p64[3, 0] += 1e-9
    with pytest.raises(ValueError, match="f32"):
        MI.model_diameter(p64, device=gpu)
    with pytest.raises(ValueError, match="f32"):
        MI.model_diameter(torch.from_numpy(p64).to(gpu))
    for shape in ((0, 3), (5, 2), (6,), (2, 3, 3)):
        with pytest.raises(ValueError):
            MI.model_info(np.zeros(shape, np.float32), device=gpu)
    d, pair = MI.model_diameter(torch.from_numpy(pts).to(gpu), return_pair=True)
    assert bits(d) == bits(ref["diameter"]) and pair == ref["pair"]


def test_meshcode_model_info_feeds_symmetries_and_json(gpu, tmp_path):
    from zebrapose_amd import metric as M
    from zebrapose_amd.meshcode import encode_mesh
    from zebrapose_amd.modelinfo import save_models_info
    v, f = MESH.icosphere(2)
    v = v * np.float32(40)
    mc = encode_mesh(v, f, bits=5, device=gpu)
    plain = mc.model_info()
    assert list(plain) == list(KEYS)
    ref = MR.model_info_ref(v)
    assert bits(plain["diameter"]) == bits(ref["diameter"]) and bits(plain["min_z"]) == bits(ref["min"][2])
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])
    info = mc.model_info(symmetries_discrete=[flip.ravel().tolist()])
    assert {k: info[k] for k in KEYS} == plain
    R, t = M.symmetry_transformations(info)
    assert R.shape == (2, 3, 3) and np.array_equal(R[1], flip[:3, :3]) and not t.any()
    path = tmp_path / "models_info.json"
    save_models_info(path, {7: info})
    back = json.load(open(path))
    assert list(back) == ["7"] and back["7"] == info
    assert all(bits(back["7"][k]) == bits(info[k]) for k in KEYS)


@pytest.mark.parametrize("name", ("all_above", "thresholds", "nan_failed", "random"))
def test_add_scores_on_a_device_tensor_equals_cpu(gpu, golden, name):
    from zebrapose_amd import metric as M
    G = golden("model_info.npz")
    e, s, d = G[f"score_{name}_errors"], G[f"score_{name}_success"], float(G[f"score_{name}_diameter"])
    cpu = M.add_scores(torch.from_numpy(e), d, success=torch.from_numpy(s), fractions=FRACTIONS)
    dev = M.add_scores(torch.from_numpy(e).to(gpu), d, success=torch.from_numpy(s).to(gpu), fractions=FRACTIONS)
    assert dev["pass"] == cpu["pass"] and dev["auc_steps"] == cpu["auc_steps"]
    for k in ("auc_posecnn", "mean_error"):
        assert (math.isnan(dev[k]) and math.isnan(cpu[k])) or abs(dev[k] - cpu[k]) <= 1e-9 * max(1.0, abs(cpu[k])), k
    assert dev["pass"] == [float(v) for v in G[f"score_{name}_pass"]]
    assert dev["auc_steps"] == float(G[f"score_{name}_auc_steps"])
