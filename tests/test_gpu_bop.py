"""BOP pose errors on the device (zp_pose_error_sym, zp_vsd; zebrapose_amd/metric.py) against the
numpy restatement tests/bop_ref.py and against what the reference's own pose_error.mssd / mspd / vsd
returned (tests/golden/bop_errors.npz, tools/capture_bop_fixtures.py).

MSSD / MSPD tolerance: 1e-9 max(1, want), the one test_gpu_metric.py uses for the same f64 transforms.
VSD: counts equal and errors bitwise equal; the inputs carry margins (bop_ref.vsd_scene), asserted on
the reference-side arrays, so a 1-ulp difference in a square root cannot flip a count."""
import numpy as np
import pytest

from tests import bop_ref as BR
from tests.test_bop_host import INFOS

pytestmark = pytest.mark.gpu


def _poses(rng, B):
    Rg = np.stack([BR.rot(rng) for _ in range(B)])
    tg = rng.uniform(-50, 50, (B, 3)) + np.array([0, 0, 800.0])
    Re = np.stack([r @ BR.rot(np.random.default_rng(k)) if k % 2 else r for k, r in enumerate(Rg)])
    te = tg + rng.normal(0, 5, (B, 3))
    K4 = np.stack([rng.uniform(550, 650, B), rng.uniform(550, 650, B), rng.uniform(300, 340, B),
                   rng.uniform(220, 260, B)], 1)
    return Re, te, Rg, tg, K4


def _syms(rng, S):
    """S transformations: the identity first, then random rigid ones (the kernel does not need a group)."""
    R = np.stack([np.eye(3)] + [BR.rot(rng) for _ in range(S - 1)])
    t = np.concatenate([np.zeros((1, 3)), rng.uniform(-5, 5, (S - 1, 3))])
    return R, t


def _check_sym(pts, Re, te, Rg, tg, K4, sR, st):
    from zebrapose_amd.metric import MSPD, MSSD, pose_errors_sym
    got_s = pose_errors_sym(pts, Re, te, Rg, tg, (sR, st), MSSD).cpu().numpy()
    got_p = pose_errors_sym(pts, Re, te, Rg, tg, (sR, st), MSPD, K=K4).cpu().numpy()
    for b in range(len(Re)):
        want_s = BR.mssd(pts, Re[b], te[b], Rg[b], tg[b], sR, st)
        want_p = BR.mspd(pts, Re[b], te[b], Rg[b], tg[b], K4[b], sR, st)
        assert abs(got_s[b] - want_s) <= 1e-9 * max(1.0, want_s), (b, got_s[b], want_s)
        assert abs(got_p[b] - want_p) <= 1e-9 * max(1.0, want_p), (b, got_p[b], want_p)
    return got_s, got_p


@pytest.mark.parametrize("S", [1, 3, 70])
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_mssd_mspd_match_bop_ref(gpu, n, S):
    rng = np.random.default_rng(1000 * S + n)
    pts = rng.uniform(-60, 60, (n, 3)).astype(np.float32)
    Re, te, Rg, tg, K4 = _poses(rng, 5)
    sR, st = _syms(rng, S)
    _check_sym(pts, Re, te, Rg, tg, K4, sR, st)


def test_mssd_mspd_full_symmetry_set_and_dict_form(gpu):
    """n = 300, S = 628 (discrete x continuous), B = 2; the reference's list-of-dicts form gives the same bits."""
    from zebrapose_amd.metric import MSSD, pose_errors_sym, symmetry_transformations
    rng = np.random.default_rng(628)
    pts = rng.uniform(-60, 60, (300, 3)).astype(np.float32)
    Re, te, Rg, tg, K4 = _poses(rng, 2)
    sR, st = symmetry_transformations(INFOS["both"], 0.01)
    assert len(sR) == 628
    got_s, _ = _check_sym(pts, Re, te, Rg, tg, K4, sR, st)
    dicts = [{"R": R, "t": t.reshape(3, 1)} for R, t in zip(sR, st)]
    again = pose_errors_sym(pts, Re, te, Rg, tg, dicts, MSSD).cpu().numpy()
    assert np.array_equal(got_s.view(np.int64), again.view(np.int64))


def test_min_over_symmetries_is_taken(gpu):
    """est = gt o sym_k (k > 0) shifted by 0.1 mm: the small value with the set, the large one with the
    identity alone; and the host wrappers agree with the batched call."""
    from zebrapose_amd.metric import MSPD, MSSD, mspd, mssd, pose_errors_sym, symmetry_transformations
    rng = np.random.default_rng(7)
    pts = rng.uniform(-60, 60, (1000, 3)).astype(np.float32)
    _, _, Rg, tg, K4 = _poses(rng, 3)
    sR, st = symmetry_transformations(INFOS["cont"], 0.01)
    ks = [5, 157, 313]
    Re = np.stack([Rg[b] @ sR[k] for b, k in enumerate(ks)])
    te = np.stack([Rg[b] @ st[k] + tg[b] + np.array([0.1, 0, 0]) for b, k in enumerate(ks)])
    small = pose_errors_sym(pts, Re, te, Rg, tg, (sR, st), MSSD).cpu().numpy()
    large = pose_errors_sym(pts, Re, te, Rg, tg, (np.eye(3)[None], np.zeros((1, 3))), MSSD).cpu().numpy()
    assert np.all(np.abs(small - 0.1) < 1e-9), small
    assert large[1] > 100 and np.all(large > 1.0), large
    small_p = pose_errors_sym(pts, Re, te, Rg, tg, (sR, st), MSPD, K=K4).cpu().numpy()
    large_p = pose_errors_sym(pts, Re, te, Rg, tg, (np.eye(3)[None], np.zeros((1, 3))), MSPD, K=K4).cpu().numpy()
    assert np.all(small_p < 0.2) and np.all(large_p > 5 * small_p), (small_p, large_p)
    K = np.array([[K4[1, 0], 0, K4[1, 2]], [0, K4[1, 1], K4[1, 3]], [0, 0, 1.0]])
    dicts = [{"R": R, "t": t.reshape(3, 1)} for R, t in zip(sR, st)]
    assert mssd(Re[1], te[1].reshape(3, 1), Rg[1], tg[1].reshape(3, 1), pts, dicts) == small[1]
    assert mspd(Re[1], te[1].reshape(3, 1), Rg[1], tg[1].reshape(3, 1), K, pts, dicts) == small_p[1]


def test_mssd_bounds_add_and_is_bitwise_reproducible(gpu):
    from zebrapose_amd.metric import ADD, MSPD, MSSD, pose_errors, pose_errors_sym
    rng = np.random.default_rng(11)
    pts = rng.uniform(-60, 60, (5000, 3)).astype(np.float32)
    Re, te, Rg, tg, K4 = _poses(rng, 5)
    ident = (np.eye(3)[None], np.zeros((1, 3)))
    add = pose_errors(pts, Re, te, Rg, tg, ADD).cpu().numpy()
    m1 = pose_errors_sym(pts, Re, te, Rg, tg, ident, MSSD).cpu().numpy()
    assert np.all(m1 >= add) and np.all(m1 > 0)
    sR, st = _syms(rng, 70)
    for mode in (MSSD, MSPD):
        a = pose_errors_sym(pts, Re, te, Rg, tg, (sR, st), mode, K=K4).cpu().numpy()
        b = pose_errors_sym(pts, Re, te, Rg, tg, (sR, st), mode, K=K4).cpu().numpy()
        assert np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- VSD pixel stage --------------------------------------------------------------------------------

TAUS = {1: (np.array([0.2]), np.array([20.0])), 10: (np.arange(0.05, 0.51, 0.05), np.arange(0.05, 0.51, 0.05) * 100.0)}
_SCENES = {}


def _scene(H, W):
    """Inputs and their bop_ref results, computed once per shape: B = 4, poses 1 and 2 share test image 1."""
    if (H, W) not in _SCENES:
        rng = np.random.default_rng(100 * H + W)
        ti = np.array([0, 1, 1, 2])
        est, gt, test, K, diam = BR.vsd_scene(rng, 4, H, W, ti)
        want = {}
        for ntau in (1, 10):
            for norm in (True, False):
                taus = TAUS[ntau][0 if norm else 1]
                for b in range(4):
                    _, _, parts = BR.vsd_pixels(est[b], gt[b], test[ti[b]], K[b], 15.0, taus, diam[b] if norm else None,
                                                return_parts=True)
                    assert BR.margins_ok(parts, 15.0, taus), (H, W, ntau, norm, b)
                want[ntau, norm] = BR.vsd_batch(est, gt, test, K, 15.0, taus, diam if norm else None, ti)
        _SCENES[H, W] = (est, gt, test, K, diam, ti, want)
    return _SCENES[H, W]


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("ntau", [1, 10])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 13), (48, 64), (120, 160)])
def test_vsd_pixel_stage_matches_bop_ref_exactly(gpu, H, W, ntau, norm):
    from zebrapose_amd.metric import vsd_from_depth
    est, gt, test, K, diam, ti, want = _scene(H, W)
    taus = TAUS[ntau][0 if norm else 1]
    out, counts = vsd_from_depth(est, gt, test, K, 15.0, taus, norm, diam if norm else None, test_index=ti,
                                 return_counts=True)
    wc, we = want[ntau, norm]
    assert out.shape == (4, ntau) and counts.shape == (4, 2 + ntau)
    assert np.array_equal(counts.cpu().numpy(), wc), (counts.cpu().numpy(), wc)
    assert np.array_equal(out.cpu().numpy().view(np.int64), we.view(np.int64))
    if H * W > 1000:  # every kind of pixel occurs
        assert np.all(wc[:, 0] > wc[:, 1]) and np.all(wc[:, 1] > wc[:, 2]) and np.all(wc[:, 2] > 0)


def test_vsd_more_than_sixteen_taus_and_no_index(gpu):
    """17 .. 32 taus take the wider kernel; without test_index pose b reads test image b."""
    from zebrapose_amd.metric import vsd_from_depth
    rng = np.random.default_rng(32)
    est, gt, test, K, diam = BR.vsd_scene(rng, 3, 31, 45)
    taus = np.linspace(1.0, 63.0, 32)
    for b in range(3):
        _, _, parts = BR.vsd_pixels(est[b], gt[b], test[b], K[b], 15.0, taus, None, return_parts=True)
        assert BR.margins_ok(parts, 15.0, taus)
    wc, we = BR.vsd_batch(est, gt, test, K, 15.0, taus)
    out, counts = vsd_from_depth(est, gt, test, K, 15.0, taus, False, return_counts=True)
    assert np.array_equal(counts.cpu().numpy(), wc)
    assert np.array_equal(out.cpu().numpy().view(np.int64), we.view(np.int64))


def _one_pixel(est, gt, test, delta, taus, diameter=None):
    from zebrapose_amd.metric import vsd_from_depth
    a = [np.full((1, 1, 1), v, np.float32) for v in (est, gt, test)]
    out, counts = vsd_from_depth(a[0], a[1], a[2], [1.0, 1.0, 0.0, 0.0], delta, taus, diameter is not None, diameter,
                                 return_counts=True)
    return out.cpu().numpy()[0].tolist(), counts.cpu().numpy()[0].tolist()


def test_vsd_exact_boundaries(gpu):
    """H = W = 1 and cx = cy = 0: dist = depth exactly, so every comparison can be put on its boundary."""
    up = float(np.nextafter(np.float32(485.0), np.float32(0)))  # just in front of gt - delta
    # diff == delta counts as visible; a hair more does not (the pixel then leaves both masks)
    assert _one_pixel(500, 500, 485, 15.0, [20.0]) == ([0.0], [1, 1, 0])
    assert _one_pixel(500, 500, up, 15.0, [20.0]) == ([1.0], [0, 0, 0])
    # dists == tau counts as a cost; the next tau up does not
    assert _one_pixel(520, 500, 500, 15.0, [20.0, float(np.nextafter(20.0, 21.0))]) == ([1.0, 0.0], [1, 1, 1, 0])
    assert _one_pixel(520, 500, 500, 15.0, [0.25], diameter=80.0) == ([1.0], [1, 1, 1])
    # union == 0 gives 1.0 at every tau
    assert _one_pixel(0, 0, 500, 15.0, [1.0, 2.0, 3.0]) == ([1.0, 1.0, 1.0], [0, 0, 0, 0, 0])
    # depth_test == 0 is visible, however far the model is
    assert _one_pixel(900, 900, 0, 15.0, [20.0]) == ([0.0], [1, 1, 0])
    # est 100 behind the scene is not visible by itself; visib_gt makes it so
    assert _one_pixel(600, 500, 500, 15.0, [20.0]) == ([1.0], [1, 1, 1])
    assert _one_pixel(600, 0, 500, 15.0, [20.0]) == ([1.0], [0, 0, 0])
    # only gt visible: in the union, not in the intersection
    assert _one_pixel(0, 500, 500, 15.0, [20.0]) == ([1.0], [1, 0, 0])


# ---- end to end with the renderer ----------------------------------------------------------------------

def test_vsd_end_to_end_with_mesh_renderer(gpu):
    from zebrapose_amd.metric import BOP19_TAUS, BOP19_VSD_DELTA, vsd, vsd_errors
    from zebrapose_amd.render import MeshRenderer
    v, f = BR.icosphere(3)
    assert len(v) == 642
    v = v * np.float32(50.0)
    diameter = 100.0
    r = MeshRenderer(v, f, device=gpu)
    H, W = 96, 128
    K = np.array([[150.0, 0, 64.0], [0, 150.0, 48.0], [0, 0, 1.0]])
    Rg, tg = BR.rot(np.random.default_rng(1)), np.array([5.0, -3.0, 400.0])
    depth_gt = r.render(Rg[None], tg[None], K, H, W, outputs=("depth",))["depth"]
    dg = depth_gt.cpu().numpy()[0]
    assert 800 < (dg > 0).sum() < H * W // 2
    # est = gt on the rendered gt depth: 0 everywhere; two diameters to the side: 1 everywhere; 2 mm back: 0 again
    Re = np.stack([Rg, Rg, Rg])
    te = np.stack([tg, tg + np.array([2 * diameter, 0, 0]), tg + np.array([0, 0, 2.0])])
    out, counts = vsd_errors(r, Re, te, np.stack([Rg] * 3), np.stack([tg] * 3), depth_gt, K, BOP19_VSD_DELTA, BOP19_TAUS,
                             True, diameter, return_counts=True)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert np.all(out[0] == 0.0) and counts[0, 0] == counts[0, 1] == (dg > 0).sum()
    assert np.all(out[1] == 1.0) and counts[1, 1] == 0 and counts[1, 0] > counts[0, 0]
    assert np.all(out[2] < 0.3) and out[2, -1] < 0.05  # only rim pixels differ by more than 5 mm
    # an occluder plane in front of the left half halves the union
    occ = dg.copy()
    occ[:, : W // 2 + 3] = 200.0
    out_o, counts_o = vsd_errors(r, Rg[None], tg[None], Rg[None], tg[None], occ, K, BOP19_VSD_DELTA, BOP19_TAUS, True,
                                 diameter, return_counts=True)
    k4 = [150.0, 150.0, 64.0, 48.0]
    wc, we = BR.vsd_pixels(dg, dg, occ, k4, BOP19_VSD_DELTA, BOP19_TAUS, diameter)
    assert np.array_equal(counts_o.cpu().numpy()[0], wc) and np.array_equal(out_o.cpu().numpy()[0], we)
    assert 0.4 * counts[0, 0] < wc[0] < 0.6 * counts[0, 0]
    # the reference-signature wrapper agrees with the batched call
    one = vsd(Re[2], te[2].reshape(3, 1), Rg, tg.reshape(3, 1), dg, K, BOP19_VSD_DELTA, list(BOP19_TAUS), True, diameter, r,
              1)
    assert isinstance(one, list) and one == out[2].tolist()


# ---- what the reference's own functions returned -----------------------------------------------------------

def test_bop_errors_match_the_reference_fixture(gpu, golden):
    from zebrapose_amd.metric import MSPD, MSSD, pose_errors_sym, vsd_from_depth
    f = golden("bop_errors.npz")
    for name in INFOS:
        syms = (f[f"sym_{name}_R"], f[f"sym_{name}_t"])
        args = (f["pts"], f["R_est"], f["t_est"], f["R_gt"], f["t_gt"], syms)
        np.testing.assert_allclose(pose_errors_sym(*args, MSSD).cpu().numpy(), f[f"mssd_{name}"], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(pose_errors_sym(*args, MSPD, K=f["K"]).cpu().numpy(), f[f"mspd_{name}"], rtol=1e-9,
                                   atol=1e-11)
    # atol: coordinates of ~1e3 carry ~1e-12 of f64 rounding, which is all that is left where the error is 0
    assert f["mssd_disc2"][2] < 0.2 < 100 < f["mssd_none"][2]  # the fixture itself needs the min over s
    ti = f["vsd_test_index"]
    for taus, norm, want in ((f["vsd_taus_norm"], True, f["vsd_norm"]), (f["vsd_taus_mm"], False, f["vsd_mm"])):
        for b in range(len(ti)):  # the same margins as above, on the stored inputs
            _, _, parts = BR.vsd_pixels(f["vsd_est"][b], f["vsd_gt"][b], f["vsd_test"][ti[b]], f["vsd_K"][b],
                                        float(f["vsd_delta"]), taus, f["vsd_diameter"][b] if norm else None,
                                        return_parts=True)
            assert BR.margins_ok(parts, float(f["vsd_delta"]), taus)
        out = vsd_from_depth(f["vsd_est"], f["vsd_gt"], f["vsd_test"], f["vsd_K"], float(f["vsd_delta"]), taus, norm,
                             f["vsd_diameter"] if norm else None, test_index=ti)
        assert np.array_equal(out.cpu().numpy(), want)
    assert np.all(f["vsd_norm"][4] == 1.0) and np.all(f["vsd_norm"][5] == 0.0) and 0 < f["vsd_norm"][0, 0] < 1
