"""Host side of the training augmentation (zebrapose_amd/augment.py, crop.aug_Bbox): the
sampler's distributions against the probabilities and ranges of
GDR_Net_Augmentation.build_augmentations (:161-178), the LUT and stencil builders against their
formulas, aug_Bbox against bop_dataset_pytorch.py:141-160 for injected draws.  No GPU."""
import numpy as np
import pytest

from tests import aug_ref as R

N_SAMPLES = 4000


@pytest.fixture(scope="module")
def drawn():
    from zebrapose_amd.augment import AugmentSampler
    return AugmentSampler(True, True, np.random.default_rng(1234)).sample(N_SAMPLES, 16, 24)


def test_sampler_is_deterministic_per_seed():
    from zebrapose_amd.augment import AugmentSampler
    a = AugmentSampler(True, True, np.random.default_rng(7)).sample(64, 40, 60)
    b = AugmentSampler(True, True, np.random.default_rng(7)).sample(64, 40, 60)
    c = AugmentSampler(True, True, np.random.default_rng(8)).sample(64, 40, 60)
    for k in ("flags", "sp_seed", "sp_thresh", "kA", "kB", "masks", "luts", "beta_tab"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    assert a.desc().tobytes() == b.desc().tobytes()
    assert a.desc().tobytes() != c.desc().tobytes()
    assert a.masks.shape == (64, 3, 3) and a.luts.shape == (64, 3, 256)  # max(int(0.05 * 40), 3), max(int(3.0), 3)
    assert a.desc().dtype.itemsize == 53 * 4


def _rate(hits, n, p, what):
    sd = np.sqrt(p * (1 - p) / n)
    assert abs(hits / n - p) <= 4 * sd, f"{what}: {hits}/{n} vs p = {p} (4 sigma = {4 * sd:.4f})"


def test_sometimes_rates(drawn):
    ps = drawn.params
    on = [p for p in ps if p["chain"]]
    _rate(len(on), len(ps), 0.8, "chain")
    for key, p in (("sp", 0.3), ("motion", 0.2), ("dropout", 0.4), ("gauss", 0.5), ("add", 0.5), ("invert", 0.4),
                   ("mul", 0.5), ("mul2", 0.5), ("contrast", 0.5)):
        _rate(sum(bool(q[key]) for q in on), len(on), p, key)
    for stage, key, p in (("add", "add_pc", 0.3), ("mul", "mul_pc", 0.8), ("contrast", "contrast_pc", 0.3)):
        sub = [q for q in on if q[stage]]
        _rate(sum(bool(q[key]) for q in sub), len(sub), p, key)
    inv = np.array([q["invert_on"] for q in on if q["invert"]])
    _rate(int(inv.sum()), inv.size, 0.2, "invert per channel")
    drop = drawn.masks[[i for i, q in enumerate(ps) if q["chain"] and q["dropout"]]]
    _rate(int((drop == 0).sum()), drop.size, 0.1, "dropout cells")
    # flags mirror the choices; a skipped chain is all identity
    for i, q in enumerate(ps):
        f = int(drawn.flags[i])
        if not q["chain"]:
            assert f == 0
            continue
        assert bool(f & R.SP) == q["sp"] and bool(f & R.STENCIL_A) == q["motion"] and bool(f & R.DROPOUT) == q["dropout"]
        assert bool(f & R.STENCIL_B) == (q["gauss"] and q["sigma"] >= 1e-3)
        assert bool(f & R.LUT) == (q["add"] or q["invert"] or q["mul"] or q["mul2"] or q["contrast"])


def test_switches_turn_the_two_optional_stages_off():
    from zebrapose_amd.augment import AugmentSampler
    b = AugmentSampler(False, False, np.random.default_rng(3)).sample(500, 16, 16)
    assert not (b.flags & (R.SP | R.STENCIL_A)).any() and b.flags.any()


def test_parameters_in_range(drawn):
    for i, q in enumerate(drawn.params):
        if not q["chain"]:
            continue
        assert 0.0 <= q["sigma"] < 1.0
        if q["sp"]:
            assert int(drawn.sp_thresh[i]) == int(0.05 * 2 ** 32)
        if q["motion"]:
            assert 0.0 <= q["angle"] < 360.0 and -1.0 <= q["direction"] <= 1.0
        if q["add"]:
            v = np.asarray(q["add_v"])
            assert v.shape == (3,) and (v >= -20).all() and (v <= 20).all() and (v == np.round(v)).all()
            assert q["add_pc"] or (v == v[0]).all()
        if q["mul"]:
            m = np.asarray(q["mul_m"])
            assert (m >= 0.7).all() and (m <= 1.4).all() and (q["mul_pc"] or (m == m[0]).all())
        if q["mul2"]:
            assert 0.7 <= q["mul2_m"] <= 1.4
        if q["contrast"]:
            a = np.asarray(q["alpha"])
            assert (a >= 0.5).all() and (a <= 2.0).all() and (q["contrast_pc"] or (a == a[0]).all())
    adds = np.array([q["add_v"] for q in drawn.params if q["chain"] and q["add"]])
    assert adds.min() == -20 and adds.max() == 20  # both ends of Add((-20, 20)) are reachable
    assert set(np.unique(drawn.masks)) <= {0, 1}


def test_lut_formulas():
    from zebrapose_amd import augment as A
    i = np.arange(256)
    v, m, a = [-20, 7, 20], [0.7, 1.0, 1.4], [0.5, 1.3, 2.0]
    on = [True, False, True]
    la, li, lm, lc = A.lut_add(v), A.lut_invert(on), A.lut_multiply(m), A.lut_contrast(a)
    for c in range(3):
        np.testing.assert_array_equal(la[c], np.clip(i + v[c], 0, 255))
        np.testing.assert_array_equal(li[c], 255 - i if on[c] else i)
        np.testing.assert_array_equal(lm[c], np.clip(np.round(i * m[c]), 0, 255))
        np.testing.assert_array_equal(lc[c], np.clip(127 + a[c] * (i - 127), 0, 255).astype(np.uint8))
    for l in (la, li, lm, lc):
        assert l.dtype == np.uint8 and l.shape == (3, 256)
    img = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    seq = img
    for l in (la, li, lm, lm, lc):
        seq = R.apply_lut(seq, l)
    np.testing.assert_array_equal(R.apply_lut(img, A.compose_luts([la, li, lm, lm, lc])), seq)


def test_sampled_lut_is_the_composition_of_its_stages(drawn):
    """Rebuilt here from the recorded parameters with the formulas written out, in the chain's order."""
    i = np.arange(256)
    seen = 0
    for b, q in enumerate(drawn.params):
        if not q["chain"] or seen >= 200:
            continue
        seen += 1
        for c in range(3):
            t = i.copy()
            if q["add"]:
                t = np.clip(t + q["add_v"][c], 0, 255)
            if q["invert"] and q["invert_on"][c]:
                t = 255 - t
            if q["mul"]:
                t = np.clip(np.round(t * q["mul_m"][c]), 0, 255).astype(np.int64)
            if q["mul2"]:
                t = np.clip(np.round(t * q["mul2_m"]), 0, 255).astype(np.int64)
            if q["contrast"]:
                t = np.clip(127 + q["alpha"][c] * (t - 127), 0, 255).astype(np.uint8)
            np.testing.assert_array_equal(drawn.luts[b, c], t, err_msg=f"sample {b} channel {c}: {q}")


def test_gaussian_kernels(drawn):
    from zebrapose_amd import augment as A
    np.testing.assert_array_equal(A.gaussian_taps(0.5), [0, 27, 202, 27, 0])
    np.testing.assert_array_equal(A.gaussian_taps(0.8), [6, 58, 128, 58, 6])
    for s in (1e-3, 0.05, 0.3, 0.5, 0.8, 0.999):
        k = A.gaussian_kernel(s)
        assert k.dtype == np.int32 and k.shape == (5, 5) and k.sum() == 65536 and (k >= 0).all()
        np.testing.assert_array_equal(k, k.T)
        np.testing.assert_array_equal(k, k[::-1, ::-1])
        np.testing.assert_array_equal(k, k[::-1])
    for b, q in enumerate(drawn.params):
        if q["chain"] and q["gauss"] and q["sigma"] >= 1e-3:
            np.testing.assert_array_equal(drawn.kB[b], A.gaussian_kernel(q["sigma"]))
            assert drawn.kB[b].sum() == 65536


def test_motion_kernels(drawn):
    from zebrapose_amd import augment as A
    n = 0
    for b, q in enumerate(drawn.params):
        if q["chain"] and q["motion"]:
            k = drawn.kA[b]
            assert k.sum() == 65536 and (k >= 0).all() and k[2, 2] > 0, (q, k)
            n += 1
    assert n > 300
    # angle 0: the untouched centre column with imgaug's direction ramp linspace(d, 1 - d) (d = 0 here:
    # weights 0, 1/4, 1/2, 3/4, 1 down the column as u8 levels 0, 63, 127, 191, 255)
    k = A.motion_kernel(0.0, -1.0)
    assert (k[:, [0, 1, 3, 4]] == 0).all()
    lv = np.array([0, 63, 127, 191, 255])
    assert np.abs(k[:, 2] - 65536 * lv / lv.sum()).max() <= 1
    # direction 0 is the uniform line; a quarter turn lays it along the centre row
    k = A.motion_kernel(90.0, 0.0)
    assert (k[[0, 1, 3, 4]] == 0).all() and np.abs(k[2] - 65536 / 5).max() <= 1
    assert A.motion_kernel(37.0, 0.6).sum() == 65536
    # not symmetric in general: what makes the fused kernel's reflected halo worth testing
    k = A.motion_kernel(30.0, 0.8)
    assert (k != k[::-1, ::-1]).any()


class _Injected:
    def __init__(self, scale, shift):
        self.vals = [scale, np.asarray(shift, np.float64)]

    def random(self, n=None):
        v = self.vals.pop(0)
        assert (n is None) == np.isscalar(v)
        return v


@pytest.mark.parametrize("box", [[100, 80, 200, 150], [-40, -30, 120, 200], [560, 400, 150, 120], [0, 0, 0, 0],
                                 [620, -20, 40, 90]])
@pytest.mark.parametrize("u", [(0.0, (0.0, 0.0)), (0.999, (0.999, 0.0)), (0.37, (0.81, 0.12)), (0.5, (0.5, 0.5))])
def test_aug_bbox_formula(box, u):
    from zebrapose_amd.crop import aug_Bbox
    got = aug_Bbox(np.array(box), 1.5, _Injected(u[0], u[1]))
    x, y, w, h = box
    scale = 1 + 0.25 * (2 * u[0] - 1)
    cx = x + w / 2 + w * 0.25 * (2 * u[1][0] - 1)
    cy = y + h / 2 + h * 0.25 * (2 * u[1][1] - 1)
    aw, ah = int(w * scale * 1.5), int(h * scale * 1.5)
    np.testing.assert_array_equal(got, [int(cx - aw / 2), int(cy - ah / 2), aw, ah])
    assert got.shape == (4,) and np.issubdtype(got.dtype, np.integer)


def test_aug_bbox_draw_order_and_range():
    from zebrapose_amd.crop import aug_Bbox
    a = aug_Bbox(np.array([100, 80, 200, 150]), 1.5, np.random.default_rng(5))
    r = np.random.default_rng(5)
    s, sh = r.random(), r.random(2)
    b = aug_Bbox(np.array([100, 80, 200, 150]), 1.5, _Injected(s, sh))
    np.testing.assert_array_equal(a, b)
    rng = np.random.default_rng(0)
    for _ in range(200):
        x, y, w, h = aug_Bbox(np.array([100, 80, 200, 150]), 1.5, rng)
        assert 225 <= w <= 375 and 168 <= h <= 282
        assert abs(x + w / 2 - 200) <= 51 and abs(y + h / 2 - 155) <= 39
