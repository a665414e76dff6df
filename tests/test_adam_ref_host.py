"""tests/adam_ref.py against torch.optim.Adam(foreach=False) on the CPU, bit for bit (no GPU needed).

exp_avg, exp_avg_sq and param are compared after each of three steps, the state fed forward, at sizes
1..69 (ATen's vector bodies and scalar tails) and 2^20 + 3 (its parallel chunks), for gradient scales 1,
3e18 and 1e-22 (denormal a * m and exp_avg_sq) with a fifth of the gradients zero, and beta1 = 0.9 and 0.3
(both branches of lerp).  Nothing is excluded.

torch's vectorised float32 sqrt is not correctly rounded (adam_ref's docstring), so the step is checked
twice: with torch's own sqrt in place of the root every bit of the three tensors must agree, which pins
every other rounding; with the IEEE root exp_avg and exp_avg_sq must still agree on every bit, and param
may differ only where torch's root is off by its one ulp."""
import numpy as np
import pytest
import torch

from tests import adam_ref as R

SIZES = list(range(1, 70)) + [2 ** 20 + 3]
HYPER = {"b1_0.9": (4e-4, 0.9, 0.999, 1e-8), "b1_0.3": (1e-2, 0.3, 0.9, 1e-8)}


def _torch_sqrt(v):
    return torch.from_numpy(np.ascontiguousarray(v)).sqrt().numpy()


def _ieee_sqrt(v):
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(v, np.float64)).astype(np.float32)  # sqrt: f64 -> f32 is correctly rounded


def _run(n, scale, hyper, seed):
    """three steps of torch and of both forms of the reference -> lists of mismatch counts"""
    lr, b1, b2, eps = hyper
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    p, m, v = p0, np.zeros(n, np.float32), np.zeros(n, np.float32)
    for s in (1, 2, 3):
        g = (rng.standard_normal(n) * scale).astype(np.float32)
        g[rng.random(n) < 0.2] = 0.0
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[tp]
        tm, tv, tpp = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), tp.detach().numpy()
        pi, mi, vi = R.step(p, g, m, v, lr, b1, b2, eps, s)                 # the IEEE root
        p, m, v = R.step(p, g, m, v, lr, b1, b2, eps, s, sqrt=_torch_sqrt)  # torch's root; fed forward
        for name, got, want in (("exp_avg", m, tm), ("exp_avg_sq", v, tv), ("param", p, tpp)):
            bad = R.mismatches(got, want)
            assert bad.size == 0, (name, n, scale, b1, s, bad.size, bad[:4], got[bad[:4]], want[bad[:4]])
        assert R.same_bits(mi, tm) and R.same_bits(vi, tv)
        off = R.mismatches(pi, tpp)
        root_off = R.mismatches(_torch_sqrt(v), _ieee_sqrt(v))
        assert np.isin(off, root_off).all(), (n, scale, b1, s, off.size)


@pytest.mark.parametrize("hyper", list(HYPER), ids=list(HYPER))
@pytest.mark.parametrize("scale", [1.0, 3e18, 1e-22], ids=["1", "3e18", "1e-22"])
def test_adam_ref_is_torch_bit_for_bit(scale, hyper):
    for n in SIZES:
        _run(n, scale, HYPER[hyper], seed=n)


def test_numpy_sqrt_is_the_ieee_root_and_torch_is_within_one_ulp():
    rng = np.random.default_rng(0)
    v = np.abs(rng.standard_normal(1 << 18) * np.exp(rng.uniform(-80, 80, 1 << 18))).astype(np.float32)
    v[:4] = [0.0, 1e-45, np.inf, 3.4e38]
    want = _ieee_sqrt(v)
    assert R.same_bits(np.sqrt(v), want)
    d = _torch_sqrt(v).view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)
    assert np.abs(d).max() <= 1


def test_fma_is_one_rounding():
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * np.exp(rng.uniform(-20, 20, 4000))).astype(np.float32)
    # sums that sit on or beside an f32 midpoint, where rounding an f64 sum again goes wrong:
    # 1 + 2^-24 is the midpoint of 1 and 1 + 2^-23; the products below land 2^-48 .. 2^-70 away from it
    one, h = np.float32(1.0), np.float32(2.0 ** -24)
    ea = np.array([h, h, h, h, h, h], np.float32)
    eb = np.array([1.0, 1 + 2.0 ** -23, 1 - 2.0 ** -24, 1.0, 1.0, 1.0], np.float32)
    ec = np.array([one, one, one, 1 + 2.0 ** -23, -one, 2.0 ** -126], np.float32)
    a, b, c = np.concatenate([a, ea]), np.concatenate([b, eb]), np.concatenate([c, ec])
    got = R.fma(a, b, c)

    def exact(x, y, z):
        e = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        r = np.float32(float(e))  # python rounds the rational to f64 correctly; then decide among neighbours
        cands = [np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))]
        return min(cands, key=lambda q: (abs(Fraction(float(q)) - e), int(q.view(np.uint32)) & 1))

    want = np.array([exact(*t) for t in zip(a, b, c)], np.float32)
    assert R.same_bits(got, want), R.mismatches(got, want)
    assert got[-6] == one and got[-5] == np.float32(1 + 2.0 ** -23) and got[-4] == one  # tie, above, below


def test_lerp_branch_and_constants():
    w1, b2, w2, a, s, e = R.constants(1e-2, 0.3, 0.9, 1e-8, 2)
    assert w1 >= 0.5 and a < 0 and R.constants(4e-4, 0.9, 0.999, 1e-8, 1)[0] < 0.5
    g, m = np.array([3.0], np.float32), np.array([1.0], np.float32)
    z = np.zeros(1, np.float32)
    _, m1, _ = R.step(z, g, m, z, 1e-2, 0.3, 0.9, 1e-8, 1)
    want = torch.lerp(torch.from_numpy(m), torch.from_numpy(g), float(1 - 0.3)).numpy()
    assert R.same_bits(m1, want)
