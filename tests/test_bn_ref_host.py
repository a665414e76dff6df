"""tests/bn_ref.py held to torch.nn.BatchNorm2d in float64 (training mode), on the CPU: forward, the running
statistics after two steps, autograd's dx / dgamma / dbeta -- with and without ReLU and a residual, with
count == 1 and with a conv bias -- and the preconditions of the exact cases tests/test_gpu_bn_edges.py
compares bit for bit (every partial sum an integer multiple of its grid below 2^24 times that grid)."""
import numpy as np
import pytest
import torch

from tests import bn_ref as R


def _bounds(P, nparts):
    """nparts pixel ranges covering [0, P), one of them empty when there is room for it"""
    cuts = sorted(set(np.linspace(0, P, nparts, dtype=int).tolist() + [0, P]))
    b = list(zip(cuts[:-1], cuts[1:]))
    return b + [(P, P)] if len(b) > 1 else b


@pytest.mark.parametrize("N,H,W", [(3, 5, 7), (1, 1, 1)], ids=["p105", "count1"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_against_torch_batchnorm_f64(N, H, W, relu, res, bias):
    C, P, eps, mom = 6, N * H * W, 1e-5, 0.1
    g = torch.Generator().manual_seed(N * 100 + relu * 10 + res)
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=mom).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    cb = torch.randn(C, generator=g, dtype=torch.float64) if bias else None
    rm, rv, nbt = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy(), 0
    gamma, beta = bn.weight.detach().numpy().copy(), bn.bias.detach().numpy().copy()
    for step in range(2):
        raw = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.3   # the conv output without its bias
        r = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) if res else None
        dy = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
        xin = (raw if cb is None else raw + cb.view(1, C, 1, 1)).requires_grad_(True)
        if P > 1:
            y = bn(xin)
        else:   # the module refuses one value per channel; the operator under it does not
            y = torch.batch_norm(xin, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, mom, eps, False)
            bn.num_batches_tracked += 1
        if res:
            y = y + r
        if relu:
            y = torch.relu(y)
        bn.zero_grad()
        y.backward(dy)
        flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(P, C).numpy()  # noqa: E731
        # bn_ref on the raw values, the bias handed to the finalize as the engine does
        x = flat(raw)
        f = R.finalize(*R.parts_of(x, _bounds(P, 4)), eps, mom, gamma, beta, None if cb is None else cb.numpy(),
                       rm, rv, nbt, rnd=R.ident)
        np.testing.assert_allclose(f["rm"], bn.running_mean.numpy(), rtol=1e-12, atol=1e-12)
        if P > 1:
            np.testing.assert_allclose(f["rv"], bn.running_var.numpy(), rtol=1e-12, atol=1e-12)
        else:   # n == 1: torch's n / (n - 1) divides by zero; zp.h takes the biased variance, 0
            np.testing.assert_allclose(f["rv"], (1 - mom) * rv, rtol=1e-15)
            with torch.no_grad():
                bn.running_var.copy_(torch.from_numpy(f["rv"]))
        rm, rv, nbt = f["rm"], f["rv"], f["nbt"]
        assert nbt == int(bn.num_batches_tracked)
        yr = x * f["scale"] + f["shift"] + (flat(r) if res else 0.0)
        yr = np.maximum(yr, 0.0) if relu else yr
        np.testing.assert_allclose(yr, flat(y), rtol=1e-11, atol=1e-11)
        if P == 1:
            assert (f["var"] == 0).all() and np.allclose(f["save"][1], 1 / np.sqrt(eps))
        m = R.mask(1, y=yr) if relu else None
        gg, xhat, gx = R.bwd_terms(flat(dy), m, x, f["save"])
        (_, sg), (_, sgx) = R.bwd_sums(gg, 16), R.bwd_sums(gx, 16)
        np.testing.assert_allclose(sg, bn.bias.grad.numpy(), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(sgx, bn.weight.grad.numpy(), rtol=1e-8, atol=1e-8 * (1 + 300 * (P == 1)))
        dx = R.bwd_dx(gg, xhat, sg, sgx, gamma, f["save"])
        np.testing.assert_allclose(dx, flat(xin.grad), rtol=1e-8, atol=1e-8 * (1 + 300 * (P == 1)))
        # the f32 rounding points move the saved statistics by no more than their roundings
        f32v = R.finalize(*R.parts_of(x, _bounds(P, 4)), eps, mom, R.f32(gamma), R.f32(beta))
        assert (np.abs(f32v["save"][:2] - f["save"][:2]) <= 2.0 ** -23 * np.abs(f["save"][:2])).all()


def test_mask_from_raw_is_the_apply_sign():
    """rule 2 is the sign of the value zp_bn_apply forms before its store, fma included: where the product
    rounded first would give 0, the fma keeps the residual's sign"""
    x, sc = np.float64(np.float32(1 + 2.0 ** -7)), np.float64(np.float32(1 + 2.0 ** -20))
    sh = -R.f32(x * sc)
    exact = x * sc + sh
    assert exact != 0 and R.fma32(x, sc, sh) == exact
    save = np.array([[0.0], [1.0], [sc], [sh]])
    assert bool(R.mask(2, x=np.array([[x]]), save=save)[0, 0]) == (exact > 0)
    assert not R.mask(1, y=np.array([[0.0, -0.0]])).any()


def test_rn32_sum_rounds_once():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(20000) * 2.0 ** rng.integers(-30, 30, 20000)
    b = rng.standard_normal(20000) * 2.0 ** rng.integers(-30, 30, 20000)
    a[:4], b[:4] = [1.0, 1.0, -1.0, 3.0], [2.0 ** -24 + 2.0 ** -70, 2.0 ** -24 - 2.0 ** -70, -2.0 ** -24 - 2.0 ** -70, 2.0 ** -23]
    from fractions import Fraction
    got = R.rn32_sum(a, b)
    for i in range(300):
        ex = Fraction(float(a[i])) + Fraction(float(b[i]))
        c = np.float32(float(ex))
        cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - ex), int(np.float32(v).view(np.uint32)) & 1))
        assert float(best) == got[i], i


@pytest.mark.parametrize("parts", [1, 3, 127, 128, 129, 511, 512, 513, 577, 1100])
@pytest.mark.parametrize("C", [1, 7, 9, 33, 40])
def test_exact_finalize_cases_are_exact(parts, C):
    c = R.exact_finalize_case(parts, C)
    for v in (c["cnt"], c["mean"], c["m2"]):
        assert (v == np.round(v)).all() and (R.f32(v) == v).all()
    assert (np.abs(c["cnt"] * c["mean"]).sum(0) < 2 ** 24).all()
    one = R.finalize(c["cnt"], c["mean"], c["m2"], c["eps"], 1.0, c["gamma"], c["beta"], c["bias"], c["rm"], c["rv"])
    two = R.finalize(c["cnt"], c["mean"], c["m2"], c["eps"], 1.0, c["gamma"], c["beta"], c["bias"], c["rm"], c["rv"],
                     level1=64)
    assert (one["mean"] == np.round(one["mean"])).all() and np.isin(one["var"], [16.0, 64.0]).all()
    q = c["m2"] + c["cnt"] * (c["mean"] - one["mean"]) ** 2
    assert (q == np.round(q)).all() and (q.sum(0) < 2 ** 24).all()
    for k in ("save", "rm", "rv"):
        assert (one[k] == two[k]).all()           # the first level's f32 write-back rounds nothing here
    assert np.isin(one["save"][1], [0.25, 0.125]).all()
    assert (one["save"][3] == c["beta"] - one["save"][0] * one["save"][2]).all()


@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("P,C", [(1, 8), (1024, 8), (2051, 8), (683, 24), (64, 64), (259, 64), (11, 1600), (64, 2048)])
def test_exact_backward_cases_are_exact(P, C, relu):
    c = R.exact_bwd_case(P, C, relu)
    for k in ("dy", "x", "y", "gamma"):
        assert (R.to_store(c[k], R.BF16) == c[k]).all()
    m = R.mask(relu, c["y"], c["x"], c["save"])
    if relu == 2:
        assert (m == (c["x"] * c["save"][2] + c["save"][3] > 0)).all()     # the fma is exact: half-integers
    if relu == 1:
        assert ((c["y"] == 0) & np.signbit(c["y"])).any() or P * C < 64     # -0 is drawn
    g, xhat, gx = R.bwd_terms(c["dy"], m, c["x"], c["save"])
    assert (2 * gx == np.round(2 * gx)).all() and (2 * np.abs(gx).sum(0) < 2 ** 24).all()
    assert (np.abs(g).sum(0) < 2 ** 24).all()
    if P & (P - 1) == 0:   # 1 / P enters dx: every term a multiple of 2^-k / 4 below 2^24 such steps
        sg, sgx = g.sum(0), gx.sum(0)
        step = 0.25 / P
        for t in (sg / P, xhat * (sgx / P), g - sg / P - xhat * (sgx / P)):
            assert (t / step == np.round(t / step)).all() and (np.abs(t) / step < 2 ** 24).all()
