"""CPU checks of the references that tests/test_gpu_glue.py and tests/test_gpu_loss_edges.py hold
the kernels to: the mask_code / use_hist options of oracle.ref_cpu.binary_code_loss, the half-ulp
helper, the interpolation backward (adjoint of the forward) and the planted threshold values."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from tests import test_gpu_glue as glue
from tests import test_gpu_loss_edges as edges


def _case():
    code, mlog, gts, _ = edges._code_inputs("c")
    return (torch.from_numpy(code), torch.from_numpy(ref_cpu.threshold_np(mlog)),
            torch.from_numpy(gts[0].astype(np.float64)), torch.from_numpy(gts[1].astype(np.float64)))


def test_binary_code_loss_defaults_unchanged():
    """Keyword defaults are the old function: same value bit for bit, same state, over two calls."""
    code, m, g0, g1 = _case()
    s0, s1 = ref_cpu.HistLossState(), ref_cpu.HistLossState()
    for g in (g0, g1):
        a = ref_cpu.binary_code_loss(s0, code, m, g)
        b = ref_cpu.binary_code_loss(s1, code, m, g, mask_code=True, use_hist=True)
        # the expression of the function before the options, restated
        z = m.clone().detach() * code
        w = torch.exp(torch.minimum(s0.histogram, 0.51 - s0.histogram) * 3)
        old = torch.sum(F.binary_cross_entropy_with_logits(z, g, reduction="none").mean([0, 2, 3]) * w) / torch.sum(w)
        assert a.dtype == torch.float64 and a.item() == b.item() == old.item()
        assert torch.equal(s0.histogram, s1.histogram)


def test_binary_code_loss_options():
    code, m, g0, _ = _case()
    # unmasked: the loss of an all-ones mask's BCE term; the histogram still uses the mask
    st = ref_cpu.HistLossState()
    got = ref_cpu.binary_code_loss(st, code, m, g0, mask_code=False)
    _, h = ref_cpu.hamming(code, g0, m)
    w = torch.exp(torch.minimum(h, 0.51 - h) * 3)
    x = code.double()
    bce = (torch.clamp(x, min=0) - x * g0 + torch.log1p(torch.exp(-x.abs()))).mean([0, 2, 3])
    np.testing.assert_allclose(got.item(), float((bce * w).sum() / w.sum()), rtol=1e-14)
    assert torch.equal(st.histogram, h)
    # no histogram: the plain mean over every element, state untouched
    st = ref_cpu.HistLossState()
    got = ref_cpu.binary_code_loss(st, code, m, g0, use_hist=False)
    z = m * code
    want = F.binary_cross_entropy_with_logits(z, g0, reduction="mean")
    np.testing.assert_allclose(got.item(), want.item(), rtol=1e-14)
    assert st.histogram is None
    got = ref_cpu.binary_code_loss(st, code, m, g0, mask_code=False, use_hist=False)
    np.testing.assert_allclose(got.item(), float(bce.mean()), rtol=1e-14)


def test_half_ulp():
    assert float(glue.half_ulp(torch.tensor(1.0, dtype=torch.float64), torch.float32)) == 2.0 ** -24
    assert float(glue.half_ulp(torch.tensor(-1.5, dtype=torch.float64), torch.bfloat16)) == 2.0 ** -8
    assert float(glue.half_ulp(torch.tensor(0.75, dtype=torch.float64), torch.float16)) == 2.0 ** -12
    assert float(glue.half_ulp(torch.tensor(1e-7, dtype=torch.float64), torch.float16)) == 2.0 ** -25
    assert float(glue.half_ulp(torch.tensor(0.0, dtype=torch.float64), torch.float32)) == 2.0 ** -150
    torch.manual_seed(0)
    v = torch.randn(20000, dtype=torch.float64)
    for dt in glue.MANT:
        r = (v.float().to(dt).double() - v.float().double()).abs() / glue.half_ulp(v.float().double(), dt)
        assert float(r.max()) <= 1.0 and (dt == torch.float32 or float(r.max()) > 0.95)


def test_interp_bwd_ref_is_the_adjoint():
    for ih, iw, oh, ow in glue.INTERP:
        torch.manual_seed(1)
        x = torch.randn(2, 1, ih, iw)
        dy = torch.randn(2, oh, ow)
        y = F.interpolate(x, (oh, ow), mode="bilinear", align_corners=False)[:, 0]
        dx = glue._interp_bwd_ref(dy, ih, iw)
        np.testing.assert_allclose(float((y.double() * dy.double()).sum()), float((x.double() * dx.double()).sum()),
                                   rtol=0, atol=1e-5 * float(dy.abs().sum()))
        # weights of every output sum to 1
        np.testing.assert_allclose(dx.double().sum().item(), dy.double().sum().item(), atol=1e-5 * float(dy.abs().sum()))


def test_threshold_planted_values():
    x, pos, want = glue._threshold_input()
    assert x.size == 777 and np.array_equal(ref_cpu.threshold_np(x)[pos], want)
    s = torch.sigmoid(torch.from_numpy(x))  # the definition the boundary restates (common_ops.py:5-11)
    with np.errstate(invalid="ignore"):
        assert np.array_equal((s > 0.5).numpy().astype(np.float64), ref_cpu.threshold_np(x))
