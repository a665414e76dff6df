"""The loss kernels (zp_loss.hip) at the sizes and options the fixtures do not reach: tail lanes,
waves and blocks of the reductions, L % 8 != 0 and L = 32, the grid-stride loops of the gradient and
mask-partial kernels (more than 8192 x 256 and 262 144 elements), uint8 targets, the mask taken from
logits, mask_code / use_hist off, and a soft (non-0/1) f64 mask.

Driven through BinaryCodeLoss / MaskLoss and their autograd functions with (3 * loss_b +
loss_m).backward(), as the trainer does; references are oracle.ref_cpu (BCE, mask) and
F.cross_entropy (CE) on the CPU in f64 from the same f32 logits.  The histogram term thresholds the
f32 sigmoid, as the reference does (x > kHalfLogit); logits are planted at kHalfLogit and its neighbours.

Bounds: f64 losses rtol 1e-12, histogram atol 1e-15, code gradients rtol 1e-5 / atol 1e-12, the f32
mask loss rtol 1e-6 (f64 reduction; the f32 sigmoid and the final cast round), its gradient rtol
1e-4 / atol 1e-10 -- tests/test_gpu_parity.py's bounds for the same kernels.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KH = np.float32(8.940696716308594e-08)  # zp_common.h kHalfLogit: CPU fp32 sigmoid(x) > 0.5  <=>  x > kHalfLogit
PLANT = np.array([40.0, -40.0, 0.0, -0.0, KH, np.nextafter(KH, np.float32(1)), np.nextafter(KH, np.float32(-1))],
                 dtype=np.float32)


def _logits(rng, shape):
    """N(0, 3) with the edge values planted (twice each) at random places, when there is room."""
    x = (rng.standard_normal(shape) * 3).astype(np.float32)
    if x.size >= 4 * PLANT.size:
        pos = rng.choice(x.size, 2 * PLANT.size, replace=False)
        x.reshape(-1)[pos] = np.tile(PLANT, 2)
    return x


# ------------------------------------------------------------------------------------ binary code loss
CODE_CASES = {"a": (1, 1, 1, 1), "b": (3, 7, 9, 7), "c": (2, 20, 13, 11), "d": (1, 32, 5, 53), "e": (1, 2, 1449, 1448)}
CODE_RUNS = [(c, g, m, mc, uh) for c in "abcd"
             for g, m, mc, uh in itertools.product(["f64", "u8"], ["mask01", "logits"], [True, False], [True, False])]
CODE_RUNS.append(("e", "u8", "logits", True, True))


def _code_inputs(case):
    Bc, Lc, Hc, Wc = CODE_CASES[case]
    rng = np.random.default_rng([21, ord(case)])
    code = _logits(rng, (Bc, Lc, Hc, Wc))
    mlog = _logits(rng, (Bc, 1, Hc, Wc))
    gts = [(rng.random((Bc, Lc, Hc, Wc)) < 0.5).astype(np.uint8) for _ in range(2)]
    gmask = (rng.random((Bc, Hc, Wc)) < 0.5).astype(np.float32)
    return code, mlog, gts, gmask


def _run_code_loss(gpu, code, mlog, mask01, gts, gmask, gt_kind, mask_kind, mask_code, use_hist):
    """One trainer-shaped step on the device and on the oracle, then a second forward with a new
    target (the histogram EMA).  ``mask01`` f64 [B, 1, H, W] is what the oracle multiplies by."""
    from oracle import ref_cpu
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeLoss, MaskLoss
    bcl, ml = BinaryCodeLoss("BCE", mask_code, 2, use_hist), MaskLoss()
    c = torch.from_numpy(code).to(gpu).requires_grad_(True)
    m = torch.from_numpy(mlog).to(gpu).requires_grad_(True)
    m01 = torch.from_numpy(mask01).to(gpu)

    def dev_gt(g):
        return torch.from_numpy(g.astype(np.float64) if gt_kind == "f64" else g).to(gpu)

    def dev_loss(cc, g):
        if mask_kind == "logits":
            return bcl.forward_from_logits(cc, m, dev_gt(g))
        return bcl(cc, m01, dev_gt(g))

    lb = dev_loss(c, gts[0])
    lm = ml(m, torch.from_numpy(gmask).to(gpu))
    assert lb.dtype == torch.float64 and lm.dtype == torch.float32
    (3 * lb + lm).backward()
    c2 = torch.from_numpy(code).requires_grad_(True)
    m2 = torch.from_numpy(mlog).requires_grad_(True)
    st = ref_cpu.HistLossState()
    mt = torch.from_numpy(mask01)
    lb2 = ref_cpu.binary_code_loss(st, c2, mt, torch.from_numpy(gts[0].astype(np.float64)), mask_code=mask_code,
                                   use_hist=use_hist)
    assert lb2.dtype == torch.float64
    (3 * lb2 + ref_cpu.mask_loss(m2, torch.from_numpy(gmask))).backward()
    g_got, g_ref = c.grad.cpu().numpy(), c2.grad.numpy()
    print(f"loss_b {lb.item():.17g} ref {lb2.item():.17g} rel {abs(lb.item() - lb2.item()) / abs(lb2.item()):.3g}; "
          f"grad max |d| {np.abs(g_got - g_ref).max():.3g}")
    np.testing.assert_allclose(lb.item(), lb2.item(), rtol=1e-12)
    np.testing.assert_allclose(g_got, g_ref, rtol=1e-5, atol=1e-12)
    if not use_hist:
        assert bcl.histogram is None and st.histogram is None
        return
    np.testing.assert_allclose(bcl.histogram.cpu().numpy(), st.histogram.numpy(), atol=1e-15)
    lb3 = dev_loss(c.detach(), gts[1])
    lb4 = ref_cpu.binary_code_loss(st, c2.detach(), mt, torch.from_numpy(gts[1].astype(np.float64)),
                                   mask_code=mask_code, use_hist=True)
    np.testing.assert_allclose(bcl.histogram.cpu().numpy(), st.histogram.numpy(), atol=1e-15)
    np.testing.assert_allclose(lb3.item(), lb4.item(), rtol=1e-12)


@pytest.mark.parametrize("case,gt_kind,mask_kind,mask_code,use_hist", CODE_RUNS,
                         ids=["%s-%s-%s-mc%d-hist%d" % r for r in CODE_RUNS])
def test_code_loss(gpu, case, gt_kind, mask_kind, mask_code, use_hist):
    """a: one element; b: 189 pixels (a 61-lane last wave), L < 8; c: 286 pixels (a 30-lane last
    block), L = 8 + 8 + 4; d: L = 32, the most the kernel takes; e: 2 098 152 pixels, past the 8192 x 256
    threads of k_code_grad, so its grid-stride loop runs."""
    from oracle import ref_cpu
    code, mlog, gts, gmask = _code_inputs(case)
    mask01 = ref_cpu.threshold_np(mlog)  # train_v6.py:325-326: the host's f64 0/1 mask of the same logits
    _run_code_loss(gpu, code, mlog, mask01, gts, gmask, gt_kind, mask_kind, mask_code, use_hist)


def test_code_loss_soft_mask(gpu):
    """A non-0/1 f64 mask (case c): the Hamming term uses round().clamp(0, 1) -- 0.5 -> 0 and
    1.5 -> 2 -> 1, half to even -- while the BCE term multiplies the logits by the raw value."""
    code, mlog, gts, gmask = _code_inputs("c")
    rng = np.random.default_rng(22)
    mask = rng.choice(np.array([0.0, 1.0, 0.5, 1.5, 0.25, -0.2]), size=mlog.shape)
    assert all((mask == v).any() for v in (0.5, 1.5, 0.25, -0.2))
    _run_code_loss(gpu, code, mlog, mask, gts, gmask, "f64", "mask01", True, True)


def test_code_loss_refuses_33_bits(gpu):
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeLoss
    c = torch.zeros(1, 33, 2, 2, device=gpu)
    with pytest.raises(RuntimeError, match="bad sizes"):
        BinaryCodeLoss("BCE", True, 2, True)(c, torch.ones(1, 1, 2, 2, dtype=torch.float64, device=gpu),
                                             torch.zeros(1, 33, 2, 2, dtype=torch.float64, device=gpu))


# ------------------------------------------------------------------------------------------- mask loss
@pytest.mark.parametrize("n", [1, 63, 257, 2048 + 1, 262144 + 77, 8192 * 256 + 5])
def test_mask_loss(gpu, n):
    """n past 262 144 enters the grid-stride loop of k_mask_partials (1024 blocks), n past
    8192 x 256 that of k_mask_grad.  Targets 0/1; where x = 0 and g = 0.5 the f32 sigmoid equals the
    target, the sign is 0 and the gradient exactly 0; logits at +-100 saturate the sigmoid."""
    from oracle import ref_cpu
    from zebrapose_amd.model.BinaryCodeNet import MaskLoss
    rng = np.random.default_rng([23, n])
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    g = (rng.random(n) < 0.5).astype(np.float32)
    zero = np.zeros(0, dtype=int)
    if n >= 63:
        zero = np.array([0, n // 2, n - 1])
        x[zero], g[zero] = 0.0, 0.5
        x[[1, 2, n - 3, n - 2]] = [100.0, 100.0, -100.0, -100.0]
        g[[1, 2, n - 3, n - 2]] = [1.0, 0.0, 1.0, 0.0]
    xt = torch.from_numpy(x).reshape(1, 1, 1, n)
    gt = torch.from_numpy(g).reshape(1, 1, n)
    xd = xt.to(gpu).requires_grad_(True)
    lm = MaskLoss()(xd, gt.to(gpu))
    assert lm.dtype == torch.float32
    (3 * lm).backward()
    ref = float((torch.sigmoid(xt[:, 0]).double() - gt.double()).abs().mean())
    print(f"mask loss n={n}: {lm.item():.9g} ref {ref:.17g} rel {abs(lm.item() - ref) / ref:.3g}")
    np.testing.assert_allclose(lm.item(), ref, rtol=1e-6)
    x2 = xt.clone().requires_grad_(True)
    (3 * ref_cpu.mask_loss(x2, gt)).backward()
    got = xd.grad.cpu().numpy()
    np.testing.assert_allclose(got, x2.grad.numpy(), rtol=1e-4, atol=1e-10)
    assert np.all(got.reshape(-1)[zero] == 0.0)


# --------------------------------------------------------------------------------------------- CE loss
CE_CASES = [(2, 3, 1, 1, 1), (4, 8, 3, 9, 7), (16, 4, 2, 13, 11), (256, 2, 1, 5, 53), (4, 2, 1, 1025, 1024)]


@pytest.mark.parametrize("mask_kind", ["mask01", "logits"])
@pytest.mark.parametrize("mask_code", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("d,Lc,Bc,Hc,Wc", CE_CASES, ids=["d%d-L%d-%dx%dx%d" % c for c in CE_CASES])
def test_ce_loss(gpu, d, Lc, Bc, Hc, Wc, mask_code, mask_kind):
    """nn.CrossEntropyLoss(mean) in f64 over pred.reshape(-1, d, H, W) (BinaryCodeNet.py:57-60, 65),
    the mask applied to the logits (:47-48).  The last case has 2 099 200 rows, past the 8192 x 256
    threads of k_ce_grad.  The f64 mask goes with f64 digits, the logits mask with uint8 digits."""
    from oracle import ref_cpu
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeLoss
    rng = np.random.default_rng([24, d, Lc, Hc])
    code = _logits(rng, (Bc, Lc * d, Hc, Wc))
    mlog = _logits(rng, (Bc, 1, Hc, Wc))
    gt = rng.integers(0, d, (Bc, Lc, Hc, Wc)).astype(np.uint8)
    mask01 = ref_cpu.threshold_np(mlog)
    fn = BinaryCodeLoss("CE", mask_code, d, False)
    c = torch.from_numpy(code).to(gpu).requires_grad_(True)
    if mask_kind == "logits":
        loss = fn.forward_from_logits(c, torch.from_numpy(mlog).to(gpu), torch.from_numpy(gt).to(gpu))
    else:
        loss = fn(c, torch.from_numpy(mask01).to(gpu), torch.from_numpy(gt.astype(np.float64)).to(gpu))
    assert loss.dtype == torch.float64
    (3 * loss).backward()
    c2 = torch.from_numpy(code).requires_grad_(True)
    z = torch.from_numpy(mask01) * c2 if mask_code else c2.double()
    ref = F.cross_entropy(z.reshape(-1, d, Hc, Wc), torch.from_numpy(gt).view(-1, Hc, Wc).long(), reduction="mean")
    (3 * ref).backward()
    got, want = c.grad.cpu().numpy(), c2.grad.numpy()
    print(f"CE d={d} L={Lc}: loss {loss.item():.17g} ref {ref.item():.17g} "
          f"rel {abs(loss.item() - ref.item()) / ref.item():.3g}; grad max |d| {np.abs(got - want).max():.3g}")
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-12)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("d", [1, 257])
def test_ce_loss_refuses_class_count(gpu, d):
    from zebrapose_amd import _lib as L
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeLoss
    with pytest.raises(ValueError):
        BinaryCodeLoss("CE", True, d, False)
    code = torch.zeros(1, d, 2, 2, device=gpu)
    m01 = torch.ones(1, 1, 2, 2, dtype=torch.float64, device=gpu)
    gt = torch.zeros(1, 1, 2, 2, dtype=torch.uint8, device=gpu)
    out = torch.full((1,), 7.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(L.lib.zp_ce_loss_ws_bytes(1, 1, 2, 2)), dtype=torch.uint8, device=gpu)
    dcode = torch.full_like(code, 7.0)
    with pytest.raises(RuntimeError, match="bad sizes"):
        L.call("zp_ce_loss", code.data_ptr(), m01.data_ptr(), None, gt.data_ptr(), 0, 1, 1, d, 2, 2, 1, out.data_ptr(),
               ws.data_ptr(), L.stream_ptr())
    with pytest.raises(RuntimeError, match="bad sizes"):
        L.call("zp_ce_loss_bwd", code.data_ptr(), m01.data_ptr(), None, gt.data_ptr(), 0, 1, 1, d, 2, 2, 1, None,
               dcode.data_ptr(), L.stream_ptr())
    assert float(out.cpu()[0]) == 7.0 and bool((dcode.cpu() == 7.0).all())
