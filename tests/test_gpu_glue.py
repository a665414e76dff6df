"""The small kernels between the convolutions (zp_glue.hip, zp_pool.hip, zp_bn.hip), each called through the C ABI and
compared with a CPU reference of the same operation on the same stored values: zp_copy_slice,
zp_head_grad_to_nhwc, zp_add_broadcast_hw, zp_bn_fold, zp_mask_interp / _bwd and zp_threshold.

Every destination is pre-filled with a sentinel (7.0): whatever lies outside the addressed channel
slice must still hold it, whatever lies inside must have been written.  A 16-bit operand is rounded
to its dtype first and widened from there.  Default geometry: 3 x 9 x 14 = 378 pixels, a multiple of
neither the 256-thread block nor the 64-lane wave.

Bounds (each derived next to its test): pure copies / casts / repacks exact; one f32 multiply-add
half an ulp of the output plus 2^-22 of the operands (contracted to an fma or not); the BN fold four
f32 roundings; the bilinear resampling half an ulp of the output plus four f32 roundings of max|x|;
its backward 2^-18 of the same backward on |dy| (at most 64 products per element) and, per image,
sum(dx) = sum(dy) (every output's weights sum to 1).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 7.0
B, H, W = 3, 9, 14
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}
# (H, W) -> (OH, OW): the network's 4:1 and 2:1, a non-integer upsample, a ragged downsample,
# identity, one pixel in, one pixel out
INTERP = [(8, 8, 2, 2), (8, 8, 4, 4), (5, 7, 13, 9), (37, 29, 13, 8), (7, 7, 7, 7), (1, 1, 4, 3), (4, 3, 1, 1)]
INTERP_IDS = ["%dx%d-%dx%d" % c for c in INTERP]


def half_ulp(ref, dt):
    """Half the spacing of ``dt`` at |ref| (f64 tensor), subnormal spacing below the normal range."""
    _, e = torch.frexp(ref.abs().double())  # |ref| = m * 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, EMIN[dt]), (e - 1).clamp_min(EMIN[dt]))  # frexp(0) = (0, 0)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - MANT[dt] - 1)


def sentinel_outside(yc, c0, C):
    """Everything of the NHWC buffer ``yc`` outside channels [c0, c0 + C) still holds the sentinel."""
    return bool((yc[..., :c0] == SENT).all()) and bool((yc[..., c0 + C:] == SENT).all())


# ------------------------------------------------------------------------------------ zp_copy_slice
COPY = {"odd": (B * H * W, 5, 11, 3, 9, 2), "concat": (2 * 8 * 8, 64, 64, 0, 1088, 960)}  # P, C, ldx, cx0, ldy, cy0


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("ydt", ["fp32", "bf16"])
@pytest.mark.parametrize("xdt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(COPY))
def test_copy_slice(gpu, case, xdt, ydt, acc):
    """y[p, cy0 + c] (+)= x[p, cx0 + c]: one f32 add of the stored values, rounded to y's dtype."""
    from zebrapose_amd import _lib as L
    P, C, ldx, cx0, ldy, cy0 = COPY[case]
    xd, yd = DT[xdt], DT[ydt]
    torch.manual_seed(11)
    x = torch.randn(P, ldx).to(xd)
    y = torch.full((P, ldy), SENT, dtype=yd)
    if acc:
        y[:, cy0:cy0 + C] = torch.randn(P, C).to(yd)
    want = x[:, cx0:cx0 + C].float()
    if acc:
        want = want + y[:, cy0:cy0 + C].float()
    want = want.to(yd)
    assert bool((want.float() != SENT).all())  # so that an unwritten element cannot pass
    yg = y.to(gpu)
    L.call("zp_copy_slice", x.to(gpu).data_ptr(), ldx, cx0, L.dtype_code(xd), yg.data_ptr(), ldy, cy0,
           L.dtype_code(yd), P, C, acc, L.stream_ptr())
    yc = yg.cpu()
    assert torch.equal(yc[:, cy0:cy0 + C], want)
    assert sentinel_outside(yc, cy0, C)


@pytest.mark.parametrize("side", ["x", "y"])
def test_copy_slice_refuses_fp16(gpu, side):
    from zebrapose_amd import _lib as L
    x = torch.zeros(4, 8, dtype=torch.float16, device=gpu)
    y = torch.zeros(4, 8, dtype=torch.float16, device=gpu)
    xc, yc = (L.ZP_F16, L.ZP_BF16) if side == "x" else (L.ZP_BF16, L.ZP_F16)
    with pytest.raises(RuntimeError, match="inference-only"):
        L.call("zp_copy_slice", x.data_ptr(), 8, 0, xc, y.data_ptr(), 8, 0, yc, 4, 8, 0, L.stream_ptr())


# ----------------------------------------------------------------------------- zp_head_grad_to_nhwc
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("Lc,ldy", [(16, 32), (16, 17), (5, 8), (0, 32), (64, 72)])
def test_head_grad_to_nhwc(gpu, prec, Lc, ldy):
    """Channel 0 = dmask, 1..L = dcode, L+1..ldy-1 zero (not the sentinel), rounded to the dtype.
    bf16 with ldy % 8 == 0 takes the 16-byte form, ldy = 17 and every fp32 call the scalar one;
    L = 0 passes no dcode."""
    from zebrapose_amd import _lib as L
    dt = DT[prec]
    torch.manual_seed(12)
    dmask = torch.randn(B, 1, H, W)
    dcode = torch.randn(B, Lc, H, W) if Lc else None
    want = torch.zeros(B, H, W, ldy)
    want[..., 0] = dmask[:, 0]
    if Lc:
        want[..., 1:Lc + 1] = dcode.permute(0, 2, 3, 1)
    y = torch.full((B, H, W, ldy), SENT, dtype=dt, device=gpu)
    dcg = dcode.to(gpu) if Lc else None
    L.call("zp_head_grad_to_nhwc", dmask.to(gpu).data_ptr(), L.ptr(dcg), B, Lc, H, W, ldy, L.dtype_code(dt),
           y.data_ptr(), L.stream_ptr())
    assert torch.equal(y.cpu(), want.to(dt))


def test_head_grad_to_nhwc_refuses_narrow_rows(gpu):
    from zebrapose_amd import _lib as L
    dmask = torch.zeros(1, 1, 2, 2, device=gpu)
    dcode = torch.zeros(1, 16, 2, 2, device=gpu)
    y = torch.full((1, 2, 2, 16), SENT, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(RuntimeError, match="bad args"):
        L.call("zp_head_grad_to_nhwc", dmask.data_ptr(), dcode.data_ptr(), 1, 16, 2, 2, 16, L.ZP_BF16, y.data_ptr(),
               L.stream_ptr())
    assert bool((y.cpu().float() == SENT).all())


# ------------------------------------------------------------------------------ zp_add_broadcast_hw
@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("C,ld,c0", [(20, 24, 2), (256, 1280, 1024)])
def test_add_broadcast_hw(gpu, prec, C, ld, c0, acc):
    """y[b, h, w, c0 + c] (+)= src[b, c] * mul against f64.  The f32 product and sum round once each,
    or once together when the compiler contracts them: half an ulp of the output at the reference
    plus 2^-22 (|src * mul| + |y|)."""
    from zebrapose_amd import _lib as L
    dt = DT[prec]
    torch.manual_seed(13)
    mul = np.float32(1.0 / (H * W))
    src = torch.randn(B, C).to(dt)
    y = torch.full((B, H, W, ld), SENT, dtype=dt)
    if acc:
        y[..., c0:c0 + C] = torch.randn(B, H, W, C).to(dt)
    prod = (src.double() * float(mul))[:, None, None, :].expand(B, H, W, C)
    y0 = y[..., c0:c0 + C].double() if acc else torch.zeros(B, H, W, C, dtype=torch.float64)
    ref = prod + y0
    yg = y.to(gpu)
    L.call("zp_add_broadcast_hw", src.to(gpu).data_ptr(), float(mul), B, C, L.dtype_code(dt), yg.data_ptr(), H, W, ld,
           c0, acc, L.stream_ptr())
    yc = yg.cpu()
    got = yc[..., c0:c0 + C].double()
    err = (got - ref).abs()
    bound = half_ulp(ref, dt) + 2.0 ** -22 * (prod.abs() + y0.abs())
    print(f"add_broadcast_hw {prec} C={C} acc={acc}: max err/bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    assert bool((got != SENT).all())
    assert sentinel_outside(yc, c0, C)


# --------------------------------------------------------------------------------------- zp_bn_fold
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("C", [1, 17, 256, 513])
def test_bn_fold(gpu, C, with_bias):
    """scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale against f64.  The f32
    scale takes four roundings (the add, halved by the root; the root; the divide; the multiply):
    rtol 4 * 2^-24.  The shift inherits them on its two products: 4 * 2^-24 of the terms' magnitudes."""
    from zebrapose_amd import _lib as L
    g = torch.Generator().manual_seed(14 + C)
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma[C // 2] = 0.0
    beta = torch.randn(C, generator=g) * 0.1
    mean = torch.randn(C, generator=g)
    var = torch.rand(C, generator=g) * (4 - 1e-3) + 1e-3
    bias = torch.randn(C, generator=g) if with_bias else None
    eps = np.float32(1e-5)
    scale = torch.full((C + 1,), SENT, device=gpu)  # one element past C: the tail block must stop at C
    shift = torch.full((C + 1,), SENT, device=gpu)
    dev = [t.to(gpu) for t in (gamma, beta, mean, var)]
    bg = bias.to(gpu) if with_bias else None
    L.call("zp_bn_fold", dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), L.ptr(bg),
           float(eps), C, scale.data_ptr(), shift.data_ptr(), L.stream_ptr())
    s_ref = gamma.double() / torch.sqrt(var.double() + float(eps))
    b64 = bias.double() if with_bias else torch.zeros(C, dtype=torch.float64)
    sh_ref = beta.double() + (b64 - mean.double()) * s_ref
    sc, shc = scale.cpu(), shift.cpu()
    assert float(sc[C]) == SENT and float(shc[C]) == SENT
    ds = (sc[:C].double() - s_ref).abs()
    dsh = (shc[:C].double() - sh_ref).abs()
    u = 4 * 2.0 ** -24
    sh_bound = u * (beta.double().abs() + (mean.double() * s_ref).abs() + (b64 * s_ref).abs())
    print(f"bn_fold C={C} bias={with_bias}: scale max rel {float((ds / s_ref.abs().clamp_min(1e-300)).max() / 2.0 ** -24):.3g} "
          f"x 2^-24, shift max err/bound {float((dsh / sh_bound).max()):.3g}")
    assert bool((ds <= u * s_ref.abs()).all())
    assert float(sc[C // 2]) == 0.0
    assert bool((dsh <= sh_bound).all())


# ----------------------------------------------------------------------------------- zp_mask_interp
LDY, CY0 = 24, 17


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", INTERP, ids=INTERP_IDS)
def test_mask_interp(gpu, case, prec):
    """F.interpolate(bilinear, align_corners=False) of the CPU in fp32, written into channel 17 of
    24.  Four products and three adds, contracted or not: half an ulp of the output at the reference
    + 4 * 2^-23 max|x|.  Where the size ratio is an integer every weight is 0, 0.25, 0.5 or 1: small
    integer inputs then give the exact result."""
    from zebrapose_amd import _lib as L
    ih, iw, oh, ow = case
    dt = DT[prec]
    torch.manual_seed(15)
    x = torch.randn(B, 1, ih, iw)
    inputs = [(x, False)]
    if prec == "fp32" and ih % oh == 0 and iw % ow == 0:
        inputs.append((torch.randint(-8, 9, (B, 1, ih, iw)).float(), True))
    for xin, exact in inputs:
        ref = F.interpolate(xin, (oh, ow), mode="bilinear", align_corners=False)[:, 0]
        y = torch.full((B, oh, ow, LDY), SENT, dtype=dt, device=gpu)
        L.call("zp_mask_interp", xin.to(gpu).data_ptr(), B, ih, iw, oh, ow, L.dtype_code(dt), y.data_ptr(), LDY, CY0,
               L.stream_ptr())
        yc = y.cpu()
        assert sentinel_outside(yc, CY0, 1)
        got = yc[..., CY0]
        if exact:
            assert torch.equal(got, ref)
            continue
        err = (got.double() - ref.double()).abs()
        bound = half_ulp(ref.double(), dt) + 4 * 2.0 ** -23 * float(xin.abs().max())
        print(f"mask_interp {case} {prec}: max err/bound {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all())


def _interp_bwd_ref(dy, ih, iw):
    """autograd of the fp32 CPU F.interpolate: dy [B, OH, OW] f32 -> dx [B, 1, ih, iw]"""
    x0 = torch.zeros(dy.shape[0], 1, ih, iw, requires_grad=True)
    F.interpolate(x0, tuple(dy.shape[1:]), mode="bilinear", align_corners=False).backward(dy[:, None])
    return x0.grad


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", INTERP, ids=INTERP_IDS)
def test_mask_interp_bwd(gpu, case, prec, acc):
    """The gather-form backward, dy [B, OH, OW] in channel 17 of 24 -> dx [B, 1, H, W] f32, against
    autograd of the CPU interpolate on the stored dy.  With A the same backward of |dy|, an element
    sums at most 64 products: |got - ref| <= 2^-18 A (+ 2^-23 |dx before| when accumulating).  Each
    output's weights sum to 1, so per image sum(dx) = sum(dy) to 1e-5 sum|dy|: a dropped or doubled
    border tap shows there even if one element hides it."""
    from zebrapose_amd import _lib as L
    ih, iw, oh, ow = case
    dt = DT[prec]
    torch.manual_seed(16)
    dyb = torch.randn(B, oh, ow, LDY).to(dt)
    dy = dyb[..., CY0].float()
    before = torch.randn(B, 1, ih, iw) if acc else torch.full((B, 1, ih, iw), SENT)
    ref = _interp_bwd_ref(dy, ih, iw).double()
    A = _interp_bwd_ref(dy.abs(), ih, iw).double()
    bound = 2.0 ** -18 * A
    if acc:
        ref = ref + before.double()
        bound = bound + 2.0 ** -23 * before.double().abs()
    dx = before.to(gpu)
    L.call("zp_mask_interp_bwd", dyb.to(gpu).data_ptr(), LDY, CY0, B, oh, ow, ih, iw, L.dtype_code(dt), dx.data_ptr(),
           acc, L.stream_ptr())
    got = dx.cpu().double()
    err = (got - ref).abs()
    print(f"mask_interp_bwd {case} {prec} acc={acc}: max err {float(err.max()):.3g}, "
          f"max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bound).all())
    moved = got - before.double() if acc else got
    s_dx = moved.sum(dim=(1, 2, 3))
    s_dy = dy.double().sum(dim=(1, 2))
    tol = 1e-5 * dy.double().abs().sum(dim=(1, 2))
    print(f"  per-image |sum dx - sum dy| / tol: {(s_dx - s_dy).abs().div(tol).tolist()}")
    assert bool(((s_dx - s_dy).abs() <= tol).all())


def test_mask_interp_bwd_refuses_fp16(gpu):
    from zebrapose_amd import _lib as L
    dy = torch.zeros(1, 2, 2, LDY, dtype=torch.float16, device=gpu)
    dx = torch.full((1, 1, 8, 8), SENT, device=gpu)
    with pytest.raises(RuntimeError, match="inference-only"):
        L.call("zp_mask_interp_bwd", dy.data_ptr(), LDY, CY0, 1, 2, 2, 8, 8, L.ZP_F16, dx.data_ptr(), 0,
               L.stream_ptr())
    assert bool((dx.cpu() == SENT).all())


# ------------------------------------------------------------------------------------- zp_threshold
def _threshold_input(n=777):
    k = np.float32(8.940696716308594e-08)  # zp_common.h kHalfLogit: CPU fp32 sigmoid(x) > 0.5 <=> x > kHalfLogit
    edge = np.array([0.0, -0.0, k, np.nextafter(k, np.float32(1)), np.nextafter(k, np.float32(-1)), np.inf, -np.inf,
                     np.nan, np.float32(1e-45), -np.float32(1e-45)], dtype=np.float32)
    want = np.array([0, 0, 0, 1, 0, 1, 0, 0, 0, 0], dtype=np.float64)
    x = np.random.default_rng(17).standard_normal(n).astype(np.float32)
    pos = np.linspace(0, n - 1, len(edge)).astype(int)  # spread over all four blocks, first and last lane included
    x[pos] = edge
    return x, pos, want


@pytest.mark.parametrize("out_f64", [0, 1], ids=["u8", "f64"])
def test_threshold_edges(gpu, out_f64):
    """bit = x > kHalfLogit at +-0, kHalfLogit and its two neighbours, +-inf, NaN and the smallest subnormals,
    exactly as oracle.ref_cpu.threshold_np; n = 777 ends in a partial block; n = 0 writes nothing."""
    from oracle import ref_cpu
    from zebrapose_amd import _lib as L
    x, pos, want_edge = _threshold_input()
    want = ref_cpu.threshold_np(x)
    assert np.array_equal(want[pos], want_edge)  # the oracle itself at the planted values
    n = x.size
    odt = torch.float64 if out_f64 else torch.uint8
    out = torch.full((n + 3,), 7, dtype=odt, device=gpu)
    xg = torch.from_numpy(x).to(gpu)
    L.call("zp_threshold", xg.data_ptr(), 0, out_f64, out.data_ptr(), L.stream_ptr())
    assert bool((out.cpu() == 7).all())
    L.call("zp_threshold", xg.data_ptr(), n, out_f64, out.data_ptr(), L.stream_ptr())
    oc = out.cpu().double().numpy()
    assert np.array_equal(oc[:n], want)
    assert np.all(oc[n:] == 7)
