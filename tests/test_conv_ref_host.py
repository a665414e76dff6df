"""tests/conv_ref.py validated on the CPU, and the preconditions of tests/test_gpu_conv_edges.py.

The reference against torch's f64 F.conv2d / F.conv_transpose2d on random real operands, to 1e-12
relative: strides 1 and 2, dilations, kernels 1 / 3 / 7, non-square images, channel slices, the epilogue;
the four-phase ConvT plan; the merged ASPP launch; and the data-gradient plans against autograd's dx on
every geometry family the GPU cases use.

For every entry of the GPU case table, on the actual draw: every sum |w| |x| (plus shift and residual)
stays below 2^24, so any order of summation is exact in f32; every stored value is on the stored type's
grid and, for a 16-bit store, below 256 (bf16) / 2048 (fp16), where one lost product moves it by at
least one ulp; x and the residual hold NaN outside their slices; and the kernel zp_conv2d_config names
is the one the case is sized for (the plan without a device assumes the MI355X's 256 compute units)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as CR
from tests import test_gpu_conv_edges as T
from tests.conv_ref import BF16, F16, F32
from tests.test_gpu_conv_edges import Case


def _nchw(v):
    return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.detach().numpy().transpose(0, 2, 3, 1)


def _close(got, want):
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def _real(c, **kw):
    return c.build(xdraw="real", wdraw="real", **kw)


def _dense(b):
    """the whole output image [N][OH][OW][Cout] of a one-slice launch, zeros where nothing is written"""
    out = np.zeros((b.a.N, b.OH, b.OW, b.a.Cout))
    for s in range(b.a.nsub):
        oy, ox = b.out_pixels(s)
        out[:, oy, ox] += b.values(s)
    return out


CONVS = [  # k, s, p, d, H, W
    (1, 1, 0, 1, 5, 7), (3, 1, 1, 1, 6, 9), (3, 2, 1, 1, 7, 10), (3, 1, 6, 6, 9, 14), (7, 2, 3, 1, 13, 18),
    (1, 2, 0, 1, 9, 11), (3, 1, 12, 12, 16, 16),
]
IDS = [f"k{c[0]}s{c[1]}p{c[2]}d{c[3]}-{c[4]}x{c[5]}" for c in CONVS]


@pytest.mark.parametrize("k,s,p,d,H,W", CONVS, ids=IDS)
def test_ref_is_conv2d(k, s, p, d, H, W):
    c = Case("t", None, F32, 2, H, W, ("conv", k, s, p, d), 8, 6,
             dict(cx0=4, ldx=16, cy0=4, ldy=12, res=True, cr0=4, ldr=12, relu=1, scale=True, shift=True))
    b = _real(c, seed=k + s)
    w = torch.from_numpy(b.subs[0][0])
    y = F.conv2d(_nchw(b.x[..., 4:12]), w, None, s, p, d)
    y = y * torch.from_numpy(b.scale[0])[None, :, None, None] + torch.from_numpy(b.shift[0])[None, :, None, None]
    y = torch.relu(y + _nchw(b.res[..., 4:10]))
    _close(b.values(0), _nhwc(y))
    full = b.want()  # (rounded once to the stored f32)
    assert (full[..., 4:10] == _nhwc(y).astype(np.float32)).all()
    assert (full[..., :4] == CR.GARBAGE).all() and (full[..., 10:] == CR.GARBAGE).all()


def test_ref_is_conv_transpose2d_by_phases():
    b = _real(Case("t", None, F32, 2, 5, 9, ("convT",), 8, 6), seed=1)
    assert b.a.nsub == 4 and (b.OH, b.OW) == (10, 18)
    y = F.conv_transpose2d(_nchw(b.x), torch.from_numpy(b.subs[0][0]), None, 2, 1, 1)
    _close(_dense(b), _nhwc(y))
    assert (b.want() != CR.GARBAGE).all()  # the four phases write every pixel


def test_ref_is_merged_aspp():
    b = _real(Case("t", None, F32, 2, 9, 13, ("aspp", 2, 4, 6), 8, 4), seed=2)
    full = b.want()
    for s, (k, d) in enumerate(((1, 1), (3, 2), (3, 4), (3, 6))):
        y = F.conv2d(_nchw(b.x), torch.from_numpy(b.subs[s][0]), None, 1, 0 if k == 1 else d, d)
        _close(b.values(s), _nhwc(y))
        assert (full[..., 4 * s:4 * s + 4] == b.stored(s)).all()


DGRADS = [(3, 1, 1, 1, 6, 10), (3, 2, 1, 1, 8, 12), (1, 2, 0, 1, 8, 12), (7, 1, 3, 1, 8, 5), (3, 1, 6, 6, 9, 14)]


@pytest.mark.parametrize("k,s,p,d,H,W", DGRADS, ids=[f"k{c[0]}s{c[1]}p{c[2]}d{c[3]}-{c[4]}x{c[5]}" for c in DGRADS])
def test_dgrad_plan_is_autograd_dx(k, s, p, d, H, W):
    """conv_dgrad over dy with the transposed packing: autograd's dx, zero where no phase writes"""
    ci, co = 6, 8                        # of the forward conv; the launch reads co channels, writes ci
    b = _real(Case("t", None, F32, 2, H, W, ("dgrad", k, s, p, d), co, ci), seed=k)
    x = torch.zeros(2, ci, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, torch.from_numpy(b.subs[0][0]), None, s, p, d).backward(_nchw(b.x))
    _close(_dense(b), _nhwc(x.grad))
    if (k, s) == (1, 2):                 # three of the four phases have no taps: their pixels stay as found
        full = b.want()
        assert b.a.nsub == 1 and (full[:, 1::2] == CR.GARBAGE).all() and (full[:, :, 1::2] == CR.GARBAGE).all()


def test_convT_dgrad_plan_is_autograd_dx():
    ct_in, ct_out = 6, 8
    b = _real(Case("t", None, F32, 2, 5, 9, ("convT_dgrad",), ct_out, ct_in), seed=3)
    assert b.x.shape[1:3] == (10, 18) and b.a.sy == 2
    x = torch.zeros(2, ct_in, 5, 9, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(x, torch.from_numpy(b.subs[0][0]), None, 2, 1, 1).backward(_nchw(b.x))
    _close(_dense(b), _nhwc(x.grad))


def test_join_planes():
    v = np.array([0.0, 1.0, -3.0, 4097.0, -65503.0, 12345.0], np.float32)
    hi = CR.to_store(v, BF16)
    mid = CR.to_store(v - hi, BF16)
    lo = CR.to_store(v - hi - mid, BF16)
    w3 = np.stack([(p.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16) for p in (hi, mid, lo)])
    assert (CR.join_planes(w3, CR.X3) == v).all()
    h = v.astype(np.float16)
    w2 = np.stack([h.view(np.uint16), ((v - h.astype(np.float32)) * 2048).astype(np.float16).view(np.uint16)])
    assert (CR.join_planes(w2, CR.H2) == v).all()


ALL = (T.CASES + T.REAL_CASES + T.STAT_CASES + T.BNR_CASES + [T.HEAD_CASE]
       + [c for _, cs in T.ENV_RUNS for c in cs])
PLANNED = {c.id for c in T.CASES + T.REAL_CASES + T.STAT_CASES + T.BNR_CASES}


@pytest.mark.parametrize("c", ALL, ids=[c.id for c in ALL])
def test_case_preconditions(c):
    with T.tuned(c.tuning):
        b = c.build()
        if c.id in PLANNED:  # (the environment's cases are planned in their own process)
            T.check_plan(c, b)
    a, E = b.a, CR.chunk(c.dtype)
    xin = b.x[..., a.cx0:a.cx0 + a.Cin]
    assert np.isfinite(xin).all() and (xin != 0).all() and np.isnan(b.x).sum() == b.x.size - xin.size
    assert a.Cin % E == 0 and a.cx0 % E == 0 and a.ldx % E == 0
    if b.res is not None:
        rin = b.res[..., a.cr0:a.cr0 + a.Cout]
        assert np.isfinite(rin).all() and np.isnan(b.res).sum() == b.res.size - rin.size
    if c.kw.get("xdraw") == "real":
        return
    wide = [k for k in ("xdraw", "wdraw") if c.kw.get(k) == "wide"]
    assert len(wide) <= 1 and (c.dtype == F32 or not wide), "a 12-bit operand: f32 only, on one side"
    assert c.dtype != F32 or wide or a.out_mode in (CR.X3, CR.H2)
    for s in range(a.nsub):
        w = b.subs[s][0]
        assert (w == np.rint(w)).all() and (xin == np.rint(xin)).all()
        top = b.acc(s, absolute=True)
        if b.scale[s] is not None:
            top = top * np.abs(b.scale[s])
        top = top + (0 if b.shift[s] is None else np.abs(b.shift[s])) + (0 if b.res is None else 3)
        assert top.max() < 2 ** 24, (c.id, top.max())
        v = b.values(s)
        store = F32 if b.store == "planes" else b.store
        assert (CR.to_store(v, store) == v).all(), f"{c.id}: a stored value is off the {store} grid"
        if store in CR.EXACT_BELOW:
            assert np.abs(v).max() < CR.EXACT_BELOW[store], (c.id, np.abs(v).max())
        if a.out_mode == CR.H2:
            assert np.abs(v).max() < 2048 * 2048 and np.abs(v).max() < 65504
        assert np.abs(v).max() > 0
    if c.kw.get("bnr"):
        for s in range(a.nsub):
            g, gx = b.bnr_terms(s)
            assert np.abs(g).sum(0).max() < 2 ** 24 and np.abs(gx).sum(0).max() < 2 ** 24
            assert (gx == gx.astype(np.float32)).all() and (g != 0).any() and (g == 0).any()
    if c.dtype == F32:
        assert b.M <= 2048


def test_head_reference_is_exact():
    b = T.HEAD_CASE.build()
    for hcout in (17, 32):
        _, mask, code = T.head_args(b, hcout)
        out = np.concatenate([mask, code], 1)
        assert (out == np.rint(out)).all() and np.abs(out).max() < 2 ** 24
        assert 256 * 255 + 32 * 3 + 8 < 2 ** 24  # every partial sum of |hw| |feature|, plus the bias
