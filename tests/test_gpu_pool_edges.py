"""zp_maxpool3s2 and zp_maxpool3s2_bwd (csrc/zp_pool.hip) pinned to tests/pool_ref.py bit for bit, straight
through the C ABI.  pool_ref is torch's CPU max_pool2d rule (tests/test_pool_ref_host.py holds it to torch):
first maximum in (ky, kx) order, NaN takes over, a window of -inf alone sends its gradient to its first
in-bounds tap; the backward adds in f32 in (oy, ox) order, then the existing dx, and rounds once.

x, y, dy and dx are channel slices of wider buffers with different ld / c0 each; outside its slice x holds
NaN and the others a canary, and the whole buffer must come back as the reference says.  Words are compared
as uint16 / uint32, NaNs as NaN-ness.  The split forms (ZP_F32X3 / ZP_F32H2, forward only) are given as
planes; the expected planes are the split of the maximum of the joined values (tests/pack_ref.py)."""
import numpy as np
import pytest

from tests import pack_ref as P
from tests import pool_ref as R

pytestmark = pytest.mark.gpu

# 7..10 cross the backward's chunk of MP_ROWS = 4 block rows (8 input rows); 1 and 2 have no interior
EXTENTS = [(1, 1), (1, 4), (2, 3), (3, 2), (4, 5), (5, 7), (7, 8), (8, 9), (9, 10), (10, 17), (17, 1), (17, 9)]
CANARY = 777.0
B = 2


def vec(kind):
    return 4 if kind == "f32" else 8


def encode(v, kind):
    """f32 values -> stored words ([NPL][...] for the split forms)"""
    return P.store(np.asarray(v, np.float32), P.DTYPES[kind])


def decode(w, kind):
    if kind == "f32":
        return w.view(np.float32)
    if kind == "bf16":
        return P.bf16_value(w)
    if kind == "f16":
        return P.f16_value(w)
    return P.join3(w) if kind == "x3" else P.join2(w)


def on_grid(v, kind):
    return decode(encode(v, kind), kind)


def assert_words(got, want, kind, what):
    """bit for bit; a NaN (plane 0 of a split form) against any NaN"""
    lead = kind in ("x3", "h2")
    gv = decode(got[:1] if lead else got, "bf16" if kind == "x3" else "f16" if kind == "h2" else kind)
    wv = decode(want[:1] if lead else want, "bf16" if kind == "x3" else "f16" if kind == "h2" else kind)
    gn, wn = np.isnan(gv), np.isnan(wv)
    assert np.array_equal(gn, wn), (what, "NaN-ness", int((gn != wn).sum()))
    skip = np.zeros(got.shape, bool)
    if lead:
        skip[:1] = wn
    else:
        skip = wn
    bad = np.argwhere((got != want) & ~skip)
    assert bad.shape[0] == 0, (what, f"{bad.shape[0]} words differ", bad[:5].tolist(),
                               [hex(got[tuple(i)]) for i in bad[:5]], [hex(want[tuple(i)]) for i in bad[:5]])


def upload(words, device):
    import torch
    s = {2: np.int16, 4: np.int32}[words.dtype.itemsize]
    return torch.from_numpy(np.ascontiguousarray(words).view(s)).to(device)


def download(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def sliced(shape4, ld, c0, inner, fill, kind):
    """words of a [B][H][W][ld] buffer of `fill` with `inner` ([B][H][W][C] f32, or None) at channel c0"""
    b, h, w, c = shape4
    full = np.full((b, h, w, ld), fill, np.float32)
    if inner is not None:
        full[..., c0:c0 + c] = inner
    return encode(full, kind)


@pytest.mark.parametrize("ih,iw", EXTENTS)
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16", "x3", "h2"])
def test_maxpool_forward(gpu, kind, ih, iw):
    import torch
    from zebrapose_amd import _lib as L
    N = vec(kind)
    oh, ow = R.out_size(ih), R.out_size(iw)
    for C in (N, 3 * N):
        ldx, cx0, ldy, cy0 = C + 2 * N, N, C + N, N
        x = R.edge_input(B, ih, iw, C, seed=ih * 31 + iw + C)
        xw = sliced((B, ih, iw, C), ldx, cx0, x, np.nan, kind)
        y, _ = R.forward(decode(xw, kind)[..., cx0:cx0 + C])   # of the values as the kernel reads them
        want = sliced((B, oh, ow, C), ldy, cy0, y, CANARY, kind)
        xd, yd = upload(xw, gpu), upload(sliced((B, oh, ow, C), ldy, cy0, None, CANARY, kind), gpu)
        L.call("zp_maxpool3s2", xd.data_ptr(), B, ih, iw, ldx, cx0, C, P.DTYPES[kind], yd.data_ptr(), oh, ow, ldy, cy0,
               L.stream_ptr())
        torch.cuda.synchronize()
        assert_words(download(yd, want), want, kind, ("forward", kind, ih, iw, C))
        assert_words(download(xd, xw), xw, kind, ("forward input", kind, ih, iw, C))


@pytest.mark.parametrize("ih,iw", EXTENTS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_maxpool_backward(gpu, kind, accumulate, ih, iw):
    import torch
    from zebrapose_amd import _lib as L
    N = vec(kind)
    oh, ow = R.out_size(ih), R.out_size(iw)
    for C in (N, 3 * N):
        ldx, cx0, lddy, cdy0, lddx, cdx0 = C + 2 * N, N, C + N, 0, C + 3 * N, 2 * N
        rng = np.random.default_rng(ih * 131 + iw * 7 + C + accumulate)
        x = R.edge_input(B, ih, iw, C, seed=ih * 31 + iw + C)
        dy = on_grid(rng.standard_normal((B, oh, ow, C)), kind)
        old = on_grid(rng.standard_normal((B, ih, iw, C)), kind) if accumulate else np.full(x.shape, CANARY, np.float32)
        xw = sliced(x.shape, ldx, cx0, x, np.nan, kind)
        dyw = sliced(dy.shape, lddy, cdy0, dy, np.nan, kind)
        dxw = sliced(x.shape, lddx, cdx0, old, CANARY, kind)
        want = sliced(x.shape, lddx, cdx0, R.backward(x, dy, old if accumulate else None), CANARY, kind)
        xd, dyd, dxd = upload(xw, gpu), upload(dyw, gpu), upload(dxw, gpu)
        L.call("zp_maxpool3s2_bwd", xd.data_ptr(), ldx, cx0, dyd.data_ptr(), lddy, cdy0, B, ih, iw, C, oh, ow,
               P.DTYPES[kind], dxd.data_ptr(), lddx, cdx0, accumulate, L.stream_ptr())
        torch.cuda.synchronize()
        assert_words(download(dxd, want), want, kind, ("backward", kind, accumulate, ih, iw, C))
        assert_words(download(xd, xw), xw, kind, "backward x")
        assert_words(download(dyd, dyw), dyw, kind, "backward dy")
