"""The preconditions of tests/test_gpu_conv3_trim.py and k_conv3's tap-row trimming rule, on the CPU.

For every case and both split forms, on the actual draw: x, the weights and the residual are integers that
plane 0 of the split holds exactly (below 256 for ZP_F32X3's bf16, below 2048 for ZP_F32H2's fp16), so the
other planes -- and with them every correction product -- are zero; every sum |w| |x| (times |scale|, plus
shift and residual) stays below 2^24, so the hi * hi products and every partial sum in any order are exact
in f32; every stored value comes back exactly from its split store; and the kernel zp_conv2d_config names
is the one the case is sized for (the plan without a device assumes the MI355X's 256 compute units).

The rule (csrc/zp_conv3.hip, restated here from its comment): a tile inside one image walks tap rows
[qlo, qhi], the rows q for which some row of the tile reads inside [0, IH), judged from the tile's first and
last pixel alone.  trim_range must never drop a tap row that holds a valid tap for any pixel of the tile
(brute force over the pixels), must leave tiles that span two images alone, and gives the tap counts the
case table names."""
import ctypes as C

import numpy as np
import pytest

from tests import conv_ref as CR
from tests import test_gpu_conv3_trim as T
from tests.test_gpu_conv3_trim import H2, X3


def trim_range(p0, tp, M, GH, GW, sy, IH, ty0, dty, ny):
    """(qlo, qhi) of the tile [p0, p0 + tp): k_conv3's scalar test"""
    if ny <= 1:
        return 0, ny - 1
    ghw, mlast = GH * GW, min(p0 + tp, M) - 1
    n0, n1 = p0 // ghw, mlast // ghw
    if n0 != n1:
        return 0, ny - 1
    ya, yb = (p0 - n0 * ghw) // GW * sy, (mlast - n1 * ghw) // GW * sy
    live = [q for q in range(ny) if yb + ty0 + q * dty >= 0 and ya + ty0 + q * dty <= IH - 1]
    return (live[0], live[-1]) if live else (0, ny - 1)


def tap_rows(S):
    """(ny, nx, ty0, dty) of a sub's tap grid, rows outer (conv3_launch)"""
    nx = 1
    while nx < S.ntaps and S.ty[nx] == S.ty[0]:
        nx += 1
    ny = S.ntaps // nx
    assert ny * nx == S.ntaps
    return ny, nx, int(S.ty[0]), (int(S.ty[nx]) - int(S.ty[0])) if ny > 1 else 0


def taps_run(c):
    """per sub, the taps each tile walks under the rule; every dropped row checked dead pixel by pixel"""
    b, _, _ = c.host(H2)
    a, tp = b.a, c.cfg[2]
    out = []
    for s in range(a.nsub):
        ny, nx, ty0, dty = tap_rows(a.sub[s])
        per_tile = []
        for p0 in range(0, b.M, tp):
            qlo, qhi = trim_range(p0, tp, b.M, a.GH, a.GW, a.sy, a.IH, ty0, dty, ny)
            pix = np.arange(p0, min(p0 + tp, b.M))
            y0 = (pix % (a.GH * a.GW)) // a.GW * a.sy
            for q in list(range(qlo)) + list(range(qhi + 1, ny)):
                iy = y0 + ty0 + q * dty
                assert ((iy < 0) | (iy >= a.IH)).all(), f"{c.id}: tile {p0} drops live tap row {q} of sub {s}"
            per_tile.append((qhi - qlo + 1) * nx)
        out.append(per_tile)
    return out


@pytest.mark.parametrize("c", T.CASES, ids=[c.id for c in T.CASES])
def test_rule_is_conservative(c):
    taps_run(c)


def test_rule_tap_counts():
    run = {i: taps_run(T.BY_ID[i]) for i in ("d12-c64", "d18-c32", "d6-4x20-n3", "d12-8x32", "d1", "d18-33x32",
                                            "aspp", "w-aspp", "convT")}
    # 32 x 32, four-row tiles: dy = -d is live from the tile whose last row reaches d, dy = +d mirrored
    assert run["d12-c64"][0] == [6, 6, 6, 9, 9, 6, 6, 6] * 2
    assert run["d18-c32"][0] == [6, 6, 6, 6, 6, 6, 6, 6] * 2
    assert run["d6-4x20-n3"][0] == [9, 9]                    # both tiles span two images
    assert run["d12-8x32"][0] == [3] * 4
    assert run["d1"][0] == [9] * 8                           # every tile reads a row of the image at dy = +-1
    assert run["d18-33x32"][0] == [6, 6, 6, 6, 6, 6, 6, 6, 6]  # the ragged tile (row 32): dy = +18 dead
    assert run["aspp"] == [[1] * 8, [6] + [9] * 6 + [6], [6, 6, 6, 9, 9, 6, 6, 6], [6] * 8]
    # eight-row tiles (the batch-32 launch): 1 + 9 + 7.5 + 6 = 23.5 of 28 taps on average
    assert run["w-aspp"] == [[1] * 8, [9] * 8, [6, 9, 9, 6] * 2, [6] * 8]
    # ConvT phases (tap rows 0 and +1): a four-row tile always holds a row that reads row + 1 inside
    assert run["convT"] == [[1] * 4, [2] * 4, [2] * 4, [4] * 4]


@pytest.mark.parametrize("c,form", T.PARAMS)
def test_case_preconditions(c, form):
    with T.tuned(c.tuning):
        b, _, _ = c.host(form)
        T.check_plan(c, b)
        if c.splitk:
            from zebrapose_amd import _lib as L
            assert L.lib.zp_conv2d_split_ws(C.byref(b.a)) > 0
    a = b.a
    lim = 256 if form == X3 else 2048
    xin = b.x[..., a.cx0:a.cx0 + a.Cin]
    assert np.isfinite(xin).all() and (xin != 0).all() and np.isnan(b.x).sum() == b.x.size - xin.size
    assert (xin == np.rint(xin)).all() and np.abs(xin).max() < lim
    T.plane_words(b.x, form)
    rmax = 0
    if b.res is not None:
        rin = b.res[..., a.cr0:a.cr0 + a.Cout]
        assert np.isnan(b.res).sum() == b.res.size - rin.size and (rin == np.rint(rin)).all()
        rmax = np.abs(rin).max()
        assert rmax < lim
    assert a.Cin % 32 == 0 and a.k_pad % 32 == 0 and a.cx0 % 8 == 0 and a.ldx % 8 == 0
    for s in range(a.nsub):
        w = b.subs[s][0]
        assert (w == np.rint(w)).all() and np.abs(w).max() < 32      # (ZP_F32H2's weight bound, zp.h)
        top = b.acc(s, absolute=True)
        if b.scale[s] is not None:
            top = top * np.abs(b.scale[s])
        top = top + (0 if b.shift[s] is None else np.abs(b.shift[s])) + rmax
        assert top.max() < 2 ** 24, (c.id, top.max())
        v = b.values(s)
        assert np.abs(v).max() > 0 and np.abs(v).max() < 65504
        # the split store and its join give the value back
        v32 = v.astype(np.float32)
        if form == X3:
            hi = CR.to_store(v32, CR.BF16)
            mid = CR.to_store(v32 - hi, CR.BF16)
            lo = CR.to_store(v32 - hi - mid, CR.BF16)
            words = np.stack([(p.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16) for p in (hi, mid, lo)])
        else:
            h = v32.astype(np.float16)
            words = np.stack([h.view(np.uint16),
                              ((v32 - h.astype(np.float32)) * 2048).astype(np.float16).view(np.uint16)])
        assert (T.join_words(words, form) == v32).all(), f"{c.id}-{form}: a stored value does not survive the split"
    assert b.M <= 2048
