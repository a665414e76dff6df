"""Tap-row trimming of the split-fp32 tile k_conv3 (csrc/zp_conv3.hip; ZP_CONV_FLAGS / zp_conv_tuning key 1,
bit 4) pinned to the exact reference of tests/conv_ref.py, straight through the C ABI, on ZP_F32H2 and
ZP_F32X3 operands.

The operands are small integers, so plane 0 of every split value holds it exactly, the other planes are
zero, every product and every partial sum is an integer below 2^24 and every stored value survives the
split store: a launch must equal the f64 reference BIT FOR BIT over the whole guarded output buffer (the
guards, the channels outside [cy0, cy0 + Cout)), with bit 4 off and with bit 4 on, and again on a second
launch.  `cfg` is (variant, cout tile, pixel tile) of zp_conv2d_config: a case that lands elsewhere fails as
wrongly sized.  tests/test_conv3_trim_host.py proves each case's exactness preconditions and the trimming
rule itself on the CPU.

  d12-c32 d12-c64 d18-c32 d18-c64   3x3 at 32 x 32, N 2, Cout 256: 128-pixel tiles of four rows, most of which
                                    drop one outer tap row (d18: the first and last four tiles of an image)
  d6-4x20-n3                        80-pixel images: every tile crosses an image boundary, nothing trimmed
  d18-33x32 d18-32x30               M = 1056 / 960, no multiple of 128 (a 32 x 32 image is 8 whole tiles, so
                                    the ragged cases take one more row / two fewer columns): the last tile
                                    is judged by its true last pixel
  d12-8x32                          both outer tap rows dead in every tile: 3 of 9 taps run
  aspp                              the merged four-sub launch (1 + 9 + 9 + 9 taps, four y slices) at 32 x 32,
                                    N 1, Cin 256; aspp-splitk: the same with the split-K workspace, which
                                    keeps its K ranges whole (equal bits under either flag)
  convT                             the four ConvT phases (1 / 2 / 2 / 4 taps)
  d1                                3x3 d1 at 32 x 32 (k_conv3s switched off): no tile has a dead row
  w-d12 w-d18 w-aspp                the 128 x 256 eight-wave tile the batch-32 ASPP launch runs on (key 8 = 0)
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import pytest

from tests import conv_ref as CR

pytestmark = pytest.mark.gpu

H2, X3 = "h2", "x3"
NPL = {H2: 2, X3: 3}
FLAGS_ON = 94 + 128 + 256          # conv_flags()'s default (csrc/zp_conv.hip)
FLAGS_OFF = FLAGS_ON & ~16


@dataclass(frozen=True)
class Case:
    id: str
    cfg: tuple             # (variant, tc, tp) the case is sized for
    N: int
    H: int
    W: int
    geo: tuple             # ("conv", k, s, p, d), ("convT",), ("aspp", d1, d2, d3)
    Cin: int
    Cout: int
    kw: dict = field(default_factory=dict)   # conv_ref.build's keywords
    tuning: tuple = ()     # zp_conv_tuning (key, value) pairs for the launch
    splitk: bool = False   # with the split-K workspace (zp_conv2d_split_ws)

    def host(self, form, seed=0):
        """conv_ref's host build (an f32 case) turned into a split-dtype call"""
        from zebrapose_amd import geometry as G
        from zebrapose_amd import _lib as L
        H, W, ci, co, g = self.H, self.W, self.Cin, self.Cout, self.geo
        kw = dict(self.kw)
        if g[0] == "conv":
            k, s, p, d = g[1:]
            plan, weights = G.conv_fwd(H, W, k, s, p, d), [(0, (co, ci, k, k), 0)]
        elif g[0] == "convT":
            plan, weights = G.convT_fwd(H, W), [(0, (ci, co, 3, 3), 1)] * 4
        else:
            plans = [G.conv_fwd(H, W, 1, 1, 0, 1)] + [G.conv_fwd(H, W, 3, 1, d, d) for d in g[1:]]
            plan = G.Plan(H, W, 1, [p.subs[0] for p in plans])
            weights = [(i, (co, ci, k, k), 0) for i, k in enumerate((1, 3, 3, 3))]
            kw.setdefault("cy0", [i * co for i in range(4)])
        b = CR.build(CR.F32, self.N, H, W, plan, ci, co, weights=weights, seed=seed, **kw)
        b.a.dtype = {H2: L.ZP_F32H2, X3: L.ZP_F32X3}[form]
        b.store = "planes"
        return b, plan, weights


def dil(d):
    return ("conv", 3, 1, d, d)


P64, P128 = (4, 64, 128), (4, 128, 128)
OFF8 = dict(cy0=4, ldy=264)        # a y slice off the 8-channel grid: k_conv3's tiles, channels either side
ASPP_KW = dict(wdraw="half", relu=1, scale=True, shift=True)
CASES = [
    Case("d12-c32", P64, 2, 32, 32, dil(12), 32, 256, OFF8),
    Case("d12-c64", P64, 2, 32, 32, dil(12), 64, 256, OFF8),
    Case("d18-c32", P64, 2, 32, 32, dil(18), 32, 256, OFF8),
    Case("d18-c64", P64, 2, 32, 32, dil(18), 64, 256, OFF8),
    Case("d6-4x20-n3", P64, 3, 4, 20, dil(6), 64, 64),
    Case("d18-33x32", P64, 1, 33, 32, dil(18), 32, 256, OFF8),
    Case("d18-32x30", P64, 1, 32, 30, dil(18), 32, 256, OFF8),
    Case("d12-8x32", P64, 2, 8, 32, dil(12), 64, 256, OFF8),
    Case("aspp", P64, 1, 32, 32, ("aspp", 6, 12, 18), 256, 256, ASPP_KW),
    Case("aspp-splitk", P64, 1, 32, 32, ("aspp", 6, 12, 18), 256, 256, ASPP_KW, splitk=True),
    Case("convT", P64, 2, 8, 32, ("convT",), 64, 256, dict(cy0=4, ldy=264)),
    Case("d1", P64, 1, 32, 32, ("conv", 3, 1, 1, 1), 64, 256, dict(OFF8, res=True, cr0=4, ldr=264), ((7, 0),)),
    Case("w-d12", (4, 128, 256), 2, 32, 32, dil(12), 64, 256, OFF8, ((8, 0),)),
    Case("w-d18", (4, 128, 256), 2, 32, 32, dil(18), 32, 256, OFF8, ((8, 0),)),
    Case("w-aspp", (4, 128, 256), 2, 32, 32, ("aspp", 6, 12, 18), 64, 256, ASPP_KW, ((8, 0),)),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
PARAMS = [pytest.param(c, f, id=f"{c.id}-{f}") for c in CASES for f in (H2, X3)]


def tuned(kvs):
    from tests.test_gpu_conv_edges import tuned as t
    return t(kvs)


def plane_words(v, form):
    """split planes [NPL][...] (16-bit words) of values whose plane 0 holds them exactly: integers below 256
    (bf16) / 2048 (fp16), the other planes zero; NaN (outside a slice) in every plane"""
    v = np.asarray(v, np.float64)
    if form == X3:
        w0 = (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        back = (w0.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    else:
        h = v.astype(np.float16)
        w0, back = h.view(np.uint16), h.astype(np.float64)
    nan = np.isnan(v)
    assert (back[~nan] == v[~nan]).all(), "a value is off plane 0's grid"
    out = np.zeros((NPL[form],) + v.shape, np.uint16)
    out[0] = w0
    out[:, nan] = w0[nan]
    return out.view(np.int16)


def join_words(words, form):
    return CR.join_planes(np.asarray(words).view(np.uint16), CR.X3 if form == X3 else CR.H2)


def upload(c, form, device):
    """the case on the device: guarded planes of x, the packed weights, the residual and y (-> Built)"""
    import torch
    from zebrapose_amd import _lib as L
    b, plan, weights = c.host(form)
    a, npl = b.a, NPL[form]
    i16 = torch.int16
    b.dev["device"] = device
    a.x = b.guarded("x", plane_words(b.x, form), i16)
    packed = {}
    for i, ((idx, shape, tr), sb) in enumerate(zip(weights, plan.subs)):
        key = (idx, tuple(sb.taps))
        if key not in packed:
            src = torch.from_numpy(b.subs[i][0].astype(np.float32)).to(device)
            b.keep.append(src)
            dst = b.guarded(f"w{i}", np.full(npl * a.w_rows * a.k_pad, CR.GARBAGE_WORD, np.int16), i16)
            ky, kx = [t[0] for t in sb.taps], [t[1] for t in sb.taps]
            rc = L.lib.zp_pack_weight(src.data_ptr(), shape[0], shape[1], shape[2], shape[3], tr, len(sb.taps),
                                      (C.c_int * len(ky))(*ky), (C.c_int * len(kx))(*kx), a.Cin, a.dtype, dst,
                                      a.w_rows, a.k_pad, L.stream_ptr())
            assert rc == 0, L.lib.zp_last_error()
            torch.cuda.synchronize()
            b.dev[f"w{i}@"] = b.dev[f"w{i}"].cpu()  # as packed: an input from here on
            packed[key] = dst
        a.sub[i].w = packed[key]
        if b.scale[i] is not None:
            a.sub[i].scale = b.guarded(f"scale{i}", b.scale[i])
        if b.shift[i] is not None:
            a.sub[i].shift = b.guarded(f"shift{i}", b.shift[i])
    if b.res is not None:
        a.res = b.guarded("res", plane_words(b.res, form), i16)
    ny = npl * int(np.prod(b.y_shape()))
    y = b.guarded("y", np.full(ny, CR.GARBAGE_WORD, np.int16), i16)
    for i in range(a.nsub):
        a.sub[i].y = y
    nb = int(L.lib.zp_conv2d_split_ws(C.byref(a)))
    if c.splitk:
        assert nb > 0, f"{c.id}: sized for split-K, the plan takes one slice"
        a.stats = b.guarded("stats", np.full(nb // 4, CR.GARBAGE))
    return b


def check_plan(c, b):
    got = b.config()[:3]
    assert got == c.cfg, f"{c.id}: sized for (variant, tc, tp) {c.cfg}, the plan takes {got}"


def compare(b, form):
    """the guarded y planes against the reference, bit for bit -> (problems, the words read)"""
    bad = []
    want, written = b.want()
    words, ok = b.read("y", (NPL[form],) + want.shape)
    if not ok:
        bad.append("y: a guard was overwritten")
    got = join_words(words, form)
    w32 = want.astype(np.float32)
    ne = got[written].view(np.uint32) != w32[written].view(np.uint32)
    if ne.any():
        idx = np.argwhere(got.view(np.uint32) != np.where(written, w32, got).view(np.uint32))
        bad.append(f"y: {int(ne.sum())} of {ne.size} values differ; first {idx[:5].tolist()}, got "
                   f"{[float(got[tuple(i)]) for i in idx[:5]]}, want {[float(want[tuple(i)]) for i in idx[:5]]}")
    if (words[:, ~written].view(np.uint16) != CR.GARBAGE_WORD).any():
        bad.append("y: a word outside the written channels changed")
    if not b.inputs_intact():
        bad.append("an input buffer or its guard changed")
    return bad, words.copy()


@pytest.mark.parametrize("c,form", PARAMS)
def test_trim_exact(gpu, c, form):
    """(a) the reference bit for bit, (b) equal bits with bit 4 off and on, (c) equal bits on a second launch"""
    runs = {}
    with tuned(c.tuning):
        b = upload(c, form, gpu)
        check_plan(c, b)
        for name, flags in (("off", FLAGS_OFF), ("on", FLAGS_ON), ("on again", FLAGS_ON)):
            with tuned(((1, flags),)):
                rc = b.launch()
            assert rc == 0, (c.id, name, rc)
            runs[name] = compare(b, form)
    print(f"{c.id}-{form}: cfg {c.cfg}, M {b.M}, split-K workspace {'yes' if c.splitk else 'no'}")
    for name, (bad, _) in runs.items():
        assert not bad, f"{c.id}-{form}, bit 4 {name}: " + "; ".join(bad)
    assert (runs["off"][1] == runs["on"][1]).all(), f"{c.id}-{form}: bit 4 off and on differ"
    assert (runs["on"][1] == runs["on again"][1]).all(), f"{c.id}-{form}: two launches differ"
