"""zp_conv2d (csrc/zp_conv.hip) pinned to an exact reference at its edges, straight through the C ABI.

The operands are small integers (tests/conv_ref.py), so every partial sum is an integer below 2^24 and
exact in f32 in any order: each launch must equal the f64 reference BIT FOR BIT over the whole guarded
output buffer -- the guards, the channels outside [cy0, cy0 + Cout), the pixels the plan does not
write --, twice over with equal bits, on the kernel the case is sized for: `cfg` is (variant, cout tile,
pixel tile, ring stages) of zp_conv2d_config, and a case that lands elsewhere fails as wrongly sized.
tests/test_conv_ref_host.py proves each case's exactness preconditions on the CPU.

  k_conv tile (variant 0)
    t-m1 t-m129 t-m257          a ragged last pixel tile on the 128- and 256-pixel tiles; Cout 136: a
                                partial second channel tile
    t-gw15-n3                   tiles crossing rows and images off a power of two; Cin 128, Cout 72
    t-cout17                    the 32-channel tile on its 2-stage ring; Cin 320
    t-slice-a t-slice-b         x, y and the residual as channel slices, 8- and 4-aligned
    t-s2-3x3 t-s2-1x1           stride 2 on an odd image
    t-dil6                      3x3 d6 on a 4 x 20 grid: most taps read padding
    t-dil12 t-dil18             32 x 32, 8-row tiles whose padding-only tap rows are trimmed
    t-convT                     the four ConvT phases (1 / 2 / 2 / 4 taps)
    t-dgrad-*                   the data-gradient plans of a stride-1 3x3, a stride-2 3x3, a stride-2
                                1x1 (the phases without taps leave their pixels as found) and a ConvT
    t-aspp                      the merged ASPP launch: four subs with 1 and 9 taps, four y slices
    t-tc256-1 t-tc256-4         the 256-channel tile under zp_conv_tuning(0, 0), one and four subs
    t-near-*                    near-misses of the strip rule that must stay on the tile
    t-key2-off t-quad-off       strip / quad geometry with the kernel switched off or left at its
                                default threshold: the tile, the same bits (test_same_bits)
  small-Cin form
    s-cin8-7x7 s-cin16 s-cin24 s-kpad f32-s-cin8
  k_conv_strip / k_conv_strip2 (variants 1 / 2; DMA forms through zp_conv_tuning(1, flags))
    st-8x32 st-4x64 st-2x128, st-d4-w32 st-d8-w64 st-d16-w128 (the largest padding that fits),
    st-16x32-n3 (halos between tiles and images), st-c128 st-c192 st-c256, st-res-relu,
    st2-dm0 st2-dm1 st1 st1-spread
  k_conv_quad (variant 3, zp_conv_tuning(6, 0)): q-w32-ms q-w32 q-w64-ms q-w64
  k_conv1x1n (variant 7): n-32-64 n-64-256 (M = 65552: a last group that is no whole pass) n-slice;
    t-near-1x1n (M = 65535) stays on the tile
  epilogue / outputs: e-* on one tile and one strip case
  fp16 (forward): h-*     f32 (E = 4, one side +-[1, 4095]): f32-*
"""
import dataclasses
import json
import os
import subprocess
import sys
from contextlib import contextmanager
from dataclasses import dataclass, field

import numpy as np
import pytest

from tests import conv_ref as CR
from tests.conv_ref import BF16, F16, F32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@dataclass(frozen=True)
class Case:
    id: str
    cfg: tuple             # (variant, tc, tp, stages) the case is sized for
    dtype: str
    N: int
    H: int                 # the image the plan is made for (forward: x; data gradient: dx)
    W: int
    geo: tuple             # ("conv" | "dgrad", k, s, p, d), ("convT",), ("convT_dgrad",), ("aspp", d1, d2, d3)
    Cin: int               # channels of the launch's input and output
    Cout: int
    kw: dict = field(default_factory=dict)   # conv_ref.build's keywords
    tuning: tuple = ()     # zp_conv_tuning (key, value) pairs for the launch

    def spec(self):
        """(IH, IW, plan, weights, small, out_hw) of the launch"""
        from zebrapose_amd import geometry as G
        H, W, ci, co, g = self.H, self.W, self.Cin, self.Cout, self.geo
        small_below = 8 * CR.chunk(self.dtype)
        if g[0] == "conv":
            k, s, p, d = g[1:]
            plan = G.conv_fwd(H, W, k, s, p, d)
            return H, W, plan, [(0, (co, ci, k, k), 0)], (k, d, p) if ci < small_below else None, None
        if g[0] == "convT":
            plan = G.convT_fwd(H, W)
            return H, W, plan, [(0, (ci, co, 3, 3), 1)] * 4, None, None
        if g[0] == "dgrad":
            k, s, p, d = g[1:]
            plan = G.conv_dgrad(H, W, k, s, p, d)
            ih, iw = G.out_size(H, k, s, p, d), G.out_size(W, k, s, p, d)
            small = (k, -d, -p) if ci < small_below else None
            return ih, iw, plan, [(0, (ci, co, k, k), 1)] * len(plan.subs), small, (H, W)
        if g[0] == "convT_dgrad":
            return 2 * H, 2 * W, G.convT_dgrad(H, W), [(0, (co, ci, 3, 3), 0)], None, (H, W)
        assert g[0] == "aspp"  # as Engine.aspp_branches_fwd merges them
        plans = [G.conv_fwd(H, W, 1, 1, 0, 1)] + [G.conv_fwd(H, W, 3, 1, d, d) for d in g[1:]]
        merged = G.Plan(H, W, 1, [p.subs[0] for p in plans])
        return H, W, merged, [(i, (co, ci, k, k), 0) for i, k in enumerate((1, 3, 3, 3))], None, None

    def build(self, device=None, seed=0, **over):
        ih, iw, plan, weights, small, out_hw = self.spec()
        kw = dict(self.kw, **over)
        if self.geo[0] == "aspp":
            kw.setdefault("cy0", [i * self.Cout for i in range(4)])
        return CR.build(self.dtype, self.N, ih, iw, plan, self.Cin, self.Cout, weights=weights, small=small,
                        out_hw=out_hw, seed=seed, device=device, **kw)


K3, K1, K3S2, K1S2 = ("conv", 3, 1, 1, 1), ("conv", 1, 1, 0, 1), ("conv", 3, 2, 1, 1), ("conv", 1, 2, 0, 1)
RAW = dict(out_mode=CR.NHWC_F32)                 # the raw f32 store of a 16-bit call
PM = dict(xdraw="pm1", wdraw="pm1")              # 16-bit stores: every |y| below 256
PMH = dict(xdraw="pm1", wdraw="half")
T64, T128, T256 = (0, 64, 128, 3), (0, 128, 128, 3), (0, 128, 256, 3)
S64 = (2, 64, 256, 3)


def dil(d):
    return ("conv", 3, 1, d, d)


TILE = [
    Case("t-m1", T64, BF16, 1, 1, 1, K1, 64, 64, PM),
    Case("t-m129", T128, BF16, 1, 3, 43, K3, 64, 128, PM),
    Case("t-m257", T256, BF16, 1, 1, 257, K3, 64, 136, PM),
    Case("t-gw15-n3", T128, BF16, 3, 7, 15, K3, 128, 72, RAW),
    Case("t-cout17", (0, 32, 128, 2), BF16, 2, 5, 13, K1, 320, 17, dict(PM, ldy=20)),
    Case("t-slice-a", T128, BF16, 2, 6, 10, K3, 64, 72,
         dict(PM, cx0=8, ldx=80, cy0=8, ldy=88, res=True, cr0=8, ldr=80)),
    Case("t-slice-b", T128, BF16, 2, 6, 10, K3, 64, 72,
         dict(PM, cx0=16, ldx=96, cy0=4, ldy=80, res=True, cr0=4, ldr=76)),
    Case("t-s2-3x3", T64, BF16, 2, 9, 11, K3S2, 64, 64, PM),
    Case("t-s2-1x1", T64, BF16, 2, 9, 11, K1S2, 64, 64, PM),
    Case("t-dil6", T64, BF16, 2, 4, 20, dil(6), 64, 64, PM),
    Case("t-dil12", T256, BF16, 1, 32, 32, dil(12), 64, 192, RAW),
    Case("t-dil18", T256, BF16, 1, 32, 32, dil(18), 64, 192, RAW),
    Case("t-convT", T64, BF16, 2, 5, 9, ("convT",), 64, 64, PM),
    Case("t-dgrad-s1", T64, BF16, 2, 6, 10, ("dgrad", 3, 1, 1, 1), 64, 64, PM),
    Case("t-dgrad-s2", T64, BF16, 2, 8, 12, ("dgrad", 3, 2, 1, 1), 64, 64, PM),
    Case("t-dgrad-s2-1x1", T64, BF16, 2, 8, 12, ("dgrad", 1, 2, 0, 1), 64, 64, PM),
    Case("t-dgrad-convT", T64, BF16, 2, 5, 9, ("convT_dgrad",), 64, 64, PM),
    Case("t-aspp", T256, BF16, 1, 9, 13, ("aspp", 6, 12, 18), 64, 256, dict(PMH, relu=1, scale=True, shift=True)),
    Case("t-tc256-1", (0, 256, 256, 2), BF16, 1, 5, 20, K3, 64, 256, PM, ((0, 0),)),
    Case("t-tc256-4", (0, 256, 256, 2), BF16, 2, 5, 9, ("convT",), 64, 256, PM, ((0, 0),)),
    Case("t-near-d5-w32", T64, BF16, 1, 8, 32, dil(5), 64, 64, PM),
    Case("t-near-ghw224", T64, BF16, 1, 7, 32, K3, 64, 64, PM),
    Case("t-near-w48", T64, BF16, 1, 16, 48, K3, 64, 64, PM),
    Case("t-key2-off", T64, BF16, 1, 8, 32, K3, 64, 64, PM, ((2, 0),)),
    Case("t-quad-off", T64, BF16, 1, 8, 32, ("convT",), 64, 64, PM),
    Case("t-near-1x1n", T64, BF16, 1, 255, 257, K1, 64, 64, PM),
]
SMALL = [
    Case("s-cin8-7x7", (0, 64, 256, 2), BF16, 2, 9, 11, ("conv", 7, 2, 3, 1), 8, 64, PM),
    Case("s-cin16", (0, 64, 256, 2), BF16, 2, 6, 10, K3, 16, 64, PM),
    Case("s-cin24", (0, 64, 256, 2), BF16, 2, 6, 10, K3, 24, 64, PM),
    Case("s-kpad", (0, 64, 256, 2), BF16, 2, 6, 10, K3, 8, 64, dict(PM, k_pad=192)),
]
STRIP = [
    Case("st-8x32", S64, BF16, 1, 8, 32, K3, 64, 64, PM),
    Case("st-4x64", S64, BF16, 1, 4, 64, K3, 64, 64, PM),
    Case("st-2x128", S64, BF16, 1, 2, 128, K3, 64, 64, PM),
    Case("st-d4-w32", S64, BF16, 1, 8, 32, dil(4), 64, 64, PM),
    Case("st-d8-w64", S64, BF16, 1, 4, 64, dil(8), 64, 64, PM),
    Case("st-d16-w128", S64, BF16, 1, 2, 128, dil(16), 64, 64, PM),
    Case("st-16x32-n3", S64, BF16, 3, 16, 32, K3, 64, 64, PM),
    Case("st-c128", S64, BF16, 1, 8, 32, K3, 64, 128, PM),
    Case("st-c192", S64, BF16, 1, 8, 32, K3, 128, 192, PM),
    Case("st-c256", S64, BF16, 1, 8, 32, K3, 64, 256, PM),
    Case("st-res-relu", S64, BF16, 2, 8, 32, K3, 64, 64, dict(PM, res=True, relu=1)),
    Case("st2-dm0", S64, BF16, 2, 8, 32, K3, 64, 64, PM, ((1, 222),)),
    Case("st2-dm1", S64, BF16, 2, 8, 32, K3, 64, 64, PM, ((1, 254),)),
    Case("st1", (1, 64, 256, 3), BF16, 2, 8, 32, K3, 64, 64, PM, ((1, 158),)),
    Case("st1-spread", (1, 64, 256, 3), BF16, 2, 8, 32, K3, 64, 128, PM, ((1, 190),)),
]
Q = (3, 64, 256, 3)
QUAD = [
    Case("q-w32-ms", Q, BF16, 1, 8, 32, ("convT",), 64, 64, PM, ((6, 0),)),
    Case("q-w32", Q, BF16, 2, 8, 32, ("convT",), 64, 128, PM, ((6, 0), (1, 222))),
    Case("q-w64-ms", Q, BF16, 1, 4, 64, ("convT",), 64, 128, PM, ((6, 0),)),
    Case("q-w64", Q, BF16, 1, 4, 64, ("convT",), 128, 64, PM, ((6, 0), (1, 222))),
]
C1N = [
    Case("n-32-64", (7, 64, 256, 2), BF16, 1, 256, 256, K1, 32, 64, PM),
    Case("n-64-256", (7, 128, 256, 3), BF16, 1, 241, 272, K1, 64, 256, PM),
    Case("n-slice", (7, 64, 128, 3), BF16, 1, 256, 256, K1, 64, 64, dict(PM, cx0=8, ldx=72, cy0=8, ldy=72)),
]
_EP = [("scale", dict(scale=True)), ("shift", dict(shift=True)),
       ("all", dict(scale=True, shift=True, res=True, relu=1)), ("f32", dict(RAW, scale=True, shift=True))]
EPI = ([Case(f"e-tile-{n}", T128, BF16, 2, 7, 15, K3, 64, 72, dict(PMH, **kw)) for n, kw in _EP]
       + [Case(f"e-strip-{n}", S64, BF16, 1, 8, 32, K3, 64, 64, dict(PMH, **kw)) for n, kw in _EP]
       + [Case("e-head-1", (0, 32, 128, 2), BF16, 2, 7, 15, K1, 64, 1, dict(out_mode=CR.HEAD, shift=True)),
          Case("e-head-17", (0, 32, 128, 2), BF16, 2, 7, 15, K3, 64, 17, dict(out_mode=CR.HEAD, shift=True)),
          Case("e-x3", (0, 128, 128, 3), F32, 2, 7, 15, K3, 32, 72, dict(out_mode=CR.X3, scale=True, shift=True)),
          Case("e-h2", (0, 128, 128, 3), F32, 2, 7, 15, K3, 32, 72, dict(out_mode=CR.H2, scale=True, shift=True))])
HALF = [dataclasses.replace(c, id="h-" + c.id, dtype=F16)
        for c in (TILE[1], TILE[3], TILE[5], TILE[12], TILE[17], SMALL[0], STRIP[0], STRIP[6], QUAD[0], C1N[0])]
_F32 = [
    Case("f32-m1", (0, 64, 128, 3), F32, 1, 1, 1, K1, 32, 64),
    Case("f32-gw15-n3", (0, 128, 128, 3), F32, 3, 7, 15, K3, 64, 72, dict(cx0=4, ldx=72, cy0=4, ldy=80)),
    Case("f32-cout17", (0, 32, 128, 2), F32, 2, 5, 13, K3S2, 32, 17, dict(ldy=20, res=True, cr0=4, ldr=24)),
    Case("f32-convT", (0, 128, 256, 3), F32, 2, 5, 9, ("convT",), 32, 136),
    Case("f32-dgrad-s2", (0, 64, 128, 3), F32, 2, 8, 12, ("dgrad", 3, 2, 1, 1), 32, 64),
    Case("f32-s-cin8", (0, 64, 256, 2), F32, 2, 9, 11, ("conv", 7, 2, 3, 1), 8, 64),
]
F32S = [dataclasses.replace(c, id=f"{c.id}-wide-{s}", kw=dict(c.kw, **{s + "draw": "wide"}))
        for c in _F32 for s in ("x", "w")]
CASES = TILE + SMALL + STRIP + QUAD + C1N + EPI + HALF + F32S
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the same launch on two kernels: equal bits
SAME_BITS = [("st-8x32", "t-key2-off"), ("q-w32-ms", "t-quad-off")]

# N(0, 1) operands on the dtype's grid: the derived bound of test_real_values
REAL_CASES = [dataclasses.replace(BY_ID[i], id="real-" + i, kw=dict(BY_ID[i].kw, xdraw="real", wdraw="real"))
              for i in ("t-gw15-n3", "st-16x32-n3", "f32-gw15-n3-wide-x")]

# statistics: (case, parts per pixel tile) over tile, strip (one part per wave half), strip2 and quad
STAT_CASES = [dataclasses.replace(BY_ID[i], id="stats-" + i, kw=dict(BY_ID[i].kw, stats=True)) for i in
              ("t-m129", "t-m257", "t-convT", "st-16x32-n3", "st1", "q-w32-ms", "f32-gw15-n3-wide-x")]
BNR_CASES = [dataclasses.replace(BY_ID[i], id="bnr-" + i, kw=dict(BY_ID[i].kw, bnr=True)) for i in
             ("t-dgrad-s1", "t-dgrad-convT", "f32-dgrad-s2-wide-x")] + [
    Case("bnr-strip", S64, BF16, 2, 8, 32, ("dgrad", 3, 1, 1, 1), 64, 64, dict(PM, bnr=True))]

# paths an environment variable read once per process selects, two settings of each per child:
# (environment, cases with the cfg expected there)
def _env(i, tag, cfg):
    return dataclasses.replace(BY_ID[i], id=f"{i}-{tag}", cfg=cfg)


ENV_RUNS = [
    ({"ZP_CONV_STRIP": "0", "ZP_CONV_STAGES": "2", "ZP_CONV_TP": "256"},
     [_env(i, "nostrip", (0, 64, 256, 2)) for i in ("st-8x32", "st-d8-w64", "st-16x32-n3")]
     + [_env(i, "tp256-st2", (0, BY_ID[i].cfg[1], 256, 2))
        for i in ("t-m129", "t-gw15-n3", "t-dil6", "t-m257", "t-convT", "t-dil12")]),
    ({"ZP_STRIP_TC64": "0", "ZP_CONV_STAGES": "3", "ZP_CONV_TP": "128"},
     [_env(i, "tc128", (2, 128, 256, 3)) for i in ("st-c256", "st-c192")]
     + [_env("t-cout17", "st3", (0, 32, 128, 3)), _env("s-cin8-7x7", "tp128-st3", (0, 64, 128, 3))]
     + [_env(i, "tp128", (0, 128, 128, 3)) for i in ("t-m257", "t-dil12", "t-aspp")]),
]
# the fused 16-bit head (the strip tile of 128 channels: at this size under ZP_STRIP_TC64=0)
HEAD_ENV = {"ZP_STRIP_TC64": "0"}
HEAD_CASE = Case("head", (2, 128, 256, 3), BF16, 1, 8, 32, K3, 64, 256, dict(PMH, relu=1, scale=True, shift=True))


@contextmanager
def tuned(kvs):
    """zp_conv_tuning(key, value) for the block; the old values back afterwards"""
    from zebrapose_amd import _lib as L
    old = [(k, L.lib.zp_conv_tuning(k, v)) for k, v in kvs]
    try:
        yield
    finally:
        for k, v in reversed(old):
            L.lib.zp_conv_tuning(k, v)


def check_plan(c, b):
    """the kernel the case is sized for (a failure here: the case is wrongly sized)"""
    got = b.config()
    assert got == c.cfg, f"{c.id}: sized for (variant, tc, tp, stages) {c.cfg}, the plan takes {got}"


def f32bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def compare(b, what="y"):
    """the output buffers against the reference, bit for bit -> problems (a list of strings)"""
    a, bad = b.a, []

    def cmp(name, want):
        got, ok = b.read(name, want.shape)
        if not ok:
            bad.append(f"{name}: a guard was overwritten")
        w32 = want.astype(np.float32)
        assert (w32.astype(np.float64) == want).all()
        ne = f32bits(got) != f32bits(w32)
        if ne.any():
            idx = np.argwhere(ne)
            bad.append(f"{name}: {len(idx)} of {ne.size} elements differ; first {idx[:5].tolist()}, got "
                       f"{[float(got[tuple(i)]) for i in idx[:5]]}, want {[float(want[tuple(i)]) for i in idx[:5]]}")

    if a.out_mode == CR.HEAD:
        y, y2 = b.want()
        cmp("y", y)
        if a.Cout > 1:
            cmp("y2", y2)
        else:
            cmp("y2", np.full(1, CR.GARBAGE))
    elif b.store == "planes":
        want, written = b.want()
        npl = 3 if a.out_mode == CR.X3 else 2
        words, ok = b.read("y", (npl,) + want.shape)
        if not ok:
            bad.append("y: a guard was overwritten")
        joined = CR.join_planes(words.view(np.uint16), a.out_mode)
        if (f32bits(joined[written]) != f32bits(want[written])).any():
            bad.append("y: joined planes differ from the reference")
        if (words[:, ~written] != CR.GARBAGE_WORD).any():
            bad.append("y: a word outside the written channels changed")
    else:
        cmp("y", b.want())
    if not b.inputs_intact():
        bad.append("an input buffer or its guard changed")
    return bad


def run_exact(c, device, extra_check=None):
    """the case twice: plan, return codes, exact equality with the reference, equal bits -> y"""
    with tuned(c.tuning):
        b = c.build(device)
        check_plan(c, b)
        rc1 = b.launch()
        bad = compare(b)
        got1 = {n: b.dev[n].clone() for n in b.outputs if n in b.dev}
        if extra_check:
            extra_check(b)
        rc2 = b.launch()
    assert rc1 == 0 and rc2 == 0, (rc1, rc2)
    print(f"{c.id}: cfg {c.cfg}, M {b.M}")
    assert not bad, f"{c.id}: " + "; ".join(bad)
    import torch
    for n, t in got1.items():
        bits = torch.int16 if t.element_size() == 2 else torch.int32
        assert bool((t.view(bits) == b.dev[n].view(bits)).all()), f"{c.id}: two launches differ in {n}"
    return got1["y"]


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_exact(gpu, c):
    run_exact(c, gpu)


@pytest.mark.parametrize("i,j", SAME_BITS)
def test_same_bits(gpu, i, j):
    """the same arguments on the special kernel and on the tile: the same bits"""
    import torch
    p, q = run_exact(BY_ID[i], gpu), run_exact(BY_ID[j], gpu)
    assert bool((p.view(torch.int16) == q.view(torch.int16)).all())


def stat_bound(v, n):
    """(mean, M2) error of one part of n f32 values |v| <= V taken as the kernels take them: exact
    integer sums, mean = sum / n (one rounding), n differences, squares and adds (<= 2 roundings of
    2^-24 per term on dlt^2 <= 4 V^2, n + 1 adds), then at most 3 pairwise merges of wave halves (<= 8
    roundings each on values below 2 V, resp. on 4 n V^2).  Derived, not measured."""
    V, u = float(np.abs(v).max()), 2.0 ** -24
    return 32 * u * V, (n + 64) * 2 * u * 4 * n * V * V


def check_stats(c, b):
    """counts per part exact; the parts merged in f64 (pairwise formula) against the reference"""
    from zebrapose_amd import _lib as L
    import ctypes
    a = b.a
    parts = int(L.lib.zp_conv2d_stat_parts(ctypes.byref(a)))
    var, tc, tp, _ = b.config()
    per_tile = 4 if var in (1, 3) else 1          # k_conv_strip: wave halves; k_conv_quad: the four phases
    tiles = b.part_pixels(tp)
    nsub = a.nsub
    assert parts == len(tiles) * (per_tile if var in (1, 3) else nsub), (parts, len(tiles), nsub)
    st, ok = b.read("stats", (3, parts, a.Cout))
    assert ok, "stats: a guard was overwritten"
    st = st.astype(np.float64)
    for s in range(nsub):
        v = b.stored(s).reshape(b.M, a.Cout)
        if var == 3:      # part = tile * 4 + phase
            idx = [(t * 4 + s, lo, hi) for t, (lo, hi) in enumerate(tiles)]
        elif var == 1:    # part = tile * 4 + wave half of 64 pixels
            idx = [(t * 4 + h, lo + 64 * h, lo + 64 * h + 64) for t, (lo, hi) in enumerate(tiles) for h in range(4)]
        else:             # part = sub * tiles + tile
            idx = [(s * len(tiles) + t, lo, hi) for t, (lo, hi) in enumerate(tiles)]
        n_tot, mu, m2, e_mu, e_m2 = 0.0, np.zeros(a.Cout), np.zeros(a.Cout), 0.0, 0.0
        for k, lo, hi in idx:
            n = hi - lo
            assert (st[0, k] == n).all(), f"{c.id}: part {k} counts {st[0, k][:4]}, its tile has {n} pixels"
            em, eq = stat_bound(v[lo:hi], n)
            ref_mu, ref_m2 = v[lo:hi].mean(0), ((v[lo:hi] - v[lo:hi].mean(0)) ** 2).sum(0)
            assert (np.abs(st[1, k] - ref_mu) <= em).all() and (np.abs(st[2, k] - ref_m2) <= eq).all(), (c.id, k)
            d = st[1, k] - mu
            mu = mu + d * n / (n_tot + n)
            m2 = m2 + st[2, k] + d * d * n_tot * n / (n_tot + n)
            n_tot += n
            e_mu, e_m2 = max(e_mu, em), e_m2 + eq + n * 4 * float(np.abs(v).max()) * em
        assert n_tot == b.M
        assert (np.abs(mu - v.mean(0)) <= e_mu).all(), f"{c.id}: merged mean off by {np.abs(mu - v.mean(0)).max()}"
        assert (np.abs(m2 - ((v - v.mean(0)) ** 2).sum(0)) <= e_m2).all(), f"{c.id}: merged M2"


@pytest.mark.parametrize("c", STAT_CASES, ids=[c.id for c in STAT_CASES])
def test_stats(gpu, c):
    run_exact(c, gpu, extra_check=lambda b: check_stats(c, b))


def check_bnr(c, b):
    """the parts as written, and finished by zp_bn_bwd_totals, against the reference bit for bit"""
    import ctypes
    import torch
    from zebrapose_amd import _lib as L
    a = b.a
    parts = int(L.lib.zp_conv2d_bnr_parts(ctypes.byref(a)))
    var, tc, tp, _ = b.config()
    tiles = b.part_pixels(tp)
    assert var in (0, 2) and parts == len(tiles) * a.nsub
    pt, ok = b.read("bnr_part", (2, parts + 1, a.Cout))
    assert ok, "bnr_part: a guard was overwritten"
    tot = np.zeros((2, a.Cout))
    for s in range(a.nsub):
        g, gx = b.bnr_terms(s)
        for t, (lo, hi) in enumerate(tiles):
            k = s * len(tiles) + t
            for i, term in enumerate((g, gx)):
                want = term[lo:hi].sum(0)
                assert (f32bits(pt[i, k]) == f32bits(want + 0.0)).all(), f"{c.id}: partials[{i}][{k}]"
                tot[i] += want
    dg = torch.full((2, a.Cout), CR.GARBAGE, dtype=torch.float32, device=b.dev["device"])
    ptr = b.dev["bnr_part"].data_ptr() + 4 * CR.GUARD
    assert L.lib.zp_bn_bwd_totals(ptr, parts, a.Cout, parts, dg[1].data_ptr(), dg[0].data_ptr(), 0, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    pt, ok = b.read("bnr_part", (2, parts + 1, a.Cout))
    assert ok
    for i in range(2):
        assert (f32bits(pt[i, parts]) == f32bits(tot[i] + 0.0)).all(), f"{c.id}: totals row {i}"
        assert (f32bits(dg[i].cpu().numpy()) == f32bits(tot[i] + 0.0)).all(), f"{c.id}: dbeta / dgamma"


@pytest.mark.parametrize("c", BNR_CASES, ids=[c.id for c in BNR_CASES])
def test_bnr_part(gpu, c):
    run_exact(c, gpu, extra_check=lambda b: check_bnr(c, b))


def _bad_cin(b):
    b.a.Cin = 72          # ldx stays 80: only Cin is off the 64-channel K step


def _bad_ldy(b):
    b.a.sub[0].ldy = b.a.sub[0].cy0 + b.a.Cout - 4


def _bad_cy0(b):
    b.a.sub[0].cy0 = 6


def _bad_kpad(b):
    b.a.k_pad = 9 * 64 - 64


def _bad_wrows(b):
    b.a.w_rows = b.a.w_rows + 8


def _bad_stats_res(b):
    b.a.stats = b.a.res  # (any valid pointer: the launch must be refused before it is used)


@pytest.mark.parametrize("spoil", [_bad_cin, _bad_ldy, _bad_cy0, _bad_kpad, _bad_wrows, _bad_stats_res],
                         ids=lambda f: f.__name__[5:])
def test_argument_errors(gpu, spoil):
    """one bad field, valid pointers and sizes everywhere else: ZP_ERR_ARG, and nothing launched"""
    c = Case("args", T128, BF16, 2, 6, 10, K3, 64, 72, dict(PM, ldx=80, cy0=8, ldy=96, res=True))
    b = c.build(gpu)
    check_plan(c, b)
    spoil(b)
    rc = b.launch()
    assert rc == 1, rc
    got, ok = b.read("y")
    assert ok and (f32bits(got) == f32bits(CR.to_store(CR.GARBAGE, BF16))).all(), "y written by a refused launch"
    assert b.inputs_intact()


@pytest.mark.parametrize("c", REAL_CASES, ids=[c.id for c in REAL_CASES])
def test_real_values(gpu, c):
    """N(0, 1) operands on the dtype's grid (bf16 products are exact in f32): per element
    |got - ref| <= (K + 1) * 2^-23 * sum |w| |x| -- K = taps * Cin terms, one rounding or truncation
    per add in any order -- plus one rounding of the stored value; derived, not measured."""
    b = c.build(gpu, out_mode=CR.NHWC_F32 if c.dtype != F32 else CR.NHWC)
    check_plan(c, b)
    assert b.launch() == 0
    got, ok = b.read("y", b.y_shape())
    assert ok
    K = max(b.a.sub[s].ntaps for s in range(b.a.nsub)) * b.a.Cin
    ratio = 0.0
    for s in range(b.a.nsub):
        oy, ox = b.out_pixels(s)
        c0 = b.a.sub[s].cy0
        g = got[:, oy, ox, c0:c0 + b.a.Cout].astype(np.float64)
        want = b.values(s)
        lim = (K + 1) * 2.0 ** -23 * b.acc(s, absolute=True) + 2.0 ** -24 * np.abs(want)
        assert np.isfinite(g).all() and (lim > 0).all()
        ratio = max(ratio, float((np.abs(g - want) / lim).max()))
    print(f"{c.id}: cfg {c.cfg}, K {K}, largest |got - ref| / bound = {ratio:.3g}")
    assert ratio <= 1.0, f"{c.id}: |got - ref| reaches {ratio:.3g} of the bound"


def head_args(b, hcout, seed=5):
    """L.HeadArgs of the fused head over [the conv's 256 channels | 32 channels of an x2 slice], and the
    reference (mask, code)"""
    import ctypes
    from zebrapose_amd import _lib as L
    a, rng = b.a, np.random.default_rng(seed)
    C2, cx20, ldx2 = 32, 8, 48
    P = a.N * a.GH * a.GW
    hw = rng.choice([-1.0, 1.0], (hcout, a.Cout + C2))
    bias = rng.integers(-8, 9, hcout).astype(np.float64)
    x2 = np.full((P, ldx2), np.nan)
    x2[:, cx20:cx20 + C2] = rng.integers(1, 4, (P, C2)) * rng.choice([-1, 1], (P, C2))
    feat = np.concatenate([b.stored(0).reshape(P, a.Cout), x2[:, cx20:cx20 + C2]], 1)
    out = feat @ hw.T + bias                                   # [P][hcout]: integers below 2^24
    out = out.reshape(a.N, a.GH * a.GW, hcout).transpose(0, 2, 1)
    h = L.HeadArgs()
    h.k_pad, h.cout, h.ldx2, h.cx20, h.C2 = a.Cout + C2, hcout, ldx2, cx20, C2
    if b.dev:
        import torch
        tdt = CR.torch_dtype(b.dtype)
        src = torch.from_numpy(hw.astype(np.float32)).to(b.dev["device"])
        h.w = b.guarded("hw", np.full(32 * h.k_pad, CR.GARBAGE), tdt)
        z = (ctypes.c_int * 1)(0)
        assert L.lib.zp_pack_weight(src.data_ptr(), hcout, a.Cout + C2, 1, 1, 0, 1, z, z, a.Cout + C2, a.dtype, h.w,
                                    32, h.k_pad, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        b.dev["hw@"] = b.dev["hw"].cpu()
        h.bias = b.guarded("hbias", bias)
        h.x2 = b.guarded("x2", x2, tdt)
        h.mask = b.guarded("mask", np.full(P, CR.GARBAGE))
        h.code = b.guarded("code", np.full(P * max(1, hcout - 1), CR.GARBAGE))
        ws = int(L.lib.zp_conv2d_head_ws(ctypes.byref(a)))
        assert ws == 2 * 32 * P * 4
        h.ws = b.guarded("ws", np.full(ws // 4, CR.GARBAGE))
    return h, out[:, :1], out[:, 1:]


def child_head():
    """the fused 16-bit head, hcout 17 and 32, in this process: one JSON line per case"""
    import torch
    from zebrapose_amd import _lib as L
    import ctypes
    dev = torch.device("cuda:0")
    for hcout in (17, 32):
        b = HEAD_CASE.build(dev)
        h, mask, code = head_args(b, hcout)
        okh = int(L.lib.zp_conv2d_head_ok(ctypes.byref(b.a)))
        rec = {"id": f"head-{hcout}", "cfg": list(b.config()), "head_ok": okh, "rc": [], "bad": []}
        outs = []
        for _ in range(2):
            rec["rc"].append(b.launch(head=h))
            m, ok1 = b.read("mask", mask.shape)
            cd, ok2 = b.read("code", code.shape)
            _, ok3 = b.read("ws")
            y, ok4 = b.read("y")
            if not (ok1 and ok2 and ok3 and ok4):
                rec["bad"].append("a guard was overwritten")
            if (f32bits(m) != f32bits(mask)).any() or (f32bits(cd) != f32bits(code)).any():
                rec["bad"].append(f"mask / code differ in {int((f32bits(m) != f32bits(mask)).sum())} / "
                                  f"{int((f32bits(cd) != f32bits(code)).sum())} elements")
            if (f32bits(y) != f32bits(CR.to_store(CR.GARBAGE, BF16))).any():
                rec["bad"].append("y written by the fused launch")
            if not b.inputs_intact():
                rec["bad"].append("an input changed")
            outs.append((m.copy(), cd.copy()))
        if (f32bits(outs[0][0]) != f32bits(outs[1][0])).any() or (f32bits(outs[0][1]) != f32bits(outs[1][1])).any():
            rec["bad"].append("two launches differ")
        print(json.dumps(rec), flush=True)


def child(run):
    """ENV_RUNS[run]'s cases in this process: one JSON line per case"""
    import torch
    dev = torch.device("cuda:0")
    for c in ENV_RUNS[int(run)][1]:
        b = c.build(dev)
        rec = {"id": c.id, "cfg": list(b.config()), "rc": [], "bad": []}
        outs = []
        for _ in range(2):
            rec["rc"].append(b.launch())
            rec["bad"] += compare(b)
            outs.append(b.dev["y"].clone())
        if not bool((outs[0].view(torch.int16) == outs[1].view(torch.int16)).all()):
            rec["bad"].append("two launches differ")
        print(json.dumps(rec), flush=True)


def _child(code, extra):
    env = dict(os.environ, ZP_QUIET="1", **extra)
    r = subprocess.run([sys.executable, "-c", f"from tests.test_gpu_conv_edges import child, child_head; {code}"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, (extra, r.returncode, r.stderr[-3000:])
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_env_selected_kernels(gpu):
    """ZP_CONV_STRIP=0 and ZP_STRIP_TC64=0, each with one setting of the stage and pixel-tile overrides
    (ZP_CONV_STAGES, ZP_CONV_TP): read once per process, so one fresh child per environment, one after
    the other; the first failure ends it."""
    for run, (extra, cases) in enumerate(ENV_RUNS):
        recs = _child(f"child({run})", extra)
        print(f"{extra}: {recs}")
        assert [x["id"] for x in recs] == [c.id for c in cases]
        for x, c in zip(recs, cases):
            assert tuple(x["cfg"]) == c.cfg, f"{c.id} under {extra}: sized for {c.cfg}, the plan takes {x['cfg']}"
            assert x["rc"] == [0, 0] and not x["bad"], (extra, x)


def test_fused_head(gpu):
    """zp_conv2d_head on the 16-bit path: N 1, 8 x 32, Cin 64, Cout 256, an x2 slice, hcout 17 and 32; the
    workspace exactly zp_conv2d_head_ws bytes between guards; mask and code exact, both launches."""
    recs = _child("child_head()", HEAD_ENV)
    print(recs)
    assert [x["id"] for x in recs] == ["head-17", "head-32"]
    for x in recs:
        assert tuple(x["cfg"]) == HEAD_CASE.cfg and x["head_ok"] == 1, x
        assert x["rc"] == [0, 0] and not x["bad"], x


@pytest.mark.parametrize("geo", [("conv", 1, 2, 0, 1), ("conv", 3, 2, 1, 1)], ids=["s2-1x1", "s2-3x3"])
def test_engine_dx_stride2(gpu, geo):
    """Engine.unit_bwd of a conv unit (no BN: the head form) with stride 2 on an even image, integer
    weights and gradients: dx equals the reference exactly -- the engine zero-fills the pixels of the
    phases that have no taps."""
    import torch
    from zebrapose_amd.engine import Act, Engine, Unit
    _, k, s, p, d = geo
    N, H, W, ci, co = 2, 8, 12, 64, 64
    c = Case("engine-dx", T64, BF16, N, H, W, ("dgrad", k, s, p, d), co, ci, PM)
    b = c.build()
    conv = torch.nn.Conv2d(ci, co, k, s, p, bias=False).to(gpu)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(b.subs[0][0].astype(np.float32)))
    unit = Unit(conv, None, relu=False)
    eng = Engine(torch.nn.Module(), torch.bfloat16)
    x = Act(torch.zeros(N, H, W, ci, dtype=torch.bfloat16, device=gpu))
    gy = Act(torch.from_numpy(b.x.astype(np.float32)).to(gpu, torch.bfloat16))
    want = np.zeros((N, H, W, ci))
    for sb in range(b.a.nsub):
        oy, ox = b.out_pixels(sb)
        want[:, oy, ox] += b.stored(sb)
    for _ in range(2):
        gmap, grads = {"gy": gy}, {}
        eng.unit_bwd(("head", unit, x, "gy", None, None, None), gmap, grads)
        torch.cuda.synchronize()
        dx = gmap[x.buf.data_ptr()].float().cpu().numpy()
        assert (f32bits(dx) == f32bits(want)).all(), f"{int((f32bits(dx) != f32bits(want)).sum())} elements differ"
