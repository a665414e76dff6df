"""zp_conv2d_wgrad pinned to an exact reference at its edges, straight through the C ABI.

The operands are small non-zero integers (tests/wgrad_ref.py), so every product and every partial sum
is an integer below 2^24 and exact in f32 in any order: each launch must equal the f64 reference BIT
FOR BIT, twice over with equal bits, with the guards around dw and around the workspace (exactly
zp_conv2d_wgrad_ws_bytes long, NaN-filled before the first launch) intact.  A dropped, doubled or
misplaced pixel, a padded channel or a NaN from outside a channel slice reaching dw, a partial the
reduce reads but no kernel wrote: each changes the bits.

CASES names, per case, the kernel it is sized to reach -- k_wgrad (f32; bf16 under ZP_WGRAD=0),
k_wgrad_lds, or k_wgrad2 (the lean kernel) -- which the test asserts with a restatement of the
launch plan's eligibility rule, and where a case exists for its split count, that count, read as
ws_bytes / (nsub * Cout * cols_max * 4).  The split counts are sized for the MI355X's 256 compute
units.  tests/test_wgrad_ref_host.py checks the exactness preconditions of every entry on the CPU.

  k_wgrad_lds (bf16, not lean-eligible)
    lds-wrap16        GW 16: KP / 16 = 4 row wraps of the incremental walk in one K step; M = 240 is
                      not a whole K step
    lds-divide        GW 15 < 16: the divide path
    lds-pool-1x1      a 1 x 1 grid, N 70: 64 images inside one K step; the 256-row tile
    lds-straddle      Cin 72: column panels straddle taps; Cout 136: a partial second output-channel
                      tile and a partial third column tile; stride 2 on an odd image
    lds-slice-*       Cout 17 in a dy slice (lddy 32 / cdy0 0, lddy 40 / cdy0 8); x a slice (cx0 16)
    lds-dilated       3x3 d6 on a 4 x 20 grid: most taps in the padding
    lds-convT         the four ConvT phases: four sub-problems with 1 / 2 / 2 / 4 taps
    lds-split2        M = 2160, two splits of 1088: split 1 starts at image 4, row 5, column 8
    lds-padded        the same under zp_conv_tuning(5, 0): splits padded with empty pixel ranges
    near-*            near-misses of the lean kernel's rule (GHW 96; Cin 72; stride 2 with an odd IH)
    lean-off          lean-k1 with the lean kernel switched off (zp_conv_tuning(3, 0))
  k_wgrad2 (bf16, lean)
    lean-k1           one K step, the 2-stage ring
    lean-ring3-gh*    1..4 K steps on the 3-stage ring: its prologues and the first wrap
    lean-w128         W 128, Cout 256: the plan picks the 128 x 256 tile
    lean-s2-*         the stride-2 walk at W 32 (3x3 and 1x1) and W 128
    lean-split2-w128  M = 2688: split 1 starts at pixel 1344 = image 3, row 1, second half of the row
    lean-split2-w32   M = 2112: split 1 starts at pixel 1088 = image 5, row 4
  k_wgrad (f32; each with the 12-bit operand on either side)
    f32-m1, f32-m17, f32-split (M = 300, splits >= 2, pix_per no multiple of GW), f32-cw3-cout5,
    f32-cout130, f32-convT
  acc-*               accumulate = 1 onto a pre-filled dw
"""
import dataclasses
import json
import os
import subprocess
import sys
from contextlib import contextmanager
from dataclasses import dataclass

import numpy as np
import pytest

from tests import wgrad_ref as WR
from tests.wgrad_ref import BF16, F32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS, LEAN, REG = "k_wgrad_lds", "k_wgrad2", "k_wgrad"


@dataclass(frozen=True)
class Case:
    id: str
    kernel: str            # the kernel the case is sized to reach
    dtype: str
    N: int
    IH: int                # x is N x IH x IW
    IW: int
    conv: tuple            # (k, stride, pad, dilation) of a conv, or "convT" (3, s2, p1, op1: four phases)
    Cin: int
    Cw: int
    Cout: int
    cx0: int = 0
    ldx: int = None
    cdy0: int = 0
    lddy: int = None
    accumulate: int = 0
    wide: str = None       # f32: the operand drawn from +-[1, 4095]
    values: str = "int"
    splits: object = None  # an int: the plan's split count; ">=2"
    tuning: tuple = None   # zp_conv_tuning (key, value) for the launch
    plan_hw: tuple = None  # the image the plan is made for, when not IH x IW

    def plan(self):
        from zebrapose_amd import geometry as G
        h, w = self.plan_hw or (self.IH, self.IW)
        return G.convT_fwd(h, w) if self.conv == "convT" else G.conv_fwd(h, w, *self.conv)

    def build(self, device=None, seed=0):
        k = 3 if self.conv == "convT" else self.conv[0]
        return WR.build(self.dtype, self.N, self.IH, self.IW, self.plan(), self.Cin, self.Cw, self.Cout, kh=k, kw=k,
                        transposed_w=int(self.conv == "convT"), cx0=self.cx0, ldx=self.ldx, cdy0=self.cdy0,
                        lddy=self.lddy, accumulate=self.accumulate, values=self.values, wide=self.wide, seed=seed,
                        device=device)


K3, K1, K3S2, K1S2 = (3, 1, 1, 1), (1, 1, 0, 1), (3, 2, 1, 1), (1, 2, 0, 1)

BF16_CASES = [
    Case("lds-wrap16", LDS, BF16, 3, 5, 16, K3, 8, 3, 64),
    Case("lds-divide", LDS, BF16, 2, 7, 15, K3, 8, 3, 64),
    Case("lds-pool-1x1", LDS, BF16, 70, 1, 1, K1, 64, 64, 256),
    Case("lds-straddle", LDS, BF16, 5, 5, 33, K3S2, 72, 72, 136),
    Case("lds-slice-cdy0", LDS, BF16, 2, 6, 20, K1, 40, 40, 17, cx0=16, ldx=64, cdy0=0, lddy=32),
    Case("lds-slice-cdy8", LDS, BF16, 2, 6, 20, K1, 40, 40, 17, cx0=16, ldx=64, cdy0=8, lddy=40),
    Case("lds-dilated", LDS, BF16, 2, 4, 20, (3, 1, 6, 6), 16, 16, 32),
    Case("lds-convT", LDS, BF16, 3, 5, 9, "convT", 72, 72, 64),
    Case("lds-split2", LDS, BF16, 9, 10, 24, K3, 64, 64, 64, splits=2),
    # two splits of pixels and two of padding: (splits * 2 tiles) a multiple of 8 workgroups
    Case("lds-padded", LDS, BF16, 9, 10, 24, K3, 64, 64, 64, splits=4, tuning=(5, 0)),
    Case("lean-k1", LEAN, BF16, 1, 2, 32, K3, 64, 64, 64),
    *[Case(f"lean-ring3-gh{gh}", LEAN, BF16, 1, gh, 64, K3, 64, 64, 128) for gh in (1, 2, 3, 4)],
    Case("lean-w128", LEAN, BF16, 2, 1, 128, K3, 64, 64, 256),
    Case("lean-s2-w32", LEAN, BF16, 1, 8, 64, K3S2, 64, 64, 64),
    Case("lean-s2-w32-1x1", LEAN, BF16, 1, 8, 64, K1S2, 64, 64, 128),
    Case("lean-s2-w128", LEAN, BF16, 2, 2, 256, K3S2, 64, 64, 64),
    Case("lean-split2-w128", LEAN, BF16, 7, 3, 128, K3, 64, 64, 64, splits=2),
    Case("lean-split2-w32", LEAN, BF16, 11, 6, 32, K3, 64, 64, 64, splits=2),
    Case("near-ghw96", LDS, BF16, 1, 3, 32, K3, 64, 64, 64),
    Case("near-cin72", LDS, BF16, 1, 2, 32, K3, 72, 72, 64),
    # the stride-2 3x3 over a 2 x 32 grid whose image has one row more than 2 GH (no tap reaches it)
    Case("near-s2-odd-ih", LDS, BF16, 1, 5, 64, K3S2, 64, 64, 64, plan_hw=(4, 64)),
    Case("lean-off", LDS, BF16, 1, 2, 32, K3, 64, 64, 64, tuning=(3, 0)),
]

_F32 = [
    Case("f32-m1", REG, F32, 1, 1, 1, K3, 8, 8, 16),
    Case("f32-m17", REG, F32, 1, 1, 17, K3, 8, 8, 16),
    Case("f32-split", REG, F32, 2, 6, 25, K3, 8, 8, 64, splits=">=2"),
    Case("f32-cw3-cout5", REG, F32, 2, 5, 7, K3, 4, 3, 5, lddy=8),
    Case("f32-cout130", REG, F32, 2, 5, 7, K3, 4, 3, 130),
    Case("f32-convT", REG, F32, 3, 5, 9, "convT", 72, 72, 64),
]
F32_CASES = [dataclasses.replace(c, id=f"{c.id}-wide-{w}", wide=w) for c in _F32 for w in ("x", "dy")]

BY_ID = {c.id: c for c in BF16_CASES + F32_CASES}
ACC_CASES = [dataclasses.replace(BY_ID[i], id=f"acc-{i}", accumulate=1)
             for i in ("lds-wrap16", "lean-k1", "f32-m17-wide-x", "f32-m17-wide-dy")]
CASES = BF16_CASES + F32_CASES + ACC_CASES
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# N(0, 1) operands: the derived bound of test_real_values
REAL_CASES = [dataclasses.replace(BY_ID[i], id=f"real-{i}", values="real", wide=None)
              for i in ("lds-straddle", "lean-split2-w128", "f32-split-wide-x")]

# paths an environment variable read once per process selects: (environment, kernel, cases)
ENV_RUNS = [
    ({"ZP_WGRAD": "0"}, "k_wgrad<bf16>", [BY_ID[i] for i in ("lds-wrap16", "lds-straddle", "lds-convT", "lds-split2")]),
    ({"ZP_WGRAD_BIG": "2"}, "k_wgrad2<4,4,2,2>", [dataclasses.replace(BY_ID[i], id=f"{i}-cout256", Cout=256)
                                                  for i in ("lean-w128", "lean-split2-w128")]),
]


@contextmanager
def tuned(kv):
    """zp_conv_tuning(key, value) for the block; the old value back afterwards"""
    from zebrapose_amd import _lib as L
    old = L.lib.zp_conv_tuning(*kv) if kv else None
    try:
        yield
    finally:
        if kv:
            L.lib.zp_conv_tuning(kv[0], old)


def check_plan(c, b):
    """the kernel and split count the case is sized for (a failure here: the case is wrongly sized)"""
    key3 = 0 if c.tuning and c.tuning[0] == 3 and not c.tuning[1] else 1
    lean = WR.lean_eligible(b.a, key3)
    kernel = REG if c.dtype == F32 else (LEAN if lean else LDS)
    assert kernel == c.kernel, f"{c.id}: sized for {c.kernel}, the plan takes {kernel}"
    if c.splits == ">=2":
        assert b.splits >= 2, (c.id, b.splits)
    elif c.splits is not None:
        assert b.splits == c.splits, (c.id, b.splits)


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def mismatches(got, want):
    """number of elements of got (f32) that are not want (f64, exactly representable) bit for bit"""
    w32 = want.astype(np.float32)
    assert (w32.astype(np.float64) == want).all()
    return int((bits(got) != bits(w32)).sum())


def describe(b, got, want):
    bad = np.argwhere(bits(got) != bits(want.astype(np.float32)))
    d = got.astype(np.float64) - want
    return (f"{len(bad)} of {got.size} elements differ; first (dw index) {bad[:6].tolist()}, "
            f"got - want there {[d[tuple(i)] for i in bad[:6]]}; M {b.M}, splits {b.splits}")


def run_exact(c, device):
    """the case twice -> dw; asserts plan, return codes, exact equality with the reference, equal bits"""
    with tuned(c.tuning):
        b = c.build(device)
        check_plan(c, b)
        rc1, got1 = b.launch()
        rc2, got2 = b.launch()
    assert rc1 == 0 and rc2 == 0, (rc1, rc2)
    want = b.want()
    print(f"{c.id}: {c.kernel}, M {b.M}, splits {b.splits}")
    assert mismatches(got1, want) == 0, describe(b, got1, want)
    assert (bits(got1) == bits(got2)).all(), "two launches of the same case differ"
    return got1


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_exact(gpu, c):
    run_exact(c, gpu)


def test_lean_off_gives_lean_bits(gpu):
    """k_wgrad_lds in the lean kernel's place (zp_conv_tuning(3, 0)): the same bits"""
    a, b = run_exact(BY_ID["lean-k1"], gpu), run_exact(BY_ID["lean-off"], gpu)
    assert (bits(a) == bits(b)).all()


@pytest.mark.parametrize("swap", [True, False], ids=["swap", "phases"])
def test_engine_convT_both_forms(gpu, swap):
    """Engine._wgrad on a ConvT over a 2 x 32 image: as the stride-2 conv over dy with x as its output
    gradient (k_wgrad2, one K step per image) and as four phases (k_wgrad_lds); both equal the
    reference, hence each other."""
    import torch
    from zebrapose_amd.engine import Act, Engine, Unit
    from zebrapose_amd.model import layers as LY
    c = Case("engine-convT", LDS, BF16, 2, 2, 32, "convT", 64, 64, 64)
    b = c.build()
    conv = LY.ConvTranspose2d(c.Cw, c.Cout, 3, 2, 1, output_padding=1, bias=False).to(gpu)
    unit = Unit(conv, None, relu=False, cin_act=c.Cin)
    eng = Engine(torch.nn.Module(), torch.bfloat16)
    eng.convT_wgrad_swap = swap
    xa = Act(torch.from_numpy(b.x.astype(np.float32)).to(gpu, torch.bfloat16))
    dya = Act(torch.from_numpy(b.dy.astype(np.float32)).to(gpu, torch.bfloat16), 0, c.Cout)
    assert eng._convT_wgrad_swap(unit, xa, dya) == swap
    got = []
    for _ in range(2):
        dw = torch.full_like(conv.weight, WR.GARBAGE)
        eng._wgrad(unit, xa, unit.fwd_plan(c.IH, c.IW), dya, dw)
        torch.cuda.synchronize()
        got.append(dw.cpu().numpy())
    want = b.want()
    assert mismatches(got[0], want) == 0, describe(b, got[0], want)
    assert (bits(got[0]) == bits(got[1])).all()


def _bad_cin(b):
    b.a.Cin = b.a.Cw = 12  # ldx stays 16: only Cin is off the 8-channel chunk


def _bad_lddy(b):
    for s in range(b.a.nsub):
        b.a.sub[s].lddy = b.a.sub[s].cdy0 + WR.roundup(b.a.Cout, 8) - 8


def _bad_cw(b):
    b.a.Cw = b.a.Cin + 1


def _bad_nsub(b):
    b.a.nsub = 0


@pytest.mark.parametrize("spoil", [_bad_cin, _bad_lddy, _bad_cw, _bad_nsub], ids=lambda f: f.__name__[5:])
def test_argument_errors(gpu, spoil):
    """one bad field, valid pointers and sizes everywhere else: ZP_ERR_ARG, and nothing launched"""
    b = Case("args", LDS, BF16, 2, 6, 20, K3, 16, 16, 32).build(gpu)
    spoil(b)
    rc, dw = b.launch()
    assert rc == 1, rc
    assert (bits(dw) == bits(np.float32(WR.GARBAGE))).all(), "dw written by a refused launch"


@pytest.mark.parametrize("c", REAL_CASES, ids=[c.id for c in REAL_CASES])
def test_real_values(gpu, c):
    """N(0, 1) operands (on bf16's grid for bf16, so products are exact in f32): per element
    |got - ref| <= (M + splits) * 2^-23 * sum |dy| |x|, the worst case of any summation order with one
    rounding or truncation per add -- derived, not measured."""
    b = c.build(gpu)
    check_plan(c, b)
    rc, got = b.launch()
    assert rc == 0
    want, lim = b.want(), (b.M + b.splits) * 2.0 ** -23 * b.bound()
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all() and (lim > 0).all()
    ratio = float((err / lim).max())
    print(f"{c.id}: {c.kernel}, M {b.M}, splits {b.splits}, largest |got - ref| / bound = {ratio:.3g}")
    assert ratio <= 1.0, f"{c.id}: |got - ref| reaches {ratio:.3g} of the bound"


def child(run):
    """ENV_RUNS[run]'s cases in this process: one JSON line per case"""
    import torch
    dev = torch.device("cuda:0")
    for c in ENV_RUNS[int(run)][2]:
        b = c.build(dev)
        rc1, got1 = b.launch()
        rc2, got2 = b.launch()
        print(json.dumps({"id": c.id, "rc": [rc1, rc2], "splits": b.splits, "mismatch": mismatches(got1, b.want()),
                          "rerun_differs": int((bits(got1) != bits(got2)).sum())}), flush=True)


def test_env_selected_kernels(gpu):
    """ZP_WGRAD=0 (k_wgrad<bf16_t>) and ZP_WGRAD_BIG=2 (k_wgrad2<4, 4, 2, 2>, the lean 256 x 256 tile):
    read once per process, so one fresh child each, one after the other; the first failure ends it."""
    for run, (extra, kernel, cases) in enumerate(ENV_RUNS):
        env = dict(os.environ, ZP_QUIET="1", **extra)
        r = subprocess.run([sys.executable, "-c", f"from tests.test_gpu_wgrad_edges import child; child({run})"],
                           capture_output=True, text=True, timeout=180, env=env, cwd=ROOT)
        assert r.returncode == 0, (extra, r.returncode, r.stderr[-3000:])
        recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        print(f"{extra} ({kernel}): {recs}")
        assert [x["id"] for x in recs] == [c.id for c in cases]
        for x, c in zip(recs, cases):
            assert x["rc"] == [0, 0] and x["mismatch"] == 0 and x["rerun_differs"] == 0, (extra, x)
            if run == 1:  # the lean kernel keeps its plan on the larger tile: still two splits mid-row
                assert c.splits is None or x["splits"] == c.splits, (extra, x)
