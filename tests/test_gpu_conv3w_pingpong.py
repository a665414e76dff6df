"""The ping-pong K loop of the wide two-plane tile (k_conv3w / k_conv3w_head, zp_conv_tuning key 22):
the two wave groups of a workgroup run half a K step apart.  Every wave keeps its K order, its
per-step flush and its split-K slice, so each launch must store the same bits under key 22 = 0
(the lock-step loop) and key 22 = 1, both planes, and raise the same range-guard word.

Shapes are the smallest that reach every branch of the loop (one 256 x 256 tile is 8 waves; key 11 = 1
lets the dispatch take the wide tile on these small grids): odd and even step counts, two cout
tiles, dilation with out-of-image taps, the widest strip (GW 128), the fused head tail, split-K
slices, and the ConvT phases (1 / 2 / 4 taps: they keep the lock-step loop whatever the key says).
Inputs are ReLU'd (exact zeros); one case scales a BN channel so that its outputs straddle the
two-plane range limit (|v| >= 65520 raises the guard, tests/test_gpu_range.py)."""
import pytest
import torch

from tests.test_gpu_x3 import BOUND, _ref64, _split_act

pytestmark = pytest.mark.gpu

PP_KEY = 22

CASES = {
    # kind, cin, cout, d, B, H, W
    "one_tile_9_steps": ("conv", 32, 256, 1, 1, 16, 16),
    "one_tile_18_steps": ("conv", 64, 256, 1, 1, 16, 16),
    "two_cout_tiles": ("conv", 64, 512, 1, 1, 16, 16),
    "dilation4_edges": ("conv", 64, 256, 4, 2, 32, 32),
    "wide_strip_gw128": ("conv", 32, 256, 1, 1, 4, 128),
    "convT_phases": ("convT", 64, 256, 1, 1, 16, 16),
}


def _unit(gpu, kind, cin, cout, d, seed, guard_edge=False):
    from zebrapose_amd.engine import Unit
    from zebrapose_amd.model import layers as LY
    torch.manual_seed(seed)
    if kind == "conv":
        conv = LY.Conv2d(cin, cout, 3, 1, d, d, bias=False)
    else:
        conv = LY.ConvTranspose2d(cin, cout, 3, 2, 1, output_padding=1, bias=False)
    bn = LY.BatchNorm2d(cout)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.1)
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
        if guard_edge:  # channel 3's outputs (the conv's are of order 0.3 here) straddle 65520
            bn.weight[3] = 2.0e5
    return Unit(conv.to(gpu).eval(), bn.to(gpu).eval(), relu=True), conv, bn


def _both_keys(eng, gpu, run):
    """run() under key 22 = 0 and = 1 -> {key: (stored planes, guard word, kernel names)}."""
    from zebrapose_amd import _lib as L
    got = {}
    old11 = L.lib.zp_conv_tuning(11, 1)
    try:
        for key in (0, 1):
            old = L.lib.zp_conv_tuning(PP_KEY, key)
            word = L.range_flag(gpu)  # the word direct launches raise (whoever registered it: restored below)
            saved = word.clone()
            try:
                word.zero_()
                eng.stage_log = []
                planes = run()
                torch.cuda.synchronize()
                raised = int(word.item())
            finally:
                word.copy_(saved)
                L.lib.zp_conv_tuning(PP_KEY, old)
            got[key] = ([p.clone() for p in planes], raised, [r[1] for r in eng.stage_log])
    finally:
        L.lib.zp_conv_tuning(11, old11)
    return got


def _assert_same(got, what):
    (p0, w0, n0), (p1, w1, n1) = got[0], got[1]
    assert n0 == n1, (what, n0, n1)
    assert w0 == w1, (what, "range-guard word", w0, w1)
    for a, b in zip(p0, p1):
        assert torch.equal(a, b), (what, int((a != b).sum()), a.numel())


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_pingpong_is_bit_identical(gpu, case):
    from zebrapose_amd.engine import Engine, Act
    kind, cin, cout, d, B, H, W = CASES[case]
    guard_edge = case == "one_tile_18_steps"
    unit, conv, bn = _unit(gpu, kind, cin, cout, d, 21, guard_edge)
    OH, OW = unit.out_hw(H, W)
    x = torch.randn(B, cin, H, W).clamp(min=0)  # exact zeros
    res = torch.randn(B, cout, OH, OW) if kind == "conv" else None
    eng = Engine(torch.nn.Module(), torch.float32, split="h2")
    xa = Act(_split_act(x.permute(0, 2, 3, 1).contiguous(), gpu, "h2"))
    ra = None if res is None else Act(_split_act(res.permute(0, 2, 3, 1).contiguous(), gpu, "h2"))

    def run():
        oa = Act(eng._empty((B, OH, OW, cout), gpu))
        oa.buf._base.zero_()
        eng.unit_fwd(unit, xa, oa, None, res=ra)
        return [oa.buf._base]
    got = _both_keys(eng, gpu, run)
    print(case, got[0][2], "guard", got[0][1])
    assert got[0][2] == ["k_conv3w<h2>"], got[0][2]
    _assert_same(got, case)
    if guard_edge:
        j = got[1][0][0][0].float() + got[1][0][0][1].float() / 2048.0
        assert got[1][1] != 0 and bool((j[..., 3] < 60000).any()), "channel 3 should straddle the range limit"
    else:
        assert got[1][1] == 0


def test_pingpong_is_f32_accurate(gpu):
    """The 18-step tile under key 22 = 1 against float64, within the two-plane bound of
    tests/test_gpu_x3.py (BOUND["h2"]: 4 x the exact-f32-MFMA kernel's error + 2^-21 of the scale)."""
    from zebrapose_amd import _lib as L
    from zebrapose_amd.engine import Engine, Act, joined
    kind, cin, cout, d, B, H, W = CASES["one_tile_18_steps"]
    unit, conv, bn = _unit(gpu, kind, cin, cout, d, 22)
    x = torch.randn(B, cin, H, W).clamp(min=0)
    res = torch.randn(B, cout, H, W)
    ref = _ref64(kind, conv, bn, x, res, True, 1, d, d)
    xh, rh = x.permute(0, 2, 3, 1).contiguous(), res.permute(0, 2, 3, 1).contiguous()
    err = {}
    old11, old = L.lib.zp_conv_tuning(11, 1), L.lib.zp_conv_tuning(PP_KEY, 1)
    try:
        for mode in ("h2", "f32"):
            if mode == "h2":
                eng = Engine(torch.nn.Module(), torch.float32, split="h2")
                xa, ra = Act(_split_act(xh, gpu, "h2")), Act(_split_act(rh, gpu, "h2"))
                oa = Act(eng._empty((B, H, W, cout), gpu))
            else:
                eng = Engine(torch.nn.Module(), torch.float32)
                xa, ra = Act(xh.to(gpu)), Act(rh.to(gpu))
                oa = Act(torch.empty(B, H, W, cout, device=gpu))
            eng.stage_log = []
            eng.unit_fwd(unit, xa, oa, None, res=ra)
            torch.cuda.synchronize()
            if mode == "h2":
                assert [r[1] for r in eng.stage_log] == ["k_conv3w<h2>"]
            err[mode] = (joined(oa.buf).permute(0, 3, 1, 2).double().cpu() - ref).abs().max().item()
    finally:
        L.lib.zp_conv_tuning(11, old11)
        L.lib.zp_conv_tuning(PP_KEY, old)
    scale = ref.abs().max().item()
    print(f"ping-pong 64 -> 256: max|d| two-plane {err['h2']:.3g} f32-MFMA {err['f32']:.3g} (scale {scale:.3g})")
    mult, floor = BOUND["h2"]
    assert err["h2"] <= mult * err["f32"] + floor * scale, (err, scale)


def test_pingpong_split_k_is_bit_identical(gpu):
    """bs 2 at 64 x 64, 256 -> 256: 32 tiles, which the plan cuts along K (4 slices of 18 steps; only
    the split makes this grid eligible for the wide tile at the default key 11).  The slices' raw sums
    and k_splitk_epi's result are the same under both keys."""
    from zebrapose_amd import _lib as L
    from zebrapose_amd.engine import Engine, Act
    unit, conv, bn = _unit(gpu, "conv", 256, 256, 1, 23)
    B, H = 2, 64
    x = torch.randn(B, 256, H, H).clamp(min=0)
    eng = Engine(torch.nn.Module(), torch.float32, split="h2")
    xa = Act(_split_act(x.permute(0, 2, 3, 1).contiguous(), gpu, "h2"))
    got = {}
    for key in (0, 1):
        old = L.lib.zp_conv_tuning(PP_KEY, key)
        try:
            oa = Act(eng._empty((B, H, H, 256), gpu))
            eng.stage_log = []
            eng.unit_fwd(unit, xa, oa, None)
            torch.cuda.synchronize()
        finally:
            L.lib.zp_conv_tuning(PP_KEY, old)
        got[key] = ([oa.buf._base.clone()], 0, [r[1] for r in eng.stage_log])
    assert got[0][2] == ["k_conv3w<h2>"], got[0][2]
    _assert_same(got, "split-K")


def test_pingpong_fused_head_is_bit_identical(gpu):
    """256 -> 256 3x3 + the 1x1 head over [conv | 64 skip channels] -> 17 at bs 1, 16 x 16 (one tile:
    the head weights are staged over the rings after the loop's last barrier)."""
    from zebrapose_amd.engine import Engine, Unit, Act
    from zebrapose_amd.model import layers as LY
    unit, conv, bn = _unit(gpu, "conv", 256, 256, 1, 24)
    torch.manual_seed(25)
    head = Unit(LY.Conv2d(320, 17, 1, 1, 0, 1, bias=True).to(gpu).eval(), None, relu=False)
    B, H = 1, 16
    x = torch.randn(B, 256, H, H).clamp(min=0)
    x2 = torch.randn(B, 64, H, H).clamp(min=0)
    eng = Engine(torch.nn.Module(), torch.float32, split="h2")
    xa = Act(_split_act(x.permute(0, 2, 3, 1).contiguous(), gpu, "h2"))
    x2a = Act(_split_act(x2.permute(0, 2, 3, 1).contiguous(), gpu, "h2"))

    def run():
        mask = torch.zeros((B, 1, H, H), dtype=torch.float32, device=gpu)
        code = torch.zeros((B, 16, H, H), dtype=torch.float32, device=gpu)
        eng.unit_fwd_head(unit, xa, head, x2a, mask, code)
        return [mask, code]
    got = _both_keys(eng, gpu, run)
    print(got[0][2])
    assert len(got[0][2]) == 1 and got[0][2][0].startswith("k_conv3w_head"), got[0][2]
    assert float(got[0][0][1].abs().max()) > 0
    _assert_same(got, "fused head")
