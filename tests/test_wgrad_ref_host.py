"""tests/wgrad_ref.py validated on the CPU, and the preconditions of tests/test_gpu_wgrad_edges.py.

ref() against torch's f64 autograd weight gradient (F.conv2d / F.conv_transpose2d) on random real
operands, to 1e-12 relative: strides 1 and 2, dilations 1 and 6, kernels 1 / 3 / 7, non-square images,
channel slices and a padded Cin; the four-phase ConvT plan; and the swap form, the stride-2 conv over
the ConvT's dy with its x as the output gradient, which lands in the ConvT weight's own layout.

For every entry of the GPU case table: no operand is zero and sum |dy| |x| < 2^24 per element of dw
(so every partial sum of the integers is exact in f32, whatever the order); the kernel the plan's
eligibility rule takes and the split count are the ones the case is sized for.  The split counts are
the plan's for 256 compute units, which the library also assumes without a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_ref as WR
from tests.test_gpu_wgrad_edges import CASES, ENV_RUNS, REAL_CASES, Case, check_plan, tuned
from tests.wgrad_ref import BF16, F32
from zebrapose_amd import geometry as G


def _nchw(v):
    return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))


def _close(got, want):
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


CONVS = [  # k, s, p, d, IH, IW
    (1, 1, 0, 1, 5, 7), (3, 1, 1, 1, 6, 9), (3, 2, 1, 1, 7, 10), (3, 1, 6, 6, 9, 14), (3, 2, 6, 6, 11, 15),
    (7, 2, 3, 1, 13, 18), (7, 1, 3, 1, 8, 5), (1, 2, 0, 1, 6, 9),
]


@pytest.mark.parametrize("k,s,p,d,IH,IW", CONVS, ids=[f"k{c[0]}s{c[1]}p{c[2]}d{c[3]}-{c[4]}x{c[5]}" for c in CONVS])
def test_ref_is_conv2d_weight_gradient(k, s, p, d, IH, IW):
    Cin, Cw, Cout, cx0, cdy0 = 8, 5, 6, 8, 4
    b = WR.build(F32, 2, IH, IW, G.conv_fwd(IH, IW, k, s, p, d), Cin, Cw, Cout, kh=k, kw=k, cx0=cx0, ldx=24,
                 cdy0=cdy0, lddy=16, values="real", seed=k + s)
    w = torch.zeros(Cout, Cw, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(_nchw(b.x[..., cx0:cx0 + Cw]), w, None, s, p, d).backward(_nchw(b.dy[..., cdy0:cdy0 + Cout]))
    _close(b.want(), w.grad.numpy())


def test_ref_is_convT_weight_gradient_by_phases():
    Cin, Cout = 8, 6
    b = WR.build(F32, 2, 5, 9, G.convT_fwd(5, 9), Cin, Cin, Cout, kh=3, kw=3, transposed_w=1, values="real", seed=1)
    assert b.a.nsub == 4 and b.dy.shape[1:3] == (10, 18)
    w = torch.zeros(Cin, Cout, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(_nchw(b.x), w, None, 2, 1, 1).backward(_nchw(b.dy[..., :Cout]))
    _close(b.want(), w.grad.numpy())


def test_ref_is_convT_weight_gradient_by_swap():
    # the launch's x is the ConvT's dy (10 x 18, 8 channels), its dy the ConvT's x (5 x 9, 4 channels)
    ct_in, ct_out = 4, 8
    b = WR.build(F32, 2, 10, 18, G.convT_dgrad(5, 9), ct_out, ct_out, ct_in, kh=3, kw=3, values="real", seed=2)
    assert (b.a.GH, b.a.GW, b.a.sy) == (5, 9, 2) and b.dy.shape[1:3] == (5, 9)
    w = torch.zeros(ct_in, ct_out, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(_nchw(b.dy[..., :ct_in]), w, None, 2, 1, 1).backward(_nchw(b.x))
    _close(b.want(), w.grad.numpy())


def test_ref_pixel_subsets_add_up():
    b = Case("t", "k_wgrad_lds", BF16, 3, 5, 16, (3, 1, 1, 1), 8, 3, 16).build()
    m = np.arange(b.M) < 100
    part = WR.ref(b.a, b.x, b.dys, m) + WR.ref(b.a, b.x, b.dys, ~m)
    assert (part == b.want()).all() and np.abs(WR.ref(b.a, b.x, b.dys, m)).max() > 0


ALL = CASES + REAL_CASES + [c for _, _, cs in ENV_RUNS for c in cs if c not in CASES]


@pytest.mark.parametrize("c", ALL, ids=[c.id for c in ALL])
def test_case_preconditions(c):
    with tuned(c.tuning):
        b = c.build()
        if c in CASES or c in REAL_CASES:
            check_plan(c, b)
    a, E = b.a, WR.chunk(c.dtype)
    # the operand windows hold no zero and no NaN; everything outside them is NaN
    xin = b.x[..., a.cx0:a.cx0 + a.Cin]
    cr = WR.roundup(a.Cout, E)
    dyin = b.dy[..., a.sub[0].cdy0:a.sub[0].cdy0 + cr]
    for v in (xin, dyin):
        assert np.isfinite(v).all() and (v != 0).all()
    assert np.isnan(b.x).sum() == b.x.size - xin.size and np.isnan(b.dy).sum() == b.dy.size - dyin.size
    assert a.Cin % E == 0 and a.cx0 % E == 0 and a.ldx % E == 0 and a.sub[0].lddy >= a.sub[0].cdy0 + cr
    if c.values == "real":
        return
    # integers whose every partial sum stays below 2^24 (dw's pre-fill included when accumulating)
    for v in (xin, dyin, b.dw0):
        assert (v == np.rint(v)).all()
    assert c.dtype == F32 or c.wide is None
    assert np.abs(xin).max() <= (4095 if c.wide == "x" else 3) and np.abs(dyin).max() <= (4095 if c.wide == "dy" else 3)
    top = b.bound() + (np.abs(b.dw0) if a.accumulate else 0)
    assert top.max() < 2 ** 24 and np.abs(b.want()).max() < 2 ** 24
    if c.dtype == F32:
        assert c.wide in ("x", "dy") and b.M <= 1024
