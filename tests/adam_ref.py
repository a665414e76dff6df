"""One step of torch.optim.Adam (_single_tensor_adam: no weight decay, amsgrad off, not capturable) in
numpy float32, every operation rounded as torch's CPU build rounds it.  tests/test_adam_ref_host.py pins
this restatement to torch bit for bit; tests/test_gpu_adam_edges.py pins csrc/zp_adam.hip to it.

The sequence, with w1 = f32(1 - beta1), w2 = f32(1 - beta2), b2 = f32(beta2), a = f32(-lr / bc1),
s = f32(bc2 ** 0.5), bc = 1 - beta ** step in double:

  exp_avg.lerp_(grad, w1)       ATen's vectorised lerp is ONE fused multiply-add on (end - self):
                                  w1 <  0.5:  m' = fma(w1,              g - m, m)
                                  w1 >= 0.5:  m' = fma(f32(w1 - 1.0f),  g - m, g)
  exp_avg_sq.mul_(beta2)        t  = v * b2
          .addcmul_(g, g, w2)   v' = fma(w2 * g, g, t)       (the products left to right, the add fused)
  denom                         d  = sqrt(v') / s + f32(eps)  (three roundings)
  param.addcdiv_(m', d, a)      p' = p + (a * m') / d         (the product first, then the quotient, then
                                                               the sum: three roundings, nothing fused)

The fused multiply-adds are computed exactly: the product of two f32 is exact in f64, one f64 add follows
and the sum is rounded to f32.  That double rounding can only differ from the single one when the f64 sum
lies within one f64 ulp of the midpoint of two neighbouring f32 (below 2^-29 of elements); those elements
are redone in rational arithmetic (fractions).

Denormals.  torch's CPU kernels keep IEEE gradual underflow and so does this module: nothing is flushed
to zero.  A gradient scale of 1e-22, where a * m' and v' are denormal, is bit exact against torch like the
normal-range scales (tests/test_adam_ref_host.py keeps it in the exact set).

The square root.  IEEE 754 requires sqrt to be correctly rounded; numpy's float32 sqrt is, and so is the
kernel's.  torch's CPU build is NOT in its vectorised loop body: about 0.7 % of float32 elements come out
one ulp off the correctly rounded root, while the same value in the scalar tail of the same tensor is exact
(torch 2.10, AVX-512 build).  That is the whole residue a restatement with the IEEE root leaves against
torch: exp_avg and exp_avg_sq agree on every bit, `denom` inherits the ulp, and it survives the final add
in roughly one element of 10^5.  step() therefore takes the root as an argument: the default is the
IEEE root (what csrc/zp_adam.hip is held to), and the host test passes torch's own sqrt to prove that
every other rounding of the step is torch's, with no element excluded."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

f32 = np.float32


def _round_exact(p, c, s):
    """f32 nearest-even of the exact p + c for the elements whose f64 sum s lies within one f64 ulp of
    the midpoint of two neighbouring f32 (p, c, s: f64 arrays; p + c rounded to s)"""
    with np.errstate(all="ignore"):
        r = s.astype(f32)
        lo = np.nextafter(r, f32(-np.inf)).astype(np.float64)
        hi = np.nextafter(r, f32(np.inf)).astype(np.float64)
        r64 = r.astype(np.float64)
        ulp = np.spacing(np.abs(s))
        near = np.isfinite(s) & np.isfinite(r64) & (
            (np.isfinite(lo) & (np.abs(s - (r64 + lo) * 0.5) <= ulp)) |
            (np.isfinite(hi) & (np.abs(s - (r64 + hi) * 0.5) <= ulp)))
    for i in np.flatnonzero(near):
        exact = Fraction(float(p.flat[i])) + Fraction(float(c.flat[i]))
        cands = sorted({float(lo.flat[i]), float(r64.flat[i]), float(hi.flat[i])})
        # nearest of the three neighbours, ties to the even significand
        best = min(cands, key=lambda q: (abs(Fraction(q) - exact), int(np.array(q, f32).view(np.uint32)) & 1))
        r.flat[i] = f32(best)
    return r


def fma(a, b, c):
    """fl32(a * b + c) with one rounding, elementwise on f32 arrays"""
    a, b, c = (np.asarray(t, f32).astype(np.float64) for t in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
    return _round_exact(p, c, s)


def constants(lr, beta1, beta2, eps, step):
    """the f32 scalars of one step: (w1, b2, w2, a, s, eps)"""
    bc1 = 1.0 - beta1 ** float(step)
    bc2 = 1.0 - beta2 ** float(step)
    return (f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(-(lr / bc1)), f32(bc2 ** 0.5), f32(eps))


def step(p, g, m, v, lr, beta1, beta2, eps, step, sqrt=np.sqrt):
    """(p', m', v') of one Adam step; inputs f32 arrays, left unchanged.  sqrt: the f32 root of an f32 array
    (default: the correctly rounded one)"""
    p, g, m, v = (np.asarray(t, f32) for t in (p, g, m, v))
    w1, b2, w2, a, s, e = constants(lr, beta1, beta2, eps, step)
    with np.errstate(all="ignore"):
        d = g - m
        if w1 < f32(0.5):
            m1 = fma(w1, d, m)
        else:
            m1 = fma(f32(w1 - f32(1.0)), d, g)
        v1 = fma(w2 * g, g, v * b2)
        den = np.asarray(sqrt(v1), f32) / s + e
        p1 = p + (a * m1) / den
    return p1, m1, v1


def mismatches(a, b):
    a, b = np.asarray(a, f32).ravel(), np.asarray(b, f32).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return np.flatnonzero((na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32))))


def same_bits(a, b):
    """bit for bit, NaNs compared as NaN-ness"""
    return np.shape(a) == np.shape(b) and mismatches(a, b).size == 0
