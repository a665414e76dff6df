"""zp_adam, zp_adam_multi and zp_adam_multi_dev (csrc/zp_adam.hip) pinned to tests/adam_ref.py bit for bit,
straight through the C ABI.  adam_ref is torch.optim.Adam's single-tensor step with every rounding stated
(tests/test_adam_ref_host.py holds it to torch); comparisons are on uint32 views, NaNs as NaN-ness.

The operands are one tensor built from the cross product of value classes -- gradients from 0 over
denormals to 2e19 and 1e25 (where (w2 * g) * g overflows: exp_avg_sq and denom become inf, the update 0), moments and
parameters at 0, denormal and normal, exp_avg_sq == 0 with grad == 0 (denom == eps), one NaN and one inf
gradient -- followed by ordinary normal draws; it is repeated to the length a case needs.  Three
consecutive steps feed the state forward.  A multi call's tensors are carved from one allocation per
operand with guard words between them: the guards, the elements past each tensor's end and the gradients
must come back as they were."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import adam_ref as R

pytestmark = pytest.mark.gpu

HYPER = {"lr4e-4_b0.9": (4e-4, 0.9, 0.999, 1e-8), "lr1e-2_b0.3": (1e-2, 0.3, 0.9, 1e-8)}
STARTS = [1, 2, 1000, 10 ** 6]
GUARD, TAIL = 16, 7                      # guard words between tensors; elements past n inside a slot
GUARD_BITS = 0x7FC0BEEF                  # a NaN with a payload: any arithmetic on it would change the bits
DEN = 1e-40                              # a denormal f32


@functools.lru_cache(maxsize=None)
def base():
    """(p, g, m, v) f32: the cross product of the value classes, the specials, then normal draws"""
    gs = [0.0, DEN, -DEN, 1e-20, -1e-20, 1.0, -1.0, 3e18, -3e18, 2e19, -2e19,
          1e25, -1e25]  # (w2 * g) * g overflows only here: 2e19 squared does, but w2 comes first
    ms = [0.0, DEN, 1.0, -1.0]
    vs = [0.0, 1e-42, 1.0, 1e30]
    ps = [0.0, 1.0, -1e-30]
    rows = list(itertools.product(ps, gs, ms, vs))
    rows += [(1.0, np.nan, 0.5, 0.25), (1.0, np.inf, 0.5, 0.25)]
    a = np.array(rows, np.float32)
    rng = np.random.default_rng(11)
    k = 294
    r = np.stack([rng.standard_normal(k), rng.standard_normal(k) * np.exp(rng.uniform(-6, 2, k)),
                  rng.standard_normal(k) * 0.1, rng.standard_normal(k) ** 2 * 1e-3], 1).astype(np.float32)
    a = np.concatenate([a, r])
    return tuple(np.ascontiguousarray(a[:, i]) for i in range(4))


def grads(step_index):
    """the gradient of the step_index-th consecutive step: the base gradient, rolled"""
    return np.roll(base()[1], 37 * step_index)


@functools.lru_cache(maxsize=None)
def reference(hyper, start):
    """states after each of three steps on the base tensor: [(p, m, v)] * 3"""
    lr, b1, b2, eps = HYPER[hyper]
    p, _, m, v = base()
    out = []
    for i in range(3):
        p, m, v = R.step(p, grads(i), m, v, lr, b1, b2, eps, start + i)
        out.append((p, m, v))
    return out


def tiled(a, n, off=0):
    return np.resize(np.roll(a, -off), n) if n else np.zeros(0, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    bad = R.mismatches(got, want)
    assert bad.size == 0, (what, f"{bad.size} of {np.size(want)} differ", bad[:6].tolist(),
                           np.asarray(got).ravel()[bad[:6]].tolist(), np.asarray(want).ravel()[bad[:6]].tolist(),
                           [hex(x) for x in _bits(got).ravel()[bad[:6]]], [hex(x) for x in _bits(want).ravel()[bad[:6]]])


class Arena:
    """One allocation per operand holding `sizes` tensors: slot i = n_i elements, TAIL more elements past
    the end, GUARD guard words.  Tensor i starts `off_i` elements into the base pattern."""

    def __init__(self, device, sizes):
        import torch
        self.torch, self.device, self.sizes = torch, device, list(sizes)
        self.starts, pos = [], GUARD
        for n in self.sizes:
            self.starts.append(pos)
            pos += n + TAIL + GUARD
        self.total = pos
        self.offs = [(131 * i) % base()[0].size for i in range(len(self.sizes))]
        self.host = {}
        self.dev = {}
        for k, name in enumerate("pgmv"):
            self.fill(name, lambda i, n, k=k: tiled(base()[k], n + TAIL, self.offs[i]))

    def fill(self, name, fn):
        h = np.full(self.total, GUARD_BITS, np.uint32).view(np.float32)
        for i, (s, n) in enumerate(zip(self.starts, self.sizes)):
            h[s:s + n + TAIL] = fn(i, n)
        self.host[name] = h
        self.dev[name] = self.torch.from_numpy(h.copy()).to(self.device)

    def set_grad(self, step_index):
        g = grads(step_index)
        self.fill("g", lambda i, n: tiled(g, n + TAIL, self.offs[i]))

    def ptrs(self, name):
        b = self.dev[name].data_ptr()
        return (C.c_void_p * max(1, len(self.sizes)))(*[b + 4 * s for s in self.starts])

    def numel(self):
        return (C.c_longlong * max(1, len(self.sizes)))(*self.sizes)

    def expect(self, ref):
        """apply the reference state (p, m, v on the base tensor) to the host copies"""
        for name, r in zip("pmv", ref):
            for i, (s, n) in enumerate(zip(self.starts, self.sizes)):
                self.host[name][s:s + n] = tiled(r, n, self.offs[i])

    def check(self, what):
        self.torch.cuda.synchronize()
        for name in "pgmv":
            assert_bits(self.dev[name].cpu().numpy(), self.host[name], (what, name))


def _single(L, ar, i, hyper, step):
    lr, b1, b2, eps = HYPER[hyper]
    a = [ar.dev[k].data_ptr() + 4 * ar.starts[i] for k in "pgmv"]
    L.call("zp_adam", a[0], a[1], a[2], a[3], ar.sizes[i], lr, b1, b2, eps, step, L.stream_ptr())


def _multi(L, ar, hyper, step, count=None, step_dev=None):
    lr, b1, b2, eps = HYPER[hyper]
    count = len(ar.sizes) if count is None else count
    args = [count] + [ar.ptrs(k) if count else None for k in "pgmv"] + [ar.numel() if count else None, lr, b1, b2, eps]
    if step_dev is None:
        L.call("zp_adam_multi", *args, step, L.stream_ptr())
    else:
        L.call("zp_adam_multi_dev", *args, step_dev.data_ptr(), L.stream_ptr())


SINGLE_SIZES = [1, 255, 256, 257, 4095, 4096, 4097]


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("hyper", list(HYPER))
def test_adam_single(gpu, hyper, start):
    from zebrapose_amd import _lib as L
    ar = Arena(gpu, SINGLE_SIZES)  # the sizes side by side in one allocation: a stray store shows next door
    for s in range(3):
        ar.set_grad(s)
        for i in range(len(SINGLE_SIZES)):
            _single(L, ar, i, hyper, start + s)
        ar.expect(reference(hyper, start)[s])
        ar.check(("zp_adam", hyper, start + s))


@pytest.mark.parametrize("hyper", list(HYPER))
def test_adam_single_grid_stride_wraps(gpu, hyper):
    """16384 blocks of 256 threads is the grid's cap: 257 elements more and the loop takes a second turn"""
    from zebrapose_amd import _lib as L
    ar = Arena(gpu, [16384 * 256 + 257])
    for s in range(3):
        ar.set_grad(s)
        _single(L, ar, 0, hyper, 1 + s)
        ar.expect(reference(hyper, 1)[s])
        ar.check(("zp_adam wrap", hyper, 1 + s))


def multi_sizes(count):
    """tensor sizes around the 4096-element block of k_adam_multi; positions 39 and 40 are empty"""
    cyc = [4095, 4096, 4097, 1, 8193, 257, 4096 * 3, 12289]
    sizes = [cyc[i % len(cyc)] for i in range(count)]
    for i in (39, 40):
        if i < count:
            sizes[i] = 0
    return sizes


@pytest.mark.parametrize("count", [0, 1, 40, 41, 81])
@pytest.mark.parametrize("hyper", list(HYPER))
def test_adam_multi(gpu, hyper, count):
    from zebrapose_amd import _lib as L
    ar = Arena(gpu, multi_sizes(count))
    one = Arena(gpu, multi_sizes(count)) if count in (41, 81) else None  # the same tensors through zp_adam
    for s in range(3):
        ar.set_grad(s)
        _multi(L, ar, hyper, 1000 + s)
        ar.expect(reference(hyper, 1000)[s])
        ar.check(("zp_adam_multi", hyper, count, 1000 + s))
        if one is not None:
            one.set_grad(s)
            for i, n in enumerate(one.sizes):
                if n:
                    _single(L, one, i, hyper, 1000 + s)
            one.torch.cuda.synchronize()
            for name in "pmv":
                assert_bits(ar.dev[name].cpu().numpy(), one.dev[name].cpu().numpy(), ("multi vs zp_adam", name, s))


def test_adam_multi_zero_count_touches_nothing(gpu):
    from zebrapose_amd import _lib as L
    ar = Arena(gpu, multi_sizes(3))
    _multi(L, ar, "lr4e-4_b0.9", 1, count=0)
    ar.check("count 0")


@pytest.mark.parametrize("start", STARTS + [2 ** 24])
@pytest.mark.parametrize("hyper", list(HYPER))
def test_adam_multi_dev(gpu, hyper, start):
    """the step count as an f32 device scalar: the host-step form's bits, and the reference's"""
    import torch
    from zebrapose_amd import _lib as L
    sizes = multi_sizes(42)
    dev, host = Arena(gpu, sizes), Arena(gpu, sizes)
    step_dev = torch.zeros(1, dtype=torch.float32, device=gpu)
    for s in range(3 if start < 2 ** 24 else 1):  # (2^24 + 1 is no f32)
        step_dev.fill_(float(start + s))
        assert int(step_dev.item()) == start + s
        for ar in (dev, host):
            ar.set_grad(s)
        _multi(L, dev, hyper, 0, step_dev=step_dev)
        _multi(L, host, hyper, start + s)
        torch.cuda.synchronize()
        lr, b1, b2, eps = HYPER[hyper]
        print("adam_multi_dev", hyper, start + s, "constants", R.constants(lr, b1, b2, eps, start + s))
        for name in "pmv":
            assert_bits(dev.dev[name].cpu().numpy(), host.dev[name].cpu().numpy(), ("dev vs host step", name, start + s))
        dev.expect(reference(hyper, start)[s])
        dev.check(("zp_adam_multi_dev", hyper, start + s))
