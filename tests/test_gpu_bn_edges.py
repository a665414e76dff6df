"""The train-mode BatchNorm chain of csrc/zp_bn.hip -- zp_bn_train_finalize, zp_bn_apply, zp_bn_bwd_reduce
(with its totals), zp_bn_bwd_apply -- and the pooled reductions zp_global_avgpool / zp_sum_hw (zp_pool.hip), pinned to
tests/bn_ref.py (numpy f64, stated from include/zp.h) at their edges, straight through the C ABI.

Every buffer lies between two guards; outputs are prefilled with a sentinel, channels of an input outside
its slice hold NaN.  After a call the WHOLE guarded output must be what the reference says: the guards and
everything outside the addressed slice as before.

  exact cases     inputs on which every f32 operation of the header is exact (bn_ref.exact_*; preconditions
                  proved in tests/test_bn_ref_host.py): the device result is fixed whatever the order of
                  summation and is compared bit for bit (the sign of a zero aside: +0 == -0 here, since
                  IEEE leaves the sign of an exact-zero sum to the order of operations)
  rounding cases  random and ill-conditioned values, against bounds derived from the count of f32 roundings
                  on the longest chain (the *_bound functions; never fitted to an output)
zp_bn_apply is one fma, one add, one max and one conversion: restated exactly (bn_ref.apply), so it is bit
for bit on random values too."""
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest

from tests import bn_ref as R
from tests.bn_ref import BF16, F16, F32

pytestmark = pytest.mark.gpu
GUARD, SENT, U = 64, 777.0, 2.0 ** -24
# rounding to the storage type, relative: half an ulp is at most 2^-p of the value, p = 8 (bf16), 11 (fp16) bits
USTORE = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 0.0}


def chunk(kind):
    return 4 if kind == F32 else 8


def _tdt(kind):
    import torch
    return {BF16: torch.bfloat16, F16: torch.float16, F32: torch.float32, "i64": torch.int64}[kind]


def _code(kind):
    from zebrapose_amd import _lib as L
    return L.dtype_code(_tdt(kind))


def _bits(t):
    import torch
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Dev:
    """guarded device buffers: put() uploads a host array between two guards of the sentinel"""

    def __init__(self, device):
        self.device, self.b = device, {}

    def put(self, name, host, kind=F32):
        import torch
        host = np.asarray(host, np.int64 if kind == "i64" else np.float64)
        t = torch.full((2 * GUARD + host.size,), int(SENT) if kind == "i64" else SENT, dtype=torch.from_numpy(host).dtype)
        t[GUARD:GUARD + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1))
        t = t.to(_tdt(kind))
        self.b[name] = (t.to(self.device), t, host.shape)
        return self.b[name][0].data_ptr() + GUARD * t.element_size()

    def out(self, name, shape, kind=F32):
        return self.put(name, np.full(shape, SENT), kind)

    def _host(self, t, shape):
        import torch
        body = t[GUARD:-GUARD]
        return (body.numpy() if body.dtype == torch.int64 else body.to(torch.float64).numpy()).reshape(shape)

    def before(self, name):
        return self._host(self.b[name][1], self.b[name][2]).copy()

    def get(self, name):
        """the body as f64 (int64), after checking both guards bit for bit"""
        dev, was, shape = self.b[name]
        got = dev.cpu()
        assert bool((_bits(got[:GUARD]) == _bits(was[:GUARD])).all() and
                    (_bits(got[-GUARD:]) == _bits(was[-GUARD:])).all()), f"{name}: a guard was overwritten"
        return self._host(got, shape)

    def snapshot(self, name):
        """from here on `name` as it is now is what before() and untouched() mean"""
        dev, _, shape = self.b[name]
        self.b[name] = (dev, dev.cpu(), shape)

    def untouched(self, *names):
        for n in names or [k for k in self.b]:
            dev, was, _ = self.b[n]
            assert bool((_bits(dev.cpu()) == _bits(was)).all()), f"{n}: changed"


def same(got, want, what=""):
    """f32-valued f64 arrays, bit for bit (NaN == NaN, +0 == -0)"""
    g = (np.asarray(got, np.float64) + 0.0).astype(np.float32)
    w64 = np.asarray(want, np.float64) + 0.0
    w = w64.astype(np.float32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert (np.isnan(w64) | (w.astype(np.float64) == w64)).all(), f"{what}: the reference is off f32's grid"
    ne = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    if ne.any():
        idx = np.argwhere(ne)
        raise AssertionError(f"{what}: {len(idx)} of {ne.size} differ; first {idx[:4].tolist()} got "
                             f"{[float(g[tuple(i)]) for i in idx[:4]]} want {[float(w[tuple(i)]) for i in idx[:4]]}")


def within(got, want, bound, what=""):
    got, want, bound = np.broadcast_arrays(np.asarray(got, np.float64), want, bound)
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = np.abs(got - want)
    bad = err > bound
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} beyond the bound; first {i}: got {got[i]!r} "
                             f"want {want[i]!r} err {err[i]:.3g} bound {bound[i]:.3g}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def in_slice(before, c0, val):
    """the buffer [P][ld] as before, channels [c0, c0 + C) replaced by val"""
    w = before.copy()
    w[:, c0:c0 + val.shape[1]] = val
    return w


def sliced(val, ld, c0, fill=np.nan):
    w = np.full((val.shape[0], ld), fill)
    w[:, c0:c0 + val.shape[1]] = val
    return w


def sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ finalize
FIN_PARTS = [1, 3, 127, 128, 129, 511, 512, 513, 577, 1100]   # 577 = 9 * 64 + 1: a last level-1 block of one part
FIN_C = [1, 7, 9, 33, 40]


def run_finalize(gpu, c, mom, bias, nbt, mode, count=None):
    """one zp_bn_train_finalize under zp_conv_tuning(15, mode) -> Dev"""
    from zebrapose_amd import _lib as L
    parts, C = c["cnt"].shape
    d = Dev(gpu)
    nfl = int(L.lib.zp_bn_finalize_floats(parts, C))
    assert nfl == 3 * parts * C + (C + 31) // 32
    body = np.full(nfl, SENT)
    body[:3 * parts * C] = np.stack([c["cnt"], c["mean"], c["m2"]]).reshape(-1)
    args = [d.put("part", body), parts, C, int(count if count is not None else max(1, c["cnt"][:, 0].sum())),
            ctypes.c_float(c["eps"]), ctypes.c_float(mom), d.put("gamma", c["gamma"]), d.put("beta", c["beta"]),
            d.put("bias", c["bias"]) if bias else None, d.put("rm", c["rm"]), d.put("rv", c["rv"]),
            d.put("nbt", [nbt], "i64") if nbt is not None else None, d.out("scale", C), d.out("shift", C),
            d.out("save", (4, C)), L.stream_ptr()]
    old = L.lib.zp_conv_tuning(15, mode)
    try:
        L.call("zp_bn_train_finalize", *args)
        sync()
    finally:
        L.lib.zp_conv_tuning(15, old)
    return d


def check_scratch(d, c, mode, exact):
    """what the header says of the partials buffer: up to 512 parts it is only read; beyond, the first level
    overwrites every 64th part (with its group's merge) and nothing else; the one-launch merge's counters
    past the statistics are zero afterwards, the two-launch form leaves them alone"""
    parts, C = c["cnt"].shape
    got, was = d.get("part"), d.before("part")
    if parts <= 512:
        return d.untouched("part")
    st, st0 = got[:3 * parts * C].reshape(3, parts, C), was[:3 * parts * C].reshape(3, parts, C)
    keep = np.arange(parts) % 64 != 0
    same(st[:, keep], st0[:, keep], "parts off the 64-part grid")
    same(got[3 * parts * C:], np.zeros((C + 31) // 32) if mode else was[3 * parts * C:], "counters")
    if exact:
        for k in range(0, parts, 64):
            n, mu, q = R.merge(c["cnt"][k:k + 64], c["mean"][k:k + 64], c["m2"][k:k + 64])
            same(st[:, k], np.stack([n, mu, q]), f"level-1 part {k}")


@pytest.mark.parametrize("C", FIN_C)
@pytest.mark.parametrize("parts", FIN_PARTS)
def test_finalize_exact(gpu, parts, C):
    """bn_ref.exact_finalize_case: every output bit for bit, in both merge modes beyond 512 parts, with
    momentum 0 / 0.1 / 1, conv_bias and num_batches_tracked NULL and given, running_* preloaded.  At momentum
    0.1 the running statistics are (1 - m) r + m v in f64 rounded once: 1 ulp of f32 (the f64 expression may
    be contracted), bit for bit at 0 and 1 where it is exact."""
    c = R.exact_finalize_case(parts, C)
    for mode in ((0, 1) if parts > 512 else (1,)):
        for mom, bias, nbt in ((0.0, False, None), (0.1, True, 41), (1.0, True, 0)):
            ref = R.finalize(c["cnt"], c["mean"], c["m2"], c["eps"], mom, c["gamma"], c["beta"],
                             c["bias"] if bias else None, c["rm"], c["rv"], nbt)
            d = run_finalize(gpu, c, mom, bias, nbt, mode)
            same(d.get("save"), ref["save"], "save")
            same(d.get("scale"), ref["scale"], "scale")
            same(d.get("shift"), ref["shift"], "shift")
            for k in ("rm", "rv"):
                if mom == 0.1:
                    within(d.get(k), ref[k], 2 * U * np.abs(ref[k]), k)
                else:
                    same(d.get(k), ref[k], k)
            if nbt is not None:
                assert int(d.get("nbt")[0]) == nbt + 1
            d.untouched("gamma", "beta", *(["bias"] if bias else []))
            check_scratch(d, c, mode, exact=True)


def finalize_bound(c, ref, two_level):
    """(mean, invstd, var) error bounds of the saved statistics against the one-level f64 merge `ref`.
    One level (parts <= 512): the merge is f64 throughout -- its own error, at most ~parts * 2^-53 relative
    to sum n_k |m_k| / n, resp. M2, is below a quarter of an f32 ulp for the cases here (mean 1e3 with std
    1e-3 included: the differences m_k - mean are formed in f64 from the given f32 parts) -- then one f32
    rounding: 1 ulp <= 2^-23 |v| covers both.
    Two levels add the f32 write-back of every group's (n, mean, M2): counts are integers, exact; a group
    mean moves by d <= 2^-24 max |m_k| =: D, so the merged mean (a weighted average of them) by <= D; a
    group's M2 by 2^-24 of itself, in sum 2^-24 M2; the cross terms n_g (m_g - mean)^2 see m_g - mean move by
    <= 2 D, so they move by <= sum n_g (4 D |m_g - mean| + 4 D^2) <= 4 D sqrt(n M2) + 4 n D^2 (Cauchy-Schwarz,
    sum n_g (m_g - mean)^2 <= M2).  var = M2 / n; invstd = (var + eps)^-1/2 is monotone, so its error is at
    most its change over [var - e, var + e], plus its own rounding."""
    n, var = ref["n"], ref["var"]
    m2 = var * n
    e_mean = 2 * U * np.abs(ref["mean"])
    e_m2 = 2 * U * m2
    if two_level:
        D = U * np.abs(c["mean"]).max(0)
        e_mean = e_mean + D
        e_m2 = e_m2 + U * m2 + 4 * D * np.sqrt(n * m2) + 4 * n * D * D
    e_var = e_m2 / np.maximum(n, 1)
    eps = float(np.float32(c["eps"]))
    f = lambda v: 1.0 / np.sqrt(np.maximum(v, 0.0) + eps)  # noqa: E731
    e_inv = np.maximum(np.abs(f(var - e_var) - f(var)), np.abs(f(var + e_var) - f(var))) + 2 * U * f(var)
    return e_mean, e_inv, e_var


def rounding_finalize_case(name, parts, C, seed=0):
    rng = np.random.default_rng(7 * parts + C + seed)
    cnt = rng.integers(1, 33, (parts, C)).astype(np.float64)
    mean = R.f32(rng.standard_normal((parts, C)) * 3 + 1)
    m2 = R.f32(rng.random((parts, C)) * cnt * 2)
    if name == "illcond":      # mean 1e3, std 1e-3
        mean = R.f32(1e3 + rng.standard_normal((parts, C)) * 1e-3 / np.sqrt(cnt))
        m2 = R.f32(cnt * 1e-6 * (0.5 + rng.random((parts, C))))
    elif name == "var0":       # every part mean equal, M2 = 0: var = 0, invstd = 1 / sqrt(eps)
        mean = np.tile(R.f32(rng.standard_normal(C) * 5), (parts, 1))
        m2 = np.zeros((parts, C))
    elif name == "empty":      # parts of count 0 holding zeros
        z = rng.random(parts) < 0.4
        z[0] = parts > 1
        z[-1] = False
        cnt[z], mean[z], m2[z] = 0.0, 0.0, 0.0
    elif name == "pixel":      # the whole batch is one pixel
        cnt, mean, m2 = np.zeros((parts, C)), np.zeros((parts, C)), np.zeros((parts, C))
        cnt[parts // 2], mean[parts // 2] = 1.0, R.f32(rng.standard_normal(C))
    return dict(cnt=cnt, mean=mean, m2=m2, eps=1e-5, gamma=R.f32(rng.random(C) + 0.5) * rng.choice([-1.0, 1.0], C),
                beta=R.f32(rng.standard_normal(C)), bias=R.f32(rng.standard_normal(C)),
                rm=R.f32(rng.standard_normal(C)), rv=R.f32(rng.random(C) + 0.5))


@pytest.mark.parametrize("parts,C", [(1, 7), (3, 9), (129, 40), (512, 33), (513, 9), (577, 33), (1100, 40)])
@pytest.mark.parametrize("name", ["random", "illcond", "var0", "empty", "pixel"])
def test_finalize_rounding(gpu, name, parts, C):
    """saved mean / invstd within finalize_bound of the f64 merge; scale, shift and their copies in save
    follow from the device's own mean and invstd by one f32 multiply and one fma, so those are bit for bit
    (stricter than ulps of |mean scale| + |beta|); the running statistics within momentum times the bound
    plus their own rounding.  `count` is not what the merge uses: a wrong one changes nothing."""
    c = rounding_finalize_case(name, parts, C)
    mom = 0.1
    ref = R.finalize(c["cnt"], c["mean"], c["m2"], c["eps"], mom, c["gamma"], c["beta"], c["bias"], c["rm"], c["rv"], 5)
    if name in ("var0", "pixel"):
        assert (ref["var"] <= 1e-12 * np.abs(ref["mean"]) ** 2 + 1e-300).all()
    if name == "pixel":
        assert (ref["n"] == 1).all() and (ref["unb"] == ref["var"]).all()
    for mode in ((0, 1) if parts > 512 else (1,)):
        d = run_finalize(gpu, c, mom, True, 5, mode, count=12345 if name == "random" else None)
        e_mean, e_inv, e_var = finalize_bound(c, ref, parts > 512)
        save = d.get("save")
        r1 = within(save[0], ref["mean"], e_mean, "save mean")
        r2 = within(save[1], ref["invstd"], e_inv, "save invstd")
        sc = R.f32(c["gamma"] * save[1])
        same(save[2], sc, "save scale")
        same(save[3], R.fma32(-save[0], sc, c["beta"]), "save shift")
        same(d.get("scale"), save[2], "scale")
        same(d.get("shift"), save[3], "shift")
        m = float(np.float32(mom))
        want_rm = (1 - m) * c["rm"] + m * (ref["mean"] + c["bias"])
        want_rv = (1 - m) * c["rv"] + m * ref["unb"]
        nn = ref["n"]
        within(d.get("rm"), want_rm, m * e_mean + 2 * U * np.abs(want_rm), "running mean")
        within(d.get("rv"), want_rv, m * e_var * np.where(nn > 1, nn / np.maximum(nn - 1, 1), 1.0) + 2 * U * np.abs(want_rv),
               "running var")
        assert int(d.get("nbt")[0]) == 6
        check_scratch(d, c, mode, exact=False)
        print(f"{name} parts {parts} C {C} mode {mode}: mean {r1:.3g}, invstd {r2:.3g} of the bound")


# ------------------------------------------------------------------------------------------ apply
def apply_case(kind, P, C, seed=0):
    """random x on the storage grid, random f32 scale / shift; planted: fma exactly 0 (channel 0), and the
    residual of a rounded product, +-tiny or 0, which only a fused multiply-add gets right (channels 1, 2)"""
    rng = np.random.default_rng(31 * P + C + seed)
    x = R.to_store(rng.standard_normal((P, C)) * 2, kind)
    sc, sh = R.f32(rng.random(C) + 0.5) * rng.choice([-1.0, 1.0], C), R.f32(rng.standard_normal(C))
    x[0, 0], sc[0], sh[0] = 1.5, 2.0, -3.0
    for ch, sign in ((1, 1.0), (2, -1.0)):
        x[0, ch], sc[ch] = sign * (1 + 2.0 ** -7), 1 + 2.0 ** -20
        sh[ch] = -R.f32(x[0, ch] * sc[ch])
    res = R.to_store(rng.standard_normal((P, C)), kind)
    return x, sc, sh, res


@pytest.mark.parametrize("res,relu,slc", [(False, 1, False), (True, 0, True), (True, 1, True)])
@pytest.mark.parametrize("cn", [1, 3, 32, 256])
@pytest.mark.parametrize("kind", [BF16, F16, F32])
def test_apply_exact(gpu, kind, cn, res, relu, slc):
    """y bit for bit against one fma, one add, one max, one conversion (bn_ref.apply), C / N = 1, 32, 256 on
    the unrolled kernel and 3 on the grid-stride one, P = 1, 5, 1025; the residual read from and y written
    into channel slices of wider buffers"""
    from zebrapose_amd import _lib as L
    N = chunk(kind)
    C = cn * N
    for P in (1, 5, 1025):
        x, sc, sh, r = apply_case(kind, P, C)
        assert R.fma32(x[0, 0], sc[0], sh[0]) == 0 and abs(R.fma32(x[0, 1], sc[1], sh[1])) < 1e-6
        ldr, cr0, ldy, cy0 = (C + 2 * N, N, C + 3 * N, 2 * N) if slc else (C, 0, C, 0)
        d = Dev(gpu)
        L.call("zp_bn_apply", d.put("x", x, kind), P, C, d.put("sc", sc), d.put("sh", sh),
               d.put("res", sliced(r, ldr, cr0), kind) if res else None, ldr if res else 0, cr0 if res else 0, relu,
               _code(kind), d.out("y", (P, ldy), kind), ldy, cy0, L.stream_ptr())
        sync()
        want = R.apply(x, sc, sh, r if res else None, relu, kind)
        same(d.get("y"), in_slice(d.before("y"), cy0, want), f"y P {P}")
        d.untouched("x", "sc", "sh", *(["res"] if res else []))


# ------------------------------------------------------------------------------------------ backward
@functools.lru_cache(None)
def _pix(C):
    from zebrapose_amd import _lib as L
    pix = 1
    while int(L.lib.zp_bn_bwd_parts(pix + 1, C)) == 1:
        pix += 1
        assert pix < 1 << 14
    return pix


def bwd_pix(P, C):
    """(slots, pixels per slot) of zp_bn_bwd_reduce, read back from zp_bn_bwd_parts: pix is the largest P' that
    still takes one slot (the row count is constant over the small pixel counts used here: checked)"""
    from zebrapose_amd import _lib as L
    parts, pix = int(L.lib.zp_bn_bwd_parts(P, C)), _pix(C)
    assert parts == -(-P // pix), (P, C, parts, pix)
    return parts, pix


def sum_bound(term, pix, k):
    """slots and total of f32 sums of `term` [P][C]: a slot is summed over at most pix - 1 f32 adds in some
    order (a thread's chain, then the rows of the block), each rounding <= 2^-24 of a partial sum <= sum |t|
    of the slot; the slot's store and the count of pix instead of pix - 1 make the (ceil(P / parts) + 1) 2^-24
    sum |t| of the issue.  k more roundings are those inside a term, which that count takes as given: 0 for
    g (an input, or 0), 3 for g * xhat = g * ((x - mean) * invstd) (fewer when contracted).  The total is the
    f64 sum of the slots rounded once to f32: the slots' bounds plus 2^-24 |total|."""
    a = np.abs(term)
    slots = np.stack([a[lo:lo + pix].sum(0) for lo in range(0, len(a), pix)]) * (pix + 1 + k) * U
    return slots, slots.sum(0) + U * np.abs(term).sum(0)


def dx_bound(g, xhat, sg, sgx, P, gamma, save, kind):
    """dx = gamma invstd (g - sg / P - xhat sgx / P) in f32 from the f32 totals sg, sgx: 1 / P is rounded (1),
    sg / P is a product (1), xhat = (x - mean) invstd (2), sgx / P (1), their product (1): at most 5 roundings
    on a term; two subtractions (2), gamma invstd (1) and the last product (1): 9 roundings of 2^-24 on
    |gamma invstd| (|g| + |sg / P| + |xhat sgx / P|), taken as 10 for the second-order terms; then the
    storage type's rounding of the result."""
    mag = np.abs(gamma * save[1]) * (np.abs(g) + np.abs(sg / P) + np.abs(xhat * sgx / P))
    return 10 * U * mag, USTORE[kind]


@dataclasses.dataclass
class Bwd:
    kind: str
    relu: int
    dy: np.ndarray
    x: np.ndarray = None
    y: np.ndarray = None
    save: np.ndarray = None
    gamma: np.ndarray = None
    acc: np.ndarray = None       # dgamma / dbeta before the call: accumulate
    dres: np.ndarray = None      # dres before the call
    racc: int = 0
    slices: bool = True
    dgamma: bool = True
    dx: bool = True
    exact: bool = True


def run_bwd(gpu, b):
    """zp_bn_bwd_reduce + zp_bn_bwd_apply of one case, every output against the reference"""
    from zebrapose_amd import _lib as L
    kind, relu, N = b.kind, b.relu, chunk(b.kind)
    P, C = b.dy.shape
    parts, pix = bwd_pix(P, C)
    lddy, cdy0, ldy, cy0, lddres, cdres0 = (C + 2 * N, N, C + N, N, C + 3 * N, 2 * N) if b.slices else (C, 0, C, 0, C, 0)
    d = Dev(gpu)
    st, code = L.stream_ptr(), _code(kind)
    hx = b.x is not None
    pdy = d.put("dy", sliced(b.dy, lddy, cdy0), kind)
    py = d.put("y", sliced(b.y, ldy, cy0), kind) if relu == 1 else None
    px = d.put("x", b.x, kind) if hx else None
    psave = d.put("save", b.save) if hx else None
    acc = b.acc is not None
    pre = b.acc if acc else np.full((2, C), SENT)
    ppart = d.out("part", (2, parts + 1, C))
    pdg = d.put("dgamma", pre[0]) if b.dgamma and hx else None
    pdb = d.put("dbeta", pre[1])
    L.call("zp_bn_bwd_reduce", pdy, lddy, cdy0, py, ldy if relu == 1 else 0, cy0 if relu == 1 else 0, px, P, C, psave,
           relu, code, ppart, pdg, pdb, int(acc), st)
    sync()
    m = R.mask(relu, b.y, b.x, b.save)
    g, xhat, gx = R.bwd_terms(b.dy, m, b.x, b.save)
    part = d.get("part")
    d.snapshot("part")
    ratio = 0.0
    for i, (term, k, out) in enumerate(((g, 0, "dbeta"), (gx, 3, "dgamma"))):
        if term is None:
            continue
        slots, tot = R.bwd_sums(term, pix)
        if b.exact:
            same(part[i, :parts], slots, f"partials[{i}] slots")
            same(part[i, parts], tot, f"partials[{i}] totals row")
        else:
            es, et = sum_bound(term, pix, k)
            ratio = max(ratio, within(part[i, :parts], slots, es, f"partials[{i}] slots"),
                        within(part[i, parts], tot, et, f"partials[{i}] totals row"))
        if out in d.b:   # dgamma / dbeta: the totals row's f32 value, written or added in f32
            row = part[i, parts]
            same(d.get(out), R.rn32_sum(pre[1 - i], row) if acc else row, out)
    d.untouched("dy", *(["y"] if py else []), *(["x", "save"] if hx else []))
    if not (hx and b.dx) and b.dres is None:
        return ratio
    # ---- the apply, from the partials the reduce left
    pdx = d.out("dx", (P, C), kind) if b.dx and hx else None
    pdres = d.put("dres", sliced(b.dres, lddres, cdres0, SENT), kind) if b.dres is not None else None
    pgamma = d.put("gamma", b.gamma) if pdx else None
    L.call("zp_bn_bwd_apply", pdy, lddy, cdy0, py, ldy if relu == 1 else 0, cy0 if relu == 1 else 0, px if pdx else None,
           P, C, psave if pdx else None, ppart if pdx else None, pgamma, relu, code, pdx, pdres,
           lddres if pdres else 0, cdres0 if pdres else 0, b.racc, st)
    sync()
    d.untouched("part", "dy")
    if pdres:
        want = R.to_store(R.rn32_sum(b.dres, g), kind) if b.racc else R.to_store(g, kind)
        same(d.get("dres"), in_slice(d.before("dres"), cdres0, want), "dres")
    if pdx:
        sg, sgx = part[0, parts], part[1, parts]
        want = R.bwd_dx(g, xhat, sg, sgx, b.gamma, b.save)
        if b.exact and P & (P - 1) == 0:
            same(d.get("dx"), R.to_store(want, kind), "dx")
        else:
            e, us = dx_bound(g, xhat, sg, sgx, P, b.gamma, b.save, kind)
            ratio = max(ratio, within(d.get("dx"), want, e + us * (np.abs(want) + e), "dx"))
    return ratio


def bwd_channels(kind):
    N = chunk(kind)
    return [8, 24, 64, 200 * N] + ([2048] if kind == F32 else [])   # f32 2048: two channel groups


@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("kind,C", [(k, c) for k in (BF16, F32) for c in bwd_channels(k)])
def test_backward_exact(gpu, kind, C, relu):
    """bn_ref.exact_bwd_case at P = 1, pix - 1, pix, pix + 1 (a last slot of one row, fewer than the block's
    R wherever R > 1), 2 pix + 3, 2 pix + pix / 8 + 1 (16-bit: a last slot of R / 2 + 1 rows) and 64: slots, totals rows, dgamma /
    dbeta and dres bit for bit; dx bit for bit where P is a power of two (1 / P exact), within dx_bound
    elsewhere.  dy, y and dres are channel slices of wider buffers; dgamma / dbeta accumulate on every other
    P; dres cycles through none / written / accumulated; each (C, relu) also runs dres without dx (relu 0,
    1) and a NULL dgamma."""
    _, pix = bwd_pix(1, C)
    Ps = sorted({1, pix - 1, pix, pix + 1, 2 * pix + 3, 2 * pix + pix // 8 + 1, 64} - {0})
    for i, P in enumerate(Ps):
        c = R.exact_bwd_case(P, C, relu)
        b = Bwd(kind, relu, c["dy"], c["x"], c["y"], c["save"], c["gamma"], acc=c["acc"] if i % 2 else None,
                dres=c["dres"] if i % 3 else None, racc=int(i % 3 == 2))
        run_bwd(gpu, b)
    c = R.exact_bwd_case(pix + 1, C, relu)
    if relu != 2:
        for racc in (0, 1):
            run_bwd(gpu, Bwd(kind, relu, c["dy"], c["x"], c["y"], c["save"], c["gamma"], dres=c["dres"], racc=racc, dx=False))
    run_bwd(gpu, Bwd(kind, relu, c["dy"], c["x"], c["y"], c["save"], c["gamma"], dgamma=False))


@pytest.mark.parametrize("kind,C", [(BF16, 24), (BF16, 64), (F32, 24), (F32, 2048)])
def test_backward_bias_only(gpu, kind, C):
    """the bias gradient of a conv without BatchNorm, exactly as the engine calls it: y, x, save and dgamma
    NULL, ldy = cy0 = 0, relu 0, lddy = C; only sum g is specified then"""
    _, pix = bwd_pix(1, C)
    for P in (1, pix + 1, 2 * pix + 3):
        c = R.exact_bwd_case(P, C, 0)
        run_bwd(gpu, Bwd(kind, 0, c["dy"], slices=False))


def rounding_bwd_case(kind, P, C, relu, seed=0):
    rng = np.random.default_rng(P + 13 * C + relu + seed)
    x = R.to_store(rng.standard_normal((P, C)) * 2 + 0.3, kind)
    mean, inv = R.f32(x.mean(0)), R.f32(1 / np.sqrt(x.var(0) + 1e-5))
    gamma = R.f32(rng.random(C) + 0.5) * rng.choice([-1.0, 1.0], C)
    sc = R.f32(gamma * inv)
    sh = R.fma32(-mean, sc, R.f32(rng.standard_normal(C) * 0.5))
    x[0, 0], sc[0], sh[0] = 1.5, 2.0, -3.0                    # fma exactly 0: masked
    for ch, sign in ((1, 1.0), (2, -1.0)):                     # +-tiny: the sign of the fused residual
        x[0, ch], sc[ch] = sign * (1 + 2.0 ** -7), 1 + 2.0 ** -20
        sh[ch] = -R.f32(x[0, ch] * sc[ch])
    save = np.stack([mean, inv, sc, sh])
    y = R.apply(x, sc, sh, None, 1, kind)
    y[1, :4] = [0.0, -0.0, 0.0, -0.0]                          # y == +0 and -0 under rule 1
    return dict(dy=R.to_store(rng.standard_normal((P, C)), kind), x=x, y=y, save=save, gamma=gamma,
                dres=R.to_store(rng.standard_normal((P, C)), kind))


@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("kind,C", [(BF16, 24), (BF16, 64), (F32, 24), (F32, 64), (F32, 2048)])
def test_backward_rounding(gpu, kind, C, relu):
    """random values: slots and totals within sum_bound, dx within dx_bound of the f64 expression on the
    device's own totals, dres (the masked dy, or one f32 add) bit for bit"""
    _, pix = bwd_pix(1, C)
    P = 2 * pix + 3
    c = rounding_bwd_case(kind, P, C, relu)
    r = run_bwd(gpu, Bwd(kind, relu, c["dy"], c["x"], c["y"], c["save"], c["gamma"], dres=c["dres"], racc=relu % 2,
                         exact=False))
    print(f"{kind} C {C} relu {relu} P {P}: largest error / bound {r:.3g}")


def test_composed_conv_to_backward(gpu):
    """a small zp_conv2d with `stats` (tests/conv_ref.py, the t-m129 case of test_gpu_conv_edges) -> finalize
    -> apply -> backward, each stage against bn_ref on the conv's stored output: pins the formats handed from
    the pinned producer to the consumers ([3][parts][C] statistics, save[4][C], partials[2][parts + 1][C])"""
    from zebrapose_amd import _lib as L
    from tests.test_gpu_conv_edges import BY_ID, stat_bound
    case = dataclasses.replace(BY_ID["t-m129"], kw=dict(BY_ID["t-m129"].kw, stats=True))
    b = case.build(gpu)
    assert b.launch() == 0
    C, P = b.a.Cout, b.M
    parts = int(L.lib.zp_conv2d_stat_parts(ctypes.byref(b.a)))
    stats, ok = b.read("stats", (3, parts, C))
    assert ok and parts <= 512
    x = b.stored(0).reshape(P, C)                       # the conv's stored bf16 output: small integers
    y0, ok = b.read("y", (P, C))
    assert ok and (y0 == x).all()
    rng = np.random.default_rng(3)
    c = dict(cnt=stats[0].astype(np.float64), mean=stats[1].astype(np.float64), m2=stats[2].astype(np.float64), eps=1e-5,
             gamma=R.f32(rng.random(C) + 0.5), beta=R.f32(rng.standard_normal(C)), bias=None,
             rm=np.zeros(C), rv=np.ones(C))
    d = run_finalize(gpu, c, 0.1, False, 0, 1, count=P)
    save = d.get("save")
    # against the plain statistics of the stored output: the parts' own error (stat_bound of the producer's
    # test: 32 * 2^-24 V on a part mean, which moves n (m_k - mean)^2 by <= n 4 V e) plus finalize_bound
    V = float(np.abs(x).max())
    em, eq = stat_bound(x, 128)
    ref = dict(n=np.full(C, float(P)), mean=x.mean(0), var=x.var(0))
    assert (c["cnt"].sum(0) == P).all()
    e_mean, _, _ = finalize_bound(c, ref, False)
    within(save[0], ref["mean"], e_mean + em, "mean of the stored output")
    e_var = (parts * eq + P * 4 * V * em) / P + 2 * U * ref["var"]
    f = lambda v: 1.0 / np.sqrt(np.maximum(v, 0.0) + float(np.float32(1e-5)))  # noqa: E731
    within(save[1], f(ref["var"]), np.maximum(np.abs(f(ref["var"] - e_var) - f(ref["var"])),
                                              np.abs(f(ref["var"] + e_var) - f(ref["var"]))) + 2 * U * f(ref["var"]), "invstd")
    same(save[2], R.f32(c["gamma"] * save[1]), "scale")
    same(save[3], R.fma32(-save[0], save[2], c["beta"]), "shift")
    d2 = Dev(gpu)
    L.call("zp_bn_apply", d2.put("x", x, BF16), P, C, d2.put("sc", d.get("scale")), d2.put("sh", d.get("shift")), None, 0, 0,
           1, _code(BF16), d2.out("y", (P, C), BF16), C, 0, L.stream_ptr())
    sync()
    y = R.apply(x, save[2], save[3], None, 1, BF16)
    same(d2.get("y"), y, "y")
    dy = rng.integers(-3, 4, (P, C)).astype(np.float64)
    for relu in (1, 2):
        run_bwd(gpu, Bwd(BF16, relu, dy, x, y, save, c["gamma"], exact=False))


# ------------------------------------------------------------------------------------------ refusals
def _bwd_args(gpu, kind, P, C, relu):
    """valid arguments of both entries on sentinel-filled buffers large enough for every spoiled call"""
    from zebrapose_amd import _lib as L
    N = chunk(kind)
    ld, c0 = C + 2 * N, N
    d = Dev(gpu)
    parts = int(L.lib.zp_bn_bwd_parts(P, C))
    io = {k: d.out(k, (P, ld), kind) for k in ("dy", "y", "dres")}
    x, dx = d.out("x", (P, C), kind), d.out("dx", (P, C), kind)
    save, part, gamma = d.out("save", (4, C)), d.out("part", (2, parts + 1, C)), d.out("gamma", C)
    dg, db = d.out("dgamma", C), d.out("dbeta", C)
    red = dict(dy=io["dy"], lddy=ld, cdy0=c0, y=io["y"], ldy=ld, cy0=c0, x=x, P=P, C=C, save=save, relu=relu,
               dtype=_code(kind), partials=part, dgamma=dg, dbeta=db, accumulate=0, stream=L.stream_ptr())
    app = dict(dy=io["dy"], lddy=ld, cdy0=c0, y=io["y"], ldy=ld, cy0=c0, x=x, P=P, C=C, save=save, partials=part,
               gamma=gamma, relu=relu, dtype=_code(kind), dx=dx, dres=io["dres"], lddres=ld, cdres0=c0, racc=0,
               stream=L.stream_ptr())
    return d, red, app


# (name, spoiled arguments from (N, C), the entries that must refuse: r(educe) / a(pply))
SPOIL = [("cdy0", lambda N, C: dict(cdy0=N // 2), "ra"), ("lddy", lambda N, C: dict(lddy=C + 2 * N + 1), "ra"),
         ("cy0", lambda N, C: dict(cy0=N // 2), "ra"), ("ldy", lambda N, C: dict(ldy=C + 2 * N + N // 2), "ra"),
         ("cdres0", lambda N, C: dict(cdres0=N // 2), "a"), ("lddres", lambda N, C: dict(lddres=C + 2 * N + 1), "a"),
         ("cn257", None, "ra"), ("fp16", None, "ra"), ("relu2-no-x", lambda N, C: dict(relu=2, x=None), "r"),
         ("relu2-no-dx", lambda N, C: dict(relu=2, dx=None), "a"), ("relu1-no-y", lambda N, C: dict(y=None), "ra")]


@pytest.mark.parametrize("name,over,who", SPOIL, ids=[s[0] for s in SPOIL])
@pytest.mark.parametrize("kind", [BF16, F32])
def test_backward_refusals(gpu, kind, name, over, who):
    """one argument that ZP_CHECK_ARG rejects before any launch (read in the wrappers), valid pointers and
    sizes otherwise (relu 1, so y is read): ZP_ERR_ARG from zp_bn_bwd_reduce (r) / zp_bn_bwd_apply (a), no
    buffer touched.  Offsets are spoiled by half a vector (16-bit: the 4-aligned slices zp_conv2d accepts),
    leading dimensions by one element or half a vector."""
    from zebrapose_amd import _lib as L
    N = chunk(kind)
    P, C = 5, 8 * N
    if name == "cn257":
        C = 257 * N
    d, red, app = _bwd_args(gpu, kind, P, C, 1)
    if name == "fp16":
        red["dtype"] = app["dtype"] = L.ZP_F16
    elif over:
        over = over(N, C)
        red.update({k: v for k, v in over.items() if k in red})
        app.update({k: v for k, v in over.items() if k in app})
    if "r" in who:
        assert L.lib.zp_bn_bwd_reduce(*red.values()) == 1, name
    if "a" in who:
        assert L.lib.zp_bn_bwd_apply(*app.values()) == 1, name
    sync()
    d.untouched()


def test_backward_accepts_the_engines_forms(gpu):
    """the alignment checks leave the engine's calls alone: channel slices on vector boundaries, and the
    bias-only call with ldy = cy0 = lddres = cdres0 = 0 and NULL pointers"""
    from zebrapose_amd import _lib as L
    for kind in (BF16, F32):
        d, red, app = _bwd_args(gpu, kind, 5, 8 * chunk(kind), 0)
        red.update(y=None, ldy=0, cy0=0, x=None, save=None, dgamma=None)
        assert L.lib.zp_bn_bwd_reduce(*red.values()) == 0
        app.update(y=None, ldy=0, cy0=0, dres=None, lddres=0, cdres0=0)
        assert L.lib.zp_bn_bwd_apply(*app.values()) == 0
        sync()


# ------------------------------------------------------------------------------------------ pooled reductions
def pool_bound(x, PL, kind):
    """zp_sum_hw of HW values per channel in f32: a pixel lane adds ceil(HW / PL) values, then PL lane sums
    are added in order: at most ceil(HW / PL) + PL roundings of 2^-24 on partial sums <= sum |x|; then the
    storage type's rounding of the result"""
    HW = x.shape[1]
    a = np.abs(x).sum(1)
    return (math.ceil(HW / PL) + PL) * U * a


@pytest.mark.parametrize("form", ["vec", "scalar"])
@pytest.mark.parametrize("kind", [BF16, F16, F32])
def test_pooled_reductions(gpu, kind, form):
    """zp_global_avgpool (f64 mean -> f32 -> storage type, both roundings restated; inputs on a 1/16 grid so
    the f64 sum is exact in any order) bit for bit; zp_sum_hw bit for bit on integers and within pool_bound
    on random values; HW around the pixel-lane count PL and its 4-deep unrolled loop, C with a block-of-64
    tail, a slice at c0 > 0; the scalar form on C = 20 at c0 = 2 (4 pixel slices per block).  fp16: the
    average only (zp_sum_hw is a training entry)."""
    from zebrapose_amd import _lib as L
    N = chunk(kind)
    PL = (32 if N == 8 else 16) if form == "vec" else 4
    shapes = [(C, C + 2 * N, N) for C in (8, 72, 64 + N)] if form == "vec" else [(20, 24, 2), (70, 75, 3)]
    B, code, st = 2, _code(kind), L.stream_ptr()
    rng = np.random.default_rng(5)
    for HW in sorted({1, PL - 1, PL, 4 * PL - 1, 4 * PL, 4 * PL + 1, 8 * PL + 3} - {0}):
        for C, ld, c0 in shapes:
            d = Dev(gpu)
            grid = rng.integers(-64, 65, (B, HW, C)) / 16.0
            ints = rng.integers(-3, 4, (B, HW, C)).astype(np.float64)
            real = R.to_store(rng.standard_normal((B, HW, C)), kind)
            ptr = {n: d.put(n, np.stack([sliced(v[b], ld, c0) for b in range(B)]), kind)
                   for n, v in (("grid", grid), ("ints", ints), ("real", real))}
            L.call("zp_global_avgpool", ptr["grid"], B, 1, HW, ld, c0, C, code, d.out("avg", (B, C), kind), st)
            if kind != F16:
                L.call("zp_sum_hw", ptr["ints"], B, HW, 1, ld, c0, C, code, d.out("isum", (B, C), kind), st)
                L.call("zp_sum_hw", ptr["real"], B, 1, HW, ld, c0, C, code, d.out("rsum", (B, C), kind), st)
            sync()
            what = f"{kind} {form} HW {HW} C {C}"
            same(d.get("avg"), R.avgpool(grid, kind), "avg " + what)
            if kind != F16:
                same(d.get("isum"), R.to_store(R.sum_hw(ints), kind), "sum " + what)
                want = R.sum_hw(real)
                e = pool_bound(real, PL, kind)
                within(d.get("rsum"), want, e + USTORE[kind] * (np.abs(want) + e), "sum " + what)
            d.untouched("grid", "ints", "real")
