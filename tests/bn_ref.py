"""Train-mode BatchNorm as include/zp.h states it, in numpy f64: the reference of zp_bn_train_finalize,
zp_bn_apply, zp_bn_bwd_reduce (with its totals), zp_bn_bwd_apply and of the pooled reductions
zp_global_avgpool / zp_sum_hw.  Stated from the header, not from the kernels; reads nothing but its
arguments.

Rounding points (f32 unless said otherwise), as the header gives them:
  finalize   Chan's merge of the parts (count n_k, mean m_k, centred M2 q_k) in f64:
               n = sum n_k, mean = sum n_k m_k / n, M2 = sum q_k + sum n_k (m_k - mean)^2
             (with `level1` = R the parts are first merged in groups of R and each group's (n, mean, M2)
             is rounded to f32, the in-place first level of more than 512 parts); var = M2 / n (biased);
             save = (f32 mean, invstd = f32(1 / sqrt(var + eps)), scale = f32(gamma * invstd),
             shift = fma(-mean, scale, beta)); running mean <- (1 - m) rm + m (mean + conv bias),
             running var <- (1 - m) rv + m var n / (n - 1) (n == 1: var), both formed in f64 and rounded once
  apply      y = store(max(fma(x, scale, shift) (+ res), 0))   one fma, one add, one max, one conversion
  backward   g = dy * mask; mask: none | y > 0 | fma(x, save scale, save shift) > 0 (so y == +-0 is masked);
             xhat = (x - mean) * invstd; slots and totals of g and g * xhat; dgamma = sum g xhat, dbeta = sum g;
             dx = gamma * invstd * (g - sum_g / P - xhat * sum_gx / P); dres = g
The backward functions return unrounded f64 values: the GPU tests compare them bit for bit where the
inputs make every f32 operation exact and within derived bounds elsewhere."""
import numpy as np

BF16, F16, F32 = "bf16", "f16", "f32"


def f32(v):
    """round to nearest even onto f32's grid, kept as f64"""
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def ident(v):
    return np.asarray(v, np.float64)


def to_store(v, kind):
    """f64 -> f32 -> the storage type `kind` (both roundings to nearest even; finite values), kept as f64"""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    if kind == BF16:
        u = v32.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(v32.shape)
    if kind == F16:
        return v32.astype(np.float16).astype(np.float64)
    return v32.astype(np.float64)


def rn32_sum(a, b):
    """RN_f32(a + b) of f64 arrays, one rounding of the exact sum: TwoSum gives the f64 sum s and its exact
    error e; s is then rounded to odd (truncated towards zero, lowest bit set when e != 0), and a value
    rounded to odd at 53 bits rounds to nearest at 24 bits as the exact sum does (53 >= 24 + 2)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    inexact = e != 0
    down = inexact & ((e > 0) != (s > 0))      # the exact sum is nearer zero than s: one step towards zero
    bits = np.where(down, bits - 1, bits)      # (sign-magnitude: -1 shortens either sign; s != 0 when e != 0)
    bits = np.where(inexact, bits | 1, bits)
    return bits.view(np.float64).astype(np.float32).astype(np.float64)


def fma32(x, a, b):
    """fma(x, a, b) in f32 for f32-valued operands: x * a is exact in f64 (48 bits), the sum rounded once"""
    x, a, b = (np.asarray(v, np.float64) for v in (x, a, b))
    assert (f32(x) == x).all() and (f32(a) == a).all() and (f32(b) == b).all()
    return rn32_sum(x * a, b)


# ---------------------------------------------------------------------------------------- finalize
def merge(cnt, mean, m2, level1=0, rnd=f32):
    """Chan's merge of parts [parts][C] -> (n, mean, M2) [C] in f64; level1 = R: groups of R parts first,
    each rounded to f32 (rnd) as the in-place first level stores it"""
    cnt, mean, m2 = (np.asarray(v, np.float64) for v in (cnt, mean, m2))
    if level1:
        groups = [merge(cnt[k:k + level1], mean[k:k + level1], m2[k:k + level1]) for k in range(0, len(cnt), level1)]
        cnt, mean, m2 = (rnd(np.stack([g[i] for g in groups])) for i in range(3))
    n = cnt.sum(0)
    mu = np.where(n > 0, (cnt * mean).sum(0) / np.where(n > 0, n, 1.0), 0.0)
    q = (m2 + cnt * (mean - mu) ** 2).sum(0)
    return n, mu, q


def finalize(cnt, mean, m2, eps, momentum, gamma, beta, bias=None, rm=None, rv=None, nbt=None, level1=0, rnd=f32):
    """zp_bn_train_finalize -> dict(n, mean, var: unrounded f64; save [4][C], scale, shift, rm, rv, nbt).
    rnd=ident drops the f32 roundings (the comparison with torch in float64)."""
    n, mu, q = merge(cnt, mean, m2, level1, rnd)
    var = np.maximum(np.where(n > 0, q / np.where(n > 0, n, 1.0), 0.0), 0.0)
    eps, mom = float(rnd(eps)), float(rnd(momentum))
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    m32 = rnd(mu)
    invstd = rnd(1.0 / np.sqrt(var + eps))
    scale = rnd(gamma * invstd)
    shift = fma32(-m32, scale, beta) if rnd is f32 else beta - m32 * scale
    out = dict(n=n, mean=mu, var=var, invstd=1.0 / np.sqrt(var + eps), scale=scale, shift=shift,
               save=np.stack([m32, invstd, scale, shift]))
    mt = mu + (0.0 if bias is None else np.asarray(bias, np.float64))
    unb = np.where(n > 1, var * n / np.where(n > 1, n - 1.0, 1.0), var)
    if rm is not None:
        out["rm"] = rnd((1.0 - mom) * np.asarray(rm, np.float64) + mom * mt)
        out["rv"] = rnd((1.0 - mom) * np.asarray(rv, np.float64) + mom * unb)
    out["unb"] = unb
    out["nbt"] = None if nbt is None else int(nbt) + 1
    return out


def parts_of(x, bounds):
    """(count, mean, centred M2) [parts][C] of the pixel ranges [lo, hi) of x [P][C]; an empty range: zeros"""
    x = np.asarray(x, np.float64)
    cnt, mean, m2 = (np.zeros((len(bounds), x.shape[1])) for _ in range(3))
    for k, (lo, hi) in enumerate(bounds):
        if hi > lo:
            cnt[k] = hi - lo
            mean[k] = x[lo:hi].mean(0)
            m2[k] = ((x[lo:hi] - mean[k]) ** 2).sum(0)
    return cnt, mean, m2


# ---------------------------------------------------------------------------------------- apply
def apply(x, scale, shift, res=None, relu=0, kind=F32):
    """zp_bn_apply on f32-valued x [P][C] (values of the storage type), exactly: the stored y as f64"""
    o = fma32(x, scale, shift)
    if res is not None:
        o = rn32_sum(o, res)
    if relu:
        o = np.maximum(o, 0.0) + 0.0
    return to_store(o, kind)


# ---------------------------------------------------------------------------------------- backward
def mask(relu, y=None, x=None, save=None):
    """the three mask rules -> bool [P][C] (None: no mask)"""
    if relu == 0:
        return None
    if relu == 1:
        return np.asarray(y, np.float64) > 0            # +0 and -0 are both masked
    return fma32(x, save[2], save[3]) > 0               # as zp_bn_apply formed y, before the store


def bwd_terms(dy, m, x=None, save=None):
    """g [P][C], xhat and g * xhat (None without x), f64"""
    g = np.asarray(dy, np.float64) if m is None else np.where(m, dy, 0.0)
    if x is None:
        return g, None, None
    xhat = (np.asarray(x, np.float64) - save[0]) * save[1]
    return g, xhat, g * xhat


def bwd_sums(term, pix):
    """slots [parts][C] of `pix` pixels and the total [C]"""
    P = len(term)
    slots = np.stack([term[lo:lo + pix].sum(0) for lo in range(0, P, pix)])
    return slots, term.sum(0)


def bwd_dx(g, xhat, sum_g, sum_gx, gamma, save):
    """dx = gamma * invstd * (g - sum_g / P - xhat * sum_gx / P), f64"""
    P = float(len(g))
    return np.asarray(gamma, np.float64) * save[1] * (g - sum_g / P - xhat * (sum_gx / P))


# ---------------------------------------------------------------------------------------- pooled reductions
def avgpool(x, kind):
    """zp_global_avgpool of x [B][HW][C]: f64 mean -> f32 -> storage type"""
    return to_store(f32(np.asarray(x, np.float64).mean(1)), kind)


def sum_hw(x):
    """zp_sum_hw of x [B][HW][C] before any rounding"""
    return np.asarray(x, np.float64).sum(1)


# ---------------------------------------------------------------------------------------- exact cases
# Inputs on which every f32 operation the header describes is exact, so the device result is fixed
# whatever the order of summation; tests/test_bn_ref_host.py proves the preconditions on each draw.
def exact_finalize_case(parts, C, seed=0):
    """parts of count 4 with integer means base_c +- j in cancelling pairs (so every group of 64 parts and
    the whole have mean base_c) and integer M2 chosen to make var 16 or 64: with eps = 0 invstd is 1/4 or
    1/8, gamma a power of two, beta an integer"""
    rng = np.random.default_rng(1000 * parts + C + seed)
    d = np.zeros(parts)
    j = np.arange(parts // 2)
    d[0:2 * (parts // 2):2] = 1 + j % 3
    d[1:2 * (parts // 2):2] = -(1 + j % 3)
    base = rng.integers(-5, 6, C).astype(np.float64)
    sign = rng.choice([-1.0, 1.0], C)
    cnt = np.full((parts, C), 4.0)
    mean = base + d[:, None] * sign
    var = rng.choice([16.0, 64.0], C)
    rest = var * 4 * parts - (4 * d ** 2).sum()
    m2 = np.tile(np.floor(rest / parts), (parts, 1))
    m2[0] += rest - m2.sum(0)
    assert (m2 >= 0).all()
    return dict(cnt=cnt, mean=mean, m2=m2, eps=0.0, gamma=rng.choice([0.5, 1.0, 2.0], C) * rng.choice([-1.0, 1.0], C),
                beta=rng.integers(-4, 5, C).astype(np.float64), bias=rng.integers(-3, 4, C).astype(np.float64),
                rm=rng.integers(-8, 9, C).astype(np.float64), rv=rng.integers(1, 9, C).astype(np.float64))


def exact_bwd_case(P, C, relu, seed=0):
    """dy, x in +-{0..3}, y in {-1, -0, +0, 1, 2}, save = (integer mean, invstd in {1/2, 1, 2}, scale +-{1/2, 1,
    2}, integer shift), gamma +-{1/2, 1, 2}: all on bf16's grid; g * xhat is a multiple of 1/2 below 32"""
    rng = np.random.default_rng(100003 * P + 17 * C + relu + seed)
    pm = lambda n: rng.choice([-1.0, 1.0], n)  # noqa: E731
    save = np.stack([rng.integers(-2, 3, C).astype(np.float64), rng.choice([0.5, 1.0, 2.0], C),
                     rng.choice([0.5, 1.0, 2.0], C) * pm(C), rng.integers(-2, 3, C).astype(np.float64)])
    return dict(dy=rng.integers(-3, 4, (P, C)).astype(np.float64), x=rng.integers(-3, 4, (P, C)).astype(np.float64),
                y=rng.choice([-1.0, -0.0, 0.0, 1.0, 2.0], (P, C)), save=save,
                gamma=rng.choice([0.5, 1.0, 2.0], C) * pm(C),
                acc=rng.integers(-9, 10, (2, C)).astype(np.float64),          # dgamma / dbeta before an accumulate
                dres=rng.integers(-3, 4, (P, C)).astype(np.float64))          # dres before res_accumulate
