"""The semantics of zp_model_info (include/zp.h) and of metric.add_scores / auc_posecnn, restated in numpy.

``model_info_ref`` is the all-pairs maximum in f64 with the contract's operation order and tie rule,
taken in chunks of rows so that no n x n array is needed.  ``cloud`` builds the test clouds (shared
by the capture tool, the host test and the GPU test, so that recorded and recomputed values belong to
the same points).  ``add_scores_ref`` / ``auc_posecnn_ref`` walk the samples one by one.
"""
import math

import numpy as np

CHUNK = 256


def cloud(kind, n, seed=0):
    """f32 [n, 3].  'uniform': uniform(-100, 100).  'mixed': the same draw with every second point
    scaled by 2^-12 (exact in f32), so that coordinate differences carry more than 26 significant bits
    and the f64 products dx dx are inexact: a fused multiply-add would change the result's bits."""
    rng = np.random.default_rng([seed, n, {"uniform": 0, "mixed": 1}[kind]])
    p = rng.uniform(-100, 100, (n, 3)).astype(np.float32)
    if kind == "mixed":
        p[1::2] *= np.float32(2.0 ** -12)
    return p


def _key(v):
    """Order-preserving int32 key of f32 values: -0 below +0."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.int32)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def box_ref(pts):
    """(min f64 [3], size f64 [3]): the f32 minimum widened, f64(max) - f64(min); -0 orders below +0."""
    p = np.asarray(pts, dtype=np.float32)
    lo = np.array([p[np.argmin(_key(p[:, a])), a] for a in range(3)], dtype=np.float32).astype(np.float64)
    hi = np.array([p[np.argmax(_key(p[:, a])), a] for a in range(3)], dtype=np.float32).astype(np.float64)
    return lo, hi - lo


def model_info_ref(pts):
    """pts f32 [n, 3], finite -> dict(d2max, diameter, pair, min [3], size [3]).
    d2(i, j) = (dx dx + dy dy) + dz dz on the f64 copies, each operation rounded; the maximum runs over
    i <= j; the pair is the lexicographically lowest that attains it."""
    p32 = np.asarray(pts, dtype=np.float32)
    assert p32.ndim == 2 and p32.shape[1] == 3 and len(p32) >= 1 and np.isfinite(p32).all()
    p = p32.astype(np.float64)
    n = len(p)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    best, pair = -1.0, None
    for i0 in range(0, n, CHUNK):
        i1 = min(n, i0 + CHUNK)
        # rows i0 .. i1 against columns i0 .. n; the part of the block below the diagonal is masked out
        dx = x[i0:i1, None] - x[None, i0:]
        dy = y[i0:i1, None] - y[None, i0:]
        dz = z[i0:i1, None] - z[None, i0:]
        d2 = (dx * dx + dy * dy) + dz * dz
        r = np.arange(i1 - i0)
        d2[r[:, None] > np.arange(n - i0)[None, :]] = -1.0
        m = float(d2.max())
        if m > best:  # strictly: an equal maximum in a later chunk has a higher i
            k = int(np.argmax(d2))  # the first in row-major order: lowest i, then lowest j
            best, pair = m, (i0 + k // (n - i0), i0 + k % (n - i0))
    lo, size = box_ref(p32)
    return {"d2max": best, "diameter": math.sqrt(best), "pair": pair, "min": lo, "size": size}


def dx2_inexact(pts, limit=4000):
    """Whether some product dx dx of the cloud's first ``limit`` pairs (x only) is inexact in f64,
    decided in integers: dx = m 2^e is exact (a difference of two f64 copies of f32 values that rounds
    once; taken from the f64 result itself), and its square is exact iff m^2 fits in 53 bits once
    trailing zeros are dropped."""
    x = np.asarray(pts, dtype=np.float32)[:, 0].astype(np.float64)
    seen = 0
    for i in range(len(x)):
        for j in range(i + 1, len(x)):
            dx = float(x[i] - x[j])
            m, _ = math.frexp(dx)
            q = int(abs(m) * (1 << 53))  # the significand as an integer
            sq = q * q
            while sq and sq % 2 == 0:
                sq //= 2
            if sq.bit_length() > 53:
                return True
            seen += 1
            if seen >= limit:
                return False
    return False


def auc_posecnn_ref(errors_m):
    """The area under accuracy over error threshold, 0 .. 0.1 m, times 10, sample by sample."""
    e = sorted(float(v) for v in np.asarray(errors_m, dtype=np.float64).reshape(-1) if not math.isnan(v))
    N = int(np.asarray(errors_m).size)
    kept = [(v, (k + 1) / N) for k, v in enumerate(e) if v <= 0.1]
    if not kept:
        return float("nan")
    area, prev_x, top = 0.0, 0.0, 0.0
    for v, acc in kept + [(0.1, kept[-1][1])]:
        top = max(top, acc)
        if v != prev_x:
            area += (v - prev_x) * top
            prev_x = v
    return area * 10


def add_scores_ref(errors, diameter, success=None, fractions=(0.1, 0.05, 0.02)):
    e = [float(v) for v in np.asarray(errors, dtype=np.float64).reshape(-1)]
    ok = [True] * len(e) if success is None else [bool(s) for s in np.asarray(success).reshape(-1)]
    e = [10000.0 if (not s or math.isnan(v)) else v for v, s in zip(e, ok)]
    steps = [float(t) for t in np.linspace(10, 100, num=10)]
    shares = np.array([sum(v < t for t in steps) / 10 for v in e])
    return {"pass": [float(np.mean([1.0 if v < diameter * f else 0.0 for v in e])) for f in fractions],
            "auc_steps": float(np.mean(shares)),
            "auc_posecnn": auc_posecnn_ref(np.array(e) / 1000.0),
            "mean_error": float(np.mean(e))}
