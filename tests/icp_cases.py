"""Deterministic ICP inputs shared by tests/test_icp_cases_host.py (the preconditions, on the oracle
tests/icp_ref.py alone) and tests/test_gpu_icp_edges.py (the device).  Plain numpy, no GPU.

Every builder returns a case: dict(name, src [ns, 3], dst [nd, 3] (the two point lists), us, ud (the
draws of both subsamples, [N]), R, t (the pose that goes in), N, kw (zp_icp's remaining arguments:
max_iterations, tolerance, mode, min_fraction, angle_limit), hits (what the case is meant to reach)).
`run(case)` is the oracle on it.  Coordinates that have to tie or cancel exactly are small integers
and halves, so that they do so in f64 whatever the order of summation.
"""
import numpy as np

from tests import icp_ref as IR
from tests import refine_ref as RF
from tests.test_icp_host import cloud, moved

R0 = RF.rodrigues([1, 2, 3], 0.4)
T0 = np.array([1.0, 2.0, 500.0])
CENTRE = np.array([3.0, -4.0, 600.0])

SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 3073, 4096)
# (n, N): n = N at every size; n < N with n below / at / above a template boundary (N = 1024 k) while N
# lies in another template, a thread's later slots past n (1025 of 2049), whole idle waves (1 of 64,
# 3 of 1025, 63 of 1024, 65 of 4096), and the smallest sets in the largest template
SIZE_PAIRS = tuple((n, n) for n in SIZES) + (
    (1, 64), (2, 4096), (3, 1025), (63, 1024), (65, 4096), (1023, 1024), (1023, 1025), (1024, 1025), (1025, 2049),
    (2049, 3073), (1024, 3073), (3073, 4096))


def identity_draws(n, N=None):
    """draw i picks point i of an n-point list; entries from n on (never read) are 0.5"""
    u = np.full(N or n, 0.5)
    u[:n] = (np.arange(n) + 0.5) / n
    return u


def case(name, src, dst, us, ud, hits, N=None, R=R0, t=T0, **kw):
    us, ud = np.asarray(us, np.float64), np.asarray(ud, np.float64)
    return dict(name=name, src=np.asarray(src, np.float64).reshape(-1, 3), dst=np.asarray(dst, np.float64).reshape(-1, 3),
                us=us, ud=ud, R=R, t=t, N=N or len(us), kw=kw, hits=hits)


def run(c, **over):
    kw = dict(c["kw"], **over)
    return IR.icp_pose(c["src"], c["dst"], c["us"], c["ud"], c["R"], c["t"], N=c["N"], **kw)


# ---- one fit: clouds by the rank and conditioning of H ---------------------------------------------

def shaped(name, extents, seed, n=200, deg=1.0, hits=""):
    """n normal points scaled to `extents` along three generic orthogonal axes, and the same cloud
    turned by `deg` degrees about its centroid, shifted and given noise of 1e-3 of the smallest
    non-zero extent, in another order.  H of the fit is (cloud scatter) R^T up to the noise: its
    singular values go as the squares of the extents."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(extents, np.float64)
    Q = RF.rodrigues(rng.normal(size=3), rng.uniform(0.5, 2.0))
    A = (rng.normal(size=(n, 3)) * ext) @ Q.T + CENTRE
    B = moved(A, rng.normal(size=3), deg, [0.02, -0.015, 0.025])[0]
    B = B + ((rng.normal(size=B.shape) * (ext > 0)) @ Q.T) * 1e-3 * ext[ext > 0].min()
    perm = rng.permutation(n)
    return case(name, A, B[perm], identity_draws(n), identity_draws(n), hits, max_iterations=1)


def fit_cases():
    """name -> (case, the s2 / s1 its H is built for, or None): the clouds whose rotation is unique,
    held to fit_bound"""
    return {
        "full": (shaped("full", (40, 30, 20), 1, hits="full rank, well conditioned"), None),
        "planar": (shaped("planar", (40, 30, 0), 2, hits="rank 2: s3 = 0 up to rounding, v3 = v1 x v2"), None),
        "thin_1e-2": (shaped("thin_1e-2", (40, 4, 0.4), 3, hits="s2 / s1 = 1e-2"), 1e-2),
        "thin_1e-4": (shaped("thin_1e-4", (40, 0.4, 0.04), 4, hits="s2 / s1 = 1e-4"), 1e-4),
        "thin_1e-6": (shaped("thin_1e-6", (40, 0.04, 0.004), 5, hits="s2 / s1 = 1e-6: H^T H holds 1e-12 beside 1"), 1e-6),
        "thin_1e-6_planar": (shaped("thin_1e-6_planar", (40, 0.04, 0), 6, hits="s2 / s1 = 1e-6 and s3 = 0"), 1e-6),
        "needle_1e-2": (shaped("needle_1e-2", (40, 4, 3.9), 7, hits="s2 / s1 = 1e-2, s2 ~ s3"), 1e-2),
        "needle_1e-6": (shaped("needle_1e-6", (40, 0.04, 0.039), 8, hits="s2 / s1 = 1e-6, s2 ~ s3"), 1e-6),
    }


def sized(n, N):
    """A generic cloud for the sizes: the source list has exactly n points when n < N (a short count
    list), n + 5 otherwise; the destination list n + 9, a second draw of the distribution, moved, with
    noise (tests/test_gpu_icp.py's pair()).  n = 1, 2, 3 give H of rank 0, 1, 2."""
    rng = np.random.default_rng(100 * n + N)
    ns = n if n < N else n + 5
    A = cloud(n, ns)
    # n <= 3: the same points moved, so that every point's neighbour is its own image and the rank n - 1
    Bm = moved(cloud(n if n <= 3 else n + 1000, n + 9), rng.normal(size=3), 4.0, (2.0, -1.5, 2.5))[0]
    Bm = Bm + rng.normal(size=Bm.shape) * 0.3
    us, ud = np.full(N, 0.5), np.full(N, 0.5)
    us[:n], ud[:n] = rng.random(n), rng.random(n)
    if n <= 3:  # point i of both lists
        us[:n], ud[:n] = (np.arange(n) + 0.5) / ns, (np.arange(n) + 0.5) / (n + 9)
    return case(f"n{n}_N{N}", A, Bm, us, ud, f"n = {n} of N = {N}", N=N, max_iterations=1)


def collinear_exact():
    """Eight source points c + k d, k = -7, -5 .. 7, d = (1, 2, 2), and eight destination points
    c' + m d', d' = (2, -1, 2): integers, centroids exact, H = (sum k m) d d'^T exactly of rank 1."""
    k = np.arange(-7, 8, 2.0)
    src = CENTRE + k[:, None] * np.array([1.0, 2.0, 2.0])
    dst = CENTRE + np.array([1.0, 0.0, -1.0]) + k[:, None] * np.array([2.0, -1.0, 2.0])
    return case("collinear_exact", src, dst, identity_draws(8), identity_draws(8),
                "rank 1, exactly: the completion axis", max_iterations=1)


def collinear_real(n=65):
    """Points on two generic lines: rank 1 up to the rounding of the coordinates (s2 ~ 1e-16 s1)."""
    rng = np.random.default_rng(31)
    d1, d2 = rng.normal(size=3), rng.normal(size=3)
    src = CENTRE + rng.uniform(-50, 50, n)[:, None] * d1 / np.linalg.norm(d1)
    dst = CENTRE + np.array([1.0, -2.0, 1.5]) + rng.uniform(-50, 50, n + 4)[:, None] * d2 / np.linalg.norm(d2)
    return case("collinear_real", src, dst, identity_draws(n), identity_draws(n + 4)[:n], "rank 1 up to rounding",
                max_iterations=1)


def coincident(which, n=8):
    """Every draw of one side picks point 0: that side's subsample is n copies of one point, its
    centred form exactly 0 (integer coordinates) and H = 0."""
    rng = np.random.default_rng(32)
    src = CENTRE + rng.integers(-30, 30, (n, 3))
    dst = CENTRE + rng.integers(-30, 30, (n + 3, 3)) + np.array([0.5, 0.0, 0.0])
    us, ud = identity_draws(n), identity_draws(n + 3)[:n]
    if which == "src":
        us = np.zeros(n)
    else:
        ud = np.zeros(n)
    return case(f"coincident_{which}", src, dst, us, ud, "H = 0: the identity", max_iterations=1)


def mirrored(n=12):
    """Source point i at (x, 100 i, z), destination point i at (-x, 100 i, z): the levels are 100
    apart, so every neighbour is the point's own mirror image, H has a negative determinant and the
    best orthogonal fit is a reflection.  |x| <= 40 and |z| <= 20: the sign the fix flips (the
    smallest singular value) is z's, distinct from x's."""
    rng = np.random.default_rng(33)
    x, z = rng.uniform(-40, 40, n), rng.uniform(-20, 20, n)
    y = 100.0 * np.arange(n)
    src = CENTRE + np.stack([x, y, z], 1)
    dst = CENTRE + np.stack([-x, y, z], 1) + np.array([1.0, 2.0, -1.5])
    perm = rng.permutation(n)
    return case(f"mirrored_{n}", src, dst[perm], identity_draws(n), identity_draws(n), "reflection: det(U V^T) < 0",
                max_iterations=1)


def degenerate_cases():
    """The inputs whose rotation is not unique (or unique only through the reflection fix): checked by
    value.  name -> (case, rank of H)"""
    return {
        "collinear_exact": (collinear_exact(), 1), "collinear_real": (collinear_real(), 1),
        "coincident_src": (coincident("src"), 0), "coincident_dst": (coincident("dst"), 0),
        "n1_N1": (sized(1, 1), 0), "n1_N64": (sized(1, 64), 0), "n2_N2": (sized(2, 2), 1), "n2_N4096": (sized(2, 4096), 1),
        "mirrored_12": (mirrored(12), 3), "mirrored_200": (mirrored(200), 3),
    }


# ---- draws, loop exits, status boundaries --------------------------------------------------------------

def draw_ends():
    """A 19-point and a 21-point list drawn 16 times each, with every end of draw_index on both sides."""
    one = 1.0 - 2.0 ** -53
    ends = [0.0, one, 1.0, 1.5, 1e300, np.inf, -1e-300, -0.5, -np.inf, -0.0, np.nan, 0.5, 1.0 / 19, 1.0 / 21, 18.0 / 19, 20.0 / 21]
    src, dst = cloud(41, 19), moved(cloud(41, 21), [0.3, 0.1, 0.9], 3.0, (1.0, 0.5, -1.0))[0]
    return case("draw_ends", src, dst, ends, ends[::-1], "draw_index at 0, 1 - 2^-53, 1, above 1, negative, NaN",
                max_iterations=1)


def _loop_pair(seed=11, n=100):
    rng = np.random.default_rng(seed)
    A = cloud(seed, n + 5)
    Bm = moved(cloud(seed + 1000, n + 9), rng.normal(size=3), 4.0, (2.0, -1.5, 2.5))[0] + rng.normal(size=(n + 9, 3)) * 0.3
    return A, Bm, rng.random(n), rng.random(n)


def loop_cases():
    """name -> (case, the iteration count it is built for; None: whatever the default loop takes, more
    than 3 and fewer than max_iterations)"""
    A, Bm, us, ud = _loop_pair()
    sub = cloud(51, 60)
    return {
        "default": (case("default", A, Bm, us, ud, "the loop breaks on |prev - mean| < 5e-7"), None),
        "tolerance_0": (case("tolerance_0", A, Bm, us, ud, "|prev - mean| < 0 never holds: runs to max_iterations",
                             max_iterations=300, tolerance=0.0), 300),
        "tolerance_negative": (case("tolerance_negative", A, Bm, us, ud, "nor below a negative tolerance",
                                    max_iterations=7, tolerance=-1.0), 7),
        "tolerance_inf": (case("tolerance_inf", A, Bm, us, ud, "any finite change is below +inf: one iteration",
                               max_iterations=50, tolerance=np.inf), 1),
        # every source point is a destination point, bit for bit: every distance and the mean are 0
        "subset": (case("subset", sub[:40], sub, identity_draws(40), identity_draws(60)[:40],
                        "a mean of exactly 0 stops the default loop after one iteration"), 1),
    }


def fraction_cases():
    """(case, status): n_dst = n_src * min_fraction exactly (80 / 16 = 5 and 7 / 2 = 3.5 -> 4: products
    exact in f64) is status 0, one point fewer status 2"""
    A = cloud(61, 80)
    Bm = moved(A, [0.1, 0.2, 0.9], 3.0, [1.0, 0.5, -2.0])[0]
    out = []
    for ns, frac, nd, status in [(80, 0.0625, 5, 0), (80, 0.0625, 4, 2), (7, 0.5, 4, 0), (7, 0.5, 3, 2), (80, 0.0, 1, 0)]:
        us = np.full(80, 0.5)
        us[:nd] = (np.arange(nd) + 0.5) / ns  # source point i, whose image destination point i is
        out.append((case(f"fraction_{ns}_{frac}_{nd}", A[:ns], Bm[:nd], us, identity_draws(nd, 80),
                         f"n_dst {nd} against n_src {ns} * {frac}", N=80, max_iterations=3, min_fraction=frac), status))
    return out


def angle_cases(rel=1e-6):
    """[(case, status)] in mode no_depth around the angle theta the oracle's own T turns by: a limit of
    theta (1 + rel) keeps the pose, theta (1 - rel) drops it (the check is strict; rel is far above the
    1e-12 by which two solvers' angles differ and far below anything a caller would set)."""
    A = cloud(71, 80)
    Bm = moved(A, [0.1, 0.1, 1.0], 8.0, [0.5, -0.5, 0.0])[0]
    u = identity_draws(80)
    base = case("angle", A, Bm, u, u, "", mode=IR.NO_DEPTH, angle_limit=np.pi)
    theta = IR.rotation_angle(run(base)["T"])
    return theta, [(dict(base, name="angle_above", hits="a turn just below the limit", kw=dict(base["kw"], angle_limit=theta * (1 + rel))), 0),
                   (dict(base, name="angle_below", hits="a turn just above the limit", kw=dict(base["kw"], angle_limit=theta * (1 - rel))), 3)]


def neighbours():
    """(src, dst) of a status-1 pose (no source points) and a status-2 pose (3 destination points
    against 80 source points), for batches"""
    A = cloud(81, 80)
    return (np.zeros((0, 3)), A[:10]), (A, A[:3] + 1.0)


# ---- zp_depth_points ---------------------------------------------------------------------------------------

def depth_cases():
    """name -> dict(depth f32 [B, H, W], K [B, 4], cap, filt, factor, exact: True when a point sits
    exactly on the filter's radius (integers: both sides agree whatever the margin), hits)"""
    rng = np.random.default_rng(91)
    out = {}

    def K_of(B, H, W):
        return np.stack([[150.0 + b, 148.0, W / 2.0 - 0.25 * b, H / 2.0 + 0.5] for b in range(B)])

    def add(name, d, hits, K=None, cap=None, filt=None, factor=2.0, exact=False):
        d = np.asarray(d, np.float32)
        out[name] = dict(depth=d, K=K_of(*d.shape) if K is None else np.asarray(K, np.float64), cap=cap, filt=filt,
                         factor=factor, exact=exact, hits=hits)

    tiny = np.float32(1e-45)  # the smallest f32 denormal
    sp = np.zeros((1, 5, 8), np.float32)
    sp[0, 0, :] = [np.nan, np.inf, -np.inf, -0.0, -250.0, tiny, -tiny, 500.0]
    sp[0, 1, :4] = [np.float32(1.1e-38), np.float32(3.4e38), 0.0, 1.0]  # a denormal, near the largest f32
    add("special_values", sp, "NaN, +-inf, -0.0, negative, denormal depths")
    for H, W in [(37, 1), (1, 37), (33, 31), (1, 1)]:
        d = np.where(rng.random((2, H, W)) < 0.6, 400 + 300 * rng.random((2, H, W)), 0.0)
        d[1, H - 1, W - 1] = 321.5
        add(f"shape_{H}x{W}", d, f"{H} x {W}: W = 1 / H W no multiple of 1024")
    # tiles of 1024 pixels (16 rows of 64): full | empty | partial, and a count that lands on 1024 / 2048
    t = np.zeros((3, 48, 64), np.float32)
    t[0, :16] = 500 + rng.random((16, 64))
    t[0, 32:] = np.where(rng.random((16, 64)) < 0.3, 700.0, 0.0)
    t[1, 8:24] = 600 + rng.random((16, 64))   # 1024 kept across two tiles: the count lands on a tile's size
    t[2] = 450 + rng.random((48, 64))         # every tile full
    add("tiles", t, "a tile with all kept, one with none, a kept count of exactly 1024")
    add("tiles_cap", t, "cap below the count, stats of all kept points", cap=1000)
    add("all_empty", np.zeros((2, 33, 31), np.float32), "no pixel kept, stats zero")
    # K = (2, 2, 0, 0) and depth 2: pixel (u, v) is the point (u, v, 2).  Centre (0, 0, 2), radius 2.5,
    # factor 2: lim^2 = 25 = 3^2 + 4^2 = 5^2 + 0, so (3, 4), (4, 3), (5, 0), (0, 5) sit on the radius
    f = np.zeros((1, 7, 7), np.float32)
    f[0] = 2.0
    add("filter_on_the_radius", f, "d^2 = lim^2 exactly is dropped (strict <)", K=[[2.0, 2.0, 0.0, 0.0]],
        filt=np.array([[0.0, 0.0, 2.0, 2.5]]), factor=2.0, exact=True)
    add("filter_factor_0", f, "factor 0: nothing is closer than 0", K=[[2.0, 2.0, 0.0, 0.0]],
        filt=np.array([[0.0, 0.0, 2.0, 2.5]]), factor=0.0, exact=True)
    return out
