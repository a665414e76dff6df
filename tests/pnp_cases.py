"""Deterministic PnP inputs shared by tests/test_pnp_cases_host.py (the preconditions, on the
oracle alone) and tests/test_gpu_pnp_edges.py (the device).  Plain numpy, no GPU.

Every builder returns a scene ``(pw f32 [n,3], uv int32 [n,2], R, t)``: model points, the integer
pixels they are seen at, and the pose ``x_cam = R x_model + t`` they were built from.

*Exact-pixel* scenes start from integer pixels: a pixel's ray is cut at a chosen depth (or by a
plane of the model) and the cut is stored in the model frame as f32, ``R^T (pc - t)``, so the
projection of ``pw`` hits its integer pixel up to the f32 rounding of ``pw`` -- the only noise.
"""
import numpy as np

from oracle import pnp_ref

K0 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])

# (a) sizes around the refine's reduction edges: below / at / above one wave (64), one block pass
# (256) and two (512), and one far into the stride-256 loop; 6 and 7 are the smallest legal sets
EXACT_SIZES = (6, 7, 63, 64, 65, 255, 256, 257, 511, 513, 4099)
EXACT_HW = 4099
EXACT_THRESHOLD = 1e4


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(pw, R, t, K):
    Xc = np.asarray(pw, np.float64) @ R.T + t
    return np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1), Xc[:, 2]


def vary_K(rng, K=K0):
    """fx, fy, cx, cy each scaled by a factor in [0.8, 1.2]."""
    s = rng.uniform(0.8, 1.2, 4)
    return np.array([[K[0, 0] * s[0], 0.0, K[0, 2] * s[2]], [0.0, K[1, 1] * s[1], K[1, 2] * s[3]], [0.0, 0.0, 1.0]])


def _pose(rng, z=(500.0, 1100.0), centre_px=None, K=K0):
    R = rodrigues(rng.normal(0, 0.6, 3))
    tz = rng.uniform(*z)
    if centre_px is None:
        t = np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), tz])
    else:  # the model origin projects onto centre_px
        t = np.array([(centre_px[0] - K[0, 2]) / K[0, 0] * tz, (centre_px[1] - K[1, 2]) / K[1, 1] * tz, tz])
    return R, t


def _from_depth(uv, z, R, t, K):
    """cut the rays of integer pixels uv at integer depths z -> model points (f32)"""
    pc = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, z], 1)
    return ((pc - t) @ R).astype(np.float32)  # R^T (pc - t)


def _from_plane(uv, h, R, t, K):
    """cut the rays of integer pixels uv by the model planes z = h[i] -> model points (f32) whose
    z is h exactly"""
    d = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(uv))], 1) @ R
    o = -t @ R
    s = (h - o[2]) / d[:, 2]
    p = o + s[:, None] * d
    p[:, 2] = h
    return p.astype(np.float32)


def exact_box(rng, n, K=K0, half=(60.0, 60.0, 60.0), z=(500.0, 1100.0), centre_px=None):
    """Exact-pixel scene of a box: points drawn in +-half, seen at their rounded pixel and rounded
    depth (so they leave the box by at most a pixel's footprint and half a millimetre)."""
    R, t = _pose(rng, z, centre_px, K)
    p = rng.uniform(-1, 1, (n, 3)) * np.asarray(half)
    uv, zc = project(p, R, t, K)
    uv = np.round(uv)
    return _from_depth(uv, np.round(zc), R, t, K), uv.astype(np.int32), R, t


def exact_slab(rng, n, K=K0, half=60.0, thickness=1.0):
    """Exact-pixel scene of a slab 2*half x 2*half x thickness; thickness 0: exactly planar, every
    model z is 0.0."""
    R, t = _pose(rng, K=K)
    h = rng.uniform(-0.5, 0.5, n) * thickness
    p = np.concatenate([rng.uniform(-half, half, (n, 2)), h[:, None]], 1)
    uv = np.round(project(p, R, t, K)[0])
    return _from_plane(uv, h, R, t, K), uv.astype(np.int32), R, t


def add_outliers(rng, scene, frac):
    pw, uv, R, t = scene
    uv = uv.copy()
    out = rng.random(len(uv)) < frac
    uv[out] += rng.integers(-120, 121, (int(out.sum()), 2)).astype(np.int32)
    return pw, uv, R, t


def cube(rng, n, K=K0):
    return exact_box(rng, n, K)


def slab(rng, n, K=K0):
    return exact_slab(rng, n, K, thickness=1.0)


def planar(rng, n, K=K0):
    return exact_slab(rng, n, K, thickness=0.0)


def coarse_lut(rng, n=4000, K=K0, distinct=64):
    """What a coarse LUT leaves of an object: `distinct` 3D points shared by n pixels.  The sharing
    pixels are collapsed onto the point's own exact pixel (n / distinct copies of each pair), so
    the data still fixes the pose and a 5-point subset often holds the same point twice.  With the
    pixels spread over the point's footprint instead (+-3 px at n = 2000), the oracle's pose lies
    0.6 to 2.6 degrees from the truth and the oracle and the serial host build of the device code,
    both correct, end up to 5 degrees apart (12 seeds tried): no test could hold either to 0.1."""
    pw, uv, R, t = exact_box(rng, distinct, K)
    which = rng.permutation(np.arange(n) % distinct)
    return pw[which], uv[which], R, t


def coarse_lut_spread(rng, n=4000, K=K0, distinct=64):
    """The issue's literal coarse LUT: `distinct` 3D points, each shared by the n / distinct pixels
    of the square patch around its projection (+-4 px at n = 4000), so one 3D point comes with
    many inconsistent pixels.  Such data fixes the pose only to degrees (see coarse_lut): the
    device is run on it for its invariants only."""
    R, t = _pose(rng, K=K)
    pts = rng.uniform(-60, 60, (distinct, 3)).astype(np.float32)
    which = np.arange(n) % distinct
    side = int(np.ceil(np.sqrt(n / distinct)))
    off = rng.integers(-(side // 2), side - side // 2, (n, 2))
    uv = np.round(project(pts, R, t, K)[0])[which] + off
    return pts[which], uv.astype(np.int32), R, t


def small_far(rng, n, K=K0):
    return exact_box(rng, n, K, half=(5.0, 5.0, 5.0), z=(1500.0, 1500.0))


def off_centre(rng, n, K=K0):
    """a cube whose centre projects onto pixel (5, 5): about half its pixels are negative"""
    return exact_box(rng, n, K, z=(600.0, 900.0), centre_px=(5.0, 5.0))


def identical(rng, n=50, K=K0):
    """one 3D point seen at the pixels of the 3 x 3 patch around its projection"""
    R, t = _pose(rng, K=K)
    p = rng.uniform(-60, 60, (1, 3)).astype(np.float32)
    uv = np.round(project(p, R, t, K)[0]) + rng.integers(-1, 2, (n, 2))
    return np.repeat(p, n, 0), uv.astype(np.int32), R, t


def collinear(rng, n=50, K=K0):
    """exactly collinear model points (integer multiples of a direction f32 holds exactly), seen
    at their rounded pixels"""
    R, t = _pose(rng, K=K)
    p = (rng.integers(-80, 81, n)[:, None] * np.array([0.5, 0.25, -0.75])).astype(np.float32)
    uv = np.round(project(p, R, t, K)[0])
    return p, uv.astype(np.int32), R, t


def exact_cases(per_crop_K=False):
    """(a): one exact-pixel cube scene per size of EXACT_SIZES -> [(scene, K)]"""
    rng = np.random.default_rng(2024)
    out = []
    for n in EXACT_SIZES:
        K = vary_K(rng) if per_crop_K else K0
        out.append((cube(rng, n, K), K))
    return out


def degenerate_cases():
    """(c): name -> scene, default intrinsics, 30 % outliers where there is a pose to find"""
    def rng(k):
        return np.random.default_rng(7700 + k)
    return {
        "slab": add_outliers(rng(0), slab(rng(1), 2000), 0.3),
        "planar": add_outliers(rng(2), planar(rng(3), 2000), 0.3),
        "coarse_lut": add_outliers(rng(4), coarse_lut(rng(5), 2000), 0.3),
        "small_far": add_outliers(rng(6), small_far(rng(7), 2000), 0.3),
        "off_centre": add_outliers(rng(8), off_centre(rng(9), 2000), 0.3),
        "identical": identical(rng(10), 50),
        "collinear": collinear(rng(11), 50),
    }


def iteration_scene():
    """(d): one realistic 800-point, 50 %-outlier scene (test_gpu_pnp._scene) whose consensus the
    oracle finds inside the first chunk of 32 iterations (tests/test_pnp_cases_host.py checks it:
    a scene that has found only chance models by then pins nothing at 32 / 33)"""
    from tests.test_gpu_pnp import _scene
    return _scene(np.random.default_rng(25), 800, 0.5)


def oracle_solves(pw, uv, K=K0):
    """-> (ref, solved).  The oracle solves a case if its RANSAC succeeds with a finite pose AND
    returns that pose again (to the tolerances the device is held to: inliers within max(2, 2 %),
    0.1 degree, 1e-2 relative) when pw is perturbed by 1e-13 relative.  An answer the oracle does
    not reproduce under rounding-sized noise (collinear points: the rotation about the line is
    free) cannot pin another implementation."""
    uvf = np.asarray(uv, np.float32)
    ref = pnp_ref.solve_pnp_ransac(pw, uvf, K)
    if not (ref["success"] and np.all(np.isfinite(ref["R"])) and np.all(np.isfinite(ref["t"]))):
        return ref, False
    g = np.random.default_rng(1).normal(0, 1, np.shape(pw))
    pw2 = (np.asarray(pw, np.float64) * (1 + 1e-13 * g))
    ref2 = pnp_ref.solve_pnp_ransac(pw2, uvf, K, pw_dtype=np.float64)  # unrounded: the perturbation survives
    if not (ref2["success"] and np.all(np.isfinite(ref2["R"])) and np.all(np.isfinite(ref2["t"]))):
        return ref, False
    same = (abs(ref2["inliers"] - ref["inliers"]) <= max(2, 0.02 * len(pw))
            and rot_angle_deg(ref2["R"], ref["R"]) < 0.1
            and np.linalg.norm(ref2["t"] - ref["t"]) < 1e-2 * np.linalg.norm(ref["t"]))
    return ref, bool(same)


def well_posed(pw, uv, K, seed=0):
    """Conditioning guard, on the oracle alone: EPnP of (pw, uv) moves by < 1e-10 (R: max abs,
    t: relative) when pw is perturbed by 1e-13 relative, i.e. it amplifies rounding by at most
    1e3, which keeps the device's ~1e-15..1e-14 under a 1e-9 tolerance."""
    uv = np.asarray(uv, np.float32)
    R0, t0 = pnp_ref.epnp(pw, uv, K)
    g = np.random.default_rng(seed).normal(0, 1, np.shape(pw))
    R1, t1 = pnp_ref.epnp(np.asarray(pw, np.float64) * (1 + 1e-13 * g), uv, K)
    if not (np.all(np.isfinite(R0)) and np.all(np.isfinite(t0)) and np.all(np.isfinite(R1)) and np.all(np.isfinite(t1))):
        return False
    return bool(np.abs(R1 - R0).max() < 1e-10 and np.linalg.norm(t1 - t0) < 1e-10 * np.linalg.norm(t0))


def oracle_inliers(ref, pw, uv, K, reprojection_error=2.0):
    """the inlier mask of the oracle's winning hypothesis (the set its final EPnP ran over)"""
    thr2 = np.float32(reprojection_error * reprojection_error)
    return pnp_ref.ransac_err(ref["hyp"][0], ref["hyp"][1], pw, np.asarray(uv, np.float32), K) <= thr2


def batch(scenes, HW, garbage_tail=False):
    """scenes -> (counts int32 [B], xy int32 [B,HW,2], xyz f32 [B,HW,3]); the rows past counts[b]
    are zero, or NaN / INT32_MIN / INT32_MAX with garbage_tail"""
    B = len(scenes)
    xy = np.zeros((B, HW, 2), np.int32)
    xyz = np.zeros((B, HW, 3), np.float32)
    if garbage_tail:
        xyz[:] = np.nan
        xy[..., 0] = np.iinfo(np.int32).min
        xy[..., 1] = np.iinfo(np.int32).max
    counts = np.zeros(B, np.int32)
    for b, sc in enumerate(scenes):
        pw, uv = sc[0], sc[1]
        counts[b] = len(pw)
        xy[b, :len(pw)] = uv
        xyz[b, :len(pw)] = pw
    return counts, xy, xyz


def rot_angle_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))
