"""numpy restatement of the BOP pose errors' semantics (include/zp.h: zp_pose_error_sym, zp_vsd),
in the project's own words, as render_ref.py is for the rasteriser: the symmetry set, MSSD, MSPD and
VSD's pixel stage with its integer counts.  Everything is f64 unless the contract says f32."""
import numpy as np


def rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def axis_angle(angle, axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    x, y, z = a
    c, s, v = np.cos(angle), np.sin(angle), 1.0 - np.cos(angle)
    return np.array([[c + x * x * v, x * y * v - z * s, x * z * v + y * s],
                     [y * x * v + z * s, c + y * y * v, y * z * v - x * s],
                     [z * x * v - y * s, z * y * v + x * s, c + z * z * v]])


def symmetry_set(model_info, max_sym_disc_step=0.01):
    """Identity + discrete symmetries, each followed by every non-zero step of each continuous one
    (ceil(pi / step) steps per turn; a rotation about the axis through `offset`); discrete outermost."""
    disc = [(np.eye(3), np.zeros(3))]
    for m in model_info.get("symmetries_discrete", []):
        m = np.asarray(m, np.float64).reshape(4, 4)
        disc.append((m[:3, :3], m[:3, 3]))
    cont = []
    for c in model_info.get("symmetries_continuous", []):
        count = int(np.ceil(np.pi / max_sym_disc_step))
        off = np.asarray(c["offset"], np.float64)
        for i in range(1, count):
            R = axis_angle(i * (2.0 * np.pi / count), c["axis"])
            cont.append((R, off - R @ off))
    out = [(Rc @ Rd, Rc @ td + tc) for Rd, td in disc for Rc, tc in cont] if cont else disc
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _errors_sym(pts, R_est, t_est, R_gt, t_gt, sym_R, sym_t, project):
    p = np.asarray(pts, np.float32).astype(np.float64)
    a = project(p @ R_est.T + t_est)
    es = []
    for S, s in zip(sym_R, sym_t):
        R_s, t_s = R_gt @ S, R_gt @ s + t_gt
        es.append(np.linalg.norm(a - project(p @ R_s.T + t_s), axis=1).max())
    return np.array(es)


def mssd_per_sym(pts, R_est, t_est, R_gt, t_gt, sym_R, sym_t):
    return _errors_sym(pts, R_est, t_est, R_gt, t_gt, sym_R, sym_t, lambda c: c)


def mspd_per_sym(pts, R_est, t_est, R_gt, t_gt, K4, sym_R, sym_t):
    fx, fy, cx, cy = K4
    return _errors_sym(pts, R_est, t_est, R_gt, t_gt, sym_R, sym_t,
                       lambda c: np.stack([fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy], 1))


def mssd(pts, R_est, t_est, R_gt, t_gt, sym_R, sym_t):
    return mssd_per_sym(pts, R_est, t_est, R_gt, t_gt, sym_R, sym_t).min()


def mspd(pts, R_est, t_est, R_gt, t_gt, K4, sym_R, sym_t):
    return mspd_per_sym(pts, R_est, t_est, R_gt, t_gt, K4, sym_R, sym_t).min()


def dist_image(depth, K4):
    """dist = sqrt(((pX z)^2 + (pY z)^2) + z^2), pX = (x - cx) / fx, pY = (y - cy) / fy; every step
    one f64 operation."""
    fx, fy, cx, cy = (np.float64(v) for v in K4)
    H, W = depth.shape
    pX = ((np.arange(W, dtype=np.float64) - cx) / fx)[None, :]
    pY = ((np.arange(H, dtype=np.float64) - cy) / fy)[:, None]
    z = np.asarray(depth, np.float32).astype(np.float64)
    a, b = pX * z, pY * z
    return np.sqrt((a * a + b * b) + z * z)


def visibility(dist_test, dist_model, delta):
    """'bop19': visible where the model is at most delta behind the scene (compared in f32) or the
    scene has no depth, and the model has a surface."""
    diff = dist_model.astype(np.float32) - dist_test.astype(np.float32)
    return ((diff <= np.float32(delta)) | (dist_test == 0)) & (dist_model > 0)


def vsd_masks(dist_est, dist_gt, dist_test, delta):
    vg = visibility(dist_test, dist_gt, delta)
    ve = visibility(dist_test, dist_est, delta) | (vg & (dist_est > 0))
    return vg, ve


def vsd_pixels(depth_est, depth_gt, depth_test, K4, delta, taus, diameter=None, return_parts=False):
    """One pose.  Returns (counts i64 [2 + ntau] = (union, inter, cost_k), errors f64 [ntau])."""
    de, dg, dt = (dist_image(d, K4) for d in (depth_est, depth_gt, depth_test))
    vg, ve = vsd_masks(de, dg, dt, delta)
    inter, union = vg & ve, vg | ve
    dists = np.abs(dg[inter] - de[inter])
    if diameter is not None:
        dists = dists / np.float64(diameter)
    taus = np.asarray(taus, np.float64)
    nu, ni = int(union.sum()), int(inter.sum())
    cost = [int((dists >= t).sum()) for t in taus]
    err = np.array([1.0 if nu == 0 else float(c + (nu - ni)) / float(nu) for c in cost])
    counts = np.array([nu, ni] + cost, np.int64)
    if return_parts:
        return counts, err, dict(dists=dists, dist_est=de, dist_gt=dg, dist_test=dt, visib_gt=vg, visib_est=ve)
    return counts, err


def vsd_batch(depth_est, depth_gt, depth_test, K4, delta, taus, diameter=None, test_index=None):
    B = len(depth_est)
    res = [vsd_pixels(depth_est[b], depth_gt[b], depth_test[b if test_index is None else test_index[b]], K4[b],
                      delta, taus, None if diameter is None else diameter[b]) for b in range(B)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def margins_ok(parts, delta, taus, rel=1e-6):
    """The margins the exact comparison rests on: no f32 visibility difference within 1e-3 of delta
    and no inter-pixel distance within rel * tau of a tau (a 1-ulp difference in a square root
    cannot flip a count)."""
    dt32 = parts["dist_test"].astype(np.float32)
    for m in ("dist_gt", "dist_est"):
        d = parts[m]
        diff = (d.astype(np.float32) - dt32)[(d > 0) & (parts["dist_test"] != 0)]
        if diff.size and np.abs(diff - np.float32(delta)).min() < 1e-3:
            return False
    for t in np.asarray(taus, np.float64):
        if parts["dists"].size and np.abs(parts["dists"] - t).min() <= rel * t:
            return False
    return True


def vsd_scene(rng, B, H, W, test_index=None):
    """Depth images built with margins: a smooth scene surface in 400 .. 1200 per test image; gt = the
    scene on a random 60 % of the pixels, est = the scene + one of {-3, 0, 12, 27, 60} (+-0.5) on another
    60 %, test = the scene + one of {-40, -5, 5, 40} (+-1), 0 on 15 %.  The focal length is ~6 W, so a
    distance is at most 1.02 x its depth and every visibility difference stays 0.5 away from delta = 15.
    Returns f32 est, gt [B, H, W], test [n_test, H, W], K f64 [B, 4], diameter f64 [B]."""
    ti = np.arange(B) if test_index is None else np.asarray(test_index)
    n_test = int(ti.max()) + 1
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    scene = np.stack([rng.uniform(550, 1050) + 60 * np.sin(xx / 7 + rng.uniform(0, 6)) + 40 * np.cos(yy / 5)
                      for _ in range(n_test)])
    test = scene + rng.choice([-40.0, -5.0, 5.0, 40.0], scene.shape) + rng.uniform(-1, 1, scene.shape)
    test[rng.random(scene.shape) < 0.15] = 0
    shape = (B, H, W)
    gt = np.where(rng.random(shape) < 0.6, scene[ti], 0.0)
    e_off = rng.choice([-3.0, 0.0, 12.0, 27.0, 60.0], shape) + rng.uniform(-0.5, 0.5, shape)
    est = np.where(rng.random(shape) < 0.6, scene[ti] + e_off, 0.0)
    K = np.stack([rng.uniform(5.5, 6.5, B) * W, rng.uniform(5.5, 6.5, B) * W, W / 2 + rng.uniform(-3, 3, B),
                  H / 2 + rng.uniform(-3, 3, B)], 1)
    return (est.astype(np.float32), gt.astype(np.float32), test.astype(np.float32), K, rng.uniform(90, 110, B))


def icosphere(level):
    """Unit icosphere, 10 * 4^level + 2 vertices (level 3: 642), outward-facing triangles."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int32)
