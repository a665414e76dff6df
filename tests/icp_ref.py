"""numpy restatement of zp_depth_points and zp_icp (include/zp.h): the executable definition of their
semantics, function by function beside the reference's zebrapose/icp/icp_utils.py.  Back-projection,
squared distances and neighbour indices are exact (single IEEE f64 operations in the stated order);
the sums (centroids, H, mean distance) are in numpy's order and the 3 x 3 fit uses numpy.linalg.svd, so
transforms agree with the device up to the order of summation and the solver's rounding.  Reads nothing
outside the repository.
"""
from __future__ import annotations

import numpy as np

MIN_FRACTION = 1.0 / 20.0          # icp_utils.py:149
ANGLE_LIMIT = 20 * np.pi / 180.0   # icp_utils.py:161
FULL, DEPTH_ONLY, NO_DEPTH = 0, 1, 2


def depth_points(depth, K, cap=None, filt=None, factor=2.0):
    """rgbd_to_point_cloud (icp_utils.py:7-13) with the finite-positive rule, then the distance filter
    of :147-148 on squared distances.  depth [H, W] (read as f32), K = (fx, fy, cx, cy), filt = (centre
    x, y, z, radius) or None.  Returns dict(count: the true count, pts f64 [min(count, cap), 3] in
    row-major pixel order, stats f64 [4]: centroid of all kept points and the largest distance from it
    (:139-141; zeros without points), edge: the smallest |d2 / lim^2 - 1| over the candidates of the
    filter (inf without one), the margin by which no point sits on the filter's radius)."""
    d = np.asarray(depth, dtype=np.float32)
    fx, fy, cx, cy = (float(v) for v in K)
    with np.errstate(invalid="ignore"):
        vs, us = np.nonzero(np.isfinite(d) & (d > 0))
    zs = d[vs, us].astype(np.float64)
    xs = ((us.astype(np.float64) - cx) * zs) / fx
    ys = ((vs.astype(np.float64) - cy) * zs) / fy
    pts = np.stack([xs, ys, zs], 1)
    edge = np.inf
    if filt is not None:
        f = np.asarray(filt, dtype=np.float64)
        dx, dy, dz = pts[:, 0] - f[0], pts[:, 1] - f[1], pts[:, 2] - f[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        lim = factor * f[3]
        lim2 = lim * lim
        if len(d2) and lim2 > 0:
            edge = float(np.abs(d2 / lim2 - 1.0).min())
        pts = pts[d2 < lim2]
    stats = np.zeros(4)
    if len(pts):
        c = pts.sum(0) / len(pts)
        e = pts - c
        stats[:3] = c
        stats[3] = np.sqrt(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).max())
    return dict(count=len(pts), pts=pts if cap is None else pts[:cap], stats=stats, edge=edge)


def nearest(src, dst, chunk=512):
    """nearest_neighbor (icp_utils.py:16-32) by brute force: per source point the destination point
    with the smallest (dx dx + dy dy) + dz dz, ties to the lowest index.  Returns (Euclidean distances,
    indices, margin): margin is the smallest relative gap (second - best) / second over all source
    points, second being the smallest squared distance above the best one (exact duplicates of the best
    tie by rule and are left out)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    idx = np.empty(len(src), np.int64)
    best = np.empty(len(src))
    margin = np.inf
    for i0 in range(0, len(src), chunk):
        s = src[i0:i0 + chunk]
        dx = s[:, None, 0] - dst[None, :, 0]
        dy = s[:, None, 1] - dst[None, :, 1]
        dz = s[:, None, 2] - dst[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        j = d2.argmin(1)  # the first of equal minima
        b = d2[np.arange(len(s)), j]
        second = np.where(d2 > b[:, None], d2, np.inf).min(1)
        ok = np.isfinite(second)
        if ok.any():
            margin = min(margin, float(((second[ok] - b[ok]) / second[ok]).min()))
        idx[i0:i0 + chunk], best[i0:i0 + chunk] = j, b
    return np.sqrt(best), idx, margin


def best_fit_transform(A, B, mode=FULL):
    """best_fit_transform (icp_utils.py:35-80).  Returns (T [4, 4], R, t, H, singular values); H and the
    singular values are None in mode DEPTH_ONLY."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    cA, cB = A.mean(0), B.mean(0)
    H = S = None
    if mode == DEPTH_ONLY:
        R = np.eye(3)
        t = cB - cA
    else:
        H = (A - cA).T @ (B - cB)
        U, S, Vt = np.linalg.svd(H)
        R = Vt.T @ U.T
        if np.linalg.det(R) < 0:
            Vt[2, :] *= -1
            R = Vt.T @ U.T
        t = cB - R @ cA
        if mode == NO_DEPTH:
            t = np.array([t[0], t[1], 0.0])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T, R, t, H, S


def icp(A, B, max_iterations=200, tolerance=5e-7, mode=FULL):
    """icp (icp_utils.py:83-126) without an initial pose.  Returns dict(T, iterations: how many ran (the
    reference's i + 1), mean_error: the mean distance of the last one, nn: its neighbour indices,
    margins: nearest()'s margin per iteration, H / S: of the first iteration's fit)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    src = A.copy()
    prev, margins, first = 0.0, [], None
    for it in range(max_iterations):
        dist, idx, m = nearest(src, B)
        margins.append(m)
        T, R, t, H, S = best_fit_transform(src, B[idx], mode)
        if first is None:
            first = (H, S)
        src = src @ R.T + t
        mean = dist.mean()
        if abs(prev - mean) < tolerance:
            break
        prev = mean
    T = best_fit_transform(A, src, mode)[0]
    return dict(T=T, iterations=it + 1, mean_error=float(mean), nn=idx, margins=margins, H=first[0], S=first[1])


def rotation_angle(T):
    """|angle| of transform.rotation_from_matrix (transform.py:346-383) from the skew part and the trace."""
    a = np.array([T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1]])
    return float(np.arctan2(0.5 * np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]),
                            0.5 * (((T[0, 0] + T[1, 1]) + T[2, 2]) - 1.0)))


def draw_indices(draws, count):
    """floor(draw * count): sampling with replacement from uniform draws in [0, 1).  A draw outside
    that range still gives an index, as on the device: count - 1 from draw * count >= count on (1.0
    and above, +inf), 0 for a negative product, -0.0 and NaN."""
    v = np.asarray(draws, np.float64) * float(count)
    with np.errstate(invalid="ignore"):
        inside = (v >= 0.0) & (v < float(count))
        idx = np.where(inside, v, 0.0).astype(np.int64)
        return np.where(v >= float(count), count - 1, idx)


def icp_pose(src_pts, dst_pts, draws_src, draws_dst, R, t, N=None, max_iterations=200, tolerance=5e-7, mode=FULL,
             min_fraction=MIN_FRACTION, angle_limit=ANGLE_LIMIT):
    """zp_icp for one pose: ICPRefiner.refine from the point counts on (icp_utils.py:149-174).  Returns
    dict(R, t, status, iterations, mean_error, T, nn, margins, n, H, S)."""
    src_pts, dst_pts = np.asarray(src_pts, np.float64).reshape(-1, 3), np.asarray(dst_pts, np.float64).reshape(-1, 3)
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    N = len(draws_src) if N is None else N
    ns, nd = len(src_pts), len(dst_pts)
    out = dict(R=R, t=t, status=0, iterations=0, mean_error=0.0, T=np.eye(4), nn=np.zeros(0, np.int64), margins=[],
               n=0, H=None, S=None)
    if ns == 0:
        out["status"] = 1
        return out
    n = min(ns, nd, N)
    if float(nd) < float(ns) * min_fraction or n == 0:
        out["status"] = 2
        return out
    A = src_pts[draw_indices(draws_src[:n], ns)]
    B = dst_pts[draw_indices(draws_dst[:n], nd)]
    r = icp(A, B, max_iterations, tolerance, mode)
    out.update(n=n, A=A, B=B, **r)
    if mode == NO_DEPTH and rotation_angle(r["T"]) > angle_limit:
        out["status"] = 3
        return out
    T = r["T"]
    out["R"], out["t"] = T[:3, :3] @ R, T[:3, :3] @ t + T[:3, 3]
    return out


def refine(verts, faces, depth_meas, R, t, K, draws_src, draws_dst, N=None, max_iterations=200, tolerance=5e-7,
           mode=FULL, factor=2.0):
    """ICPRefiner.refine (icp_utils.py:134-176) for one pose: the model's depth at (R, t) from the numpy
    rasteriser with the pixel centres at integers, both clouds, the filter, zp_icp.  depth_meas [H, W].
    Returns icp_pose's dict plus edge (depth_points' filter margin)."""
    from tests import render_ref as RR
    H, W = np.asarray(depth_meas).shape
    K = np.asarray(K, np.float64).reshape(4)
    Kr = K + np.array([0, 0, 0.5, 0.5])
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    syn = RR.render(verts, faces, None, R.reshape(1, 9), t.reshape(1, 3), Kr[None], H, W)["depth"][0]
    s = depth_points(syn, K)
    d = depth_points(depth_meas, K, filt=s["stats"], factor=factor)
    out = icp_pose(s["pts"], d["pts"], draws_src, draws_dst, R, t, N, max_iterations, tolerance, mode)
    out["edge"] = d["edge"]
    return out
