"""numpy / scipy restatement of zp_mask_contour and zp_edge_refine_step (include/zp.h): the executable
definition of their semantics.  Integers (border sets, matches, costs) are exact; the f64 sums are in
numpy's order, so H, b and the pose agree with the device up to the order of summation.  Reads nothing
outside the repository.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage

from tests import render_ref as RR

MIN_BORDER = 20
SAT = 1 << 20
_CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def outer_border(img):
    """bool [H, W]: the set pixels with a 4-neighbour in the outside, the 4-connected component of
    unset pixels that contains the ring of unset pixels padded around the image."""
    s = np.asarray(img) != 0
    free = np.pad(~s, 1, constant_values=True)
    lab, _ = ndimage.label(free, structure=_CROSS)
    out = lab == lab[0, 0]
    near = out[:-2, 1:-1] | out[2:, 1:-1] | out[1:-1, :-2] | out[1:-1, 2:]
    return s & near


def border_list(img):
    """int64 [n, 2] = (x, y) of the outer-border pixels in row-major order."""
    ys, xs = np.nonzero(outer_border(img))
    return np.stack([xs, ys], 1).astype(np.int64)


def fill_passes(img):
    """How many passes of the device's fill change something: a pass closes every row of the box
    (the set pixels' bounding box grown by one, clipped) under left / right steps, then every column
    under up / down steps, starting from the unset pixels on the box's perimeter.  The device gives
    up (status 2) when this reaches 4 (H + W)."""
    s = np.asarray(img) != 0
    if not s.any():
        return 0
    H, W = s.shape
    ys, xs = np.nonzero(s)
    y0, y1, x0, x1 = max(ys.min() - 1, 0), min(ys.max() + 1, H - 1), max(xs.min() - 1, 0), min(xs.max() + 1, W - 1)
    f = ~s[y0:y1 + 1, x0:x1 + 1]
    o = np.zeros_like(f)
    o[0], o[-1], o[:, 0], o[:, -1] = f[0], f[-1], f[:, 0], f[:, -1]

    def close(o, f):  # 1-D closure along axis 1
        lab = np.cumsum(np.diff(np.pad(f, ((0, 0), (1, 0))).astype(np.int8), axis=1) == 1, axis=1) * f
        hit = np.zeros((f.shape[0], lab.max() + 1), bool)
        np.logical_or.at(hit, (np.nonzero(o)[0], lab[o]), True)
        hit[:, 0] = False
        return np.take_along_axis(hit, lab, axis=1) & f

    passes = 0
    while True:
        n = close(o, f)
        n = close(n.T, f.T).T
        if (n == o).all():
            return passes
        o, passes = n, passes + 1


def capped(img):
    """Whether the device gives up on this image: the fill's last changing pass is pass 4 (H + W) or
    later, so none of its 4 (H + W) passes sees that nothing changes (zp_mask_contour: counts = -1;
    zp_edge_refine_step: status 2)."""
    H, W = np.asarray(img).shape
    return fill_passes(img) >= 4 * (H + W)


def mask_contour(entire, visible, bbox):
    """test.py:300-307 for one crop: entire [S, S], visible [S, S] or None, bbox (x, y, w, h) ->
    int32 [n, 2] image pixels (all of them: the device's counts is n, its list the first cap)."""
    S = entire.shape[0]
    pts = border_list(entire)
    x, y = pts[:, 0], pts[:, 1]
    keep = (x > 0) & (y > 0)
    if visible is not None:
        v = np.pad(np.asarray(visible) != 0, ((1, 0), (1, 0)))
        keep &= v[y, x] | v[y, x + 1] | v[y + 1, x] | v[y + 1, x + 1]  # visible[y-1 .. y][x-1 .. x]
    x, y = x[keep], y[keep]
    bx, by, w, h = (np.float64(v) for v in bbox)
    X = (w / np.float64(S)) * x.astype(np.float64) + bx
    Y = (h / np.float64(S)) * y.astype(np.float64) + by
    return np.stack([np.trunc(X), np.trunc(Y)], 1).astype(np.int32)


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def exp_so3(w):
    """Rodrigues; the series below |w| = 1e-8."""
    w = np.asarray(w, np.float64)
    a2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    a = np.sqrt(a2)
    if a < 1e-8:
        ca, cc = 1.0 - a2 / 6.0, 0.5 - a2 / 24.0
    else:
        ca, cc = np.sin(a) / a, 2.0 * np.sin(0.5 * a) ** 2 / a2
    Kx = hat(w)
    return np.eye(3) + ca * Kx + cc * (Kx @ Kx)


def jacobian(Xc, R, t, K):
    """The 2 x 6 Jacobian of e = obs - project(R exp([th_r]x) (Xb + th_t) + t) at th = 0, columns
    (rotation | translation), for the camera point Xc = R Xb + t."""
    fx, fy = K[0], K[1]
    R = np.asarray(R, np.float64).reshape(3, 3)
    d = Xc[2]
    Jc = np.array([[-fx / d, 0, fx * Xc[0] / (d * d)], [0, -fy / d, fy * Xc[1] / (d * d)]])
    Jt = Jc @ R
    Xb = R.T @ (Xc - np.asarray(t, np.float64))
    return np.hstack([-Jt @ hat(Xb), Jt])


def step(depth, pts, R, t, K, lambda_rot, lambda_trans):
    """One zp_edge_refine_step for one pose.  depth f32 [H, W]; pts int [n, 2] (the observed points
    the device uses: the first min(counts, cap)); K = (fx, fy, cx, cy), unshifted."""
    depth = np.asarray(depth)  # f32 on the device; f64 is taken as it is (the unit test scales it)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    K = np.asarray(K, np.float64).reshape(4)
    H_, W_ = depth.shape
    sil = depth > 0
    out = {"R": R.copy(), "t": t.copy(), "cost": 0, "Hb": np.zeros(27), "match": np.zeros(0, np.int64)}
    if capped(sil):
        out.update(status=2, border=np.zeros((0, 2), np.int64))
        return out
    border = border_list(sil)
    out["border"] = border
    pts = np.clip(np.asarray(pts, np.int64).reshape(-1, 2), -SAT, SAT)
    if len(border) < MIN_BORDER or len(pts) == 0:
        out["status"] = 1
        return out
    d2 = ((pts[:, None, :] - border[None, :, :]) ** 2).sum(2)
    m = np.argmin(d2, axis=1)  # the first minimum: the lowest row-major index
    e = (pts - border[m]).astype(np.float64)
    Hm, bv = np.zeros((6, 6)), np.zeros(6)
    fx, fy, cx, cy = K
    for i, j in enumerate(m):
        xc, yc = border[j]
        d = np.float64(depth[yc, xc])
        Xc = np.array([d * (xc - cx) / fx, d * (yc - cy) / fy, d])
        J = jacobian(Xc, R, t, K)
        Hm += J.T @ J
        bv -= J.T @ e[i]
    A = Hm + np.diag([lambda_rot] * 3 + [lambda_trans] * 3)
    th = np.linalg.solve(A, bv)
    Rn = R @ exp_so3(th[:3])
    out.update(status=0, match=m, cost=int((e.astype(np.int64) ** 2).sum()), A=A, theta=th, R=Rn,
               t=t + Rn @ th[3:], Hb=np.concatenate([Hm[np.triu_indices(6)], bv]))
    return out


def refine(verts, faces, R, t, K, H, W, pts, iterations=10, lambda_rot=5000.0, lambda_trans=0.5, on_pose=None):
    """EdgeRefiner.refine for one pose: each iteration renders depth with tests/render_ref.render at
    K' = (fx, fy, cx + 1/2, cy + 1/2) and steps.  Returns (R, t, status, costs); a status other than 0
    gives the input pose back.  on_pose(R, t) sees every pose that is rendered."""
    R0, t0 = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    K = np.asarray(K, np.float64).reshape(4)
    Kr = K + np.array([0, 0, 0.5, 0.5])
    Rc, tc, costs = R0, t0, []
    for _ in range(iterations):
        if on_pose is not None:
            on_pose(Rc, tc)
        depth = RR.render(verts, faces, None, Rc.reshape(1, 9), tc[None], Kr[None], H, W)["depth"][0]
        s = step(depth, pts, Rc, tc, K, lambda_rot, lambda_trans)
        costs.append(s["cost"])
        if s["status"] != 0:
            return R0, t0, s["status"], costs + [0] * (iterations - len(costs))
        Rc, tc = s["R"], s["t"]
    return Rc, tc, 0, costs


def snap_margin(verts, R, t, K):
    """How far (in 1/256-px units, at most 0.5) the nearest vertex projection is from a rounding
    boundary of the renderer's snap: a pose difference that moves a projection by less cannot change
    the render."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3)
    X = v @ R.T + np.asarray(t, np.float64).reshape(3)
    u = 256.0 * (K[0] * X[:, 0] / X[:, 2] + K[2])
    w = 256.0 * (K[1] * X[:, 1] / X[:, 2] + K[3])
    f = np.concatenate([u, w])
    return float(np.abs(f - np.floor(f) - 0.5).min())


def deformed_icosphere(level=2, scale=(40.0, 28.0, 20.0), bump=0.35):
    """An icosphere with unequal axes and one off-axis bump, so that its silhouette pins the rotation."""
    v, f = RR.icosphere(level)
    v = v.astype(np.float64)
    c = np.array([0.6, 0.5, 0.62])
    c /= np.linalg.norm(c)
    g = np.exp(-((v - c) ** 2).sum(1) / 0.15)
    v = v * (1.0 + bump * g)[:, None] * np.asarray(scale)
    return v.astype(np.float32), f


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    return exp_so3(a / np.linalg.norm(a) * angle)


def add_error(verts, R, t, Rg, tg):
    v = np.asarray(verts, np.float64)
    return float(np.linalg.norm((v @ np.asarray(R).reshape(3, 3).T + t) - (v @ np.asarray(Rg).reshape(3, 3).T + tg),
                                axis=1).mean())
