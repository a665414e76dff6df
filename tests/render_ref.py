"""numpy restatement of zp_render (include/zp.h): the executable definition of its semantics.

Every f64 step below is one IEEE operation, written in the order the device code performs it, and
every integer step is exact int64, so the HIP kernels (csrc/zp_render.hip) must reproduce the
outputs bit for bit.  Reads nothing outside the repository.

Conventions: pixel column x / row y is sampled at (x + 1/2, y + 1/2), i.e. (256 x + 128, 256 y + 128)
in the 1/256-pixel units the vertices are snapped to.  For vertices a, b and a point p
    E(a, b, p) = (bx - ax) (py - ay) - (by - ay) (px - ax)
and a triangle (v0, v1, v2) has A = E(v0, v1, v2), E12 = E(v1, v2, p), E20 = E(v2, v0, p),
E01 = E(v0, v1, p) (E12 + E20 + E01 == A).  With s = sign(A), p is inside when every s E is > 0, or
== 0 on a top-left edge.  Edge a -> b, direction d = s (b - a), has the interior on the side
(-dy, dx); it is a LEFT edge when dy < 0 (interior towards +x) and a TOP edge when dy == 0 and
dx > 0 (interior towards +y, image rows growing downwards).  The neighbour across a shared edge
walks it in the opposite direction, so exactly one of the two owns a sample lying on it.
"""
from __future__ import annotations

import numpy as np

SUB = 256            # snapped units per pixel
SAT = float(1 << 28)  # snapped coordinates saturate here: edge functions stay below 2^60


def snap_vertices(verts, R, t, K, z_near):
    """verts f32 [nv, 3]; R f64 [9]; t f64 [3]; K f64 [4] -> (xi int64 [nv], yi int64 [nv],
    w f64 [nv] = 1 / Zc, ok bool [nv]).  A vertex is not ok when Zc >= z_near fails (a NaN fails)
    or its projection is NaN; every triangle touching it is discarded."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = (np.float64(k) for k in np.asarray(K, np.float64).reshape(4))
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        Xc = ((R[0] * x + R[1] * y) + R[2] * z) + t[0]
        Yc = ((R[3] * x + R[4] * y) + R[5] * z) + t[1]
        Zc = ((R[6] * x + R[7] * y) + R[8] * z) + t[2]
        u = (fx * Xc) / Zc + cx
        w_ = (fy * Yc) / Zc + cy
        ok = (Zc >= np.float64(z_near)) & ~np.isnan(u) & ~np.isnan(w_)
        xs = np.clip(np.rint(u * 256.0), -SAT, SAT)
        ys = np.clip(np.rint(w_ * 256.0), -SAT, SAT)
        inv = 1.0 / Zc
    xi = np.where(ok, xs, 0.0).astype(np.int64)
    yi = np.where(ok, ys, 0.0).astype(np.int64)
    return xi, yi, np.where(ok, inv, 0.0), ok


def icosphere(level):
    """Unit icosphere by `level` midpoint subdivisions: (verts f32 [nv, 3], faces i32 [20 * 4^level, 3]),
    outward winding, shared vertices."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(a, np.float64) / np.linalg.norm(a) for a in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                c = v[a] + v[b]
                v.append(c / np.linalg.norm(c))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int32)


def box_samples(verts, faces, R, t, K, H, W, z_near=1e-6):
    """Samples in each face's clipped bounding box for one render (0 for a discarded face): which of
    zp_render's two paths a face takes (in-thread up to 16 samples, the list beyond)."""
    xi, yi, w, ok = snap_vertices(verts, R, t, K, z_near)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    x, y = xi[f], yi[f]
    bx0 = np.maximum((x.min(1) + 127) >> 8, 0)
    bx1 = np.minimum((x.max(1) - 128) >> 8, W - 1)
    by0 = np.maximum((y.min(1) + 127) >> 8, 0)
    by1 = np.minimum((y.max(1) - 128) >> 8, H - 1)
    A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    keep = ok[f].all(1) & (A != 0) & (bx0 <= bx1) & (by0 <= by1)
    return np.where(keep, (bx1 - bx0 + 1) * (by1 - by0 + 1), 0)


def _keys_one(verts, faces, R, t, K, H, W, z_near):
    """The per-pixel key plane u64 [H, W] of one render: invz_bits << 32 | (0xFFFFFFFF - face), 0 =
    background; the largest key wins."""
    xi, yi, w, ok = snap_vertices(verts, R, t, K, z_near)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(xi)
    fid = np.arange(len(faces), dtype=np.int64)
    inr = np.all((faces >= 0) & (faces < nv), axis=1)  # an index outside the mesh discards the face
    fc = np.where(inr[:, None], faces, 0)
    i0, i1, i2 = fc[:, 0], fc[:, 1], fc[:, 2]
    keep = inr & ok[i0] & ok[i1] & ok[i2]
    x0, y0, x1, y1, x2, y2 = xi[i0], yi[i0], xi[i1], yi[i1], xi[i2], yi[i2]
    A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    keep &= A != 0
    # pixels whose sample lies in the closed bounding box, clipped to the image
    bx0 = np.maximum((np.minimum(np.minimum(x0, x1), x2) + 127) >> 8, 0)
    bx1 = np.minimum((np.maximum(np.maximum(x0, x1), x2) - 128) >> 8, W - 1)
    by0 = np.maximum((np.minimum(np.minimum(y0, y1), y2) + 127) >> 8, 0)
    by1 = np.minimum((np.maximum(np.maximum(y0, y1), y2) - 128) >> 8, H - 1)
    keep &= (bx0 <= bx1) & (by0 <= by1)
    keys = np.zeros(H * W, np.uint64)
    sel = np.nonzero(keep)[0]
    if len(sel) == 0:
        return keys.reshape(H, W)
    bw = (bx1 - bx0 + 1)[sel]
    cnt = bw * (by1 - by0 + 1)[sel]
    rep = np.repeat(np.arange(len(sel)), cnt)          # candidate -> position in sel
    k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    f = sel[rep]
    px = bx0[f] + k % bw[rep]
    py = by0[f] + k // bw[rep]
    sx, sy = px * SUB + 128, py * SUB + 128
    s = np.sign(A[f])

    def edge(ax, ay, bx, by):
        dx, dy = bx - ax, by - ay
        E = dx * (sy - ay) - dy * (sx - ax)
        tl = (s * dy < 0) | ((dy == 0) & (s * dx > 0))
        return E, (s * E > 0) | ((E == 0) & tl)

    E12, in12 = edge(x1[f], y1[f], x2[f], y2[f])
    E20, in20 = edge(x2[f], y2[f], x0[f], y0[f])
    E01, in01 = edge(x0[f], y0[f], x1[f], y1[f])
    ins = in12 & in20 & in01
    f, px, py, E12, E20, E01 = (a[ins] for a in (f, px, py, E12, E20, E01))
    q = (E12.astype(np.float64) * w[i0[f]] + E20.astype(np.float64) * w[i1[f]]) + E01.astype(np.float64) * w[i2[f]]
    invz = (q / A[f].astype(np.float64)).astype(np.float32)
    key = (invz.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - fid[f].astype(np.uint64))
    np.maximum.at(keys, py * W + px, key)
    return keys.reshape(H, W)


def resolve(keys, face_bgr=None):
    """keys u64 [..., H, W] -> dict(color u8 [..., 3] if face_bgr is given, depth f32, mask u8, face i32)."""
    fg = keys != 0
    face = np.where(fg, np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF)), 0).astype(np.int64)
    invz = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        depth = np.where(fg, (1.0 / invz.astype(np.float64)).astype(np.float32), np.float32(0))
    out = {"depth": depth.astype(np.float32), "mask": np.where(fg, 255, 0).astype(np.uint8),
           "face": np.where(fg, face, -1).astype(np.int32)}
    if face_bgr is not None:
        fb = np.asarray(face_bgr, np.uint8).reshape(-1, 3)
        out["color"] = np.where(fg[..., None], fb[face], 0).astype(np.uint8)
    return out


def render(verts, faces, face_bgr, R, t, K, H, W, z_near=1e-6):
    """B renders of one mesh: R [B, 9] (or [B, 3, 3]), t [B, 3], K [B, 4] = (fx, fy, cx, cy).
    Returns dict of color u8 [B, H, W, 3], depth f32 [B, H, W], mask u8 [B, H, W], face i32 [B, H, W]."""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(-1, 4)
    keys = np.stack([_keys_one(verts, faces, R[b], t[b], K[b], H, W, z_near) for b in range(len(R))])
    return resolve(keys, face_bgr)
