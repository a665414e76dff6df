"""numpy restatement of zp_render_shaded's shading pass (include/zp.h): the executable definition
of its semantics.  Visibility is tests/render_ref.py's key plane; every f64 step below is one IEEE
operation in the order the device code (csrc/zp_shade.hip) performs it, and only + - * / and sqrt
occur, so the kernels must reproduce ``shaded`` bit for bit.  Reads nothing outside the repository.
"""
from __future__ import annotations

import numpy as np

from tests import render_ref as RR


def unit(v):
    """v [..., 3] / sqrt((x x + y y) + z z); a vector whose length is not > 0 becomes zero."""
    with np.errstate(all="ignore"):
        l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]
        return np.where(l > 0, v / l, 0.0)


def vertex_attributes(verts, normals, R, t, light):
    """Per vertex of one render: (P, n_e, L_v) f64 [nv, 3]."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    n = np.asarray(normals, np.float32).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    lp = np.asarray(light, np.float64).reshape(-1)[:3]
    with np.errstate(all="ignore"):
        P = np.stack([((R[3 * k] * v[:, 0] + R[3 * k + 1] * v[:, 1]) + R[3 * k + 2] * v[:, 2]) + t[k] for k in range(3)], 1)
        m = np.stack([(R[3 * k] * n[:, 0] + R[3 * k + 1] * n[:, 1]) + R[3 * k + 2] * n[:, 2] for k in range(3)], 1)
        return P, unit(m), unit(lp[None, :] - P)


def _shade_one(keys, verts, faces, normals, rgb, R, t, K, light, z_near):
    H, W = keys.shape
    out = np.zeros((H, W, 3), np.uint8)
    ys, xs = np.nonzero(keys)
    if len(ys) == 0:
        return out
    f = (np.uint64(0xFFFFFFFF) - (keys[ys, xs] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    i0, i1, i2 = faces[f, 0], faces[f, 1], faces[f, 2]
    xi, yi, w, _ = RR.snap_vertices(verts, R, t, K, z_near)
    sx, sy = xs.astype(np.int64) * RR.SUB + 128, ys.astype(np.int64) * RR.SUB + 128

    def edge(a, b):
        return (xi[b] - xi[a]) * (sy - yi[a]) - (yi[b] - yi[a]) * (sx - xi[a])

    with np.errstate(all="ignore"):
        b0 = edge(i1, i2).astype(np.float64) * w[i0]
        b1 = edge(i2, i0).astype(np.float64) * w[i1]
        b2 = edge(i0, i1).astype(np.float64) * w[i2]
        q = (b0 + b1) + b2

        def interp(a):  # a [nv, 3]
            return ((b0[:, None] * a[i0] + b1[:, None] * a[i1]) + b2[:, None] * a[i2]) / q[:, None]

        P, ne, Lv = vertex_attributes(verts, normals, R, t, light)
        c = interp(np.asarray(rgb, np.uint8).astype(np.float64) / 255.0)
        N, Ld, Vd = unit(interp(ne)), unit(interp(Lv)), unit(interp(-P))
        nl = (N[:, 0] * Ld[:, 0] + N[:, 1] * Ld[:, 1]) + N[:, 2] * Ld[:, 2]
        d = np.where(nl > 0, nl, 0.0)
        Rv = (2.0 * nl)[:, None] * N - Ld
        rv = (Rv[:, 0] * Vd[:, 0] + Rv[:, 1] * Vd[:, 1]) + Rv[:, 2] * Vd[:, 2]
        s = np.where(rv > 0, rv, 0.0)
        ka, kd, ks = (np.float64(x) for x in np.asarray(light, np.float64).reshape(-1)[3:6])
        o = (ka * c + kd * (d[:, None] * c)) + ks * (s[:, None] * c)
        o = np.where(o > 1.0, 1.0, o)
        byte = np.rint(255.0 * o)
        byte = np.where(byte > 0, byte, 0.0)  # a negative or NaN sum gives 0
    out[ys, xs] = byte.astype(np.uint8)[:, ::-1]  # stored B, G, R
    return out


def render_shaded(verts, faces, normals, rgb, R, t, K, light, H, W, z_near=1e-6, face_bgr=None):
    """B shaded renders of one mesh: R [B, 9], t [B, 3], K [B, 4], light [B, 6] = (lx, ly, lz, ka, kd, ks).
    Returns render_ref.render's dict (color only with face_bgr) plus shaded u8 [B, H, W, 3] (B, G, R)."""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(-1, 4)
    light = np.asarray(light, np.float64).reshape(-1, 6)
    keys = np.stack([RR._keys_one(verts, faces, R[b], t[b], K[b], H, W, z_near) for b in range(len(R))])
    out = RR.resolve(keys, face_bgr)
    out["shaded"] = np.stack([_shade_one(keys[b], verts, faces, normals, rgb, R[b], t[b], K[b], light[b], z_near)
                              for b in range(len(R))])
    return out
