"""numpy restatement of the mesh coder (zp_mesh_code, include/zp.h): the executable definition the
kernels of csrc/zp_meshcode.hip match bit for bit.  All clustering arithmetic is int64 and exact,
vectorised per level over all groups; the LUT's f64 sums are single additions in ascending face
index, vertex 0, 1, 2.  Also the small meshes the mesh-coder tests share."""
from fractions import Fraction

import numpy as np

SAT = (1 << 19) - 1
IDX_BITS = 21
IDX_MASK = (1 << IDX_BITS) - 1


# ---- host-side parameters --------------------------------------------------------------------

def grid_log2(verts):
    """The largest k in [-40, 40] with rint(max|v| * 2^k) <= 2^19 - 1, so no coordinate saturates."""
    m = float(np.abs(np.asarray(verts, np.float32).astype(np.float64)).max())
    for k in range(40, -41, -1):
        if np.rint(np.ldexp(m, k)) <= SAT:
            return k
    raise ValueError("mesh too large for the grid")


def eps2_q(eps, k):
    """floor((eps * 2^k)^2), exactly; capped at 2^62 (a centre shift^2 is below 2^42)."""
    return min(int((Fraction(float(eps)) * Fraction(2) ** k) ** 2), 1 << 62)


def sample_draws(seed, attempts, bits):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(attempts, (1 << bits) - 1), dtype=np.uint32)


def quantize(verts, k):
    q = np.rint(np.ldexp(np.asarray(verts, np.float32).astype(np.float64), k))
    return np.clip(q, -SAT, SAT).astype(np.int64)


# ---- the split -------------------------------------------------------------------------------

def _labels(P, c, gs):
    """(label, d^2 to centre 0, d^2 to centre 1) of the sorted points P under centres c [G, 2, 3]."""
    d0 = ((P - c[gs, 0]) ** 2).sum(1)
    d1 = ((P - c[gs, 1]) ** 2).sum(1)
    return (d1 < d0).astype(np.int64), d0, d1  # ties -> class 0


def split_levels(q, bits, draws, iterations, eps2):
    """-> list over levels of the per-vertex group id *after* that level (level l: ids in [0, 2^(l+1)))."""
    nv = len(q)
    attempts = len(draws)
    gid = np.zeros(nv, np.int64)
    out = []
    for l in range(bits):
        G = 1 << l
        order = np.argsort(gid, kind="stable")  # groups contiguous, ascending vertex index inside
        gs = gid[order]
        start = np.searchsorted(gs, np.arange(G))
        n = np.diff(np.append(start, nv))
        assert n.min() >= 2
        P = q[order]
        best_c = best_comp = None
        for a in range(attempts):
            r = draws[a, G - 1:2 * G - 1].astype(np.int64)
            c0 = P[start + ((r * n) >> 32)]
            d = ((P - c0[gs]) ** 2).sum(1)
            far = np.maximum.reduceat((d << IDX_BITS) | (IDX_MASK - order), start)
            c = np.stack([c0, q[IDX_MASK - (far & IDX_MASK)]], 1)
            active = np.ones(G, bool)
            for _ in range(iterations):
                lab, _, _ = _labels(P, c, gs)
                newc = c.copy()
                worst = np.zeros(G, np.int64)
                for j in (0, 1):
                    m = (lab == j).astype(np.int64)
                    cnt = np.add.reduceat(m, start)
                    S = np.add.reduceat(P * m[:, None], start, axis=0)
                    cj = (2 * S + cnt[:, None]) // (2 * np.maximum(cnt, 1))[:, None]  # floor division
                    cj = np.where(cnt[:, None] > 0, cj, c[:, j])  # an empty class keeps its centre
                    worst = np.maximum(worst, ((cj - c[:, j]) ** 2).sum(1))
                    newc[:, j] = cj
                c = np.where(active[:, None, None], newc, c)
                active &= worst > eps2
                if not active.any():
                    break
            lab, d0, d1 = _labels(P, c, gs)
            comp = np.add.reduceat(np.where(lab == 0, d0, d1), start)
            if a == 0:
                best_c, best_comp = c, comp
            else:
                better = comp < best_comp  # ties -> the lowest attempt
                best_c = np.where(better[:, None, None], c, best_c)
                best_comp = np.where(better, comp, best_comp)
        lab, d0, d1 = _labels(P, best_c, gs)
        other = np.where(lab == 0, d1, d0)
        cnt0 = np.add.reduceat((lab == 0).astype(np.int64), start)
        m = n // 2
        perm = np.lexsort((np.arange(nv), -other, lab, gs))  # (group, class, d^2 descending, index ascending)
        rank = np.empty(nv, np.int64)
        rank[perm] = np.arange(nv)
        rank -= start[gs] + np.where(lab == 1, cnt0[gs], 0)
        over = np.where(lab == 0, cnt0[gs], n[gs] - cnt0[gs]) > m[gs]
        bit = lab ^ (over & (rank >= m[gs])).astype(np.int64)
        gid = np.empty(nv, np.int64)
        gid[order] = 2 * gs + bit
        out.append(gid.copy())
    return out


def face_ids_from(vertex_ids, faces):
    i0, i1, i2 = (np.asarray(vertex_ids)[np.asarray(faces)[:, j]] for j in range(3))
    return np.where((i0 == i1) | (i0 == i2), i0, np.where(i1 == i2, i1, i0))


def lut_from(verts, faces, face_ids, bits):
    """f64 mean per class over its faces' vertices, summed in ascending face index, vertex 0, 1, 2."""
    C = 1 << bits
    fo = np.argsort(face_ids, kind="stable")
    pts = np.asarray(verts, np.float32)[np.asarray(faces)[fo]].astype(np.float64).reshape(-1, 3)
    cnt = 3 * np.bincount(face_ids, minlength=C)
    st = np.cumsum(cnt) - cnt
    s = np.zeros((C, 3))
    for r in range(int(cnt.max())):
        sel = cnt > r
        s[sel] = s[sel] + pts[st[sel] + r]
    lut = np.full((C, 3), np.nan)
    has = cnt > 0
    lut[has] = s[has] / cnt[has, None].astype(np.float64)
    return lut


def encode(verts, faces, bits, attempts=3, iterations=10, eps=1.0, seed=0, return_levels=False):
    """-> dict(vertex_ids i32 [nv], face_ids i32 [nf], lut f64 [2^bits, 3], levels (optional))."""
    verts = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    assert np.isfinite(verts).all() and (1 << bits) <= len(verts) <= 1 << IDX_BITS
    k = grid_log2(verts)
    levels = split_levels(quantize(verts, k), bits, sample_draws(seed, attempts, bits), iterations, eps2_q(eps, k))
    vid = levels[-1]  # the bits assembled MSB first are the last level's group id
    fid = face_ids_from(vid, faces)
    res = {"vertex_ids": vid.astype(np.int32), "face_ids": fid.astype(np.int32), "lut": lut_from(verts, faces, fid, bits)}
    if return_levels:
        res["levels"] = levels
    return res


# ---- meshes ----------------------------------------------------------------------------------

def icosphere(level):
    """Unit icosphere: (verts f32 [10 * 4^level + 2, 3], faces i32 [20 * 4^level, 3])."""
    p = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
                  (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)], np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
                  (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11),
                  (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[ue[:, 0]] + v[ue[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)
        v = np.concatenate([v, mid])
        a, b, c = f.T
        f = np.concatenate([np.stack(t, 1) for t in ((a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2]))])
    return v.astype(np.float32), f.astype(np.int32)


def fan_faces(nv):
    """Two dummy faces per vertex: (i, i + 1, i + 2) and (i, i + 3, i + 7), indices modulo nv."""
    i = np.arange(nv)
    return np.concatenate([np.stack([i, (i + 1) % nv, (i + 2) % nv], 1),
                           np.stack([i, (i + 3) % nv, (i + 7) % nv], 1)]).astype(np.int32)


def lattice():
    """16 x 16 x 4 integer lattice (1024 vertices, many exact ties), two dummy-fan faces per vertex."""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32), fan_faces(len(g))


def random_points(n, seed):
    v = np.random.default_rng(seed).uniform(-100, 100, (n, 3)).astype(np.float32)
    return v, fan_faces(n)


def duplicate_mesh():
    """64 copies of one vertex in front of a 162-vertex sphere: groups of identical points."""
    v, f = icosphere(2)
    v = np.concatenate([np.tile(np.array([[0.25, -0.5, 0.125]], np.float32), (64, 1)), v * np.float32(50)])
    return v, np.concatenate([f + 64, fan_faces(64)]).astype(np.int32)


def blobs(count):
    """`count` equal icospheres (162 vertices, radius 1) ten radii apart along x; vertices interleaved."""
    v, f = icosphere(2)
    vs = np.stack([v + np.array([10.0 * i, 0, 0], np.float32) for i in range(count)], 1).reshape(-1, 3)
    fs = np.concatenate([f * count + i for i in range(count)])
    return vs.astype(np.float32), fs.astype(np.int32), np.tile(np.arange(count), len(v))
