"""numpy restatement of the d-ary mesh coder (zp_mesh_code_radix, include/zp.h): the executable
definition the kernels of csrc/zp_meshcode_radix.hip match bit for bit.  All clustering arithmetic is
int64 and exact, vectorised per level over all groups.  A level's groups are laid out as rows of one
[G, nmax] table (ascending vertex index along a row, padded at the end: a level's group sizes differ
by little), so that a group's d centres broadcast along its row.  The grid, the face rule, the LUT
and the test meshes are those of tests/meshcode_ref.py."""
import numpy as np

from tests.meshcode_ref import (IDX_BITS, IDX_MASK, eps2_q, face_ids_from, grid_log2, lut_from,  # noqa: F401
                                quantize)

BIG = np.iinfo(np.int64).max
CHUNK = 1 << 19  # entries of a [points, d] block worked on at a time


def draws_per_attempt(d, levels):
    return (d ** levels - 1) // (d - 1)


def sample_draws(seed, attempts, d, levels):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(attempts, draws_per_attempt(d, levels)),
                                                dtype=np.uint32)


def _dist2_blocks(P, c, rel=False):
    """Yields (group slice, rank slice, d^2 of those points of P [G, n, 3] to the d centres c [G, d, 3] of
    their row, int64 [.., .., d]) over blocks of about CHUNK entries: |p|^2 - 2 p.c + |c|^2, below 2^42.
    rel: without |p|^2, which moves no comparison between the centres of one point."""
    G, n, d = len(P), P.shape[1], c.shape[1]
    c2, ct = (c ** 2).sum(-1), -2 * c.transpose(0, 2, 1)
    gstep, pstep = max(1, CHUNK // (n * d)), max(1, CHUNK // d)  # whole rows while they are small, else pieces of one
    for g in range(0, G, gstep):
        for a in range(0, n, pstep):
            gsl, psl = slice(g, g + gstep), slice(a, a + pstep)
            D = np.matmul(P[gsl, psl], ct[gsl])
            D += c2[gsl, None, :]
            if not rel:
                D += (P[gsl, psl] ** 2).sum(-1)[..., None]
            yield gsl, psl, D


def _labels(P, c):
    """-> nearest centre of every point, ties to the lowest class, int64 [G, n]."""
    lab = np.empty(P.shape[:2], np.int64)
    for gsl, psl, D in _dist2_blocks(P, c, rel=True):
        lab[gsl, psl] = D.argmin(2)
    return lab


def _nearest_d2(P, c):
    """-> d^2 of every point to its nearest centre, int64 [G, n]."""
    dmin = np.empty(P.shape[:2], np.int64)
    for gsl, psl, D in _dist2_blocks(P, c):
        dmin[gsl, psl] = D.min(2)
    return dmin


def _group_sums(slot, val, n):
    s = np.zeros((n,) + val.shape[1:], np.int64)
    np.add.at(s, slot, val)
    return s


def split_levels(q, d, levels, draws, iterations, eps2):
    """-> list over levels of the per-vertex group id *after* that level (level l: ids in [0, d^(l+1)))."""
    nv = len(q)
    attempts = len(draws)
    gid = np.zeros(nv, np.int64)
    out = []
    for l in range(levels):
        G = d ** l
        first = (G - 1) // (d - 1)
        order = np.argsort(gid, kind="stable")  # groups contiguous, ascending vertex index inside
        gs = gid[order]
        start = np.searchsorted(gs, np.arange(G))
        n = np.diff(np.append(start, nv))
        assert n.min() >= d ** (levels - l)
        nmax = int(n.max())
        col = np.arange(nv) - start[gs]
        idx = np.full((G, nmax), -1, np.int64)  # vertex index of (group, rank); -1: padding
        idx[gs, col] = order
        valid = idx >= 0
        P = q[np.maximum(idx, 0)]
        rows = np.arange(G)
        Px, Py, Pz = (np.ascontiguousarray(P[..., x]) for x in range(3))
        tag = IDX_MASK - np.maximum(idx, 0)
        vg, vp = gs, P[valid]  # group and grid point of the valid entries, in sorted order
        best_c = best_comp = None
        for a in range(attempts):
            r = draws[a, first:first + G].astype(np.int64)
            c = np.empty((G, d, 3), np.int64)
            c[:, 0] = P[rows, (r * n) >> 32]
            mind = np.where(valid, BIG >> IDX_BITS, -1)  # padding stays below every vertex's key
            for j in range(1, d):  # farthest-point seeds: largest min d^2, ties to the lowest vertex index
                dj = (Px - c[:, j - 1, 0, None]) ** 2
                dj += (Py - c[:, j - 1, 1, None]) ** 2
                dj += (Pz - c[:, j - 1, 2, None]) ** 2
                np.minimum(mind, dj, out=mind)
                key = ((mind << IDX_BITS) | tag).max(1)
                c[:, j] = q[IDX_MASK - (key & IDX_MASK)]
            active = np.ones(G, bool)
            for _ in range(iterations):
                lab = _labels(P, c)  # ties -> the lowest class
                slot = vg * d + lab[valid]
                cnt = np.bincount(slot, minlength=G * d).reshape(G, d)
                S = _group_sums(slot, vp, G * d).reshape(G, d, 3)
                newc = (2 * S + cnt[..., None]) // (2 * np.maximum(cnt, 1))[..., None]  # floor division
                newc = np.where(cnt[..., None] > 0, newc, c)  # an empty class keeps its centre
                worst = ((newc - c) ** 2).sum(-1).max(1)
                c = np.where(active[:, None, None], newc, c)
                active &= worst > eps2
                if not active.any():
                    break
            comp = _group_sums(vg, _nearest_d2(P, c)[valid], G)
            if a == 0:
                best_c, best_comp = c, comp
            else:
                better = comp < best_comp  # ties -> the lowest attempt
                best_c = np.where(better[:, None, None], c, best_c)
                best_comp = np.where(better, comp, best_comp)
        # the peel: class j takes the floor(|U_j| / (d - j)) vertices of U_j with the lowest
        # D[p][j] - min_{i > j} D[p][i], ties to the lower vertex index
        score = np.empty((d - 1, G, nmax), np.int64)
        for gsl, psl, D in _dist2_blocks(P, best_c):
            sfx = np.minimum.accumulate(D[..., ::-1], axis=2)[..., ::-1]  # sfx[.., i] = min over classes >= i
            score[:, gsl, psl] = np.moveaxis(D[..., :-1] - sfx[..., 1:], 2, 0)
        digit = np.full((G, nmax), d - 1, np.int64)
        alive = valid.copy()
        u = n.copy()
        for j in range(d - 1):
            k = u // (d - j)
            key = np.where(alive, score[j] * (1 << IDX_BITS) + idx, BIG)  # |score| < 2^42: no overflow, no ties
            part = np.partition(key, np.unique(k - 1), axis=1)
            take = key <= part[rows, k - 1][:, None]
            assert np.array_equal(take.sum(1), k)
            digit[take] = j
            alive &= ~take
            u = u - k
        gid = np.empty(nv, np.int64)
        gid[order] = gs * d + digit[valid]
        out.append(gid.copy())
    return out


def encode(verts, faces, d, levels, attempts=3, iterations=10, eps=1.0, seed=0, return_levels=False):
    """-> dict(vertex_ids i32 [nv], face_ids i32 [nf], lut f64 [d^levels, 3], levels (optional))."""
    verts = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    s = d.bit_length() - 1
    assert 4 <= d <= 256 and d == 1 << s and levels >= 1 and d ** levels <= 65536
    assert np.isfinite(verts).all() and d ** levels <= len(verts) <= 1 << IDX_BITS
    k = grid_log2(verts)
    lv = split_levels(quantize(verts, k), d, levels, sample_draws(seed, attempts, d, levels), iterations,
                      eps2_q(eps, k))
    vid = lv[-1]  # sum_l digit_l * d^(levels - 1 - l) is the last level's group id
    fid = face_ids_from(vid, faces)
    res = {"vertex_ids": vid.astype(np.int32), "face_ids": fid.astype(np.int32),
           "lut": lut_from(verts, faces, fid, s * levels)}
    if return_levels:
        res["levels"] = lv
    return res
