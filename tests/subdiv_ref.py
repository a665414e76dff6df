"""numpy restatement of the mesh upsampling (zp_mesh_subdivide, include/zp.h): the executable
definition the kernels of csrc/zp_subdiv.hip match bit for bit, one pass (`subdivide_pass`) and the two
drivers of zebrapose_amd.meshcode (`subdivide_midpoint`, `upsample_mesh`).  Needs no torch; the faces
are walked in a plain loop.  Also the small meshes and the mesh checks the subdivision tests share."""
import numpy as np

NO_BUDGET = (1 << 31) - 1


def len2(a, b):
    """(dx dx + dy dy) + dz dz of f32 positions in f64, every operation rounded once."""
    d = np.asarray(a, np.float32).astype(np.float64) - np.asarray(b, np.float32).astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def subdivide_pass(verts, faces, abs2=0.0, rel2=0.0, max_split=NO_BUDGET):
    """One pass -> dict(vertices f32 [nv_out, 3], faces i32 [nf_out, 3], parents i32 [nv_out, 2],
    counts i64 [4] = (n_unique_edges, n_split, nv_out, nf_out), max_len2 f64)."""
    v = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    nv = len(v)
    f = np.clip(np.asarray(faces).astype(np.int64).reshape(-1, 3), 0, nv - 1)
    nf = len(f)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)  # slot 3 i + j is (vj, v(j+1)%3) of face i
    keys = (np.minimum(a, b) << 32) | np.maximum(a, b)
    ekey, slot_edge = np.unique(keys, return_inverse=True)  # ascending key order
    slot_edge = slot_edge.reshape(-1)
    lo, hi = ekey >> 32, ekey & 0xFFFFFFFF
    l2 = len2(v[lo], v[hi])
    mx = np.float64(l2.max())
    qual = (l2 > np.float64(abs2)) & (l2 > np.float64(rel2) * mx)
    split = qual.copy()
    if qual.sum() > max_split:
        q = np.flatnonzero(qual)
        order = q[np.argsort(-l2[q], kind="stable")]  # longest first, ties to the lower key
        split[:] = False
        split[order[:max_split]] = True
    n_split = int(split.sum())
    new_id = nv + np.cumsum(split) - 1  # valid where split
    mid = ((v[lo[split]].astype(np.float64) + v[hi[split]].astype(np.float64)) * 0.5).astype(np.float32)
    ov = np.concatenate([v, mid])
    parents = np.concatenate([np.stack([np.arange(nv)] * 2, 1), np.stack([lo[split], hi[split]], 1)]).astype(np.int32)
    out = []
    for i in range(nf):
        e = slot_edge[3 * i:3 * i + 3]
        s = split[e]
        m = new_id[e]
        p = f[i]
        k = int(s.sum())
        if k == 0:
            out.append((p[0], p[1], p[2]))
        elif k == 3:
            out += [(p[0], m[0], m[2]), (m[0], p[1], m[1]), (m[2], m[1], p[2]), (m[0], m[1], m[2])]
        elif k == 1:
            r = int(np.flatnonzero(s)[0])
            v0, v1, v2, m01 = p[r], p[(r + 1) % 3], p[(r + 2) % 3], m[r]
            out += [(v0, m01, v2), (m01, v1, v2)]
        else:
            r = (int(np.flatnonzero(~s)[0]) + 1) % 3
            v0, v1, v2, m01, m12 = p[r], p[(r + 1) % 3], p[(r + 2) % 3], m[r], m[(r + 1) % 3]
            out.append((m01, v1, m12))
            if len2(ov[m01], ov[v2]) < len2(ov[v0], ov[m12]):
                out += [(v0, m01, v2), (m01, m12, v2)]
            else:
                out += [(v0, m01, m12), (v0, m12, v2)]
    of = np.array(out, np.int64).reshape(-1, 3).astype(np.int32)
    return {"vertices": ov, "faces": of, "parents": parents, "max_len2": mx,
            "counts": np.array([len(ekey), n_split, len(ov), len(of)], np.int64)}


def _merge_parents(parents, res, nv_before):
    p = res["parents"].copy()
    p[:nv_before] = parents
    return p


def subdivide_midpoint(verts, faces, iterations=1, threshold=0.0):
    """`iterations` passes with abs2 = threshold^2 -> dict(vertices, faces, parents, pass_sizes)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int32).reshape(-1, 3)
    parents = np.stack([np.arange(len(v), dtype=np.int32)] * 2, 1)
    sizes = []
    t = np.float64(threshold)
    for _ in range(iterations):
        r = subdivide_pass(v, f, abs2=t * t)
        parents = _merge_parents(parents, r, len(v))
        v, f = r["vertices"], r["faces"]
        sizes.append(len(v))
    return {"vertices": v, "faces": f, "parents": parents, "pass_sizes": sizes}


def upsample_mesh(verts, faces, min_vertices=65537, max_passes=64):
    """Passes with rel2 = 0.25 and a budget of the vertices still missing, until nv >= min_vertices."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int32).reshape(-1, 3)
    parents = np.stack([np.arange(len(v), dtype=np.int32)] * 2, 1)
    sizes, longest = [], []
    while len(v) < min_vertices:
        if len(sizes) == max_passes:
            raise ValueError("max_passes reached")
        r = subdivide_pass(v, f, abs2=0.0, rel2=0.25, max_split=min_vertices - len(v))
        if r["counts"][1] == 0:
            raise ValueError("a pass split nothing")
        parents = _merge_parents(parents, r, len(v))
        v, f = r["vertices"], r["faces"]
        sizes.append(len(v))
        longest.append(float(r["max_len2"]))
    return {"vertices": v, "faces": f, "parents": parents, "pass_sizes": sizes, "max_len2": longest}


def lift(attr, parents, n_input, pass_sizes):
    """A per-vertex attribute of the input mesh carried to the output: parents' average, pass by pass, f64."""
    a = np.asarray(attr, np.float64)
    prev = n_input
    for n in pass_sizes:
        p = parents[prev:n]
        a = np.concatenate([a, (a[p[:, 0]] + a[p[:, 1]]) * 0.5])
        prev = n
    return a


# ---- mesh checks -----------------------------------------------------------------------------

def area(verts, faces):
    p = np.asarray(verts, np.float64)[np.asarray(faces)]
    return float(0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum())


def is_closed_manifold(faces):
    """Every directed edge occurs once and its reverse exactly once (no boundary, no T-junction)."""
    f = np.asarray(faces).astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    k = (d[:, 0] << 32) | d[:, 1]
    r = (d[:, 1] << 32) | d[:, 0]
    return len(np.unique(k)) == len(k) and np.array_equal(np.sort(k), np.sort(r))


def longest_edge2(verts, faces):
    f = np.asarray(faces)
    v = np.asarray(verts, np.float32)
    return float(max(len2(v[f[:, j]], v[f[:, (j + 1) % 3]]).max() for j in range(3)))


# ---- meshes ----------------------------------------------------------------------------------

def tetrahedron():
    v = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float32)
    f = np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)
    return v, f


def box(sx=100.0, sy=10.0, sz=1.0):
    """An axis-aligned box of 8 vertices and 12 outward-facing triangles."""
    v = np.array([(x, y, z) for x in (0, sx) for y in (0, sy) for z in (0, sz)], np.float32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def strip(n):
    """A strip of n triangles over two rows of vertices with uneven spacing (lengths differ)."""
    k = n // 2 + 2
    x = np.cumsum(1.0 + 0.25 * (np.arange(k) % 3))
    v = np.concatenate([np.stack([x, np.zeros(k), 0.1 * np.arange(k)], 1),
                        np.stack([x + 0.5, np.full(k, 1.5), np.zeros(k)], 1)]).astype(np.float32)
    f = []
    for i in range(n):
        j = i // 2
        f.append((j, j + 1, k + j) if i % 2 == 0 else (j + 1, k + j + 1, k + j))
    return v, np.array(f, np.int32)
