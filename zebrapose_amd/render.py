"""GT code images, depth and masks rendered from a mesh on the device (``zp_render``,
csrc/zp_render.hip).

The reference makes its GT code images with an OpenGL program
(Binary_Code_GT_Generator/Render_GT_Color_Mesh_to_GT_Img, driven by
generate_training_labels_for_BOP_v2.py): it draws ``models_GT_color/obj_*.ply`` at the GT pose, without
antialiasing, and saves a PNG that the data loader reads back.  ``MeshRenderer`` draws the same
mesh with a batched HIP rasteriser; its ``color`` / ``mask`` stacks are what ``CropPipeline`` takes
as ``gt_images`` / ``entire_masks``.  The exact semantics are in include/zp.h (zp_render) and, as
numpy, in tests/render_ref.py.

``MeshRenderer.render_shaded`` adds the Phong-shaded colour image of a vertex-coloured model
(``zp_render_shaded``, csrc/zp_shade.hip: the reference's lib/meshrenderer/meshrenderer_phong.py),
from the same visibility pass; ``vertex_normals`` makes normals for a mesh that carries none, and
zebrapose_amd/synth.py pastes the renders over backgrounds.

Host helpers: ``read_ply`` (numpy-only reader for the GT-colour meshes) and
``modified_gt_for_symmetry`` (the pose choice of the symmetry-aware ``_GT_v2`` labels,
generate_training_labels_for_BOP_v2.py:90-208).  Dataset walking and PNG writing are out of scope.
"""
from __future__ import annotations

import numpy as np

_OUTPUTS = ("color", "depth", "mask", "face")
_SHADED_OUTPUTS = ("shaded",) + _OUTPUTS
# the reference's default light, (400, 400, 400) in GL's eye frame (meshrenderer_phong.py:162), in this
# project's camera frame: realCamera's view matrix is diag(1, 1, -1) [R | t], so eye = (Xc, Yc, -Zc)
DEFAULT_LIGHT = (400.0, 400.0, -400.0)


def face_bgr_from_ids(face_ids):
    """Integer ids [nf] -> u8 [nf, 3] in the byte order zp_crop_gt reads (id = B << 16 | G << 8 | R)."""
    ids = np.asarray(face_ids).reshape(-1)
    if ids.size and (not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= 1 << 24):
        raise ValueError("face_ids must be integers in [0, 2^24)")
    ids = ids.astype(np.int64)
    return np.stack([ids >> 16, (ids >> 8) & 255, ids & 255], axis=1).astype(np.uint8)


class MeshRenderer:
    """One mesh resident on the device, rendered at batches of poses.

    vertices [nv, 3] (stored as f32), faces int [nf, 3].  Colours: ``face_colors`` u8 [nf, 3] in the
    output's byte order (B, G, R), or ``colors`` u8 [nv, 3] per vertex as a PLY stores them
    (red, green, blue): a face takes its first vertex's colour (the reference's GT meshes duplicate
    vertices so every face is uniform).  With neither, ``color`` cannot be rendered.  ``render_shaded``
    needs per-vertex ``colors`` and ``normals`` f32 [nv, 3] (``vertex_normals`` makes them for a mesh
    that carries none)."""

    def __init__(self, vertices, faces, colors=None, face_colors=None, device="cuda", normals=None):
        import torch
        v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError("faces must be an integer array [nf, 3]")
        if len(v) == 0 or len(f) == 0:
            raise ValueError("empty mesh")
        if f.min() < 0 or f.max() >= len(v):
            raise ValueError("face index outside the vertex array")
        if colors is not None and face_colors is not None:
            raise ValueError("give colors or face_colors, not both")
        fb = None
        if colors is not None:
            c = np.asarray(colors)
            if c.shape != (len(v), 3) or c.dtype != np.uint8:
                raise ValueError("colors must be u8 [nv, 3] (red, green, blue)")
            fb = c[f[:, 0]][:, ::-1]
        elif face_colors is not None:
            fb = np.asarray(face_colors)
            if fb.shape != (len(f), 3) or fb.dtype != np.uint8:
                raise ValueError("face_colors must be u8 [nf, 3] (blue, green, red)")
        self.device = torch.device(device)
        self.nv, self.nf = len(v), len(f)
        self.vertices = torch.from_numpy(v).to(self.device)
        self.faces = torch.from_numpy(np.ascontiguousarray(f.astype(np.int32))).to(self.device)
        self.face_bgr = None if fb is None else torch.from_numpy(np.ascontiguousarray(fb)).to(self.device)
        self.vert_rgb = None if colors is None else torch.from_numpy(np.ascontiguousarray(c)).to(self.device)
        self.normals = None
        if normals is not None:
            n = np.asarray(normals)
            if n.shape != (len(v), 3):
                raise ValueError("normals must be [nv, 3]")
            self.normals = torch.from_numpy(np.ascontiguousarray(n.astype(np.float32))).to(self.device)
        self._ws = {}  # stream handle -> workspace

    @classmethod
    def from_class_ids(cls, vertices, faces, face_ids, device="cuda"):
        """Colours written from one integer id per face, so that zp_crop_gt's
        RGB_image_to_class_id_image reads the id back."""
        f = np.asarray(faces)
        if len(np.asarray(face_ids).reshape(-1)) != len(f):
            raise ValueError("one id per face is needed")
        return cls(vertices, f, face_colors=face_bgr_from_ids(face_ids), device=device)

    def render(self, R, t, K, height, width, z_near=1e-6, outputs=("color", "mask")):
        """R [B, 3, 3] (or [B, 9]), t [B, 3], K [B, 4] = (fx, fy, cx, cy), or one 3 x 3 camera matrix
        or one such row for all B.  Returns a dict of the requested ``outputs``: color u8
        [B, H, W, 3], depth f32 [B, H, W] (camera Z, 0 = background), mask u8 [B, H, W] (255 / 0),
        face i32 [B, H, W] (-1 = background).  Runs on the current stream of the mesh's device."""
        import torch
        from . import _lib as L
        outputs = tuple(outputs)
        if not outputs or any(o not in _OUTPUTS for o in outputs):
            raise ValueError(f"outputs must be a non-empty subset of {_OUTPUTS}")
        if "color" in outputs and self.face_bgr is None:
            raise ValueError("this mesh has no colours")
        Rn = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(-1, 9))
        B = len(Rn)
        tn = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, 3))
        Kn = np.asarray(K, dtype=np.float64)
        if Kn.shape == (3, 3):
            Kn = np.array([Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]])
        Kn = Kn.reshape(-1, 4)
        if len(Kn) == 1 and B > 1:
            Kn = np.repeat(Kn, B, axis=0)
        Kn = np.ascontiguousarray(Kn)
        if B == 0 or len(tn) != B or len(Kn) != B:
            raise ValueError("R, t and K disagree on the batch size")
        H, W = int(height), int(width)
        need = L.lib.zp_render_ws_bytes(B, self.nv, self.nf, H, W)
        if need < 0:
            raise ValueError(f"render sizes out of range: B {B}, {H} x {W}")
        dev = self.device
        with torch.cuda.device(dev):
            # one workspace per stream, reused by later calls on it (calls on one stream are ordered)
            st = L.stream_ptr(dev)
            ws = self._ws.get(st)
            if ws is None or ws.numel() < need:
                ws = self._ws[st] = torch.empty(need, dtype=torch.uint8, device=dev)
            pose = torch.from_numpy(np.concatenate([Rn.ravel(), tn.ravel(), Kn.ravel()])).to(dev)
            Rd, td, Kd = pose[:9 * B], pose[9 * B:12 * B], pose[12 * B:]
            out = {}
            if "color" in outputs:
                out["color"] = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
            if "depth" in outputs:
                out["depth"] = torch.empty((B, H, W), dtype=torch.float32, device=dev)
            if "mask" in outputs:
                out["mask"] = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
            if "face" in outputs:
                out["face"] = torch.empty((B, H, W), dtype=torch.int32, device=dev)
            L.call("zp_render", B, self.vertices.data_ptr(), self.nv, self.faces.data_ptr(), self.nf,
                   L.ptr(self.face_bgr), Rd.data_ptr(), td.data_ptr(), Kd.data_ptr(), H, W, float(z_near),
                   L.ptr(out.get("color")), L.ptr(out.get("depth")), L.ptr(out.get("mask")), L.ptr(out.get("face")),
                   ws.data_ptr(), st)
        return out

    def render_shaded(self, R, t, K, height, width, light=None, phong=(0.4, 0.8, 0.3), z_near=1e-6,
                      outputs=("shaded", "mask")):
        """``render`` plus ``shaded`` u8 [B, H, W, 3]: the Phong-shaded colour image (B, G, R order,
        background 0) of meshrenderer_phong.py, from the same visibility pass as the other outputs
        (zp_render_shaded, include/zp.h).  light [3] or [B, 3]: the light's position in camera
        coordinates (X right, Y down, Z forward), default the reference's; phong [3] or [B, 3] =
        (ambient, diffuse, specular) weights."""
        import torch
        from . import _lib as L
        outputs = tuple(outputs)
        if not outputs or any(o not in _SHADED_OUTPUTS for o in outputs):
            raise ValueError(f"outputs must be a non-empty subset of {_SHADED_OUTPUTS}")
        if "color" in outputs and self.face_bgr is None:
            raise ValueError("this mesh has no colours")
        if "shaded" in outputs and (self.vert_rgb is None or self.normals is None):
            raise ValueError("shaded needs per-vertex colors and normals")
        Rn = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(-1, 9))
        B = len(Rn)
        tn = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, 3))
        Kn = np.asarray(K, dtype=np.float64)
        if Kn.shape == (3, 3):
            Kn = np.array([Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]])
        Kn = Kn.reshape(-1, 4)
        if len(Kn) == 1 and B > 1:
            Kn = np.repeat(Kn, B, axis=0)
        Kn = np.ascontiguousarray(Kn)
        if B == 0 or len(tn) != B or len(Kn) != B:
            raise ValueError("R, t and K disagree on the batch size")
        ln = np.asarray(DEFAULT_LIGHT if light is None else light, dtype=np.float64).reshape(-1, 3)
        pn = np.asarray(phong, dtype=np.float64).reshape(-1, 3)
        if len(ln) not in (1, B) or len(pn) not in (1, B):
            raise ValueError("light and phong must be one row or one row per render")
        lp = np.ascontiguousarray(np.concatenate([np.broadcast_to(ln, (B, 3)), np.broadcast_to(pn, (B, 3))], axis=1))
        H, W = int(height), int(width)
        need = L.lib.zp_render_shaded_ws_bytes(B, self.nv, self.nf, H, W)
        if need < 0:
            raise ValueError(f"render sizes out of range: B {B}, {H} x {W}")
        dev = self.device
        with torch.cuda.device(dev):
            st = L.stream_ptr(dev)
            ws = self._ws.get(st)
            if ws is None or ws.numel() < need:
                ws = self._ws[st] = torch.empty(need, dtype=torch.uint8, device=dev)
            pose = torch.from_numpy(np.concatenate([Rn.ravel(), tn.ravel(), Kn.ravel(), lp.ravel()])).to(dev)
            Rd, td, Kd, ld = pose[:9 * B], pose[9 * B:12 * B], pose[12 * B:16 * B], pose[16 * B:]
            out = {}
            for name, shape, dt in (("shaded", (B, H, W, 3), torch.uint8), ("color", (B, H, W, 3), torch.uint8),
                                    ("depth", (B, H, W), torch.float32), ("mask", (B, H, W), torch.uint8),
                                    ("face", (B, H, W), torch.int32)):
                if name in outputs:
                    out[name] = torch.empty(shape, dtype=dt, device=dev)
            L.call("zp_render_shaded", B, self.vertices.data_ptr(), L.ptr(self.normals), L.ptr(self.vert_rgb), self.nv,
                   self.faces.data_ptr(), self.nf, L.ptr(self.face_bgr), Rd.data_ptr(), td.data_ptr(), Kd.data_ptr(),
                   ld.data_ptr(), H, W, float(z_near), L.ptr(out.get("shaded")), L.ptr(out.get("color")),
                   L.ptr(out.get("depth")), L.ptr(out.get("mask")), L.ptr(out.get("face")), ws.data_ptr(), st)
        return out


def vertex_normals(vertices, faces):
    """Area-weighted vertex normals f32 [nv, 3] for a mesh that carries none: each face adds its
    cross product (v1 - v0) x (v2 - v0) (twice its area along its normal) to its three vertices; the
    sums are normalised in f64.  A vertex of no face (or of cancelling ones) keeps a zero normal."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0).astype(np.float32)


# ---- PLY ---------------------------------------------------------------------------------------

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path, normals=False):
    """numpy-only reader for a ``models_GT_color/obj_*.ply``: ASCII or binary little-endian; vertex
    x / y / z (f32 or f64), optional u8 red / green / blue, triangular faces as a ``vertex_indices``
    (or ``vertex_index``) list.  Other vertex properties are skipped.  Returns dict(vertices f32
    [nv, 3], faces i32 [nf, 3], colors u8 [nv, 3] or None); with ``normals=True`` also ``normals``
    f32 [nv, 3] from float or double nx / ny / nz, or None when the file has none.  Anything else
    raises ValueError."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    nl = data.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"{path}: truncated PLY header")
    body = data[nl + 1:]
    fmt, elements = None, []
    for line in data[:end].decode("ascii", errors="replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            elements[-1][2].append(tok[1:])
        else:
            raise ValueError(f"{path}: unknown header line {line!r}")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unsupported PLY format {fmt!r} (ascii and binary_little_endian are read)")
    if [e[0] for e in elements[:2]] != ["vertex", "face"] or len(elements) != 2:
        raise ValueError(f"{path}: expected exactly the elements vertex and face, in this order")
    (_, nv, vprops), (_, nf, fprops) = elements
    names = []
    for p in vprops:
        if p[0] == "list" or p[0] not in _PLY_TYPES:
            raise ValueError(f"{path}: unsupported vertex property {' '.join(p)!r}")
        names.append((p[1], _PLY_TYPES[p[0]]))
    vd = dict(names)
    if len(vd) != len(names) or any(k not in vd for k in "xyz") or any(vd[k] not in ("f4", "f8") for k in "xyz"):
        raise ValueError(f"{path}: vertex needs float or double x, y, z")
    rgb = [k in vd for k in ("red", "green", "blue")]
    if any(rgb) and not (all(rgb) and all(vd[k] == "u1" for k in ("red", "green", "blue"))):
        raise ValueError(f"{path}: vertex colours must be uchar red, green, blue")
    if (len(fprops) != 1 or fprops[0][0] != "list" or fprops[0][3] not in ("vertex_indices", "vertex_index")
            or fprops[0][1] not in _PLY_TYPES or _PLY_TYPES.get(fprops[0][2]) not in ("i4", "u4")):
        raise ValueError(f"{path}: face needs one list property vertex_indices of int or uint")
    ct, it = _PLY_TYPES[fprops[0][1]], _PLY_TYPES[fprops[0][2]]
    if fmt == "ascii":
        tok = body.decode("ascii", errors="replace").split()
        nvt = nv * len(names)
        if len(tok) < nvt + 4 * nf:
            raise ValueError(f"{path}: truncated PLY body")
        try:
            vt = np.array(tok[:nvt], dtype=np.float64).reshape(nv, len(names))
            ft = np.array(tok[nvt:nvt + 4 * nf], dtype=np.int64).reshape(nf, 4)
        except ValueError:
            raise ValueError(f"{path}: malformed PLY body") from None
        cols = {n: vt[:, i] for i, (n, ty) in enumerate(names)}
        if nf and (np.any(ft[:, 0] != 3) or len(tok) != nvt + 4 * nf):
            raise ValueError(f"{path}: faces must be triangles")
        faces = ft[:, 1:]
    else:
        vdt = np.dtype([(n, "<" + ty) for n, ty in names])
        fdt = np.dtype([("n", "<" + ct), ("v", "<" + it, (3,))])
        if len(body) < nv * vdt.itemsize:
            raise ValueError(f"{path}: truncated PLY body")
        cols = np.frombuffer(body, dtype=vdt, count=nv)
        rest = body[nv * vdt.itemsize:]
        if len(rest) != nf * fdt.itemsize:
            raise ValueError(f"{path}: faces must be triangles (face data is {len(rest)} bytes, {nf} triangles "
                             f"take {nf * fdt.itemsize})")
        fa = np.frombuffer(rest, dtype=fdt, count=nf)
        if np.any(fa["n"] != 3):
            raise ValueError(f"{path}: faces must be triangles")
        faces = fa["v"]
    vertices = np.stack([np.asarray(cols[k], dtype=np.float64) for k in "xyz"], axis=1).astype(np.float32)
    faces = np.ascontiguousarray(np.asarray(faces, dtype=np.int64))
    if nf and (faces.min() < 0 or faces.max() >= nv):
        raise ValueError(f"{path}: face index outside the vertex list")
    colors = None
    if all(rgb):
        colors = np.stack([np.asarray(cols[k]) for k in ("red", "green", "blue")], axis=1).astype(np.uint8)
    out = {"vertices": vertices, "faces": faces.astype(np.int32), "colors": colors}
    if normals:
        nrm = [k in vd for k in ("nx", "ny", "nz")]
        if any(nrm) and not (all(nrm) and all(vd[k] in ("f4", "f8") for k in ("nx", "ny", "nz"))):
            raise ValueError(f"{path}: vertex normals must be float or double nx, ny, nz")
        out["normals"] = None
        if all(nrm):
            out["normals"] = np.stack([np.asarray(cols[k], dtype=np.float64) for k in ("nx", "ny", "nz")],
                                      axis=1).astype(np.float32)
    return out


# ---- symmetry-aware GT pose ------------------------------------------------------------------

def _axis_rotation(axis, theta):
    """Rotation by theta about coordinate axis 0 / 1 / 2 (right-handed)."""
    c, s = np.cos(theta), np.sin(theta)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    S = np.eye(3)
    S[i, i], S[i, j], S[j, i], S[j, j] = c, -s, s, c
    return S


def _best_axis_rotation(R, axis):
    """The rotation S about a coordinate axis minimising ||R S - I||_F.  ||R S - I||^2 = 6 - 2 tr(R S)
    and, with (i, j) the two other axes in cyclic order, tr(R S) = R_aa + (R_ii + R_jj) cos(theta) +
    (R_ij - R_ji) sin(theta): largest at theta = atan2(R_ij - R_ji, R_ii + R_jj)."""
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    return _axis_rotation(axis, np.arctan2(R[i, j] - R[j, i], R[i, i] + R[j, j]))


def _discrete_symmetries(model_info):
    out = [(np.eye(3), np.zeros(3))]  # the identity is always a member
    for sym in model_info.get("symmetries_discrete", []):
        m = np.asarray(sym, dtype=np.float64).reshape(4, 4)
        out.append((m[:3, :3], m[:3, 3]))
    return out


def modified_gt_for_symmetry(R, t, model_info):
    """The GT pose of the symmetry-aware ``_GT_v2`` labels
    (generate_training_labels_for_BOP_v2.py:90-208): among the poses (R S, R s + t) equivalent under
    the object's symmetries (S, s), the one whose rotation is nearest the identity, min ||R S - I||_F.
    ``model_info`` is the object's entry of BOP's models_info.json.  Supported, as in the reference:
    discrete symmetries; one continuous symmetry about the x, y or z axis with zero offset; a z-axis
    continuous symmetry together with discrete ones (each discrete candidate is first turned about
    z to its own optimum).  Returns (R [3, 3], t of the input's shape), f64."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t_in = np.asarray(t, dtype=np.float64)
    tv = t_in.reshape(3)
    cont = model_info.get("symmetries_continuous")
    disc = model_info.get("symmetries_discrete")
    if cont is None and disc is None:
        return R, t_in
    axis = None
    if cont is not None:
        if len(cont) != 1:
            raise NotImplementedError("exactly one continuous symmetry is supported")
        ax = [float(a) for a in cont[0]["axis"]]
        if any(float(o) != 0 for o in cont[0].get("offset", [0, 0, 0])):
            raise NotImplementedError("a continuous symmetry with an offset is not supported")
        if ax not in ([1, 0, 0], [0, 1, 0], [0, 0, 1]):
            raise NotImplementedError(f"continuous symmetry about axis {ax}: only x, y and z are supported")
        axis = ax.index(1)
        if disc is not None and axis != 2:
            raise NotImplementedError("discrete symmetries combine only with a z-axis continuous symmetry")
    best = None
    for S, s in _discrete_symmetries(model_info) if disc is not None else [(np.eye(3), np.zeros(3))]:
        Rc, tc = R @ S, R @ s + tv
        if axis is not None:  # a rotation about an axis through the origin leaves the translation alone
            Rc = Rc @ _best_axis_rotation(Rc, axis)
        n = np.linalg.norm(Rc - np.eye(3))
        if best is None or n < best[0]:
            best = (n, Rc, tc)
    return best[1], best[2].reshape(t_in.shape)
