"""Surface codes of a raw mesh on the device (``zp_mesh_code``, csrc/zp_meshcode.hip; ``zp_mesh_code_radix``,
csrc/zp_meshcode_radix.hip).

The reference codes a mesh offline with the C++ tool
Binary_Code_GT_Generator/Generate_Mesh_with_GT_Color (PCL + OpenCV): a recursive balanced 2-means
split of the vertices, ``bits`` levels deep, gives every vertex a class id; faces take an id from
their vertices, and the class -> 3D-point LUT is the mean of each class's face vertices.  Its
outputs are the GT-colour mesh ``models_GT_color/obj_*.ply`` that ``MeshRenderer`` draws and the
LUT ``Class_CorresPoint*.txt`` that ``Decoder`` reads.  ``encode_mesh`` produces both from a raw
mesh on the device.  OpenCV's k-means++ draws cannot be reproduced, so the split is restated in
exact integer arithmetic: the semantics are in include/zp.h (zp_mesh_code) and, as numpy, in
tests/meshcode_ref.py; results are bit-for-bit reproducible for a given seed.  ``encode_mesh`` splits
in two (the reference's ``divide_number`` 2); ``encode_mesh_radix`` codes a mesh for the d-ary network
of the code-radix ablation (``divide_number_each_itration`` 4 / 16 / 256) with a balanced d-way split
per level (zp_mesh_code_radix in include/zp.h, tests/meshcode_radix_ref.py).  Dataset walking and OBJ
input are out of scope.

The generator's recipe (Binary_Code_GT_Generator/Generate_GT.md, step 1) first upsamples a model past
2^16 vertices with Meshlab's midpoint-subdivision filter, by hand.  ``upsample_mesh`` /
``subdivide_midpoint`` do that on the device (``zp_mesh_subdivide``, csrc/zp_subdiv.hip; semantics in
include/zp.h and, as numpy, in tests/subdiv_ref.py), and ``encode_mesh(..., upsample=True)`` calls it.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from .render import MeshRenderer, face_bgr_from_ids

_SAT = (1 << 19) - 1


def grid_log2(vertices):
    """The largest k in [-40, 40] for which rint(|v| * 2^k) stays within 2^19 - 1 for every coordinate."""
    m = float(np.abs(np.asarray(vertices, dtype=np.float32).astype(np.float64)).max())
    for k in range(40, -41, -1):
        if np.rint(np.ldexp(m, k)) <= _SAT:
            return k
    raise ValueError(f"mesh extent {m:g} is too large for the coder's grid")


def eps_to_grid(eps, k):
    """floor((eps * 2^k)^2) in exact arithmetic, capped at 2^62 (no centre shift^2 reaches 2^42)."""
    eps = float(eps)
    if not np.isfinite(eps) or eps < 0:
        raise ValueError("eps must be finite and >= 0")
    return min(int((Fraction(eps) * Fraction(2) ** k) ** 2), 1 << 62)


class MeshCode:
    """Result of ``encode_mesh``: ``vertex_ids`` i32 [nv], ``face_ids`` i32 [nf] and ``lut`` f64
    [2^bits, 3] (NaN rows: classes without a face) as device tensors, ``bits``, the mesh
    (``vertices`` f32 [nv, 3], ``faces`` i32 [nf, 3], numpy) and the ``draws`` u32
    [attempts, 2^bits - 1] that seeded the split.  ``divide`` is 2 and ``levels`` is ``bits``.
    From ``encode_mesh_radix``: ``divide`` = d, ``levels`` = L, ids are the L base-d digits folded MSB
    first, ``lut`` is [d^L, 3], ``bits`` = L log2 d and ``draws`` is [attempts, (d^L - 1) / (d - 1)]."""

    def __init__(self, vertices, faces, bits, vertex_ids, face_ids, lut, draws, divide=2, levels=None):
        self.vertices, self.faces, self.bits = vertices, faces, bits
        self.vertex_ids, self.face_ids, self.lut, self.draws = vertex_ids, face_ids, lut, draws
        self.divide, self.levels = int(divide), int(bits if levels is None else levels)

    def renderer(self, device=None):
        """A ``MeshRenderer`` whose colours carry the face ids (what the label generator draws)."""
        return MeshRenderer.from_class_ids(self.vertices, self.faces, self.face_ids.cpu().numpy(),
                                           device=self.face_ids.device if device is None else device)

    def decoder(self, ignore_bit=0, device=None):
        """The ``Decoder`` of this code's LUT (``class_base=divide`` for a d-ary code, which has no
        ``ignore_bit``)."""
        from .decode import Decoder
        if self.divide != 2:
            if ignore_bit:
                raise ValueError("ignore_bit needs a binary code (encode_mesh)")
            return Decoder([self.lut.cpu().numpy()], device=self.lut.device if device is None else device,
                           class_base=self.divide)
        return Decoder([self.lut.cpu().numpy()], device=self.lut.device if device is None else device,
                       ignore_bit=ignore_bit)

    def model_info(self, **sym):
        """This mesh's entry of models_info.json (``modelinfo.model_info`` of the vertices, on the
        code's device); ``symmetries_discrete`` / ``symmetries_continuous`` are passed through."""
        from .modelinfo import model_info
        return model_info(self.vertices, device=self.face_ids.device, **sym)

    def write_lut_file(self, path):
        """The generator's ``Class_CorresPoint*.txt`` (Generate_Mesh_with_GT_Color.cpp:616-624):
        ``"N d L"`` (d = 2 and L = bits for the binary code), then ``"id x y z"`` per class with ``%g``
        numbers as the C++ stream prints them; a class without a face is written as ``nan``."""
        lut = self.lut.cpu().numpy()
        with open(path, "w") as f:
            f.write(f"{len(lut)} {self.divide} {self.levels}\n")
            for i, (x, y, z) in enumerate(lut):
                f.write("%d %s %s %s\n" % (i, *("nan" if v != v else "%g" % v for v in (x, y, z))))

    def write_ply(self, path):
        """The GT-colour mesh as create_mesh_with_labeled_color builds it
        (Generate_Mesh_with_GT_Color.cpp:471-538), binary little-endian: walking the faces in order, a
        vertex's first use keeps its index and every later use appends a duplicate, so that all three
        vertices of a face carry the face's colour R = id & 255, G = (id >> 8) & 255, B = id >> 16.
        A vertex no face uses keeps its position (the reference leaves it at the origin), black."""
        v, faces = self.vertices, self.faces
        fid = self.face_ids.cpu().numpy().astype(np.int64)
        flat = faces.reshape(-1).astype(np.int64)
        first = np.zeros(len(flat), bool)
        first[np.unique(flat, return_index=True)[1]] = True
        new_index = np.where(first, flat, len(v) + np.cumsum(~first) - 1)
        rgb = face_bgr_from_ids(fid)[:, ::-1]
        out = np.zeros(len(v) + int((~first).sum()), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"),
                                                            ("green", "u1"), ("blue", "u1")])
        for a, name in enumerate("xyz"):
            out[name][:len(v)] = v[:, a]
            out[name][new_index] = v[flat, a]
        for a, name in enumerate(("red", "green", "blue")):
            out[name][new_index] = np.repeat(rgb[:, a], 3)
        fo = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        fo["n"] = 3
        fo["v"] = new_index.reshape(-1, 3)
        head = ("ply\nformat binary_little_endian 1.0\n"
                f"element vertex {len(out)}\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                f"element face {len(fo)}\nproperty list uchar int vertex_indices\nend_header\n")
        with open(path, "wb") as f:
            f.write(head.encode("ascii"))
            f.write(out.tobytes())
            f.write(fo.tobytes())


def _check_mesh(vertices, faces, classes, what):
    """The input checks both coders share -> (vertices f32 [nv, 3], faces i32 [nf, 3]), contiguous."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer) or len(f) == 0:
        raise ValueError("faces must be a non-empty integer array [nf, 3]")
    if len(v) < classes:
        raise ValueError(f"{len(v)} vertices cannot fill {what} classes")
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex")
    if f.min() < 0 or f.max() >= len(v):
        raise ValueError("face index outside the vertex array")
    return v, np.ascontiguousarray(f.astype(np.int32))


_MAX_NV, _MAX_NF, _NO_BUDGET = 1 << 21, 1 << 24, (1 << 31) - 1


class UpsampledMesh:
    """Result of ``subdivide_midpoint`` / ``upsample_mesh``: ``vertices`` f32 [nv, 3] and ``faces`` i32
    [nf, 3] (numpy, the form ``encode_mesh`` and ``MeshRenderer`` take), ``parents`` i32 [nv, 2] (an
    input vertex: its own index twice; a new one: the two ends of the edge it halves, indices of this
    mesh), ``n_input`` (the input's vertex count) and ``pass_sizes`` (the vertex count after each pass)."""

    def __init__(self, vertices, faces, parents, n_input, pass_sizes):
        self.vertices, self.faces, self.parents = vertices, faces, parents
        self.n_input, self.pass_sizes = int(n_input), [int(n) for n in pass_sizes]

    def lift(self, attr):
        """Carry a per-vertex attribute of the input mesh (colours, normals; [n_input, ...]) to this
        mesh: a new vertex gets the average of its parents', pass by pass, in f64 -> f64 [nv, ...]."""
        a = np.asarray(attr, dtype=np.float64)
        if len(a) != self.n_input:
            raise ValueError(f"attribute has {len(a)} rows, the input mesh had {self.n_input} vertices")
        prev = self.n_input
        for n in self.pass_sizes:
            p = self.parents[prev:n]
            a = np.concatenate([a, (a[p[:, 0]] + a[p[:, 1]]) * 0.5])
            prev = n
        return a


class _Subdivider:
    """The mesh on the device between passes of zp_mesh_subdivide; only ``counts`` comes back per pass."""

    def __init__(self, vertices, faces, device):
        import torch
        v, f = _check_mesh(vertices, faces, 1, "1")
        if len(v) > _MAX_NV or len(f) > _MAX_NF:
            raise ValueError(f"mesh sizes out of range: {len(v)} vertices, {len(f)} faces")
        self.dev = torch.device(device)
        self.host = (v, f)
        self.n_input, self.pass_sizes = len(v), []
        with torch.cuda.device(self.dev):
            self.v, self.f = torch.from_numpy(v).to(self.dev), torch.from_numpy(f).to(self.dev)
            self.parents = torch.arange(len(v), dtype=torch.int32, device=self.dev).repeat_interleave(2).view(-1, 2)

    def run(self, abs2, rel2, max_split):
        """One pass -> the number of edges it split."""
        import torch
        from . import _lib as L
        nv, nf = len(self.v), len(self.f)
        # every split edge adds one vertex, every split edge slot one face
        cap_v, cap_f = nv + min(int(max_split), 3 * nf), 4 * nf
        with torch.cuda.device(self.dev):
            ov = torch.empty((cap_v, 3), dtype=torch.float32, device=self.dev)
            of = torch.empty((cap_f, 3), dtype=torch.int32, device=self.dev)
            par = torch.empty((cap_v, 2), dtype=torch.int32, device=self.dev)
            counts = torch.empty(4, dtype=torch.int64, device=self.dev)
            mx = torch.empty(1, dtype=torch.float64, device=self.dev)
            ws = torch.empty(L.lib.zp_mesh_subdivide_ws_bytes(nv, nf), dtype=torch.uint8, device=self.dev)
            L.call("zp_mesh_subdivide", self.v.data_ptr(), nv, self.f.data_ptr(), nf, float(abs2), float(rel2),
                   int(max_split), ov.data_ptr(), cap_v, of.data_ptr(), cap_f, par.data_ptr(), counts.data_ptr(),
                   mx.data_ptr(), ws.data_ptr(), L.stream_ptr(self.dev))
            _, n_split, nv_out, nf_out = (int(c) for c in counts.cpu())
            if nv_out > _MAX_NV or nf_out > _MAX_NF:
                raise ValueError(f"the upsampled mesh is out of range: {nv_out} vertices, {nf_out} faces "
                                 "(at most 2^21 vertices and 2^24 faces)")
            par[:nv] = self.parents
            self.v, self.f, self.parents = ov[:nv_out].clone(), of[:nf_out].clone(), par[:nv_out].clone()
        self.pass_sizes.append(nv_out)
        return n_split

    def result(self):
        if not self.pass_sizes:
            v, f = self.host
            return UpsampledMesh(v, f, self.parents.cpu().numpy(), self.n_input, [])
        return UpsampledMesh(self.v.cpu().numpy(), self.f.cpu().numpy(), self.parents.cpu().numpy(), self.n_input,
                             self.pass_sizes)


def subdivide_midpoint(vertices, faces, iterations=1, threshold=0.0, device="cuda"):
    """Meshlab's 'subdivision surface: mid point' filter with its two parameters, on the device
    (zp_mesh_subdivide in include/zp.h; tests/subdiv_ref.py restates it): ``iterations`` passes, each
    halving every edge longer than ``threshold`` mesh units.  Returns an ``UpsampledMesh``."""
    iterations, threshold = int(iterations), float(threshold)
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    if not np.isfinite(threshold) or threshold < 0:
        raise ValueError("threshold must be finite and >= 0")
    s = _Subdivider(vertices, faces, device)
    for _ in range(iterations):
        s.run(threshold * threshold, 0.0, _NO_BUDGET)
    return s.result()


def upsample_mesh(vertices, faces, min_vertices=65537, max_passes=64, device="cuda"):
    """Upsample a mesh to exactly ``min_vertices`` vertices (step 1 of the reference's label recipe,
    Generate_GT.md: "until it has more than 2^16 vertices"): passes of zp_mesh_subdivide that halve the
    edges longer than half the longest one (rel2 = 0.25, so the long edges of a CAD mesh go first), the
    longest first and only as many as are still missing.  A mesh that is large enough already comes back
    unchanged, with no pass.  Raises if a pass splits nothing (every edge has length 0), after
    ``max_passes`` passes, or past the coder's 2^21 vertices / 2^24 faces.  Returns an ``UpsampledMesh``."""
    min_vertices, max_passes = int(min_vertices), int(max_passes)
    if min_vertices > _MAX_NV:
        raise ValueError(f"min_vertices {min_vertices} is beyond the coder's 2^21 vertices")
    s = _Subdivider(vertices, faces, device)
    nv = s.n_input
    while nv < min_vertices:
        if len(s.pass_sizes) >= max_passes:
            raise ValueError(f"{nv} of {min_vertices} vertices after max_passes = {max_passes} passes")
        if s.run(0.0, 0.25, min_vertices - nv) == 0:
            raise ValueError("a pass split no edge: every edge of the mesh has length 0")
        nv = s.pass_sizes[-1]
    return s.result()


def _upsampled(vertices, faces, classes, device):
    m = upsample_mesh(vertices, faces, min_vertices=classes + 1, device=device)
    return m.vertices, m.faces


def _encode(vertices, faces, classes, what, size_what, draws_per_attempt, c_name, split_args, bits, attempts,
            iterations, eps, seed, device, upsample, **code_kw):
    """What both coders do with checked parameters: ``classes`` classes (``what`` in messages), a
    [attempts, draws_per_attempt] table of draws, and the C entry ``c_name`` / ``c_name``_ws_bytes, which
    takes ``split_args`` after the mesh sizes.  ``bits`` and ``code_kw`` go to the ``MeshCode``."""
    import torch
    from . import _lib as L
    if upsample:
        vertices, faces = _upsampled(vertices, faces, classes, device)
    v, f = _check_mesh(vertices, faces, classes, what)
    k = grid_log2(v)
    eps2 = eps_to_grid(eps, k)
    draws = np.random.default_rng(seed).integers(0, 1 << 32, size=(attempts, draws_per_attempt), dtype=np.uint32)
    need = getattr(L.lib, c_name + "_ws_bytes")(len(v), len(f), *split_args)
    if need < 0:
        raise ValueError(f"mesh sizes out of range: {len(v)} vertices, {len(f)} faces, {size_what}")
    dev = torch.device(device)
    with torch.cuda.device(dev):
        vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        dd = torch.from_numpy(draws.view(np.int32)).to(dev)
        vid = torch.empty(len(v), dtype=torch.int32, device=dev)
        fid = torch.empty(len(f), dtype=torch.int32, device=dev)
        lut = torch.empty((classes, 3), dtype=torch.float64, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        L.call(c_name, vd.data_ptr(), len(v), fd.data_ptr(), len(f), *split_args, attempts, iterations, k, eps2,
               dd.data_ptr(), vid.data_ptr(), fid.data_ptr(), lut.data_ptr(), ws.data_ptr(), L.stream_ptr(dev))
        # the inputs and the workspace were allocated on this stream: frees are ordered behind the call
    return MeshCode(v, f, bits, vid, fid, lut, draws, **code_kw)


def encode_mesh_radix(vertices, faces, divide, levels, attempts=3, iterations=10, eps=1.0, seed=0, device="cuda",
                      upsample=False):
    """Code a triangle mesh for the d-ary network: ``levels`` levels of the balanced ``divide``-way
    split (d a power of two in 4..256, d^levels <= 65536; zp_mesh_code_radix in include/zp.h), with
    ``attempts`` tries of up to ``iterations`` Lloyd steps per group as in ``encode_mesh``.  vertices
    [nv, 3] (stored as f32, finite, d^levels <= nv <= 2^21), faces int [nf, 3].  The seeds are sampled on
    the host from ``numpy.random.default_rng(seed)``.  ``upsample`` as in ``encode_mesh``.  Returns a
    ``MeshCode`` whose ids fold the digits as ``Decoder(class_base=divide)`` and the GT digit planes do."""
    d, levels, attempts, iterations = int(divide), int(levels), int(attempts), int(iterations)
    if d == 2:
        raise ValueError("divide 2 is the binary code: use encode_mesh")
    if d < 4 or d > 256 or d & (d - 1):
        raise ValueError("divide must be a power of two in 4..256")
    if levels < 1 or d ** levels > 65536:
        raise ValueError("levels must be >= 1 with divide^levels <= 65536")
    if attempts < 1 or iterations < 1:
        raise ValueError("attempts and iterations must be >= 1")
    C = d ** levels
    return _encode(vertices, faces, C, f"{d}^{levels}", f"{d}^{levels} classes", (C - 1) // (d - 1),
                   "zp_mesh_code_radix", (d, levels), (d.bit_length() - 1) * levels, attempts, iterations, eps, seed,
                   device, upsample, divide=d, levels=levels)


def encode_mesh(vertices, faces, bits=16, attempts=3, iterations=10, eps=1.0, seed=0, device="cuda", upsample=False):
    """Code a triangle mesh: ``bits`` levels (1..16) of the balanced 2-means split, ``attempts`` tries
    of up to ``iterations`` Lloyd steps per group stopping at a centre shift of ``eps`` mesh units
    (the reference's cv::kmeans(..., TermCriteria(10, 1.0), 3, ...)).  vertices [nv, 3] (stored as
    f32, finite, 2^bits <= nv <= 2^21), faces int [nf, 3].  The seeds are sampled on the host from
    ``numpy.random.default_rng(seed)``; the split runs on the current stream of ``device``.
    ``upsample=True`` first brings a smaller mesh to 2^bits + 1 vertices with ``upsample_mesh`` (the
    reference's recipe asks for more vertices than classes); the result's ``vertices`` / ``faces`` are
    then the upsampled ones.  Returns a ``MeshCode``."""
    bits, attempts, iterations = int(bits), int(attempts), int(iterations)
    if not 1 <= bits <= 16:
        raise ValueError("bits must be in 1..16")
    if attempts < 1 or iterations < 1:
        raise ValueError("attempts and iterations must be >= 1")
    return _encode(vertices, faces, 1 << bits, f"2^{bits}", f"{bits} bits", (1 << bits) - 1, "zp_mesh_code", (bits,),
                   bits, attempts, iterations, eps, seed, device, upsample)
