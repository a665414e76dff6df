#!/usr/bin/env python
"""Times the GT renderer (zp_render) at the size the label generator runs it.

B = 32 renders at 640 x 480 of an icosphere subdivided 7 times (163,842 vertices, 327,680 faces; a
models_GT_color mesh has 2^16 or more vertices), radius 60 mm at 600-1000 mm in front of an LM-like
camera (fx = fy = 572.4), each render with its own rotation and offset.  Legs, alternated over
``--rounds`` rounds of ``--iters`` calls after a warm-up, device events around each round:
  launch   the zp_render call alone, poses resident on the device (the five passes)
  render   MeshRenderer.render (pose upload + output allocation + the same call)
The rate is taken against the bytes the five passes must move: the mesh (vertices + faces) once per
render, the key plane cleared, updated and read (3 x 8 B per pixel), and the outputs written.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ZP_QUIET", "1")

OUT_BYTES = {"color": 3, "depth": 4, "mask": 1, "face": 4}


def icosphere(level):
    """Unit icosphere, vectorised midpoint subdivision: (verts f32 [10 * 4^level + 2, 3], faces i32 [20 * 4^level, 3])."""
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
        m = len(v) + inv.reshape(3, -1)  # midpoints of edges ab, bc, ca
        v = np.concatenate([v, mid])
        a, b, c = f.T
        f = np.concatenate([np.stack(t, 1) for t in ((a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2]))])
    return v.astype(np.float32), f.astype(np.int32)


def random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--outputs", default="color,mask")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench: no GPU (timings are taken on the device only)")
    from zebrapose_amd import _lib as L
    from zebrapose_amd.render import MeshRenderer

    B, H, W = a.batch, 480, 640
    outputs = tuple(a.outputs.split(","))
    v, f = icosphere(a.level)
    v *= 60.0
    rng = np.random.default_rng(a.seed)
    mr = MeshRenderer.from_class_ids(v, f, rng.integers(1, 1 << 16, len(f)))
    R = random_rotations(rng, B)
    t = np.stack([rng.uniform(-150, 150, B), rng.uniform(-100, 100, B), rng.uniform(600, 1000, B)], 1)
    K = np.tile(np.array([[572.4114, 573.57043, 325.2611, 242.04899]]), (B, 1))

    ws = torch.empty(L.lib.zp_render_ws_bytes(B, mr.nv, mr.nf, H, W), dtype=torch.uint8, device="cuda")
    Rd, td, Kd = (torch.from_numpy(x).cuda() for x in (R, t, K))
    bufs = {"color": torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda"),
            "depth": torch.empty((B, H, W), dtype=torch.float32, device="cuda"),
            "mask": torch.empty((B, H, W), dtype=torch.uint8, device="cuda"),
            "face": torch.empty((B, H, W), dtype=torch.int32, device="cuda")}
    op = [bufs[k].data_ptr() if k in outputs else None for k in ("color", "depth", "mask", "face")]

    def launch():
        L.call("zp_render", B, mr.vertices.data_ptr(), mr.nv, mr.faces.data_ptr(), mr.nf, mr.face_bgr.data_ptr(),
               Rd.data_ptr(), td.data_ptr(), Kd.data_ptr(), H, W, 1.0, *op, ws.data_ptr(), L.stream_ptr())

    legs = {"launch": launch, "render": lambda: mr.render(R, t, K, H, W, z_near=1.0, outputs=outputs)}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    cover = float((bufs["mask"] != 0).float().mean()) if "mask" in outputs else None
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.iters)
    nbytes = B * (mr.nv * 12 + mr.nf * 12) + 3 * 8 * B * H * W + sum(OUT_BYTES[k] for k in outputs) * B * H * W
    res = {"batch": B, "H": H, "W": W, "nv": mr.nv, "nf": mr.nf, "outputs": list(outputs), "iters": a.iters,
           "rounds": a.rounds, "runs": a.iters * a.rounds, "foreground_share": cover, "bytes": int(nbytes)}
    for k in legs:
        res[k + "_ms"] = round(float(np.median(ms[k])), 4)
        res[k + "_ms_min_max"] = [round(float(min(ms[k])), 4), round(float(max(ms[k])), 4)]
    res["launch_GBps"] = round(nbytes / (res["launch_ms"] * 1e-3) / 1e9, 1)
    res["ms_per_render"] = round(res["launch_ms"] / B, 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
