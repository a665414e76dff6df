#!/usr/bin/env python
"""Times the mesh coder (zp_mesh_code) at the size the reference's generator runs it.

A synthetic ellipsoid of 2^18 vertices (an icosphere subdivided 7 times, scaled to 90 x 60 x 40 mm
semi-axes, padded to 2^18 with jittered copies of its own vertices) is coded at L = 16 with the
reference's k-means parameters (3 attempts, 10 iterations, eps 1.0).  Legs, alternated over
``--rounds`` rounds of ``--iters`` calls after a warm-up, device events around each round:
  launch   the zp_mesh_code call alone, mesh and draws resident on the device
  encode   encode_mesh (host checks, draw sampling, upload, allocation + the same call)
With ``--divide d --levels L`` the d-ary coder is timed instead (zp_mesh_code_radix /
encode_mesh_radix), ``--nv`` cutting the ellipsoid to any vertex count.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ZP_QUIET", "1")

from tools.render_bench import icosphere  # noqa: E402


def ellipsoid(nv, seed):
    v, f = icosphere(7)
    v = v * np.array([90.0, 60.0, 40.0], np.float32)
    rng = np.random.default_rng(seed)
    if nv > len(v):
        pick = rng.integers(0, len(v), nv - len(v))
        v = np.concatenate([v, v[pick] * (1 + rng.uniform(-0.02, 0.02, (len(pick), 1))).astype(np.float32)])
    return np.ascontiguousarray(v[:nv], np.float32), f[(f < nv).all(1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-nv", type=int, default=18)
    ap.add_argument("--nv", type=int, default=0, help="vertex count (default 2^log2-nv)")
    ap.add_argument("--bits", type=int, default=16)
    ap.add_argument("--divide", type=int, default=2, help="d > 2: time the d-ary coder with --levels levels")
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshcode_bench: no GPU (timings are taken on the device only)")
    from zebrapose_amd import _lib as L
    from zebrapose_amd import meshcode as MC

    v, f = ellipsoid(a.nv or 1 << a.log2_nv, a.seed)
    d, levels = a.divide, a.levels
    bits = a.bits if d == 2 else (d.bit_length() - 1) * levels
    nv, nf, attempts, iterations = len(v), len(f), 3, 10
    k = MC.grid_log2(v)
    eps2 = MC.eps_to_grid(1.0, k)
    n_draws = (1 << bits) - 1 if d == 2 else ((1 << bits) - 1) // (d - 1)
    draws = np.random.default_rng(a.seed).integers(0, 1 << 32, size=(attempts, n_draws), dtype=np.uint32)
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    dd = torch.from_numpy(draws.view(np.int32)).cuda()
    vid = torch.empty(nv, dtype=torch.int32, device="cuda")
    fid = torch.empty(nf, dtype=torch.int32, device="cuda")
    lut = torch.empty((1 << bits, 3), dtype=torch.float64, device="cuda")
    need = L.lib.zp_mesh_code_ws_bytes(nv, nf, bits) if d == 2 else L.lib.zp_mesh_code_radix_ws_bytes(nv, nf, d, levels)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def launch():
        if d == 2:
            L.call("zp_mesh_code", vd.data_ptr(), nv, fd.data_ptr(), nf, bits, attempts, iterations, k, eps2,
                   dd.data_ptr(), vid.data_ptr(), fid.data_ptr(), lut.data_ptr(), ws.data_ptr(), L.stream_ptr())
        else:
            L.call("zp_mesh_code_radix", vd.data_ptr(), nv, fd.data_ptr(), nf, d, levels, attempts, iterations, k, eps2,
                   dd.data_ptr(), vid.data_ptr(), fid.data_ptr(), lut.data_ptr(), ws.data_ptr(), L.stream_ptr())

    if d == 2:
        legs = {"launch": launch, "encode": lambda: MC.encode_mesh(v, f, bits=bits, seed=a.seed)}
    else:
        legs = {"launch": launch, "encode": lambda: MC.encode_mesh_radix(v, f, d, levels, seed=a.seed)}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    leaf = torch.bincount(vid.long(), minlength=1 << bits)
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)
    if d == 2:
        launches, sorts = bits * (attempts * (5 + 2 * iterations) + 4), 2 * bits
    else:  # per level: attempts x (d - 1 seeds, seeded, Lloyd, comp, best), d - 1 x (score, take), bounds
        launches = levels * (attempts * (d + 2 + 2 * iterations) + 2 * (d - 1) + 1) + 3
        sorts = levels * d
    res = {"nv": nv, "nf": nf, "bits": bits, "divide": d, "levels": bits if d == 2 else levels, "attempts": attempts,
           "iterations": iterations, "grid_log2": k, "iters": a.iters, "rounds": a.rounds, "runs": a.iters * a.rounds,
           "leaf_min_max": [int(leaf.min()), int(leaf.max())], "lut_nan_rows": int(torch.isnan(lut).any(1).sum()),
           "kernel_launches": launches, "sorts": sorts, "ws_MB": round(ws.numel() / 2 ** 20, 1)}
    for name in legs:
        res[name + "_ms"] = round(float(np.median(ms[name])), 3)
        res[name + "_ms_min_max"] = [round(float(min(ms[name])), 3), round(float(max(ms[name])), 3)]
    res["us_per_launch"] = round(1e3 * res["launch_ms"] / res["kernel_launches"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
