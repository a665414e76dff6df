#!/usr/bin/env python
"""Times the mesh upsampling (zp_mesh_subdivide) on the way the label recipe takes it: a level-4
icosphere (2562 vertices, 5120 faces, scaled to 90 x 60 x 40 mm semi-axes) brought to 65537 vertices,
the size ``encode_mesh(bits=16, upsample=True)`` asks for.  Legs, alternated over ``--rounds`` rounds of
``--iters`` calls after a warm-up:
  upsample  upsample_mesh end to end (upload, every pass with its read-back of the counts, download);
            the host waits for each pass's sizes, so both the device events around the calls and the wall
            clock around the synchronised window are reported
  pass      the last pass alone (the zp_mesh_subdivide call with the budget that lands on the target),
            mesh and workspace resident on the device; device events
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ZP_QUIET", "1")

from tools.render_bench import icosphere  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--min-vertices", type=int, default=65537)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subdiv_bench: no GPU (timings are taken on the device only)")
    from zebrapose_amd import _lib as L
    from zebrapose_amd import meshcode as MC

    v, f = icosphere(a.level)
    v = np.ascontiguousarray(v * np.array([90.0, 60.0, 40.0], np.float32))
    f = np.ascontiguousarray(f.astype(np.int32))
    m = MC.upsample_mesh(v, f, min_vertices=a.min_vertices)
    sizes = [len(v)] + m.pass_sizes
    # the mesh in front of the last pass: the same passes, one fewer
    before = MC.upsample_mesh(v, f, min_vertices=sizes[-2]) if len(sizes) > 2 else None
    bv, bf = (before.vertices, before.faces) if before is not None else (v, f)
    assert len(bv) == sizes[-2]
    nv, nf, budget = len(bv), len(bf), a.min_vertices - len(bv)
    vd, fd = torch.from_numpy(bv).cuda(), torch.from_numpy(bf).cuda()
    cap_v, cap_f = nv + budget, 4 * nf
    ov = torch.empty((cap_v, 3), dtype=torch.float32, device="cuda")
    of = torch.empty((cap_f, 3), dtype=torch.int32, device="cuda")
    par = torch.empty((cap_v, 2), dtype=torch.int32, device="cuda")
    counts = torch.empty(4, dtype=torch.int64, device="cuda")
    mx = torch.empty(1, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.lib.zp_mesh_subdivide_ws_bytes(nv, nf), dtype=torch.uint8, device="cuda")

    def one_pass():
        L.call("zp_mesh_subdivide", vd.data_ptr(), nv, fd.data_ptr(), nf, 0.0, 0.25, budget, ov.data_ptr(), cap_v,
               of.data_ptr(), cap_f, par.data_ptr(), counts.data_ptr(), mx.data_ptr(), ws.data_ptr(), L.stream_ptr())

    def upsample():
        MC.upsample_mesh(v, f, min_vertices=a.min_vertices)

    legs = {"upsample": upsample, "pass": one_pass}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    assert c[2] == a.min_vertices and np.array_equal(ov.cpu().numpy(), m.vertices)
    ms = {name: [] for name in legs}
    wall_ms = []
    for _ in range(a.rounds):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)
            if name == "upsample":
                wall_ms.append(1e3 * (time.perf_counter() - t0) / a.iters)
    res = {"nv_in": len(v), "nf_in": len(f), "nv_out": len(m.vertices), "nf_out": len(m.faces),
           "passes": len(m.pass_sizes), "pass_sizes": m.pass_sizes, "last_pass": {"nv": nv, "nf": nf, "budget": budget,
                                                                                  "unique_edges": int(c[0])},
           "iters": a.iters, "rounds": a.rounds, "runs": a.iters * a.rounds, "ws_MB": round(ws.numel() / 2 ** 20, 1)}
    for name in legs:
        res[name + "_ms"] = round(float(np.median(ms[name])), 3)
        res[name + "_ms_min_max"] = [round(float(min(ms[name])), 3), round(float(max(ms[name])), 3)]
    res["upsample_wall_ms"] = round(float(np.median(wall_ms)), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
