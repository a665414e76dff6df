"""Time the ICP refinement once at the workload's size (device events, inputs resident).

    python tools/icp_bench.py [--reps 20] [--level 5]

B = 1 and B = 32 poses at 640 x 480 of an LM-O-sized mesh (an ellipsoidal icosphere, level 5: 10 242
vertices, 20 480 faces, 100 x 70 x 50 mm half-axes at 800 mm), N = 3000, tolerance 5e-7, at most 200
iterations.  The measured depth is the true pose's render in front of a plane at 2 m; the starts are off
by a few degrees and millimetres, so every pose converges.  Prints one JSON line per batch size: median
and min milliseconds of the whole refine_batch (render, two back-projections, the ICP launch) and of the
ICP launch alone, the iteration counts, and beside them the wall time of the same loop on this
machine's CPU for the same clouds and draws with scipy's cKDTree as the neighbour search (one pose
after the other, as the reference runs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zebrapose_amd import _lib as L  # noqa: E402
from zebrapose_amd.icp import ANGLE_LIMIT, MIN_FRACTION, ICPRefiner  # noqa: E402
from zebrapose_amd.render import MeshRenderer  # noqa: E402
from tests import icp_ref as IR  # noqa: E402
from tools.bop_bench import timed  # noqa: E402
from tools.refine_bench import rot  # noqa: E402
from tools.render_bench import icosphere  # noqa: E402


def cpu_icp(A, B, max_iterations, tolerance):
    """tests/icp_ref.py::icp with a k-d tree for the brute-force search"""
    from scipy.spatial import cKDTree
    tree = cKDTree(B)
    src, prev = A.copy(), 0.0
    for it in range(max_iterations):
        dist, idx = tree.query(src)
        _, R, t, _, _ = IR.best_fit_transform(src, B[idx])
        src = src @ R.T + t
        mean = dist.mean()
        if abs(prev - mean) < tolerance:
            break
        prev = mean
    return IR.best_fit_transform(A, src)[0], it + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--level", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    H, W, N = 480, 640, 3000
    v, f = icosphere(args.level)
    v = (v * np.array([100.0, 70.0, 50.0])).astype(np.float32)
    rend = MeshRenderer(v, f, device=dev)
    K = np.array([572.4114, 573.57043, 325.2611, 242.04899])
    Kr = K + np.array([0, 0, 0.5, 0.5])
    for B in (1, 32):
        rng = np.random.default_rng(B)
        Rg = np.stack([rot(rng.normal(size=3), rng.uniform(0, np.pi)) for _ in range(B)])
        tg = rng.uniform(-60, 60, (B, 3)) + np.array([0, 0, 800.0])
        dm = rend.render(Rg, tg, Kr[None], H, W, outputs=("depth",))["depth"]
        dm = torch.where(dm > 0, dm, torch.full_like(dm, 2000.0))
        R0 = np.stack([Rg[b] @ rot(rng.normal(size=3), np.deg2rad(rng.uniform(2, 6))) for b in range(B)])
        t0 = tg + rng.uniform(-1, 1, (B, 3)) * np.array([5.0, 5.0, 15.0])
        Rd, td = torch.from_numpy(R0).to(dev), torch.from_numpy(t0).to(dev)
        Kd = torch.from_numpy(np.tile(K, (B, 1))).to(dev)
        ref = ICPRefiner(rend, (W, H), n_points=N, device=dev)
        draws = torch.from_numpy(rng.random((2, B, N))).to(dev)
        Ro, to, status, iters, err = ref.refine_batch(dm, Rd, td, Kd, draws=draws)
        torch.cuda.synchronize()
        total = timed(lambda: ref.refine_batch(dm, Rd, td, Kd, draws=draws), args.reps)

        st = L.stream_ptr(dev)
        w = ref._buffers(B, st, dev)  # the clouds of the last call
        Rf, tf = Rd.reshape(B, 9).contiguous(), td.contiguous()
        Rn, tn = torch.empty_like(Rf), torch.empty_like(tf)
        s1, i1 = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        e1 = torch.empty(B, dtype=torch.float64, device=dev)

        def icp():
            L.call("zp_icp", B, N, w["src"].data_ptr(), w["n_src"].data_ptr(), H * W, w["dst"].data_ptr(),
                   w["n_dst"].data_ptr(), H * W, draws[0].data_ptr(), draws[1].data_ptr(), 200, 5e-7, 0, MIN_FRACTION,
                   ANGLE_LIMIT, Rf.data_ptr(), tf.data_ptr(), Rn.data_ptr(), tn.data_ptr(), s1.data_ptr(), i1.data_ptr(),
                   e1.data_ptr(), None, None, None, st)

        loop = timed(icp, args.reps)
        ns, nd = w["n_src"].cpu().numpy(), w["n_dst"].cpu().numpy()
        dr = draws.cpu().numpy()
        clouds = []
        for b in range(B):
            n = min(ns[b], nd[b], N)
            clouds.append((w["src"][b, :ns[b]].cpu().numpy()[IR.draw_indices(dr[0, b, :n], ns[b])],
                           w["dst"][b, :nd[b]].cpu().numpy()[IR.draw_indices(dr[1, b, :n], nd[b])]))
        t_cpu, it_cpu = [], []
        for _ in range(3):
            a = time.perf_counter()
            it_cpu = [cpu_icp(A, Bc, 200, 5e-7)[1] for A, Bc in clouds]
            t_cpu.append((time.perf_counter() - a) * 1e3)
        it = iters.cpu().numpy()
        print(json.dumps({"case": f"icp_B{B}_{H}x{W}_N{N}_nv{len(v)}", "ms_median": round(total[0], 3),
                          "ms_min": round(total[1], 3), "icp_ms_median": round(loop[0], 3), "icp_ms_min": round(loop[1], 3),
                          "iterations_min": int(it.min()), "iterations_median": float(np.median(it)),
                          "iterations_max": int(it.max()), "status_nonzero": int((status != 0).sum()),
                          "cpu_kdtree_ms_median": round(float(np.median(t_cpu)), 3),
                          "cpu_iterations_median": float(np.median(it_cpu)), "reps": args.reps}))


if __name__ == "__main__":
    main()
