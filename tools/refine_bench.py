"""Time the edge refinement once at the workload's size (device events, inputs resident).

    python tools/refine_bench.py [--reps 10] [--level 5]

B = 32 poses at 640 x 480 of an LM-O-sized mesh (an ellipsoidal icosphere, level 5: 10 242 vertices,
20 480 faces, 100 x 70 x 50 mm half-axes at 800 mm), ten iterations.  The observed contour is the
true pose's, the starts are perturbed by a few degrees and millimetres.  Prints one JSON line: median
and min milliseconds of the whole ten-iteration refine, and of its two parts timed apart (ten depth
renders, ten steps on the last depth).  No reference timing exists to compare with.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zebrapose_amd import _lib as L  # noqa: E402
from zebrapose_amd.refine import EdgeRefiner, mask_contour  # noqa: E402
from zebrapose_amd.render import MeshRenderer  # noqa: E402
from tools.bop_bench import timed  # noqa: E402
from tools.render_bench import icosphere  # noqa: E402


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--level", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    B, H, W, iters = 32, 480, 640, 10
    v, f = icosphere(args.level)
    v = (v * np.array([100.0, 70.0, 50.0])).astype(np.float32)
    rend = MeshRenderer(v, f, device=dev)
    K = np.array([572.4114, 573.57043, 325.2611, 242.04899])
    Rg = np.stack([rot(rng.normal(size=3), rng.uniform(0, np.pi)) for _ in range(B)])
    tg = rng.uniform(-60, 60, (B, 3)) + np.array([0, 0, 800.0])
    Kr = K + np.array([0, 0, 0.5, 0.5])
    mask = rend.render(Rg, tg, Kr[None], H, W, outputs=("mask",))["mask"]
    # the contour of a whole image: a 640 x 640 "crop" holding it, mapped one to one
    sq = torch.zeros((B, W, W), dtype=torch.uint8, device=dev)
    sq[:, :H] = mask
    counts, xy = mask_contour(sq, None, np.tile([0, 0, W, W], (B, 1)), cap=4096)
    R0 = np.stack([Rg[b] @ rot(rng.normal(size=3), np.deg2rad(rng.uniform(2, 6))) for b in range(B)])
    t0 = tg + rng.uniform(-1, 1, (B, 3)) * np.array([5.0, 5.0, 15.0])
    Rd, td = torch.from_numpy(R0).to(dev), torch.from_numpy(t0).to(dev)
    Kd = torch.from_numpy(np.tile(K, (B, 1))).to(dev)
    ref = EdgeRefiner(rend, H, W, iterations=iters)
    Ro, to, status, cost = ref.refine(Rd, td, Kd, counts, xy)
    torch.cuda.synchronize()
    total = timed(lambda: ref.refine(Rd, td, Kd, counts, xy), args.reps)

    st = L.stream_ptr(dev)
    ws_r, ws_s, depth = ref._buffers(B, st, dev)
    Rf, tf = Rd.reshape(B, 9).contiguous(), td.contiguous()
    Krd = Kd + torch.tensor([0, 0, 0.5, 0.5], dtype=torch.float64, device=dev)
    Rn, tn = torch.empty_like(Rf), torch.empty_like(tf)
    c1 = torch.empty(B, dtype=torch.int64, device=dev)
    s1 = torch.empty(B, dtype=torch.int32, device=dev)
    cap = int(xy.shape[1])

    def renders():
        for _ in range(iters):
            L.call("zp_render", B, rend.vertices.data_ptr(), rend.nv, rend.faces.data_ptr(), rend.nf, None, Rf.data_ptr(),
                   tf.data_ptr(), Krd.data_ptr(), H, W, 1e-6, None, depth.data_ptr(), None, None, ws_r.data_ptr(), st)

    def steps():
        for _ in range(iters):
            L.call("zp_edge_refine_step", B, H, W, depth.data_ptr(), counts.data_ptr(), xy.data_ptr(), cap, Rf.data_ptr(),
                   tf.data_ptr(), Kd.data_ptr(), ref.lambda_rot, ref.lambda_trans, Rn.data_ptr(), tn.data_ptr(),
                   c1.data_ptr(), s1.data_ptr(), None, None, 0, None, None, ws_s.data_ptr(), st)

    r = timed(renders, args.reps)
    s = timed(steps, args.reps)
    cost = cost.cpu().numpy()
    print(json.dumps({"case": f"edge_refine_B{B}_{H}x{W}_nv{len(v)}_nf{len(f)}_it{iters}",
                      "ms_median": round(total[0], 3), "ms_min": round(total[1], 3),
                      "render_ms_median": round(r[0], 3), "render_ms_min": round(r[1], 3),
                      "step_ms_median": round(s[0], 3), "step_ms_min": round(s[1], 3),
                      "contour_points_mean": float(counts.float().mean()), "status_nonzero": int((status != 0).sum()),
                      "cost_first_mean": float(cost[0].mean()), "cost_last_mean": float(cost[-1].mean())}))


if __name__ == "__main__":
    main()
