#!/usr/bin/env python
"""Times the shaded renderer and the compositor at the size a synthetic batch is made.

B = 32 frames at 640 x 480 of tools/render_bench.py's mesh (an icosphere subdivided 7 times: 163,842
vertices, 327,680 faces, radius 60 mm at 600-1000 mm in front of an LM-like camera) with random vertex
colours and its own normals, over 8 random 480 x 640 backgrounds.  Legs, alternated over ``--rounds``
rounds of ``--iters`` calls after a warm-up, device events around each round:
  render_shaded  MeshRenderer.render_shaded, outputs shaded + mask (pose upload, allocation, zp_render_shaded)
  render         MeshRenderer.render, outputs color + mask, for scale (zp_render on the same mesh and poses)
  composite      zebrapose_amd.synth.composite (zp_mask_bbox + zp_composite) on the shaded frames
Prints one JSON line.  Timed, not tuned: no rate is claimed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ZP_QUIET", "1")

from tools.render_bench import icosphere, random_rotations  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("synth_bench: no GPU (timings are taken on the device only)")
    from zebrapose_amd.render import MeshRenderer
    from zebrapose_amd.synth import SyntheticBatcher, composite

    B, H, W = a.batch, 480, 640
    v, f = icosphere(a.level)
    rng = np.random.default_rng(a.seed)
    rgb = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    mr = MeshRenderer(v * 60.0, f, colors=rgb, normals=v)
    bgs = torch.from_numpy(rng.integers(0, 256, (8, 480, 640, 3)).astype(np.uint8)).cuda()
    sb = SyntheticBatcher(mr, mr, bgs, rng=rng)
    R = random_rotations(rng, B)
    t = np.stack([rng.uniform(-150, 150, B), rng.uniform(-100, 100, B), rng.uniform(600, 1000, B)], 1)
    K = np.tile(np.array([[572.4114, 573.57043, 325.2611, 242.04899]]), (B, 1))
    d = sb.sample(B)
    frames = mr.render_shaded(R, t, K, H, W, light=d["light"], phong=d["phong"], z_near=1.0)

    legs = {"render_shaded": lambda: mr.render_shaded(R, t, K, H, W, light=d["light"], phong=d["phong"], z_near=1.0),
            "render": lambda: mr.render(R, t, K, H, W, z_near=1.0),
            "composite": lambda: composite(frames["shaded"], frames["mask"], bgs, d["bg_index"], d["trunc"])}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
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
    res = {"batch": B, "H": H, "W": W, "nv": mr.nv, "nf": mr.nf, "backgrounds": [8, 480, 640], "iters": a.iters,
           "rounds": a.rounds, "foreground_share": round(float((frames["mask"] != 0).float().mean()), 4)}
    for k in legs:
        res[k + "_ms"] = round(float(np.median(ms[k])), 4)
        res[k + "_ms_min_max"] = [round(float(min(ms[k])), 4), round(float(max(ms[k])), 4)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
