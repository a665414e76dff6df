"""Time the GT masks and info once at a BOP size (device events, inputs resident).

    python tools/gtinfo_bench.py [--reps 20] [--level 4]

Twelve instances of two LM-O-sized meshes (ellipsoidal icospheres, level 4: 2 562 vertices, 5 120
faces) over three 480 x 640 images, truncation=True (renders of 1440 x 1920), depth_test=None.
Prints one JSON line: median and min milliseconds of the whole SceneLabeler.labels call (two renders
of six, the scene composition, two zp_gt_info launches and the reordering copies) and of zp_gt_info
and zp_scene_depth alone on resident renders, with the bytes zp_gt_info streams and the rate that
makes.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zebrapose_amd.gtinfo import SceneLabeler, gt_info, scene_depth  # noqa: E402
from zebrapose_amd.render import MeshRenderer  # noqa: E402
from tools.bop_bench import timed  # noqa: E402
from tools.refine_bench import rot  # noqa: E402
from tools.render_bench import icosphere  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--level", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda")
    H, W, B, n_img = 480, 640, 12, 3
    v, f = icosphere(args.level)
    meshes = {1: (v * np.array([100.0, 70.0, 50.0])).astype(np.float32),
              2: (v * np.array([60.0, 60.0, 90.0])).astype(np.float32)}
    lab = SceneLabeler({k: MeshRenderer(m, f, device=dev) for k, m in meshes.items()})
    K = np.array([572.4114, 573.57043, 325.2611, 242.04899])
    rng = np.random.default_rng(0)
    obj_ids = np.array([1, 2] * 6)
    img_index = np.repeat(np.arange(n_img), 4)
    R = np.stack([rot(rng.normal(size=3), rng.uniform(0, np.pi)) for _ in range(B)])
    # spread over the frame, some leaving it, depths 600 .. 1100 so that instances occlude one another
    t = np.stack([rng.uniform(-330, 330, B), rng.uniform(-240, 240, B), rng.uniform(600, 1100, B)], 1)

    def whole():
        return lab.labels(obj_ids, img_index, R, t, K, H, W)

    res, scene, _ = whole()
    info = res.info.cpu().numpy()
    ms, ms_min = timed(whole, args.reps)

    Ks = np.repeat((K + np.array([0, 0, W, H]))[None], B, 0)
    big = torch.cat([lab.renderers[k].render(R[obj_ids == k], t[obj_ids == k], Ks[obj_ids == k], 3 * H, 3 * W,
                                             outputs=("depth",))["depth"] for k in (1, 2)])
    order = np.concatenate([np.flatnonzero(obj_ids == k) for k in (1, 2)])
    ti = torch.from_numpy(img_index[order].astype(np.int32)).to(dev)
    win = big[:, H:2 * H, W:2 * W].contiguous()
    g_ms, g_min = timed(lambda: gt_info(big, scene, K, window=(W, H), test_index=ti), args.reps)
    s_ms, s_min = timed(lambda: scene_depth(win, ti, n_img), args.reps)
    streamed = big.numel() * 4 + 2 * B * H * W  # the renders read once, two masks written
    print(json.dumps({"case": f"gtinfo_B{B}_{H}x{W}_trunc_nv{len(v)}", "labels_ms_median": round(ms, 3),
                      "labels_ms_min": round(ms_min, 3), "gt_info_ms_median": round(g_ms, 3),
                      "gt_info_ms_min": round(g_min, 3), "gt_info_streamed_MB": round(streamed / 1e6, 1),
                      "gt_info_GBps_at_median": round(streamed / 1e6 / g_ms, 1), "scene_depth_ms_median": round(s_ms, 3),
                      "scene_depth_ms_min": round(s_min, 3), "visib_fract_min": round(float(res.visib_fract().min()), 3),
                      "visib_fract_max": round(float(res.visib_fract().max()), 3),
                      "px_count_all_median": int(np.median(info[:, 0])), "reps": args.reps}))


if __name__ == "__main__":
    main()
