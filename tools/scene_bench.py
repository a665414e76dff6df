"""Time zp_scene_compose against the same outputs assembled from what the library had before it
(device events around the calls, inputs resident).

    python tools/scene_bench.py [--reps 20]

B = 32 instances over 8 images of 480 x 640, four per image, each a disc of about 6 % of the image at
a depth of its own, so that discs overlap.  "fused": one zp_scene_compose call with every output.
"assembled": zp_scene_depth for scene and instance, torch gathers and compares for image, fg and the
visible masks, torch sums for the two counts and zp_mask_bbox for the boxes; its outputs are checked
to equal the fused ones before anything is timed.  Prints one JSON line: median and min milliseconds
per call over --reps calls after 3 warm-ups, and the bytes the fused pass has to move.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zebrapose_amd import _lib as L  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    B, n_img, H, W = 32, 8, 480, 640
    HW = H * W
    yy, xx = np.mgrid[:H, :W]
    depth = np.zeros((B, H, W), np.float32)
    for b in range(B):
        cy, cx = rng.uniform(140, 340), rng.uniform(180, 460)
        depth[b] = np.where((yy - cy) ** 2 + (xx - cx) ** 2 < 77 ** 2, rng.uniform(500, 1500), 0.0)
    idx = (np.arange(B) * 5) % n_img  # four instances per image, not sorted
    d = torch.from_numpy(depth).to(dev)
    sh = torch.from_numpy(rng.integers(1, 256, (B, H, W, 3)).astype(np.uint8)).to(dev)
    ii = torch.from_numpy(idx.astype(np.int32)).to(dev)
    ii64 = ii.long()
    image = torch.empty((n_img, H, W, 3), dtype=torch.uint8, device=dev)
    fg = torch.empty((n_img, H, W), dtype=torch.uint8, device=dev)
    scene = torch.empty((n_img, H, W), dtype=torch.float32, device=dev)
    inst = torch.empty((n_img, H, W), dtype=torch.int32, device=dev)
    visib = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    info = torch.empty((B, 6), dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.lib.zp_scene_compose_ws_bytes(B, n_img, H, W)), dtype=torch.uint8, device=dev)

    def fused():
        L.call("zp_scene_compose", B, n_img, H, W, d.data_ptr(), sh.data_ptr(), ii.data_ptr(), image.data_ptr(),
               fg.data_ptr(), scene.data_ptr(), inst.data_ptr(), visib.data_ptr(), info.data_ptr(), ws.data_ptr(),
               L.stream_ptr())

    scene2, inst2 = torch.empty_like(scene), torch.empty_like(inst)
    box2 = torch.empty((B, 4), dtype=torch.int32, device=dev)
    pix = torch.arange(HW, device=dev).view(1, HW)
    names = torch.arange(B, dtype=torch.int32, device=dev).view(B, 1, 1)
    res = {}

    def assembled():
        L.call("zp_scene_depth", B, d.data_ptr(), ii.data_ptr(), n_img, H, W, scene2.data_ptr(), inst2.data_ptr(),
               L.stream_ptr())
        won = inst2 >= 0
        src = (inst2.clamp(min=0).long().view(n_img, HW) * HW + pix).view(-1)
        img2 = sh.view(B * HW, 3)[src].view(n_img, H, W, 3) * won.unsqueeze(-1)
        fg2 = won.to(torch.uint8) * 255
        vis2 = (inst2[ii64] == names).to(torch.uint8) * 255
        L.call("zp_mask_bbox", vis2.data_ptr(), B, H, W, box2.data_ptr(), L.stream_ptr())
        res.update(image=img2, fg=fg2, visib=vis2,
                   info=torch.cat([(d > 0).sum((1, 2), dtype=torch.int32).view(B, 1),
                                   (vis2 != 0).sum((1, 2), dtype=torch.int32).view(B, 1), box2], 1))

    fused()
    assembled()
    torch.cuda.synchronize()
    for name, a, b in (("image", image, res["image"]), ("fg", fg, res["fg"]), ("scene", scene, scene2),
                       ("instance", inst, inst2), ("mask_visib", visib, res["visib"]), ("info", info, res["info"])):
        assert torch.equal(a, b), name
    f_med, f_min = timed(fused, args.reps)
    a_med, a_min = timed(assembled, args.reps)
    hidden = int((info[:, 1] < info[:, 0]).sum())
    moved = 4 * B * HW + 3 * n_img * HW + (3 + 1 + 4 + 4) * n_img * HW + B * HW
    print(json.dumps({"case": f"scene_B{B}_img{n_img}_{H}x{W}", "fused_ms_median": round(f_med, 4),
                      "fused_ms_min": round(f_min, 4), "assembled_ms_median": round(a_med, 4),
                      "assembled_ms_min": round(a_min, 4), "fused_MB_moved": round(moved / 1e6, 1),
                      "fused_GBps_at_median": round(moved / f_med / 1e6, 1), "depth_read_MB": round(4 * B * HW / 1e6, 1),
                      "outputs_written_MB": round((12 * n_img + B) * HW / 1e6, 1),
                      "instances_partly_hidden": hidden, "reps": args.reps}))


if __name__ == "__main__":
    main()
