#!/usr/bin/env python
"""Times the rectangular crops (``crop_resize``, ZP_CROP_RECT) beside the square ones on the same boxes.

B = 32 crops of 480 x 640 BGR images (one image per crop) to 256 px (image) and 128 px (GT code
planes + both masks), padded boxes of the size LM-O objects take.  Each leg is the two launches of
one batch (image crop, GT crop) through the C entry points, everything resident on the device.
Legs, alternated over ``--rounds`` rounds of ``--iters`` batches after a warm-up, device events
around each round and a host clock around the same window ending in a synchronise:
  rect           zp_crop_image_m + zp_crop_gt_m with ZP_CROP_RECT
  square         the same with ZP_CROP_SQUARE
  parent_square  zp_crop_image + zp_crop_gt of another build of the library (``--parent-lib``: the
                 commit before the method argument existed), when given
The bytes line counts what a leg has to move: each ROI's source pixels once (image 3 B, GT 3 B, two
masks 1 B each; the square ROI's zero padding is not read) plus the outputs written.  The
rectangular ROI is the box clipped to the image, the square one the box squared around its centre
and clipped, so rect reads no more source pixels than square.  Prints one JSON line.  Timed once,
not tuned: the path is a fraction of a percent of a training step either way.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ZP_QUIET", "1")


def roi_pixels(boxes, H, W, rect):
    """Source pixels inside the image that each crop's ROI covers."""
    n = 0
    for x, y, w, h in boxes:
        if rect:
            x1, y1, x2, y2 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
        else:
            w, h = max(w, 0), max(h, 0)
            cx, cy = x + w / 2, y + h / 2
            if h > w:
                x1, x2, y1, y2 = int(cx - h / 2), int(cx + h / 2), y, y + h
            else:
                x1, x2, y1, y2 = x, x + w, int(cy - w / 2), int(cy + w / 2)
            x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, W), min(y2, H)
        n += max(x2 - x1, 0) * max(y2 - y1, 0)
    return int(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--parent-lib", default=None, help="a libzp.so built from the parent commit")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("crop_rect_bench: no GPU (timings are taken on the device only)")
    from zebrapose_amd import _lib as L
    from zebrapose_amd.crop import CropPipeline

    B, H, W, S_img, S_gt = a.batch, 480, 640, 256, 128
    g = torch.Generator().manual_seed(a.seed)
    imgs = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    gts = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    mk = (torch.randint(0, 2, (B, H, W), dtype=torch.uint8, generator=g) * 255).cuda()
    rng = np.random.default_rng(a.seed)
    wh = rng.integers(60, 200, (B, 2))
    raw = np.concatenate([rng.integers(0, [W - 200, H - 200], (B, 2)), wh], axis=1)
    pad, _ = CropPipeline().boxes(raw, W, H)  # the padded boxes are the same under both methods
    box = torch.from_numpy(pad).cuda()
    idx = torch.arange(B, dtype=torch.int32, device="cuda")
    x = torch.empty((B, 3, S_img, S_img), dtype=torch.float32, device="cuda")
    code = torch.empty((B, 16, S_gt, S_gt), dtype=torch.uint8, device="cuda")
    m = torch.empty((B, S_gt, S_gt), dtype=torch.float32, device="cuda")
    e = torch.empty((B, S_gt, S_gt), dtype=torch.float32, device="cuda")
    st = L.stream_ptr()

    def leg(lib, sfx, tail):
        img_fn, gt_fn = getattr(lib, "zp_crop_image" + sfx), getattr(lib, "zp_crop_gt" + sfx)

        def run():
            rc = img_fn(imgs.data_ptr(), B, H, W, idx.data_ptr(), box.data_ptr(), B, S_img, x.data_ptr(), *tail, st)
            rc |= gt_fn(gts.data_ptr(), mk.data_ptr(), mk.data_ptr(), B, H, W, idx.data_ptr(), box.data_ptr(), B,
                        S_gt, 16, code.data_ptr(), m.data_ptr(), e.data_ptr(), *tail, st)
            if rc:
                raise RuntimeError("crop call failed")
        return run

    legs = {"rect": leg(L.lib, "_m", (L.ZP_CROP_RECT,)), "square": leg(L.lib, "_m", (L.ZP_CROP_SQUARE,))}
    outputs = {}
    if a.parent_lib:
        plib = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ("zp_crop_image", "zp_crop_gt"):
            fn = getattr(plib, name)
            fn.restype, fn.argtypes = L._SIGS[name]
        legs["parent_square"] = leg(plib, "", ())
    for k, f in legs.items():
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize()
        outputs[k] = [t.clone() for t in (x, code, m, e)]
    same = None
    if "parent_square" in outputs:  # faster and different is not faster: the square results must be the parent's
        same = all(torch.equal(p, q) for p, q in zip(outputs["square"], outputs["parent_square"]))
    dev_ms = {k: [] for k in legs}
    host_ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            host_ms[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
            dev_ms[k].append(e0.elapsed_time(e1) / a.iters)
    out_bytes = B * (3 * S_img * S_img * 4 + 16 * S_gt * S_gt + 2 * S_gt * S_gt * 4)
    res = {"batch": B, "H": H, "W": W, "crop_size_img": S_img, "crop_size_gt": S_gt, "iters": a.iters,
           "rounds": a.rounds, "square_equals_parent": same}
    for k in legs:
        res[k + "_ms"] = round(float(np.median(dev_ms[k])), 4)
        res[k + "_ms_min_max"] = [round(float(min(dev_ms[k])), 4), round(float(max(dev_ms[k])), 4)]
        res[k + "_host_ms"] = round(float(np.median(host_ms[k])), 4)
        px = roi_pixels(pad, H, W, k == "rect")
        res[k + "_roi_pixels"] = px
        res[k + "_bytes"] = px * 8 + out_bytes
    print(json.dumps(res))


if __name__ == "__main__":
    main()
