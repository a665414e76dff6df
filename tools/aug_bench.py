#!/usr/bin/env python
"""Times the training data path on the device against the crop-only path it extends.

B = 32 crops of 480 x 640 BGR images (one image per crop), boxes of the size LM-O objects take.
Legs, alternated over ``--rounds`` rounds of ``--iters`` calls after a warm-up, device events around
each round (the host work between launches is inside the window) and a host clock around the same
window ending in a synchronise:
  crop        CropPipeline.__call__ on padded boxes             (the baseline: the crop kernels alone)
  train       CropPipeline.train_batch                          (box jitter + sampler + zp_augment + crops)
  augment     the zp_augment launch alone, descriptors resident, bbox form (what train_batch launches)
  augment_all the same with bbox = NULL                         (whole images; bytes = 2 * B * H * W * 3)
The augment legs report the bytes the op has to move (the tiles it reads, halo not counted, plus
the tiles it writes) over their time.  Prints one JSON line.
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


def tiles_bytes(boxes, H, W, T=32):
    """Bytes zp_augment's bbox form reads + writes: the 32 x 32 tiles meeting each crop's copied region."""
    n = 0
    for x, y, w, h in boxes:
        w, h = max(w, 0), max(h, 0)
        s = max(w, h)
        if s <= 0:
            continue
        cx, cy = x + w / 2, y + h / 2
        if h > w:
            x1, x2, y1, y2 = int(cx - h / 2), int(cx + h / 2), y, y + h
        else:
            x1, x2, y1, y2 = x, x + w, int(cy - w / 2), int(cy + w / 2)
        x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, W), min(y2, H)
        if x2 <= x1 or y2 <= y1:
            continue
        px = (min((x2 - 1) // T * T + T, W) - x1 // T * T) * (min((y2 - 1) // T * T + T, H) - y1 // T * T)
        n += 2 * 3 * px
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aug_bench: no GPU (timings are taken on the device only)")
    from zebrapose_amd import _lib as L
    from zebrapose_amd.augment import AugmentSampler, _pack
    from zebrapose_amd.crop import CropPipeline

    B, H, W = a.batch, 480, 640
    g = torch.Generator().manual_seed(a.seed)
    imgs = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    gts = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    mk = (torch.randint(0, 2, (B, H, W), dtype=torch.uint8, generator=g) * 255).cuda()
    rng = np.random.default_rng(a.seed)
    wh = rng.integers(60, 200, (B, 2))
    raw = np.concatenate([rng.integers(0, [W - 200, H - 200], (B, 2)), wh], axis=1)
    idx = np.arange(B)
    cp = CropPipeline()
    pad, _ = cp.boxes(raw, W, H)
    sampler = AugmentSampler(True, True, np.random.default_rng(a.seed))
    aug_boxes, _ = cp.train_boxes(raw, W, H, np.random.default_rng(a.seed + 1))
    batch = AugmentSampler(True, True, np.random.default_rng(a.seed + 2)).sample(B, H, W)
    idx_d = torch.arange(B, dtype=torch.int32, device="cuda")
    box_d = torch.from_numpy(aug_boxes).cuda()
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
    buf, offs = _pack(batch)
    dbuf = torch.from_numpy(buf).cuda()
    p = [dbuf.data_ptr() + o for o in offs]
    mh, mw = batch.masks.shape[1:]

    def launch(bbox):
        L.call("zp_augment", imgs.data_ptr(), B, H, W, idx_d.data_ptr(), p[0], p[1], mh, mw, p[2], p[3], bbox, B,
               out.data_ptr(), L.stream_ptr())

    legs = {
        "crop": lambda: cp(imgs, idx, pad, gts, mk, mk),
        "train": lambda: cp.train_batch(imgs, idx, raw, gts, mk, mk, sampler),
        "augment": lambda: launch(box_d.data_ptr()),
        "augment_all": lambda: launch(None),
    }
    for f in legs.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
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
    res = {"batch": B, "H": H, "W": W, "iters": a.iters, "rounds": a.rounds,
           "flags_on": int((batch.flags != 0).sum())}
    for k in legs:
        res[k + "_ms"] = round(float(np.median(dev_ms[k])), 4)
        res[k + "_ms_min_max"] = [round(float(min(dev_ms[k])), 4), round(float(max(dev_ms[k])), 4)]
        res[k + "_host_ms"] = round(float(np.median(host_ms[k])), 4)
    for k, nbytes in (("augment", tiles_bytes(aug_boxes, H, W)), ("augment_all", 2 * B * H * W * 3)):
        res[k + "_bytes"] = int(nbytes)
        res[k + "_GBps"] = round(nbytes / (res[k + "_ms"] * 1e-3) / 1e9, 1)
    res["train_minus_crop_ms"] = round(res["train_ms"] - res["crop_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
