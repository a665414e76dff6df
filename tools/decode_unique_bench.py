#!/usr/bin/env python3
"""Times decode + PnP on a batch of synthetic crops with the non-unique correspondences (one per mask
pixel, ``Decoder(...)``) and the unique ones (one per class id, ``Decoder(..., unique=True)``).

B crops of 128 x 128 with a full-disc mask whose ids encode a planted pose (each pixel's LUT row is
its own ray cut at a smooth depth), so RANSAC stops early as on real crops.  Case (a): 16-bit ids,
one pixel per class.  Case (b): the same crops with ignore_bit=6 (16 pixels per class: two rows of
an 8 x 8 block).  The four variants alternate inside every round; each figure is the median over the
rounds of the mean time of --iters calls between two device events.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ZP_QUIET", "1")

K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def scene(S=128, bbox=(260, 180, 128, 128)):
    """-> (mask bool [S, S], ids [S, S], lut f64 [65536, 3]): id = 4 * ((block * 64) + row-major index
    inside the 8 x 8 block), the four ids of a pixel share its 3D point"""
    y, x = np.mgrid[0:S, 0:S]
    idx = ((y // 8) * (S // 8) + x // 8) * 64 + (y % 8) * 8 + x % 8
    ids = idx * 4
    mask = (x - S / 2 + 0.5) ** 2 + (y - S / 2 + 0.5) ** 2 <= (S / 2) ** 2
    R, t = rodrigues(np.array([0.2, 0.4, -0.3])), np.array([10.0, -20.0, 800.0])
    u, v = x + bbox[0], y + bbox[1]
    z = 800.0 + 0.3 * (x - S / 2) - 0.2 * (y - S / 2) + 20.0 * np.sin(x / 9.0) * np.cos(y / 7.0)
    pc = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], -1).reshape(-1, 3)
    pts = (pc - t) @ R
    lut = np.zeros((65536, 3))
    for j in range(4):
        lut[ids.reshape(-1) + j] = pts
    return mask, ids, lut


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_unique_bench needs a GPU")
    from zebrapose_amd.decode import Decoder
    from zebrapose_amd.pnp import PnP
    S, bbox = 128, (260, 180, 128, 128)
    mask, ids, lut = scene(S, bbox)
    bits = ((ids[None] >> (15 - np.arange(16))[:, None, None]) & 1) > 0
    code = torch.from_numpy(np.where(bits, 1.0, -1.0).astype(np.float32))[None].repeat(a.batch, 1, 1, 1).cuda()
    mlog = torch.from_numpy(np.where(mask, 1.0, -1.0).astype(np.float32))[None, None].repeat(a.batch, 1, 1, 1).cuda()
    bb = torch.tensor([bbox] * a.batch, dtype=torch.int32, device="cuda")
    decs = {"a": Decoder(lut, device="cuda"), "b": Decoder(lut, device="cuda", ignore_bit=6)}
    pnp = PnP()
    variants = [(c, u) for c in ("a", "b") for u in (False, True)]

    def step(c, u):
        counts, xy, xyz = decs[c](mlog, code, bb, bbox_size=S, unique=u)
        return counts, pnp(counts, xy, xyz, K)

    res = {"batch": a.batch, "H": S, "W": S, "iters": a.iters, "rounds": a.rounds, "mask_pixels": int(mask.sum())}
    for c, u in variants:
        for _ in range(a.warmup):
            counts, (R, t, ok, inl) = step(c, u)
        torch.cuda.synchronize()
        name = f"{c}_{'unique' if u else 'nonunique'}"
        res[name + "_count"] = int(counts[0])
        res[name + "_success"] = int(ok.sum())
        res[name + "_inliers"] = int(inl[0])
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                step(*v)
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) / a.iters)
    for (c, u), ts in times.items():
        name = f"{c}_{'unique' if u else 'nonunique'}"
        res[name + "_ms"] = round(float(np.median(ts)), 4)
        res[name + "_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
