#!/usr/bin/env python3
"""Times zp_pnp_ransac alone and followed by the local optimisation (zp_pnp_lo) on one batch:
B = 32 crops x HW = 16384 correspondences of a real pose each (0.7 px noise truncated to integer
pixels, 30% outliers).  Prints one line; nothing is tuned against it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ZP_QUIET", "1")


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from zebrapose_amd.pnp import PnP, PnPLocalOptimiser
    rng = np.random.default_rng(0)
    B, HW = a.batch, a.hw
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    pw = rng.uniform(-60, 60, (B, HW, 3)).astype(np.float32)
    t = np.stack([rng.uniform(-60, 60, B), rng.uniform(-60, 60, B), rng.uniform(500, 1100, B)], 1)
    Xc = pw.astype(np.float64) + t[:, None]
    uv = np.stack([K[0, 0] * Xc[..., 0] / Xc[..., 2] + K[0, 2], K[1, 1] * Xc[..., 1] / Xc[..., 2] + K[1, 2]], -1)
    uv = np.trunc(uv + rng.normal(0, 0.7, uv.shape))
    out = rng.random((B, HW)) < 0.3
    uv[out] += rng.integers(-120, 121, (int(out.sum()), 2))
    xy = torch.from_numpy(uv.astype(np.int32)).cuda()
    xyz = torch.from_numpy(pw).cuda()
    counts = torch.full((B,), HW, dtype=torch.int32).cuda()
    ransac, both, lo = PnP(), PnP(local_optimisation=True), PnPLocalOptimiser()
    R, tt, ok, inl = ransac(counts, xy, xyz)
    ms_r = timed(lambda: ransac(counts, xy, xyz), a.iters)
    ms_b = timed(lambda: both(counts, xy, xyz), a.iters)
    ms_l = timed(lambda: lo(counts, xy, xyz, None, R, tt, ok), a.iters)
    _, _, inl_lo, _, status, trace, _ = lo(counts, xy, xyz, None, R, tt, ok, debug=True)
    its = trace[..., 1].clamp_min(0).sum(1).float().mean().item()
    print(f"pnp_lo_bench B {B} HW {HW}: zp_pnp_ransac {ms_r:.3f} ms, with zp_pnp_lo {ms_b:.3f} ms, zp_pnp_lo alone "
          f"{ms_l:.3f} ms / batch (host-timed, {a.iters} iterations); status 0 in {(status == 0).sum().item()} crops, "
          f"mean LM iterations {its:.1f}, mean inliers {inl.float().mean().item():.0f} -> {inl_lo.float().mean().item():.0f}")


if __name__ == "__main__":
    main()
