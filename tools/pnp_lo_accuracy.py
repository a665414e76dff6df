#!/usr/bin/env python3
"""Accuracy of the PnP local optimisation against the true pose, on the CPU: 24 synthetic scenes
(8 seeds x 300 / 1500 / 6000 correspondences of a +-60 mm box, 0.7 px noise truncated to integer pixels,
30% outliers), oracle/pnp_ref.solve_pnp_ransac alone and followed by tests/pnp_lo_ref.refine.
Measured, not asserted; the table is in DESIGN.md §4 "PnP local optimisation"."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pnp_ref  # noqa: E402
from tests import pnp_cases as PC  # noqa: E402
from tests import pnp_lo_cases as C  # noqa: E402
from tests import pnp_lo_ref as LO  # noqa: E402


def main():
    rows = []
    for n in (300, 1500, 6000):
        for seed in range(1, 9):
            pw, uv, Rt, tt = C.noisy_scene(n, seed)
            ref = pnp_ref.solve_pnp_ransac(pw, uv.astype(np.float32), C.K0)
            lo = LO.refine(pw, uv, C.K0, ref["R"], ref["t"])
            i0 = int(LO.select(pw.astype(np.float64), uv.astype(np.float64), ref["R"], ref["t"], LO.kvec(C.K0), 4.0)[0].sum())
            rows.append((n, PC.rot_angle_deg(ref["R"], Rt), PC.rot_angle_deg(lo["R"], Rt), np.linalg.norm(ref["t"] - tt),
                         np.linalg.norm(lo["t"] - tt), ref["inliers"], i0, lo["inliers"]))
    a = np.array(rows)
    print("scenes", len(a))
    print(f"median rotation error    {np.median(a[:, 1]):.3f} -> {np.median(a[:, 2]):.3f} deg, improved in "
          f"{100 * np.mean(a[:, 2] < a[:, 1]):.0f}% of scenes")
    print(f"median translation error {np.median(a[:, 3]):.2f} -> {np.median(a[:, 4]):.2f} mm, improved in "
          f"{100 * np.mean(a[:, 4] < a[:, 3]):.0f}% of scenes")
    g = a[:, 7] / a[:, 5] - 1
    print(f"consensus against RANSAC's f32 count: {100 * g.min():.1f}% .. {100 * g.max():.1f}%; against the f64 count "
          f"under the input pose: {100 * (a[:, 7] / a[:, 6] - 1).min():.1f}% .. {100 * (a[:, 7] / a[:, 6] - 1).max():.1f}%")


if __name__ == "__main__":
    main()
