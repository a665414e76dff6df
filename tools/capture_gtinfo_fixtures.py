"""Capture tests/golden/gt_info.npz from the reference's own visibility and box functions.

Run by hand where the reference tree exists (ZP_REFERENCE, default /root/reference/zebrapose):

    python tools/capture_gtinfo_fixtures.py

It imports lib/pysixd/misc.py and visibility.py read-only, with the stand-ins of
tools/capture_bop_fixtures.py for the modules that are absent, and records what
misc.depth_im_to_dist_im_fast, visibility.estimate_visib_mask_gt (both modes) and
misc.calc_2d_bbox_xywh return for the inputs built here (5 instances over 3 scene images of
24 x 32; tests/bop_ref.py builds the depth images with margins).  Nothing of the reference's program
text is stored: inputs and returned numbers only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from capture_bop_fixtures import import_reference  # noqa: E402
from tests import bop_ref as BR  # noqa: E402
from tests import gtinfo_ref as GR  # noqa: E402


def main():
    misc, _ = import_reference()
    from lib.pysixd import visibility
    rng = np.random.default_rng(2020)
    B, H, W = 5, 24, 32
    ti = np.array([0, 1, 1, 2, 2])
    _, gt, test, K4, _ = BR.vsd_scene(rng, B, H, W, ti)
    # behind the scene by more than delta on a part of every instance, so both outcomes of the test occur
    far = rng.random(gt.shape) < 0.3
    gt = np.where(far & (gt > 0), gt + np.float32(80.0), gt).astype(np.float32)
    gt[3] = 0                      # nothing rendered
    gt[4, :, : W // 2] = 0         # half an object
    delta = 15.0
    assert GR.margin_ok(gt, (0, 0), test, K4, ti, delta)
    out = dict(depth_gt=gt, depth_test=test, test_index=ti.astype(np.int32), K=K4, delta=np.float64(delta))
    dist_gt, dist_test, boxes = [], [], []
    vis = {"bop19": [], "bop18": []}
    for b in range(B):
        K = np.array([[K4[b, 0], 0, K4[b, 2]], [0, K4[b, 1], K4[b, 3]], [0, 0, 1.0]])
        dg = misc.depth_im_to_dist_im_fast(gt[b], K)
        dt = misc.depth_im_to_dist_im_fast(test[ti[b]], K)
        dist_gt.append(dg)
        dist_test.append(dt)
        for mode in vis:
            vis[mode].append(visibility.estimate_visib_mask_gt(dt, dg, delta, visib_mode=mode))
        row = []
        for m in (gt[b] > 0, vis["bop19"][-1], vis["bop18"][-1]):
            ys, xs = np.nonzero(m)
            row.append(misc.calc_2d_bbox_xywh(xs, ys, W, H) if len(xs) else [-1, -1, -1, -1])
        boxes.append(row)
    out.update(dist_gt=np.stack(dist_gt).astype(np.float64), dist_test=np.stack(dist_test).astype(np.float64),
               visib_bop19=np.stack(vis["bop19"]).astype(np.uint8), visib_bop18=np.stack(vis["bop18"]).astype(np.uint8),
               bbox_xywh=np.array(boxes, np.int64))  # [B][mask, bop19, bop18][4]
    assert np.any(out["visib_bop19"] != out["visib_bop18"])
    path = os.path.join(ROOT, "tests", "golden", "gt_info.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print("visible pixels", out["visib_bop19"].sum((1, 2)), out["visib_bop18"].sum((1, 2)))
    print("boxes", out["bbox_xywh"][:, 1].tolist())


if __name__ == "__main__":
    main()
