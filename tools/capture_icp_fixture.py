"""Capture tests/golden/icp.npz from the reference's own ICP functions.

Run by hand where the reference tree exists (ZP_REFERENCE, default /root/reference/zebrapose) and
scikit-learn is installed:

    python tools/capture_icp_fixture.py

It imports zebrapose/icp/icp_utils.py read-only, with an empty stand-in for its OpenGL renderer module
(zebrapose.icp.opengl_utils, which nothing called here uses), and records what rgbd_to_point_cloud,
best_fit_transform (all three modes) and icp return for the inputs built here: a 24 x 32 depth image and
two sets of 60 random points related by a 5 degree / 3 mm motion plus noise.  Nothing of the
reference's program text is stored: inputs and returned numbers only.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("ZP_REFERENCE", "/root/reference/zebrapose")
sys.path.insert(0, ROOT)

from tests import refine_ref as RF  # noqa: E402


def import_reference():
    sys.path.insert(0, os.path.dirname(REF.rstrip("/")))
    sys.modules["zebrapose.icp.opengl_utils"] = types.ModuleType("zebrapose.icp.opengl_utils")
    from zebrapose.icp import icp_utils
    return icp_utils


def inputs():
    rng = np.random.default_rng(20)
    depth = np.zeros((24, 32), np.float32)
    yy, xx = np.mgrid[:24, :32]
    blob = (yy - 11) ** 2 + (xx - 17) ** 2 < 70
    depth[blob] = (600 + 40 * rng.random(blob.sum())).astype(np.float32)
    K = np.array([[120.0, 0, 15.5], [0, 118.0, 11.25], [0, 0, 1]])
    A = rng.normal(size=(60, 3)) * np.array([40.0, 30.0, 20.0]) + np.array([5.0, -8.0, 700.0])
    Rm = RF.rodrigues([0.4, -0.5, 0.75], np.deg2rad(5.0))
    c = A.mean(0)
    tm = np.array([2.0, -1.0, 2.0])  # 3 mm
    B = (A - c) @ Rm.T + c + tm + rng.normal(size=A.shape) * 0.05
    return depth, K, A, B[rng.permutation(60)], Rm, tm


def main():
    ref = import_reference()
    depth, K, A, B, Rm, tm = inputs()
    out = dict(depth=depth, K=K, A=A, B=B, motion_R=Rm, motion_t=tm)
    out["cloud"] = ref.rgbd_to_point_cloud(K, depth)
    # corresponding pairs for the fit: B reordered by its nearest neighbours, as icp's first step does
    _, idx = ref.nearest_neighbor(A, B)
    out["nn0"] = idx.astype(np.int64)
    for name, kw in (("full", {}), ("depth_only", dict(depth_only=True)), ("no_depth", dict(no_depth=True))):
        T, R, t = ref.best_fit_transform(A, B[idx], **kw)
        out[f"fit_{name}_T"], out[f"fit_{name}_R"], out[f"fit_{name}_t"] = T, R, np.asarray(t)
        T, dist, i = ref.icp(A, B, tolerance=0.0000005, **kw)
        out[f"icp_{name}_T"], out[f"icp_{name}_dist"], out[f"icp_{name}_i"] = T, dist, np.int64(i)
    path = os.path.join(ROOT, "tests", "golden", "icp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
