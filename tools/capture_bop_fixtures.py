"""Capture tests/golden/bop_errors.npz from the reference's own BOP error functions.

Run by hand where the reference tree exists (ZP_REFERENCE, default /root/reference/zebrapose):

    python tools/capture_bop_fixtures.py

It imports lib/pysixd/pose_error.py, misc.py and visibility.py read-only, with empty stand-ins for the
modules that are absent (cv2, mmcv, numba's jit / njit, termcolor, lib.pysixd.inout), the way
oracle/capture_fixtures.py::_import_pose_error stands in for its ones, and records what
pose_error.mssd / mspd / vsd and misc.get_symmetry_transformations return for the inputs built here
(500 points, 6 poses, 48 x 64 images; tests/bop_ref.py builds the depth images with margins).
pose_error.vsd gets a stand-in renderer whose render_object hands back the stored depth images, so the
reference's whole pixel stage runs.  Nothing of the reference's program text is stored: inputs and
returned numbers only.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("ZP_REFERENCE", "/root/reference/zebrapose")
sys.path.insert(0, ROOT)

from tests import bop_ref as BR  # noqa: E402
from tests.test_bop_host import INFOS  # noqa: E402


class _Stub(types.ModuleType):
    """A module whose every attribute is 0 (constants read at definition time, e.g. cv2.SOLVEPNP_*)."""
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return 0


def _passthrough(*args, **kwargs):
    """numba.jit / njit: bare decorator or decorator factory, both leave the function as it is."""
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda f: f


def import_reference():
    for name in ("cv2", "mmcv"):
        sys.modules.setdefault(name, _Stub(name))
    nb = types.ModuleType("numba")
    nb.jit = nb.njit = _passthrough
    sys.modules.setdefault("numba", nb)
    tc = types.ModuleType("termcolor")
    tc.colored = lambda s, *a, **k: s
    sys.modules.setdefault("termcolor", tc)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import lib.pysixd as P
    io = types.ModuleType("lib.pysixd.inout")  # misc imports load_ply from it; nothing here calls it
    io.load_ply = None
    sys.modules["lib.pysixd.inout"] = io
    P.inout = io
    from lib.pysixd import misc, pose_error
    return misc, pose_error


class StoredDepth:
    """Stands in for the reference's renderer: pose_error.vsd renders est first, then gt."""
    def __init__(self, est, gt):
        self.queue = [est, gt]

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        return {"depth": self.queue.pop(0)}


def main():
    misc, pose_error = import_reference()
    rng = np.random.default_rng(2019)
    out = {}
    syms = {}
    for name, info in INFOS.items():
        trans = misc.get_symmetry_transformations(info, 0.01)
        syms[name] = trans
        out[f"sym_{name}_R"] = np.stack([np.asarray(s["R"], np.float64).reshape(3, 3) for s in trans])
        out[f"sym_{name}_t"] = np.stack([np.asarray(s["t"], np.float64).reshape(3) for s in trans])

    B = 6
    pts = rng.uniform(-60, 60, (500, 3)).astype(np.float32)
    Rg = np.stack([BR.rot(rng) for _ in range(B)])
    tg = rng.uniform(-50, 50, (B, 3)) + np.array([0, 0, 800.0])
    Re, te = Rg.copy(), tg + rng.normal(0, 2, (B, 3))
    Re[1] = Rg[1] @ BR.rot(np.random.default_rng(5))
    Re[2] = Rg[2] @ out["sym_disc2_R"][2]          # a discrete symmetry of 'disc2' away, plus the shift above
    te[2] = Rg[2] @ out["sym_disc2_t"][2] + tg[2] + 0.1
    Re[3] = Rg[3] @ out["sym_cont_R"][100]         # a continuous step away
    te[3] = Rg[3] @ out["sym_cont_t"][100] + tg[3]
    Re[4] = BR.rot(rng)
    te[5] = tg[5]                                   # identical poses
    K4 = np.stack([rng.uniform(550, 650, B), rng.uniform(550, 650, B), rng.uniform(300, 340, B),
                   rng.uniform(220, 260, B)], 1)
    out.update(pts=pts, R_est=Re, t_est=te, R_gt=Rg, t_gt=tg, K=K4)
    for name, trans in syms.items():
        ms, mp = [], []
        for b in range(B):
            K = np.array([[K4[b, 0], 0, K4[b, 2]], [0, K4[b, 1], K4[b, 3]], [0, 0, 1.0]])
            p64 = pts.astype(np.float64)
            ms.append(pose_error.mssd(Re[b], te[b].reshape(3, 1), Rg[b], tg[b].reshape(3, 1), p64, trans))
            mp.append(pose_error.mspd(Re[b], te[b].reshape(3, 1), Rg[b], tg[b].reshape(3, 1), K, p64, trans))
        out[f"mssd_{name}"] = np.array(ms, np.float64)
        out[f"mspd_{name}"] = np.array(mp, np.float64)

    H, W = 48, 64
    ti = np.array([0, 1, 2, 2, 3, 4])
    est, gt, test, Kv, diam = BR.vsd_scene(rng, B, H, W, ti)
    est[5] = gt[5]  # est == gt: zero at every tau
    gt[4, :, : W // 2] = 0
    est[4, :, W // 2:] = 0  # disjoint renders: one at every tau
    delta = 15.0
    taus_n = np.arange(0.05, 0.51, 0.05)
    taus_mm = taus_n * 100.0
    vn, vm = [], []
    for b in range(B):
        K = np.array([[Kv[b, 0], 0, Kv[b, 2]], [0, Kv[b, 1], Kv[b, 3]], [0, 0, 1.0]])
        for taus, norm, dst in ((taus_n, True, vn), (taus_mm, False, vm)):
            _, _, parts = BR.vsd_pixels(est[b], gt[b], test[ti[b]], Kv[b], delta, taus, diam[b] if norm else None,
                                        return_parts=True)
            assert BR.margins_ok(parts, delta, taus), (b, norm)
            dst.append(pose_error.vsd(Re[b], te[b], Rg[b], tg[b], test[ti[b]], K, delta, list(taus), norm,
                                      float(diam[b]), StoredDepth(est[b], gt[b]), 1, cost_type="step"))
    out.update(vsd_est=est, vsd_gt=gt, vsd_test=test, vsd_test_index=ti.astype(np.int32), vsd_K=Kv, vsd_diameter=diam,
               vsd_delta=np.float64(delta), vsd_taus_norm=taus_n, vsd_taus_mm=taus_mm,
               vsd_norm=np.array(vn, np.float64), vsd_mm=np.array(vm, np.float64))
    path = os.path.join(ROOT, "tests", "golden", "bop_errors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print("mssd", {k: np.round(out[f"mssd_{k}"], 3) for k in syms})
    print("vsd norm", np.round(out["vsd_norm"][:, ::3], 3))


if __name__ == "__main__":
    main()
