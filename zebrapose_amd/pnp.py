"""Batched on-device RANSAC-EPnP over the decode's correspondences.

Replaces, per crop, the reference's
    cv2.solvePnPRansac(Points_3D, Original_Points_2D, K, None, reprojectionError=2,
                       iterationsCount=150, flags=cv2.SOLVEPNP_EPNP); cv2.Rodrigues(rvec)
(binary_code_helper/CNN_output_to_pose.py:152-156) for a whole batch in five kernel launches
(``zp_pnp_ransac``, csrc/zp_pnp.hip), with the reference's success rule (at least 6
correspondences, :126).  Inputs stay on the device: ``PnP()(counts, xy, xyz, K)`` takes
``Decoder``'s outputs directly.

``PnPLocalOptimiser`` (``zp_pnp_lo``, csrc/zp_pnp_lo.hip) refines such a pose the way a locally
optimised RANSAC does: the consensus set is re-selected from the fitted pose and the pose becomes the
Levenberg-Marquardt minimiser of the reprojection error over it.  It stands in for the local
optimisation of the reference's default solver, Progressive-X (:132-144), without its graph cuts,
spatial coherence term or multi-model proposals; ``PnP(local_optimisation=True)`` runs it on RANSAC's
output.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

LINEMOD_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])  # :101-108


def _check_inputs(counts, xy, xyz):
    if xy.dtype != torch.int32 or xyz.dtype != torch.float32 or counts.dtype != torch.int32:
        raise ValueError("expected counts / xy int32 and xyz float32 (zp_decode outputs)")


def _k_vector(K, B, dev):
    """K: 3x3 or [B, 3, 3] (default: the reference's LINEMOD intrinsics) -> f64 [B, 4] on dev"""
    K = LINEMOD_K if K is None else np.asarray(K, dtype=np.float64)
    K = np.broadcast_to(K, (B, 3, 3))
    kv = torch.from_numpy(np.ascontiguousarray(np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1)))
    return kv.to(dev)


class PnPLocalOptimiser:
    def __init__(self, reprojection_error=2.0, rounds=4, steps=10):
        self.reprojection_error = float(reprojection_error)
        self.rounds = int(rounds)
        self.steps = int(steps)

    def __call__(self, counts, xy, xyz, K, R, t, success=None, debug=False):
        """counts, xy, xyz, K as for PnP; R f64 [B,3,3], t f64 [B,3] (device): PnP's outputs; success
        bool / int [B] or None: a false entry skips its crop.  Returns (R f64 [B,3,3], t f64 [B,3],
        inliers int32 [B], cost f64 [B], status int32 [B]) on the device (status: include/zp.h, 0 =
        refined, otherwise the pose is the input's); with debug also trace int32 [B, rounds, 2] and Hb
        f64 [B, 28]."""
        B, HW = xy.shape[0], xy.shape[1]
        dev = xy.device
        _check_inputs(counts, xy, xyz)
        if R.dtype != torch.float64 or t.dtype != torch.float64:
            raise ValueError("expected R / t float64 (zp_pnp_ransac outputs)")
        if R.device != dev or t.device != dev or xyz.device != dev or counts.device != dev:
            raise ValueError("expected every input on the device of xy")
        if tuple(R.shape) != (B, 3, 3) or tuple(t.shape) != (B, 3):
            raise ValueError("expected R [B, 3, 3] and t [B, 3]")
        kv = _k_vector(K, B, dev)
        R, t = R.contiguous(), t.contiguous()
        act = None if success is None else success.to(device=dev, dtype=torch.int32).contiguous()
        Ro, to = torch.empty_like(R), torch.empty_like(t)
        inl = torch.empty(B, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        trace = torch.empty((B, self.rounds, 2), dtype=torch.int32, device=dev) if debug else None
        Hb = torch.empty((B, 28), dtype=torch.float64, device=dev) if debug else None
        nbytes = int(L.lib.zp_pnp_lo_ws_bytes(B, HW))
        if nbytes < 0:
            raise ValueError(f"zp_pnp_lo: sizes out of range: B {B}, HW {HW}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        xy, xyz, counts = xy.contiguous(), xyz.contiguous(), counts.contiguous()
        L.call("zp_pnp_lo", B, HW, counts.data_ptr(), xy.data_ptr(), xyz.data_ptr(), kv.data_ptr(), R.data_ptr(),
               t.data_ptr(), None if act is None else act.data_ptr(), self.reprojection_error, self.rounds, self.steps,
               Ro.data_ptr(), to.data_ptr(), inl.data_ptr(), cost.data_ptr(), status.data_ptr(),
               None if trace is None else trace.data_ptr(), None if Hb is None else Hb.data_ptr(), ws.data_ptr(),
               L.stream_ptr())
        if debug:
            return Ro, to, inl, cost, status, trace, Hb
        return Ro, to, inl, cost, status


class PnP:
    def __init__(self, iterations=150, reprojection_error=2.0, confidence=0.99, min_points=6,
                 local_optimisation=False, lo_rounds=4, lo_steps=10):
        self.iterations = int(iterations)
        self.reprojection_error = float(reprojection_error)
        self.confidence = float(confidence)
        self.min_points = int(min_points)
        self.local_optimiser = (PnPLocalOptimiser(self.reprojection_error, lo_rounds, lo_steps)
                                if local_optimisation else None)

    def __call__(self, counts, xy, xyz, K=None):
        """counts int32 [B], xy int32 [B, HW, 2], xyz f32 [B, HW, 3] (device); K: 3x3 or [B, 3, 3]
        (default: the reference's LINEMOD intrinsics).  Returns (R f64 [B,3,3], t f64 [B,3],
        success bool [B], inliers int32 [B]) on the device.  With local_optimisation the pose is the
        optimiser's, and inliers its count wherever its status is 0."""
        B, HW = xy.shape[0], xy.shape[1]
        dev = xy.device
        _check_inputs(counts, xy, xyz)
        K_arg = K
        kv = _k_vector(K, B, dev)
        R = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
        t = torch.empty((B, 3), dtype=torch.float64, device=dev)
        ok = torch.empty(B, dtype=torch.int32, device=dev)
        inl = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.lib.zp_pnp_ws_bytes(B, self.iterations)), dtype=torch.uint8, device=dev)
        xy, xyz, counts = xy.contiguous(), xyz.contiguous(), counts.contiguous()
        L.call("zp_pnp_ransac", B, HW, counts.data_ptr(), xy.data_ptr(), xyz.data_ptr(), kv.data_ptr(),
               self.iterations, self.reprojection_error, self.confidence, R.data_ptr(), t.data_ptr(),
               ok.data_ptr(), inl.data_ptr(), ws.data_ptr(), L.stream_ptr())
        success = (ok != 0) & (counts >= self.min_points)
        if self.local_optimiser is not None:
            R, t, lo_inl, _, status = self.local_optimiser(counts, xy, xyz, K_arg, R, t, success)
            inl = torch.where(status == 0, lo_inl, inl)
        return R, t, success, inl
