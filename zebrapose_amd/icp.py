"""ICP refinement against measured depth on the device (``zp_depth_points``, ``zp_icp``;
csrc/zp_icp.hip).

The reference's ``ICPRefiner`` (zebrapose/icp/icp_utils.py:129-176) renders the model's depth at the
estimated pose with OpenGL, back-projects it and the measured depth crop to point clouds, keeps the
measured points near the rendered cloud, subsamples both and runs point-to-point ICP with sklearn's
neighbour search, one pose at a time on the CPU.  Here the depth comes from ``zp_render``, the clouds
from ``zp_depth_points`` and the whole loop of a pose from one ``zp_icp`` workgroup; a batch of poses
stays on the device from ``PnP`` to the pose errors.  The exact semantics and the deviations from the
reference are in include/zp.h and, as numpy, in tests/icp_ref.py.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .render import MeshRenderer

FULL, DEPTH_ONLY, NO_DEPTH = 0, 1, 2
MIN_FRACTION = 1.0 / 20.0          # icp_utils.py:149
ANGLE_LIMIT = 20 * np.pi / 180.0   # icp_utils.py:161


def _k4(K, B, dev):
    Kn = K if isinstance(K, torch.Tensor) else torch.from_numpy(np.asarray(K, dtype=np.float64))
    Kd = Kn.to(dev).to(torch.float64)
    if Kd.shape == (3, 3):
        Kd = torch.stack([Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]])
    Kd = Kd.reshape(-1, 4)
    if Kd.shape[0] == 1 and B > 1:
        Kd = Kd.expand(B, 4)
    if Kd.shape[0] != B:
        raise ValueError("one K per image is needed (or one for all)")
    return Kd.contiguous()


def _depth_points(depth, Kd, cap, filt, factor, stats, counts, pts, st):
    B, H, W = depth.shape
    L.call("zp_depth_points", B, H, W, depth.data_ptr(), Kd.data_ptr(), cap, L.ptr(filt), float(factor),
           counts.data_ptr(), pts.data_ptr(), L.ptr(stats), None, st)


def depth_points(depth, K, cap=None, filter=None, factor=2.0, want_stats=False, device="cuda"):
    """Back-project B depth images to point clouds (rgbd_to_point_cloud, icp_utils.py:7-13).

    depth [B, H, W] (or [H, W]; read as f32, a pixel counts when finite and > 0), K: [B, 4] = (fx, fy,
    cx, cy), one such row or one 3 x 3 matrix.  ``filter`` f64 [B, 4] = (centre xyz, radius) keeps the
    points closer than ``factor`` * radius to the centre (:147-148).  Returns device tensors (counts
    i32 [B], pts f64 [B, cap, 3]) and, with ``want_stats``, stats f64 [B, 4]: the centroid of the kept
    points and the largest distance from it (:139-141), which is a later call's ``filter``.
    counts[b] is the true count, of which the first cap (default H * W: all) are stored, in row-major
    pixel order."""
    dev = depth.device if isinstance(depth, torch.Tensor) and depth.is_cuda else torch.device(device)
    d = torch.as_tensor(depth, device=dev).to(torch.float32)
    if d.dim() == 2:
        d = d[None]
    if d.dim() != 3:
        raise ValueError("depth must be [B, H, W]")
    d = d.contiguous()
    B, H, W = (int(v) for v in d.shape)
    cap = H * W if cap is None else int(cap)
    if L.lib.zp_depth_points_ws_bytes(B, H, W, cap) < 0:
        raise ValueError(f"sizes out of range: B {B}, {H} x {W}, cap {cap}")
    Kd = _k4(K, B, dev)
    filt = None
    if filter is not None:
        filt = torch.as_tensor(filter, device=dev).to(torch.float64).reshape(-1, 4).contiguous()
        if filt.shape[0] != B:
            raise ValueError("one filter row per image is needed")
    with torch.cuda.device(dev):
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        pts = torch.zeros((B, cap, 3), dtype=torch.float64, device=dev)
        stats = torch.empty((B, 4), dtype=torch.float64, device=dev) if want_stats else None
        _depth_points(d, Kd, cap, filt, factor, stats, counts, pts, L.stream_ptr(dev))
    return (counts, pts, stats) if want_stats else (counts, pts)


class ICPRefiner:
    """The reference's ``ICPRefiner`` for batches of poses of one mesh.

    ``model`` is a ``MeshRenderer`` or a dict with ``'pts'`` [nv, 3] and ``'faces'`` [nf, 3] as the
    reference's ``inout.load_ply`` returns; ``im_size`` = (width, height) of the depth images.  Poses,
    the mesh and the measured depth share one unit (the reference: millimetres).  The subsamples are
    drawn on the host from ``numpy.random.default_rng(seed)``: uniform numbers in [0, 1), entry i of a
    subsample being point floor(draw[i] * count) (the reference: np.random.choice's global stream)."""

    def __init__(self, model, im_size, n_points=3000, max_iterations=200, tolerance=5e-7, device="cuda", seed=None):
        if isinstance(model, MeshRenderer):
            self.renderer = model
        else:
            self.renderer = MeshRenderer(model["pts"], np.asarray(model["faces"]).astype(np.int64), device=device)
        self.width, self.height = int(im_size[0]), int(im_size[1])
        self.n_points, self.max_iterations, self.tolerance = int(n_points), int(max_iterations), float(tolerance)
        if L.lib.zp_icp_ws_bytes(1, self.n_points) < 0:
            raise ValueError(f"n_points out of range: {self.n_points}")
        if L.lib.zp_depth_points_ws_bytes(1, self.height, self.width, self.height * self.width) < 0:
            raise ValueError(f"image size out of range: {self.height} x {self.width}")
        if self.max_iterations < 1 or self.tolerance != self.tolerance:
            raise ValueError("max_iterations must be at least 1 and tolerance a number")
        self.rng = np.random.default_rng(seed)
        self._ws = {}  # (stream, B) -> buffers

    def _buffers(self, B, st, dev):
        """Per (stream, B), kept for the refiner's lifetime: the render workspace, the rendered depth and
        both whole clouds, f64 [B, H * W, 3] each (24 H W bytes a pose and cloud: 236 MB each at B = 32,
        640 x 480), although zp_icp reads only the points the draws select."""
        key = (st, B)
        buf = self._ws.get(key)
        if buf is None:
            r = self.renderer
            H, W = self.height, self.width
            need_r = L.lib.zp_render_ws_bytes(B, r.nv, r.nf, H, W)
            if need_r < 0 or L.lib.zp_depth_points_ws_bytes(B, H, W, H * W) < 0 or L.lib.zp_icp_ws_bytes(B, 1) < 0:
                raise ValueError(f"sizes out of range: B {B}, {H} x {W}")
            f64, i32 = torch.float64, torch.int32
            buf = self._ws[key] = dict(
                ws_r=torch.empty(need_r, dtype=torch.uint8, device=dev),
                depth=torch.empty((B, H, W), dtype=torch.float32, device=dev),
                src=torch.empty((B, H * W, 3), dtype=f64, device=dev), dst=torch.empty((B, H * W, 3), dtype=f64, device=dev),
                n_src=torch.empty(B, dtype=i32, device=dev), n_dst=torch.empty(B, dtype=i32, device=dev),
                stats=torch.empty((B, 4), dtype=f64, device=dev))
        return buf

    def refine_batch(self, depth, R, t, K, mode=FULL, max_mean_dist_factor=2.0, draws=None, z_near=1e-6):
        """depth [B, H, W] measured depth (0 = nothing), R [B, 3, 3] (or [B, 9]), t [B, 3], K: [B, 4] =
        (fx, fy, cx, cy), one such row or one 3 x 3 matrix; ``mode`` 0 full, 1 depth_only, 2 no_depth.
        ``draws`` f64 [2, B, n_points] in [0, 1) (rendered cloud, measured cloud) replaces the
        refiner's own generator.  Tensors on the device are used where they are (``PnP``'s R and t);
        nothing synchronises the host.  Returns device tensors (R f64 [B, 3, 3], t f64 [B, 3], status
        i32 [B], iterations i32 [B], mean_error f64 [B]); a pose whose status (include/zp.h) is not 0
        comes back as it went in."""
        r = self.renderer
        dev = r.device
        if mode not in (FULL, DEPTH_ONLY, NO_DEPTH):
            raise ValueError("mode must be 0 (full), 1 (depth_only) or 2 (no_depth)")
        Rd = torch.as_tensor(R, device=dev).to(torch.float64).reshape(-1, 9).contiguous()
        B = int(Rd.shape[0])
        td = torch.as_tensor(t, device=dev).to(torch.float64).reshape(-1, 3).contiguous()
        if B == 0 or td.shape[0] != B:
            raise ValueError("R and t disagree on the batch size")
        Kd = _k4(K, B, dev)
        H, W, N = self.height, self.width, self.n_points
        dm = torch.as_tensor(depth, device=dev).to(torch.float32).contiguous()
        if dm.shape != (B, H, W):
            raise ValueError(f"depth must be [{B}, {H}, {W}]")
        if draws is None:
            draws = self.rng.random((2, B, N))
        dr = torch.as_tensor(draws, device=dev).to(torch.float64).contiguous()
        if dr.shape != (2, B, N):
            raise ValueError(f"draws must be [2, {B}, {N}]")
        with torch.cuda.device(dev):
            st = L.stream_ptr(dev)
            w = self._buffers(B, st, dev)
            # the reference's pixel centres sit at integers (rgbd_to_point_cloud), zp_render's at half-integers
            Kr = Kd + torch.tensor([0.0, 0.0, 0.5, 0.5], dtype=torch.float64, device=dev)
            L.call("zp_render", B, r.vertices.data_ptr(), r.nv, r.faces.data_ptr(), r.nf, None, Rd.data_ptr(),
                   td.data_ptr(), Kr.data_ptr(), H, W, float(z_near), None, w["depth"].data_ptr(), None, None,
                   w["ws_r"].data_ptr(), st)
            _depth_points(w["depth"], Kd, H * W, None, 0.0, w["stats"], w["n_src"], w["src"], st)
            _depth_points(dm, Kd, H * W, w["stats"], max_mean_dist_factor, None, w["n_dst"], w["dst"], st)
            R_out, t_out = torch.empty_like(Rd), torch.empty_like(td)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            iters = torch.empty(B, dtype=torch.int32, device=dev)
            err = torch.empty(B, dtype=torch.float64, device=dev)
            L.call("zp_icp", B, N, w["src"].data_ptr(), w["n_src"].data_ptr(), H * W, w["dst"].data_ptr(),
                   w["n_dst"].data_ptr(), H * W, dr[0].data_ptr(), dr[1].data_ptr(), self.max_iterations,
                   self.tolerance, int(mode), MIN_FRACTION, ANGLE_LIMIT, Rd.data_ptr(), td.data_ptr(),
                   R_out.data_ptr(), t_out.data_ptr(), status.data_ptr(), iters.data_ptr(), err.data_ptr(), None,
                   None, None, st)
        return R_out.reshape(B, 3, 3), t_out, status, iters, err

    def refine(self, depth_crop, R_est, t_est, K_test, depth_only=False, no_depth=False, max_mean_dist_factor=2.0,
               draws=None):
        """The reference's ``refine`` (icp_utils.py:134-176) for one pose: depth_crop [H, W], R_est
        [3, 3], t_est [3] or [3, 1], K_test 3 x 3.  Returns numpy (R [3, 3], t [3]), the input pose where
        the reference returns it.  ``depth_only`` and ``no_depth`` together are not supported (the
        reference then fits the full transform but still applies the angle limit)."""
        if depth_only and no_depth:
            raise ValueError("depth_only and no_depth exclude each other")
        mode = DEPTH_ONLY if depth_only else (NO_DEPTH if no_depth else FULL)
        d = torch.as_tensor(np.asarray(depth_crop, dtype=np.float32) if not isinstance(depth_crop, torch.Tensor)
                            else depth_crop)
        Ro, to, _, _, _ = self.refine_batch(d.reshape(1, self.height, self.width), np.asarray(R_est, np.float64).reshape(1, 9),
                                            np.asarray(t_est, np.float64).reshape(1, 3), K_test, mode,
                                            max_mean_dist_factor, draws)
        return Ro[0].cpu().numpy(), to[0].cpu().numpy()
