"""Edge refinement on the device (``zp_mask_contour``, ``zp_edge_refine_step``; csrc/zp_refine.hip).

The reference's best LM-O numbers come from ``refine = True`` (test.py:276-313): after PnP it takes
the outer contour of the object's entire mask, keeps the pixels the visible mask supports, and hands
them to ``py_edge_refine`` (edge_refine/examples/edge_refine.cpp), ten Gauss-Newton steps that each
render the model, match every observed contour pixel to the nearest pixel of the rendered
silhouette's contour and move the pose so that the matched surface points project onto the observed
pixels.  Here the contour comes from ``mask_contour``, the render from ``zp_render`` and the step
from ``zp_edge_refine_step``; poses stay on the device from ``PnP`` to the pose errors.  The exact
semantics and the deviations from the reference are in include/zp.h and, as numpy, in
tests/refine_ref.py.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .render import MeshRenderer, read_ply


def _u8(m, dev):
    m = torch.as_tensor(m, device=dev)
    if m.dtype != torch.uint8:
        m = (m != 0).to(torch.uint8)
    return m.contiguous()


def mask_contour(entire, visible, bbox, cap=None, device="cuda"):
    """The visible contour of B mask crops in image coordinates (test.py:300-307).

    entire [B, S, S] (non-zero = object), visible [B, S, S] or None, bbox int [B, 4] = (x, y, w, h) of
    each crop in the image.  Returns device tensors (counts i32 [B], xy i32 [B, cap, 2]); counts[b] is
    the true number of contour pixels, of which the first cap (default S * S: all) are stored."""
    dev = entire.device if isinstance(entire, torch.Tensor) and entire.is_cuda else torch.device(device)
    ent = _u8(entire, dev)
    if ent.dim() != 3 or ent.shape[1] != ent.shape[2]:
        raise ValueError("entire must be [B, S, S]")
    B, S = int(ent.shape[0]), int(ent.shape[1])
    vis = None
    if visible is not None:
        vis = _u8(visible, dev)
        if vis.shape != ent.shape:
            raise ValueError("visible must have the shape of entire")
    bb = torch.as_tensor(bbox, device=dev).to(torch.int32).reshape(-1, 4).contiguous()
    if bb.shape[0] != B:
        raise ValueError("one bbox per crop is needed")
    cap = S * S if cap is None else int(cap)
    with torch.cuda.device(dev):
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        xy = torch.zeros((B, max(cap, 1), 2), dtype=torch.int32, device=dev)
        L.call("zp_mask_contour", B, S, ent.data_ptr(), L.ptr(vis), bb.data_ptr(), cap, counts.data_ptr(),
               xy.data_ptr(), L.stream_ptr(dev))
    return counts, xy


class EdgeRefiner:
    """py_edge_refine's loop for batches of poses of one mesh.

    ``renderer`` holds the mesh; poses are in the mesh's units (millimetres for BOP models) and
    ``unit`` is that unit in metres: the reference works in metres with lambda_rot = 5000 and
    lambda_trans = 500000, and the same problem in mesh units has lambda_trans * unit^2."""

    def __init__(self, renderer: MeshRenderer, height, width, iterations=10, lambda_rot=5000., lambda_trans=500000.,
                 unit=0.001):
        self.renderer = renderer
        self.height, self.width = int(height), int(width)
        self.iterations = int(iterations)
        if self.iterations < 1:
            raise ValueError("iterations must be at least 1")
        self.lambda_rot = float(lambda_rot)
        self.lambda_trans = float(lambda_trans) * float(unit) ** 2
        if L.lib.zp_edge_refine_ws_bytes(1, self.height, self.width) < 0:
            raise ValueError(f"image size out of range: {self.height} x {self.width}")
        self._ws = {}  # (stream, B) -> (render workspace, step workspace, depth)

    def _buffers(self, B, st, dev):
        key = (st, B)
        buf = self._ws.get(key)
        if buf is None:
            r = self.renderer
            need_r = L.lib.zp_render_ws_bytes(B, r.nv, r.nf, self.height, self.width)
            need_s = L.lib.zp_edge_refine_ws_bytes(B, self.height, self.width)
            if need_r < 0 or need_s < 0:
                raise ValueError(f"sizes out of range: B {B}, {self.height} x {self.width}")
            buf = self._ws[key] = (torch.empty(need_r, dtype=torch.uint8, device=dev),
                                   torch.empty(need_s, dtype=torch.uint8, device=dev),
                                   torch.empty((B, self.height, self.width), dtype=torch.float32, device=dev))
        return buf

    def refine(self, R, t, K, counts, xy, z_near=1e-6):
        """R [B, 3, 3] (or [B, 9]), t [B, 3], K: [B, 4] = (fx, fy, cx, cy), one such row or one 3 x 3
        matrix; counts i32 [B] and xy i32 [B, cap, 2] from ``mask_contour``.  Tensors on the device
        are used where they are (``PnP``'s R and t, ``mask_contour``'s counts and xy); nothing
        synchronises the host.  Returns device tensors (R f64 [B, 3, 3], t f64 [B, 3], status i32 [B],
        cost i64 [iterations, B]).  A pose for which any iteration reported a status other than 0
        (include/zp.h) comes back as it went in, with that status."""
        r = self.renderer
        dev = r.device
        Rd = torch.as_tensor(R, device=dev).to(torch.float64).reshape(-1, 9).contiguous()
        B = int(Rd.shape[0])
        td = torch.as_tensor(t, device=dev).to(torch.float64).reshape(-1, 3).contiguous()
        Kn = K if isinstance(K, torch.Tensor) else torch.from_numpy(np.asarray(K, dtype=np.float64))
        Kd = Kn.to(dev).to(torch.float64)
        if Kd.shape == (3, 3):
            Kd = torch.stack([Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]])
        Kd = Kd.reshape(-1, 4)
        if Kd.shape[0] == 1 and B > 1:
            Kd = Kd.expand(B, 4)
        Kd = Kd.contiguous()
        if B == 0 or td.shape[0] != B or Kd.shape[0] != B:
            raise ValueError("R, t and K disagree on the batch size")
        counts = torch.as_tensor(counts, device=dev).to(torch.int32).contiguous()
        xy = torch.as_tensor(xy, device=dev).to(torch.int32).contiguous()
        if counts.shape != (B,) or xy.dim() != 3 or xy.shape[0] != B or xy.shape[2] != 2 or xy.shape[1] < 1:
            raise ValueError("counts must be [B] and xy [B, cap, 2]")
        cap = int(xy.shape[1])
        H, W = self.height, self.width
        with torch.cuda.device(dev):
            st = L.stream_ptr(dev)
            ws_r, ws_s, depth = self._buffers(B, st, dev)
            # SRT3D's pixel centres sit at integers (renderer.cpp:115-118), zp_render's at half-integers
            Kr = Kd + torch.tensor([0.0, 0.0, 0.5, 0.5], dtype=torch.float64, device=dev)
            pose = [(Rd, td), (torch.empty_like(Rd), torch.empty_like(td)), (torch.empty_like(Rd), torch.empty_like(td))]
            cost = torch.empty((self.iterations, B), dtype=torch.int64, device=dev)
            stat = torch.empty((self.iterations, B), dtype=torch.int32, device=dev)
            cur = 0
            for it in range(self.iterations):
                nxt = 1 if cur != 1 else 2  # ping-pong between the two scratch poses; the input is kept
                Rc, tc = pose[cur]
                Rn, tn = pose[nxt]
                L.call("zp_render", B, r.vertices.data_ptr(), r.nv, r.faces.data_ptr(), r.nf, None, Rc.data_ptr(),
                       tc.data_ptr(), Kr.data_ptr(), H, W, float(z_near), None, depth.data_ptr(), None, None,
                       ws_r.data_ptr(), st)
                L.call("zp_edge_refine_step", B, H, W, depth.data_ptr(), counts.data_ptr(), xy.data_ptr(), cap,
                       Rc.data_ptr(), tc.data_ptr(), Kd.data_ptr(), self.lambda_rot, self.lambda_trans,
                       Rn.data_ptr(), tn.data_ptr(), cost[it].data_ptr(), stat[it].data_ptr(), None, None, 0, None,
                       None, ws_s.data_ptr(), st)
                cur = nxt
            # the first status other than 0, and the input pose where there is one (the reference's
            # early return leaves R and t untouched)
            bad = stat != 0
            first = torch.argmax(bad.to(torch.uint8), dim=0)
            status = torch.gather(stat, 0, first[None].to(torch.int64))[0]
            keep = (status != 0)[:, None]
            R_out = torch.where(keep, Rd, pose[cur][0]).reshape(B, 3, 3)
            t_out = torch.where(keep, td, pose[cur][1])
        return R_out, t_out, status, cost


_RENDERERS = {}  # (path, device) -> MeshRenderer


def py_edge_refine(R, t, fx, fy, cx, cy, width, height, contour, ply_path, save_dir=None, device="cuda"):
    """The reference's ``py_edge_refine`` (edge_refine/examples/edge_refine.cpp:185-200; test.py:309):
    R [3, 3], t [3] in metres, ``contour`` [N, 2] = (x, y) image pixels, ``ply_path`` a model in
    millimetres (the reference scales it by 0.001).  ``save_dir`` is ignored: no debug images are
    written.  One renderer is kept per path.  Returns (R f32 [3, 3], t f32 [3] in metres), the
    reference's types; the iteration itself is f64."""
    unit = 0.001
    key = (str(ply_path), str(device))
    rend = _RENDERERS.get(key)
    if rend is None:
        ply = read_ply(ply_path)
        rend = _RENDERERS[key] = MeshRenderer(ply["vertices"], ply["faces"], device=device)
    pts = np.asarray(contour, dtype=np.float64).reshape(-1, 2).astype(np.int32)  # the reference reads them as int
    xy = torch.from_numpy(np.ascontiguousarray(pts[None] if len(pts) else np.zeros((1, 1, 2), np.int32)))
    counts = torch.tensor([len(pts)], dtype=torch.int32)
    ref = EdgeRefiner(rend, height, width, unit=unit)
    t_mm = np.asarray(t, dtype=np.float64).reshape(1, 3) / unit
    Ro, to, _, _ = ref.refine(np.asarray(R, dtype=np.float64).reshape(1, 9), t_mm,
                              np.array([[fx, fy, cx, cy]], dtype=np.float64), counts, xy)
    return Ro[0].cpu().numpy().astype(np.float32), (to[0].cpu().numpy() * unit).astype(np.float32)
