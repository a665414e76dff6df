"""Visible masks and ``scene_gt_info.json`` on the device (``zp_scene_depth``, ``zp_gt_info``;
csrc/zp_gtinfo.hip).

The reference's loader reads, beside the GT code images, every instance's visible mask
(``mask_visib/*.png``) and ``scene_gt_info.json``: ``bbox_visib`` is the box each crop is cut from
(bop_dataset_pytorch.py:249, 411) and ``visib_fract`` selects the instances of a training set
(tools_for_BOP/bop_io.py:71-72, 269-270).  In a BOP dataset these come from the BOP toolkit's
calc_gt_masks.py / calc_gt_info.py (an OpenGL renderer plus numpy).  Here they are made from
``MeshRenderer``'s depth: ``scene_depth`` composes a synthetic scene from per-instance renders,
``gt_info`` applies the visibility test of lib/pysixd/visibility.py and counts, and
``SceneLabeler`` drives both from poses.  The exact semantics are in include/zp.h and, as numpy, in
tests/gtinfo_ref.py.  Deviations from the toolkit: the depth is this rasteriser's, not OpenGL's;
the toolkit itself is not part of the reference, so for px_count_all, the large render and the
empty-box rule include/zp.h is the specification.
"""
from __future__ import annotations

import numpy as np

VISIB_MODES = {"bop19": 0, "bop18": 1}
INFO_FIELDS = ("px_count_all", "px_count_valid", "px_count_visib", "obj_x0", "obj_y0", "obj_x1", "obj_y1",
               "vis_x0", "vis_y0", "vis_x1", "vis_y1")
# SceneLabeler: instances rendered at once, so that the 3 H x 3 W depth buffer stays within this
MAX_RENDER_BYTES = 256 << 20


def _f32_stack(t, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 3):
        raise ValueError(f"{name}: expected a float32 device tensor [n, H, W]")
    if t.shape[0] < 1 or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"{name}: empty")
    return t.contiguous()


def _need_device(t, name):
    """Checked after the shapes, so that a shape is refused the same way with or without a GPU."""
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor, got one on {t.device}")


def _same_device(a, b):
    import torch
    cur = torch.cuda.current_device() if a.index is None or b.index is None else 0
    return a.type == b.type and (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


def _index(idx, n, name, dev):
    """int [n], host or device, any integer dtype -> i32 [n] on the device."""
    import torch
    if isinstance(idx, torch.Tensor):
        if idx.dtype not in (torch.int32, torch.int64) or idx.dim() != 1 or len(idx) != n:
            raise ValueError(f"{name}: expected {n} integers")
        return idx.to(device=dev, dtype=torch.int32).contiguous()
    a = np.asarray(idx)
    if a.ndim != 1 or len(a) != n or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: expected {n} integers")
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)


def _k4_host(K, B):
    """One 3 x 3 camera matrix, one (fx, fy, cx, cy) row, or B of either -> f64 [B, 4] (host)."""
    import torch
    k = np.asarray(K.cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    if k.shape[-2:] == (3, 3):
        k = np.stack([k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2]], axis=-1)
    k = k.reshape(-1, 4)
    if len(k) == 1 and B > 1:
        k = np.repeat(k, B, axis=0)
    if len(k) != B:
        raise ValueError(f"K has {len(k)} rows for a batch of {B}")
    return np.ascontiguousarray(k)


def scene_depth(depth, img_index, n_img, return_instance=True):
    """The depth image of each of ``n_img`` scenes from its instances' renders (zp_scene_depth).
    depth f32 [B, H, W] on the device (0 = no surface); img_index int [B]: the image of each instance,
    in any order; an index outside [0, n_img) contributes nothing.  Returns (scene f32 [n_img, H, W] =
    the smallest positive depth, 0 where there is none; instance i32 [n_img, H, W] = the instance that
    supplied it, the lowest on a tie, -1 for background, or None without ``return_instance``)."""
    import torch
    from . import _lib as L
    d = _f32_stack(depth, "depth")
    B, H, W = d.shape
    n_img = int(n_img)
    if n_img < 1 or n_img > 65535 or B > 65535 or H * W >= 2 ** 31 - 1024:
        raise ValueError(f"sizes out of range: B {B}, n_img {n_img}, {H} x {W}")
    if len(img_index) != B:
        raise ValueError(f"img_index: expected {B} integers")
    _need_device(d, "depth")
    dev = d.device
    with torch.cuda.device(dev):
        ii = _index(img_index, B, "img_index", dev)
        scene = torch.empty((n_img, H, W), dtype=torch.float32, device=dev)
        inst = torch.empty((n_img, H, W), dtype=torch.int32, device=dev) if return_instance else None
        L.call("zp_scene_depth", B, d.data_ptr(), ii.data_ptr(), n_img, H, W, scene.data_ptr(), L.ptr(inst),
               L.stream_ptr(dev))
    return scene, inst


class GtInfo:
    """What ``gt_info`` returns: ``mask`` / ``mask_visib`` u8 [B, H, W] (255 / 0) and ``info`` i32
    [B, 11] (INFO_FIELDS) on the device; any of them None when it was not asked for.  The methods
    read ``info`` back to the host once."""

    def __init__(self, mask, mask_visib, info):
        self.mask, self.mask_visib, self.info = mask, mask_visib, info
        self._host = None

    def _info_host(self):
        if self.info is None:
            raise ValueError("gt_info ran without info")
        if self._host is None:
            self._host = self.info.cpu().numpy().astype(np.int64)
        return self._host

    def visib_fract(self):
        """f64 [B] on the device: px_count_visib / px_count_all, 0.0 where px_count_all == 0."""
        import torch
        if self.info is None:
            raise ValueError("gt_info ran without info")
        n_all, n_vis = self.info[:, 0].to(torch.float64), self.info[:, 2].to(torch.float64)
        return torch.where(n_all > 0, n_vis / n_all.clamp(min=1.0), torch.zeros_like(n_all))

    def bboxes(self, inclusive=False):
        """(bbox_obj, bbox_visib), host int64 [B, 4] = (x, y, w, h) in image coordinates.
        ``inclusive=False`` is the BOP toolkit's convention, w = x1 - x0 and h = y1 - y0, which the
        scene_gt_info.json files of the BOP datasets carry and the loader reads; ``inclusive=True``
        gives w = x1 - x0 + 1 as the reference's misc.calc_2d_bbox_xywh (misc.py:644-654).  As in the
        toolkit's calc_gt_info.py, BOTH boxes are (-1, -1, -1, -1) when px_count_visib == 0."""
        h = self._info_host()
        one = 1 if inclusive else 0
        out = []
        for c in (3, 7):
            x0, y0, x1, y1 = (h[:, c + k] for k in range(4))
            box = np.stack([x0, y0, x1 - x0 + one, y1 - y0 + one], axis=1)
            box[h[:, 2] == 0] = -1
            out.append(box)
        return out[0], out[1]

    def scene_gt_info(self):
        """One dict per instance with the keys of BOP's scene_gt_info.json (bbox_obj, bbox_visib,
        px_count_all, px_count_valid, px_count_visib, visib_fract), Python ints and floats."""
        h = self._info_host()
        obj, vis = self.bboxes()
        fract = self.visib_fract().cpu().numpy()
        return [{"bbox_obj": [int(v) for v in obj[b]], "bbox_visib": [int(v) for v in vis[b]],
                 "px_count_all": int(h[b, 0]), "px_count_valid": int(h[b, 1]), "px_count_visib": int(h[b, 2]),
                 "visib_fract": float(fract[b])} for b in range(len(h))]


def _run(dg, ox, oy, dt, ti, Kd, delta, mode, mask, mask_visib, info):
    from . import _lib as L
    B, Hg, Wg = dg.shape
    n_test, H, W = dt.shape
    L.call("zp_gt_info", B, dg.data_ptr(), Hg, Wg, ox, oy, H, W, dt.data_ptr(), n_test, L.ptr(ti), Kd.data_ptr(),
           float(delta), mode, L.ptr(mask), L.ptr(mask_visib), L.ptr(info), L.stream_ptr(dg.device))


def gt_info(depth_gt, depth_test, K, window=None, test_index=None, delta=15.0, visib_mode="bop19",
            outputs=("mask", "mask_visib", "info")):
    """Masks, pixel counts and boxes of B instances (zp_gt_info).
    depth_gt f32 [B, Hg, Wg] on the device: each instance rendered alone.  depth_test f32
    [n_test, H, W] on the device: the scene's depth, measured or from ``scene_depth``; its size is
    the image's.  ``window`` = (ox, oy): where the image lies in depth_gt (the rest of depth_gt is the
    object outside the frame); None: depth_gt is the image, Hg x Wg = H x W.  K: the IMAGE's
    intrinsics, one 3 x 3 matrix or (fx, fy, cx, cy) row for all or B of them.  ``test_index`` int [B]
    names each instance's scene image (default: image b, or image 0 when there is one).  ``delta``
    in the unit of the depth images; ``visib_mode`` 'bop19' (an instance is visible where the scene
    has no depth) or 'bop18' (it is not).  Returns a GtInfo."""
    import torch
    if visib_mode not in VISIB_MODES:
        raise ValueError(f"visib_mode must be one of {sorted(VISIB_MODES)}")
    outputs = tuple(outputs)
    if not outputs or any(o not in ("mask", "mask_visib", "info") for o in outputs):
        raise ValueError("outputs must be a non-empty subset of ('mask', 'mask_visib', 'info')")
    dg = _f32_stack(depth_gt, "depth_gt")
    dt = _f32_stack(depth_test, "depth_test")
    B, Hg, Wg = dg.shape
    n_test, H, W = dt.shape
    if window is None:
        if (Hg, Wg) != (H, W):
            raise ValueError(f"depth_gt is {Hg} x {Wg} and the image {H} x {W}: give the window's origin")
        ox = oy = 0
    else:
        ox, oy = (int(v) for v in window)
    if ox < 0 or oy < 0 or ox + W > Wg or oy + H > Hg:
        raise ValueError(f"the {H} x {W} window at ({ox}, {oy}) leaves the {Hg} x {Wg} render")
    if B > 65535 or Hg * Wg >= 2 ** 31 - 1024:
        raise ValueError(f"sizes out of range: B {B}, {Hg} x {Wg}")
    if not np.isfinite(delta):
        raise ValueError("delta must be finite")
    if test_index is not None and len(test_index) != B:
        raise ValueError(f"test_index: expected {B} integers")
    if test_index is None and 1 < n_test < B:
        raise ValueError(f"{n_test} scene images for {B} instances: give test_index")
    _k4_host(K, B)
    _need_device(dg, "depth_gt")
    _need_device(dt, "depth_test")
    if not _same_device(dt.device, dg.device):
        raise ValueError("depth_gt and depth_test are on different devices")
    dev = dg.device
    with torch.cuda.device(dev):
        if test_index is None and n_test == 1 and B > 1:
            test_index = np.zeros(B, np.int32)
        ti = None
        if test_index is not None:
            ti = _index(test_index, B, "test_index", dev)
        Kd = torch.from_numpy(_k4_host(K, B)).to(dev)
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if "mask" in outputs else None
        visib = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if "mask_visib" in outputs else None
        info = torch.empty((B, len(INFO_FIELDS)), dtype=torch.int32, device=dev) if "info" in outputs else None
        _run(dg, ox, oy, dt, ti, Kd, delta, VISIB_MODES[visib_mode], mask, visib, info)
    return GtInfo(mask, visib, info)


class SceneLabeler:
    """GT masks and info of whole scenes from poses: ``renderers`` maps obj_id -> MeshRenderer (all
    on one device)."""

    def __init__(self, renderers):
        self.renderers = dict(renderers)
        if not self.renderers:
            raise ValueError("no renderers")
        devs = [r.device for r in self.renderers.values()]
        if not all(_same_device(d, devs[0]) for d in devs):
            raise ValueError("the renderers are on different devices")
        self.device = devs[0]

    def labels(self, obj_ids, img_index, R, t, K, height, width, depth_test=None, truncation=True, delta=15.0,
               visib_mode="bop19"):
        """Labels of B instances spread over the images of a batch.
        obj_ids int [B] (keys of ``renderers``), img_index int [B] (the image of each instance), R
        [B, 3, 3], t [B, 3], K as ``gt_info`` takes it (the image's intrinsics), all on the host.
        Instances are grouped by object and each group is rendered with MeshRenderer.render.

        truncation=True renders, as the BOP toolkit does, at 3 H x 3 W with the principal point moved
        by (W, H), so px_count_all and bbox_obj cover the part of an object outside the frame.  That
        depth buffer is bounded: a group is rendered in chunks of at most MAX_RENDER_BYTES (256 MiB)
        / (36 H W bytes) instances, 23 at 480 x 640.  truncation=False renders at H x W with a zero
        window origin; px_count_all is then the in-frame count (a deviation: visib_fract does not
        fall for an object that leaves the frame) and bbox_obj is clipped to the frame.

        depth_test: the measured depth f32 [n_img, H, W] on the device in the unit of the poses; None:
        the scene is composed from the instances' own in-frame renders with ``scene_depth``.  Each
        instance's test image is its img_index.  When depth_test is None and the batch needs more
        than one chunk, every chunk is rendered twice (once for the scene, once for its labels)
        so that memory stays bounded.

        Returns (GtInfo in the caller's instance order, scene f32 [n_img, H, W], instance i32
        [n_img, H, W] or None when depth_test was given).  mask / mask_visib are u8 255 / 0 stacks
        indexed by instance: CropPipeline takes them with img_index = arange(B)."""
        import torch
        if visib_mode not in VISIB_MODES:
            raise ValueError(f"visib_mode must be one of {sorted(VISIB_MODES)}")
        ids = np.asarray(obj_ids).reshape(-1)
        B = len(ids)
        if B == 0:
            raise ValueError("no instances")
        missing = sorted(set(ids.tolist()) - set(self.renderers))
        if missing:
            raise ValueError(f"no renderer for obj_id {missing}")
        ii = np.asarray(img_index)
        if ii.shape != (B,) or not np.issubdtype(ii.dtype, np.integer) or ii.min() < 0:
            raise ValueError("img_index needs one non-negative integer per instance")
        Rn = np.asarray(R, dtype=np.float64).reshape(-1, 9)
        tn = np.asarray(t, dtype=np.float64).reshape(-1, 3)
        if len(Rn) != B or len(tn) != B:
            raise ValueError("obj_ids, R and t disagree on the batch size")
        Kn = _k4_host(K, B)
        H, W = int(height), int(width)
        if H < 1 or W < 1:
            raise ValueError("empty image")
        dev = self.device
        if depth_test is not None:
            dt = _f32_stack(depth_test, "depth_test")
            _need_device(dt, "depth_test")
            if tuple(dt.shape[1:]) != (H, W) or not _same_device(dt.device, dev):
                raise ValueError(f"depth_test must be [n_img, {H}, {W}] on {dev}")
            n_img = dt.shape[0]
            if ii.max() >= n_img:
                raise ValueError("img_index names an image depth_test does not have")
        else:
            dt, n_img = None, int(ii.max()) + 1
        if truncation:
            Hg, Wg, ox, oy = 3 * H, 3 * W, W, H
        else:
            Hg, Wg, ox, oy = H, W, 0, 0
        Kr = Kn + np.array([0.0, 0.0, ox, oy])
        per = max(1, MAX_RENDER_BYTES // (4 * Hg * Wg))
        chunks = []  # (renderer, caller indices)
        for oid in sorted(set(ids.tolist())):
            idx = np.flatnonzero(ids == oid)
            chunks += [(self.renderers[oid], idx[j:j + per]) for j in range(0, len(idx), per)]

        def render(r, idx):
            return r.render(Rn[idx], tn[idx], Kr[idx], Hg, Wg, outputs=("depth",))["depth"]

        with torch.cuda.device(dev):
            kept = None
            instance = None
            if dt is None:
                win = torch.empty((B, H, W), dtype=torch.float32, device=dev)
                for r, idx in chunks:
                    d = render(r, idx)
                    win[torch.from_numpy(idx).to(dev)] = d[:, oy:oy + H, ox:ox + W]
                    if len(chunks) == 1:
                        kept = d
                dt, instance = scene_depth(win, ii, n_img)
                del win
            mode = VISIB_MODES[visib_mode]
            Kd = torch.from_numpy(Kn).to(dev)
            tid = torch.from_numpy(ii.astype(np.int32)).to(dev)
            mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
            visib = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
            info = torch.empty((B, len(INFO_FIELDS)), dtype=torch.int32, device=dev)
            for r, idx in chunks:
                d = kept if kept is not None else render(r, idx)
                n = len(idx)
                if n == B and np.array_equal(idx, np.arange(B)):  # one object, one chunk: no reordering
                    _run(d, ox, oy, dt, tid, Kd, delta, mode, mask, visib, info)
                    continue
                sel = torch.from_numpy(idx).to(dev)
                m = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
                v = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
                f = torch.empty((n, len(INFO_FIELDS)), dtype=torch.int32, device=dev)
                _run(d, ox, oy, dt, tid[sel].contiguous(), Kd[sel].contiguous(), delta, mode, m, v, f)
                mask[sel], visib[sel], info[sel] = m, v, f
        return GtInfo(mask, visib, info), dt, instance
