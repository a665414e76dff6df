"""Whole synthetic training samples on the device: a shaded render of the object over a background,
its GT code image, masks and box, in the form ``CropPipeline.train_batch`` takes.

The reference makes such frames on the host: lib/meshrenderer/meshrenderer_phong.py renders the
object (``render(random_light=True)``) and GDR_Net_Augmentation.py:78-153 (``get_bg_image``,
``replace_bg``) pastes it over a random background, optionally truncating the foreground.  Here
``MeshRenderer.render_shaded`` (zp_render_shaded) draws, ``zp_mask_bbox`` / ``zp_composite``
(csrc/zp_shade.hip) paste; only the random draws and the integer geometry of the background stay
on the host.  The exact semantics are in include/zp.h and, as numpy, in tests/synth_ref.py.

``SceneBatcher`` makes frames of whole scenes, several objects hiding one another, which the
reference takes from BlenderProc (the ``pbr`` training sets): ``scene_compose`` (zp_scene_compose,
csrc/zp_scene.hip; as numpy in tests/scene_ref.py) composes the per-instance renders into the
frame and every instance's exact visible mask, counts and box.
"""
from __future__ import annotations

import numpy as np


def bg_geometry(bg_h, bg_w, H, W):
    """The integer geometry of get_bg_image (:78-115) and resize_short_edge (:37-57) for a bg_h x
    bg_w background and an H x W image -> (crop_w, crop_h, out_w, out_h, f).

    The background's top-left crop takes the image's aspect: a tall or square background
    (bg_h >= bg_w) keeps ceil(bg_w * H / W) rows, a wide one ceil(bg_h / (H / W)) columns, never more
    than it has (both aspect branches of get_bg_image come to this: where they differ, numpy's
    slice clamps).  The crop's short side is scaled to min(H, W) by f; if round(f * long side) >
    max(H, W), f = max(H, W) / long side instead.  The output size is cv2.resize's dsize for
    fx = fy = f: rint(size * f), half to even.  It may exceed the image by a row or column, which
    zp_composite drops."""
    bg_h, bg_w, H, W = int(bg_h), int(bg_w), int(H), int(W)
    if min(bg_h, bg_w, H, W) < 1:
        raise ValueError("sizes must be >= 1")
    target_size, max_size = min(H, W), max(H, W)
    real_hw_ratio = float(H) / float(W)
    crop_h, crop_w = bg_h, bg_w
    if bg_h >= bg_w:
        crop_h = min(int(np.ceil(bg_w * real_hw_ratio)), bg_h)
    else:
        crop_w = min(int(np.ceil(bg_h / real_hw_ratio)), bg_w)
    size_min, size_max = min(crop_h, crop_w), max(crop_h, crop_w)
    f = float(target_size) / float(size_min)
    if np.round(f * size_max) > max_size:
        f = float(max_size) / float(size_max)
    out_w, out_h = int(np.rint(crop_w * f)), int(np.rint(crop_h * f))
    if out_w < 1 or out_h < 1:
        raise ValueError(f"background {bg_h} x {bg_w} resizes to nothing for a {H} x {W} image")
    return crop_w, crop_h, out_w, out_h, f


def mask_bbox(masks):
    """masks u8 [B, H, W] (device) -> i32 [B, 4] (device) = (r1, c1, r2, c2), inclusive; (0, 0, -1, -1)
    for an empty mask (zp_mask_bbox)."""
    import torch
    from . import _lib as L
    if not (isinstance(masks, torch.Tensor) and masks.dtype == torch.uint8 and masks.is_cuda and masks.dim() == 3):
        raise ValueError("masks: expected a uint8 CUDA tensor [B, H, W]")
    masks = masks.contiguous()
    B, H, W = masks.shape
    with torch.cuda.device(masks.device):
        out = torch.empty((B, 4), dtype=torch.int32, device=masks.device)
        L.call("zp_mask_bbox", masks.data_ptr(), B, H, W, out.data_ptr(), L.stream_ptr(masks.device))
    return out


def composite(fg, masks, backgrounds, bg_index, trunc, bbox=None):
    """replace_bg for a batch (zp_composite): fg u8 [B, H, W, 3] and masks u8 [B, H, W] (device),
    backgrounds u8 [n_bg, Hb, Wb, 3] (device), bg_index int [B], trunc f64 [B, 2] = (rnd, u) with
    rnd < 0 for no truncation.  Returns (images u8 [B, H, W, 3], truncated masks u8 [B, H, W])."""
    import torch
    from . import _lib as L
    dev = fg.device
    for name, a, nd in (("fg", fg, 4), ("masks", masks, 3), ("backgrounds", backgrounds, 4)):
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.uint8 and a.is_cuda and a.dim() == nd):
            raise ValueError(f"{name}: expected a uint8 CUDA tensor with {nd} dims")
    fg, masks, backgrounds = fg.contiguous(), masks.contiguous(), backgrounds.contiguous()
    B, H, W, C = fg.shape
    n_bg, Hb, Wb, Cb = backgrounds.shape
    if C != 3 or Cb != 3 or tuple(masks.shape) != (B, H, W):
        raise ValueError("fg [B, H, W, 3], masks [B, H, W] and backgrounds [n_bg, Hb, Wb, 3] are needed")
    idx = np.asarray(bg_index, dtype=np.int64).reshape(-1)
    tr = np.ascontiguousarray(np.asarray(trunc, dtype=np.float64).reshape(-1, 2))
    if len(idx) != B or len(tr) != B or idx.min() < 0 or idx.max() >= n_bg:
        raise ValueError("bg_index / trunc: one in-range entry per sample is needed")
    cw, ch, ow, oh, f = bg_geometry(Hb, Wb, H, W)
    with torch.cuda.device(dev):
        if bbox is None:
            bbox = mask_bbox(masks)
        ints = torch.from_numpy(np.concatenate([idx.astype(np.int32), np.tile(np.array([cw, ch, ow, oh], np.int32), B)])).to(dev)
        reals = torch.from_numpy(np.concatenate([np.full(B, f, np.float64), tr.ravel()])).to(dev)
        out = torch.empty_like(fg)
        mo = torch.empty_like(masks)
        L.call("zp_composite", fg.data_ptr(), masks.data_ptr(), bbox.data_ptr(), B, H, W, backgrounds.data_ptr(), n_bg,
               Hb, Wb, ints[:B].data_ptr(), ints[B:].data_ptr(), reals[:B].data_ptr(), reals[B:].data_ptr(),
               out.data_ptr(), mo.data_ptr(), L.stream_ptr(dev))
    return out, mo


class SyntheticBatcher:
    """Synthetic training batches of one object.

    renderer_shaded: a ``MeshRenderer`` with per-vertex colours and normals (the textured model);
    renderer_codes: one whose face colours spell the surface codes (``models_GT_color``, or
    ``MeshRenderer.from_class_ids``); it may be the same object.  backgrounds: u8 [n_bg, Hb, Wb, 3],
    B, G, R (host array or device tensor), uploaded once.  phong: the (ambient, diffuse, specular)
    weights the jitter is applied to; random_light / truncate_fg as the reference's switches."""

    def __init__(self, renderer_shaded, renderer_codes, backgrounds, phong=(0.4, 0.8, 0.3), random_light=True,
                 truncate_fg=True, rng: np.random.Generator | None = None):
        import torch
        self.rs, self.rc = renderer_shaded, renderer_codes
        if not isinstance(backgrounds, torch.Tensor):
            backgrounds = torch.from_numpy(np.ascontiguousarray(np.asarray(backgrounds, dtype=np.uint8)))
        if backgrounds.dim() != 4 or backgrounds.shape[3] != 3 or backgrounds.dtype != torch.uint8 or backgrounds.shape[0] < 1:
            raise ValueError("backgrounds must be u8 [n_bg, Hb, Wb, 3]")
        self.backgrounds = backgrounds.to(self.rs.device).contiguous()
        self.phong = tuple(float(p) for p in phong)
        self.random_light, self.truncate_fg = bool(random_light), bool(truncate_fg)
        self.rng = rng if rng is not None else np.random.default_rng()

    def sample(self, B):
        """The host draws of B samples: dict(light f64 [B, 3], phong f64 [B, 3], bg_index i64 [B],
        trunc f64 [B, 2]).  Light and weights as meshrenderer_phong.py ``render(random_light=True)``
        (:153-157): position 1000 * random(3) in GL's eye frame, i.e. (x, y, -z) in camera
        coordinates; diffuse and specular + 0.1 * (2 * rand - 1).  bg_index and (rnd, u) as
        replace_bg's randint, random and uniform."""
        from .render import DEFAULT_LIGHT
        r = self.rng
        light = np.tile(np.asarray(DEFAULT_LIGHT, np.float64), (B, 1))
        phong = np.tile(np.asarray(self.phong, np.float64), (B, 1))
        bg_index = np.zeros(B, np.int64)
        trunc = np.full((B, 2), -1.0)
        for b in range(B):
            if self.random_light:
                light[b] = 1000.0 * r.random(3) * np.array([1.0, 1.0, -1.0])
                phong[b, 1] += 0.1 * (2 * r.random() - 1)
                phong[b, 2] += 0.1 * (2 * r.random() - 1)
            bg_index[b] = r.integers(0, len(self.backgrounds))
            if self.truncate_fg:
                trunc[b] = (r.random(), r.random())
        return {"light": light, "phong": phong, "bg_index": bg_index, "trunc": trunc}

    def __call__(self, R, t, K, height, width, draws=None, z_near=1e-6):
        """R [B, 3, 3], t [B, 3], K as ``MeshRenderer.render``; draws: ``sample``'s dict (drawn here when
        None).  Returns a dict of ``train_batch``'s arguments -- images u8 [B, H, W, 3] (the
        composite), gt_images u8 [B, H, W, 3] (the code colours at the same poses), entire_masks
        (the render's mask) and masks (the truncated mask) u8 [B, H, W], all on the device, img_index
        = arange(B), raw_boxes int64 [B, 4] = the truncated mask's box as x, y, w, h (host: the box
        arithmetic of train_batch is host code; 16 bytes per sample are copied back) -- plus ``draws``."""
        B = len(np.asarray(R, dtype=np.float64).reshape(-1, 9))
        if draws is None:
            draws = self.sample(B)
        if self.rc is self.rs:
            o = self.rs.render_shaded(R, t, K, height, width, light=draws["light"], phong=draws["phong"], z_near=z_near,
                                      outputs=("shaded", "color", "mask"))
            gt = o["color"]
        else:
            o = self.rs.render_shaded(R, t, K, height, width, light=draws["light"], phong=draws["phong"], z_near=z_near,
                                      outputs=("shaded", "mask"))
            gt = self.rc.render(R, t, K, height, width, z_near=z_near, outputs=("color",))["color"]
        images, masks = composite(o["shaded"], o["mask"], self.backgrounds, draws["bg_index"], draws["trunc"])
        bb = mask_bbox(masks).cpu().numpy().astype(np.int64)
        raw_boxes = np.stack([bb[:, 1], bb[:, 0], bb[:, 3] - bb[:, 1] + 1, bb[:, 2] - bb[:, 0] + 1], axis=1)
        return {"images": images, "img_index": np.arange(B), "raw_boxes": raw_boxes, "gt_images": gt, "masks": masks,
                "entire_masks": o["mask"], "draws": draws}


SCENE_OUTPUTS = ("image", "fg", "scene", "instance", "mask_visib", "info")


def _xywh(rc):
    """(r1, c1, r2, c2) inclusive, int [B, 4] -> (x, y, w, h) int64; the empty box (0, 0, -1, -1) -> zeros."""
    rc = np.asarray(rc, dtype=np.int64)
    return np.stack([rc[:, 1], rc[:, 0], rc[:, 3] - rc[:, 1] + 1, rc[:, 2] - rc[:, 0] + 1], axis=1)


def scene_compose(depth, img_index, n_img, shaded=None, outputs=None):
    """Whole scenes from per-instance renders (zp_scene_compose, include/zp.h).
    depth f32 [B, H, W] on the device (0 = no surface), as ``MeshRenderer`` renders each instance
    alone; img_index int [B], host or device: the image of each instance, in any order; an index
    outside [0, n_img) belongs to no image (empty visible mask, px_count_visib 0).  shaded u8
    [B, H, W, 3] on the device, needed for ``image``.  outputs: a subset of SCENE_OUTPUTS; None: all
    of them (``image`` only with ``shaded``).

    Returns a dict of device tensors: image u8 [n_img, H, W, 3] (the nearest instance's shaded pixel,
    0 for background), fg u8 [n_img, H, W] (255 / 0), scene f32 and instance i32 [n_img, H, W] (as
    ``gtinfo.scene_depth``), mask_visib u8 [B, H, W] (255 exactly where the instance is the one
    shown: exact occupancy, not ``gtinfo.gt_info``'s delta test), info i32 [B, 6] = (px_all,
    px_visib, r1, c1, r2, c2).  With ``info`` also, on the host (one copy of 24 bytes per instance):
    bbox_visib int64 [B, 4] = (x, y, w, h) with inclusive sizes, zeros when nothing is visible;
    px_count_all (the in-frame count: the renders are the image's size), px_count_visib int64 [B];
    visib_fract f64 [B] = px_visib / px_all, 0 where px_all is 0."""
    import torch
    from . import _lib as L
    from .gtinfo import _f32_stack, _index, _need_device, _same_device
    if outputs is None:
        outputs = tuple(o for o in SCENE_OUTPUTS if o != "image" or shaded is not None)
    outputs = tuple(outputs)
    if not outputs or any(o not in SCENE_OUTPUTS for o in outputs):
        raise ValueError(f"outputs must be a non-empty subset of {SCENE_OUTPUTS}")
    if "image" in outputs and shaded is None:
        raise ValueError("image needs shaded")
    d = _f32_stack(depth, "depth")
    B, H, W = d.shape
    n_img = int(n_img)
    if n_img < 1 or n_img > 65535 or B > 65535 or H > 32768 or W > 32768 or max(B, n_img) * H * W >= 2 ** 31 - 1024:
        raise ValueError(f"sizes out of range: B {B}, n_img {n_img}, {H} x {W}")
    if len(img_index) != B:
        raise ValueError(f"img_index: expected {B} integers")
    if shaded is not None:
        if not (isinstance(shaded, torch.Tensor) and shaded.dtype == torch.uint8 and tuple(shaded.shape) == (B, H, W, 3)):
            raise ValueError(f"shaded: expected a uint8 device tensor [{B}, {H}, {W}, 3]")
        shaded = shaded.contiguous()
    _need_device(d, "depth")
    if shaded is not None:
        _need_device(shaded, "shaded")
        if not _same_device(shaded.device, d.device):
            raise ValueError("depth and shaded are on different devices")
    dev = d.device
    shapes = {"image": ((n_img, H, W, 3), torch.uint8), "fg": ((n_img, H, W), torch.uint8),
              "scene": ((n_img, H, W), torch.float32), "instance": ((n_img, H, W), torch.int32),
              "mask_visib": ((B, H, W), torch.uint8), "info": ((B, 6), torch.int32)}
    with torch.cuda.device(dev):
        ii = _index(img_index, B, "img_index", dev)
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in SCENE_OUTPUTS if k in outputs}
        ws = None
        if "info" in outputs:
            ws = torch.empty(L.lib.zp_scene_compose_ws_bytes(B, n_img, H, W), dtype=torch.uint8, device=dev)
        L.call("zp_scene_compose", B, n_img, H, W, d.data_ptr(), L.ptr(shaded if "image" in outputs else None),
               ii.data_ptr(), *(L.ptr(out.get(k)) for k in SCENE_OUTPUTS), L.ptr(ws), L.stream_ptr(dev))
        if "info" in outputs:
            h = out["info"].cpu().numpy().astype(np.int64)
            out.update(bbox_visib=_xywh(h[:, 2:]), px_count_all=h[:, 0], px_count_visib=h[:, 1],
                       visib_fract=np.where(h[:, 0] > 0, h[:, 1] / np.maximum(h[:, 0], 1), 0.0))
    return out


class SceneBatcher:
    """Synthetic training frames of whole scenes: several objects per image, the nearer hiding the
    farther, over a background; every instance with its GT code image, its exact visible mask and
    its entire mask, in the form ``CropPipeline.train_batch(..., gt_index=...)`` takes.  The
    reference trains on such frames from BlenderProc (the ``pbr`` sets), made outside it.

    renderers_shaded / renderers_codes: obj_id -> ``MeshRenderer`` as ``SyntheticBatcher``'s two
    renderers, all on one device; renderers_codes[k] may be the same object as renderers_shaded[k].
    backgrounds, phong, random_light as ``SyntheticBatcher``.  There is no foreground truncation:
    occlusion takes its place."""

    def __init__(self, renderers_shaded, renderers_codes, backgrounds, phong=(0.4, 0.8, 0.3), random_light=True,
                 rng: np.random.Generator | None = None):
        import torch
        from .gtinfo import _same_device
        self.rs, self.rc = dict(renderers_shaded), dict(renderers_codes)
        if not self.rs:
            raise ValueError("no renderers")
        if set(self.rs) != set(self.rc):
            raise ValueError("renderers_shaded and renderers_codes must have the same obj_ids")
        devs = [r.device for r in list(self.rs.values()) + list(self.rc.values())]
        if not all(d == devs[0] or (d.type == devs[0].type == "cuda" and _same_device(d, devs[0])) for d in devs):
            raise ValueError("the renderers are on different devices")
        self.device = devs[0]
        if not isinstance(backgrounds, torch.Tensor):
            backgrounds = torch.from_numpy(np.ascontiguousarray(np.asarray(backgrounds, dtype=np.uint8)))
        if backgrounds.dim() != 4 or backgrounds.shape[3] != 3 or backgrounds.dtype != torch.uint8 or backgrounds.shape[0] < 1:
            raise ValueError("backgrounds must be u8 [n_bg, Hb, Wb, 3]")
        self.backgrounds = backgrounds.to(self.device).contiguous()
        self.phong = tuple(float(p) for p in phong)
        if len(self.phong) != 3:
            raise ValueError("phong: (ambient, diffuse, specular)")
        self.random_light = bool(random_light)
        self.rng = rng if rng is not None else np.random.default_rng()

    def sample(self, n_img):
        """The host draws of n_img images: dict(light f64 [n_img, 3], phong f64 [n_img, 3], bg_index i64
        [n_img]) by ``SyntheticBatcher.sample``'s formulas, in its order: one light, one Phong jitter
        and one background per IMAGE, so every object of a frame is lit alike."""
        from .render import DEFAULT_LIGHT
        n_img = int(n_img)
        if n_img < 1:
            raise ValueError("n_img must be >= 1")
        r = self.rng
        light = np.tile(np.asarray(DEFAULT_LIGHT, np.float64), (n_img, 1))
        phong = np.tile(np.asarray(self.phong, np.float64), (n_img, 1))
        bg_index = np.zeros(n_img, np.int64)
        for i in range(n_img):
            if self.random_light:
                light[i] = 1000.0 * r.random(3) * np.array([1.0, 1.0, -1.0])
                phong[i, 1] += 0.1 * (2 * r.random() - 1)
                phong[i, 2] += 0.1 * (2 * r.random() - 1)
            bg_index[i] = r.integers(0, len(self.backgrounds))
        return {"light": light, "phong": phong, "bg_index": bg_index}

    def __call__(self, obj_ids, img_index, R, t, K, height, width, targets=None, draws=None, min_visib_fract=0.0,
                 z_near=1e-6):
        """B instances spread over the images of a batch.  obj_ids int [B] (keys of the renderers),
        img_index int [B] (non-negative; the image of each instance), R [B, 3, 3], t [B, 3], K as
        ``MeshRenderer.render`` (one for all or one per instance), all on the host.  draws:
        ``sample``'s dict, which fixes the number of images (drawn here for max(img_index) + 1 images
        when None).  targets: indices into the instances whose labels are wanted (None: all); the
        others only occlude.  A target with no visible pixel or with visib_fract < min_visib_fract is
        dropped.

        Instances are grouped by object; each group is drawn by ``render_shaded`` at height x width
        with its image's light, the scene is composed by ``scene_compose`` and pasted over the
        images' backgrounds by ``composite`` (no truncation), and the code colours of the targets
        that remain are rendered (or taken from the same pass when the code renderer is the shaded
        one).  The per-instance buffers (depth, shaded, mask) take 8 bytes per pixel and instance
        and are not chunked: more than ``gtinfo.MAX_RENDER_BYTES`` (256 MiB; 109 instances at 480 x
        640) is a ValueError naming the largest B that fits.

        Returns ``train_batch``'s arguments for the T targets kept -- images u8 [n_img, H, W, 3],
        img_index int64 [T], gt_index = arange(T), raw_boxes int64 [T, 4] (bbox_visib as x, y, w, h),
        gt_images u8 [T, H, W, 3], masks u8 [T, H, W] (the exact visible masks), entire_masks u8
        [T, H, W] (each instance's own render mask) -- plus visib_fract f64 [T] (of the in-frame
        pixels), kept int64 [T] (indices into the instances), instance i32 [n_img, H, W] (device, -1 =
        background) and ``draws``."""
        import torch
        from .gtinfo import MAX_RENDER_BYTES
        ids = np.asarray(obj_ids).reshape(-1)
        B = len(ids)
        if B == 0:
            raise ValueError("no instances")
        missing = sorted(set(ids.tolist()) - set(self.rs))
        if missing:
            raise ValueError(f"no renderer for obj_id {missing}")
        ii = np.asarray(img_index)
        if ii.shape != (B,) or not np.issubdtype(ii.dtype, np.integer) or ii.min() < 0:
            raise ValueError("img_index needs one non-negative integer per instance")
        ii = ii.astype(np.int64)
        Rn = np.asarray(R, dtype=np.float64).reshape(-1, 9)
        tn = np.asarray(t, dtype=np.float64).reshape(-1, 3)
        if len(Rn) != B or len(tn) != B:
            raise ValueError("obj_ids, R and t disagree on the batch size")
        Kn = np.asarray(K, dtype=np.float64)
        if Kn.shape == (3, 3):
            Kn = np.array([Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]])
        Kn = Kn.reshape(-1, 4)
        if len(Kn) == 1 and B > 1:
            Kn = np.repeat(Kn, B, axis=0)
        if len(Kn) != B:
            raise ValueError(f"K has {len(Kn)} rows for a batch of {B}")
        H, W = int(height), int(width)
        if H < 1 or W < 1:
            raise ValueError("empty image")
        if targets is None:
            tg = np.arange(B)
        else:
            tg = np.asarray(targets)
            if tg.ndim != 1 or (len(tg) and not np.issubdtype(tg.dtype, np.integer)):
                raise ValueError("targets: expected a 1-D integer index array")
            tg = tg.astype(np.int64)
            if len(tg) and (tg.min() < 0 or tg.max() >= B or len(np.unique(tg)) != len(tg)):
                raise ValueError("targets: distinct indices into the instances are needed")
        if not 0.0 <= float(min_visib_fract) <= 1.0:
            raise ValueError("min_visib_fract must lie in [0, 1]")
        if draws is None:
            draws = self.sample(int(ii.max()) + 1)
        n_img = len(draws["bg_index"])
        if len(draws["light"]) != n_img or len(draws["phong"]) != n_img:
            raise ValueError("draws: light, phong and bg_index disagree on the number of images")
        if ii.max() >= n_img:
            raise ValueError(f"img_index names an image beyond the {n_img} of draws")
        if B * H * W * 8 > MAX_RENDER_BYTES:
            raise ValueError(f"{B} instances at {H} x {W} need {B * H * W * 8} bytes of per-instance buffers; at most "
                             f"{MAX_RENDER_BYTES // (8 * H * W)} fit in {MAX_RENDER_BYTES}")
        dev = self.device
        is_target = np.zeros(B, bool)
        is_target[tg] = True
        groups = [(oid, np.flatnonzero(ids == oid)) for oid in sorted(set(ids.tolist()))]
        with torch.cuda.device(dev):
            whole = len(groups) == 1  # one object: the render is the stack, no reordering
            depth = shaded = mask = None
            if not whole:
                depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
                shaded = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
                mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
            colors = {}  # obj_id -> (group indices, code colours of the whole group), when both renderers are one
            for oid, idx in groups:
                same = self.rc[oid] is self.rs[oid] and is_target[idx].any()
                o = self.rs[oid].render_shaded(Rn[idx], tn[idx], Kn[idx], H, W, light=draws["light"][ii[idx]],
                                               phong=draws["phong"][ii[idx]], z_near=z_near,
                                               outputs=("shaded", "depth", "mask") + (("color",) if same else ()))
                if same:
                    colors[oid] = o["color"]
                if whole:
                    depth, shaded, mask = o["depth"], o["shaded"], o["mask"]
                else:
                    sel = torch.from_numpy(idx).to(dev)
                    depth[sel], shaded[sel], mask[sel] = o["depth"], o["shaded"], o["mask"]
            sc = scene_compose(depth, ii, n_img, shaded=shaded, outputs=("image", "fg", "instance", "mask_visib", "info"))
            images, _ = composite(sc["image"], sc["fg"], self.backgrounds, draws["bg_index"], np.full((n_img, 2), -1.0))
            fract = sc["visib_fract"]
            kept = tg[(sc["px_count_visib"][tg] > 0) & (fract[tg] >= float(min_visib_fract))]
            T = len(kept)
            gt = torch.zeros((T, H, W, 3), dtype=torch.uint8, device=dev)
            for oid, idx in groups:
                pos = np.flatnonzero(ids[kept] == oid)  # places in the output
                if len(pos) == 0:
                    continue
                k = kept[pos]
                if oid in colors:
                    src = colors[oid][torch.from_numpy(np.searchsorted(idx, k)).to(dev)]
                else:
                    src = self.rc[oid].render(Rn[k], tn[k], Kn[k], H, W, z_near=z_near, outputs=("color",))["color"]
                gt[torch.from_numpy(pos).to(dev)] = src
            ksel = torch.from_numpy(kept).to(dev)
            masks, entire = sc["mask_visib"][ksel], mask[ksel]
        return {"images": images, "img_index": ii[kept], "gt_index": np.arange(T), "raw_boxes": sc["bbox_visib"][kept],
                "gt_images": gt, "masks": masks, "entire_masks": entire, "visib_fract": fract[kept], "kept": kept,
                "instance": sc["instance"], "draws": draws}
