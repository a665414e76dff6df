"""Whole synthetic training samples on the device: a shaded render of the object over a background,
its GT code image, masks and box, in the form ``CropPipeline.train_batch`` takes.

The reference makes such frames on the host: lib/meshrenderer/meshrenderer_phong.py renders the
object (``render(random_light=True)``) and GDR_Net_Augmentation.py:78-153 (``get_bg_image``,
``replace_bg``) pastes it over a random background, optionally truncating the foreground.  Here
``MeshRenderer.render_shaded`` (zp_render_shaded) draws, ``zp_mask_bbox`` / ``zp_composite``
(csrc/zp_shade.hip) paste; only the random draws and the integer geometry of the background stay
on the host.  The exact semantics are in include/zp.h and, as numpy, in tests/synth_ref.py.
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
