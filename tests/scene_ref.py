"""numpy restatement of the scene compositor (include/zp.h: zp_scene_compose) and of
zebrapose_amd.synth.scene_compose's host fields, in the project's own words.  There is no reference
program; this file is the executable definition."""
import numpy as np


def scene_compose(depth, img_index, n_img, shaded=None):
    """depth f32 [B, H, W], img_index int [B], shaded u8 [B, H, W, 3] or None -> dict(image u8
    [n_img, H, W, 3] (None without shaded), fg u8 [n_img, H, W], scene f32 [n_img, H, W], instance
    i32 [n_img, H, W], mask_visib u8 [B, H, W], info i32 [B, 6]).

    Walks the instances in ascending order.  A surface is depth > 0 (NaN, 0 and negative values are
    none; +inf and subnormals are one).  An instance takes a pixel of its image when it has a surface
    there and the pixel has no winner yet or its depth is strictly smaller than the winner's, so a
    tie stays with the lowest instance.  An instance whose image is outside [0, n_img) takes nothing."""
    depth = np.asarray(depth, np.float32)
    B, H, W = depth.shape
    scene = np.zeros((n_img, H, W), np.float32)
    inst = np.full((n_img, H, W), -1, np.int32)
    image = None if shaded is None else np.zeros((n_img, H, W, 3), np.uint8)
    with np.errstate(invalid="ignore"):
        surf = depth > 0
        for b in range(B):
            n = int(img_index[b])
            if not 0 <= n < n_img:
                continue
            take = surf[b] & ((inst[n] < 0) | (depth[b] < scene[n]))
            scene[n][take] = depth[b][take]
            inst[n][take] = b
            if image is not None:
                image[n][take] = np.asarray(shaded[b], np.uint8)[take]
    fg = np.where(inst >= 0, 255, 0).astype(np.uint8)
    visib = np.zeros((B, H, W), np.uint8)
    info = np.zeros((B, 6), np.int32)
    for b in range(B):
        n = int(img_index[b])
        if 0 <= n < n_img:
            visib[b] = np.where(inst[n] == b, 255, 0)
        ys, xs = np.nonzero(visib[b])
        box = [0, 0, -1, -1] if len(ys) == 0 else [ys.min(), xs.min(), ys.max(), xs.max()]
        info[b] = [surf[b].sum(), len(ys)] + box
    return {"image": image, "fg": fg, "scene": scene, "instance": inst, "mask_visib": visib, "info": info}


def host_fields(info):
    """info [B, 6] -> dict(bbox_visib int64 [B, 4] = (x, y, w, h) with inclusive sizes, (0, 0, 0, 0) when
    empty; px_count_all, px_count_visib int64 [B]; visib_fract f64 [B] = px_visib / px_all, 0 where
    px_all is 0)."""
    info = np.asarray(info, np.int64)
    n_all, n_vis = info[:, 0], info[:, 1]
    box = np.stack([info[:, 3], info[:, 2], info[:, 5] - info[:, 3] + 1, info[:, 4] - info[:, 2] + 1], axis=1)
    fract = np.where(n_all > 0, n_vis / np.maximum(n_all, 1), 0.0)
    return {"bbox_visib": box, "px_count_all": n_all, "px_count_visib": n_vis, "visib_fract": fract}
