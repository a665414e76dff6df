"""Device crop pipeline: the DataLoader worker's per-crop CPU work of
bop_dataset_pytorch.py, batched on the GPU.

The reference's ``__getitem__`` (bop_dataset_pytorch.py:280-347) reads the image, GT code image
and masks with cv2, pads the box (``padding_Bbox``), crops a zero-padded square ROI and resizes it
(``crop_square_resize``; INTER_LINEAR to 256 px for the image, INTER_NEAREST to 128 px for the GT
image and masks), turns the GT colours into 16 code planes (``RGB_image_to_class_id_image`` +
``class_id_image_to_class_code_images``), normalises the image (``transform_pre``) and returns
``get_final_Bbox``'s box.  Here the box arithmetic stays on the host (a few integer operations
per crop, same functions as the reference) and the pixel work is two kernels over a whole batch
(``zp_crop_image_m``, ``zp_crop_gt_m``, csrc/zp_crop.hip) reading images resident in HBM.
Two of the reference's three ``resize_method``s are on the device: ``"crop_square_resize"`` (the
``config_BOP`` files; the default) and ``"crop_resize"`` (:74-88; every ``config_paper`` and
``config_ablation`` file): the box clipped to the image, sliced without squaring or zero padding
and resized with one scale per axis.  ``"crop_resize_by_warp_affine"``, which no config selects,
is not.  An empty clipped box, on which the reference's ``cv2.resize`` raises, is handled like a
missing detection (zero boxes, the all-zero dummy crop).  Parity of the resize with OpenCV itself
is unpinned for both methods (oracle/crop_ref.py, tests/crop_rect_ref.py restate it).

``CropPipeline.train_batch`` is the ``is_train`` branch (:267-277): ``aug_Bbox`` jitters the box
on the host, ``zp_augment`` (augment.py) runs the imgaug colour chain over the part of the image
the crop reads, and the same two crop kernels follow.  numpy's global RNG of the reference is a
``np.random.Generator`` here, so the draws differ from the reference's for a given seed.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L


def padding_Bbox(Bbox, padding_ratio):
    """bop_dataset_pytorch.py:124-139."""
    x1, x2 = Bbox[0], Bbox[0] + Bbox[2]
    y1, y2 = Bbox[1], Bbox[1] + Bbox[3]
    cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    bh, bw = y2 - y1, x2 - x1
    pbw, pbh = int(bw * padding_ratio), int(bh * padding_ratio)
    return np.array([int(cx - pbw / 2), int(cy - pbh / 2), int(pbw), int(pbh)])


def aug_Bbox(GT_Bbox, padding_ratio, rng):
    """bop_dataset_pytorch.py:141-160 with ``rng.random()`` then ``rng.random(2)`` for the two
    np.random.random_sample calls."""
    x1, x2 = GT_Bbox[0], GT_Bbox[0] + GT_Bbox[2]
    y1, y2 = GT_Bbox[1], GT_Bbox[1] + GT_Bbox[3]
    cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    bh, bw = y2 - y1, x2 - x1
    scale_ratio = 1 + 0.25 * (2 * rng.random() - 1)  # [1 - 0.25, 1 + 0.25]
    shift_ratio = 0.25 * (2 * rng.random(2) - 1)  # [-0.25, 0.25]
    center = np.array([cx + bw * shift_ratio[0], cy + bh * shift_ratio[1]])
    abw, abh = int(bw * scale_ratio * padding_ratio), int(bh * scale_ratio * padding_ratio)
    return np.array([int(center[0] - abw / 2), int(center[1] - abh / 2), abw, abh])


def get_final_Bbox(Bbox, resize_method, max_x, max_y):
    """bop_dataset_pytorch.py:162-194 (the box the decode maps pixels back with)."""
    x1, bw = Bbox[0], Bbox[2]
    y1, bh = Bbox[1], Bbox[3]
    x2, y2 = x1 + bw, y1 + bh
    if resize_method in ("crop_square_resize", "crop_resize_by_warp_affine"):
        c = np.array([0.5 * (x1 + x2), 0.5 * (y1 + y2)])
        if bh > bw:
            x1, x2 = c[0] - bh / 2, c[0] + bh / 2
        else:
            y1, y2 = c[1] - bw / 2, c[1] + bw / 2
        x1, y1, x2, y2 = int(x1), int(y1), int(x2), int(y2)
        return np.array([x1, y1, x2 - x1, y2 - y1])
    if resize_method == "crop_resize":
        x1, y1 = int(max(x1, 0)), int(max(y1, 0))
        x2, y2 = int(min(x2, max_x)), int(min(y2, max_y))
        return np.array([x1, y1, x2 - x1, y2 - y1])
    return Bbox


def _u8(t, name, ndim):
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_cuda and t.dim() == ndim):
        raise ValueError(f"{name}: expected a uint8 CUDA tensor with {ndim} dims")
    return t.contiguous()


class CropPipeline:
    """Batched crops of device-resident images: square ROIs (``crop_square_resize``) or the clipped
    rectangular ones of ``crop_resize``."""

    _METHODS = {"crop_square_resize": L.ZP_CROP_SQUARE, "crop_resize": L.ZP_CROP_RECT}

    def __init__(self, crop_size_img=256, crop_size_gt=128, code_bits=16, padding_ratio=1.5, class_base=2,
                 iterations=None, resize_method="crop_square_resize"):
        """class_base d != 2 (the d-ary code ablation): ``code`` holds the ``iterations`` digit planes
        of class_id_image_to_class_code_images(id, d, iterations, 65536)
        (class_id_encoder_decoder.py:43-63; iterations defaults to log_d 65536).
        resize_method: the config key of that name, ``"crop_square_resize"`` or ``"crop_resize"``."""
        if resize_method == "crop_resize_by_warp_affine":
            raise NotImplementedError("resize_method crop_resize_by_warp_affine is not on the device (no config "
                                      "selects it); use crop_square_resize or crop_resize")
        if resize_method not in self._METHODS:
            raise NotImplementedError(f"unknown decoder type: {resize_method}")  # get_roi (:122)
        self.resize_method = resize_method
        self.method = self._METHODS[resize_method]
        self.S_img, self.S_gt = int(crop_size_img), int(crop_size_gt)
        self.L = int(code_bits)
        self.padding_ratio = padding_ratio
        self.class_base = d = int(class_base)
        self.digit_bits = 0
        if d != 2:
            s = d.bit_length() - 1
            if d < 2 or d > 256 or d & (d - 1) or 16 % s:
                raise ValueError(f"class_base {class_base}: a power of two whose power is 65536 is needed")
            if iterations is None:
                iterations = 16 // s
            if d ** int(iterations) != 65536:  # class_id_encoder_decoder.py:47-48
                raise ValueError("this combination of base and iteration is not possible")
            self.digit_bits, self.L = s, 16
        elif iterations is not None and int(iterations) != self.L:
            raise ValueError("class_base 2: iterations is code_bits")

    def boxes(self, Bboxes, img_w, img_h):
        """Host box arithmetic for a batch of raw boxes [B, 4] -> (padded boxes int32 [B, 4] fed to
        the kernels, final boxes int64 [B, 4] for the decode).  A box of -1s (no detection) stays a
        zero box: the kernels then emit the reference's all-zero dummy crop.  So does, under
        ``"crop_resize"``, a box whose clipped ROI is empty."""
        pad, fin = [], []
        for bb in np.asarray(Bboxes).reshape(-1, 4):
            if np.any(np.isclose(bb, -1)):  # :291-298
                pad.append(np.zeros(4, np.int64))
                fin.append(np.zeros(4, np.int64))
                continue
            p, f = self._final(padding_Bbox(bb, self.padding_ratio), img_w, img_h)
            pad.append(p)
            fin.append(f)
        return np.stack(pad).astype(np.int32), np.stack(fin).astype(np.int64)

    def _final(self, box, img_w, img_h):
        """(box, get_final_Bbox of it); two zero boxes when ``crop_resize`` clips the box to nothing."""
        f = get_final_Bbox(box, self.resize_method, img_w, img_h)
        if self.method == L.ZP_CROP_RECT and (f[2] <= 0 or f[3] <= 0):
            return np.zeros(4, np.int64), np.zeros(4, np.int64)
        return box, f

    def __call__(self, images, img_index, boxes, gt_images=None, masks=None, entire_masks=None, gt_index=None):
        """images u8 [N, H, W, 3] (BGR, device); img_index int [B]; boxes = padded boxes int [B, 4].
        Returns dict: x f32 [B, 3, S_img, S_img] and, when the GT inputs are given, code u8
        [B, L, S_gt, S_gt] (bit planes, or the d-ary digits for class_base d), mask / entire_mask f32 [B, S_gt, S_gt].
        gt_index int [B] (default None: the GT stacks are aligned with the images and crop b reads GT
        image img_index[b]): the GT stacks have a first dimension Ng of their own, one entry per
        instance as in a BOP dataset (one GT code image and mask file per instance, one RGB per
        frame) or in ``synth.SceneBatcher``'s output, and crop b reads GT image gt_index[b]."""
        images, gt_images, masks, entire_masks, ii, gi = self._check(images, img_index, gt_images, masks, entire_masks,
                                                                     gt_index)
        bb = torch.as_tensor(np.asarray(boxes), dtype=torch.int32).reshape(len(ii), 4).to(images.device).contiguous()
        return self._crop(images, ii, bb, gt_images, masks, entire_masks, gi)

    @staticmethod
    def _check(images, img_index, gt_images, masks, entire_masks, gt_index=None):
        images = _u8(images, "images", 4)
        gt_images = _u8(gt_images, "gt_images", 4)
        masks = _u8(masks, "masks", 3)
        entire_masks = _u8(entire_masks, "entire_masks", 3)
        N, H, W, C = images.shape
        if C != 3:
            raise ValueError("images must be HWC with 3 channels")
        gts = [t for t in (gt_images, masks, entire_masks) if t is not None]
        if gt_index is None:
            Ng = N
        elif not gts:
            raise ValueError("gt_index without GT images or masks")
        else:
            Ng = gts[0].shape[0]
        for t in gts:
            if t.shape[0] != Ng or t.shape[1] != H or t.shape[2] != W:
                raise ValueError("GT images / masks must match the image stack" if gt_index is None else
                                 "with gt_index, GT images / masks must agree on their first dimension and match "
                                 "the images' height and width")
        idx = np.asarray(img_index, dtype=np.int64).reshape(-1)
        if len(idx) == 0 or idx.min() < 0 or idx.max() >= N:
            raise ValueError("img_index out of range")
        ii = torch.from_numpy(idx.astype(np.int32)).to(images.device)
        if gt_index is None:
            return images, gt_images, masks, entire_masks, ii, ii
        g = np.asarray(gt_index.cpu() if isinstance(gt_index, torch.Tensor) else gt_index)
        if g.ndim != 1 or len(g) != len(idx) or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"gt_index: expected {len(idx)} integers")
        if g.min() < 0 or g.max() >= Ng:
            raise ValueError("gt_index out of range")
        return images, gt_images, masks, entire_masks, ii, torch.from_numpy(g.astype(np.int32)).to(images.device)

    def _crop(self, images, ii, bb, gt_images, masks, entire_masks, gt_ii):
        """The two crop kernels: crop b reads images[ii[b]] and the GT stacks' image gt_ii[b]."""
        N, H, W, _ = images.shape
        B = len(ii)
        dev = images.device
        st = L.stream_ptr()
        out = {"x": torch.empty((B, 3, self.S_img, self.S_img), dtype=torch.float32, device=dev)}
        L.call("zp_crop_image_m", images.data_ptr(), N, H, W, ii.data_ptr(), bb.data_ptr(), B, self.S_img,
               out["x"].data_ptr(), self.method, st)
        if gt_images is not None or masks is not None or entire_masks is not None:
            S = self.S_gt
            Ng = next(t for t in (gt_images, masks, entire_masks) if t is not None).shape[0]
            code = torch.empty((B, self.L, S, S), dtype=torch.uint8, device=dev) if gt_images is not None else None
            m = torch.empty((B, S, S), dtype=torch.float32, device=dev) if masks is not None else None
            e = torch.empty((B, S, S), dtype=torch.float32, device=dev) if entire_masks is not None else None
            L.call("zp_crop_gt_m", L.ptr(gt_images), L.ptr(masks), L.ptr(entire_masks), Ng, H, W, gt_ii.data_ptr(),
                   bb.data_ptr(), B, S, self.L, L.ptr(code), L.ptr(m), L.ptr(e), self.method, st)
            if code is not None and self.digit_bits:  # the 16 bit planes -> 16 / s digit planes (zp_pack_digits)
                digits = torch.empty((B, 16 // self.digit_bits, S, S), dtype=torch.uint8, device=dev)
                L.call("zp_pack_digits", code.data_ptr(), B, 16, S, S, self.digit_bits, digits.data_ptr(), st)
                code = digits
            out.update(code=code, mask=m, entire_mask=e)
        return out

    def train_boxes(self, Bboxes, img_w, img_h, rng):
        """``boxes`` for the training branch: aug_Bbox in place of padding_Bbox (:270, :277)."""
        aug, fin = [], []
        for bb in np.asarray(Bboxes).reshape(-1, 4):
            a, f = self._final(aug_Bbox(bb, self.padding_ratio, rng), img_w, img_h)
            aug.append(a)
            fin.append(f)
        return np.stack(aug).astype(np.int32), np.stack(fin).astype(np.int64)

    def train_batch(self, images, img_index, raw_boxes, gt_images, masks, entire_masks, sampler, gt_index=None):
        """The ``is_train`` branch (bop_dataset_pytorch.py:267-277) for a batch: raw_boxes [B, 4] are
        the GT ``bbox_visib`` boxes; ``sampler`` (augment.AugmentSampler) supplies the colour chain's
        draws and, through ``sampler.rng``, aug_Bbox's.  aug boxes -> zp_augment over each crop's
        copied region -> zp_crop_image on the augmented stack -> zp_crop_gt on the untouched GT
        stacks.  Returns ``__call__``'s dict plus ``final_boxes`` (int64 [B, 4], get_final_Bbox) and
        ``boxes`` (the augmented boxes, int32 [B, 4]).  gt_index as in ``__call__``: per-instance GT stacks."""
        from .augment import augment_images
        images, gt_images, masks, entire_masks, ii, gi = self._check(images, img_index, gt_images, masks, entire_masks,
                                                                     gt_index)
        N, H, W, _ = images.shape
        B = len(ii)
        aug_boxes, final_boxes = self.train_boxes(raw_boxes, W, H, sampler.rng)
        if len(aug_boxes) != B:
            raise ValueError("raw_boxes and img_index disagree on the batch size")
        batch = sampler.sample(B, H, W)
        bb = torch.from_numpy(aug_boxes).to(images.device)
        aug = augment_images(images, ii, batch, bbox=bb, method=self.method)
        out = self._crop(aug, torch.arange(B, dtype=torch.int32, device=images.device), bb, gt_images, masks,
                         entire_masks, gi)
        out.update(final_boxes=final_boxes, boxes=aug_boxes, aug=batch)
        return out
