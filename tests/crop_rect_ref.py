"""Plain numpy restatement of the reference's ``crop_resize`` (bop_dataset_pytorch.py:74-88) --
test infrastructure only, written from the reference and OpenCV 4.x's generic resize rules, not
from the kernels (zebrapose_amd/csrc/zp_crop.hip).

  crop_resize          :74-88     clip the box to the image, slice img[y1:y2, x1:x2] (no squaring, no
                                  zero padding), cv2.resize(roi, (S, S)): the two axes scale apart
  get_final_Bbox       :183-192   the same clipped box
  __getitem__          :304-307   image INTER_LINEAR to crop_size_img; GT image and masks INTER_NEAREST

The resize is oracle/crop_ref.py's restatement applied per axis (its ``_lin_taps`` with n = sw for
x and n = sh for y): scale = 1 / (S / n) in double; the horizontal pass alone has the ``edge``
rule; the 2 x 2 box filter replaces INTER_LINEAR only when BOTH scales are exactly 2; sw == sh == S
is a copy.  PARITY UNPINNED against OpenCV itself, exactly as for the square path (no cv2 here).

An empty slice (cv2.resize raises on it; a negative x2 even wraps the Python slice around) is the
all-zero dummy crop here: ``rect_region`` returns None for it.
"""
import numpy as np

from oracle.crop_ref import MEAN, STD, _lin_taps


def rect_region(bbox, H, W):
    """(x1, y1, x2, y2) of the slice crop_resize takes, None when it is empty."""
    bx, by, bw, bh = (int(v) for v in bbox)
    x1, x2 = max(0, bx), min(W, bx + bw)
    y1, y2 = max(0, by), min(H, by + bh)
    if x2 <= x1 or y2 <= y1:
        return None
    return x1, y1, x2, y2


def _exactly_two(scale):
    return int(np.rint(scale)) == 2 and abs(scale - 2) < np.finfo(np.float64).eps


def resize_linear_u8(roi, S):
    """cv2.resize(roi, (S, S), interpolation=cv2.INTER_LINEAR) for a uint8 sh x sw x C roi."""
    sh, sw = roi.shape[:2]
    if sw == S and sh == S:
        return roi.copy()
    r = roi.astype(np.int64)
    if _exactly_two(1.0 / (S / sw)) and _exactly_two(1.0 / (S / sh)):
        return ((r[0::2, 0::2] + r[0::2, 1::2] + r[1::2, 0::2] + r[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xs0, xs1, xa, xedge = _lin_taps(S, sw)
    ys0, ys1, ya, _ = _lin_taps(S, sh)
    h = r[:, xs0] * xa[:, 0][None, :, None] + r[:, xs1] * xa[:, 1][None, :, None]
    h[:, xedge] = r[:, xs0[xedge]] * 2048
    h0 = np.clip(h[ys0] >> 4, -32768, 32767)
    h1 = np.clip(h[ys1] >> 4, -32768, 32767)
    v = ((h0 * ya[:, 0][:, None, None]) >> 16) + ((h1 * ya[:, 1][:, None, None]) >> 16)
    return np.clip((v + 2) >> 2, 0, 255).astype(np.uint8)


def nearest_index(S, n):
    """INTER_NEAREST source index of every output index along one axis of n source pixels."""
    return np.minimum(np.floor(np.arange(S) * (1.0 / (S / n))).astype(np.int64), n - 1)


def resize_nearest(roi, S):
    sh, sw = roi.shape[:2]
    return roi[nearest_index(S, sh)][:, nearest_index(S, sw)]


def crop_image_rect(img, bbox, S):
    """-> f32 [3, S, S]: ToTensor + Normalize of the INTER_LINEAR crop (BGR order kept)."""
    reg = rect_region(bbox, img.shape[0], img.shape[1])
    if reg is None:
        return np.zeros((3, S, S), np.float32)
    x1, y1, x2, y2 = reg
    roi = resize_linear_u8(img[y1:y2, x1:x2], S)
    x = roi.astype(np.float32) / np.float32(255)
    return ((x - MEAN) / STD).transpose(2, 0, 1).astype(np.float32)


def crop_ids_rect(gt, bbox, S):
    """-> int64 [S, S]: id = B << 16 | G << 8 | R of the INTER_NEAREST GT crop (0 for an empty slice)."""
    reg = rect_region(bbox, gt.shape[0], gt.shape[1])
    if reg is None:
        return np.zeros((S, S), np.int64)
    x1, y1, x2, y2 = reg
    g = resize_nearest(gt[y1:y2, x1:x2], S).astype(np.int64)
    return (g[:, :, 0] << 16) + (g[:, :, 1] << 8) + g[:, :, 2]


def crop_gt_rect(gt, mask, entire, bbox, S, L):
    """-> (code u8 [L, S, S], mask f32 [S, S], entire f32 [S, S])."""
    cid = crop_ids_rect(gt, bbox, S)
    code = np.stack([(cid >> (L - 1 - i)) & 1 for i in range(L)]).astype(np.uint8)
    reg = rect_region(bbox, gt.shape[0], gt.shape[1])
    if reg is None:
        return code, np.zeros((S, S), np.float32), np.zeros((S, S), np.float32)
    x1, y1, x2, y2 = reg
    m = (resize_nearest(mask[y1:y2, x1:x2], S) / 255.).astype(np.float32)
    e = (resize_nearest(entire[y1:y2, x1:x2], S) / 255.).astype(np.float32)
    return code, m, e


def tile_mask(bbox, H, W, T=32):
    """bool [H, W]: the T-aligned tiles meeting rect_region (what the augmentation's box form writes)."""
    out = np.zeros((H, W), bool)
    reg = rect_region(bbox, H, W)
    if reg is not None:
        x1, y1, x2, y2 = reg
        out[y1 // T * T:(y2 - 1) // T * T + T, x1 // T * T:(x2 - 1) // T * T + T] = True
    return out
