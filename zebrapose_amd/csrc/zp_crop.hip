// Device-side crop pipeline: ROI crop + resize + normalisation of the
// RGB input, nearest-neighbour crops of the GT code image and the masks, GT colour -> 16-bit
// code planes.  Replaces the CPU DataLoader worker path of bop_dataset_pytorch.py:
//   padding_Bbox (:124-139, host) -> get_roi (:110-122) with one of two resize_methods,
//     ZP_CROP_SQUARE  "crop_square_resize" (:36-72, the config_BOP files): the box squared around its
//                     centre, a zero-padded s x s ROI
//     ZP_CROP_RECT    "crop_resize" (:74-88, the paper and ablation configs): the box clipped to the
//                     image, an sw x sh ROI wholly inside it, each axis resized with its own scale
//     (crop_resize_by_warp_affine, which no config selects, is not on the device)
//   with cv2.INTER_LINEAR (image, 256) / cv2.INTER_NEAREST (GT image, masks, 128) (:304-316)
//   -> RGB_image_to_class_id_image + class_id_image_to_class_code_images
//      (class_id_encoder_decoder.py:6-15, 43-63) -> transform_pre (:333-347: ToTensor +
//      Normalize with the RGB ImageNet constants on the BGR array, masks / 255.)
// cv2.resize is a third-party dependency absent from the image; the resize arithmetic follows
// OpenCV 4.x's generic (non-IPP) path, restated in oracle/crop_ref.py for a square source and in
// tests/crop_rect_ref.py per axis (parity vs OpenCV unpinned for both methods); below, n is the ROI's
// side along the axis (sw for x, sh for y) and scale = 1 / (dsize / n):
//   INTER_LINEAR, 8U: fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), clamped at both
//     borders with fx = 0; 11-bit fixed-point coefficients saturate_cast<short>(c * 2048);
//     horizontal pass exact in int32; vertical pass as the SIMD kernel computes it:
//     u8((mulhi16(h0 >> 4, b0) + mulhi16(h1 >> 4, b1) + 2) >> 2); an exact 2x downscale of BOTH axes
//     is routed to INTER_AREA (2x2 box, (a + b + c + d + 2) >> 2) as cv::resize does; sw == sh == S copies.
//   INTER_NEAREST: sx = min(floor(dx * (1 / (dsize / ssize))), ssize - 1).
// One thread per output pixel; the source image stays in HBM/L2 (one crop reads at most its
// ROI once), outputs are written coalesced.
// The training branch's colour augmentation (apply_augmentation, :349-355) runs ahead of the image
// crop as one fused tile kernel (k_augment below, zp_augment), sharing crop_geo with the crops.
// An empty ROI (either side <= 0; cv2.resize raises on it) is the all-zero dummy crop under both methods.
#include <math.h>
#include "zp_common.h"

namespace zp {

struct CropGeo {
  int x1, y1, xe, ye;  // ROI origin in the image, exclusive end of the copied image region
  int sw, sh;          // ROI sides; both 0 = dummy crop
};

// ZP_CROP_RECT, crop_resize (:74-88): the box clipped to the image is the ROI, every pixel of it in the image.
// ZP_CROP_SQUARE, crop_square_resize (:36-72): square-ify around the box centre, int() truncation, the ROI is
// s x s (s = max(bh, bw)) with roi(y, x) = img(y1 + y, x1 + x) inside [0, min(H, y2)) x [0, min(W, x2)), else 0
__device__ __forceinline__ CropGeo crop_geo(const int* bb, int H, int W, int method) {
  CropGeo g;
  const int bx = bb[0], by = bb[1];
  if (method == ZP_CROP_RECT) {
    g.x1 = max(bx, 0);
    g.y1 = max(by, 0);
    g.xe = (int)max(min((long long)bx + bb[2], (long long)W), 0ll);  // 64-bit sum: no wrap for any int32 box
    g.ye = (int)max(min((long long)by + bb[3], (long long)H), 0ll);
    g.sw = g.xe - g.x1;
    g.sh = g.ye - g.y1;
    if (g.sw <= 0 || g.sh <= 0) g.sw = g.sh = 0;
    return g;
  }
  const int bw = max(bb[2], 0), bh = max(bb[3], 0);
  double x1 = bx, x2 = (double)bx + bw, y1 = by, y2 = (double)by + bh;
  const double cx = 0.5 * (x1 + x2), cy = 0.5 * (y1 + y2);
  if (bh > bw) {
    x1 = cx - bh / 2.0;
    x2 = cx + bh / 2.0;
  } else {
    y1 = cy - bw / 2.0;
    y2 = cy + bw / 2.0;
  }
  g.x1 = (int)x1;  // Python int(): truncation toward zero
  g.y1 = (int)y1;
  g.xe = min((int)x2, W);
  g.ye = min((int)y2, H);
  g.sw = g.sh = max(bh, bw);
  return g;
}

__device__ __forceinline__ int roi_px(const uint8_t* img, int W, const CropGeo& g, int y, int x, int c) {
  const int iy = g.y1 + y, ix = g.x1 + x;
  if (iy < 0 || ix < 0 || iy >= g.ye || ix >= g.xe) return 0;
  return img[((size_t)iy * W + ix) * 3 + c];
}

// OpenCV cvRound on float (round half to even) then saturate to short
__device__ __forceinline__ int coef_q11(float c) { return (int)rintf(c * 2048.f); }

struct LinTap {
  int s0, s1;  // source index pair
  int a0, a1;  // Q11 coefficients
  bool edge;   // beyond xmax / clamped: only s0 * 2048 (horizontal pass)
};

__device__ __forceinline__ LinTap lin_tap(int d, double scale, int n) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  LinTap t;
  t.edge = false;
  if (s < 0) {
    f = 0.f;
    s = 0;
  }
  if (s + 1 >= n) {
    t.edge = true;
    if (s >= n - 1) {
      f = 0.f;
      s = n - 1;
    }
  }
  t.s0 = s;
  t.s1 = min(s + 1, n - 1);
  t.a0 = coef_q11(1.f - f);
  t.a1 = coef_q11(f);
  return t;
}

// cv::resize's is_area_fast test for a scale of 2: within DBL_EPSILON of the integer
__device__ __forceinline__ bool exactly_2x(double scale) {
  const int iscale = (int)rint(scale);
  return iscale == 2 && fabs(scale - iscale) < 2.220446049250313e-16;
}

__device__ __forceinline__ int mulhi16(int a, int b) {
  a = max(-32768, min(32767, a));  // v_pack saturation
  return (a * b) >> 16;
}

// image crop: out f32 NCHW [B][3][S][S], normalised ((v / 255 - mean[c]) / std[c], BGR order kept)
__global__ void __launch_bounds__(256) k_crop_image(const uint8_t* __restrict__ imgs, int H, int W,
                                                    const int* __restrict__ img_index, const int* __restrict__ bbox,
                                                    int S, float* __restrict__ out, int method) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= S * S) return;
  const int dy = p / S, dx = p - dy * S;
  const CropGeo g = crop_geo(bbox + 4 * b, H, W, method);
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  float* o = out + (size_t)b * 3 * S * S + p;
  if (g.sw <= 0) {  // the reference's dummy input for a missing detection (:285-298): zeros
    for (int c = 0; c < 3; ++c) o[(size_t)c * S * S] = 0.f;
    return;
  }
  const uint8_t* img = imgs + (size_t)img_index[b] * H * W * 3;
  int v[3];
  // cv::resize per axis: inv_scale = dsize / ssize, scale = 1 / inv_scale
  // (equal sides, always so for ZP_CROP_SQUARE, share one pair of f64 divisions)
  const double scale_x = 1.0 / ((double)S / g.sw);
  const double scale_y = g.sh == g.sw ? scale_x : 1.0 / ((double)S / g.sh);
  if (g.sw == S && g.sh == S) {
    for (int c = 0; c < 3; ++c) v[c] = roi_px(img, W, g, dy, dx, c);
  } else if (exactly_2x(scale_x) && exactly_2x(scale_y)) {
    // INTER_LINEAR at an exact 2x downscale of both axes -> INTER_AREA fast path (2 x 2 box)
    for (int c = 0; c < 3; ++c)
      v[c] = (roi_px(img, W, g, 2 * dy, 2 * dx, c) + roi_px(img, W, g, 2 * dy, 2 * dx + 1, c) +
              roi_px(img, W, g, 2 * dy + 1, 2 * dx, c) + roi_px(img, W, g, 2 * dy + 1, 2 * dx + 1, c) + 2) >> 2;
  } else {
    const LinTap tx = lin_tap(dx, scale_x, g.sw), ty = lin_tap(dy, scale_y, g.sh);
    for (int c = 0; c < 3; ++c) {
      int h[2];
      for (int k = 0; k < 2; ++k) {
        const int sy = k == 0 ? ty.s0 : ty.s1;
        const int p0 = roi_px(img, W, g, sy, tx.s0, c);
        h[k] = tx.edge ? p0 * 2048 : p0 * tx.a0 + roi_px(img, W, g, sy, tx.s1, c) * tx.a1;
      }
      const int r = (mulhi16(h[0] >> 4, ty.a0) + mulhi16(h[1] >> 4, ty.a1) + 2) >> 2;
      v[c] = max(0, min(255, r));
    }
  }
  for (int c = 0; c < 3; ++c) {
    const float x = (float)v[c] / 255.f;  // ToTensor: byte -> float / 255
    o[(size_t)c * S * S] = (x - mean[c]) / stdv[c];
  }
}

// GT crop (nearest, S_gt): code planes u8 [B][L][S][S] (bit i = (id >> (L - 1 - i)) & 1 with
// id = B << 16 | G << 8 | R of the BGR GT image), visible / entire masks f32 [B][S][S] = v / 255.
__global__ void __launch_bounds__(256) k_crop_gt(const uint8_t* __restrict__ gts, const uint8_t* __restrict__ masks,
                                                 const uint8_t* __restrict__ entire, int H, int W,
                                                 const int* __restrict__ img_index, const int* __restrict__ bbox, int S,
                                                 int L, uint8_t* __restrict__ code, float* __restrict__ mask_out,
                                                 float* __restrict__ entire_out, int method) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= S * S) return;
  const int dy = p / S, dx = p - dy * S;
  const CropGeo g = crop_geo(bbox + 4 * b, H, W, method);
  int id = 0, mv = 0, ev = 0;
  if (g.sw > 0) {
    const double ifx = 1.0 / ((double)S / g.sw);
    const double ify = g.sh == g.sw ? ifx : 1.0 / ((double)S / g.sh);
    const int sx = min((int)floor(dx * ifx), g.sw - 1), sy = min((int)floor(dy * ify), g.sh - 1);
    const int iy = g.y1 + sy, ix = g.x1 + sx;
    if (iy >= 0 && ix >= 0 && iy < g.ye && ix < g.xe) {
      const size_t im = (size_t)img_index[b] * H * W;
      const size_t q = im + (size_t)iy * W + ix;
      if (gts) id = (gts[q * 3] << 16) | (gts[q * 3 + 1] << 8) | gts[q * 3 + 2];
      if (masks) mv = masks[q];
      if (entire) ev = entire[q];
    }
  }
  if (code) {
    uint8_t* cp = code + (size_t)b * L * S * S + p;
    for (int i = 0; i < L; ++i) cp[(size_t)i * S * S] = (uint8_t)((id >> (L - 1 - i)) & 1);
  }
  if (mask_out) mask_out[(size_t)b * S * S + p] = (float)((double)mv / 255.0);
  if (entire_out) entire_out[(size_t)b * S * S + p] = (float)((double)ev / 255.0);
}

// digit planes of a d-ary code from zp_crop_gt's 16 bit planes (d = 2^s, L = 16 / s steps):
// class_id_image_to_class_code_images(id, d, L, 65536) (class_id_encoder_decoder.py:43-63) gives
// digit_i = (id >> s (L - 1 - i)) & (d - 1), i.e. bit planes [s i, s i + s) of id's low 16 bits, MSB first
__global__ void __launch_bounds__(256) k_pack_digits(const uint8_t* __restrict__ bits, int HW, int nbits, int s,
                                                     uint8_t* __restrict__ digits) {
  const int b = blockIdx.z, i = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int L = nbits / s;
  const uint8_t* bp = bits + ((size_t)b * nbits + (size_t)i * s) * HW + p;
  int v = 0;
  for (int j = 0; j < s; ++j) v = (v << 1) | (bp[(size_t)j * HW] & 1);
  digits[((size_t)b * L + i) * HW + p] = (uint8_t)v;
}

// ---- training-branch colour augmentation (zp_augment, include/zp.h) ---------------------------
// One workgroup per AUG_T x AUG_T output tile and crop, fused through two LDS planes of packed
// B | G << 8 | R << 16 pixels:
//   p0: stage 0 (salt and pepper) of the tile + 4 px halo, loaded from the reflected in-image position
//   p1: stages 1-2 (stencil A, coarse dropout) of the tile + 2 px halo
//   out: stages 3-4 (stencil B, LUT) -> byte tile in LDS -> coalesced stores
// Every plane entry is indexed by its UNREFLECTED coordinate c and holds the stage's value AT
// reflect101(c): a p1 entry outside the image is stencil A evaluated around the in-image pixel it
// mirrors (whose own taps are in p0, see the index bounds below), not stencil A over a mirrored
// extension of stage 0 -- the two differ for an asymmetric (motion) kernel.
constexpr int AUG_T = 32, AUG_P0 = AUG_T + 8, AUG_P1 = AUG_T + 4;

struct AugDesc {  // = zp_aug_desc
  uint32_t flags, sp_seed, sp_thresh;
  int kA[25], kB[25];
};

__device__ __forceinline__ int reflect101(int c, int n) {  // one reflection (|overhang| <= n - 1), then clamped
  c = c < 0 ? -c : c;
  c = c >= n ? 2 * n - 2 - c : c;
  return max(0, min(n - 1, c));
}

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// 5 x 5 Q16 stencil around p[0] (row stride ld) on packed pixels
__device__ __forceinline__ uint32_t stencil5(const uint32_t* p, int ld, const int* __restrict__ k) {
  int a0 = 32768, a1 = 32768, a2 = 32768;
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const uint32_t v = p[(i - 2) * ld + (j - 2)];
      const int w = k[i * 5 + j];
      a0 += w * (int)(v & 255u);
      a1 += w * (int)((v >> 8) & 255u);
      a2 += w * (int)(v >> 16);
    }
  return (uint32_t)min(255, a0 >> 16) | ((uint32_t)min(255, a1 >> 16) << 8) | ((uint32_t)min(255, a2 >> 16) << 16);
}

__global__ void __launch_bounds__(256) k_augment(const uint8_t* __restrict__ imgs, int H, int W,
                                                 const int* __restrict__ img_index, const AugDesc* __restrict__ desc,
                                                 const uint8_t* __restrict__ masks, int mh, int mw,
                                                 const uint8_t* __restrict__ luts, const uint8_t* __restrict__ beta_tab,
                                                 const int* __restrict__ bbox, uint8_t* __restrict__ out, int vec,
                                                 int method) {
  __shared__ uint32_t p0[AUG_P0 * AUG_P0];
  __shared__ uint32_t p1[AUG_P1 * AUG_P1];
  __shared__ uint32_t obuf[AUG_T * AUG_T * 3 / 4];
  __shared__ uint8_t lut_s[3 * 256];
  __shared__ int mrow[AUG_P1], mcol[AUG_P1];
  const int b = blockIdx.z, ty0 = blockIdx.y * AUG_T, tx0 = blockIdx.x * AUG_T, tid = threadIdx.x;
  if (bbox) {  // only tiles meeting the region the crop copies: [max(x1,0), xe) x [max(y1,0), ye)
    const CropGeo g = crop_geo(bbox + 4 * b, H, W, method);
    if (g.sw <= 0 || tx0 >= g.xe || ty0 >= g.ye || tx0 + AUG_T <= max(g.x1, 0) || ty0 + AUG_T <= max(g.y1, 0)) return;
  }
  const AugDesc* d = desc + b;
  const uint32_t flags = d->flags;
  const uint8_t* img = imgs + (size_t)img_index[b] * H * W * 3;

  // stage 0 into p0; coordinates [t0 - 4, t0 + T + 4)
  const bool sp = flags & 1u;
  const uint32_t seed = d->sp_seed, thresh = d->sp_thresh;
  for (int idx = tid; idx < AUG_P0 * AUG_P0; idx += 256) {
    const int i = idx / AUG_P0, j = idx - i * AUG_P0;
    const int y = reflect101(ty0 - 4 + i, H), x = reflect101(tx0 - 4 + j, W);
    const uint8_t* s = img + ((size_t)y * W + x) * 3;
    uint32_t v = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
    if (sp) {
      const uint32_t h1 = fmix32(seed ^ (((uint32_t)y * (uint32_t)W + (uint32_t)x) * 0x9E3779B9u));
      if (h1 < thresh) v = (uint32_t)beta_tab[fmix32(h1 ^ 0x68bc21ebu) >> 24] * 0x010101u;
    }
    p0[idx] = v;
  }
  if (flags & 4u) {  // INTER_NEAREST row / column of the keep-mask for p1's coordinates
    if (tid < AUG_P1)
      mrow[tid] = min((int)floor(reflect101(ty0 - 2 + tid, H) * (1.0 / ((double)H / mh))), mh - 1);
    else if (tid >= 64 && tid < 64 + AUG_P1)
      mcol[tid - 64] = min((int)floor(reflect101(tx0 - 2 + tid - 64, W) * (1.0 / ((double)W / mw))), mw - 1);
  }
  if (flags & 16u)
    for (int idx = tid; idx < 3 * 256; idx += 256) lut_s[idx] = luts[(size_t)b * 768 + idx];
  __syncthreads();

  // stages 1-2 into p1; coordinates [t0 - 2, t0 + T + 2).  An entry at c reads p0 around q = reflect101(c):
  // rows q - 2 .. q + 2 relative to t0 - 4.  In the image q = c and the rows are c - t0 + 2 .. c - t0 + 6, within
  // [0, T + 8).  c in {-2, -1} (t0 = 0): q in {1, 2}, rows 3 .. 8.  c in {n, n + 1} (n <= t0 + T + 1, t0 <= n - 1):
  // q = 2n - 2 - c, rows 2n - c - t0 >= n - 1 - t0 >= 0 up to n + 4 - t0 <= T + 5.  Entries beyond n + 1 are
  // never read by an in-image output and are left unset.
  const uint8_t* mk = masks + (size_t)b * mh * mw;
  for (int idx = tid; idx < AUG_P1 * AUG_P1; idx += 256) {
    const int i = idx / AUG_P1, j = idx - i * AUG_P1;
    const int cy = ty0 - 2 + i, cx = tx0 - 2 + j;
    if (cy > H + 1 || cx > W + 1) continue;
    const int by = min(max(reflect101(cy, H) - (ty0 - 4), 2), AUG_P0 - 3);
    const int bx = min(max(reflect101(cx, W) - (tx0 - 4), 2), AUG_P0 - 3);
    const uint32_t* c = p0 + by * AUG_P0 + bx;
    uint32_t v = (flags & 2u) ? stencil5(c, AUG_P0, d->kA) : c[0];
    if ((flags & 4u) && !mk[mrow[i] * mw + mcol[j]]) v = 0;
    p1[idx] = v;
  }
  __syncthreads();

  // stages 3-4 into the byte tile
  uint8_t* ob = (uint8_t*)obuf;
  for (int idx = tid; idx < AUG_T * AUG_T; idx += 256) {
    const int oy = idx / AUG_T, ox = idx - oy * AUG_T;
    if (ty0 + oy >= H || tx0 + ox >= W) continue;
    const uint32_t* c = p1 + (oy + 2) * AUG_P1 + ox + 2;
    const uint32_t v = (flags & 8u) ? stencil5(c, AUG_P1, d->kB) : c[0];
    uint32_t c0 = v & 255u, c1 = (v >> 8) & 255u, c2 = v >> 16;
    if (flags & 16u) {
      c0 = lut_s[c0];
      c1 = lut_s[256 + c1];
      c2 = lut_s[512 + c2];
    }
    ob[idx * 3] = (uint8_t)c0;
    ob[idx * 3 + 1] = (uint8_t)c1;
    ob[idx * 3 + 2] = (uint8_t)c2;
  }
  __syncthreads();

  // tile rows are wv * 3 contiguous bytes; as dwords when every row start is 4-byte aligned (vec)
  const int hv = min(AUG_T, H - ty0), wv = min(AUG_T, W - tx0);
  uint8_t* o = out + ((size_t)b * H * W + (size_t)ty0 * W + tx0) * 3;
  if (vec) {
    const int nd = wv * 3 / 4;
    for (int idx = tid; idx < hv * nd; idx += 256) {
      const int r = idx / nd, q = idx - r * nd;
      ((uint32_t*)(o + (size_t)r * W * 3))[q] = obuf[r * (AUG_T * 3 / 4) + q];
    }
  } else {
    const int nb = wv * 3;
    for (int idx = tid; idx < hv * nb; idx += 256) {
      const int r = idx / nb, q = idx - r * nb;
      o[(size_t)r * W * 3 + q] = ob[r * AUG_T * 3 + q];
    }
  }
}

}  // namespace zp

using namespace zp;

#define ZP_CHECK_METHOD(fn) \
  ZP_CHECK_ARG(method == ZP_CROP_SQUARE || method == ZP_CROP_RECT, fn ": unknown crop method %d", method)

extern "C" int zp_crop_image_m(const uint8_t* imgs, int n_img, int H, int W, const int* img_index, const int* bbox,
                               int B, int S, float* out, int method, void* stream) {
  ZP_CHECK_METHOD("zp_crop_image_m");
  ZP_CHECK_ARG(imgs && img_index && bbox && out && n_img > 0 && H > 0 && W > 0 && B > 0 && S > 0,
               "zp_crop_image: bad args");
  ZP_CHECK_ARG((long long)n_img * H * W * 3 < (1ll << 40), "zp_crop_image: image stack too large");
  hipLaunchKernelGGL(k_crop_image, dim3((S * S + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, imgs, H, W,
                     img_index, bbox, S, out, method);
  ZP_LAUNCH_CHECK("zp_crop_image");
  return ZP_OK;
}

extern "C" int zp_crop_image(const uint8_t* imgs, int n_img, int H, int W, const int* img_index, const int* bbox,
                             int B, int S, float* out, void* stream) {
  return zp_crop_image_m(imgs, n_img, H, W, img_index, bbox, B, S, out, ZP_CROP_SQUARE, stream);
}

extern "C" int zp_crop_gt_m(const uint8_t* gts, const uint8_t* masks, const uint8_t* entire_masks, int n_img, int H,
                            int W, const int* img_index, const int* bbox, int B, int S, int L, uint8_t* code,
                            float* mask_out, float* entire_out, int method, void* stream) {
  ZP_CHECK_METHOD("zp_crop_gt_m");
  ZP_CHECK_ARG(img_index && bbox && n_img > 0 && H > 0 && W > 0 && B > 0 && S > 0, "zp_crop_gt: bad args");
  ZP_CHECK_ARG(!code || (gts && L >= 1 && L <= 24), "zp_crop_gt: code planes need the GT image and 1 <= L <= 24");
  ZP_CHECK_ARG(!mask_out || masks, "zp_crop_gt: mask_out needs masks");
  ZP_CHECK_ARG(!entire_out || entire_masks, "zp_crop_gt: entire_out needs entire_masks");
  hipLaunchKernelGGL(k_crop_gt, dim3((S * S + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, gts, masks,
                     entire_masks, H, W, img_index, bbox, S, L, code, mask_out, entire_out, method);
  ZP_LAUNCH_CHECK("zp_crop_gt");
  return ZP_OK;
}

extern "C" int zp_crop_gt(const uint8_t* gts, const uint8_t* masks, const uint8_t* entire_masks, int n_img, int H,
                          int W, const int* img_index, const int* bbox, int B, int S, int L, uint8_t* code,
                          float* mask_out, float* entire_out, void* stream) {
  return zp_crop_gt_m(gts, masks, entire_masks, n_img, H, W, img_index, bbox, B, S, L, code, mask_out, entire_out,
                      ZP_CROP_SQUARE, stream);
}

extern "C" int zp_pack_digits(const uint8_t* bits, int B, int nbits, int H, int W, int s, uint8_t* digits, void* stream) {
  ZP_CHECK_ARG(bits && digits && B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 30),
               "zp_pack_digits: bad args");
  ZP_CHECK_ARG(s >= 1 && s <= 8 && nbits >= s && nbits <= 24 && nbits % s == 0,
               "zp_pack_digits: %d bit planes do not split into digits of %d bits", nbits, s);
  const int HW = H * W;
  hipLaunchKernelGGL(k_pack_digits, dim3((HW + 255) / 256, nbits / s, B), dim3(256), 0, (hipStream_t)stream, bits, HW,
                     nbits, s, digits);
  ZP_LAUNCH_CHECK("zp_pack_digits");
  return ZP_OK;
}

extern "C" int zp_augment_m(const uint8_t* imgs, int n_img, int H, int W, const int* img_index,
                            const zp_aug_desc* desc, const uint8_t* masks, int mh, int mw, const uint8_t* luts,
                            const uint8_t* beta_tab, const int* bbox, int B, uint8_t* out, int method, void* stream) {
  ZP_CHECK_METHOD("zp_augment_m");
  static_assert(sizeof(AugDesc) == sizeof(zp_aug_desc) && sizeof(zp_aug_desc) == 53 * 4, "zp_aug_desc layout");
  ZP_CHECK_ARG(imgs && img_index && desc && masks && luts && beta_tab && out, "zp_augment: null pointer");
  ZP_CHECK_ARG(n_img > 0 && B > 0 && B <= 65535, "zp_augment: bad n_img %d / B %d", n_img, B);
  ZP_CHECK_ARG(H >= 8 && W >= 8 && H < (1 << 20) && W < (1 << 20),
               "zp_augment: image %d x %d (the 5 x 5 stencils' reflected borders need H, W >= 8)", H, W);
  ZP_CHECK_ARG(mh >= 1 && mw >= 1 && mh <= H && mw <= W, "zp_augment: dropout mask %d x %d for a %d x %d image", mh,
               mw, H, W);
  ZP_CHECK_ARG((long long)n_img * H * W * 3 < (1ll << 40) && (long long)B * H * W * 3 < (1ll << 40),
               "zp_augment: image stack too large");
  const int vec = (W * 3) % 4 == 0 && ((uintptr_t)out & 3) == 0;
  hipLaunchKernelGGL(k_augment, dim3((W + AUG_T - 1) / AUG_T, (H + AUG_T - 1) / AUG_T, B), dim3(256), 0,
                     (hipStream_t)stream, imgs, H, W, img_index, (const AugDesc*)desc, masks, mh, mw, luts, beta_tab,
                     bbox, out, vec, method);
  ZP_LAUNCH_CHECK("zp_augment");
  return ZP_OK;
}

extern "C" int zp_augment(const uint8_t* imgs, int n_img, int H, int W, const int* img_index, const zp_aug_desc* desc,
                          const uint8_t* masks, int mh, int mw, const uint8_t* luts, const uint8_t* beta_tab,
                          const int* bbox, int B, uint8_t* out, void* stream) {
  return zp_augment_m(imgs, n_img, H, W, img_index, desc, masks, mh, mw, luts, beta_tab, bbox, B, out, ZP_CROP_SQUARE,
                      stream);
}
