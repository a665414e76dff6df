// Shaded colour renders and the background compositor: whole synthetic training frames on the device.
// Reference: lib/meshrenderer/meshrenderer_phong.py with shader/depth_shader_phong.vs / .frag (Phong
// shading of a vertex-coloured model: per-vertex view vector, light vector and eye-space normal,
// interpolated, normalised per fragment; ambient + diffuse + specular without a shininess exponent,
// clamped at 1), and GDR_Net_Augmentation.py:37-153 (resize_short_edge, get_bg_image, replace_bg:
// a background cropped to the image's aspect, resized with cv2.INTER_LINEAR, pasted at the top-left
// of a zero image, shown wherever the optionally truncated object mask is clear).
//
// zp_render_shaded runs zp_render's visibility passes unchanged (zp_render_core.h: the same key
// plane, so the common outputs are zp_render's bit for bit) and adds two passes: k_shade_verts (one
// thread per vertex and render: camera-space position, normalised R n, normalised light vector)
// and k_shade (one thread per pixel: the winning face from the key, its exact int64 edge values at
// the sample, perspective-correct interpolation and Phong).  All shading arithmetic is f64, one
// IEEE operation per step in the order written (+ - * / sqrt only); tests/shade_ref.py restates it
// in numpy and matches bit for bit.  zp_mask_bbox is one block per mask (integer min / max, exact
// in any order); zp_composite is one thread per pixel, restating OpenCV's fixed-point bilinear
// resize for u8 (tests/synth_ref.py).  The exact semantics and the deviations from the reference are
// in include/zp.h.
#include "zp_render_core.h"

#include <float.h>

// single IEEE operations in the order written: the Makefile compiles this file with
// -ffp-contract=off; the pragma covers other build routes
#pragma clang fp contract(off)

namespace zp {

struct SVert {  // per vertex and render: camera-space position, unit normal, unit vector to the light
  double P[3], n[3], L[3];
};

// v / |v|, |v| = sqrt((x x + y y) + z z); a vector whose length is not > 0 becomes zero
__device__ __forceinline__ void unit3(const double v[3], double o[3]) {
  const double l = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const bool ok = l > 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = ok ? v[k] / l : 0.0;
}

__global__ void __launch_bounds__(256) k_shade_verts(const float* __restrict__ verts,
                                                     const float* __restrict__ normals, int nv, int B,
                                                     const double* __restrict__ R, const double* __restrict__ t,
                                                     const double* __restrict__ light, SVert* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * nv) return;
  const int b = i / nv, v = i - b * nv;
  const double* r = R + 9 * b;
  const double x = verts[3 * (size_t)v], y = verts[3 * (size_t)v + 1], z = verts[3 * (size_t)v + 2];
  const double nx = normals[3 * (size_t)v], ny = normals[3 * (size_t)v + 1], nz = normals[3 * (size_t)v + 2];
  SVert o;
  double m[3], d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.P[k] = ((r[3 * k] * x + r[3 * k + 1] * y) + r[3 * k + 2] * z) + t[3 * b + k];
    m[k] = (r[3 * k] * nx + r[3 * k + 1] * ny) + r[3 * k + 2] * nz;
    d[k] = light[6 * b + k] - o.P[k];
  }
  unit3(m, o.n);
  unit3(d, o.L);
  out[i] = o;
}

__global__ void __launch_bounds__(256) k_shade(const u64* __restrict__ keys, long long npix, int H, int W,
                                               const RVert* __restrict__ rverts, const SVert* __restrict__ sverts,
                                               int nv, const int* __restrict__ faces, int nf,
                                               const uint8_t* __restrict__ vert_rgb, const double* __restrict__ light,
                                               uint8_t* __restrict__ shaded) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const u64 key = keys[i];
  const unsigned f = 0xFFFFFFFFu - (unsigned)key;
  uint8_t o3[3] = {0, 0, 0};  // r, g, b
  const int hw = H * W;
  const int b = (int)(i / hw), rem = (int)(i - (long long)b * hw);
  const int y = rem / W, x = rem - y * W;
  RTri T;
  // a key is only ever written for a face that passed tri_setup, so this holds for every winner
  if (key != 0 && f < (unsigned)nf && tri_setup(rverts + (size_t)b * nv, faces, nv, (int)f, H, W, T)) {
    const long long sx = 256LL * x + 128, sy = 256LL * y + 128;
    const double b0 = (double)edge_at(T, 0, sx, sy) * T.w0;
    const double b1 = (double)edge_at(T, 1, sx, sy) * T.w1;
    const double b2 = (double)edge_at(T, 2, sx, sy) * T.w2;
    const double q = (b0 + b1) + b2;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    const SVert* sb = sverts + (size_t)b * nv;
    const SVert* s0 = sb + i0;
    const SVert* s1 = sb + i1;
    const SVert* s2 = sb + i2;
    double n[3], l[3], vw[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      n[k] = ((b0 * s0->n[k] + b1 * s1->n[k]) + b2 * s2->n[k]) / q;
      l[k] = ((b0 * s0->L[k] + b1 * s1->L[k]) + b2 * s2->L[k]) / q;
      vw[k] = ((b0 * -s0->P[k] + b1 * -s1->P[k]) + b2 * -s2->P[k]) / q;
      const double c0 = (double)vert_rgb[3 * (size_t)i0 + k] / 255.0, c1 = (double)vert_rgb[3 * (size_t)i1 + k] / 255.0,
                   c2 = (double)vert_rgb[3 * (size_t)i2 + k] / 255.0;
      c[k] = ((b0 * c0 + b1 * c1) + b2 * c2) / q;
    }
    double N[3], Ld[3], Vd[3], Rv[3];
    unit3(n, N);
    unit3(l, Ld);
    unit3(vw, Vd);
    const double ndl = (N[0] * Ld[0] + N[1] * Ld[1]) + N[2] * Ld[2];
    const double d = ndl > 0.0 ? ndl : 0.0;
    const double two = 2.0 * ndl;
#pragma unroll
    for (int k = 0; k < 3; ++k) Rv[k] = two * N[k] - Ld[k];
    const double rdv = (Rv[0] * Vd[0] + Rv[1] * Vd[1]) + Rv[2] * Vd[2];
    const double s = rdv > 0.0 ? rdv : 0.0;
    const double ka = light[6 * b + 3], kd = light[6 * b + 4], ks = light[6 * b + 5];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double o = (ka * c[k] + kd * (d * c[k])) + ks * (s * c[k]);
      if (o > 1.0) o = 1.0;
      const double byte = rint(255.0 * o);  // half to even
      o3[k] = byte > 0.0 ? (uint8_t)byte : (uint8_t)0;  // a negative or NaN sum (negative weights) gives 0
    }
  }
  shaded[3 * i] = o3[2];
  shaded[3 * i + 1] = o3[1];
  shaded[3 * i + 2] = o3[0];
}

inline SVert* shade_carve(void* ws, int B, int nv, int nf, int H, int W, size_t* total) {
  size_t base = 0;
  carve(ws, B, nv, nf, H, W, &base);
  if (total) *total = align256(base + (size_t)B * nv * sizeof(SVert));
  return (SVert*)((char*)ws + base);
}

// ---- mask bounding boxes -------------------------------------------------------------------------

constexpr int BB_THREADS = 1024;

__global__ void __launch_bounds__(BB_THREADS) k_mask_bbox(const uint8_t* __restrict__ mask, int H, int W,
                                                          int* __restrict__ out) {
  __shared__ int s[4];  // min row, min column, max row, max column
  const int b = blockIdx.x, hw = H * W;
  if (threadIdx.x == 0) {
    s[0] = 0x7FFFFFFF;
    s[1] = 0x7FFFFFFF;
    s[2] = -1;
    s[3] = -1;
  }
  __syncthreads();
  const uint8_t* m = mask + (size_t)b * hw;
  int r1 = 0x7FFFFFFF, c1 = 0x7FFFFFFF, r2 = -1, c2 = -1;
  for (int i = threadIdx.x; i < hw; i += BB_THREADS) {
    if (m[i]) {
      const int y = i / W, x = i - y * W;
      r1 = min(r1, y);
      c1 = min(c1, x);
      r2 = max(r2, y);
      c2 = max(c2, x);
    }
  }
  if (r2 >= 0) {
    atomicMin(&s[0], r1);
    atomicMin(&s[1], c1);
    atomicMax(&s[2], r2);
    atomicMax(&s[3], c2);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool any = s[2] >= 0;
    out[4 * b] = any ? s[0] : 0;
    out[4 * b + 1] = any ? s[1] : 0;
    out[4 * b + 2] = s[2];
    out[4 * b + 3] = s[3];
  }
}

// ---- compositor ----------------------------------------------------------------------------------

// OpenCV's INTER_LINEAR tap of destination index i over n source samples (resize.cpp, 8-bit path):
// position f32((i + 1/2) scale - 1/2), clamped to the first / last sample, weights round(w 2048)
__device__ __forceinline__ void lin_tap(int i, int n, double scale, int& s0, int& s1, int& a0, int& a1) {
  const float f = (float)(((double)i + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  float fr;
  if (fl < 0.f) {
    s0 = 0;
    fr = 0.f;
  } else if (fl >= (float)(n - 1)) {
    s0 = n - 1;
    fr = 0.f;
  } else {
    s0 = (int)fl;
    fr = f - fl;
  }
  s1 = min(s0 + 1, n - 1);
  a0 = (int)rintf((1.f - fr) * 2048.f);
  a1 = (int)rintf(fr * 2048.f);
}

// channel ch of pixel (y, x) of the cw x ch_ crop of `bg` (row stride Wb pixels) resized by f
__device__ __forceinline__ int bg_sample(const uint8_t* __restrict__ bg, int Wb, int cw, int chh, int ow, int oh,
                                         double f, int y, int x, int ch) {
  const size_t rs = (size_t)Wb * 3;
  if (ow == cw && oh == chh) return bg[y * rs + 3 * (size_t)x + ch];  // same size: a copy
  const double scale = 1.0 / f;
  if (fabs(scale - 2.0) < DBL_EPSILON) {
    // exact 2x reduction: OpenCV switches INTER_LINEAR to its INTER_AREA fast path, (a + b + c + d + 2) >> 2;
    // a block cut by the crop's last row or column averages its 1 or 2 samples, rounding half to even
    const int sy = 2 * y, sx = 2 * x;
    if (sy >= chh || sx >= cw) return 0;
    const bool fy = sy + 1 < chh, fx = sx + 1 < cw;
    const uint8_t* p = bg + sy * rs + 3 * (size_t)sx + ch;
    if (fy && fx) return ((int)p[0] + p[3] + p[rs] + p[rs + 3] + 2) >> 2;
    if (!fy && !fx) return p[0];
    const int sum = (int)p[0] + (fx ? p[3] : p[rs]);
    int h = sum >> 1;
    if (sum & 1) h += h & 1;
    return h;
  }
  int xs0, xs1, xa0, xa1, ys0, ys1, ya0, ya1;
  lin_tap(x, cw, scale, xs0, xs1, xa0, xa1);
  lin_tap(y, chh, scale, ys0, ys1, ya0, ya1);
  const uint8_t* r0 = bg + ys0 * rs + ch;
  const uint8_t* r1 = bg + ys1 * rs + ch;
  const int h0 = (int)r0[3 * (size_t)xs0] * xa0 + (int)r0[3 * (size_t)xs1] * xa1;
  const int h1 = (int)r1[3 * (size_t)xs0] * xa0 + (int)r1[3 * (size_t)xs1] * xa1;
  const int v = (((h0 >> 4) * ya0) >> 16) + (((h1 >> 4) * ya1) >> 16);
  return min(max((v + 2) >> 2, 0), 255);
}

// int(a + (b - a) u), truncating; kept inside [0, 65536] so the conversion is defined for any u
__device__ __forceinline__ int cut_at(double a, double b, double u) {
  const double v = a + (b - a) * u;
  if (!(v >= 0.0)) return 0;
  if (v > 65536.0) return 65536;
  return (int)v;
}

__global__ void __launch_bounds__(256) k_composite(const uint8_t* __restrict__ fg, const uint8_t* __restrict__ mask,
                                                   const int* __restrict__ bbox, const uint8_t* __restrict__ bgs,
                                                   int n_bg, int Hb, int Wb, const int* __restrict__ bg_index,
                                                   const int* __restrict__ bg_geo, const double* __restrict__ bg_f,
                                                   const double* __restrict__ trunc, long long npix, int H, int W,
                                                   uint8_t* __restrict__ out, uint8_t* __restrict__ mask_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const int hw = H * W;
  const int b = (int)(i / hw), rem = (int)(i - (long long)b * hw);
  const int y = rem / W, x = rem - y * W;
  bool m = mask[i] != 0;
  const int r1 = bbox[4 * b], c1 = bbox[4 * b + 1], r2 = bbox[4 * b + 2], c2 = bbox[4 * b + 3];
  const double rnd = trunc[2 * b], u = trunc[2 * b + 1];
  if (m && r2 >= 0 && c2 >= 0 && !(rnd < 0.0)) {
    const double ch = 0.5 * (double)(r1 + r2), cw = 0.5 * (double)(c1 + c2);
    if (rnd < 0.2) {
      m = y >= cut_at((double)r1, ch, u);
    } else if (rnd < 0.4) {
      m = y < cut_at(ch, (double)r2, u);
    } else if (rnd < 0.6) {
      m = x >= cut_at((double)c1, cw, u);
    } else if (rnd < 0.8) {
      m = x < cut_at(cw, (double)c2, u);
    }
  }
  if (mask_out) mask_out[i] = m ? 255 : 0;
  if (!out) return;
  int o[3] = {0, 0, 0};
  if (m) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = fg[3 * i + k];
  } else {
    const int bi = bg_index[b];
    const int cw = bg_geo[4 * b], chh = bg_geo[4 * b + 1], ow = bg_geo[4 * b + 2], oh = bg_geo[4 * b + 3];
    const double f = bg_f[b];
    // a geometry that does not fit the background stack shows no background rather than reading outside it
    const bool ok = bi >= 0 && bi < n_bg && cw >= 1 && chh >= 1 && cw <= Wb && chh <= Hb && ow >= 1 && oh >= 1 && f > 0.0;
    if (ok && x < ow && y < oh) {
      const uint8_t* bg = bgs + (size_t)bi * Hb * Wb * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) o[k] = bg_sample(bg, Wb, cw, chh, ow, oh, f, y, x, k);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3 * i + k] = (uint8_t)o[k];
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_render_shaded_ws_bytes(int B, int nv, int nf, int H, int W) {
  if (!render_sizes_ok(B, nv, nf, H, W)) return -1;
  size_t total = 0;
  shade_carve(nullptr, B, nv, nf, H, W, &total);
  return (long long)total;
}

extern "C" int zp_render_shaded(int B, const float* verts, const float* vert_normals, const uint8_t* vert_rgb, int nv,
                                const int* faces, int nf, const uint8_t* face_bgr, const double* R, const double* t,
                                const double* K, const double* light, int H, int W, double z_near, uint8_t* shaded,
                                uint8_t* color, float* depth, uint8_t* mask, int* face_out, void* ws, void* stream) {
  ZP_CHECK_ARG(B >= 1 && nv >= 1 && nf >= 1 && H >= 1 && W >= 1,
               "zp_render_shaded: B %d nv %d nf %d H %d W %d must be >= 1", B, nv, nf, H, W);
  ZP_CHECK_ARG(render_sizes_ok(B, nv, nf, H, W), "zp_render_shaded: sizes B %d nv %d nf %d H %d W %d out of range", B,
               nv, nf, H, W);
  ZP_CHECK_ARG(z_near > 0, "zp_render_shaded: z_near must be > 0");
  ZP_CHECK_ARG(verts && faces && R && t && K && ws,
               "zp_render_shaded: NULL pointer (verts, faces, R, t, K, ws are required)");
  ZP_CHECK_ARG(face_bgr || !color, "zp_render_shaded: color needs face_bgr");
  ZP_CHECK_ARG(!shaded || (vert_normals && vert_rgb && light),
               "zp_render_shaded: shaded needs vert_normals, vert_rgb and light");
  if (!shaded && !color && !depth && !mask && !face_out) return ZP_OK;
  hipStream_t st = (hipStream_t)stream;
  const RWs w = carve(ws, B, nv, nf, H, W, nullptr);
  SVert* sv = shade_carve(ws, B, nv, nf, H, W, nullptr);
  const long long npix = (long long)B * H * W;
  int rc = render_visibility(B, verts, nv, faces, nf, R, t, K, H, W, z_near, w, st);
  if (rc != ZP_OK) return rc;
  if (color || depth || mask || face_out) {
    rc = render_resolve(w, npix, face_bgr, nf, color, depth, mask, face_out, st);
    if (rc != ZP_OK) return rc;
  }
  if (shaded) {
    hipLaunchKernelGGL(k_shade_verts, dim3(ceil_div((long)B * nv, 256)), dim3(256), 0, st, verts, vert_normals, nv, B, R,
                       t, light, sv);
    ZP_LAUNCH_CHECK("zp_render_shaded verts");
    hipLaunchKernelGGL(k_shade, dim3(ceil_div(npix, 256)), dim3(256), 0, st, (const u64*)w.keys, npix, H, W,
                       (const RVert*)w.verts, (const SVert*)sv, nv, faces, nf, vert_rgb, light, shaded);
    ZP_LAUNCH_CHECK("zp_render_shaded shade");
  }
  return ZP_OK;
}

static bool image_sizes_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (long long)B * H * W <= 2147483647LL - 1024;
}

extern "C" int zp_mask_bbox(const uint8_t* mask, int B, int H, int W, int* bbox, void* stream) {
  ZP_CHECK_ARG(image_sizes_ok(B, H, W), "zp_mask_bbox: sizes B %d H %d W %d out of range", B, H, W);
  ZP_CHECK_ARG(mask && bbox, "zp_mask_bbox: NULL pointer");
  hipLaunchKernelGGL(k_mask_bbox, dim3(B), dim3(BB_THREADS), 0, (hipStream_t)stream, mask, H, W, bbox);
  ZP_LAUNCH_CHECK("zp_mask_bbox");
  return ZP_OK;
}

extern "C" int zp_composite(const uint8_t* fg, const uint8_t* mask, const int* bbox, int B, int H, int W,
                            const uint8_t* bgs, int n_bg, int Hb, int Wb, const int* bg_index, const int* bg_geo,
                            const double* bg_f, const double* trunc, uint8_t* out, uint8_t* mask_out, void* stream) {
  ZP_CHECK_ARG(image_sizes_ok(B, H, W), "zp_composite: sizes B %d H %d W %d out of range", B, H, W);
  ZP_CHECK_ARG(n_bg >= 1 && Hb >= 1 && Wb >= 1 && Hb <= 32768 && Wb <= 32768,
               "zp_composite: backgrounds n_bg %d Hb %d Wb %d out of range", n_bg, Hb, Wb);
  ZP_CHECK_ARG(fg && mask && bbox && bgs && bg_index && bg_geo && bg_f && trunc,
               "zp_composite: NULL pointer (only out and mask_out may be NULL)");
  if (!out && !mask_out) return ZP_OK;
  const long long npix = (long long)B * H * W;
  hipLaunchKernelGGL(k_composite, dim3(ceil_div(npix, 256)), dim3(256), 0, (hipStream_t)stream, fg, mask, bbox, bgs,
                     n_bg, Hb, Wb, bg_index, bg_geo, bg_f, trunc, npix, H, W, out, mask_out);
  ZP_LAUNCH_CHECK("zp_composite");
  return ZP_OK;
}
