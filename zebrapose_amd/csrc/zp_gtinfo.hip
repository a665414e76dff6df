// BOP GT masks and info on the device: zp_scene_depth composes a scene's depth from per-instance
// renders, zp_gt_info makes every instance's entire / visible mask and the counters and boxes of
// scene_gt_info.json.  Reference: lib/pysixd/visibility.py:29-36 (both visibility modes),
// lib/pysixd/misc.py:571-590 (depth_im_to_dist_im_fast) and :644-654 (calc_2d_bbox_xywh); the BOP
// toolkit's calc_gt_masks.py / calc_gt_info.py are not in the reference, so the contracts in
// include/zp.h are the specification.  tests/gtinfo_ref.py restates them in numpy.
//
// zp_scene_depth is a gather: the thread that owns four pixels of image n walks the instances in
// ascending order, reads those of image n and keeps the smallest positive depth (strictly smaller
// replaces, so a tie stays with the lowest instance).  Every depth is read once and every output
// written once; no key plane to clear and resolve, no atomics, nothing that depends on arrival order.
//
// zp_gt_info is one streaming pass over the B * Hg * Wg render, four pixels per thread and step.  Only
// a pixel inside the window that has a surface reads the scene and takes the two square roots.  The
// eleven integers per instance go thread -> wave shuffles -> LDS -> one integer atomic each per
// workgroup (skipped when the workgroup has nothing to add): exact in any order.
// This file is built with -ffp-contract=off: the distance image is specified operation by operation.
#include <limits.h>
#include <math.h>
#include "zp_common.h"

namespace zp {

constexpr int GI_NI = 11;  // px_count_all, _valid, _visib, obj x0 y0 x1 y1, vis x0 y0 x1 y1
constexpr int GI_MAX_BLOCKS = 2048;
constexpr int GI_MAX_CHUNKS = 256;

// blocks along x for `rows` slices (instances or images) of n pixels each
static int gi_chunks(int rows, long n) {
  const long groups = (n + 3) / 4;
  long cap = GI_MAX_BLOCKS / rows;
  cap = cap < 1 ? 1 : (cap > GI_MAX_CHUNKS ? GI_MAX_CHUNKS : cap);
  const long want = (groups + 255) / 256;
  return (int)(want < cap ? want : cap);
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_scene_depth(const float* __restrict__ depth, const int* __restrict__ img_index,
                                                     int B, long HW, float* __restrict__ scene,
                                                     int* __restrict__ instance) {
  const int n = blockIdx.y;
  const long groups = (HW + 3) / 4;
  float* s = scene + (size_t)n * HW;
  int* w = instance ? instance + (size_t)n * HW : nullptr;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < groups; q += (long)gridDim.x * 256) {
    const long i = 4 * q;
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int who[4] = {-1, -1, -1, -1};
    for (int b = 0; b < B; ++b) {
      if (img_index[b] != n) continue;  // the same for every thread of the block
      const float* d = depth + (size_t)b * HW + i;
      float v[4];
      if (VEC) {
        const float4 a = *reinterpret_cast<const float4*>(d);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + u < HW ? d[u] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (v[u] > 0.f && (who[u] < 0 || v[u] < best[u])) best[u] = v[u], who[u] = b;
    }
    if (VEC) {
      *reinterpret_cast<float4*>(s + i) = make_float4(best[0], best[1], best[2], best[3]);
      if (w) *reinterpret_cast<int4*>(w + i) = make_int4(who[0], who[1], who[2], who[3]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u < HW) {
          s[i + u] = best[u];
          if (w) w[i + u] = who[u];
        }
    }
  }
}

struct GiGeom {
  int Hg, Wg, ox, oy, H, W;
};

// misc.py:586-588, one IEEE operation each (as zp_bop.hip's)
__device__ __forceinline__ double gi_dist(float d, double pX, double pY) {
  const double z = (double)d;
  const double a = pX * z, c = pY * z;
  return sqrt((a * a + c * c) + z * z);
}

__device__ __forceinline__ bool gi_is_min(int k) { return k == 3 || k == 4 || k == 7 || k == 8; }

__global__ void __launch_bounds__(256) k_gt_info_init(int* __restrict__ info, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int k = i % GI_NI;
    info[i] = k < 3 ? 0 : (gi_is_min(k) ? INT_MAX : INT_MIN);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_gt_info(const float* __restrict__ gt, const float* __restrict__ test,
                                                 int n_test, const int* __restrict__ test_index, GiGeom G,
                                                 const double* __restrict__ K, float delta, int bop18,
                                                 uint8_t* __restrict__ mask, uint8_t* __restrict__ mask_visib,
                                                 int* __restrict__ info) {
  __shared__ int wred[4][GI_NI];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long HWg = (long)G.Hg * G.Wg, HW = (long)G.H * G.W;
  int ti = test_index ? test_index[b] : b;
  ti = ti < 0 ? 0 : (ti >= n_test ? n_test - 1 : ti);
  const float* g = gt + (size_t)b * HWg;
  const float* t = test + (size_t)ti * HW;
  uint8_t* m = mask ? mask + (size_t)b * HW : nullptr;
  uint8_t* mv = mask_visib ? mask_visib + (size_t)b * HW : nullptr;
  const double fx = K[4 * b], fy = K[4 * b + 1], cx = K[4 * b + 2], cy = K[4 * b + 3];

  int acc[GI_NI];
#pragma unroll
  for (int k = 0; k < GI_NI; ++k) acc[k] = k < 3 ? 0 : (gi_is_min(k) ? INT_MAX : INT_MIN);

  const long groups = (HWg + 3) / 4;
  for (long q = (long)blockIdx.x * 256 + tid; q < groups; q += (long)gridDim.x * 256) {
    const long i = 4 * q;
    float gv[4];
    if (VEC) {
      const float4 a = *reinterpret_cast<const float4*>(g + i);
      gv[0] = a.x, gv[1] = a.y, gv[2] = a.z, gv[3] = a.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[u] = i + u < HWg ? g[i + u] : 0.f;
    }
    int yg = (int)(i / G.Wg), xg = (int)(i - (long)yg * G.Wg);
    // four pixels span at most rows yg .. yg + 3: an empty group above or below the window has nothing to do
    if (gv[0] == 0.f && gv[1] == 0.f && gv[2] == 0.f && gv[3] == 0.f && (yg + 3 < G.oy || yg >= G.oy + G.H)) continue;
    // the four pixels are four consecutive window pixels when they share a row inside the window
    const bool quad = xg + 3 < G.Wg && xg >= G.ox && xg + 3 < G.ox + G.W && yg >= G.oy && yg < G.oy + G.H;
    const long wq = (long)(yg - G.oy) * G.W + (xg - G.ox);
    uint32_t pm = 0, pv = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // a pixel past the end of the render (the tail of the last group) has yg >= Hg >= oy + H: not inside
      const int x = xg - G.ox, y = yg - G.oy;
      const bool inside = (unsigned)x < (unsigned)G.W && (unsigned)y < (unsigned)G.H;
      const float d = gv[u];
      const bool surf = d > 0.f;
      if (surf) {
        ++acc[0];
        acc[3] = min(acc[3], x), acc[4] = min(acc[4], y), acc[5] = max(acc[5], x), acc[6] = max(acc[6], y);
      }
      if (inside) {
        const long wi = (long)y * G.W + x;
        bool vis = false;
        if (!(d == 0.f)) {
          const double pX = ((double)x - cx) / fx, pY = ((double)y - cy) / fy;
          const double dg = gi_dist(d, pX, pY), dt = gi_dist(t[wi], pX, pY);
          const bool within = ((float)dg - (float)dt) <= delta;
          vis = bop18 ? (within && dt > 0.0 && dg > 0.0) : ((within || dt == 0.0) && dg > 0.0);
          acc[1] += dg > 0.0 && dt > 0.0;
          if (vis) {
            ++acc[2];
            acc[7] = min(acc[7], x), acc[8] = min(acc[8], y), acc[9] = max(acc[9], x), acc[10] = max(acc[10], y);
          }
        }
        if (quad) {
          pm |= (surf ? 255u : 0u) << (8 * u);
          pv |= (vis ? 255u : 0u) << (8 * u);
        } else {
          if (m) m[wi] = surf ? 255 : 0;
          if (mv) mv[wi] = vis ? 255 : 0;
        }
      }
      if (++xg == G.Wg) xg = 0, ++yg;
    }
    if (quad) {
      if (m) {
        if (((uintptr_t)(m + wq) & 3) == 0) {
          *reinterpret_cast<uint32_t*>(m + wq) = pm;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) m[wq + u] = (uint8_t)(pm >> (8 * u));
        }
      }
      if (mv) {
        if (((uintptr_t)(mv + wq) & 3) == 0) {
          *reinterpret_cast<uint32_t*>(mv + wq) = pv;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) mv[wq + u] = (uint8_t)(pv >> (8 * u));
        }
      }
    }
  }
  if (!info) return;  // the same for every thread

  // wave -> block -> one atomic per counter
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < GI_NI; ++k) {
      const int o = __shfl_down(acc[k], off);
      acc[k] = k < 3 ? acc[k] + o : (gi_is_min(k) ? min(acc[k], o) : max(acc[k], o));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < GI_NI; ++k) wred[wave][k] = acc[k];
  }
  __syncthreads();
  if (tid < GI_NI) {
    const int a = wred[0][tid], c = wred[1][tid], d = wred[2][tid], e = wred[3][tid];
    int* dst = info + (size_t)b * GI_NI + tid;
    if (tid < 3) {
      const int s = (a + c) + (d + e);
      if (s != 0) atomicAdd(dst, s);
    } else if (gi_is_min(tid)) {
      const int s = min(min(a, c), min(d, e));
      if (s != INT_MAX) atomicMin(dst, s);
    } else {
      const int s = max(max(a, c), max(d, e));
      if (s != INT_MIN) atomicMax(dst, s);
    }
  }
}

// a box with no pixels is (-1, -1, -1, -1)
__global__ void __launch_bounds__(256) k_gt_info_final(int* __restrict__ info, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int* r = info + (size_t)b * GI_NI;
  if (r[0] == 0) r[3] = r[4] = r[5] = r[6] = -1;
  if (r[2] == 0) r[7] = r[8] = r[9] = r[10] = -1;
}

static bool gi_image_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < 2147483647LL - 1024; }

}  // namespace zp

using namespace zp;

extern "C" int zp_scene_depth(int B, const float* depth, const int* img_index, int n_img, int H, int W, float* scene,
                              int* instance, void* stream) {
  ZP_CHECK_ARG(B >= 1 && B <= 65535 && n_img >= 1 && n_img <= 65535, "zp_scene_depth: B %d, n_img %d outside [1, 65535]",
               B, n_img);
  ZP_CHECK_ARG(gi_image_ok(H, W), "zp_scene_depth: image size out of range: %d x %d", H, W);
  ZP_CHECK_ARG(depth && img_index && scene, "zp_scene_depth: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const long HW = (long)H * W;
  const dim3 grid(gi_chunks(n_img, HW), n_img);
  const bool vec = HW % 4 == 0 && (((uintptr_t)depth | (uintptr_t)scene | (uintptr_t)instance) & 15) == 0;
  if (vec) hipLaunchKernelGGL(k_scene_depth<true>, grid, dim3(256), 0, st, depth, img_index, B, HW, scene, instance);
  else hipLaunchKernelGGL(k_scene_depth<false>, grid, dim3(256), 0, st, depth, img_index, B, HW, scene, instance);
  ZP_LAUNCH_CHECK("zp_scene_depth");
  return ZP_OK;
}

extern "C" int zp_gt_info(int B, const float* depth_gt, int Hg, int Wg, int ox, int oy, int H, int W,
                          const float* depth_test, int n_test, const int* test_index, const double* K, double delta,
                          int visib_mode, uint8_t* mask, uint8_t* mask_visib, int* info, void* stream) {
  ZP_CHECK_ARG(B >= 1 && B <= 65535, "zp_gt_info: B %d outside [1, 65535]", B);
  ZP_CHECK_ARG(gi_image_ok(Hg, Wg) && gi_image_ok(H, W), "zp_gt_info: sizes out of range: render %d x %d, image %d x %d", Hg,
               Wg, H, W);
  ZP_CHECK_ARG(ox >= 0 && oy >= 0 && (long long)ox + W <= Wg && (long long)oy + H <= Hg,
               "zp_gt_info: window %d x %d at (%d, %d) leaves the %d x %d render", H, W, ox, oy, Hg, Wg);
  ZP_CHECK_ARG(visib_mode == ZP_VISIB_BOP19 || visib_mode == ZP_VISIB_BOP18, "zp_gt_info: visib_mode %d", visib_mode);
  ZP_CHECK_ARG(n_test >= 1 && (test_index || n_test >= B), "zp_gt_info: n_test %d (B %d, %s test_index)", n_test, B,
               test_index ? "with" : "without");
  ZP_CHECK_ARG(depth_gt && depth_test && K, "zp_gt_info: NULL pointer");
  if (!mask && !mask_visib && !info) return ZP_OK;
  hipStream_t st = (hipStream_t)stream;
  const long HWg = (long)Hg * Wg;
  const GiGeom G = {Hg, Wg, ox, oy, H, W};
  if (info) {
    hipLaunchKernelGGL(k_gt_info_init, dim3((B * GI_NI + 255) / 256), dim3(256), 0, st, info, B * GI_NI);
    ZP_LAUNCH_CHECK("zp_gt_info init");
  }
  const dim3 grid(gi_chunks(B, HWg), B);
  const bool vec = HWg % 4 == 0 && ((uintptr_t)depth_gt & 15) == 0;
  const float fdelta = (float)delta;
  const int bop18 = visib_mode == ZP_VISIB_BOP18;
  if (vec)
    hipLaunchKernelGGL(k_gt_info<true>, grid, dim3(256), 0, st, depth_gt, depth_test, n_test, test_index, G, K, fdelta,
                       bop18, mask, mask_visib, info);
  else
    hipLaunchKernelGGL(k_gt_info<false>, grid, dim3(256), 0, st, depth_gt, depth_test, n_test, test_index, G, K, fdelta,
                       bop18, mask, mask_visib, info);
  ZP_LAUNCH_CHECK("zp_gt_info");
  if (info) {
    hipLaunchKernelGGL(k_gt_info_final, dim3((B + 255) / 256), dim3(256), 0, st, info, B);
    ZP_LAUNCH_CHECK("zp_gt_info final");
  }
  return ZP_OK;
}
