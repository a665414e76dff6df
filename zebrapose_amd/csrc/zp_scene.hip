// Scene compositor: zp_scene_compose turns the per-instance renders of a batch of scenes (depth and
// shaded colour, as zp_render_shaded writes them) into each scene's colour image, foreground mask,
// depth and instance map, and every instance's exact visible mask, pixel counts and visible box.
// There is no reference program: the reference takes such frames from BlenderProc.  The contract is
// in include/zp.h; tests/scene_ref.py restates it in numpy and every output matches it bit for bit.
//
// The winner of a pixel is zp_scene_depth's (zp_gtinfo.hip): a surface is depth > 0, the nearest one
// wins, strictly smaller replaces, so a tie stays with the lowest instance.  A gather like that
// kernel: the thread that owns a few pixels of image n walks the instances in ascending order and
// reads those of image n (a scan of img_index over all B, the same for every thread of the block).
//
// Main pass, k_scene_compose: a thread owns SC_ITEMS items of V pixels (V = 4 consecutive pixels of
// one row with 16-byte depth loads when W % 4 == 0 and the pointers allow, V = 1 otherwise), items
// a block apart so that every load and store is coalesced across the wave.  Walk 1 reads each depth
// once, keeps the winner and its colour (the 12 colour bytes of an item are read only where the
// instance takes a pixel) and counts the instance's surface pixels.  The per-image outputs are
// written once.  Walk 2 reads nothing: per instance of the image it writes the visible mask (every
// byte, zeros included) and counts the pixels won and their box.  Counters: per-thread integers ->
// wave shuffles -> one integer atomic per wave, instance and counter that has something to add, on
// the raw counters in ws: integer sums, minima and maxima, exact in any order.
// k_scene_orphans covers the instances of no image (img_index outside [0, n_img)): it clears their
// visible masks and counts their surface pixels; such an instance is never used as an index.
// k_scene_init / k_scene_final initialise the raw counters and turn them into info.
#include <limits.h>
#include "zp_common.h"

namespace zp {

constexpr int SC_ITEMS = 4;   // items per thread in the main pass
constexpr int SC_NI = 6;      // px_all, px_visib, r1, c1, r2, c2
constexpr int SC_ORPHAN_CHUNKS = 64;

__device__ __forceinline__ int sc_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}
__device__ __forceinline__ int sc_wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_down(v, off));
  return v;
}
__device__ __forceinline__ int sc_wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_down(v, off));
  return v;
}

__global__ void __launch_bounds__(256) k_scene_init(int* __restrict__ cnt, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int k = i % SC_NI;
    cnt[i] = k < 2 ? 0 : (k < 4 ? INT_MAX : INT_MIN);
  }
}

// an empty visible mask has the box (0, 0, -1, -1), as zp_mask_bbox
__global__ void __launch_bounds__(256) k_scene_final(const int* __restrict__ cnt, int* __restrict__ info, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int* c = cnt + (size_t)b * SC_NI;
  int* r = info + (size_t)b * SC_NI;
  const bool any = c[1] > 0;
  r[0] = c[0];
  r[1] = c[1];
  r[2] = any ? c[2] : 0;
  r[3] = any ? c[3] : 0;
  r[4] = any ? c[4] : -1;
  r[5] = any ? c[5] : -1;
}

// blockIdx.y = instance; only the blocks of an instance that belongs to no image do anything
__global__ void __launch_bounds__(256) k_scene_orphans(const float* __restrict__ depth, const int* __restrict__ img_index,
                                                       int n_img, long HW, uint8_t* __restrict__ mask_visib,
                                                       int* __restrict__ cnt) {
  const int b = blockIdx.y;
  const int n = img_index[b];
  if (n >= 0 && n < n_img) return;  // the same for every thread of the block
  const float* d = depth + (size_t)b * HW;
  uint8_t* mv = mask_visib ? mask_visib + (size_t)b * HW : nullptr;
  int all = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
    if (mv) mv[i] = 0;
    if (cnt) all += d[i] > 0.f;
  }
  if (!cnt) return;
  all = sc_wave_sum(all);
  if ((threadIdx.x & 63) == 0 && all != 0) atomicAdd(cnt + (size_t)b * SC_NI, all);
}

template <int V>
__global__ void __launch_bounds__(256) k_scene_compose(int B, long HW, int W, const float* __restrict__ depth,
                                                       const uint8_t* __restrict__ shaded,
                                                       const int* __restrict__ img_index, uint8_t* __restrict__ image,
                                                       uint8_t* __restrict__ fg, float* __restrict__ scene,
                                                       int* __restrict__ instance, uint8_t* __restrict__ mask_visib,
                                                       int* __restrict__ cnt) {
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const long items = HW / V;  // V == 4 only when HW % 4 == 0
  const bool want_col = image != nullptr;

  long px[SC_ITEMS];   // first pixel of the item
  bool on[SC_ITEMS];   // the item exists
  float best[SC_ITEMS][V];
  int who[SC_ITEMS][V];
  uint32_t col[SC_ITEMS][V];  // the winner's B | G << 8 | R << 16
#pragma unroll
  for (int g = 0; g < SC_ITEMS; ++g) {
    const long q = ((long)blockIdx.x * SC_ITEMS + g) * 256 + tid;
    on[g] = q < items;
    px[g] = q * V;
#pragma unroll
    for (int u = 0; u < V; ++u) best[g][u] = 0.f, who[g][u] = -1, col[g][u] = 0u;
  }

  // walk 1: the winner, its colour, and each instance's surface count
  for (int b = 0; b < B; ++b) {
    if (img_index[b] != n) continue;  // the same for every thread of the block
    const float* d = depth + (size_t)b * HW;
    const uint8_t* s = want_col ? shaded + (size_t)b * HW * 3 : nullptr;
    int all = 0;
#pragma unroll
    for (int g = 0; g < SC_ITEMS; ++g) {
      float v[V];
      if constexpr (V == 4) {
        const float4 a = on[g] ? *reinterpret_cast<const float4*>(d + px[g]) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
      } else {
        v[0] = on[g] ? d[px[g]] : 0.f;
      }
      bool take[V], any = false;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const bool surf = v[u] > 0.f;
        all += surf;
        take[u] = surf && (who[g][u] < 0 || v[u] < best[g][u]);
        any |= take[u];
        if (take[u]) best[g][u] = v[u], who[g][u] = b;
      }
      if (want_col && any) {
        uint32_t c[V];
        if constexpr (V == 4) {
          const uint32_t* w = reinterpret_cast<const uint32_t*>(s + px[g] * 3);
          const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
          c[0] = w0 & 0xFFFFFFu;
          c[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
          c[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
          c[3] = w2 >> 8;
        } else {
          const uint8_t* p = s + px[g] * 3;
          c[0] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
#pragma unroll
        for (int u = 0; u < V; ++u)
          if (take[u]) col[g][u] = c[u];
      }
    }
    if (cnt) {
      all = sc_wave_sum(all);
      if (lane == 0 && all != 0) atomicAdd(cnt + (size_t)b * SC_NI, all);
    }
  }

  // the per-image outputs, once
#pragma unroll
  for (int g = 0; g < SC_ITEMS; ++g) {
    if (!on[g]) continue;
    const size_t o = (size_t)n * HW + px[g];
    if constexpr (V == 4) {
      if (scene) *reinterpret_cast<float4*>(scene + o) = make_float4(best[g][0], best[g][1], best[g][2], best[g][3]);
      if (instance) *reinterpret_cast<int4*>(instance + o) = make_int4(who[g][0], who[g][1], who[g][2], who[g][3]);
      if (fg) {
        uint32_t m = 0;
#pragma unroll
        for (int u = 0; u < V; ++u) m |= (who[g][u] >= 0 ? 255u : 0u) << (8 * u);
        *reinterpret_cast<uint32_t*>(fg + o) = m;
      }
      if (image) {
        uint32_t* w = reinterpret_cast<uint32_t*>(image + o * 3);
        w[0] = col[g][0] | (col[g][1] << 24);
        w[1] = (col[g][1] >> 8) | (col[g][2] << 16);
        w[2] = (col[g][2] >> 16) | (col[g][3] << 8);
      }
    } else {
      if (scene) scene[o] = best[g][0];
      if (instance) instance[o] = who[g][0];
      if (fg) fg[o] = who[g][0] >= 0 ? 255 : 0;
      if (image) {
        uint8_t* p = image + o * 3;
        p[0] = (uint8_t)col[g][0], p[1] = (uint8_t)(col[g][0] >> 8), p[2] = (uint8_t)(col[g][0] >> 16);
      }
    }
  }
  if (!mask_visib && !cnt) return;  // the same for every thread

  // walk 2: each instance's visible mask, pixels won and box; no loads
  int row[SC_ITEMS], colx[SC_ITEMS];
#pragma unroll
  for (int g = 0; g < SC_ITEMS; ++g) {
    row[g] = on[g] ? (int)(px[g] / W) : 0;
    colx[g] = on[g] ? (int)(px[g] - (long)row[g] * W) : 0;
  }
  for (int b = 0; b < B; ++b) {
    if (img_index[b] != n) continue;
    uint8_t* mv = mask_visib ? mask_visib + (size_t)b * HW : nullptr;
    int vis = 0, r1 = INT_MAX, c1 = INT_MAX, r2 = INT_MIN, c2 = INT_MIN;
#pragma unroll
    for (int g = 0; g < SC_ITEMS; ++g) {
      if (!on[g]) continue;
      uint32_t m = 0;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        if (who[g][u] == b) {  // the V pixels of an item share a row (W % 4 == 0 when V == 4)
          m |= 255u << (8 * u);
          ++vis;
          r1 = min(r1, row[g]), r2 = max(r2, row[g]);
          c1 = min(c1, colx[g] + u), c2 = max(c2, colx[g] + u);
        }
      }
      if (mv) {
        if constexpr (V == 4) *reinterpret_cast<uint32_t*>(mv + px[g]) = m;
        else mv[px[g]] = (uint8_t)m;
      }
    }
    if (cnt) {  // every lane of the wave is here: the loops above are uniform
      vis = sc_wave_sum(vis);
      r1 = sc_wave_min(r1), c1 = sc_wave_min(c1);
      r2 = sc_wave_max(r2), c2 = sc_wave_max(c2);
      if (lane == 0 && vis != 0) {
        int* c = cnt + (size_t)b * SC_NI;
        atomicAdd(c + 1, vis);
        atomicMin(c + 2, r1);
        atomicMin(c + 3, c1);
        atomicMax(c + 4, r2);
        atomicMax(c + 5, c2);
      }
    }
  }
}

static bool sc_sizes_ok(int B, int n_img, int H, int W) {
  const long long lim = 2147483647LL - 1024;
  return B >= 1 && B <= 65535 && n_img >= 1 && n_img <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 &&
         (long long)B * H * W <= lim && (long long)n_img * H * W <= lim;
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_scene_compose_ws_bytes(int B, int n_img, int H, int W) {
  if (!sc_sizes_ok(B, n_img, H, W)) return -1;
  return (long long)(((size_t)B * SC_NI * sizeof(int) + 255) & ~(size_t)255);
}

extern "C" int zp_scene_compose(int B, int n_img, int H, int W, const float* depth, const uint8_t* shaded,
                                const int* img_index, uint8_t* image, uint8_t* fg, float* scene, int* instance,
                                uint8_t* mask_visib, int* info, void* ws, void* stream) {
  ZP_CHECK_ARG(sc_sizes_ok(B, n_img, H, W), "zp_scene_compose: sizes out of range: B %d, n_img %d, %d x %d", B, n_img, H,
               W);
  ZP_CHECK_ARG(depth && img_index, "zp_scene_compose: NULL pointer");
  ZP_CHECK_ARG(!image || shaded, "zp_scene_compose: image needs shaded");
  ZP_CHECK_ARG(!info || ws, "zp_scene_compose: info needs the workspace");
  if (!image && !fg && !scene && !instance && !mask_visib && !info) return ZP_OK;
  hipStream_t st = (hipStream_t)stream;
  const long HW = (long)H * W;
  int* cnt = info ? (int*)ws : nullptr;
  if (cnt) {
    hipLaunchKernelGGL(k_scene_init, dim3((B * SC_NI + 255) / 256), dim3(256), 0, st, cnt, B * SC_NI);
    ZP_LAUNCH_CHECK("zp_scene_compose init");
  }
  if (cnt || mask_visib) {
    const long want = (HW + 255) / 256;
    const dim3 grid((unsigned)(want < SC_ORPHAN_CHUNKS ? want : SC_ORPHAN_CHUNKS), B);
    hipLaunchKernelGGL(k_scene_orphans, grid, dim3(256), 0, st, depth, img_index, n_img, HW, mask_visib, cnt);
    ZP_LAUNCH_CHECK("zp_scene_compose orphans");
  }
  // the 4-pixel form: rows of whole items, 16-byte depth / scene / instance, 4-byte colour and masks
  const uintptr_t a16 = (uintptr_t)depth | (uintptr_t)scene | (uintptr_t)instance;
  const uintptr_t a4 = (uintptr_t)shaded | (uintptr_t)image | (uintptr_t)fg | (uintptr_t)mask_visib;
  const bool vec = W % 4 == 0 && (a16 & 15) == 0 && (a4 & 3) == 0;
  const uint8_t* sh = image ? shaded : nullptr;
  if (vec) {
    const dim3 grid((unsigned)((HW / 4 + 256 * SC_ITEMS - 1) / (256 * SC_ITEMS)), n_img);
    hipLaunchKernelGGL(k_scene_compose<4>, grid, dim3(256), 0, st, B, HW, W, depth, sh, img_index, image, fg, scene,
                       instance, mask_visib, cnt);
  } else {
    const dim3 grid((unsigned)((HW + 256 * SC_ITEMS - 1) / (256 * SC_ITEMS)), n_img);
    hipLaunchKernelGGL(k_scene_compose<1>, grid, dim3(256), 0, st, B, HW, W, depth, sh, img_index, image, fg, scene,
                       instance, mask_visib, cnt);
  }
  ZP_LAUNCH_CHECK("zp_scene_compose");
  if (cnt) {
    hipLaunchKernelGGL(k_scene_final, dim3((B + 255) / 256), dim3(256), 0, st, cnt, info, B);
    ZP_LAUNCH_CHECK("zp_scene_compose final");
  }
  return ZP_OK;
}
