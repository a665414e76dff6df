// Code -> vertex decode on gfx950: logits -> mask / code bits -> 16-bit class id -> LUT
// gather -> row-major compaction of the mask pixels -> original-image coordinates.
//
// Reference (lyltc1/ZebraPose):
//   common_ops.py:5-19                               sigmoid(x) > 0.5 (CPU fp32) == x > 8.940696716308594e-08f
//   class_id_encoder_decoder.py:17-28                id = sum_i bit_i * 2^(L-1-i)  (channel 0 = MSB)
//   CNN_output_to_pose.py:53-64                      P2D = (x, y) of mask.nonzero() (row-major),
//                                                    P3D = LUT[id], NaN rows -> [0,0,0] (kept)
//   CNN_output_to_pose.py:67-91                      unique form: one row per class id in first-pixel
//                                                    order, P2D = f64 mean of the class's pixels
//   CNN_output_to_pose.py:34-50                      x' = int(Bbox[2]/Bbox_Size * x + Bbox[0]) (f64, trunc)
//   CNN_output_to_pose.py:128-129                    P2D/P3D cast to float32 for PnP
//   generate_new_dict.py:4-33                        ignore_bit LUT = f64 mean of the 2^k children
//   common_ops.py:21-28 ('CE')                       digit_i = argmax_k softmax(code[i * d .. i * d + d))_k
//   class_id_encoder_decoder.py:17-28 (class_base d) id = sum_i digit_i * d^(L-1-i)
//
// Two passes over tiles of 1024 pixels: (1) ids + per-tile mask counts, (2) per-tile
// offsets (prefix over the crop's earlier tiles) + block scan + ordered writes.
#include "zp_common.h"

namespace zp {

constexpr int DEC_TILE = 1024;  // pixels per tile (256 threads x 4)
constexpr float kHalfLogit = 8.940696716308594e-08f;

__global__ void __launch_bounds__(256) k_decode_ids(const float* __restrict__ mlog, const float* __restrict__ clog, int HW,
                                                    int Lfull, int L, int* __restrict__ packed, int* __restrict__ ids,
                                                    int* __restrict__ tile_cnt, int tiles) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const int p0 = tile * DEC_TILE + threadIdx.x * 4;
  __shared__ int wsum[4];
  int cnt = 0;
  const float* mrow = mlog + (size_t)b * HW;
  const float* crow = clog + (size_t)b * Lfull * HW;
  if (p0 + 3 < HW && (HW & 3) == 0) {
    float4 m = *(const float4*)(mrow + p0);
    int id[4] = {0, 0, 0, 0};
    for (int i = 0; i < L; ++i) {
      float4 c = *(const float4*)(crow + (size_t)i * HW + p0);
      id[0] = (id[0] << 1) | (c.x > kHalfLogit);
      id[1] = (id[1] << 1) | (c.y > kHalfLogit);
      id[2] = (id[2] << 1) | (c.z > kHalfLogit);
      id[3] = (id[3] << 1) | (c.w > kHalfLogit);
    }
    int mb[4] = {m.x > kHalfLogit, m.y > kHalfLogit, m.z > kHalfLogit, m.w > kHalfLogit};
    int4 pk = make_int4(mb[0] ? id[0] : -1, mb[1] ? id[1] : -1, mb[2] ? id[2] : -1, mb[3] ? id[3] : -1);
    *(int4*)(packed + (size_t)b * HW + p0) = pk;
    if (ids) *(int4*)(ids + (size_t)b * HW + p0) = make_int4(id[0], id[1], id[2], id[3]);
    cnt = mb[0] + mb[1] + mb[2] + mb[3];
  } else {
    for (int k = 0; k < 4; ++k) {
      int p = p0 + k;
      if (p >= HW) break;
      int id = 0;
      for (int i = 0; i < L; ++i) id = (id << 1) | (crow[(size_t)i * HW + p] > kHalfLogit);
      int mb = mrow[p] > kHalfLogit;
      packed[(size_t)b * HW + p] = mb ? id : -1;
      if (ids) ids[(size_t)b * HW + p] = id;
      cnt += mb;
    }
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[b * tiles + tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void __launch_bounds__(256) k_decode_emit(const int* __restrict__ packed, const int* __restrict__ tile_cnt,
                                                     int tiles, int H, int W, size_t lut_floats,
                                                     const float* __restrict__ lut,
                                                     const int* __restrict__ lut_index, const int* __restrict__ bbox,
                                                     int bbox_size, int* __restrict__ counts, int* __restrict__ xy,
                                                     float* __restrict__ xyz) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const int HW = H * W;
  __shared__ int scan[256];
  __shared__ int base_s;
  if (threadIdx.x == 0) {
    int base = 0, total = 0;
    for (int t = 0; t < tiles; ++t) {
      int c = tile_cnt[b * tiles + t];
      if (t < tile) base += c;
      total += c;
    }
    base_s = base;
    if (tile == 0) counts[b] = total;
  }
  const int p0 = tile * DEC_TILE + threadIdx.x * 4;
  int v[4];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int p = p0 + k;
    v[k] = p < HW ? packed[(size_t)b * HW + p] : -1;
    mine += v[k] >= 0;
  }
  scan[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    int t = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
    __syncthreads();
    scan[threadIdx.x] += t;
    __syncthreads();
  }
  int pos = base_s + scan[threadIdx.x] - mine;
  const double bx = bbox[b * 4 + 0], by = bbox[b * 4 + 1];
  const double rx = (double)bbox[b * 4 + 2] / (double)bbox_size;
  const double ry = (double)bbox[b * 4 + 3] / (double)bbox_size;
  const float* L3 = lut + (size_t)(lut_index ? lut_index[b] : 0) * lut_floats;  // (3 floats per class id)
  int* oxy = xy + (size_t)b * HW * 2;
  float* oxyz = xyz + (size_t)b * HW * 3;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v[k] < 0) continue;
    int p = p0 + k;
    int py = p / W, px = p - py * W;
    // f64 multiply then add, no FMA contraction (numpy order); astype('int') truncates toward zero
    oxy[2 * pos] = (int)__dadd_rn(__dmul_rn(rx, (double)px), bx);
    oxy[2 * pos + 1] = (int)__dadd_rn(__dmul_rn(ry, (double)py), by);
    float a = L3[(size_t)v[k] * 3], c = L3[(size_t)v[k] * 3 + 1], d = L3[(size_t)v[k] * 3 + 2];
    if (isnan(a) || isnan(c) || isnan(d)) a = c = d = 0.f;
    oxyz[3 * pos] = a;
    oxyz[3 * pos + 1] = c;
    oxyz[3 * pos + 2] = d;
    ++pos;
  }
}

// argmax over the d class logits of step i at four consecutive pixels (planes HW apart): the first
// maximum wins (np.argmax, common_ops.py:26), a NaN never does.  softmax is monotonic, so the argmax
// of the logits is the argmax of the reference's probabilities wherever the top two logits differ by
// more than the f32 softmax's rounding.
__device__ __forceinline__ void digits4(const float* __restrict__ x, size_t HW, int d, int n, bool vec, int* dg) {
  float best[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    best[q] = 0.f;
    dg[q] = 0;
  }
  for (int k = 0; k < d; ++k) {
    const float* xr = x + (size_t)k * HW;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      const float4 t = *(const float4*)xr;
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
      for (int q = 0; q < n; ++q) v[q] = xr[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k == 0 || v[q] > best[q]) {
        best[q] = v[q];
        dg[q] = k;
      }
  }
}

// digit planes of d-ary code logits [B][L * d][HW] -> [B][L][HW] (u8, or f64 like the reference's
// numpy result); one thread per (b, i, 4 pixels)
__global__ void __launch_bounds__(256) k_code_digits(const float* __restrict__ clog, int HW, int L, int d, int out_f64,
                                                     void* __restrict__ out) {
  const int b = blockIdx.z, i = blockIdx.y;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= HW) return;
  const int n = min(4, HW - p0);
  const bool vec = n == 4 && (HW & 3) == 0;
  int dg[4];
  digits4(clog + ((size_t)(b * L + i) * d) * HW + p0, (size_t)HW, d, n, vec, dg);
  const size_t o = (size_t)(b * L + i) * HW + p0;
  for (int q = 0; q < n; ++q) {
    if (out_f64) ((double*)out)[o + q] = (double)dg[q];
    else ((uint8_t*)out)[o + q] = (uint8_t)dg[q];
  }
}

// k_decode_ids for d-ary codes: id = sum_i digit_i * d^(L-1-i) (Horner), same packed / ids / tile counts
__global__ void __launch_bounds__(256) k_decode_ids_radix(const float* __restrict__ mlog, const float* __restrict__ clog,
                                                          int HW, int L, int d, int* __restrict__ packed,
                                                          int* __restrict__ ids, int* __restrict__ tile_cnt, int tiles) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const int p0 = tile * DEC_TILE + threadIdx.x * 4;
  __shared__ int wsum[4];
  int cnt = 0;
  if (p0 < HW) {
    const int n = min(4, HW - p0);
    const bool vec = n == 4 && (HW & 3) == 0;
    int id[4] = {0, 0, 0, 0};
    for (int i = 0; i < L; ++i) {
      int dg[4];
      digits4(clog + ((size_t)(b * L + i) * d) * HW + p0, (size_t)HW, d, n, vec, dg);
#pragma unroll
      for (int q = 0; q < 4; ++q) id[q] = id[q] * d + dg[q];
    }
    for (int q = 0; q < n; ++q) {
      const int mb = mlog[(size_t)b * HW + p0 + q] > kHalfLogit;
      packed[(size_t)b * HW + p0 + q] = mb ? id[q] : -1;
      if (ids) ids[(size_t)b * HW + p0 + q] = id[q];
      cnt += mb;
    }
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[b * tiles + tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ---- unique correspondences (CNN_output_to_pose.py:67-91): one row per decoded class ----------
// Per crop an open-addressed table of T = 2^logT >= 2 * HW slots (keys: class id, -1 = empty;
// first: lowest pixel index of the class, as unsigned, 0xFFFFFFFF = none) and three integer
// accumulators per pixel (n, sum x, sum y), used at the class's first pixel.  Everything that
// depends on arrival order is an integer min or sum, so the result does not.

__device__ __forceinline__ uint32_t uq_hash(int id, int logT) { return ((uint32_t)id * 2654435761u) >> (32 - logT); }

// pass 0: keys / first <- all ones (empty, no pixel), the accumulators behind them <- 0
__global__ void __launch_bounds__(256) k_unique_init(int* __restrict__ tab, size_t n_ones, size_t n_all) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_all; i += (size_t)gridDim.x * 256) tab[i] = i < n_ones ? -1 : 0;
}

// pass 1: claim the class's slot, lower its first pixel; packed[p] <- slot (or stays -1)
__global__ void __launch_bounds__(256) k_unique_insert(int* __restrict__ packed, int HW, int logT, int* __restrict__ keys,
                                                       unsigned* __restrict__ first) {
  const int b = blockIdx.y;
  const uint32_t T = 1u << logT;
  int* kb = keys + ((size_t)b << logT);
  unsigned* fb = first + ((size_t)b << logT);
  const int p0 = blockIdx.x * DEC_TILE + threadIdx.x * 4;
  for (int k = 0; k < 4; ++k) {
    const int p = p0 + k;
    if (p >= HW) break;
    const int v = packed[(size_t)b * HW + p];
    if (v < 0) continue;
    uint32_t h = uq_hash(v, logT);
    int slot = -1;
    for (uint32_t i = 0; i < T; ++i) {  // at most HW < T keys per crop: an empty slot is always met
      const int prev = atomicCAS(&kb[h], -1, v);
      if (prev == -1 || prev == v) {
        slot = (int)h;
        break;
      }
      h = (h + 1) & (T - 1);
    }
    if (slot >= 0) atomicMin(&fb[slot], (unsigned)p);
    packed[(size_t)b * HW + p] = slot;
  }
}

// pass 2: add every pixel into the accumulators of its class's first pixel; count the heads per tile
__global__ void __launch_bounds__(256) k_unique_accum(const int* __restrict__ slots, int HW, int W, int logT,
                                                      const unsigned* __restrict__ first, int* __restrict__ acc_n,
                                                      int* __restrict__ acc_x, int* __restrict__ acc_y,
                                                      int* __restrict__ head_cnt, int tiles) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const unsigned* fb = first + ((size_t)b << logT);
  const int p0 = tile * DEC_TILE + threadIdx.x * 4;
  __shared__ int wsum[4];
  int cnt = 0;
  for (int k = 0; k < 4; ++k) {
    const int p = p0 + k;
    if (p >= HW) break;
    const int s = slots[(size_t)b * HW + p];
    if (s < 0) continue;
    const int f = (int)fb[s];  // <= p: this pixel lowered it in pass 1
    if ((unsigned)f >= (unsigned)HW) continue;
    const int py = p / W, px = p - py * W;
    const size_t o = (size_t)b * HW + f;
    atomicAdd(&acc_n[o], 1);
    atomicAdd(&acc_x[o], px);
    atomicAdd(&acc_y[o], py);
    cnt += f == p;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) head_cnt[b * tiles + tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// pass 3: k_decode_emit over the heads (a pixel that is its class's first), in row-major order
__global__ void __launch_bounds__(256) k_unique_emit(const int* __restrict__ slots, const int* __restrict__ head_cnt,
                                                     int tiles, int H, int W, int logT, const int* __restrict__ keys,
                                                     const unsigned* __restrict__ first, const int* __restrict__ acc_n,
                                                     const int* __restrict__ acc_x, const int* __restrict__ acc_y,
                                                     size_t lut_floats, const float* __restrict__ lut,
                                                     const int* __restrict__ lut_index, const int* __restrict__ bbox,
                                                     int bbox_size, int* __restrict__ counts, int* __restrict__ xy,
                                                     float* __restrict__ xyz, int* __restrict__ mult,
                                                     double* __restrict__ mean_xy) {
  // every f64 operation of this kernel is rounded on its own.  The __dmul_rn / __dadd_rn wrappers do
  // not ensure that: they inline to a plain multiply and add, which the compiler contracts into an FMA.
#pragma clang fp contract(off)
  const int b = blockIdx.y, tile = blockIdx.x;
  const int HW = H * W;
  __shared__ int scan[256];
  __shared__ int base_s;
  if (threadIdx.x == 0) {
    int base = 0, total = 0;
    for (int t = 0; t < tiles; ++t) {
      int c = head_cnt[b * tiles + t];
      if (t < tile) base += c;
      total += c;
    }
    base_s = base;
    if (tile == 0) counts[b] = total;
  }
  const int* kb = keys + ((size_t)b << logT);
  const unsigned* fb = first + ((size_t)b << logT);
  const int p0 = tile * DEC_TILE + threadIdx.x * 4;
  int v[4];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = p0 + k;
    const int s = p < HW ? slots[(size_t)b * HW + p] : -1;
    v[k] = (s >= 0 && (int)fb[s] == p) ? kb[s] : -1;
    mine += v[k] >= 0;
  }
  scan[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    int t = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
    __syncthreads();
    scan[threadIdx.x] += t;
    __syncthreads();
  }
  int pos = base_s + scan[threadIdx.x] - mine;
  const double bx = bbox[b * 4 + 0], by = bbox[b * 4 + 1];
  const double rx = (double)bbox[b * 4 + 2] / (double)bbox_size;
  const double ry = (double)bbox[b * 4 + 3] / (double)bbox_size;
  const float* L3 = lut + (size_t)(lut_index ? lut_index[b] : 0) * lut_floats;
  int* oxy = xy + (size_t)b * HW * 2;
  float* oxyz = xyz + (size_t)b * HW * 3;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v[k] < 0) continue;
    const size_t o = (size_t)b * HW + p0 + k;
    const int n = acc_n[o];
    // exact integer sums, one correctly rounded division per axis; then multiply, add (no FMA), truncate
    const double mx = (double)acc_x[o] / (double)n;
    const double my = (double)acc_y[o] / (double)n;
    const double tx = rx * mx, ty = ry * my;
    oxy[2 * pos] = (int)(tx + bx);
    oxy[2 * pos + 1] = (int)(ty + by);
    float a = L3[(size_t)v[k] * 3], c = L3[(size_t)v[k] * 3 + 1], d = L3[(size_t)v[k] * 3 + 2];
    if (isnan(a) || isnan(c) || isnan(d)) a = c = d = 0.f;
    oxyz[3 * pos] = a;
    oxyz[3 * pos + 1] = c;
    oxyz[3 * pos + 2] = d;
    if (mult) mult[(size_t)b * HW + pos] = n;
    if (mean_xy) {
      mean_xy[((size_t)b * HW + pos) * 2] = mx;
      mean_xy[((size_t)b * HW + pos) * 2 + 1] = my;
    }
    ++pos;
  }
}

__global__ void k_lut_coarsen(const double* __restrict__ lut, int k, int n_new, float* __restrict__ out) {
  int nid = blockIdx.x * blockDim.x + threadIdx.x;
  if (nid >= n_new) return;
  double s0 = 0, s1 = 0, s2 = 0;
  const int nch = 1 << k;
  for (int c = 0; c < nch; ++c) {
    const double* r = lut + ((size_t)nid * nch + c) * 3;
    s0 = s0 + r[0];
    s1 = s1 + r[1];
    s2 = s2 + r[2];
  }
  out[(size_t)nid * 3] = (float)(s0 / nch);
  out[(size_t)nid * 3 + 1] = (float)(s1 / nch);
  out[(size_t)nid * 3 + 2] = (float)(s2 / nch);
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_decode_ws_bytes(int B, int H, int W) {
  long long HW = (long long)H * W;
  long long tiles = (HW + DEC_TILE - 1) / DEC_TILE;
  return (long long)B * HW * 4 + (long long)B * tiles * 4 + 256;
}

extern "C" int zp_decode(const float* mask_logits, const float* code_logits, int B, int H, int W, int Lfull, int L,
                         const float* lut, const int* lut_index, const int* bbox, int bbox_size, int* ids, int* counts,
                         int* xy, float* xyz, void* ws, void* stream) {
  ZP_CHECK_ARG(mask_logits && code_logits && lut && bbox && counts && xy && xyz && ws, "zp_decode: null pointer");
  ZP_CHECK_ARG(B > 0 && H > 0 && W > 0 && L >= 1 && L <= 24 && L <= Lfull && bbox_size > 0, "zp_decode: bad sizes");
  const int HW = H * W;
  const int tiles = (HW + DEC_TILE - 1) / DEC_TILE;
  int* packed = (int*)ws;
  int* tile_cnt = packed + (size_t)B * HW;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_decode_ids, dim3(tiles, B), dim3(256), 0, st, mask_logits, code_logits, HW, Lfull, L, packed,
                     ids, tile_cnt, tiles);
  ZP_LAUNCH_CHECK("zp_decode ids");
  hipLaunchKernelGGL(k_decode_emit, dim3(tiles, B), dim3(256), 0, st, packed, tile_cnt, tiles, H, W, (size_t)3 << L, lut,
                     lut_index, bbox, bbox_size, counts, xy, xyz);
  ZP_LAUNCH_CHECK("zp_decode emit");
  return ZP_OK;
}

extern "C" int zp_code_digits(const float* code_logits, int B, int L, int d, int H, int W, int out_f64, void* digits,
                              void* stream) {
  ZP_CHECK_ARG(code_logits && digits, "zp_code_digits: null pointer");
  ZP_CHECK_ARG(B > 0 && B <= 65535 && L >= 1 && L <= 65535 && d >= 2 && d <= 256 && H > 0 && W > 0 &&
                   (long long)H * W < (1ll << 30),
               "zp_code_digits: bad sizes");
  const int HW = H * W;
  hipLaunchKernelGGL(k_code_digits, dim3((HW + 1023) / 1024, L, B), dim3(256), 0, (hipStream_t)stream, code_logits, HW, L,
                     d, out_f64, digits);
  ZP_LAUNCH_CHECK("zp_code_digits");
  return ZP_OK;
}

extern "C" int zp_decode_radix(const float* mask_logits, const float* code_logits, int B, int H, int W, int L, int d,
                               const float* lut, const int* lut_index, const int* bbox, int bbox_size, int* ids,
                               int* counts, int* xy, float* xyz, void* ws, void* stream) {
  ZP_CHECK_ARG(mask_logits && code_logits && lut && bbox && counts && xy && xyz && ws, "zp_decode_radix: null pointer");
  ZP_CHECK_ARG(B > 0 && H > 0 && W > 0 && L >= 1 && d >= 2 && d <= 256 && bbox_size > 0, "zp_decode_radix: bad sizes");
  long long nid = 1;  // d^L class ids, at most 2^24 (zp_decode's limit)
  for (int i = 0; i < L && nid <= (1ll << 24); ++i) nid *= d;
  ZP_CHECK_ARG(nid <= (1ll << 24), "zp_decode_radix: %d steps of %d classes exceed 2^24 class ids", L, d);
  const int HW = H * W;
  const int tiles = (HW + DEC_TILE - 1) / DEC_TILE;
  int* packed = (int*)ws;
  int* tile_cnt = packed + (size_t)B * HW;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_decode_ids_radix, dim3(tiles, B), dim3(256), 0, st, mask_logits, code_logits, HW, L, d, packed, ids,
                     tile_cnt, tiles);
  ZP_LAUNCH_CHECK("zp_decode_radix ids");
  hipLaunchKernelGGL(k_decode_emit, dim3(tiles, B), dim3(256), 0, st, packed, tile_cnt, tiles, H, W, (size_t)3 * nid, lut,
                     lut_index, bbox, bbox_size, counts, xy, xyz);
  ZP_LAUNCH_CHECK("zp_decode_radix emit");
  return ZP_OK;
}

// workspace of zp_decode_unique: slots [B][HW], mask and head tile counts [2][B][tiles], then
// keys [B][T] and first [B][T] (filled with ones), then n / sum x / sum y [3][B][HW] (zeroed): k_unique_init
static int uq_log_table(long long HW) {
  int logT = 1;
  while ((1ll << logT) < 2 * HW) ++logT;
  return logT;
}

extern "C" long long zp_decode_unique_ws_bytes(int B, int H, int W) {
  long long HW = (long long)H * W;
  long long tiles = (HW + DEC_TILE - 1) / DEC_TILE;
  long long T = 1ll << uq_log_table(HW);
  return (long long)B * HW * 4 + 2 * (long long)B * tiles * 4 + 2 * (long long)B * T * 4 + 3 * (long long)B * HW * 4 + 256;
}

extern "C" int zp_decode_unique(const float* mask_logits, const float* code_logits, int B, int H, int W, int Lfull, int L,
                                int d, const float* lut, const int* lut_index, const int* bbox, int bbox_size, int* ids,
                                int* counts, int* xy, float* xyz, int* mult, double* mean_xy, void* ws, void* stream) {
  ZP_CHECK_ARG(mask_logits && code_logits && lut && bbox && counts && xy && xyz && ws, "zp_decode_unique: null pointer");
  ZP_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && L >= 1 && d >= 2 && d <= 256 && bbox_size > 0,
               "zp_decode_unique: bad sizes");
  long long nid = 1;  // class ids: 2^L (d == 2) or d^L, at most 2^24 as in zp_decode / zp_decode_radix
  for (int i = 0; i < L && nid <= (1ll << 24); ++i) nid *= d;
  ZP_CHECK_ARG(nid <= (1ll << 24), "zp_decode_unique: %d steps of %d classes exceed 2^24 class ids", L, d);
  ZP_CHECK_ARG(d == 2 ? L <= Lfull : Lfull == L * d, "zp_decode_unique: %d code channels for %d steps of %d classes", Lfull,
               L, d);
  // a class may hold every pixel: its coordinate sums stay below HW * max(H, W), kept in int32
  ZP_CHECK_ARG((long long)H * W * (H > W ? H : W) < (1ll << 31),
               "zp_decode_unique: %d x %d crops could overflow the int32 coordinate sums", H, W);
  const int HW = H * W;
  const int tiles = (HW + DEC_TILE - 1) / DEC_TILE;
  const int logT = uq_log_table(HW);
  const size_t T = (size_t)1 << logT;
  int* slots = (int*)ws;
  int* tile_cnt = slots + (size_t)B * HW;
  int* head_cnt = tile_cnt + (size_t)B * tiles;
  int* keys = head_cnt + (size_t)B * tiles;
  unsigned* first = (unsigned*)(keys + (size_t)B * T);
  int* acc_n = (int*)(first + (size_t)B * T);
  int* acc_x = acc_n + (size_t)B * HW;
  int* acc_y = acc_x + (size_t)B * HW;
  hipStream_t st = (hipStream_t)stream;
  const size_t n_ones = 2 * (size_t)B * T, n_all = n_ones + 3 * (size_t)B * HW;  // keys, first | n, sum x, sum y
  const size_t init_blocks = (n_all + 255) / 256;
  hipLaunchKernelGGL(k_unique_init, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(256), 0, st, keys, n_ones,
                     n_all);
  ZP_LAUNCH_CHECK("zp_decode_unique init");
  if (d == 2)
    hipLaunchKernelGGL(k_decode_ids, dim3(tiles, B), dim3(256), 0, st, mask_logits, code_logits, HW, Lfull, L, slots, ids,
                       tile_cnt, tiles);
  else
    hipLaunchKernelGGL(k_decode_ids_radix, dim3(tiles, B), dim3(256), 0, st, mask_logits, code_logits, HW, L, d, slots,
                       ids, tile_cnt, tiles);
  ZP_LAUNCH_CHECK("zp_decode_unique ids");
  hipLaunchKernelGGL(k_unique_insert, dim3(tiles, B), dim3(256), 0, st, slots, HW, logT, keys, first);
  ZP_LAUNCH_CHECK("zp_decode_unique insert");
  hipLaunchKernelGGL(k_unique_accum, dim3(tiles, B), dim3(256), 0, st, slots, HW, W, logT, first, acc_n, acc_x, acc_y,
                     head_cnt, tiles);
  ZP_LAUNCH_CHECK("zp_decode_unique accum");
  hipLaunchKernelGGL(k_unique_emit, dim3(tiles, B), dim3(256), 0, st, slots, head_cnt, tiles, H, W, logT, keys, first,
                     acc_n, acc_x, acc_y, (size_t)3 * nid, lut, lut_index, bbox, bbox_size, counts, xy, xyz, mult, mean_xy);
  ZP_LAUNCH_CHECK("zp_decode_unique emit");
  return ZP_OK;
}

extern "C" int zp_lut_coarsen(const double* lut64, int old_bits, int new_bits, float* out, void* stream) {
  ZP_CHECK_ARG(lut64 && out && new_bits >= 1 && new_bits <= old_bits && old_bits <= 24, "zp_lut_coarsen: bad args");
  const int n_new = 1 << new_bits;
  hipLaunchKernelGGL(k_lut_coarsen, dim3((n_new + 255) / 256), dim3(256), 0, (hipStream_t)stream, lut64,
                     old_bits - new_bits, n_new, out);
  ZP_LAUNCH_CHECK("zp_lut_coarsen");
  return ZP_OK;
}
