// Code -> vertex decode on gfx950: logits -> mask / code bits -> 16-bit class id -> LUT
// gather -> row-major compaction of the mask pixels -> original-image coordinates.
//
// Reference (lyltc1/ZebraPose):
//   common_ops.py:5-19                               sigmoid(x) > 0.5 (CPU fp32) == x > kHalfLogit
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

// the crop -> image map's f64 steps are single IEEE operations (the Makefile passes -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace zp {

constexpr int DEC_TILE = 1024;  // pixels per tile (256 threads x 4)

// ---- what the tile kernels share ----------------------------------------------------------------

// *dst <- the tile's sum of cnt: xor tree over each wave, four LDS words, thread 0 adds them in order
__device__ __forceinline__ void tile_count(int cnt, int* __restrict__ dst) {
  __shared__ int wsum[4];
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) *dst = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// The first output row of a thread that emits `mine` rows: the counts of the crop's earlier tiles
// (cnt_row[0 .. tile)) plus the tile's exclusive scan.  Thread 0 of tile 0 writes the crop's total.
__device__ __forceinline__ int tile_emit_pos(const int* __restrict__ cnt_row, int tiles, int tile, int mine,
                                             int* __restrict__ counts_b) {
  __shared__ int scan[256];
  __shared__ int base_s;
  if (threadIdx.x == 0) {
    int base = 0, total = 0;
    for (int t = 0; t < tiles; ++t) {
      int c = cnt_row[t];
      if (t < tile) base += c;
      total += c;
    }
    base_s = base;
    if (tile == 0) *counts_b = total;
  }
  scan[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    int t = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
    __syncthreads();
    scan[threadIdx.x] += t;
    __syncthreads();
  }
  return base_s + scan[threadIdx.x] - mine;
}

// n <= 4 consecutive floats (vec: all four in one 16-byte load), zeros behind them
__device__ __forceinline__ void load4(const float* __restrict__ x, int n, bool vec, float* v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = 0.f;
  if (vec) {
    const float4 t = *(const float4*)x;
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    for (int q = 0; q < n; ++q) v[q] = x[q];
  }
}

// bits of one logit plane at four consecutive pixels
__device__ __forceinline__ void bits4(const float* __restrict__ x, int n, bool vec, int* bit) {
  float v[4];
  load4(x, n, vec, v);
#pragma unroll
  for (int q = 0; q < 4; ++q) bit[q] = v[q] > kHalfLogit;
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
    float v[4];
    load4(x + (size_t)k * HW, n, vec, v);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k == 0 || v[q] > best[q]) {
        best[q] = v[q];
        dg[q] = k;
      }
  }
}

// One crop's output rows and its crop -> image map (CNN_output_to_pose.py:34-50).
struct EmitCrop {
  double bx, by, rx, ry;
  const float* L3;  // the crop's LUT (3 floats per class id)
  int* oxy;
  float* oxyz;
  __device__ __forceinline__ EmitCrop(int b, int HW, size_t lut_floats, const float* __restrict__ lut,
                                      const int* __restrict__ lut_index, const int* __restrict__ bbox, int bbox_size,
                                      int* __restrict__ xy, float* __restrict__ xyz) {
    bx = bbox[b * 4 + 0], by = bbox[b * 4 + 1];
    rx = (double)bbox[b * 4 + 2] / (double)bbox_size;
    ry = (double)bbox[b * 4 + 3] / (double)bbox_size;
    L3 = lut + (size_t)(lut_index ? lut_index[b] : 0) * lut_floats;
    oxy = xy + (size_t)b * HW * 2;
    oxyz = xyz + (size_t)b * HW * 3;
  }
};

// row pos of the crop <- the crop point (x, y) mapped to the image, and the 3D point of class id.
// x' = int(w / S * x + x0): a multiply, then an add (numpy's order), then astype('int')'s truncation.
__device__ __forceinline__ void emit_row(const EmitCrop& c, int pos, double x, double y, int id) {
  const double tx = c.rx * x, ty = c.ry * y;
  c.oxy[2 * pos] = (int)(tx + c.bx);
  c.oxy[2 * pos + 1] = (int)(ty + c.by);
  float p0 = c.L3[(size_t)id * 3], p1 = c.L3[(size_t)id * 3 + 1], p2 = c.L3[(size_t)id * 3 + 2];
  if (isnan(p0) || isnan(p1) || isnan(p2)) p0 = p1 = p2 = 0.f;
  c.oxyz[3 * pos] = p0;
  c.oxyz[3 * pos + 1] = p1;
  c.oxyz[3 * pos + 2] = p2;
}

// ---- pass 1: class ids ----------------------------------------------------------------------------
// packed <- id under the mask, -1 elsewhere; ids (optional) <- id; tile_cnt <- mask pixels per tile.
// id = sum_i digit_i * d^(L-1-i) (Horner) over the crop's Lfull code planes.  RADIX: step i owns d
// planes and its digit is their argmax (Lfull = L * d); else d = 2, step i owns one plane and its
// digit is the plane's bit (the leading L of Lfull planes: ignore_bit).
template <bool RADIX>
__global__ void __launch_bounds__(256) k_decode_ids(const float* __restrict__ mlog, const float* __restrict__ clog, int HW,
                                                    int Lfull, int L, int d, int* __restrict__ packed,
                                                    int* __restrict__ ids, int* __restrict__ tile_cnt, int tiles) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const int p0 = tile * DEC_TILE + threadIdx.x * 4;
  int cnt = 0;
  if (p0 < HW) {
    const int n = min(4, HW - p0);
    const bool vec = (HW & 3) == 0;  // the same for every thread; n == 4 then
    const size_t o = (size_t)b * HW + p0;
    const float* crow = clog + (size_t)b * Lfull * HW + p0;
    int mb[4], id[4] = {0, 0, 0, 0};
    bits4(mlog + o, n, vec, mb);
    for (int i = 0; i < L; ++i) {
      int dg[4];
      if constexpr (RADIX) digits4(crow + (size_t)i * d * HW, (size_t)HW, d, n, vec, dg);
      else bits4(crow + (size_t)i * HW, n, vec, dg);
#pragma unroll
      for (int q = 0; q < 4; ++q) id[q] = id[q] * (RADIX ? d : 2) + dg[q];
    }
    if (vec) {
      *(int4*)(packed + o) = make_int4(mb[0] ? id[0] : -1, mb[1] ? id[1] : -1, mb[2] ? id[2] : -1, mb[3] ? id[3] : -1);
      if (ids) *(int4*)(ids + o) = make_int4(id[0], id[1], id[2], id[3]);
    } else {
      for (int q = 0; q < n; ++q) {
        packed[o + q] = mb[q] ? id[q] : -1;
        if (ids) ids[o + q] = id[q];
      }
    }
    cnt = mb[0] + mb[1] + mb[2] + mb[3];  // pixels past the crop read as 0
  }
  tile_count(cnt, tile_cnt + b * tiles + tile);
}

// ---- pass 2: one row per mask pixel ---------------------------------------------------------------
__global__ void __launch_bounds__(256) k_decode_emit(const int* __restrict__ packed, const int* __restrict__ tile_cnt,
                                                     int tiles, int H, int W, size_t lut_floats,
                                                     const float* __restrict__ lut,
                                                     const int* __restrict__ lut_index, const int* __restrict__ bbox,
                                                     int bbox_size, int* __restrict__ counts, int* __restrict__ xy,
                                                     float* __restrict__ xyz) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const int HW = H * W;
  const int p0 = tile * DEC_TILE + threadIdx.x * 4;
  int v[4];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int p = p0 + k;
    v[k] = p < HW ? packed[(size_t)b * HW + p] : -1;
    mine += v[k] >= 0;
  }
  int pos = tile_emit_pos(tile_cnt + b * tiles, tiles, tile, mine, counts + b);
  const EmitCrop c(b, HW, lut_floats, lut, lut_index, bbox, bbox_size, xy, xyz);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v[k] < 0) continue;
    int p = p0 + k;
    int py = p / W, px = p - py * W;
    emit_row(c, pos++, (double)px, (double)py, v[k]);
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
  tile_count(cnt, head_cnt + b * tiles + tile);
}

// pass 3: k_decode_emit over the heads (a pixel that is its class's first), in row-major order, at
// the class's mean pixel: exact integer sums, one correctly rounded division per axis
__global__ void __launch_bounds__(256) k_unique_emit(const int* __restrict__ slots, const int* __restrict__ head_cnt,
                                                     int tiles, int H, int W, int logT, const int* __restrict__ keys,
                                                     const unsigned* __restrict__ first, const int* __restrict__ acc_n,
                                                     const int* __restrict__ acc_x, const int* __restrict__ acc_y,
                                                     size_t lut_floats, const float* __restrict__ lut,
                                                     const int* __restrict__ lut_index, const int* __restrict__ bbox,
                                                     int bbox_size, int* __restrict__ counts, int* __restrict__ xy,
                                                     float* __restrict__ xyz, int* __restrict__ mult,
                                                     double* __restrict__ mean_xy) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const int HW = H * W;
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
  int pos = tile_emit_pos(head_cnt + b * tiles, tiles, tile, mine, counts + b);
  const EmitCrop c(b, HW, lut_floats, lut, lut_index, bbox, bbox_size, xy, xyz);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v[k] < 0) continue;
    const size_t o = (size_t)b * HW + p0 + k;
    const int n = acc_n[o];
    const double mx = (double)acc_x[o] / (double)n;
    const double my = (double)acc_y[o] / (double)n;
    emit_row(c, pos, mx, my, v[k]);
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

// ---- host -----------------------------------------------------------------------------------------

inline int dec_tiles(long long HW) { return (int)((HW + DEC_TILE - 1) / DEC_TILE); }

// Each workspace is laid out by one carve, called with a null base for its size.  Every part is
// 4-byte words, so the parts follow each other unpadded; 256 spare bytes close the workspace.
struct DecWs {
  int* packed;    // [B][HW] id under the mask, -1 elsewhere
  int* tile_cnt;  // [B][tiles] mask pixels
};

inline DecWs dec_carve(void* ws, int B, long long HW, long long* total) {
  DecWs w;
  w.packed = (int*)ws;
  w.tile_cnt = w.packed + B * HW;
  if (total) *total = (w.tile_cnt + (long long)B * dec_tiles(HW) - w.packed) * 4 + 256;
  return w;
}

struct UqWs {
  int* slots;                  // [B][HW] DecWs::packed, then the slot of the id in the crop's table
  int *tile_cnt, *head_cnt;    // [B][tiles] mask pixels; first pixels of a class
  int* keys;                   // [B][T] class ids, T = 2^logT >= 2 * HW slots per crop
  unsigned* first;             // [B][T] first pixels.  k_unique_init fills these two with ones
  int *acc_n, *acc_x, *acc_y;  // [B][HW] and zeroes these: pixels, sum x, sum y of the class that starts here
  int logT;
};

inline UqWs uq_carve(void* ws, int B, long long HW, long long* total) {
  UqWs w;
  w.logT = 1;
  while ((1ll << w.logT) < 2 * HW) ++w.logT;
  const long long tiles = dec_tiles(HW), T = 1ll << w.logT;
  w.slots = (int*)ws;
  w.tile_cnt = w.slots + B * HW;
  w.head_cnt = w.tile_cnt + B * tiles;
  w.keys = w.head_cnt + B * tiles;
  w.first = (unsigned*)(w.keys + B * T);
  w.acc_n = (int*)(w.first + B * T);
  w.acc_x = w.acc_n + B * HW;
  w.acc_y = w.acc_x + B * HW;
  if (total) *total = (w.acc_y + B * HW - w.slots) * 4 + 256;
  return w;
}

// The checks the three decode entry points share (`who`, for the message): pointers, sizes, and
// *nid <- the d^L class ids of L steps of d classes, at most 2^24.  The grids are (tiles, B): B <= 65535.
static int dec_check(const char* who, bool pointers, int B, int H, int W, int L, int d, int bbox_size, long long* nid) {
  ZP_CHECK_ARG(pointers, "%s: null pointer", who);
  ZP_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && L >= 1 && d >= 2 && d <= 256 && bbox_size > 0, "%s: bad sizes",
               who);
  *nid = 1;
  for (int i = 0; i < L && *nid <= (1ll << 24); ++i) *nid *= d;
  ZP_CHECK_ARG(*nid <= (1ll << 24), "%s: %d steps of %d classes exceed 2^24 class ids", who, L, d);
  return ZP_OK;
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_decode_ws_bytes(int B, int H, int W) {
  long long total;
  dec_carve(nullptr, B, (long long)H * W, &total);
  return total;
}

extern "C" int zp_decode(const float* mask_logits, const float* code_logits, int B, int H, int W, int Lfull, int L,
                         const float* lut, const int* lut_index, const int* bbox, int bbox_size, int* ids, int* counts,
                         int* xy, float* xyz, void* ws, void* stream) {
  long long nid;
  if (int rc = dec_check("zp_decode", mask_logits && code_logits && lut && bbox && counts && xy && xyz && ws, B, H, W, L, 2,
                         bbox_size, &nid))
    return rc;
  ZP_CHECK_ARG(L <= Lfull, "zp_decode: %d code channels for %d bits", Lfull, L);
  const int HW = H * W, tiles = dec_tiles(HW);
  const DecWs w = dec_carve(ws, B, HW, nullptr);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_decode_ids<false>, dim3(tiles, B), dim3(256), 0, st, mask_logits, code_logits, HW, Lfull, L, 2,
                     w.packed, ids, w.tile_cnt, tiles);
  ZP_LAUNCH_CHECK("zp_decode ids");
  hipLaunchKernelGGL(k_decode_emit, dim3(tiles, B), dim3(256), 0, st, w.packed, w.tile_cnt, tiles, H, W, (size_t)3 * nid,
                     lut, lut_index, bbox, bbox_size, counts, xy, xyz);
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
  long long nid;
  if (int rc = dec_check("zp_decode_radix", mask_logits && code_logits && lut && bbox && counts && xy && xyz && ws, B, H, W,
                         L, d, bbox_size, &nid))
    return rc;
  const int HW = H * W, tiles = dec_tiles(HW);
  const DecWs w = dec_carve(ws, B, HW, nullptr);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_decode_ids<true>, dim3(tiles, B), dim3(256), 0, st, mask_logits, code_logits, HW, L * d, L, d,
                     w.packed, ids, w.tile_cnt, tiles);
  ZP_LAUNCH_CHECK("zp_decode_radix ids");
  hipLaunchKernelGGL(k_decode_emit, dim3(tiles, B), dim3(256), 0, st, w.packed, w.tile_cnt, tiles, H, W, (size_t)3 * nid,
                     lut, lut_index, bbox, bbox_size, counts, xy, xyz);
  ZP_LAUNCH_CHECK("zp_decode_radix emit");
  return ZP_OK;
}

extern "C" long long zp_decode_unique_ws_bytes(int B, int H, int W) {
  long long total;
  uq_carve(nullptr, B, (long long)H * W, &total);
  return total;
}

extern "C" int zp_decode_unique(const float* mask_logits, const float* code_logits, int B, int H, int W, int Lfull, int L,
                                int d, const float* lut, const int* lut_index, const int* bbox, int bbox_size, int* ids,
                                int* counts, int* xy, float* xyz, int* mult, double* mean_xy, void* ws, void* stream) {
  long long nid;  // class ids: 2^L (d == 2) or d^L
  if (int rc = dec_check("zp_decode_unique", mask_logits && code_logits && lut && bbox && counts && xy && xyz && ws, B, H,
                         W, L, d, bbox_size, &nid))
    return rc;
  ZP_CHECK_ARG(d == 2 ? L <= Lfull : Lfull == L * d, "zp_decode_unique: %d code channels for %d steps of %d classes", Lfull,
               L, d);
  // a class may hold every pixel: its coordinate sums stay below HW * max(H, W), kept in int32
  ZP_CHECK_ARG((long long)H * W * (H > W ? H : W) < (1ll << 31),
               "zp_decode_unique: %d x %d crops could overflow the int32 coordinate sums", H, W);
  const int HW = H * W, tiles = dec_tiles(HW);
  const UqWs w = uq_carve(ws, B, HW, nullptr);
  hipStream_t st = (hipStream_t)stream;
  const size_t n_ones = (size_t)(w.acc_n - w.keys), n_all = (size_t)(w.acc_y + (size_t)B * HW - w.keys);
  const size_t init_blocks = (n_all + 255) / 256;
  hipLaunchKernelGGL(k_unique_init, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(256), 0, st, w.keys,
                     n_ones, n_all);
  ZP_LAUNCH_CHECK("zp_decode_unique init");
  if (d == 2)
    hipLaunchKernelGGL(k_decode_ids<false>, dim3(tiles, B), dim3(256), 0, st, mask_logits, code_logits, HW, Lfull, L, d,
                       w.slots, ids, w.tile_cnt, tiles);
  else
    hipLaunchKernelGGL(k_decode_ids<true>, dim3(tiles, B), dim3(256), 0, st, mask_logits, code_logits, HW, Lfull, L, d,
                       w.slots, ids, w.tile_cnt, tiles);
  ZP_LAUNCH_CHECK("zp_decode_unique ids");
  hipLaunchKernelGGL(k_unique_insert, dim3(tiles, B), dim3(256), 0, st, w.slots, HW, w.logT, w.keys, w.first);
  ZP_LAUNCH_CHECK("zp_decode_unique insert");
  hipLaunchKernelGGL(k_unique_accum, dim3(tiles, B), dim3(256), 0, st, w.slots, HW, W, w.logT, w.first, w.acc_n, w.acc_x,
                     w.acc_y, w.head_cnt, tiles);
  ZP_LAUNCH_CHECK("zp_decode_unique accum");
  hipLaunchKernelGGL(k_unique_emit, dim3(tiles, B), dim3(256), 0, st, w.slots, w.head_cnt, tiles, H, W, w.logT, w.keys,
                     w.first, w.acc_n, w.acc_x, w.acc_y, (size_t)3 * nid, lut, lut_index, bbox, bbox_size, counts, xy, xyz,
                     mult, mean_xy);
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
