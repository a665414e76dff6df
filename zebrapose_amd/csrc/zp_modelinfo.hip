// Model diameter and the box of models_info.json on the device: zp_model_info.  Reference:
// lib/pysixd/misc.py:952-966 (calc_pts_diameter: the largest distance over all pairs i <= j, a Python
// loop of n numpy passes) and the min_* / size_* entries BOP ships with its models.  The contract in
// include/zp.h is the specification; tests/modelinfo_ref.py restates it in numpy.
//
// k_mi_pairs walks the 256 x 256 tiles of the upper triangle (tile row <= tile column) with a fixed
// grid.  A thread keeps one i point in registers as f64; the 256 j points sit in LDS as f64 (6 KB),
// every lane reads the same address (a broadcast, no bank conflict).  The thread scans j ascending
// and replaces on a strictly larger d2, so its lowest j survives; its tile result joins its running
// best by (larger d2, then lower i, then lower j).  Lanes, waves and workgroups reduce by the same
// order, which makes the maximum and its pair independent of how the work was split: no atomics, and
// two runs give the same bits.  Each workgroup writes one 16-byte partial.
// k_mi_final (one workgroup) reduces the partials, takes the box and the finiteness flag in a pass
// over the points, and writes out / pair / status.
// This file is built with -ffp-contract=off: d2 is specified operation by operation.
#include <limits.h>
#include <math.h>
#include "zp_common.h"

#pragma clang fp contract(off)

namespace zp {

constexpr int MI_T = 256;          // tile edge = workgroup size
constexpr int MI_MAX_PARTS = 1024;  // grid of k_mi_pairs: four workgroups per CU of an MI355X

struct MiBest {
  double d2;  // -1: nothing yet (every real d2 is >= 0 or NaN)
  int i, j;
};

// a replaces b: larger d2, then lower i, then lower j.  A NaN never replaces and is never replaced
// by an equal; status reports it.
__device__ __forceinline__ bool mi_better(double ad2, int ai, int aj, double bd2, int bi, int bj) {
  return ad2 > bd2 || (ad2 == bd2 && (ai < bi || (ai == bi && aj < bj)));
}

__device__ __forceinline__ void mi_join(MiBest& b, double d2, int i, int j) {
  if (mi_better(d2, i, j, b.d2, b.i, b.j)) b.d2 = d2, b.i = i, b.j = j;
}

// wave -> workgroup; the result is valid in thread 0
__device__ __forceinline__ void mi_block_reduce(MiBest& b, MiBest (&wred)[MI_T / 64]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double d2 = __shfl_down(b.d2, off);
    const int i = __shfl_down(b.i, off), j = __shfl_down(b.j, off);
    mi_join(b, d2, i, j);
  }
  if (lane == 0) wred[wave] = b;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < MI_T / 64; ++w) mi_join(b, wred[w].d2, wred[w].i, wred[w].j);
  }
}

// linear index L of the upper triangle, column by column: tile (r, c), r <= c, is L = c (c + 1) / 2 + r
__device__ __forceinline__ void mi_tile(long long L, int& r, int& c) {
  long long cc = (long long)((sqrt(8.0 * (double)L + 1.0) - 1.0) * 0.5);  // 8 L + 1 < 2^53: exact
  while (cc * (cc + 1) / 2 > L) --cc;
  while ((cc + 1) * (cc + 2) / 2 <= L) ++cc;
  c = (int)cc;
  r = (int)(L - cc * (cc + 1) / 2);
}

__global__ void __launch_bounds__(MI_T) k_mi_pairs(const float* __restrict__ pts, int n, long long ntiles,
                                                   MiBest* __restrict__ parts) {
  __shared__ double sj[MI_T * 3];
  __shared__ MiBest wred[MI_T / 64];
  const int tid = threadIdx.x;
  MiBest best = {-1.0, INT_MAX, INT_MAX};
  for (long long L = blockIdx.x; L < ntiles; L += gridDim.x) {
    int tr, tc;
    mi_tile(L, tr, tc);
    const int i = tr * MI_T + tid, j0 = tc * MI_T;
    const int cnt = min(MI_T, n - j0);  // the last tile column is partial: entries from cnt on are never read
    __syncthreads();                    // the previous tile's scan is over
    if (tid < cnt) {
      const float* p = pts + (size_t)(j0 + tid) * 3;
      sj[3 * tid] = (double)p[0], sj[3 * tid + 1] = (double)p[1], sj[3 * tid + 2] = (double)p[2];
    }
    double xi = 0.0, yi = 0.0, zi = 0.0;
    // first j of this lane: itself on a diagonal tile (j < i belongs to the pair (j, i)), none for a
    // lane past the last point
    int lo = MI_T;
    if (i < n) {
      const float* p = pts + (size_t)i * 3;
      xi = (double)p[0], yi = (double)p[1], zi = (double)p[2];
      lo = tr == tc ? tid : 0;
    }
    __syncthreads();
    double td2 = -1.0;
    int tj = INT_MAX;
#pragma unroll 8
    for (int jj = 0; jj < cnt; ++jj) {
      const double dx = xi - sj[3 * jj], dy = yi - sj[3 * jj + 1], dz = zi - sj[3 * jj + 2];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (jj >= lo && d2 > td2) td2 = d2, tj = jj;
    }
    if (tj != INT_MAX) mi_join(best, td2, i, j0 + tj);
  }
  mi_block_reduce(best, wred);
  if (tid == 0) parts[blockIdx.x] = best;
}

// order-preserving integer key of an f32 (-0 below +0), and back
__device__ __forceinline__ int mi_key(float v) {
  const int b = __float_as_int(v);
  return b < 0 ? b ^ 0x7fffffff : b;
}
__device__ __forceinline__ double mi_unkey(int k) { return (double)__int_as_float(k < 0 ? k ^ 0x7fffffff : k); }

__global__ void __launch_bounds__(MI_T) k_mi_final(const float* __restrict__ pts, int n,
                                                   const MiBest* __restrict__ parts, int nparts,
                                                   double* __restrict__ out, int* __restrict__ pair,
                                                   int* __restrict__ status) {
  __shared__ MiBest wred[MI_T / 64];
  __shared__ int bred[MI_T / 64][7];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  MiBest best = {-1.0, INT_MAX, INT_MAX};
  for (int k = tid; k < nparts; k += MI_T) mi_join(best, parts[k].d2, parts[k].i, parts[k].j);
  mi_block_reduce(best, wred);

  // box: integer min / max of the keys (exact in any order); acc[6]: a non-finite coordinate was seen
  int acc[7] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0};
  for (int p = tid; p < n; p += MI_T) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = pts[(size_t)p * 3 + a];
      const int k = mi_key(v);
      acc[a] = min(acc[a], k), acc[3 + a] = max(acc[3 + a], k);
      acc[6] |= !__builtin_isfinite(v);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      const int o = __shfl_down(acc[a], off);
      acc[a] = a < 3 ? min(acc[a], o) : (a < 6 ? max(acc[a], o) : (acc[a] | o));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 7; ++a) bred[wave][a] = acc[a];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < MI_T / 64; ++w) {
#pragma unroll
      for (int a = 0; a < 7; ++a)
        acc[a] = a < 3 ? min(acc[a], bred[w][a]) : (a < 6 ? max(acc[a], bred[w][a]) : (acc[a] | bred[w][a]));
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double lo = mi_unkey(acc[a]), hi = mi_unkey(acc[3 + a]);
      out[a] = lo, out[3 + a] = hi - lo;
    }
    out[6] = sqrt(best.d2), out[7] = best.d2;
    if (pair) pair[0] = best.i, pair[1] = best.j;
    status[0] = acc[6];
  }
}

static bool mi_n_ok(int n) { return n >= 1 && 3LL * n < 2147483647LL - 1024; }

}  // namespace zp

using namespace zp;

extern "C" long long zp_model_info_ws_bytes(int n) {
  if (!mi_n_ok(n)) return -1;
  return (long long)MI_MAX_PARTS * (long long)sizeof(MiBest);
}

extern "C" int zp_model_info(const float* pts, int n, double* out, int* pair, int* status, void* ws, void* stream) {
  ZP_CHECK_ARG(mi_n_ok(n), "zp_model_info: n %d outside [1, (2^31 - 1024) / 3)", n);
  ZP_CHECK_ARG(pts && out && status && ws, "zp_model_info: NULL pointer (pts %p, out %p, status %p, ws %p)",
               (const void*)pts, (void*)out, (void*)status, ws);
  hipStream_t st = (hipStream_t)stream;
  const long long nt = ((long long)n + MI_T - 1) / MI_T, ntiles = nt * (nt + 1) / 2;
  const int grid = (int)(ntiles < MI_MAX_PARTS ? ntiles : MI_MAX_PARTS);
  MiBest* parts = (MiBest*)ws;
  hipLaunchKernelGGL(k_mi_pairs, dim3(grid), dim3(MI_T), 0, st, pts, n, ntiles, parts);
  ZP_LAUNCH_CHECK("zp_model_info pairs");
  hipLaunchKernelGGL(k_mi_final, dim3(1), dim3(MI_T), 0, st, pts, n, (const MiBest*)parts, grid, out, pair, status);
  ZP_LAUNCH_CHECK("zp_model_info final");
  return ZP_OK;
}
