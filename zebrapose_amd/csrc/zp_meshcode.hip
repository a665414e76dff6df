// Mesh coder: per-vertex / per-face surface codes and the class -> 3D-point LUT of a raw mesh.
// Reference: Binary_Code_GT_Generator/Generate_Mesh_with_GT_Color/Generate_Mesh_with_GT_Color.cpp
// -- Divide_PointCloud_Opencv_Samesize (:61-218: cv::kmeans into 2 clusters, 3 attempts, 10
// iterations, eps 1.0, then the balancing that moves the over-full cluster's points nearest the
// other centre), generate_point_id_class_result (:322-353, first split = MSB),
// generate_face_id_class_result (:356-393) and generate_class_corres_point_result (:396-455).
// OpenCV's RNG and k-means++ draws cannot be reproduced, so the split is restated in exact integer
// arithmetic (include/zp.h, zp_mesh_code; tests/meshcode_ref.py is the executable definition):
//
//   grid     q = rint(f64(v) * 2^k), saturated to +-(2^19 - 1); all clustering arithmetic is int64
//   level l  2^l groups, each kept contiguous and in ascending vertex index (gs / order / gstart)
//   2-means  per attempt: c0 = the group's vertex at rank (draw * n) >> 32, c1 = the vertex farthest
//            from c0 (lowest index on ties); Lloyd steps with label ties to class 0, centres
//            floor((2 S + n) / (2 n)), stop once the larger centre shift^2 <= eps2_q; the attempt
//            with the lowest compactness wins (lowest attempt on ties)
//   balance  the over-full class keeps its floor(n / 2) vertices farthest from the other centre
//            (lower index on ties); children 2g (bit 0) and 2g + 1 (bit 1)
//
// A level runs as launches over all groups at once and nothing is read back: a converged group
// raises its own `done` word and later steps skip it.  Per-group sums are integer atomics, so their
// result is exact in any order; in front of them every wave sums the runs of equal group among its
// lanes with shuffles (group_reduce), and keeps summing in registers across its M_ITEMS positions
// per lane for as long as the whole wave stays inside the same groups: at the top levels one wave
// issues 7 atomics per 512 vertices, at the bottom levels one set per (group, wave).
// From rocPRIM (header-only): the stable radix sort that (a) regroups the vertices by child group
// after each level, (b) ranks a group's vertices by (class, d^2 to the other centre descending,
// index ascending) for the balance, (c) groups the faces by class for the LUT.  The LUT sums are f64
// additions in ascending face index, vertex 0, 1, 2: one thread per class walks its faces.
//
// zp_mesh_code_radix (the second half of this file; tests/meshcode_radix_ref.py) splits d ways per
// level, d = 4 .. 256, for the d-ary codes: the same grid, group layout, faces and LUT; farthest-point
// seeds c_1 .. c_(d-1), d-way Lloyd steps, and in place of the 2-way balance a peel, class by class,
// that leaves every class floor(n / d) or ceil(n / d) vertices (the reference's own balancing touches
// classes 0 and 1 only).  Its kernels are k_rx_*.
#include "zp_common.h"

#include <rocprim/device/device_radix_sort.hpp>

// the LUT's f64 steps are single IEEE operations (the Makefile passes -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace zp {

typedef unsigned long long u64;

constexpr int M_SAT = (1 << 19) - 1;
constexpr int M_IDX_BITS = 21;  // nv <= 2^21
constexpr u64 M_IDX_MASK = (1ull << M_IDX_BITS) - 1;
constexpr int M_D2_BITS = 42;  // d^2 <= 3 * (2^20)^2 < 2^42
constexpr u64 M_D2_MASK = (1ull << M_D2_BITS) - 1;
constexpr int M_ITEMS = 8;  // positions per thread of the per-vertex kernels
constexpr int M_NSUM = 7;   // S0 xyz, S1 xyz, n0 | n1 << 32
constexpr long long M_TEMP_FIXED = 16ll << 20, M_TEMP_PER_ELEM = 32;  // budget for rocPRIM's temporary storage

struct MWs {
  int4* q;        // [nv] grid coordinates (w unused)
  int* gid;       // [nv] group of vertex v at the next level
  unsigned* gs;   // [nv] group of sorted position p
  int* order;     // [nv] vertex at sorted position p
  int* iota;      // [max(nv, nf)] 0, 1, 2, ...
  u64* key;       // [nv] balance keys, and their sorted copy
  u64* key2;
  int* val2;      // [nv] vertices in balance order
  int* gstart;    // [G + 1]
  int* cen;       // [G][6] c0 xyz, c1 xyz of the running attempt
  int* bcen;      // [G][6] of the best attempt
  u64* sums;      // [G][M_NSUM]
  u64* far;       // [G] farthest-point key
  u64* comp;      // [G] compactness of the running attempt
  u64* bcomp;     // [G] of the best
  u64* cnt0;      // [G] class-0 count under the best centres
  int* done;      // [G]
  unsigned* fkey2;  // [nf] face ids sorted
  int* fval2;     // [nf] faces in class order
  void* temp;
  size_t temp_bytes;
};

inline size_t m_align(size_t v) { return (v + 255) & ~(size_t)255; }

inline MWs m_carve(void* ws, int nv, int nf, int bits, size_t* total) {
  char* p = (char*)ws;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* r = p + o;
    o = m_align(o + bytes);
    return (void*)r;
  };
  const size_t G = (size_t)1 << (bits - 1), nmax = (size_t)(nv > nf ? nv : nf);
  MWs w;
  w.q = (int4*)take((size_t)nv * 16);
  w.gid = (int*)take((size_t)nv * 4);
  w.gs = (unsigned*)take((size_t)nv * 4);
  w.order = (int*)take((size_t)nv * 4);
  w.iota = (int*)take(nmax * 4);
  w.key = (u64*)take((size_t)nv * 8);
  w.key2 = (u64*)take((size_t)nv * 8);
  w.val2 = (int*)take((size_t)nv * 4);
  w.gstart = (int*)take((G + 1) * 4);
  w.cen = (int*)take(G * 24);
  w.bcen = (int*)take(G * 24);
  w.sums = (u64*)take(G * M_NSUM * 8);
  w.far = (u64*)take(G * 8);
  w.comp = (u64*)take(G * 8);
  w.bcomp = (u64*)take(G * 8);
  w.cnt0 = (u64*)take(G * 8);
  w.done = (int*)take(G * 4);
  w.fkey2 = (unsigned*)take((size_t)nf * 4);
  w.fval2 = (int*)take((size_t)nf * 4);
  w.temp_bytes = (size_t)(M_TEMP_FIXED + M_TEMP_PER_ELEM * (long long)nmax);
  w.temp = take(w.temp_bytes);
  if (total) *total = o;
  return w;
}

static bool mesh_sizes_ok(int nv, int nf, int bits) {
  return bits >= 1 && bits <= 16 && nv >= (1 << bits) && nv <= (1 << M_IDX_BITS) && nf >= 1 && nf <= (1 << 24);
}

// ---- per-vertex set-up -------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_mesh_quant(const float* __restrict__ verts, int nv, int k,
                                                    int4* __restrict__ q) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s = rint(ldexp((double)verts[3 * (size_t)v + a], k));
    c[a] = s == s ? (int)fmin(fmax(s, (double)-M_SAT), (double)M_SAT) : 0;
  }
  q[v] = make_int4(c[0], c[1], c[2], 0);
}

__global__ void __launch_bounds__(256) k_mesh_init(int nv, int nmax, unsigned* __restrict__ gs, int* __restrict__ order,
                                                   int* __restrict__ iota, int* __restrict__ gstart,
                                                   int* __restrict__ vertex_ids) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < nmax) iota[p] = p;
  if (p < nv) {
    gs[p] = 0u;
    order[p] = p;
    vertex_ids[p] = 0;
  }
  if (p == 0) {
    gstart[0] = 0;
    gstart[1] = nv;
  }
}

// ---- sums over the vertices of each group ----------------------------------------------------------

__device__ __forceinline__ long long dist2(const int4 p, const int* __restrict__ c) {
  const long long dx = (long long)p.x - c[0], dy = (long long)p.y - c[1], dz = (long long)p.z - c[2];
  return dx * dx + dy * dy + dz * dz;
}

// Every lane holds NV partial values of group g (g < 0: none); groups lie in runs of neighbouring
// lanes.  Sums (MAX: maxima) each run into its first lane, which merges it into dst[g][NV].
template <int NV, bool MAX>
__device__ __forceinline__ void wave_flush(u64 (&acc)[NV], int g, u64* __restrict__ dst, int lane) {
  if (__all(g < 0)) return;
  for (int off = 1; off < 64; off <<= 1) {
    const int og = __shfl_down(g, off);
    const bool take = lane + off < 64 && og == g;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const u64 o = __shfl_down(acc[i], off);
      if (take) acc[i] = MAX ? (o > acc[i] ? o : acc[i]) : acc[i] + o;
    }
  }
  const int pg = __shfl_up(g, 1);
  if (g >= 0 && (lane == 0 || pg != g)) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (!acc[i]) continue;
      if (MAX)
        atomicMax(dst + (size_t)g * NV + i, acc[i]);
      else
        atomicAdd(dst + (size_t)g * NV + i, acc[i]);
    }
  }
}

// item(p, val) fills the NV values of sorted position p and returns its group, or -1 to leave it
// out.  A block covers 256 * M_ITEMS consecutive positions, lane-contiguous for every item; while a
// whole wave keeps the groups of its previous item the values add up in registers.
template <int NV, bool MAX, typename F>
__device__ __forceinline__ void group_reduce(int nv, u64* __restrict__ dst, F item) {
  const int lane = threadIdx.x & 63;
  const long long base = (long long)blockIdx.x * (256 * M_ITEMS) + threadIdx.x;
  u64 acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0;
  int gcur = -1;
  for (int k = 0; k < M_ITEMS; ++k) {
    const long long p = base + k * 256;
    u64 val[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) val[i] = 0;
    int g = -1;
    if (p < nv) g = item((int)p, val);
    if (__all(g == gcur)) {
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] = MAX ? (val[i] > acc[i] ? val[i] : acc[i]) : acc[i] + val[i];
    } else {
      wave_flush<NV, MAX>(acc, gcur, dst, lane);
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] = val[i];
      gcur = g;
    }
  }
  wave_flush<NV, MAX>(acc, gcur, dst, lane);
}

struct MPos {
  int g, v;
  int4 pt;
};

// sorted position p -> group, vertex, grid point; false when the group word is out of range
__device__ __forceinline__ bool load_pos(int p, int nv, int G, const unsigned* __restrict__ gs,
                                         const int* __restrict__ order, const int4* __restrict__ q, MPos& r) {
  const unsigned g = gs[p];
  if (g >= (unsigned)G) return false;
  int v = order[p];
  if ((unsigned)v >= (unsigned)nv) v = 0;
  r.g = (int)g;
  r.v = v;
  r.pt = q[v];
  return true;
}

__global__ void __launch_bounds__(256) k_mesh_far(int nv, int G, const unsigned* __restrict__ gs,
                                                  const int* __restrict__ order, const int4* __restrict__ q,
                                                  const int* __restrict__ cen, u64* __restrict__ far) {
  group_reduce<1, true>(nv, far, [&](int p, u64(&val)[1]) {
    MPos r;
    if (!load_pos(p, nv, G, gs, order, q, r)) return -1;
    val[0] = ((u64)dist2(r.pt, cen + 6 * (size_t)r.g) << M_IDX_BITS) | (M_IDX_MASK - (u64)r.v);
    return r.g;
  });
}

__global__ void __launch_bounds__(256) k_mesh_accum(int nv, int G, const unsigned* __restrict__ gs,
                                                    const int* __restrict__ order, const int4* __restrict__ q,
                                                    const int* __restrict__ cen, const int* __restrict__ done,
                                                    u64* __restrict__ sums) {
  group_reduce<M_NSUM, false>(nv, sums, [&](int p, u64(&val)[M_NSUM]) {
    MPos r;
    if (!load_pos(p, nv, G, gs, order, q, r) || done[r.g]) return -1;
    const int* c = cen + 6 * (size_t)r.g;
    const int j = dist2(r.pt, c) <= dist2(r.pt, c + 3) ? 0 : 1;
    val[3 * j] = (u64)(long long)r.pt.x;
    val[3 * j + 1] = (u64)(long long)r.pt.y;
    val[3 * j + 2] = (u64)(long long)r.pt.z;
    val[6] = j ? 1ull << 32 : 1ull;
    return r.g;
  });
}

__global__ void __launch_bounds__(256) k_mesh_comp(int nv, int G, const unsigned* __restrict__ gs,
                                                   const int* __restrict__ order, const int4* __restrict__ q,
                                                   const int* __restrict__ cen, u64* __restrict__ comp) {
  group_reduce<1, false>(nv, comp, [&](int p, u64(&val)[1]) {
    MPos r;
    if (!load_pos(p, nv, G, gs, order, q, r)) return -1;
    const int* c = cen + 6 * (size_t)r.g;
    const long long d0 = dist2(r.pt, c), d1 = dist2(r.pt, c + 3);
    val[0] = (u64)(d0 <= d1 ? d0 : d1);
    return r.g;
  });
}

// labels under the best centres: the balance key (group, class, d^2 to the other centre descending)
// of every position and the class-0 count of every group
__global__ void __launch_bounds__(256) k_mesh_final(int nv, int G, const unsigned* __restrict__ gs,
                                                    const int* __restrict__ order, const int4* __restrict__ q,
                                                    const int* __restrict__ bcen, u64* __restrict__ key,
                                                    u64* __restrict__ cnt0) {
  group_reduce<1, false>(nv, cnt0, [&](int p, u64(&val)[1]) {
    MPos r;
    if (!load_pos(p, nv, G, gs, order, q, r)) {
      key[p] = ~0ull;
      return -1;
    }
    const int* c = bcen + 6 * (size_t)r.g;
    const long long d0 = dist2(r.pt, c), d1 = dist2(r.pt, c + 3);
    const int j = d0 <= d1 ? 0 : 1;
    const u64 other = (u64)(j ? d0 : d1);
    key[p] = ((u64)r.g << (M_D2_BITS + 1)) | ((u64)j << M_D2_BITS) | (M_D2_MASK - other);
    val[0] = j ? 0ull : 1ull;
    return r.g;
  });
}

// ---- per-group steps ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_mesh_seed0(int G, int nv, const int* __restrict__ gstart,
                                                    const int* __restrict__ order, const int4* __restrict__ q,
                                                    const uint32_t* __restrict__ draws, int* __restrict__ cen,
                                                    u64* __restrict__ far) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const int s = gstart[g];
  const long long n = (long long)gstart[g + 1] - s;
  long long pos = s + (long long)(((u64)draws[g] * (u64)(n > 0 ? n : 0)) >> 32);
  pos = pos < 0 ? 0 : (pos >= nv ? nv - 1 : pos);
  int v = order[pos];
  if ((unsigned)v >= (unsigned)nv) v = 0;
  const int4 pt = q[v];
  cen[6 * (size_t)g] = pt.x;
  cen[6 * (size_t)g + 1] = pt.y;
  cen[6 * (size_t)g + 2] = pt.z;
  far[g] = 0;
}

__global__ void __launch_bounds__(256) k_mesh_seed1(int G, int nv, const int4* __restrict__ q,
                                                    const u64* __restrict__ far, int* __restrict__ cen,
                                                    u64* __restrict__ sums, u64* __restrict__ comp,
                                                    int* __restrict__ done) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  long long v = (long long)(M_IDX_MASK - (far[g] & M_IDX_MASK));
  if (v >= nv) v = nv - 1;
  const int4 pt = q[v];
  cen[6 * (size_t)g + 3] = pt.x;
  cen[6 * (size_t)g + 4] = pt.y;
  cen[6 * (size_t)g + 5] = pt.z;
#pragma unroll
  for (int i = 0; i < M_NSUM; ++i) sums[(size_t)g * M_NSUM + i] = 0;
  comp[g] = 0;
  done[g] = 0;
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {  // b > 0
  long long r = a / b;
  if (a % b != 0 && a < 0) --r;
  return r;
}

__global__ void __launch_bounds__(256) k_mesh_update(int G, long long eps2, int* __restrict__ cen,
                                                     u64* __restrict__ sums, int* __restrict__ done) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G || done[g]) return;
  u64* s = sums + (size_t)g * M_NSUM;
  const long long n[2] = {(long long)(s[6] & 0xFFFFFFFFull), (long long)(s[6] >> 32)};
  long long worst = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (n[j] <= 0) continue;  // an empty class keeps its centre
    long long shift = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const long long c = floor_div(2 * (long long)s[3 * j + a] + n[j], 2 * n[j]);
      const long long d = c - cen[6 * (size_t)g + 3 * j + a];
      shift += d * d;
      cen[6 * (size_t)g + 3 * j + a] = (int)c;
    }
    worst = shift > worst ? shift : worst;
  }
  if (worst <= eps2) done[g] = 1;
#pragma unroll
  for (int i = 0; i < M_NSUM; ++i) s[i] = 0;
}

__global__ void __launch_bounds__(256) k_mesh_best(int G, int attempt, const int* __restrict__ cen,
                                                   const u64* __restrict__ comp, int* __restrict__ bcen,
                                                   u64* __restrict__ bcomp, u64* __restrict__ cnt0) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  if (attempt == 0 || comp[g] < bcomp[g]) {
    bcomp[g] = comp[g];
#pragma unroll
    for (int i = 0; i < 6; ++i) bcen[6 * (size_t)g + i] = cen[6 * (size_t)g + i];
  }
  cnt0[g] = 0;
}

// positions in balance order: (group, class) runs, each by d^2 to the other centre descending, index
// ascending.  The over-full class keeps its first floor(n / 2); the rest change sides.
__global__ void __launch_bounds__(256) k_mesh_balance(int nv, int G, int shift, const u64* __restrict__ key2,
                                                      const int* __restrict__ val2, const int* __restrict__ gstart,
                                                      const u64* __restrict__ cnt0, int* __restrict__ gid,
                                                      int* __restrict__ vertex_ids) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nv) return;
  const u64 k = key2[p];
  const u64 g = k >> (M_D2_BITS + 1);
  const int v = val2[p];
  if (g >= (u64)G || (unsigned)v >= (unsigned)nv) return;
  const int j = (int)((k >> M_D2_BITS) & 1);
  const long long s = gstart[g], n = (long long)gstart[g + 1] - s, m = n / 2, c0 = (long long)cnt0[g];
  const long long rank = p - s - (j ? c0 : 0), cnt = j ? n - c0 : c0;
  const int bit = (cnt > m && rank >= m) ? j ^ 1 : j;
  gid[v] = (int)(2 * g) + bit;
  if (bit) vertex_ids[v] |= 1 << shift;
}

__global__ void __launch_bounds__(256) k_mesh_bounds(int nv, int G, const unsigned* __restrict__ gs,
                                                     int* __restrict__ gstart) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nv) return;
  const unsigned g = gs[p];
  if (g >= (unsigned)G) return;
  if (p == 0) {
    gstart[g] = 0;
    gstart[G] = nv;
  } else if (gs[p - 1] != g) {
    gstart[g] = p;
  }
}

// ---- faces and the LUT -------------------------------------------------------------------------

__device__ __forceinline__ int clamp_index(int i, int nv) { return i < 0 ? 0 : (i >= nv ? nv - 1 : i); }

__global__ void __launch_bounds__(256) k_mesh_faces(int nf, int nv, const int* __restrict__ faces,
                                                    const int* __restrict__ vertex_ids, int* __restrict__ face_ids) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int i0 = vertex_ids[clamp_index(faces[3 * (size_t)f], nv)];
  const int i1 = vertex_ids[clamp_index(faces[3 * (size_t)f + 1], nv)];
  const int i2 = vertex_ids[clamp_index(faces[3 * (size_t)f + 2], nv)];
  face_ids[f] = (i0 == i1 || i0 == i2) ? i0 : (i1 == i2 ? i1 : i0);
}

__device__ __forceinline__ int lower_bound(const unsigned* __restrict__ a, int n, unsigned x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) k_mesh_lut(int C, int nf, int nv, const unsigned* __restrict__ fkey2,
                                                  const int* __restrict__ fval2, const int* __restrict__ faces,
                                                  const float* __restrict__ verts, double* __restrict__ lut) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int a = lower_bound(fkey2, nf, (unsigned)c), b = lower_bound(fkey2, nf, (unsigned)c + 1u);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int i = a; i < b; ++i) {
    int f = fval2[i];
    if ((unsigned)f >= (unsigned)nf) f = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const size_t v = (size_t)clamp_index(faces[3 * (size_t)f + j], nv);
      sx += (double)verts[3 * v];
      sy += (double)verts[3 * v + 1];
      sz += (double)verts[3 * v + 2];
    }
  }
  const double n = (double)(3ll * (b - a));
  const double nan = __longlong_as_double(0x7FF8000000000000ll);  // 0 / 0, with the bits pinned
  lut[3 * (size_t)c] = b > a ? sx / n : nan;
  lut[3 * (size_t)c + 1] = b > a ? sy / n : nan;
  lut[3 * (size_t)c + 2] = b > a ? sz / n : nan;
}

// stable sort of (key, value) pairs on key bits [0, end_bit); the temporary storage rocPRIM asks for
// must fit the workspace's share
template <typename K>
static int sort_pairs(const MWs& w, const K* kin, K* kout, const int* vin, int* vout, int n, int end_bit,
                      hipStream_t st) {
  size_t need = 0;
  hipError_t e = rocprim::radix_sort_pairs((void*)nullptr, need, kin, kout, vin, vout, (size_t)n, 0u,
                                           (unsigned)end_bit, st);
  if (e == hipSuccess && need > w.temp_bytes) {
    set_error("zp_mesh_code: the sort needs %zu bytes of temporary storage, the workspace holds %zu", need,
              w.temp_bytes);
    return ZP_ERR_HIP;
  }
  if (e == hipSuccess)
    e = rocprim::radix_sort_pairs(w.temp, need, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)end_bit, st);
  if (e != hipSuccess) {
    set_error("zp_mesh_code: sort failed: %s", hipGetErrorString(e));
    return ZP_ERR_HIP;
  }
  return ZP_OK;
}

// ---- d-ary split (zp_mesh_code_radix) -------------------------------------------------------------
// A level's d^l groups lie contiguous as above; the d centres of group g are slots g * d .. g * d + d - 1
// of the centre, sum and seed-key arrays.  A block covers RX_POS consecutive positions.  Every group
// holds at least d vertices (include/zp.h), so those positions span at most RX_POS / d + 1 groups, that
// is RX_POS + d slots: the block stages every centre it can meet in LDS and sums per slot there (64-bit
// integer LDS atomics), then merges the slots it touched into the global sums with integer atomics.  No
// thread holds more than one running minimum, whatever d is.

constexpr int RX_ITEMS = 4;                // positions per thread
constexpr int RX_POS = 256 * RX_ITEMS;     // positions per block
constexpr int RX_SLOTS = RX_POS + 256;     // (group, class) slots a block can meet, d <= 256
constexpr int RX_GROUPS = RX_POS / 4 + 1;  // groups a block can meet, d >= 4
constexpr int RX_SCORE_BITS = 43;          // |D_j - min D_i| < 2^42, biased by 2^42

struct RWs : MWs {  // of MWs: cen, bcen and cnt0 stay unused; sums is [C][4], far [C]
  int4* rcen;       // [C] centres of the running attempt, slot g * d + j (w unused)
  int4* rbcen;      // [C] of the best attempt
  int* digit;       // [nv] class of sorted position p once a peel has taken it, else -1
  int* urem;        // [2][C / d] |U_j| of every group, double-buffered over the peels
};

static bool radix_sizes_ok(int nv, int nf, int divide, int levels) {
  if (divide < 4 || divide > 256 || (divide & (divide - 1)) || levels < 1 || levels > 16) return false;
  const int s = __builtin_ctz((unsigned)divide);
  return s * levels <= 16 && nv >= (1 << (s * levels)) && nv <= (1 << M_IDX_BITS) && nf >= 1 && nf <= (1 << 24);
}

// C = d^levels.  `key` doubles as the seeding's running minimum (u64 [nv]): the peel starts after it.
inline RWs rx_carve(void* ws, int nv, int nf, int C, int d, size_t* total) {
  char* p = (char*)ws;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* r = p + o;
    o = m_align(o + bytes);
    return (void*)r;
  };
  const size_t G = (size_t)C / d, nmax = (size_t)(nv > nf ? nv : nf);
  RWs w;
  w.cen = w.bcen = nullptr;
  w.cnt0 = nullptr;
  w.q = (int4*)take((size_t)nv * 16);
  w.gid = (int*)take((size_t)nv * 4);
  w.gs = (unsigned*)take((size_t)nv * 4);
  w.order = (int*)take((size_t)nv * 4);
  w.iota = (int*)take(nmax * 4);
  w.key = (u64*)take((size_t)nv * 8);
  w.key2 = (u64*)take((size_t)nv * 8);
  w.val2 = (int*)take((size_t)nv * 4);
  w.digit = (int*)take((size_t)nv * 4);
  w.gstart = (int*)take((G + 1) * 4);
  w.rcen = (int4*)take((size_t)C * 16);
  w.rbcen = (int4*)take((size_t)C * 16);
  w.sums = (u64*)take((size_t)C * 4 * 8);
  w.far = (u64*)take((size_t)C * 8);
  w.comp = (u64*)take(G * 8);
  w.bcomp = (u64*)take(G * 8);
  w.done = (int*)take(G * 4);
  w.urem = (int*)take(2 * G * 4);
  w.fkey2 = (unsigned*)take((size_t)nf * 4);
  w.fval2 = (int*)take((size_t)nf * 4);
  w.temp_bytes = (size_t)(M_TEMP_FIXED + M_TEMP_PER_ELEM * (long long)nmax);
  w.temp = take(w.temp_bytes);
  if (total) *total = o;
  return w;
}

// |delta| <= 2^20 per axis: three 32 x 32 -> 64-bit multiply-adds
__device__ __forceinline__ long long rx_dist2(const int4 p, const int4 c) {
  const int dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
  return (long long)dx * dx + (long long)dy * dy + (long long)dz * dz;
}

// the groups g0 .. g0 + ng - 1 met by this block's positions (ng = 0: group words out of range)
struct RxBlk {
  int p0, g0, ng;
};

__device__ __forceinline__ RxBlk rx_block(int nv, int G, int d, const unsigned* __restrict__ gs) {
  RxBlk b;
  b.p0 = blockIdx.x * RX_POS;
  const int last = (b.p0 + RX_POS < nv ? b.p0 + RX_POS : nv) - 1;
  const unsigned ga = gs[b.p0], gb = gs[last];
  b.g0 = (int)ga;
  b.ng = (ga < (unsigned)G && gb < (unsigned)G && gb >= ga) ? (int)(gb - ga) + 1 : 0;
  if (b.ng > RX_SLOTS / d) b.ng = RX_SLOTS / d;  // cannot happen while every group holds >= d vertices
  return b;
}

// calls f(p, r, t) for every valid position p of the block: r = its group / vertex / grid point, t = its
// group's index among the block's staged groups
template <typename F>
__device__ __forceinline__ void rx_positions(const RxBlk& b, int nv, int G, const unsigned* __restrict__ gs,
                                             const int* __restrict__ order, const int4* __restrict__ q, F f) {
#pragma unroll
  for (int k = 0; k < RX_ITEMS; ++k) {
    const int p = b.p0 + k * 256 + (int)threadIdx.x;
    MPos r;
    if (p >= nv || !load_pos(p, nv, G, gs, order, q, r)) continue;
    const int t = r.g - b.g0;
    if ((unsigned)t < (unsigned)b.ng) f(p, r, t);
  }
}

// seed 0 of group g: the grid point of its vertex at rank (draw * n) >> 32
__device__ __forceinline__ int4 rx_seed0(int g, int nv, const int* __restrict__ gstart, const int* __restrict__ order,
                                         const int4* __restrict__ q, const uint32_t* __restrict__ draws) {
  const int s = gstart[g];
  const long long n = (long long)gstart[g + 1] - s;
  long long pos = s + (long long)(((u64)draws[g] * (u64)(n > 0 ? n : 0)) >> 32);
  pos = pos < 0 ? 0 : (pos >= nv ? nv - 1 : pos);
  int v = order[pos];
  if ((unsigned)v >= (unsigned)nv) v = 0;
  return q[v];
}

__device__ __forceinline__ int4 rx_far_point(u64 key, int nv, const int4* __restrict__ q) {
  long long v = (long long)(M_IDX_MASK - (key & M_IDX_MASK));
  if (v >= nv) v = nv - 1;
  return q[v];
}

// seed j (1 <= j < d) of every group: the vertex with the largest minimum d^2 to seeds 0 .. j - 1, lowest
// index on ties, as the maximum of the key (min d^2 << 21 | 2^21 - 1 - index) in far[g * d + j].  Seed
// j - 1 is read back from far (seed 0: from the draw) and folded into mind, the running minimum.
__global__ void __launch_bounds__(256) k_rx_seed(int nv, int G, int d, int j, const unsigned* __restrict__ gs,
                                                 const int* __restrict__ order, const int4* __restrict__ q,
                                                 const int* __restrict__ gstart, const uint32_t* __restrict__ draws,
                                                 u64* __restrict__ mind, u64* __restrict__ far) {
  __shared__ int4 shc[RX_GROUPS];
  __shared__ u64 shk[RX_GROUPS];
  const RxBlk b = rx_block(nv, G, d, gs);
  const int ng = b.ng < RX_GROUPS ? b.ng : RX_GROUPS;
  for (int t = threadIdx.x; t < ng; t += 256) {
    const int g = b.g0 + t;
    shc[t] = j == 1 ? rx_seed0(g, nv, gstart, order, q, draws) : rx_far_point(far[(size_t)g * d + j - 1], nv, q);
    shk[t] = 0;
  }
  __syncthreads();
  rx_positions(b, nv, G, gs, order, q, [&](int p, const MPos& r, int t) {
    if (t >= ng) return;
    u64 m = (u64)rx_dist2(r.pt, shc[t]);
    if (j > 1) {
      const u64 o = mind[p];
      m = o < m ? o : m;
    }
    mind[p] = m;
    atomicMax(&shk[t], (m << M_IDX_BITS) | (M_IDX_MASK - (u64)r.v));
  });
  __syncthreads();
  for (int t = threadIdx.x; t < ng; t += 256)
    if (shk[t]) atomicMax(far + (size_t)(b.g0 + t) * d + j, shk[t]);
}

// per slot: the seeds become the running centres; sums, compactness and the done word start at zero
__global__ void __launch_bounds__(256) k_rx_seeded(int C, int d, int nv, const int* __restrict__ gstart,
                                                   const int* __restrict__ order, const int4* __restrict__ q,
                                                   const uint32_t* __restrict__ draws, const u64* __restrict__ far,
                                                   int4* __restrict__ cen, u64* __restrict__ sums,
                                                   u64* __restrict__ comp, int* __restrict__ done) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= C) return;
  const int g = t / d, j = t - g * d;
  cen[t] = j == 0 ? rx_seed0(g, nv, gstart, order, q, draws) : rx_far_point(far[t], nv, q);
#pragma unroll
  for (int i = 0; i < 4; ++i) sums[4 * (size_t)t + i] = 0;
  if (j == 0) {
    comp[g] = 0;
    done[g] = 0;
  }
}

// nearest of the centres c[0 .. n), ties to the lowest class; best = its d^2
__device__ __forceinline__ int rx_nearest(const int4* c, int n, const int4 pt, long long& best) {
  best = rx_dist2(pt, c[0]);
  int bj = 0;
#pragma unroll 4
  for (int j = 1; j < n; ++j) {
    const long long dd = rx_dist2(pt, c[j]);
    if (dd < best) {
      best = dd;
      bj = j;
    }
  }
  return bj;
}

__device__ __forceinline__ void rx_stage(const RxBlk& b, int d, const int4* __restrict__ cen, int4* shc) {
  for (int t = threadIdx.x; t < b.ng * d; t += 256) shc[t] = cen[(size_t)b.g0 * d + t];
}

// one Lloyd labelling: S xyz and the count of every (group, class) slot of the groups still running
__global__ void __launch_bounds__(256) k_rx_accum(int nv, int G, int d, const unsigned* __restrict__ gs,
                                                  const int* __restrict__ order, const int4* __restrict__ q,
                                                  const int4* __restrict__ cen, const int* __restrict__ done,
                                                  u64* __restrict__ sums) {
  __shared__ int4 shc[RX_SLOTS];
  __shared__ u64 acc[RX_SLOTS * 4];
  const RxBlk b = rx_block(nv, G, d, gs);
  rx_stage(b, d, cen, shc);
  for (int t = threadIdx.x; t < b.ng * d * 4; t += 256) acc[t] = 0;
  __syncthreads();
  rx_positions(b, nv, G, gs, order, q, [&](int p, const MPos& r, int t) {
    if (done[r.g]) return;
    long long best;
    const int slot = t * d + rx_nearest(shc + t * d, d, r.pt, best);
    atomicAdd(&acc[4 * slot], (u64)(long long)r.pt.x);
    atomicAdd(&acc[4 * slot + 1], (u64)(long long)r.pt.y);
    atomicAdd(&acc[4 * slot + 2], (u64)(long long)r.pt.z);
    atomicAdd(&acc[4 * slot + 3], 1ull);
  });
  __syncthreads();
  for (int t = threadIdx.x; t < b.ng * d; t += 256) {
    if (!acc[4 * t + 3]) continue;
    u64* dst = sums + 4 * ((size_t)b.g0 * d + t);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (acc[4 * t + i]) atomicAdd(dst + i, acc[4 * t + i]);
  }
}

// per slot: the new centre of a non-empty class; a group stops after the step in which the largest of its
// d centre shifts^2 is <= eps2.  The d slots of a group sit in one block (d divides 256).
__global__ void __launch_bounds__(256) k_rx_update(int C, int d, long long eps2, int4* __restrict__ cen,
                                                   u64* __restrict__ sums, int* __restrict__ done) {
  __shared__ u64 worst[64];
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int g = t / d, j = t - g * d, lg = (int)threadIdx.x / d;
  if (threadIdx.x < 64) worst[threadIdx.x] = 0;
  const bool live = t < C && !done[g];
  __syncthreads();
  if (live) {
    u64* s = sums + 4 * (size_t)t;
    const long long n = (long long)s[3];
    if (n > 0) {  // an empty class keeps its centre
      const int4 o = cen[t];
      const long long cx = floor_div(2 * (long long)s[0] + n, 2 * n), cy = floor_div(2 * (long long)s[1] + n, 2 * n),
                      cz = floor_div(2 * (long long)s[2] + n, 2 * n);
      const long long dx = cx - o.x, dy = cy - o.y, dz = cz - o.z;
      cen[t] = make_int4((int)cx, (int)cy, (int)cz, 0);
      atomicMax(&worst[lg], (u64)(dx * dx + dy * dy + dz * dz));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = 0;
  }
  __syncthreads();
  if (live && j == 0 && worst[lg] <= (u64)eps2) done[g] = 1;
}

__global__ void __launch_bounds__(256) k_rx_comp(int nv, int G, int d, const unsigned* __restrict__ gs,
                                                 const int* __restrict__ order, const int4* __restrict__ q,
                                                 const int4* __restrict__ cen, u64* __restrict__ comp) {
  __shared__ int4 shc[RX_SLOTS];
  __shared__ u64 acc[RX_GROUPS];
  const RxBlk b = rx_block(nv, G, d, gs);
  const int ng = b.ng < RX_GROUPS ? b.ng : RX_GROUPS;
  rx_stage(b, d, cen, shc);
  for (int t = threadIdx.x; t < ng; t += 256) acc[t] = 0;
  __syncthreads();
  rx_positions(b, nv, G, gs, order, q, [&](int p, const MPos& r, int t) {
    if (t >= ng) return;
    long long best;
    rx_nearest(shc + t * d, d, r.pt, best);
    atomicAdd(&acc[t], (u64)best);
  });
  __syncthreads();
  for (int t = threadIdx.x; t < ng; t += 256)
    if (acc[t]) atomicAdd(comp + b.g0 + t, acc[t]);
}

// per slot: keep the running centres where the attempt's compactness is lower (ties: the earlier attempt)
__global__ void __launch_bounds__(256) k_rx_best(int C, int d, int attempt, const int4* __restrict__ cen,
                                                 const u64* __restrict__ comp, int4* __restrict__ bcen,
                                                 u64* __restrict__ bcomp) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int g = t / d, j = t - g * d;
  const bool better = t < C && (attempt == 0 || comp[g] < bcomp[g]);
  __syncthreads();  // every slot of the group has read bcomp[g]
  if (!better) return;
  bcen[t] = cen[t];
  if (j == 0) bcomp[g] = comp[g];
}

// peel j: the sort key (group, taken, D_j - min_{i > j} D_i + 2^42) of every position under the best
// centres; the distances are computed again in every peel, none is kept
__global__ void __launch_bounds__(256) k_rx_score(int nv, int G, int d, int j, const unsigned* __restrict__ gs,
                                                  const int* __restrict__ order, const int4* __restrict__ q,
                                                  const int4* __restrict__ bcen, int* __restrict__ digit,
                                                  u64* __restrict__ key) {
  __shared__ int4 shc[RX_SLOTS];
  const RxBlk b = rx_block(nv, G, d, gs);
  rx_stage(b, d, bcen, shc);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < RX_ITEMS; ++k) {
    const int p = b.p0 + k * 256 + (int)threadIdx.x;
    if (p >= nv) continue;
    MPos r;
    if (!load_pos(p, nv, G, gs, order, q, r) || (unsigned)(r.g - b.g0) >= (unsigned)b.ng) {
      key[p] = ~0ull;
      continue;
    }
    if (j == 0) digit[p] = -1;
    if (j > 0 && digit[p] >= 0) {
      key[p] = ((u64)r.g << (RX_SCORE_BITS + 1)) | (1ull << RX_SCORE_BITS);
      continue;
    }
    const int4* c = shc + (r.g - b.g0) * d;
    long long rest;
    rx_nearest(c + j + 1, d - j - 1, r.pt, rest);
    const long long s = rx_dist2(r.pt, c[j]) - rest + (1ll << (RX_SCORE_BITS - 1));
    key[p] = ((u64)r.g << (RX_SCORE_BITS + 1)) | (u64)s;
  }
}

// peel j over the positions in key order: a group's run still starts at gstart[g], its untaken vertices
// first, by score then index.  Class j takes the first floor(|U_j| / (d - j)); the last peel (j = d - 2)
// leaves the rest to class d - 1.  The run's first element carries |U_(j + 1)| to the next peel.
__global__ void __launch_bounds__(256) k_rx_take(int nv, int G, int d, int j, int shift, const u64* __restrict__ key2,
                                                 const int* __restrict__ val2, const int* __restrict__ gstart,
                                                 const int* __restrict__ order, const int* __restrict__ ucur,
                                                 int* __restrict__ unext, int* __restrict__ digit,
                                                 int* __restrict__ gid, int* __restrict__ vertex_ids) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const u64 k = key2[i];
  const u64 g = k >> (RX_SCORE_BITS + 1);
  if (g >= (u64)G) return;
  const int s = gstart[g];
  const int u = j == 0 ? gstart[g + 1] - s : ucur[g];
  const int quota = u > 0 ? u / (d - j) : 0;
  if (i == s) unext[g] = u - quota;
  if ((k >> RX_SCORE_BITS) & 1) return;  // taken by an earlier peel
  const int p = val2[i];
  if ((unsigned)p >= (unsigned)nv) return;
  const int v = order[p];
  if ((unsigned)v >= (unsigned)nv) return;
  const int c = i - s < quota ? j : (j == d - 2 ? d - 1 : -1);
  if (c < 0) return;
  digit[p] = c;
  gid[v] = (int)g * d + c;
  vertex_ids[v] |= c << shift;
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_mesh_code_ws_bytes(int nv, int nf, int bits) {
  if (!mesh_sizes_ok(nv, nf, bits)) return -1;
  size_t total = 0;
  m_carve(nullptr, nv, nf, bits, &total);
  return (long long)total;
}

extern "C" int zp_mesh_code(const float* verts, int nv, const int* faces, int nf, int bits, int attempts,
                            int iterations, int grid_log2, long long eps2_q, const uint32_t* draws, int* vertex_ids,
                            int* face_ids, double* lut, void* ws, void* stream) {
  ZP_CHECK_ARG(bits >= 1 && bits <= 16, "zp_mesh_code: bits %d outside 1..16", bits);
  ZP_CHECK_ARG(nv >= (1 << bits), "zp_mesh_code: nv %d below 2^bits = %d", nv, 1 << bits);
  ZP_CHECK_ARG(mesh_sizes_ok(nv, nf, bits), "zp_mesh_code: sizes nv %d nf %d out of range (nv <= 2^21, 1 <= nf <= 2^24)",
               nv, nf);
  ZP_CHECK_ARG(attempts >= 1 && attempts <= 64, "zp_mesh_code: attempts %d outside 1..64", attempts);
  ZP_CHECK_ARG(iterations >= 1 && iterations <= 1000, "zp_mesh_code: iterations %d outside 1..1000", iterations);
  ZP_CHECK_ARG(grid_log2 >= -40 && grid_log2 <= 40, "zp_mesh_code: grid_log2 %d outside -40..40", grid_log2);
  ZP_CHECK_ARG(eps2_q >= 0, "zp_mesh_code: eps2_q must be >= 0");
  ZP_CHECK_ARG(verts && faces && draws && vertex_ids && face_ids && lut && ws,
               "zp_mesh_code: NULL pointer (verts, faces, draws, vertex_ids, face_ids, lut, ws are required)");
  hipStream_t st = (hipStream_t)stream;
  const MWs w = m_carve(ws, nv, nf, bits, nullptr);
  const int nmax = nv > nf ? nv : nf;
  const int vblocks = ceil_div(nv, 256), rblocks = ceil_div(nv, 256 * M_ITEMS);
  const size_t draws_per_attempt = ((size_t)1 << bits) - 1;

  hipLaunchKernelGGL(k_mesh_quant, dim3(vblocks), dim3(256), 0, st, verts, nv, grid_log2, w.q);
  ZP_LAUNCH_CHECK("zp_mesh_code quant");
  hipLaunchKernelGGL(k_mesh_init, dim3(ceil_div(nmax, 256)), dim3(256), 0, st, nv, nmax, w.gs, w.order, w.iota,
                     w.gstart, vertex_ids);
  ZP_LAUNCH_CHECK("zp_mesh_code init");

  for (int l = 0; l < bits; ++l) {
    const int G = 1 << l, gblocks = ceil_div(G, 256);
    for (int a = 0; a < attempts; ++a) {
      hipLaunchKernelGGL(k_mesh_seed0, dim3(gblocks), dim3(256), 0, st, G, nv, (const int*)w.gstart,
                         (const int*)w.order, (const int4*)w.q, draws + a * draws_per_attempt + (size_t)(G - 1), w.cen,
                         w.far);
      hipLaunchKernelGGL(k_mesh_far, dim3(rblocks), dim3(256), 0, st, nv, G, (const unsigned*)w.gs,
                         (const int*)w.order, (const int4*)w.q, (const int*)w.cen, w.far);
      hipLaunchKernelGGL(k_mesh_seed1, dim3(gblocks), dim3(256), 0, st, G, nv, (const int4*)w.q, (const u64*)w.far,
                         w.cen, w.sums, w.comp, w.done);
      ZP_LAUNCH_CHECK("zp_mesh_code seeds");
      for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_mesh_accum, dim3(rblocks), dim3(256), 0, st, nv, G, (const unsigned*)w.gs,
                           (const int*)w.order, (const int4*)w.q, (const int*)w.cen, (const int*)w.done, w.sums);
        hipLaunchKernelGGL(k_mesh_update, dim3(gblocks), dim3(256), 0, st, G, eps2_q, w.cen, w.sums, w.done);
      }
      ZP_LAUNCH_CHECK("zp_mesh_code lloyd");
      hipLaunchKernelGGL(k_mesh_comp, dim3(rblocks), dim3(256), 0, st, nv, G, (const unsigned*)w.gs,
                         (const int*)w.order, (const int4*)w.q, (const int*)w.cen, w.comp);
      hipLaunchKernelGGL(k_mesh_best, dim3(gblocks), dim3(256), 0, st, G, a, (const int*)w.cen, (const u64*)w.comp,
                         w.bcen, w.bcomp, w.cnt0);
      ZP_LAUNCH_CHECK("zp_mesh_code compactness");
    }
    hipLaunchKernelGGL(k_mesh_final, dim3(rblocks), dim3(256), 0, st, nv, G, (const unsigned*)w.gs,
                       (const int*)w.order, (const int4*)w.q, (const int*)w.bcen, w.key, w.cnt0);
    ZP_LAUNCH_CHECK("zp_mesh_code labels");
    int rc = sort_pairs<u64>(w, w.key, w.key2, w.order, w.val2, nv, M_D2_BITS + 1 + l, st);
    if (rc != ZP_OK) return rc;
    hipLaunchKernelGGL(k_mesh_balance, dim3(vblocks), dim3(256), 0, st, nv, G, bits - 1 - l, (const u64*)w.key2,
                       (const int*)w.val2, (const int*)w.gstart, (const u64*)w.cnt0, w.gid, vertex_ids);
    ZP_LAUNCH_CHECK("zp_mesh_code balance");
    if (l + 1 < bits) {
      rc = sort_pairs<unsigned>(w, (const unsigned*)w.gid, w.gs, w.iota, w.order, nv, l + 1, st);
      if (rc != ZP_OK) return rc;
      hipLaunchKernelGGL(k_mesh_bounds, dim3(vblocks), dim3(256), 0, st, nv, 2 * G, (const unsigned*)w.gs, w.gstart);
      ZP_LAUNCH_CHECK("zp_mesh_code bounds");
    }
  }

  hipLaunchKernelGGL(k_mesh_faces, dim3(ceil_div(nf, 256)), dim3(256), 0, st, nf, nv, faces, (const int*)vertex_ids,
                     face_ids);
  ZP_LAUNCH_CHECK("zp_mesh_code faces");
  const int rc = sort_pairs<unsigned>(w, (const unsigned*)face_ids, w.fkey2, w.iota, w.fval2, nf, bits, st);
  if (rc != ZP_OK) return rc;
  const int C = 1 << bits;
  hipLaunchKernelGGL(k_mesh_lut, dim3(ceil_div(C, 256)), dim3(256), 0, st, C, nf, nv, (const unsigned*)w.fkey2,
                     (const int*)w.fval2, faces, verts, lut);
  ZP_LAUNCH_CHECK("zp_mesh_code lut");
  return ZP_OK;
}

extern "C" long long zp_mesh_code_radix_ws_bytes(int nv, int nf, int divide, int levels) {
  if (!radix_sizes_ok(nv, nf, divide, levels)) return -1;
  size_t total = 0;
  rx_carve(nullptr, nv, nf, 1 << (__builtin_ctz((unsigned)divide) * levels), divide, &total);
  return (long long)total;
}

extern "C" int zp_mesh_code_radix(const float* verts, int nv, const int* faces, int nf, int divide, int levels,
                                  int attempts, int iterations, int grid_log2, long long eps2_q, const uint32_t* draws,
                                  int* vertex_ids, int* face_ids, double* lut, void* ws, void* stream) {
  ZP_CHECK_ARG(divide != 2, "zp_mesh_code_radix: divide 2 is the binary split: call zp_mesh_code");
  ZP_CHECK_ARG(divide >= 4 && divide <= 256 && !(divide & (divide - 1)),
               "zp_mesh_code_radix: divide %d is no power of two in 4..256", divide);
  const int d = divide, s = __builtin_ctz((unsigned)d);
  ZP_CHECK_ARG(levels >= 1 && s * (long long)levels <= 16,
               "zp_mesh_code_radix: levels %d: divide^levels must lie in divide..65536", levels);
  const int C = 1 << (s * levels);
  ZP_CHECK_ARG(nv >= C, "zp_mesh_code_radix: nv %d below divide^levels = %d", nv, C);
  ZP_CHECK_ARG(radix_sizes_ok(nv, nf, d, levels),
               "zp_mesh_code_radix: sizes nv %d nf %d out of range (nv <= 2^21, 1 <= nf <= 2^24)", nv, nf);
  ZP_CHECK_ARG(attempts >= 1 && attempts <= 64, "zp_mesh_code_radix: attempts %d outside 1..64", attempts);
  ZP_CHECK_ARG(iterations >= 1 && iterations <= 1000, "zp_mesh_code_radix: iterations %d outside 1..1000", iterations);
  ZP_CHECK_ARG(grid_log2 >= -40 && grid_log2 <= 40, "zp_mesh_code_radix: grid_log2 %d outside -40..40", grid_log2);
  ZP_CHECK_ARG(eps2_q >= 0, "zp_mesh_code_radix: eps2_q must be >= 0");
  ZP_CHECK_ARG(verts && faces && draws && vertex_ids && face_ids && lut && ws,
               "zp_mesh_code_radix: NULL pointer (verts, faces, draws, vertex_ids, face_ids, lut, ws are required)");
  hipStream_t st = (hipStream_t)stream;
  const RWs w = rx_carve(ws, nv, nf, C, d, nullptr);
  const int nmax = nv > nf ? nv : nf, Gmax = C / d;
  const int vblocks = ceil_div(nv, 256), rblocks = ceil_div(nv, RX_POS);
  const size_t draws_per_attempt = ((size_t)C - 1) / (size_t)(d - 1);

  hipLaunchKernelGGL(k_mesh_quant, dim3(vblocks), dim3(256), 0, st, verts, nv, grid_log2, w.q);
  ZP_LAUNCH_CHECK("zp_mesh_code_radix quant");
  hipLaunchKernelGGL(k_mesh_init, dim3(ceil_div(nmax, 256)), dim3(256), 0, st, nv, nmax, w.gs, w.order, w.iota,
                     w.gstart, vertex_ids);
  ZP_LAUNCH_CHECK("zp_mesh_code_radix init");

  for (int l = 0; l < levels; ++l) {
    const int G = 1 << (s * l), S = G * d, sblocks = ceil_div(S, 256);  // S slots: (group, class)
    const size_t first = ((size_t)G - 1) / (size_t)(d - 1);
    for (int a = 0; a < attempts; ++a) {
      const uint32_t* dr = draws + a * draws_per_attempt + first;
      const hipError_t e = hipMemsetAsync(w.far, 0, (size_t)S * 8, st);
      if (e != hipSuccess) {
        set_error("zp_mesh_code_radix: clearing the seed keys failed: %s", hipGetErrorString(e));
        return ZP_ERR_HIP;
      }
      for (int j = 1; j < d; ++j)
        hipLaunchKernelGGL(k_rx_seed, dim3(rblocks), dim3(256), 0, st, nv, G, d, j, (const unsigned*)w.gs,
                           (const int*)w.order, (const int4*)w.q, (const int*)w.gstart, dr, w.key, w.far);
      hipLaunchKernelGGL(k_rx_seeded, dim3(sblocks), dim3(256), 0, st, S, d, nv, (const int*)w.gstart,
                         (const int*)w.order, (const int4*)w.q, dr, (const u64*)w.far, w.rcen, w.sums, w.comp, w.done);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix seeds");
      for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_rx_accum, dim3(rblocks), dim3(256), 0, st, nv, G, d, (const unsigned*)w.gs,
                           (const int*)w.order, (const int4*)w.q, (const int4*)w.rcen, (const int*)w.done, w.sums);
        hipLaunchKernelGGL(k_rx_update, dim3(sblocks), dim3(256), 0, st, S, d, eps2_q, w.rcen, w.sums, w.done);
      }
      ZP_LAUNCH_CHECK("zp_mesh_code_radix lloyd");
      hipLaunchKernelGGL(k_rx_comp, dim3(rblocks), dim3(256), 0, st, nv, G, d, (const unsigned*)w.gs,
                         (const int*)w.order, (const int4*)w.q, (const int4*)w.rcen, w.comp);
      hipLaunchKernelGGL(k_rx_best, dim3(sblocks), dim3(256), 0, st, S, d, a, (const int4*)w.rcen, (const u64*)w.comp,
                         w.rbcen, w.bcomp);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix compactness");
    }
    for (int j = 0; j < d - 1; ++j) {
      hipLaunchKernelGGL(k_rx_score, dim3(rblocks), dim3(256), 0, st, nv, G, d, j, (const unsigned*)w.gs,
                         (const int*)w.order, (const int4*)w.q, (const int4*)w.rbcen, w.digit, w.key);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix scores");
      const int rc = sort_pairs<u64>(w, w.key, w.key2, w.iota, w.val2, nv, RX_SCORE_BITS + 1 + s * l, st);
      if (rc != ZP_OK) return rc;
      hipLaunchKernelGGL(k_rx_take, dim3(vblocks), dim3(256), 0, st, nv, G, d, j, s * (levels - 1 - l),
                         (const u64*)w.key2, (const int*)w.val2, (const int*)w.gstart, (const int*)w.order,
                         (const int*)(w.urem + (size_t)(j & 1) * Gmax), w.urem + (size_t)((j + 1) & 1) * Gmax, w.digit,
                         w.gid, vertex_ids);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix peel");
    }
    if (l + 1 < levels) {
      const int rc = sort_pairs<unsigned>(w, (const unsigned*)w.gid, w.gs, w.iota, w.order, nv, s * (l + 1), st);
      if (rc != ZP_OK) return rc;
      hipLaunchKernelGGL(k_mesh_bounds, dim3(vblocks), dim3(256), 0, st, nv, S, (const unsigned*)w.gs, w.gstart);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix bounds");
    }
  }

  hipLaunchKernelGGL(k_mesh_faces, dim3(ceil_div(nf, 256)), dim3(256), 0, st, nf, nv, faces, (const int*)vertex_ids,
                     face_ids);
  ZP_LAUNCH_CHECK("zp_mesh_code_radix faces");
  const int rc = sort_pairs<unsigned>(w, (const unsigned*)face_ids, w.fkey2, w.iota, w.fval2, nf, s * levels, st);
  if (rc != ZP_OK) return rc;
  hipLaunchKernelGGL(k_mesh_lut, dim3(ceil_div(C, 256)), dim3(256), 0, st, C, nf, nv, (const unsigned*)w.fkey2,
                     (const int*)w.fval2, faces, verts, lut);
  ZP_LAUNCH_CHECK("zp_mesh_code_radix lut");
  return ZP_OK;
}
