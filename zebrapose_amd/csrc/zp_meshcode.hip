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
// The stable radix sort (sort_pairs, zp_mesh.h) (a) regroups the vertices by child group after each
// level, (b) ranks a group's vertices by (class, d^2 to the other centre descending, index ascending)
// for the balance, (c) groups the faces by class for the LUT.  The LUT sums are f64 additions in
// ascending face index, vertex 0, 1, 2: one thread per class walks its faces.
//
// zp_mesh_code_radix (zp_meshcode_radix.hip) splits d ways per level for the d-ary codes.  It shares
// the grid, the group layout, the regrouping, the faces and the LUT: those kernels live here, behind
// the driver steps mesh_prologue / mesh_regroup / mesh_epilogue and the argument checks both entry
// points make (mesh_check_args), all declared in zp_mesh.h beside the workspace part (MeshWs) and the
// device helpers the two splits have in common.  The per-vertex kernels of the two splits stay apart:
// they are different algorithms (run sums in registers here, centres staged in LDS there).
#include "zp_mesh.h"

// the LUT's f64 steps are single IEEE operations (the Makefile passes -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace zp {

constexpr int M_SAT = (1 << 19) - 1;
constexpr int M_D2_BITS = 42;  // d^2 <= 3 * (2^20)^2 < 2^42
constexpr u64 M_D2_MASK = (1ull << M_D2_BITS) - 1;
constexpr int M_ITEMS = 8;  // positions per thread of the per-vertex kernels
constexpr int M_NSUM = 7;   // S0 xyz, S1 xyz, n0 | n1 << 32

struct BinWs {  // beside MeshWs; G = 2^(bits - 1) groups
  int* cen;     // [G][6] c0 xyz, c1 xyz of the running attempt
  int* bcen;    // [G][6] of the best attempt
  u64* sums;    // [G][M_NSUM]
  u64* far;     // [G] farthest-point key
  u64* cnt0;    // [G] class-0 count under the best centres
};

static size_t m_carve(void* ws, int nv, int nf, int bits, MeshWs& w, BinWs& b) {
  Carver c(ws);
  const size_t G = (size_t)1 << (bits - 1);
  b.cen = c.take<int>(G * 6);
  b.bcen = c.take<int>(G * 6);
  b.sums = c.take<u64>(G * M_NSUM);
  b.far = c.take<u64>(G);
  b.cnt0 = c.take<u64>(G);
  w = carve_mesh(c, nv, nf, G);
  return c.total();
}

static bool mesh_sizes_ok(int nv, int nf, int bits) {
  return bits >= 1 && bits <= 16 && nv >= (1 << bits) && mesh_range_ok(nv, nf);
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
  const int4 pt = seed0(g, nv, gstart, order, q, draws);
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
  const int4 pt = far_point(far[g], nv, q);
  cen[6 * (size_t)g + 3] = pt.x;
  cen[6 * (size_t)g + 4] = pt.y;
  cen[6 * (size_t)g + 5] = pt.z;
#pragma unroll
  for (int i = 0; i < M_NSUM; ++i) sums[(size_t)g * M_NSUM + i] = 0;
  comp[g] = 0;
  done[g] = 0;
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

// ---- the driver steps both entry points share (zp_mesh.h) ----------------------------------------

int mesh_check_args(const char* who, int nv, int nf, int attempts, int iterations, int grid_log2, long long eps2_q,
                    bool pointers) {
  ZP_CHECK_ARG(mesh_range_ok(nv, nf), "%s: sizes nv %d nf %d out of range (nv <= 2^21, 1 <= nf <= 2^24)", who, nv, nf);
  ZP_CHECK_ARG(attempts >= 1 && attempts <= 64, "%s: attempts %d outside 1..64", who, attempts);
  ZP_CHECK_ARG(iterations >= 1 && iterations <= 1000, "%s: iterations %d outside 1..1000", who, iterations);
  ZP_CHECK_ARG(grid_log2 >= -40 && grid_log2 <= 40, "%s: grid_log2 %d outside -40..40", who, grid_log2);
  ZP_CHECK_ARG(eps2_q >= 0, "%s: eps2_q must be >= 0", who);
  ZP_CHECK_ARG(pointers, "%s: NULL pointer (verts, faces, draws, vertex_ids, face_ids, lut, ws are required)", who);
  return ZP_OK;
}

// ZP_LAUNCH_CHECK under the entry point's name
static int launched(const char* who, const char* step) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return ZP_OK;
  set_error("%s %s: launch failed: %s", who, step, hipGetErrorString(e));
  return ZP_ERR_HIP;
}

int mesh_prologue(const char* who, const MeshWs& w, const float* verts, int nv, int nf, int grid_log2,
                  int* vertex_ids, hipStream_t st) {
  const int nmax = nv > nf ? nv : nf;
  hipLaunchKernelGGL(k_mesh_quant, dim3(ceil_div(nv, 256)), dim3(256), 0, st, verts, nv, grid_log2, w.q);
  if (const int rc = launched(who, "quant")) return rc;
  hipLaunchKernelGGL(k_mesh_init, dim3(ceil_div(nmax, 256)), dim3(256), 0, st, nv, nmax, w.gs, w.order, w.iota,
                     w.gstart, vertex_ids);
  return launched(who, "init");
}

int mesh_regroup(const char* who, const MeshWs& w, int nv, int end_bit, int G, hipStream_t st) {
  const int rc = sort_pairs((const unsigned*)w.gid, w.gs, w.iota, w.order, nv, end_bit, w.temp, w.temp_bytes, st, who);
  if (rc != ZP_OK) return rc;
  hipLaunchKernelGGL(k_mesh_bounds, dim3(ceil_div(nv, 256)), dim3(256), 0, st, nv, G, (const unsigned*)w.gs, w.gstart);
  return launched(who, "bounds");
}

int mesh_epilogue(const char* who, const MeshWs& w, const float* verts, int nv, const int* faces, int nf,
                  int code_bits, const int* vertex_ids, int* face_ids, double* lut, hipStream_t st) {
  hipLaunchKernelGGL(k_mesh_faces, dim3(ceil_div(nf, 256)), dim3(256), 0, st, nf, nv, faces, vertex_ids, face_ids);
  if (const int rc = launched(who, "faces")) return rc;
  const int rc = sort_pairs((const unsigned*)face_ids, w.fkey2, w.iota, w.fval2, nf, code_bits, w.temp, w.temp_bytes,
                            st, who);
  if (rc != ZP_OK) return rc;
  const int C = 1 << code_bits;
  hipLaunchKernelGGL(k_mesh_lut, dim3(ceil_div(C, 256)), dim3(256), 0, st, C, nf, nv, (const unsigned*)w.fkey2,
                     (const int*)w.fval2, faces, verts, lut);
  return launched(who, "lut");
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_mesh_code_ws_bytes(int nv, int nf, int bits) {
  if (!mesh_sizes_ok(nv, nf, bits)) return -1;
  MeshWs w;
  BinWs b;
  return (long long)m_carve(nullptr, nv, nf, bits, w, b);
}

extern "C" int zp_mesh_code(const float* verts, int nv, const int* faces, int nf, int bits, int attempts,
                            int iterations, int grid_log2, long long eps2_q, const uint32_t* draws, int* vertex_ids,
                            int* face_ids, double* lut, void* ws, void* stream) {
  const char* who = "zp_mesh_code";
  ZP_CHECK_ARG(bits >= 1 && bits <= 16, "zp_mesh_code: bits %d outside 1..16", bits);
  ZP_CHECK_ARG(nv >= (1 << bits), "zp_mesh_code: nv %d below 2^bits = %d", nv, 1 << bits);
  int rc = mesh_check_args(who, nv, nf, attempts, iterations, grid_log2, eps2_q,
                           verts && faces && draws && vertex_ids && face_ids && lut && ws);
  if (rc != ZP_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MeshWs w;
  BinWs b;
  m_carve(ws, nv, nf, bits, w, b);
  const int vblocks = ceil_div(nv, 256), rblocks = ceil_div(nv, 256 * M_ITEMS);
  const size_t draws_per_attempt = ((size_t)1 << bits) - 1;

  if ((rc = mesh_prologue(who, w, verts, nv, nf, grid_log2, vertex_ids, st)) != ZP_OK) return rc;

  for (int l = 0; l < bits; ++l) {
    const int G = 1 << l, gblocks = ceil_div(G, 256);
    for (int a = 0; a < attempts; ++a) {
      hipLaunchKernelGGL(k_mesh_seed0, dim3(gblocks), dim3(256), 0, st, G, nv, (const int*)w.gstart,
                         (const int*)w.order, (const int4*)w.q, draws + a * draws_per_attempt + (size_t)(G - 1), b.cen,
                         b.far);
      hipLaunchKernelGGL(k_mesh_far, dim3(rblocks), dim3(256), 0, st, nv, G, (const unsigned*)w.gs,
                         (const int*)w.order, (const int4*)w.q, (const int*)b.cen, b.far);
      hipLaunchKernelGGL(k_mesh_seed1, dim3(gblocks), dim3(256), 0, st, G, nv, (const int4*)w.q, (const u64*)b.far,
                         b.cen, b.sums, w.comp, w.done);
      ZP_LAUNCH_CHECK("zp_mesh_code seeds");
      for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_mesh_accum, dim3(rblocks), dim3(256), 0, st, nv, G, (const unsigned*)w.gs,
                           (const int*)w.order, (const int4*)w.q, (const int*)b.cen, (const int*)w.done, b.sums);
        hipLaunchKernelGGL(k_mesh_update, dim3(gblocks), dim3(256), 0, st, G, eps2_q, b.cen, b.sums, w.done);
      }
      ZP_LAUNCH_CHECK("zp_mesh_code lloyd");
      hipLaunchKernelGGL(k_mesh_comp, dim3(rblocks), dim3(256), 0, st, nv, G, (const unsigned*)w.gs,
                         (const int*)w.order, (const int4*)w.q, (const int*)b.cen, w.comp);
      hipLaunchKernelGGL(k_mesh_best, dim3(gblocks), dim3(256), 0, st, G, a, (const int*)b.cen, (const u64*)w.comp,
                         b.bcen, w.bcomp, b.cnt0);
      ZP_LAUNCH_CHECK("zp_mesh_code compactness");
    }
    hipLaunchKernelGGL(k_mesh_final, dim3(rblocks), dim3(256), 0, st, nv, G, (const unsigned*)w.gs,
                       (const int*)w.order, (const int4*)w.q, (const int*)b.bcen, w.key, b.cnt0);
    ZP_LAUNCH_CHECK("zp_mesh_code labels");
    rc = sort_pairs(w.key, w.key2, w.order, w.val2, nv, M_D2_BITS + 1 + l, w.temp, w.temp_bytes, st, who);
    if (rc != ZP_OK) return rc;
    hipLaunchKernelGGL(k_mesh_balance, dim3(vblocks), dim3(256), 0, st, nv, G, bits - 1 - l, (const u64*)w.key2,
                       (const int*)w.val2, (const int*)w.gstart, (const u64*)b.cnt0, w.gid, vertex_ids);
    ZP_LAUNCH_CHECK("zp_mesh_code balance");
    if (l + 1 < bits && (rc = mesh_regroup(who, w, nv, l + 1, 2 * G, st)) != ZP_OK) return rc;
  }
  return mesh_epilogue(who, w, verts, nv, faces, nf, bits, vertex_ids, face_ids, lut, st);
}

