// Mesh upsampling: one pass of midpoint subdivision with an edge-length threshold (zp_mesh_subdivide).
// Reference: step 1 of the label-generation recipe Binary_Code_GT_Generator/Generate_GT.md (:90-92),
// "upsample the mesh until it has more than 2^16 vertices" with Meshlab's 'subdivision surface: mid
// point' filter, which the reference runs by hand.  The filter is restated with exact semantics that
// depend on the order of no summation and of no atomic (include/zp.h, zp_mesh_subdivide;
// tests/subdiv_ref.py is the executable definition):
//
//   edges    slot j of face (v0, v1, v2) is (vj, v(j+1)%3); an edge is the unordered index pair, key
//            (min << 32) | max, unique edges in ascending key order
//   len2     d = f64(a) - f64(b) per axis (exact), (dx dx + dy dy) + dz dz, every operation rounded once
//   split    len2 > abs2 and len2 > rel2 * max len2; over budget: the max_split longest, ties to the lower key
//   vertices old ones keep their index, split edges in key order get nv, nv + 1, ...;
//            midpoint f32((f64(a) + f64(b)) * 0.5)
//   faces    children of face i at the exclusive prefix sum of 1 + (its split edges), by the templates below
//
// One thread per edge slot, unique edge or face; nothing is read back.  The sort key packs the pair as
// (min << 21) | max (indices stay below 2^21), which orders like the 64-bit key.  Through the wrappers
// of zp_mesh.h (sort_pairs, inclusive_scan, exclusive_scan): the stable radix sort that brings equal
// edges together and, when a budget binds, ranks the qualifying edges by inverted length bits (stable
// over edges already in key order, so ties go to the lower key), and the integer scans (exact in any
// order) that number unique edges, new vertices and child faces.  The one atomic is a maximum over the
// bit patterns of non-negative doubles.  The size limits, the workspace carver and clamp_index are the
// mesh coders' (zp_mesh.h).
#include "zp_mesh.h"

#include <limits.h>

// len2 and the midpoints are single IEEE operations (the Makefile passes -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace zp {

struct SWs {
  u64* key;        // [E] slot keys; then the selection keys (inverted length bits)
  u64* key2;       // [E] their sorted copies
  u64* ekey;       // [E] key of unique edge e
  double* len2;    // [E] squared length of unique edge e (0 beyond the last)
  int* iota;       // [E] 0, 1, 2, ...
  int* val2;       // [E] slots in key order; then edges in selection order
  int* flag;       // [E] first slot of its edge; then: edge e splits
  int* scan;       // [E] inclusive scan of flag
  int* slot_edge;  // [E] unique edge of slot s
  int* fcnt;       // [nf] children of face f
  int* foff;       // [nf] first child of face f
  int* hdr;        // {n_unique_edges, outputs fit}
  void* temp;
  size_t temp_bytes;
};

inline SWs sd_carve(void* ws, int nf, size_t* total) {
  Carver c(ws);
  const size_t E = 3 * (size_t)nf;
  SWs w;
  w.key = c.take<u64>(E);
  w.key2 = c.take<u64>(E);
  w.ekey = c.take<u64>(E);
  w.len2 = c.take<double>(E);
  w.iota = c.take<int>(E);
  w.val2 = c.take<int>(E);
  w.flag = c.take<int>(E);
  w.scan = c.take<int>(E);
  w.slot_edge = c.take<int>(E);
  w.fcnt = c.take<int>(nf);
  w.foff = c.take<int>(nf);
  w.hdr = c.take<int>(64);
  w.temp_bytes = prim_temp_bytes(E);
  w.temp = c.take<char>(w.temp_bytes);
  if (total) *total = c.total();
  return w;
}

static bool sd_sizes_ok(int nv, int nf) { return nv >= 1 && mesh_range_ok(nv, nf); }

__device__ __forceinline__ double sd_len2(const float* __restrict__ a, const float* __restrict__ b) {
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// ---- unique edges ------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_sd_keys(int E, int nv, const int* __restrict__ faces, u64* __restrict__ key,
                                                 int* __restrict__ iota, double* __restrict__ max_len2) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= E) return;
  const int f = s / 3, j = s - 3 * f;
  const int a = clamp_index(faces[3 * (size_t)f + j], nv), b = clamp_index(faces[3 * (size_t)f + (j == 2 ? 0 : j + 1)], nv);
  key[s] = ((u64)(a < b ? a : b) << M_IDX_BITS) | (u64)(a < b ? b : a);
  iota[s] = s;
  if (s == 0) *max_len2 = 0.0;
}

__global__ void __launch_bounds__(256) k_sd_flag(int E, const u64* __restrict__ key2, int* __restrict__ flag) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= E) return;
  flag[p] = (p == 0 || key2[p] != key2[p - 1]) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_sd_rank(int E, const u64* __restrict__ key2, const int* __restrict__ val2,
                                                 const int* __restrict__ flag, const int* __restrict__ scan,
                                                 int* __restrict__ slot_edge, u64* __restrict__ ekey,
                                                 int* __restrict__ hdr) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= E) return;
  const int e = scan[p] - 1, s = val2[p];
  if (p == E - 1) hdr[0] = scan[p] < 0 ? 0 : (scan[p] > E ? E : scan[p]);
  if ((unsigned)e >= (unsigned)E || (unsigned)s >= (unsigned)E) return;
  slot_edge[s] = e;
  if (flag[p]) ekey[e] = key2[p];
}

// ---- lengths and the selection -----------------------------------------------------------------

__global__ void __launch_bounds__(256) k_sd_len(int E, int nv, const int* __restrict__ hdr, const u64* __restrict__ ekey,
                                                const float* __restrict__ verts, double* __restrict__ len2,
                                                u64* __restrict__ max_bits) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  double l = 0.0;
  if (e < hdr[0]) {
    const u64 k = ekey[e];
    const int a = clamp_index((int)(k >> M_IDX_BITS), nv), b = clamp_index((int)(k & M_IDX_MASK), nv);
    l = sd_len2(verts + 3 * (size_t)a, verts + 3 * (size_t)b);
  }
  if (e < E) len2[e] = l;
  // len2 >= 0, so the bit patterns order like the values and the maximum is exact in any order
  u64 m = l > 0.0 ? (u64)__double_as_longlong(l) : 0ull;
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const u64 t = __shfl_xor(m, o);
    m = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(max_bits, m);
}

__device__ __forceinline__ bool sd_qualifies(double l, double abs2, double rel2, double max_len2) {
  const double r = rel2 * max_len2;
  return l > abs2 && l > r;
}

// no budget can bind: every qualifying edge splits
__global__ void __launch_bounds__(256) k_sd_split_all(int E, const int* __restrict__ hdr, const double* __restrict__ len2,
                                                      const double* __restrict__ max_len2, double abs2, double rel2,
                                                      int* __restrict__ split) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  split[e] = (e < hdr[0] && sd_qualifies(len2[e], abs2, rel2, *max_len2)) ? 1 : 0;
}

// selection keys: inverted length bits for a qualifying edge (len2 > 0, so never all ones), all ones otherwise
__global__ void __launch_bounds__(256) k_sd_sel_keys(int E, const int* __restrict__ hdr, const double* __restrict__ len2,
                                                     const double* __restrict__ max_len2, double abs2, double rel2,
                                                     u64* __restrict__ key) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const double l = len2[e];
  key[e] = (e < hdr[0] && sd_qualifies(l, abs2, rel2, *max_len2)) ? ~(u64)__double_as_longlong(l) : ~0ull;
}

__global__ void __launch_bounds__(256) k_sd_take(int E, int max_split, const u64* __restrict__ key2,
                                                 const int* __restrict__ val2, int* __restrict__ split) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= E) return;
  const int e = val2[r];
  if ((unsigned)e >= (unsigned)E) return;
  split[e] = (r < max_split && key2[r] != ~0ull) ? 1 : 0;
}

// ---- sizes, vertices and faces -----------------------------------------------------------------

__global__ void __launch_bounds__(256) k_sd_fcnt(int nf, int E, const int* __restrict__ slot_edge,
                                                 const int* __restrict__ split, int* __restrict__ fcnt) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  int n = 1;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int e = slot_edge[3 * (size_t)f + j];
    n += ((unsigned)e < (unsigned)E && split[e]) ? 1 : 0;
  }
  fcnt[f] = n;
}

__global__ void k_sd_counts(int nv, int nf, int E, int cap_v, int cap_f, const int* __restrict__ scan,
                            const int* __restrict__ fcnt, const int* __restrict__ foff, int* __restrict__ hdr,
                            long long* __restrict__ counts) {
  if (blockIdx.x || threadIdx.x) return;
  const long long ns = scan[E - 1], nfo = (long long)foff[nf - 1] + fcnt[nf - 1];
  counts[0] = hdr[0];
  counts[1] = ns;
  counts[2] = nv + ns;
  counts[3] = nfo;
  hdr[1] = (ns >= 0 && ns <= E && nv + ns <= cap_v && nfo >= nf && nfo <= cap_f) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_sd_verts(int n, int nv, int E, int cap_v, const int* __restrict__ hdr,
                                                  const float* __restrict__ verts, const u64* __restrict__ ekey,
                                                  const int* __restrict__ split, const int* __restrict__ scan,
                                                  float* __restrict__ out_verts, int* __restrict__ parents) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !hdr[1]) return;
  if (i < nv) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out_verts[3 * (size_t)i + a] = verts[3 * (size_t)i + a];
    parents[2 * (size_t)i] = i;
    parents[2 * (size_t)i + 1] = i;
  }
  if (i < E && i < hdr[0] && split[i]) {
    const long long id = (long long)nv + scan[i] - 1;
    if (id < nv || id >= cap_v) return;
    const u64 k = ekey[i];
    const int lo = clamp_index((int)(k >> M_IDX_BITS), nv), hi = clamp_index((int)(k & M_IDX_MASK), nv);
#pragma unroll
    for (int a = 0; a < 3; ++a)  // the sum of two f32 and its half are exact in f64: one rounding, to f32
      out_verts[3 * (size_t)id + a] = (float)(((double)verts[3 * (size_t)lo + a] + (double)verts[3 * (size_t)hi + a]) * 0.5);
    parents[2 * (size_t)id] = lo;
    parents[2 * (size_t)id + 1] = hi;
  }
}

__device__ __forceinline__ void sd_put(int* __restrict__ out_faces, long long o, int a, int b, int c) {
  out_faces[3 * o] = a;
  out_faces[3 * o + 1] = b;
  out_faces[3 * o + 2] = c;
}

// Children of a face, orientation kept; mij is the midpoint of (vi, vj):
//   0 split  (v0, v1, v2)
//   3 split  (v0, m01, m20), (m01, v1, m12), (m20, m12, v2), (m01, m12, m20)
//   1 split  rotated so that the split edge is (v0, v1): (v0, m01, v2), (m01, v1, v2)
//   2 split  rotated so that the unsplit edge is (v2, v0): (m01, v1, m12), then the quad (v0, m01, m12, v2)
//            cut by (m01, v2) if that is strictly shorter than (v0, m12) in the f32 output positions
__global__ void __launch_bounds__(256) k_sd_emit(int nf, int nv, int E, int cap_v, int cap_f,
                                                 const int* __restrict__ hdr, const int* __restrict__ faces,
                                                 const int* __restrict__ slot_edge, const int* __restrict__ split,
                                                 const int* __restrict__ scan, const int* __restrict__ foff,
                                                 const float* __restrict__ out_verts, int* __restrict__ out_faces) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf || !hdr[1]) return;
  int v[3], m[3], ns = 0, first = -1, unsplit = -1;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    v[j] = clamp_index(faces[3 * (size_t)f + j], nv);
    const int e = slot_edge[3 * (size_t)f + j];
    const bool s = (unsigned)e < (unsigned)E && split[e];
    const long long id = s ? (long long)nv + scan[e] - 1 : -1;
    m[j] = (s && id >= nv && id < cap_v) ? (int)id : -1;
    if (m[j] >= 0) {
      ++ns;
      if (first < 0) first = j;
    } else {
      unsplit = j;
    }
  }
  const long long o = foff[f];
  if (o < 0 || o + ns >= cap_f) return;
  if (ns == 0) {
    sd_put(out_faces, o, v[0], v[1], v[2]);
  } else if (ns == 3) {
    sd_put(out_faces, o, v[0], m[0], m[2]);
    sd_put(out_faces, o + 1, m[0], v[1], m[1]);
    sd_put(out_faces, o + 2, m[2], m[1], v[2]);
    sd_put(out_faces, o + 3, m[0], m[1], m[2]);
  } else if (ns == 1) {
    const int r = first, a = v[r], b = v[(r + 1) % 3], c = v[(r + 2) % 3], mab = m[r];
    sd_put(out_faces, o, a, mab, c);
    sd_put(out_faces, o + 1, mab, b, c);
  } else {
    const int r = (unsplit + 1) % 3;
    const int a = v[r], b = v[(r + 1) % 3], c = v[(r + 2) % 3], mab = m[r], mbc = m[(r + 1) % 3];
    sd_put(out_faces, o, mab, b, mbc);
    const double d0 = sd_len2(out_verts + 3 * (size_t)mab, out_verts + 3 * (size_t)c);
    const double d1 = sd_len2(out_verts + 3 * (size_t)a, out_verts + 3 * (size_t)mbc);
    if (d0 < d1) {
      sd_put(out_faces, o + 1, a, mab, c);
      sd_put(out_faces, o + 2, mab, mbc, c);
    } else {
      sd_put(out_faces, o + 1, a, mab, mbc);
      sd_put(out_faces, o + 2, a, mbc, c);
    }
  }
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_mesh_subdivide_ws_bytes(int nv, int nf) {
  if (!sd_sizes_ok(nv, nf)) return -1;
  size_t total = 0;
  sd_carve(nullptr, nf, &total);
  return (long long)total;
}

extern "C" int zp_mesh_subdivide(const float* verts, int nv, const int* faces, int nf, double abs2, double rel2,
                                 int max_split, float* out_verts, int cap_v, int* out_faces, int cap_f, int* parents,
                                 long long* counts, double* max_len2, void* ws, void* stream) {
  ZP_CHECK_ARG(sd_sizes_ok(nv, nf), "zp_mesh_subdivide: sizes nv %d nf %d out of range (1 <= nv <= 2^21, 1 <= nf <= 2^24)",
               nv, nf);
  ZP_CHECK_ARG(abs2 >= 0.0, "zp_mesh_subdivide: abs2 %g must be >= 0", abs2);
  ZP_CHECK_ARG(rel2 >= 0.0 && rel2 < 1.0, "zp_mesh_subdivide: rel2 %g outside [0, 1)", rel2);
  ZP_CHECK_ARG(max_split >= 0, "zp_mesh_subdivide: max_split %d must be >= 0", max_split);
  ZP_CHECK_ARG(cap_v >= 0 && cap_f >= 0, "zp_mesh_subdivide: cap_v %d / cap_f %d must be >= 0", cap_v, cap_f);
  ZP_CHECK_ARG(verts && faces && out_verts && out_faces && parents && counts && max_len2 && ws,
               "zp_mesh_subdivide: NULL pointer (verts, faces, out_verts, out_faces, parents, counts, max_len2, ws "
               "are required)");
  hipStream_t st = (hipStream_t)stream;
  const SWs w = sd_carve(ws, nf, nullptr);
  const int E = 3 * nf, eblocks = ceil_div(E, 256), fblocks = ceil_div(nf, 256);

  hipLaunchKernelGGL(k_sd_keys, dim3(eblocks), dim3(256), 0, st, E, nv, faces, w.key, w.iota, max_len2);
  ZP_LAUNCH_CHECK("zp_mesh_subdivide keys");
  int rc = sort_pairs(w.key, w.key2, w.iota, w.val2, E, 2 * M_IDX_BITS, w.temp, w.temp_bytes, st,
                      "zp_mesh_subdivide (edges)");
  if (rc != ZP_OK) return rc;
  hipLaunchKernelGGL(k_sd_flag, dim3(eblocks), dim3(256), 0, st, E, (const u64*)w.key2, w.flag);
  ZP_LAUNCH_CHECK("zp_mesh_subdivide flags");
  rc = inclusive_scan(w.flag, w.scan, E, w.temp, w.temp_bytes, st, "zp_mesh_subdivide (edges)");
  if (rc != ZP_OK) return rc;
  hipLaunchKernelGGL(k_sd_rank, dim3(eblocks), dim3(256), 0, st, E, (const u64*)w.key2, (const int*)w.val2,
                     (const int*)w.flag, (const int*)w.scan, w.slot_edge, w.ekey, w.hdr);
  ZP_LAUNCH_CHECK("zp_mesh_subdivide ranks");

  hipLaunchKernelGGL(k_sd_len, dim3(eblocks), dim3(256), 0, st, E, nv, (const int*)w.hdr, (const u64*)w.ekey, verts,
                     w.len2, (u64*)max_len2);
  ZP_LAUNCH_CHECK("zp_mesh_subdivide lengths");
  int* split = w.flag;  // the unique-edge flags are spent
  if (max_split >= E) {
    hipLaunchKernelGGL(k_sd_split_all, dim3(eblocks), dim3(256), 0, st, E, (const int*)w.hdr, (const double*)w.len2,
                       (const double*)max_len2, abs2, rel2, split);
    ZP_LAUNCH_CHECK("zp_mesh_subdivide selection");
  } else {
    hipLaunchKernelGGL(k_sd_sel_keys, dim3(eblocks), dim3(256), 0, st, E, (const int*)w.hdr, (const double*)w.len2,
                       (const double*)max_len2, abs2, rel2, w.key);
    ZP_LAUNCH_CHECK("zp_mesh_subdivide selection keys");
    rc = sort_pairs(w.key, w.key2, w.iota, w.val2, E, 64, w.temp, w.temp_bytes, st, "zp_mesh_subdivide (lengths)");
    if (rc != ZP_OK) return rc;
    hipLaunchKernelGGL(k_sd_take, dim3(eblocks), dim3(256), 0, st, E, max_split, (const u64*)w.key2, (const int*)w.val2,
                       split);
    ZP_LAUNCH_CHECK("zp_mesh_subdivide selection");
  }
  rc = inclusive_scan(split, w.scan, E, w.temp, w.temp_bytes, st, "zp_mesh_subdivide (new vertices)");
  if (rc != ZP_OK) return rc;

  hipLaunchKernelGGL(k_sd_fcnt, dim3(fblocks), dim3(256), 0, st, nf, E, (const int*)w.slot_edge, (const int*)split,
                     w.fcnt);
  ZP_LAUNCH_CHECK("zp_mesh_subdivide face counts");
  rc = exclusive_scan(w.fcnt, w.foff, nf, w.temp, w.temp_bytes, st, "zp_mesh_subdivide (child faces)");
  if (rc != ZP_OK) return rc;
  hipLaunchKernelGGL(k_sd_counts, dim3(1), dim3(64), 0, st, nv, nf, E, cap_v, cap_f, (const int*)w.scan,
                     (const int*)w.fcnt, (const int*)w.foff, w.hdr, counts);
  ZP_LAUNCH_CHECK("zp_mesh_subdivide counts");
  const int n = nv > E ? nv : E;
  hipLaunchKernelGGL(k_sd_verts, dim3(ceil_div(n, 256)), dim3(256), 0, st, n, nv, E, cap_v, (const int*)w.hdr, verts,
                     (const u64*)w.ekey, (const int*)split, (const int*)w.scan, out_verts, parents);
  ZP_LAUNCH_CHECK("zp_mesh_subdivide vertices");
  hipLaunchKernelGGL(k_sd_emit, dim3(fblocks), dim3(256), 0, st, nf, nv, E, cap_v, cap_f, (const int*)w.hdr, faces,
                     (const int*)w.slot_edge, (const int*)split, (const int*)w.scan, (const int*)w.foff,
                     (const float*)out_verts, out_faces);
  ZP_LAUNCH_CHECK("zp_mesh_subdivide faces");
  return ZP_OK;
}
