// d-ary mesh coder (zp_mesh_code_radix; tests/meshcode_radix_ref.py is the executable definition): the
// mesh coder of zp_meshcode.hip with a d-way split per level, d = 4 .. 256, for the d-ary codes.  The
// grid, the group layout, the regrouping, the faces and the LUT are the binary coder's and run through
// its driver steps (zp_mesh.h); what differs is the split: farthest-point seeds c_1 .. c_(d-1), d-way
// Lloyd steps, and in place of the 2-way balance a peel, class by class, that leaves every class
// floor(n / d) or ceil(n / d) vertices (the reference's own balancing touches classes 0 and 1 only).
//
// A level's d^l groups lie contiguous; the d centres of group g are slots g * d .. g * d + d - 1 of the
// centre, sum and seed-key arrays.  A block covers RX_POS consecutive positions.  Every group holds at
// least d vertices (include/zp.h), so those positions span at most RX_POS / d + 1 groups, that is
// RX_POS + d slots: the block stages every centre it can meet in LDS and sums per slot there (64-bit
// integer LDS atomics), then merges the slots it touched into the global sums with integer atomics.  No
// thread holds more than one running minimum, whatever d is.  All arithmetic is integer.
#include "zp_mesh.h"

namespace zp {

constexpr int RX_ITEMS = 4;                // positions per thread
constexpr int RX_POS = 256 * RX_ITEMS;     // positions per block
constexpr int RX_SLOTS = RX_POS + 256;     // (group, class) slots a block can meet, d <= 256
constexpr int RX_GROUPS = RX_POS / 4 + 1;  // groups a block can meet, d >= 4
constexpr int RX_SCORE_BITS = 43;          // |D_j - min D_i| < 2^42, biased by 2^42

struct RadixWs {  // beside MeshWs; C = d^levels slots
  int4* rcen;     // [C] centres of the running attempt, slot g * d + j (w unused)
  int4* rbcen;    // [C] of the best attempt
  u64* sums;      // [C][4] S xyz and the count of every slot
  u64* far;       // [C] farthest-point key of seed j in slot g * d + j
  int* digit;     // [nv] class of sorted position p once a peel has taken it, else -1
  int* urem;      // [2][C / d] |U_j| of every group, double-buffered over the peels
};

static bool radix_sizes_ok(int nv, int nf, int divide, int levels) {
  if (divide < 4 || divide > 256 || (divide & (divide - 1)) || levels < 1 || levels > 16) return false;
  const int s = __builtin_ctz((unsigned)divide);
  return s * levels <= 16 && nv >= (1 << (s * levels)) && mesh_range_ok(nv, nf);
}

// C = d^levels
static size_t rx_carve(void* ws, int nv, int nf, int C, int d, MeshWs& w, RadixWs& r) {
  Carver c(ws);
  const size_t G = (size_t)C / d;
  r.rcen = c.take<int4>(C);
  r.rbcen = c.take<int4>(C);
  r.sums = c.take<u64>((size_t)C * 4);
  r.far = c.take<u64>(C);
  r.digit = c.take<int>(nv);
  r.urem = c.take<int>(2 * G);
  w = carve_mesh(c, nv, nf, G);
  return c.total();
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
    shc[t] = j == 1 ? seed0(g, nv, gstart, order, q, draws) : far_point(far[(size_t)g * d + j - 1], nv, q);
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
  cen[t] = j == 0 ? seed0(g, nv, gstart, order, q, draws) : far_point(far[t], nv, q);
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

extern "C" long long zp_mesh_code_radix_ws_bytes(int nv, int nf, int divide, int levels) {
  if (!radix_sizes_ok(nv, nf, divide, levels)) return -1;
  MeshWs w;
  RadixWs r;
  return (long long)rx_carve(nullptr, nv, nf, 1 << (__builtin_ctz((unsigned)divide) * levels), divide, w, r);
}

extern "C" int zp_mesh_code_radix(const float* verts, int nv, const int* faces, int nf, int divide, int levels,
                                  int attempts, int iterations, int grid_log2, long long eps2_q, const uint32_t* draws,
                                  int* vertex_ids, int* face_ids, double* lut, void* ws, void* stream) {
  const char* who = "zp_mesh_code_radix";
  ZP_CHECK_ARG(divide != 2, "zp_mesh_code_radix: divide 2 is the binary split: call zp_mesh_code");
  ZP_CHECK_ARG(divide >= 4 && divide <= 256 && !(divide & (divide - 1)),
               "zp_mesh_code_radix: divide %d is no power of two in 4..256", divide);
  const int d = divide, s = __builtin_ctz((unsigned)d);
  ZP_CHECK_ARG(levels >= 1 && s * (long long)levels <= 16,
               "zp_mesh_code_radix: levels %d: divide^levels must lie in divide..65536", levels);
  const int C = 1 << (s * levels);
  ZP_CHECK_ARG(nv >= C, "zp_mesh_code_radix: nv %d below divide^levels = %d", nv, C);
  int rc = mesh_check_args(who, nv, nf, attempts, iterations, grid_log2, eps2_q,
                           verts && faces && draws && vertex_ids && face_ids && lut && ws);
  if (rc != ZP_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MeshWs w;
  RadixWs r;
  rx_carve(ws, nv, nf, C, d, w, r);
  const int Gmax = C / d, vblocks = ceil_div(nv, 256), rblocks = ceil_div(nv, RX_POS);
  const size_t draws_per_attempt = ((size_t)C - 1) / (size_t)(d - 1);

  if ((rc = mesh_prologue(who, w, verts, nv, nf, grid_log2, vertex_ids, st)) != ZP_OK) return rc;

  for (int l = 0; l < levels; ++l) {
    const int G = 1 << (s * l), S = G * d, sblocks = ceil_div(S, 256);  // S slots: (group, class)
    const size_t first = ((size_t)G - 1) / (size_t)(d - 1);
    for (int a = 0; a < attempts; ++a) {
      const uint32_t* dr = draws + a * draws_per_attempt + first;
      const hipError_t e = hipMemsetAsync(r.far, 0, (size_t)S * 8, st);
      if (e != hipSuccess) {
        set_error("zp_mesh_code_radix: clearing the seed keys failed: %s", hipGetErrorString(e));
        return ZP_ERR_HIP;
      }
      for (int j = 1; j < d; ++j)  // w.key is the running minimum here: the peel starts after the seeding
        hipLaunchKernelGGL(k_rx_seed, dim3(rblocks), dim3(256), 0, st, nv, G, d, j, (const unsigned*)w.gs,
                           (const int*)w.order, (const int4*)w.q, (const int*)w.gstart, dr, w.key, r.far);
      hipLaunchKernelGGL(k_rx_seeded, dim3(sblocks), dim3(256), 0, st, S, d, nv, (const int*)w.gstart,
                         (const int*)w.order, (const int4*)w.q, dr, (const u64*)r.far, r.rcen, r.sums, w.comp, w.done);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix seeds");
      for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_rx_accum, dim3(rblocks), dim3(256), 0, st, nv, G, d, (const unsigned*)w.gs,
                           (const int*)w.order, (const int4*)w.q, (const int4*)r.rcen, (const int*)w.done, r.sums);
        hipLaunchKernelGGL(k_rx_update, dim3(sblocks), dim3(256), 0, st, S, d, eps2_q, r.rcen, r.sums, w.done);
      }
      ZP_LAUNCH_CHECK("zp_mesh_code_radix lloyd");
      hipLaunchKernelGGL(k_rx_comp, dim3(rblocks), dim3(256), 0, st, nv, G, d, (const unsigned*)w.gs,
                         (const int*)w.order, (const int4*)w.q, (const int4*)r.rcen, w.comp);
      hipLaunchKernelGGL(k_rx_best, dim3(sblocks), dim3(256), 0, st, S, d, a, (const int4*)r.rcen, (const u64*)w.comp,
                         r.rbcen, w.bcomp);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix compactness");
    }
    for (int j = 0; j < d - 1; ++j) {
      hipLaunchKernelGGL(k_rx_score, dim3(rblocks), dim3(256), 0, st, nv, G, d, j, (const unsigned*)w.gs,
                         (const int*)w.order, (const int4*)w.q, (const int4*)r.rbcen, r.digit, w.key);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix scores");
      rc = sort_pairs(w.key, w.key2, w.iota, w.val2, nv, RX_SCORE_BITS + 1 + s * l, w.temp, w.temp_bytes, st, who);
      if (rc != ZP_OK) return rc;
      hipLaunchKernelGGL(k_rx_take, dim3(vblocks), dim3(256), 0, st, nv, G, d, j, s * (levels - 1 - l),
                         (const u64*)w.key2, (const int*)w.val2, (const int*)w.gstart, (const int*)w.order,
                         (const int*)(r.urem + (size_t)(j & 1) * Gmax), r.urem + (size_t)((j + 1) & 1) * Gmax, r.digit,
                         w.gid, vertex_ids);
      ZP_LAUNCH_CHECK("zp_mesh_code_radix peel");
    }
    if (l + 1 < levels && (rc = mesh_regroup(who, w, nv, s * (l + 1), S, st)) != ZP_OK) return rc;
  }
  return mesh_epilogue(who, w, verts, nv, faces, nf, s * levels, vertex_ids, face_ids, lut, st);
}
