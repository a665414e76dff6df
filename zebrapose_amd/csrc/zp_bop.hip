// BOP pose errors on the device: MSSD / MSPD (zp_pose_error_sym) and the pixel stage of VSD (zp_vsd).
// Reference: lib/pysixd/pose_error.py:22-179 (vsd, mssd, mspd), lib/pysixd/visibility.py ('bop19'),
// lib/pysixd/misc.py:511-525 (project_pts) and :571-590 (depth_im_to_dist_im_fast).  The contracts are
// in include/zp.h; tests/bop_ref.py restates them in numpy.
//
// MSSD / MSPD: out[b] = min_s max_i d(est p_i, gt_s p_i).  One block stages tiles of 512 points in LDS
// (the raw point and its image under the estimated pose) and covers SG symmetries, SG a power of two:
// thread (s, slice) keeps the composed pose gt o sym_s in registers and a running maximum of the
// squared distance over every (256 / SG)-th point of the tile, so no cross-lane work is done per
// symmetry.  SG is chosen per call (sym_plan): 1 .. 8 for a handful of symmetries, where the 256
// threads are slices of the point tile, 64 .. 256 for hundreds, where a wave reads one LDS address.
// Partial maxima go to ws[b][s][part]; k_sym_final takes the max over parts, the min over s and one
// square root.  max and min are exact, so the result does not depend on the partition or the order.
//
// VSD: one pass over the pixels, four per thread and step, skipping a pixel where neither render has
// a surface (it can be in neither mask); integer counters per thread -> wave shuffles -> LDS ->
// partials [b][chunk][2 + NT] summed by k_vsd_final.  Integers only: exact in any order.
// This file is built with -ffp-contract=off: the distance image is specified operation by operation.
#include <math.h>
#include "zp_common.h"

namespace zp {

constexpr int SYM_TP = 512;        // points per LDS tile
constexpr int SYM_MAX_BLOCKS = 2048;

struct SymPlan {
  int SG, nsg, parts;
};
// SG minimises ceil(S / SG) * (SG + 1): thread slots per point, plus the staging transform each block
// of a symmetry group repeats (S = 3 -> 4, 70 -> 8, 314 -> 64, 628 -> 128)
static SymPlan sym_plan(int B, int n, int S) {
  SymPlan p;
  long best = -1;
  p.SG = 1;
  for (int g = 1; g <= 256; g <<= 1) {
    const long c = (long)((S + g - 1) / g) * (g + 1);
    if (best < 0 || c < best) {
      best = c;
      p.SG = g;
    }
  }
  p.nsg = (S + p.SG - 1) / p.SG;
  const long tiles = ((long)n + SYM_TP - 1) / SYM_TP;
  const long room = SYM_MAX_BLOCKS / ((long)p.nsg * B);
  p.parts = (int)(tiles < room ? tiles : (room < 1 ? 1 : room));
  return p;
}

template <int MODE>
__global__ void __launch_bounds__(256) k_sym(const float* __restrict__ pts, int n, const double* __restrict__ Re,
                                             const double* __restrict__ te, const double* __restrict__ Rg,
                                             const double* __restrict__ tg, const double* __restrict__ K,
                                             const double* __restrict__ symR, const double* __restrict__ symt, int S,
                                             int sg_log2, int nsg, int parts, double* __restrict__ ws) {
  __shared__ float rp[3][SYM_TP];
  __shared__ double ep[3][SYM_TP];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int part = blockIdx.x % parts;
  const int sg = (blockIdx.x / parts) % nsg;
  const int b = blockIdx.x / (parts * nsg);
  const int SG = 1 << sg_log2;
  const int sl = tid & (SG - 1), slice = tid >> sg_log2, nsl = 256 >> sg_log2;
  const int s = sg * SG + sl;
  const bool live = s < S;

  double fx = 1, fy = 1, cx = 0, cy = 0;
  if (MODE == ZP_METRIC_MSPD) {
    fx = K[4 * b], fy = K[4 * b + 1], cx = K[4 * b + 2], cy = K[4 * b + 3];
  }
  // est pose (staging) and the composed pose R_s = R_gt sym_R[s], t_s = R_gt sym_t[s] + t_gt
  double E[9], et[3], R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = Re[9 * (size_t)b + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) et[k] = te[3 * (size_t)b + k];
  {
    const double* G = Rg + 9 * (size_t)b;
    const double* A = symR + 9 * (size_t)(live ? s : 0);
    const double* a = symt + 3 * (size_t)(live ? s : 0);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = G[3 * r] * A[c] + G[3 * r + 1] * A[3 + c] + G[3 * r + 2] * A[6 + c];
      t[r] = (G[3 * r] * a[0] + G[3 * r + 1] * a[1] + G[3 * r + 2] * a[2]) + tg[3 * (size_t)b + r];
    }
  }

  double best = 0.0;  // squared distances are >= 0; a NaN one is dropped by fmax
  for (long long i0 = (long long)part * SYM_TP; i0 < n; i0 += (long long)parts * SYM_TP) {
    __syncthreads();
    for (int j = tid; j < SYM_TP; j += 256) {
      const long long i = i0 + j;
      if (i < n) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        rp[0][j] = x, rp[1][j] = y, rp[2][j] = z;
        const double X = __builtin_fma(E[0], x, __builtin_fma(E[1], y, __builtin_fma(E[2], z, et[0])));
        const double Y = __builtin_fma(E[3], x, __builtin_fma(E[4], y, __builtin_fma(E[5], z, et[1])));
        const double Z = __builtin_fma(E[6], x, __builtin_fma(E[7], y, __builtin_fma(E[8], z, et[2])));
        if (MODE == ZP_METRIC_MSPD) {
          const double iz = 1.0 / Z;
          ep[0][j] = __builtin_fma(fx * X, iz, cx);
          ep[1][j] = __builtin_fma(fy * Y, iz, cy);
        } else {
          ep[0][j] = X, ep[1][j] = Y, ep[2][j] = Z;
        }
      }
    }
    __syncthreads();
    const int m = (int)(n - i0 < SYM_TP ? n - i0 : SYM_TP);
    if (live) {
#pragma unroll 4
      for (int j = slice; j < m; j += nsl) {
        const double x = rp[0][j], y = rp[1][j], z = rp[2][j];
        const double X = __builtin_fma(R[0], x, __builtin_fma(R[1], y, __builtin_fma(R[2], z, t[0])));
        const double Y = __builtin_fma(R[3], x, __builtin_fma(R[4], y, __builtin_fma(R[5], z, t[1])));
        const double Z = __builtin_fma(R[6], x, __builtin_fma(R[7], y, __builtin_fma(R[8], z, t[2])));
        double d2;
        if (MODE == ZP_METRIC_MSPD) {
          const double iz = 1.0 / Z;
          const double du = ep[0][j] - __builtin_fma(fx * X, iz, cx), dv = ep[1][j] - __builtin_fma(fy * Y, iz, cy);
          d2 = __builtin_fma(du, du, dv * dv);
        } else {
          const double dx = ep[0][j] - X, dy = ep[1][j] - Y, dz = ep[2][j] - Z;
          d2 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
        }
        best = fmax(best, d2);
      }
    }
  }
  red[tid] = best;
  __syncthreads();
  if (tid < SG && live) {
    for (int k = 1; k < nsl; ++k) best = fmax(best, red[tid + k * SG]);
    ws[((size_t)b * S + s) * parts + part] = best;
  }
}

__global__ void __launch_bounds__(256) k_sym_final(const double* __restrict__ ws, int S, int parts,
                                                   double* __restrict__ out) {
  __shared__ double red[256];
  const int b = blockIdx.x;
  double mn = INFINITY;
  for (int s = threadIdx.x; s < S; s += 256) {
    const double* w = ws + ((size_t)b * S + s) * parts;
    double e = w[0];
    for (int k = 1; k < parts; ++k) e = fmax(e, w[k]);
    mn = fmin(mn, e);
  }
  red[threadIdx.x] = mn;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + k]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[b] = sqrt(red[0]);
}

// ---- VSD -------------------------------------------------------------------------------------------

constexpr int VSD_MAX_TAU = 32;
constexpr int VSD_NC = 2 + VSD_MAX_TAU;  // counters per partial: union, inter, cost_0 ..
constexpr int VSD_MAX_CHUNKS = 256;

struct VsdTaus {
  double v[VSD_MAX_TAU];  // entries past ntau are +inf: no distance reaches them
};

static int vsd_chunks(int B, long HW) {
  const long groups = (HW + 3) / 4;
  long cap = SYM_MAX_BLOCKS / B;
  cap = cap < 1 ? 1 : (cap > VSD_MAX_CHUNKS ? VSD_MAX_CHUNKS : cap);
  const long want = (groups + 255) / 256;
  return (int)(want < cap ? want : cap);
}

// misc.py:586-588, one IEEE operation each
__device__ __forceinline__ double dist_of(float d, double pX, double pY) {
  const double z = (double)d;
  const double a = pX * z, c = pY * z;
  return sqrt((a * a + c * c) + z * z);
}

template <int NT, bool VEC>
__global__ void __launch_bounds__(256) k_vsd(const float* __restrict__ est, const float* __restrict__ gt,
                                             const float* __restrict__ test, int n_test,
                                             const int* __restrict__ test_index, int H, int W,
                                             const double* __restrict__ K, float delta, VsdTaus taus,
                                             const double* __restrict__ diameter, int* __restrict__ part) {
  __shared__ int wred[4][2 + NT];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long HW = (long)H * W;
  int ti = test_index ? test_index[b] : b;
  ti = ti < 0 ? 0 : (ti >= n_test ? n_test - 1 : ti);
  const float* e = est + (size_t)b * HW;
  const float* g = gt + (size_t)b * HW;
  const float* t = test + (size_t)ti * HW;
  const double fx = K[4 * b], fy = K[4 * b + 1], cx = K[4 * b + 2], cy = K[4 * b + 3];
  const bool norm = diameter != nullptr;
  const double diam = norm ? diameter[b] : 1.0;

  int uni = 0, inter = 0, cnt[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) cnt[k] = 0;

  const long groups = (HW + 3) / 4;
  for (long q = (long)blockIdx.x * 256 + tid; q < groups; q += (long)gridDim.x * 256) {
    const long i = 4 * q;
    float ev[4], gv[4], tv[4];
    if (VEC) {
      const float4 a = *reinterpret_cast<const float4*>(e + i), c = *reinterpret_cast<const float4*>(g + i);
      ev[0] = a.x, ev[1] = a.y, ev[2] = a.z, ev[3] = a.w;
      gv[0] = c.x, gv[1] = c.y, gv[2] = c.z, gv[3] = c.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ev[u] = i + u < HW ? e[i + u] : 0.f;
        gv[u] = i + u < HW ? g[i + u] : 0.f;
      }
    }
    // a pixel where both renders are empty has dist_model == 0 twice: it is in neither mask
    bool any = false;
#pragma unroll
    for (int u = 0; u < 4; ++u) any |= !(ev[u] == 0.f && gv[u] == 0.f);
    if (!any) continue;
    if (VEC) {
      const float4 a = *reinterpret_cast<const float4*>(t + i);
      tv[0] = a.x, tv[1] = a.y, tv[2] = a.z, tv[3] = a.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) tv[u] = i + u < HW ? t[i + u] : 0.f;
    }
    int y = (int)(i / W), x = (int)(i - (long)y * W);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!(ev[u] == 0.f && gv[u] == 0.f)) {
        const double pX = ((double)x - cx) / fx, pY = ((double)y - cy) / fy;
        const double dt = dist_of(tv[u], pX, pY), dg = dist_of(gv[u], pX, pY), de = dist_of(ev[u], pX, pY);
        const float ft = (float)dt;
        const bool hole = dt == 0.0;
        const bool vg = (((float)dg - ft) <= delta || hole) && dg > 0.0;
        const bool ve = ((((float)de - ft) <= delta || hole) && de > 0.0) || (vg && de > 0.0);
        uni += vg || ve;
        if (vg && ve) {
          ++inter;
          double d = fabs(dg - de);
          if (norm) d = d / diam;
#pragma unroll
          for (int k = 0; k < NT; ++k) cnt[k] += d >= taus.v[k];
        }
      }
      if (++x == W) x = 0, ++y;
    }
  }

  // wave -> block -> partial
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uni += __shfl_down(uni, off);
    inter += __shfl_down(inter, off);
#pragma unroll
    for (int k = 0; k < NT; ++k) cnt[k] += __shfl_down(cnt[k], off);
  }
  if (lane == 0) {
    wred[wave][0] = uni;
    wred[wave][1] = inter;
#pragma unroll
    for (int k = 0; k < NT; ++k) wred[wave][2 + k] = cnt[k];
  }
  __syncthreads();
  if (tid < 2 + NT)
    part[((size_t)b * gridDim.x + blockIdx.x) * VSD_NC + tid] = (wred[0][tid] + wred[1][tid]) + (wred[2][tid] + wred[3][tid]);
}

// out[b][k] = (cost_k + (union - inter)) / union (pose_error.py:125), 1.0 when union == 0 (:110-111)
__global__ void __launch_bounds__(64) k_vsd_final(const int* __restrict__ part, int chunks, int ntau,
                                                  double* __restrict__ out, int* __restrict__ counts) {
  __shared__ int tot[VSD_NC];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 2 + ntau) {
    int s = 0;
    for (int c = 0; c < chunks; ++c) s += part[((size_t)b * chunks + c) * VSD_NC + tid];
    tot[tid] = s;
    if (counts) counts[(size_t)b * (2 + ntau) + tid] = s;
  }
  __syncthreads();
  if (tid < ntau) {
    const int uni = tot[0], inter = tot[1];
    out[(size_t)b * ntau + tid] = uni == 0 ? 1.0 : (double)(tot[2 + tid] + (uni - inter)) / (double)uni;
  }
}

static bool sym_sizes_ok(int B, int n, int S) {
  if (B <= 0 || n <= 0 || S < 1 || S > 4096) return false;
  const SymPlan p = sym_plan(B, n, S);
  return (long long)B * p.nsg * p.parts < 2147483647LL;
}

static bool vsd_sizes_ok(int B, int H, int W, int ntau) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)H * W < 2147483647LL - 1024 && ntau >= 1 &&
         ntau <= VSD_MAX_TAU;
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_pose_error_sym_ws_bytes(int B, int n, int S, int mode) {
  if (!sym_sizes_ok(B, n, S) || (mode != ZP_METRIC_MSSD && mode != ZP_METRIC_MSPD)) return -1;
  return (long long)B * S * sym_plan(B, n, S).parts * 8;
}

extern "C" int zp_pose_error_sym(int B, const float* pts, int n, const double* R_est, const double* t_est,
                                 const double* R_gt, const double* t_gt, const double* K, const double* sym_R,
                                 const double* sym_t, int S, int mode, double* out, void* ws, void* stream) {
  ZP_CHECK_ARG(mode == ZP_METRIC_MSSD || mode == ZP_METRIC_MSPD, "zp_pose_error_sym: mode %d", mode);
  ZP_CHECK_ARG(S >= 1 && S <= 4096, "zp_pose_error_sym: S %d outside [1, 4096]", S);
  ZP_CHECK_ARG(sym_sizes_ok(B, n, S), "zp_pose_error_sym: sizes out of range: B %d, n %d", B, n);
  ZP_CHECK_ARG(pts && R_est && t_est && R_gt && t_gt && sym_R && sym_t && out && ws, "zp_pose_error_sym: NULL pointer");
  ZP_CHECK_ARG(mode != ZP_METRIC_MSPD || K, "zp_pose_error_sym: NULL K with ZP_METRIC_MSPD");
  hipStream_t st = (hipStream_t)stream;
  const SymPlan p = sym_plan(B, n, S);
  int lg = 0;
  while ((1 << lg) < p.SG) ++lg;
  const dim3 grid((unsigned)((long long)B * p.nsg * p.parts));
  if (mode == ZP_METRIC_MSPD)
    hipLaunchKernelGGL(k_sym<ZP_METRIC_MSPD>, grid, dim3(256), 0, st, pts, n, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t,
                       S, lg, p.nsg, p.parts, (double*)ws);
  else
    hipLaunchKernelGGL(k_sym<ZP_METRIC_MSSD>, grid, dim3(256), 0, st, pts, n, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t,
                       S, lg, p.nsg, p.parts, (double*)ws);
  ZP_LAUNCH_CHECK("zp_pose_error_sym");
  hipLaunchKernelGGL(k_sym_final, dim3(B), dim3(256), 0, st, (const double*)ws, S, p.parts, out);
  ZP_LAUNCH_CHECK("zp_pose_error_sym final");
  return ZP_OK;
}

extern "C" long long zp_vsd_ws_bytes(int B, int H, int W, int ntau) {
  if (!vsd_sizes_ok(B, H, W, ntau)) return -1;
  return (long long)B * vsd_chunks(B, (long)H * W) * VSD_NC * 4;
}

extern "C" int zp_vsd(int B, const float* depth_est, const float* depth_gt, const float* depth_test, int n_test,
                      const int* test_index, int H, int W, const double* K, double delta, const double* taus, int ntau,
                      const double* diameter, double* out, int* counts, void* ws, void* stream) {
  ZP_CHECK_ARG(ntau >= 1 && ntau <= VSD_MAX_TAU, "zp_vsd: ntau %d outside [1, %d]", ntau, VSD_MAX_TAU);
  ZP_CHECK_ARG(vsd_sizes_ok(B, H, W, ntau), "zp_vsd: sizes out of range: B %d, %d x %d", B, H, W);
  ZP_CHECK_ARG(n_test >= 1 && (test_index || n_test >= B), "zp_vsd: n_test %d (B %d, %s test_index)", n_test, B,
               test_index ? "with" : "without");
  ZP_CHECK_ARG(depth_est && depth_gt && depth_test && K && taus && out && ws, "zp_vsd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  VsdTaus tv;
  for (int k = 0; k < VSD_MAX_TAU; ++k) tv.v[k] = k < ntau ? taus[k] : INFINITY;
  const long HW = (long)H * W;
  const int chunks = vsd_chunks(B, HW);
  const dim3 grid(chunks, B);
  const bool vec = HW % 4 == 0 && (((uintptr_t)depth_est | (uintptr_t)depth_gt | (uintptr_t)depth_test) & 15) == 0;
  const float fdelta = (float)delta;
#define ZP_VSD_LAUNCH(NT, VEC)                                                                                      \
  hipLaunchKernelGGL((k_vsd<NT, VEC>), grid, dim3(256), 0, st, depth_est, depth_gt, depth_test, n_test, test_index, \
                     H, W, K, fdelta, tv, diameter, (int*)ws)
  if (ntau <= 16) {
    if (vec) ZP_VSD_LAUNCH(16, true);
    else ZP_VSD_LAUNCH(16, false);
  } else {
    if (vec) ZP_VSD_LAUNCH(32, true);
    else ZP_VSD_LAUNCH(32, false);
  }
#undef ZP_VSD_LAUNCH
  ZP_LAUNCH_CHECK("zp_vsd");
  hipLaunchKernelGGL(k_vsd_final, dim3(B), dim3(64), 0, st, (const int*)ws, chunks, ntau, out, counts);
  ZP_LAUNCH_CHECK("zp_vsd final");
  return ZP_OK;
}
