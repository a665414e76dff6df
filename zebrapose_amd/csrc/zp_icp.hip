// ICP refinement against measured depth on the device: the ordered depth -> point-cloud compaction
// (zp_depth_points) and the whole point-to-point ICP loop of one pose in one workgroup (zp_icp).
// Reference: zebrapose/icp/icp_utils.py:7-13 (rgbd_to_point_cloud), :35-126 (best_fit_transform, icp)
// and :134-176 (ICPRefiner.refine).  The contracts are in include/zp.h; tests/icp_ref.py restates them
// in numpy.
//
// k_depth_points: one workgroup of 1024 threads per image walks it in tiles of 1024 pixels, a lane per
// pixel (coalesced reads).  Per tile: one ballot per wave, the rank of a kept pixel from the popcount
// of the lanes below it, the sixteen wave counts through LDS, and a running base: the points land in
// row-major pixel order whatever the timing.  The statistics are a second walk (the largest distance
// needs the centroid first).
//
// k_icp<NS>: one workgroup of 1024 threads per pose, NS = ceil(N / 1024) source points per thread in
// registers, the destination subsample in LDS as f64 x, y, z (24 bytes a point, 96 KB at N = 4096) and
// behind it each source point's neighbour index (16 KB; parked there while thread 0 solves the fit).
// The neighbour search reads one destination point per step, every lane the same address (an LDS
// broadcast), and uses it for all NS source points of the thread.  Sums (centroids, the mean distance,
// H) go thread -> wave (shuffle tree) -> workgroup (a fixed tree over the sixteen waves): no atomics,
// two runs give the same bits.  Thread 0 solves the 3 x 3 fit.  The only loop is bounded by
// max_iterations; nothing waits on another workgroup.
// Built with -ffp-contract=off: back-projection and squared distances are single IEEE operations.
#include <math.h>
#include "zp_common.h"

namespace zp {

constexpr int IC_T = 1024;  // threads per workgroup
constexpr int IC_WAVES = IC_T / 64;
constexpr int IC_MAXN = 4096;  // subsample size: 4 source points per thread, 112 KB of LDS
constexpr int IC_NRED = 9;     // widest block sum (H)

struct IcpShared {
  double red[IC_WAVES][IC_NRED];
  double tot[IC_NRED];
  double cen[6];  // the last fit's centroids, parked here while thread 0 solves for R
  double T[12];   // the last fit, 3 x 4 row-major
  int wcnt[IC_WAVES];
};

// v[k] summed over the workgroup into s.tot[k]; the same order on every run
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], IcpShared& s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += __shfl_down(v[k], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) s.red[wave][k] = v[k];
  }
  __syncthreads();
  if (tid < NV) {
    const double a = ((s.red[0][tid] + s.red[1][tid]) + (s.red[2][tid] + s.red[3][tid])) +
                     ((s.red[4][tid] + s.red[5][tid]) + (s.red[6][tid] + s.red[7][tid]));
    const double b = ((s.red[8][tid] + s.red[9][tid]) + (s.red[10][tid] + s.red[11][tid])) +
                     ((s.red[12][tid] + s.red[13][tid]) + (s.red[14][tid] + s.red[15][tid]));
    s.tot[tid] = a + b;
  }
  __syncthreads();
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double norm3(const double* a) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }

// V (columns: eigenvectors of H^T H, largest first) of a thin cloud, polished against H itself.  H^T H
// holds s2^2 beside s1^2, so its eigenvectors fix v2 against v3 only to 2^-53 s1^2 / (s2^2 - s3^2); v1 is
// good to 2^-53.  H v2 and H v3 hold s2 and s3 themselves: v2 and v3 are turned in their plane until
// those two are orthogonal (one-sided Jacobi on one pair; from a V that close the second turn is already
// rounding), which makes them as accurate as a 2^-53 |H| change of H allows.
__device__ void polish_v(const double* Hm, double (&V)[3][3]) {
  for (int turn = 0; turn < 3; ++turn) {
    double g[3], h[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      g[i] = (Hm[3 * i] * V[0][1] + Hm[3 * i + 1] * V[1][1]) + Hm[3 * i + 2] * V[2][1];
      h[i] = (Hm[3 * i] * V[0][2] + Hm[3 * i + 1] * V[1][2]) + Hm[3 * i + 2] * V[2][2];
    }
    double a = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    double b = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
    const double c = (g[0] * h[0] + g[1] * h[1]) + g[2] * h[2];
    if (b > a) {  // v2 is the longer of the two; a turn (below 45 degrees) keeps it the longer
      const double a_ = a;
      a = b, b = a_;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double v_ = V[k][1];
        V[k][1] = V[k][2], V[k][2] = v_;
      }
    }
    if (fabs(c) <= 1e-15 * sqrt(a * b) || c == 0.0) break;
    const double theta = (b - a) / (2.0 * c);
    const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double vp = V[k][1], vq = V[k][2];
      V[k][1] = cs * vp - sn * vq, V[k][2] = sn * vp + cs * vq;
    }
  }
}

// Kabsch rotation of H = sum a b^T = U S V^T: R = V U^T with the reflection fix, as
// R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T.  v1, v2: the two leading eigenvectors of H^T H (cyclic
// Jacobi, every index a constant so the matrices stay in registers; polished against H where the cloud
// is thin), u_k = H v_k / |H v_k|.
__device__ void kabsch(const double* Hm, double* R) {
  double A[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A[i][j] = (Hm[i] * Hm[j] + Hm[3 + i] * Hm[3 + j]) + Hm[6 + i] * Hm[6 + j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = A[p][q];
        if (fabs(apq) <= 1e-17 * sqrt(fabs(A[p][p] * A[q][q])) || apq == 0.0) continue;
        rotated = true;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - sn * akq;
          A[k][q] = sn * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - sn * aqk;
          A[q][k] = sn * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - sn * vkq;
          V[k][q] = sn * vkp + c * vkq;
        }
      }
    if (!rotated) break;
  }
  // the two largest eigenvalues' columns to the front (three compare-swaps)
  double ev[3] = {A[0][0], A[1][1], A[2][2]};
#define ZP_ICP_CSWAP(i, j)                         \
  if (ev[j] > ev[i]) {                             \
    const double e_ = ev[i];                       \
    ev[i] = ev[j], ev[j] = e_;                     \
    for (int k = 0; k < 3; ++k) {                  \
      const double v_ = V[k][i];                   \
      V[k][i] = V[k][j], V[k][j] = v_;             \
    }                                              \
  }
  ZP_ICP_CSWAP(0, 1)
  ZP_ICP_CSWAP(0, 2)
  ZP_ICP_CSWAP(1, 2)
#undef ZP_ICP_CSWAP
  // a thin cloud, s2 <= 1e-3 s1 (a thicker one keeps its bits; its V is good to 1e-10 or better)
  if (ev[1] < 1e-6 * ev[0]) polish_v(Hm, V);
  const double v1[3] = {V[0][0], V[1][0], V[2][0]}, v2[3] = {V[0][1], V[1][1], V[2][1]};
  double u1[3], u2[3], v3[3], u3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u1[i] = (Hm[3 * i] * v1[0] + Hm[3 * i + 1] * v1[1]) + Hm[3 * i + 2] * v1[2];
    u2[i] = (Hm[3 * i] * v2[0] + Hm[3 * i + 1] * v2[1]) + Hm[3 * i + 2] * v2[2];
  }
  const double s1 = norm3(u1);
  if (!(s1 > 0.0)) {  // H = 0 (or not finite): no rotation is better than another
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (k & 3) == 0 ? 1.0 : 0.0;
    return;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] /= s1;
  const double d12 = (u2[0] * u1[0] + u2[1] * u1[1]) + u2[2] * u1[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) u2[i] -= d12 * u1[i];
  double s2 = norm3(u2);
  if (!(s2 > 1e-14 * s1)) {  // rank 1: any unit vector across u1 (the axis u1 leans on least)
    const double a0 = fabs(u1[0]), a1 = fabs(u1[1]), a2 = fabs(u1[2]);
    const int e = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = (i == e ? 1.0 : 0.0) - u1[e] * u1[i];
    s2 = norm3(u2);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) u2[i] /= s2;
  cross3(v1, v2, v3);
  cross3(u1, u2, u3);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (v1[i] * u1[j] + v2[i] * u2[j]) + v3[i] * u3[j];
}

// best_fit_transform (icp_utils.py:35-80) of the pairs a -> b of all threads into s.T: slot k of thread
// tid is pair tid + 1024 k, counted while below n, and geta / getb(k, p) fetch its two points (they are
// called twice, so that the points need not stay in registers between the two sums).  dsum rides along
// and comes back as its mean over the n pairs.  mode 0: full, 1: translation alone (depth_only), 2: no
// z shift (no_depth).
template <int NS, class GetA, class GetB>
__device__ __forceinline__ double fit(int n, int mode, double dsum, IcpShared& s, GetA geta, GetB getb) {
  const int tid = threadIdx.x;
  double v7[7] = {0, 0, 0, 0, 0, 0, dsum};
#pragma unroll
  for (int k = 0; k < NS; ++k)
    if (tid + IC_T * k < n) {
      double a[3], b[3];
      geta(k, a), getb(k, b);
#pragma unroll
      for (int c = 0; c < 3; ++c) v7[c] += a[c], v7[3 + c] += b[c];
    }
  block_sum<7>(v7, s);
  const double dn = (double)n;
  const double cA[3] = {s.tot[0] / dn, s.tot[1] / dn, s.tot[2] / dn};
  const double cB[3] = {s.tot[3] / dn, s.tot[4] / dn, s.tot[5] / dn};
  const double mean = s.tot[6] / dn;
  if (mode != 1) {
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < NS; ++k)
      if (tid + IC_T * k < n) {
        double a[3], b[3];
        geta(k, a), getb(k, b);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) h[3 * r + c] += (a[r] - cA[r]) * (b[c] - cB[c]);
      }
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) s.cen[c] = cA[c], s.cen[3 + c] = cB[c];
    }
    block_sum<9>(h, s);
  }
  if (tid == 0) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3];
    if (mode != 1) {
      kabsch(s.tot, R);
#pragma unroll
      for (int r = 0; r < 3; ++r)
        t[r] = s.cen[3 + r] - ((R[3 * r] * s.cen[0] + R[3 * r + 1] * s.cen[1]) + R[3 * r + 2] * s.cen[2]);
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r) t[r] = cB[r] - cA[r];
    }
    if (mode == 2) t[2] = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      s.T[4 * r] = R[3 * r], s.T[4 * r + 1] = R[3 * r + 1], s.T[4 * r + 2] = R[3 * r + 2], s.T[4 * r + 3] = t[r];
    }
  }
  __syncthreads();
  return mean;
}

// floor(draw * count) as an index below count, whatever the draw holds
__device__ __forceinline__ int draw_index(double draw, int count) {
  const double v = draw * (double)count;
  return v >= 0.0 ? (v < (double)count ? (int)v : count - 1) : 0;
}

template <int NS>
__global__ void __launch_bounds__(IC_T) k_icp(
    int N, const double* __restrict__ src_pts, const int* __restrict__ src_counts, int src_cap,
    const double* __restrict__ dst_pts, const int* __restrict__ dst_counts, int dst_cap,
    const double* __restrict__ draws_src, const double* __restrict__ draws_dst, int max_iterations, double tolerance,
    int mode, double min_fraction, double angle_limit, const double* __restrict__ Rin, const double* __restrict__ tin,
    double* __restrict__ R_out, double* __restrict__ t_out, int* __restrict__ status, int* __restrict__ iterations,
    double* __restrict__ mean_error, int* __restrict__ nn, double* __restrict__ T_out) {
  extern __shared__ double dstL[];  // [N][3], then the neighbour indices i32 [N]
  int* nnL = reinterpret_cast<int*>(dstL + 3 * (size_t)N);
  __shared__ IcpShared s;
  const int b = blockIdx.x, tid = threadIdx.x;
  int ns = src_counts[b], nd = dst_counts[b];
  ns = ns < 0 ? 0 : (ns > src_cap ? src_cap : ns);
  nd = nd < 0 ? 0 : (nd > dst_cap ? dst_cap : nd);
  int n = ns < nd ? ns : nd;
  n = n < N ? n : N;
  const int st0 = ns == 0 ? 1 : ((double)nd < (double)ns * min_fraction || n == 0) ? 2 : 0;
  if (st0 != 0) {  // uniform over the workgroup
    if (tid < 9) R_out[9 * (size_t)b + tid] = Rin[9 * (size_t)b + tid];
    if (tid < 3) t_out[3 * (size_t)b + tid] = tin[3 * (size_t)b + tid];
    if (tid == 0) status[b] = st0, iterations[b] = 0, mean_error[b] = 0.0;
    if (T_out && tid < 16) T_out[16 * (size_t)b + tid] = (tid % 5) == 0 ? 1.0 : 0.0;
    if (nn)
      for (int i = tid; i < N; i += IC_T) nn[(size_t)b * N + i] = -1;
    return;
  }

  // the two subsamples (icp_utils.py:155-156): index i is floor(draw[i] * count)
  const double* sp = src_pts + (size_t)b * src_cap * 3;
  const double* dp = dst_pts + (size_t)b * dst_cap * 3;
  double cur[NS][3];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int i = tid + IC_T * k;
#pragma unroll
    for (int c = 0; c < 3; ++c) cur[k][c] = 0.0;
    if (i < n) {
      const int js = draw_index(draws_src[(size_t)b * N + i], ns);
      const int jd = draw_index(draws_dst[(size_t)b * N + i], nd);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        cur[k][c] = sp[3 * (size_t)js + c];
        dstL[3 * i + c] = dp[3 * (size_t)jd + c];
      }
    }
  }
  __syncthreads();

  auto get_cur = [&](int k, double* p) { p[0] = cur[k][0], p[1] = cur[k][1], p[2] = cur[k][2]; };
  int it_run = 0;
  double prev = 0.0, mean = 0.0;
  for (int it = 0; it < max_iterations; ++it) {
    double best[NS];
    int bj[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) best[k] = INFINITY, bj[k] = 0;
    // a thread whose first slot is past n has no point at all and skips the search (whole idle waves
    // when n is small); a thread's later slots past n are searched with the rest and never read, which
    // keeps the loop body free of per-slot branches
    const int nj = tid < n ? n : 0;
#pragma unroll 2
    for (int j = 0; j < nj; ++j) {
      const double qx = dstL[3 * j], qy = dstL[3 * j + 1], qz = dstL[3 * j + 2];
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const double dx = cur[k][0] - qx, dy = cur[k][1] - qy, dz = cur[k][2] - qz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best[k]) best[k] = d2, bj[k] = j;  // strict: ties stay with the lowest index
      }
    }
    double dsum = 0.0;
#pragma unroll
    for (int k = 0; k < NS; ++k)
      if (tid + IC_T * k < n) dsum += sqrt(best[k]), nnL[tid + IC_T * k] = bj[k];  // read back by this thread alone
    mean = fit<NS>(n, mode, dsum, s, get_cur, [&](int k, double* p) {
      const int j = nnL[tid + IC_T * k];
      p[0] = dstL[3 * j], p[1] = dstL[3 * j + 1], p[2] = dstL[3 * j + 2];
    });
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const double x = cur[k][0], y = cur[k][1], z = cur[k][2];
#pragma unroll
      for (int r = 0; r < 3; ++r) cur[k][r] = ((s.T[4 * r] * x + s.T[4 * r + 1] * y) + s.T[4 * r + 2] * z) + s.T[4 * r + 3];
    }
    it_run = it + 1;
    if (fabs(prev - mean) < tolerance) break;  // mean comes from LDS: the same in every thread
    prev = mean;
  }
  if (nn) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = tid + IC_T * k;
      if (i < N) nn[(size_t)b * N + i] = i < n ? nnL[i] : -1;
    }
  }

  // the final transform: from the original subsample to where it ended up (icp_utils.py:119)
  fit<NS>(n, mode, 0.0, s, [&](int k, double* p) {
    const int js = draw_index(draws_src[(size_t)b * N + tid + IC_T * k], ns);
    p[0] = sp[3 * (size_t)js], p[1] = sp[3 * (size_t)js + 1], p[2] = sp[3 * (size_t)js + 2];
  }, get_cur);
  if (tid != 0) return;
  double Tm[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) Tm[k] = s.T[k];
  int st = 0;
  if (mode == 2) {  // transform.rotation_from_matrix's angle: atan2(|sin|, cos) from the skew part and the trace
    const double ax = Tm[9] - Tm[6], ay = Tm[2] - Tm[8], az = Tm[4] - Tm[1];
    const double sn = 0.5 * sqrt((ax * ax + ay * ay) + az * az), cs = 0.5 * (((Tm[0] + Tm[5]) + Tm[10]) - 1.0);
    if (atan2(sn, cs) > angle_limit) st = 3;
  }
  const double* Rb = Rin + 9 * (size_t)b;
  const double* tb = tin + 3 * (size_t)b;
  if (st == 0) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c)
        R_out[9 * (size_t)b + 3 * r + c] = (Tm[4 * r] * Rb[c] + Tm[4 * r + 1] * Rb[3 + c]) + Tm[4 * r + 2] * Rb[6 + c];
      t_out[3 * (size_t)b + r] = ((Tm[4 * r] * tb[0] + Tm[4 * r + 1] * tb[1]) + Tm[4 * r + 2] * tb[2]) + Tm[4 * r + 3];
    }
  } else {
    for (int k = 0; k < 9; ++k) R_out[9 * (size_t)b + k] = Rb[k];
    for (int k = 0; k < 3; ++k) t_out[3 * (size_t)b + k] = tb[k];
  }
  status[b] = st, iterations[b] = it_run, mean_error[b] = mean;
  if (T_out) {
    for (int k = 0; k < 12; ++k) T_out[16 * (size_t)b + k] = Tm[k];
    for (int k = 12; k < 16; ++k) T_out[16 * (size_t)b + k] = k == 15 ? 1.0 : 0.0;
  }
}

// One pixel of rgbd_to_point_cloud (icp_utils.py:7-13): kept iff the depth is finite and positive and,
// with a filter, the point lies within lim2 (squared) of the filter's centre.
struct DpCam {
  double fx, fy, cx, cy, fcx, fcy, fcz, lim2;
  bool filt;
};
__device__ __forceinline__ bool depth_point(const float* __restrict__ img, long long i, long long npix, int W,
                                            const DpCam& c, double* p) {
  if (i >= npix) return false;
  const float zf = img[i];
  if (!(zf > 0.f) || !(zf < INFINITY)) return false;
  const int v = (int)(i / W), u = (int)(i - (long long)v * W);
  const double z = (double)zf;
  p[0] = (((double)u - c.cx) * z) / c.fx;
  p[1] = (((double)v - c.cy) * z) / c.fy;
  p[2] = z;
  if (c.filt) {
    const double dx = p[0] - c.fcx, dy = p[1] - c.fcy, dz = p[2] - c.fcz;
    if (!((dx * dx + dy * dy) + dz * dz < c.lim2)) return false;
  }
  return true;
}

__global__ void __launch_bounds__(IC_T) k_depth_points(const float* __restrict__ depth, const double* __restrict__ K,
                                                       int H, int W, int cap, const double* __restrict__ filter,
                                                       double factor, int* __restrict__ counts,
                                                       double* __restrict__ pts, double* __restrict__ stats) {
  __shared__ IcpShared s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long npix = (long long)H * W;
  const float* img = depth + (size_t)b * npix;
  double* out = pts + (size_t)b * cap * 3;
  DpCam c;
  c.fx = K[4 * b], c.fy = K[4 * b + 1], c.cx = K[4 * b + 2], c.cy = K[4 * b + 3];
  c.filt = filter != nullptr;
  c.fcx = c.fcy = c.fcz = c.lim2 = 0.0;
  if (c.filt) {
    c.fcx = filter[4 * b], c.fcy = filter[4 * b + 1], c.fcz = filter[4 * b + 2];
    const double lim = factor * filter[4 * b + 3];
    c.lim2 = lim * lim;
  }
  long long base = 0;
  double sum[3] = {0, 0, 0};
  for (long long t0 = 0; t0 < npix; t0 += IC_T) {  // the trip count is the same in every thread
    double p[3];
    const bool keep = depth_point(img, t0 + tid, npix, W, c, p);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s.wcnt[wave] = __popcll(m);
    __syncthreads();
    int below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < IC_WAVES; ++w) {
      const int cw = s.wcnt[w];
      below += w < wave ? cw : 0;
      total += cw;
    }
    if (keep) {
      const long long pos = base + below + __popcll(m & ((1ull << lane) - 1ull));
      if (pos < cap) out[3 * pos] = p[0], out[3 * pos + 1] = p[1], out[3 * pos + 2] = p[2];
      sum[0] += p[0], sum[1] += p[1], sum[2] += p[2];
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) counts[b] = (int)base;
  if (!stats) return;
  if (base == 0) {
    if (tid < 4) stats[4 * (size_t)b + tid] = 0.0;
    return;
  }
  // centroid and the largest distance from it (icp_utils.py:139-141)
  block_sum<3>(sum, s);
  const double dn = (double)base;
  const double cen[3] = {s.tot[0] / dn, s.tot[1] / dn, s.tot[2] / dn};
  double far2 = 0.0;
  for (long long t0 = 0; t0 < npix; t0 += IC_T) {
    double p[3];
    if (depth_point(img, t0 + tid, npix, W, c, p)) {
      const double dx = p[0] - cen[0], dy = p[1] - cen[1], dz = p[2] - cen[2];
      far2 = fmax(far2, (dx * dx + dy * dy) + dz * dz);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) far2 = fmax(far2, __shfl_down(far2, off));
  __syncthreads();  // every thread has read s.tot
  if (lane == 0) s.red[wave][0] = far2;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < IC_WAVES; ++w) far2 = fmax(far2, s.red[w][0]);
    double* o = stats + 4 * (size_t)b;
    o[0] = cen[0], o[1] = cen[1], o[2] = cen[2], o[3] = sqrt(far2);
  }
}

static bool depth_sizes_ok(int B, int H, int W, int cap) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && (long long)H * W <= (1LL << 24) &&
         cap >= 1 && cap <= (1 << 24) && (long long)B * cap <= (1LL << 28);
}
static bool icp_sizes_ok(int B, int N) { return B >= 1 && B <= 65535 && N >= 1 && N <= IC_MAXN; }

typedef void (*icp_kernel_t)(int, const double*, const int*, int, const double*, const int*, int, const double*,
                             const double*, int, double, int, double, double, const double*, const double*, double*,
                             double*, int*, int*, double*, int*, double*);
static icp_kernel_t icp_kernel(int ns) {
  switch (ns) {
    case 1: return k_icp<1>;
    case 2: return k_icp<2>;
    case 3: return k_icp<3>;
    default: return k_icp<4>;
  }
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_depth_points_ws_bytes(int B, int H, int W, int cap) {
  return depth_sizes_ok(B, H, W, cap) ? 0 : -1;
}

extern "C" int zp_depth_points(int B, int H, int W, const float* depth, const double* K, int cap, const double* filter,
                               double factor, int* counts, double* pts, double* stats, void* ws, void* stream) {
  (void)ws;
  ZP_CHECK_ARG(depth_sizes_ok(B, H, W, cap), "zp_depth_points: sizes out of range: B %d, %d x %d, cap %d", B, H, W, cap);
  ZP_CHECK_ARG(depth && K && counts && pts, "zp_depth_points: NULL pointer");
  ZP_CHECK_ARG(!filter || (factor >= 0 && factor < INFINITY), "zp_depth_points: factor %g must be finite and >= 0",
               factor);
  ZP_CHECK_ARG(!filter || filter != stats, "zp_depth_points: stats cannot overwrite the filter");
  hipLaunchKernelGGL(k_depth_points, dim3(B), dim3(IC_T), 0, (hipStream_t)stream, depth, K, H, W, cap, filter, factor,
                     counts, pts, stats);
  ZP_LAUNCH_CHECK("zp_depth_points");
  return ZP_OK;
}

extern "C" long long zp_icp_ws_bytes(int B, int N) { return icp_sizes_ok(B, N) ? 0 : -1; }

extern "C" int zp_icp(int B, int N, const double* src_pts, const int* src_counts, int src_cap, const double* dst_pts,
                      const int* dst_counts, int dst_cap, const double* draws_src, const double* draws_dst,
                      int max_iterations, double tolerance, int mode, double min_fraction, double angle_limit,
                      const double* R, const double* t, double* R_out, double* t_out, int* status, int* iterations,
                      double* mean_error, int* nn, double* T, void* ws, void* stream) {
  (void)ws;
  ZP_CHECK_ARG(icp_sizes_ok(B, N), "zp_icp: sizes out of range: B %d, N %d (1 .. %d)", B, N, IC_MAXN);
  ZP_CHECK_ARG(src_cap >= 1 && dst_cap >= 1 && (long long)B * src_cap <= (1LL << 28) &&
                   (long long)B * dst_cap <= (1LL << 28),
               "zp_icp: src_cap %d, dst_cap %d", src_cap, dst_cap);
  ZP_CHECK_ARG(max_iterations >= 1 && max_iterations <= 100000, "zp_icp: max_iterations %d (1 .. 100000)",
               max_iterations);
  ZP_CHECK_ARG(tolerance == tolerance, "zp_icp: tolerance is NaN");
  ZP_CHECK_ARG(mode >= 0 && mode <= 2, "zp_icp: mode %d (0 full, 1 depth_only, 2 no_depth)", mode);
  ZP_CHECK_ARG(min_fraction >= 0 && min_fraction < INFINITY && angle_limit >= 0,
               "zp_icp: min_fraction %g must be finite and >= 0, angle_limit %g >= 0", min_fraction, angle_limit);
  ZP_CHECK_ARG(src_pts && src_counts && dst_pts && dst_counts && draws_src && draws_dst && R && t && R_out && t_out &&
                   status && iterations && mean_error,
               "zp_icp: NULL pointer");
  ZP_CHECK_ARG(R != R_out && t != t_out, "zp_icp: the pose cannot be updated in place");
  // the destination points and neighbour indices take up to 112 KB of LDS, beyond the 64 KB a kernel
  // gets unasked: raised once per device (a process can drive several GPUs), and a failure is reported
  // as such.  Two threads racing here both set the same value: the flags need no lock.
  static bool attr[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    set_error("zp_icp: no current device");
    return ZP_ERR_HIP;
  }
  if (!attr[dev]) {
    for (int ns = 1; ns <= 4; ++ns)
      if (hipFuncSetAttribute((const void*)icp_kernel(ns), hipFuncAttributeMaxDynamicSharedMemorySize,
                              IC_MAXN * 28) != hipSuccess) {
        set_error("zp_icp: hipFuncSetAttribute(MaxDynamicSharedMemorySize, %d bytes) failed on device %d",
                  IC_MAXN * 28, dev);
        return ZP_ERR_HIP;
      }
    attr[dev] = true;
  }
  const size_t lds = (size_t)N * 28;
  hipLaunchKernelGGL(icp_kernel((N + IC_T - 1) / IC_T), dim3(B), dim3(IC_T), lds, (hipStream_t)stream, N, src_pts,
                     src_counts, src_cap, dst_pts, dst_counts, dst_cap, draws_src, draws_dst, max_iterations,
                     tolerance, mode, min_fraction, angle_limit, R, t, R_out, t_out, status, iterations, mean_error,
                     nn, T);
  ZP_LAUNCH_CHECK("zp_icp");
  return ZP_OK;
}
