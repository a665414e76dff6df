// Local optimisation of a RANSAC-EPnP pose on the device (zp_pnp_lo, include/zp.h "PnP local
// optimisation"): rounds of inlier re-selection under the current pose, each followed by
// Levenberg-Marquardt on the selected set's reprojection error.  It stands in for the local
// optimisation of the reference's default solver (Progressive-X,
// binary_code_helper/CNN_output_to_pose.py:132-144) without its graph cuts, spatial coherence term
// or multi-model proposals; tests/pnp_lo_ref.py is the executable definition.
//
// One workgroup of 256 threads per crop, the whole loop in one launch (as zp_icp).  The points are
// re-read from memory in every pass (they stay in L2), the inlier mask lives in the workspace, one
// byte per point, and thread t owns points t, t + 256, ...  Every sum is reduced thread -> wave
// (butterfly) -> the four wave partials in a fixed order, and every thread receives the total, so the
// control flow below (lo_run) is executed by all 256 threads on the same values and needs no
// broadcast.  No atomics.
//
// The per-point math and the loop are host + device code: tools/pnp_lo_host_check.hip runs lo_run
// on the CPU with serial sums.  This file is built with -ffp-contract=off: the header fixes the
// per-point operation order, one IEEE operation per step.
#include <math.h>
#include "zp_common.h"

#define ZP_HD __host__ __device__

namespace zp {

struct LoCam {
  double fx, fy, cx, cy;
};
struct LoPose {
  double R[9], t[3];
};

constexpr int LO_T = 256;       // threads per crop
constexpr int LO_NACC = 28;     // upper triangle of H (21), g (6), C
constexpr int LO_MIN_SET = 6;

// Xc = R p + t, e = (u, v) - projection, r2 = |e|^2; true iff the point passes the inlier test's
// geometric half (Xc.z > 0 and r2 finite)
ZP_HD inline bool lo_project(const LoPose& P, const LoCam& K, const double* p, double u, double v, double* Xc,
                             double* e, double* r2) {
  Xc[0] = ((P.R[0] * p[0] + P.R[1] * p[1]) + P.R[2] * p[2]) + P.t[0];
  Xc[1] = ((P.R[3] * p[0] + P.R[4] * p[1]) + P.R[5] * p[2]) + P.t[1];
  Xc[2] = ((P.R[6] * p[0] + P.R[7] * p[1]) + P.R[8] * p[2]) + P.t[2];
  e[0] = u - ((K.fx * Xc[0]) / Xc[2] + K.cx);
  e[1] = v - ((K.fy * Xc[1]) / Xc[2] + K.cy);
  *r2 = e[0] * e[0] + e[1] * e[1];
  return Xc[2] > 0.0 && __builtin_isfinite(*r2);
}

// the rows of J = Jp [-[Xc]x | I]
ZP_HD inline void lo_jacobian(const LoCam& K, const double* Xc, double* J0, double* J1) {
  const double a = K.fx / Xc[2], b = K.fy / Xc[2], zz = Xc[2] * Xc[2];
  const double c = -((K.fx * Xc[0]) / zz), d = -((K.fy * Xc[1]) / zz);
  J0[0] = c * Xc[1];
  J0[1] = a * Xc[2] - c * Xc[0];
  J0[2] = -(a * Xc[1]);
  J0[3] = a;
  J0[4] = 0.0;
  J0[5] = c;
  J1[0] = d * Xc[1] - b * Xc[2];
  J1[1] = -(d * Xc[0]);
  J1[2] = b * Xc[0];
  J1[3] = 0.0;
  J1[4] = b;
  J1[5] = d;
}

// one point's terms of H (upper triangle by rows), g and C
ZP_HD inline void lo_accum(const LoCam& K, const double* Xc, const double* e, double r2, double* acc) {
  double J0[6], J1[6];
  lo_jacobian(K, Xc, J0, J1);
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) acc[k++] += J0[r] * J0[c] + J1[r] * J1[c];
#pragma unroll
  for (int r = 0; r < 6; ++r) acc[21 + r] += J0[r] * e[0] + J1[r] * e[1];
  acc[27] += r2;
}

// (H + lambda diag(H)) theta = g by Cholesky; false on a pivot that is not positive and finite
ZP_HD inline bool lo_solve(const double* hb, double lambda, double* th) {
  double A[6][6];
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) A[r][c] = A[c][r] = hb[k++];
  for (int r = 0; r < 6; ++r) A[r][r] = A[r][r] + lambda * A[r][r];
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    for (int q = 0; q < j; ++q) s = s - A[j][q] * A[j][q];
    if (!(s > 0.0 && __builtin_isfinite(s))) return false;
    const double l = sqrt(s);
    A[j][j] = l;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int q = 0; q < j; ++q) v = v - A[i][q] * A[j][q];
      A[i][j] = v / l;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double v = hb[21 + i];
    for (int q = 0; q < i; ++q) v = v - A[i][q] * th[q];
    th[i] = v / A[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = th[i];
    for (int q = i + 1; q < 6; ++q) v = v - A[q][i] * th[q];
    th[i] = v / A[i][i];
  }
  return true;
}

// R' = E R, t' = E t + theta_t, E = exp([theta_r]x) = I + a K + c K^2 (zp_edge_refine_step's form)
ZP_HD inline void lo_update(const LoPose& P, const double* th, LoPose& Q) {
  const double wx = th[0], wy = th[1], wz = th[2];
  const double a2 = (wx * wx + wy * wy) + wz * wz, an = sqrt(a2);
  double ca, cc;
  if (an < 1e-8) {
    ca = 1.0 - a2 / 6.0, cc = 0.5 - a2 / 24.0;
  } else {
    const double sh = sin(0.5 * an);
    ca = sin(an) / an, cc = 2.0 * sh * sh / a2;
  }
  const double Kx[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
  double E[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double k2 = (Kx[3 * r] * Kx[c] + Kx[3 * r + 1] * Kx[3 + c]) + Kx[3 * r + 2] * Kx[6 + c];
      E[3 * r + c] = ((r == c ? 1.0 : 0.0) + ca * Kx[3 * r + c]) + cc * k2;
    }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Q.R[3 * r + c] = (E[3 * r] * P.R[c] + E[3 * r + 1] * P.R[3 + c]) + E[3 * r + 2] * P.R[6 + c];
    Q.t[r] = ((E[3 * r] * P.t[0] + E[3 * r + 1] * P.t[1]) + E[3 * r + 2] * P.t[2]) + th[3 + r];
  }
}

// The loop.  Ctx supplies the sums over the crop's points, each returning the same value to every
// caller (one caller on the host, the 256 threads of a workgroup on the device):
//   select(P, thr2, compare, &count, &changed)  new mask under P; changed: entries that differ from
//                                               the mask before (counted only with compare)
//   normal(P, acc[28])                          H, g, C over the mask
//   trial(P)                                    C' over the mask, +inf with a masked point at Z <= 0
//   final(P, thr2, &count, &cost)               the set under P (the mask is left alone)
//   writer()                                    whether this caller stores trace / Hb
template <class Ctx>
ZP_HD void lo_run(Ctx& cx, const LoPose& in, double thr2, int rounds, int steps, LoPose& P, int* inliers,
                  double* cost, int* status, int* trace, double* Hb) {
  P = in;
  const bool wr = cx.writer();
  if (wr && trace)
    for (int k = 0; k < 2 * rounds; ++k) trace[k] = -1;
  bool hb_open = true;
  for (int r = 0; r < rounds; ++r) {
    int cnt, changed;
    cx.select(P, thr2, r > 0, &cnt, &changed);
    if (wr && trace) trace[2 * r] = cnt, trace[2 * r + 1] = 0;
    if (cnt < LO_MIN_SET) {
      if (r == 0) {
        *inliers = cnt;
        *cost = 0.0;
        *status = 2;
        if (wr && Hb)
          for (int k = 0; k < LO_NACC; ++k) Hb[k] = 0.0;
        return;
      }
      break;
    }
    if (r > 0 && changed == 0) break;
    double lambda = 1e-3, acc[LO_NACC];
    bool fresh = false;
    int its = 0;
    while (its < steps) {
      ++its;
      if (!fresh) {
        cx.normal(P, acc);
        fresh = true;
        if (hb_open) {
          hb_open = false;
          if (wr && Hb)
            for (int k = 0; k < LO_NACC; ++k) Hb[k] = acc[k];
        }
      }
      const double C = acc[27];
      double th[6];
      bool accept = false;
      LoPose Q;
      double Cn = 0.0;
      if (lo_solve(acc, lambda, th)) {
        lo_update(P, th, Q);
        Cn = cx.trial(Q);
        accept = __builtin_isfinite(Cn) && Cn < C;
      }
      if (accept) {
        P = Q;
        fresh = false;
        lambda = fmax(0.1 * lambda, 1e-9);
        if (C - Cn <= 1e-10 * C) break;
      } else {
        lambda = 10.0 * lambda;
        if (lambda > 1e6) break;
      }
    }
    if (wr && trace) trace[2 * r + 1] = its;
  }
  int cnt;
  double c;
  cx.final(P, thr2, &cnt, &c);
  *inliers = cnt;
  *cost = c;
  *status = 0;
}

// block reduction of NV doubles: wave butterfly, then the 4 wave partials in a fixed order; every
// thread ends with the total (k_pnp_refine's block_sum)
template <int NV>
__device__ void lo_block_sum(double (&v)[NV], double* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double x = v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    if (lane == 0) sh[k * 4 + w] = x;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = ((sh[k * 4] + sh[k * 4 + 1]) + sh[k * 4 + 2]) + sh[k * 4 + 3];
  __syncthreads();
}

struct LoDevCtx {
  int n;
  const int* xy;       // the crop's [n][2]
  const float* xyz;    // the crop's [n][3]
  uint8_t* mask;       // the crop's [HW]
  LoCam K;
  double* sh;          // LDS [LO_NACC][4]

  __device__ void load(int i, double* p, double* u, double* v) const {
    p[0] = (double)xyz[3 * (size_t)i];
    p[1] = (double)xyz[3 * (size_t)i + 1];
    p[2] = (double)xyz[3 * (size_t)i + 2];
    *u = (double)xy[2 * (size_t)i];
    *v = (double)xy[2 * (size_t)i + 1];
  }
  __device__ bool writer() const { return threadIdx.x == 0; }
  __device__ void select(const LoPose& P, double thr2, bool compare, int* count, int* changed) {
    double s[2] = {0.0, 0.0};  // counts <= 2^24: exact in f64
    for (int i = threadIdx.x; i < n; i += LO_T) {
      double p[3], u, v, Xc[3], e[2], r2;
      load(i, p, &u, &v);
      const bool in = lo_project(P, K, p, u, v, Xc, e, &r2) && r2 <= thr2;
      s[0] += in ? 1.0 : 0.0;
      if (compare) s[1] += (mask[i] != 0) != in ? 1.0 : 0.0;
      mask[i] = in ? 1 : 0;
    }
    lo_block_sum<2>(s, sh);
    *count = (int)s[0];
    *changed = (int)s[1];
  }
  __device__ void normal(const LoPose& P, double (&acc)[LO_NACC]) {
#pragma unroll
    for (int k = 0; k < LO_NACC; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += LO_T) {
      if (!mask[i]) continue;
      double p[3], u, v, Xc[3], e[2], r2;
      load(i, p, &u, &v);
      lo_project(P, K, p, u, v, Xc, e, &r2);
      lo_accum(K, Xc, e, r2, acc);
    }
    lo_block_sum<LO_NACC>(acc, sh);
  }
  __device__ double trial(const LoPose& P) {
    double s[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += LO_T) {
      if (!mask[i]) continue;
      double p[3], u, v, Xc[3], e[2], r2;
      load(i, p, &u, &v);
      lo_project(P, K, p, u, v, Xc, e, &r2);
      s[0] += Xc[2] > 0.0 ? r2 : INFINITY;
    }
    lo_block_sum<1>(s, sh);
    return s[0];
  }
  __device__ void final(const LoPose& P, double thr2, int* count, double* cost) {
    double s[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += LO_T) {
      double p[3], u, v, Xc[3], e[2], r2;
      load(i, p, &u, &v);
      if (lo_project(P, K, p, u, v, Xc, e, &r2) && r2 <= thr2) {
        s[0] += 1.0;
        s[1] += r2;
      }
    }
    lo_block_sum<2>(s, sh);
    *count = (int)s[0];
    *cost = s[1];
  }
};

__global__ void __launch_bounds__(LO_T) k_pnp_lo(int HW, const int* __restrict__ counts, const int* __restrict__ xy,
                                                 const float* __restrict__ xyz, const double* __restrict__ Kd,
                                                 const double* __restrict__ R, const double* __restrict__ t,
                                                 const int* __restrict__ active, double thr2, int rounds, int steps,
                                                 double* __restrict__ R_out, double* __restrict__ t_out,
                                                 int* __restrict__ inliers, double* __restrict__ cost,
                                                 int* __restrict__ status, int* __restrict__ trace,
                                                 double* __restrict__ Hb, uint8_t* __restrict__ ws) {
  __shared__ double sh[LO_NACC * 4];
  const size_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = min(max(counts[b], 0), HW);
  int* tr = trace ? trace + b * 2 * rounds : nullptr;
  double* hb = Hb ? Hb + b * LO_NACC : nullptr;
  LoPose in;
  bool finite = true;
  for (int k = 0; k < 9; ++k) in.R[k] = R[9 * b + k], finite = finite && __builtin_isfinite(in.R[k]);
  for (int k = 0; k < 3; ++k) in.t[k] = t[3 * b + k], finite = finite && __builtin_isfinite(in.t[k]);
  LoPose out = in;
  int inl = 0, st = 1;
  double c = 0.0;
  if ((active && active[b] == 0) || n < LO_MIN_SET || !finite) {
    if (tid == 0) {
      if (tr)
        for (int k = 0; k < 2 * rounds; ++k) tr[k] = -1;
      if (hb)
        for (int k = 0; k < LO_NACC; ++k) hb[k] = 0.0;
    }
  } else {
    LoDevCtx cx{n, xy + b * HW * 2, xyz + b * HW * 3, ws + b * HW, LoCam{Kd[4 * b], Kd[4 * b + 1], Kd[4 * b + 2], Kd[4 * b + 3]}, sh};
    lo_run(cx, in, thr2, rounds, steps, out, &inl, &c, &st, tr, hb);
    if (st != 0) out = in;  // copied through bit for bit
  }
  if (tid == 0) {
    for (int k = 0; k < 9; ++k) R_out[9 * b + k] = out.R[k];
    for (int k = 0; k < 3; ++k) t_out[3 * b + k] = out.t[k];
    inliers[b] = inl;
    cost[b] = c;
    status[b] = st;
  }
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_pnp_lo_ws_bytes(int B, int HW) {
  if (B < 1 || B > 65535 || HW < 1 || HW > (1 << 24)) return -1;
  return (long long)B * HW;
}

extern "C" int zp_pnp_lo(int B, int HW, const int* counts, const int* xy, const float* xyz, const double* K,
                         const double* R, const double* t, const int* active, double reproj_err, int rounds, int steps,
                         double* R_out, double* t_out, int* inliers, double* cost, int* status, int* trace, double* Hb,
                         void* ws, void* stream) {
  ZP_CHECK_ARG(zp_pnp_lo_ws_bytes(B, HW) > 0, "zp_pnp_lo: sizes out of range: B %d, HW %d", B, HW);
  ZP_CHECK_ARG(rounds >= 1 && rounds <= 64 && steps >= 1 && steps <= 64, "zp_pnp_lo: rounds %d, steps %d must be 1..64",
               rounds, steps);
  ZP_CHECK_ARG(reproj_err > 0 && reproj_err < INFINITY, "zp_pnp_lo: reproj_err %g must be positive and finite",
               reproj_err);
  ZP_CHECK_ARG(counts && xy && xyz && K && R && t && R_out && t_out && inliers && cost && status && ws,
               "zp_pnp_lo: NULL pointer");
  ZP_CHECK_ARG(R != R_out && t != t_out, "zp_pnp_lo: the pose cannot be updated in place");
  hipLaunchKernelGGL(k_pnp_lo, dim3(B), dim3(LO_T), 0, (hipStream_t)stream, HW, counts, xy, xyz, K, R, t, active,
                     reproj_err * reproj_err, rounds, steps, R_out, t_out, inliers, cost, status, trace, Hb, (uint8_t*)ws);
  ZP_LAUNCH_CHECK("zp_pnp_lo");
  return ZP_OK;
}
