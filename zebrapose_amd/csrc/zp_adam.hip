// The Adam step on gfx950, op for op as torch.optim.Adam rounds it: one tensor per launch, many
// tensors per launch, and the capturable form whose step count lives on the device.
#include "zp_elem.h"

namespace zp {

// One element of torch.optim.Adam (_single_tensor_adam), each op rounded as torch's CPU build rounds it
// (tests/adam_ref.py restates it, pinned to torch bit for bit):
//   exp_avg.lerp_(grad, w1 = 1 - beta1)     ATen's lerp is one fma on (end - self):
//                                             w1 <  0.5: fma(w1, g - m, m);  w1 >= 0.5: fma(w1 - 1, g - m, g)
//   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = w2 = 1 - beta2)     fma(w2 * g, g, v * b2)
//   denom = exp_avg_sq.sqrt() / sqrt(bc2) + eps                             three roundings
//   param.addcdiv_(exp_avg, denom, value = -lr / bc1)                       p + (a * m) / denom, nothing fused
__device__ __forceinline__ void adam_elem(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, long long e, float lr_bc1, float w1, float b2, float w2,
                                          float bc2_sqrt, float eps) {
  const float gg = g[e];
  float mm = m[e];
  const float d = __fsub_rn(gg, mm);
  mm = w1 < 0.5f ? fmaf(w1, d, mm) : fmaf(__fsub_rn(w1, 1.f), d, gg);
  const float vv = fmaf(__fmul_rn(w2, gg), gg, __fmul_rn(v[e], b2));
  m[e] = mm;
  v[e] = vv;
  // sqrtf and / are the correctly rounded IEEE operations, denormals included (__fsqrt_rn is not: it is the
  // hardware's approximate root); the Makefile builds this file with -ffp-contract=off, so only the fmaf fuse
  const float denom = __fadd_rn(__fdiv_rn(sqrtf(vv), bc2_sqrt), eps);
  p[e] = __fadd_rn(p[e], __fdiv_rn(__fmul_rn(-lr_bc1, mm), denom));
}

__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                       long n, float lr_bc1, float w1, float b2, float w2, float bc2_sqrt, float eps) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x)
    adam_elem(p, g, m, v, e, lr_bc1, w1, b2, w2, bc2_sqrt, eps);
}

// multi-tensor Adam: one launch updates up to ADAM_MT tensors; the tensor of a block comes from
// the prefix sums of per-tensor block counts (ADAM_CHUNK elements per block)
constexpr int ADAM_MT = 40;
constexpr int ADAM_CHUNK = 4096;
struct AdamTable {
  float* p[ADAM_MT];
  const float* g[ADAM_MT];
  float* m[ADAM_MT];
  float* v[ADAM_MT];
  long long n[ADAM_MT];
  int blk0[ADAM_MT + 1];
  int count;
};

__global__ void __launch_bounds__(256) k_adam_multi(const AdamTable T, float lr_bc1, float w1, float b2, float w2,
                                                    float bc2_sqrt, float eps, const float* __restrict__ step_dev,
                                                    double lr, double beta1, double beta2) {
  if (step_dev) {
    // capturable form (zp_adam_multi_dev): the step count lives on the device, so a captured
    // graph replays with the current count; the host's double-precision bias corrections, per block
    const double st = (double)step_dev[0];
    lr_bc1 = (float)(lr / (1.0 - pow(beta1, st)));
    bc2_sqrt = (float)sqrt(1.0 - pow(beta2, st));
  }
  const int b = blockIdx.x;
  int lo = 0, hi = T.count - 1;  // last t with blk0[t] <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.blk0[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const int t = lo;
  const long long e0 = (long long)(b - T.blk0[t]) * ADAM_CHUNK;
  const long long e1 = min(T.n[t], e0 + ADAM_CHUNK);
  float* __restrict__ p = T.p[t];
  const float* __restrict__ g = T.g[t];
  float* __restrict__ m = T.m[t];
  float* __restrict__ v = T.v[t];
  for (long long e = e0 + threadIdx.x; e < e1; e += 256)  // the op sequence of k_adam
    adam_elem(p, g, m, v, e, lr_bc1, w1, b2, w2, bc2_sqrt, eps);
}

}  // namespace zp
using namespace zp;

extern "C" int zp_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr,
                       double beta1, double beta2, double eps, long long step, void* stream) {
  ZP_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n >= 0 && step >= 1, "zp_adam: bad args");
  if (n == 0) return ZP_OK;
  double bc1 = 1.0 - pow(beta1, (double)step);
  double bc2 = 1.0 - pow(beta2, (double)step);
  hipLaunchKernelGGL(k_adam, dim3(grid_for(n, 256, 16384)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, (long)n, (float)(lr / bc1), (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)sqrt(bc2), (float)eps);
  ZP_LAUNCH_CHECK("zp_adam");
  return ZP_OK;
}

static int adam_multi(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const long long* numel, double lr, double beta1, double beta2,
                      double eps, long long step, const float* step_dev, void* stream) {
  ZP_CHECK_ARG(count >= 0 && (count == 0 || (params && grads && exp_avg && exp_avg_sq && numel)) &&
                   (step >= 1 || step_dev),
               "zp_adam_multi: bad args");
  const double bc1 = step_dev ? 1.0 : 1.0 - pow(beta1, (double)step);
  const double bc2 = step_dev ? 1.0 : 1.0 - pow(beta2, (double)step);
  // each launch takes up to ADAM_MT non-empty tensors; the next launch starts where this one's scan
  // stopped (empty tensors are skipped, never counted twice)
  for (int t0 = 0; t0 < count;) {
    AdamTable T{};
    int nb = 0;
    T.count = 0;
    int t = t0;
    for (; t < count && T.count < ADAM_MT; ++t) {
      ZP_CHECK_ARG(numel[t] >= 0 && (numel[t] == 0 || (params[t] && grads[t] && exp_avg[t] && exp_avg_sq[t])),
                   "zp_adam_multi: tensor %d", t);
      if (numel[t] == 0) continue;
      const int k = T.count++;
      T.p[k] = params[t];
      T.g[k] = grads[t];
      T.m[k] = exp_avg[t];
      T.v[k] = exp_avg_sq[t];
      T.n[k] = numel[t];
      T.blk0[k] = nb;
      const long long blocks = (numel[t] + ADAM_CHUNK - 1) / ADAM_CHUNK;
      ZP_CHECK_ARG(nb + blocks < (1ll << 30), "zp_adam_multi: too many elements");
      nb += (int)blocks;
    }
    t0 = t;
    T.blk0[T.count] = nb;
    if (nb == 0) continue;
    hipLaunchKernelGGL(k_adam_multi, dim3(nb), dim3(256), 0, (hipStream_t)stream, T, (float)(lr / bc1),
                       (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(bc2), (float)eps,
                       step_dev, lr, beta1, beta2);
    ZP_LAUNCH_CHECK("zp_adam_multi");
  }
  return ZP_OK;
}

extern "C" int zp_adam_multi(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, const long long* numel, double lr, double beta1, double beta2,
                             double eps, long long step, void* stream) {
  return adam_multi(count, params, grads, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, step, nullptr, stream);
}

extern "C" int zp_adam_multi_dev(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                                 float* const* exp_avg_sq, const long long* numel, double lr, double beta1,
                                 double beta2, double eps, const float* step_dev, void* stream) {
  ZP_CHECK_ARG(step_dev, "zp_adam_multi_dev: step_dev");
  return adam_multi(count, params, grads, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, 0, step_dev, stream);
}
