// What the memory-bound .hip files (zp_pack, zp_bn, zp_pool, zp_glue, zp_adam) share: the 16-byte vector of an
// element type, the grid-stride grid size, the entry points' two dtype checks and their dtype dispatchers.
#pragma once
#include <math.h>
#include <type_traits>
#include "zp_common.h"

namespace zp {

// 16-byte vector of dtype T
template <typename T> struct V16;
template <> struct V16<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float* f) {
    uint4 u = *(const uint4*)p;
    uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(w[i] << 16);
      f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float* f) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(f[2 * i]) | ((uint32_t)f2bf(f[2 * i + 1]) << 16);
    *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <> struct V16<f16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const f16_t* p, float* f) {
    const f16x8 h = *(const f16x8*)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)h[i];
  }
  static __device__ __forceinline__ void store(f16_t* p, const float* f) {
    f16x8 h;
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = (f16_t)f[i];
    *(f16x8*)p = h;
  }
};
template <> struct V16<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float* f) {
    float4 v = *(const float4*)p;
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
  static __device__ __forceinline__ void store(float* p, const float* f) { *(float4*)p = make_float4(f[0], f[1], f[2], f[3]); }
};

static inline int grid_for(long n, int block = 256, int cap = 8192) {
  long g = (n + block - 1) / block;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}

// ZP_F16 is an inference dtype: accepted by the forward-path entry points, refused by the
// training-only ones (ZP_DTYPE_CHECK_TRAIN)
#define ZP_DTYPE_CHECK(fn, dt) \
  ZP_CHECK_ARG((dt) == ZP_F32 || (dt) == ZP_BF16 || (dt) == ZP_F16, fn ": bad dtype %d", (int)(dt))
#define ZP_DTYPE_CHECK_TRAIN(fn, dt) \
  ZP_CHECK_ARG((dt) == ZP_F32 || (dt) == ZP_BF16, fn ": dtype %d (fp16 is inference-only)", (int)(dt))

// The dispatchers hand the (already checked) dtype to a generic lambda as a tag, so each launch is written once:
//   by_dtype(dtype, [&](auto tag) { using T = typename decltype(tag)::type; ... k<T> ... (const T*)x ... });
template <typename T> struct ElemTag { using type = T; };

// {bf16, fp16, f32}: entry points guarded by ZP_DTYPE_CHECK
template <typename F> inline void by_dtype(int dt, F&& f) {
  if (dt == ZP_BF16) f(ElemTag<bf16_t>{});
  else if (dt == ZP_F16) f(ElemTag<f16_t>{});
  else f(ElemTag<float>{});
}

// {bf16, f32}: entry points guarded by ZP_DTYPE_CHECK_TRAIN
template <typename F> inline void by_train_dtype(int dt, F&& f) {
  if (dt == ZP_BF16) f(ElemTag<bf16_t>{});
  else f(ElemTag<float>{});
}

// the split-fp32 forms by plane count, tag.value: ZP_F32X3 -> 3, ZP_F32H2 -> 2
template <typename F> inline void by_planes(int dt, F&& f) {
  if (dt == ZP_F32X3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 2>{});
}

}  // namespace zp
