// Weight packing on gfx950: a checkpoint's f32 conv weights into the padded [rows_pad][k_pad] operand
// of the conv kernels, in any compute dtype or split-fp32 form; one job per launch or many.
#include "zp_elem.h"

namespace zp {

// ------------------------------------------------------------------ weight packing
struct PackArgs {
  const float* src;
  void* dst;
  int d0, d1, kh, kw, transposed, ntaps, cstride, rows_pad, k_pad;
  signed char ky[ZP_MAX_TAPS], kx[ZP_MAX_TAPS];
};

template <typename T>
__global__ void k_pack(const PackArgs a) {
  const long total = (long)a.rows_pad * a.k_pad;
  const int rows = a.transposed ? a.d1 : a.d0;
  const int chans = a.transposed ? a.d0 : a.d1;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int r = (int)(e / a.k_pad), k = (int)(e - (long)r * a.k_pad);
    int t = k / a.cstride, c = k - t * a.cstride;
    float v = 0.f;
    if (r < rows && t < a.ntaps && c < chans) {
      int ky = a.ky[t], kx = a.kx[t];
      size_t idx = a.transposed ? (((size_t)c * a.d1 + r) * a.kh + ky) * a.kw + kx
                                : (((size_t)r * a.d1 + c) * a.kh + ky) * a.kw + kx;
      v = a.src[idx];
    }
    ((T*)a.dst)[e] = Elem<T>::cvt(v);
  }
}

// split-fp32 packing (ZP_F32X3 / ZP_F32H2): the same element map as k_pack, the f32 weight split
// into NPL planes [NPL][rows_pad][k_pad] (SplitF32<NPL>)
template <int NPL>
__global__ void k_pack_split(const PackArgs a, unsigned* rflag) {
  const long total = (long)a.rows_pad * a.k_pad;
  bool bad = false;
  const int rows = a.transposed ? a.d1 : a.d0;
  const int chans = a.transposed ? a.d0 : a.d1;
  unsigned short* d = (unsigned short*)a.dst;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    int r = (int)(e / a.k_pad), k = (int)(e - (long)r * a.k_pad);
    int t = k / a.cstride, c = k - t * a.cstride;
    float v = 0.f;
    if (r < rows && t < a.ntaps && c < chans) {
      int ky = a.ky[t], kx = a.kx[t];
      size_t idx = a.transposed ? (((size_t)c * a.d1 + r) * a.kh + ky) * a.kw + kx
                                : (((size_t)r * a.d1 + c) * a.kh + ky) * a.kw + kx;
      v = a.src[idx];
    }
    unsigned short q[NPL];
    SplitF32<NPL>::split(v, q);
    if constexpr (NPL == 2) bad |= h2w_overflow(v);
#pragma unroll
    for (int p = 0; p < NPL; ++p) d[e + p * total] = q[p];
  }
  if constexpr (NPL == 2) raise_range_flag(rflag, bad);
}

// one launch for many pack jobs: blockIdx.y = job (read once, uniform), threads over the job's
// (row, channel) pairs; each thread reads its pair's kh x kw taps (contiguous in the checkpoint
// layout, so a wave reads one contiguous span) and writes them at k = t * cstride + c (adjacent
// threads -> adjacent k: coalesced 2-byte stores), then the pair's share of the k_pad tail (zeros).
// Same result as zp_pack_weight per job.
__device__ __forceinline__ void pack_store(const zp_pack_job& a, int d, float v, unsigned* rflag) {
  if (a.dtype == ZP_F32X3) {  // three planes of rows_pad * k_pad
    const size_t ps = (size_t)a.rows_pad * a.k_pad;
    unsigned short q[3];
    SplitF32<3>::split(v, q);
    for (int p = 0; p < 3; ++p) ((unsigned short*)a.dst)[d + p * ps] = q[p];
  } else if (a.dtype == ZP_F32H2) {  // two planes
    const size_t ps = (size_t)a.rows_pad * a.k_pad;
    unsigned short q[2];
    SplitF32<2>::split(v, q);
    for (int p = 0; p < 2; ++p) ((unsigned short*)a.dst)[d + p * ps] = q[p];
    raise_range_flag(rflag, h2w_overflow(v));
  } else if (a.dtype == ZP_BF16) ((bf16_t*)a.dst)[d] = f2bf(v);
  else if (a.dtype == ZP_F16) ((f16_t*)a.dst)[d] = (f16_t)v;
  else ((float*)a.dst)[d] = v;
}

// Tiled form for kh x kw <= 9 (every job but the 7x7 stem): a block stages a tile of PK_R packed
// rows x PK_C channels x the kh*kw taps in LDS with reads contiguous in the checkpoint layout (rows
// of [c][tap] for a forward packing, [r][tap] runs per channel for a transposed / data-gradient one),
// then writes each packed row's (tap, channel) run as consecutive 2-byte stores.  The per-pair form
// below it read the transposed layouts one scattered 36-byte run per lane (r02 PMC: 1.3 GB moved per
// 116 MB of weights).
constexpr int PK_R = 8, PK_C = 64, PK_ROW = PK_C * 9 + 1;  // +1: the transposed fill hits distinct banks
// KHW / NT: the job's kh * kw and tap count as compile-time constants (9 / 9: a full 3x3 forward packing;
// 9 / -9: the reversed taps of a 3x3 data-gradient packing; 1 / 1: the 1x1s), or 0 for the runtime
// values (ConvT phase sub-problems); with them a tile's loads are all issued before its LDS writes
// (one memory round trip per tile instead of one per element batch)
template <int KHW, int NT>
__device__ __forceinline__ void pack_tiled(const zp_pack_job& a, const int* toff, float* tile, unsigned* rflag) {
  const int rows = a.transposed ? a.d1 : a.d0;
  const int chans = a.transposed ? a.d0 : a.d1;
  const int khw = KHW ? KHW : a.kh * a.kw;
  const int ntaps = NT > 0 ? NT : (NT < 0 ? -NT : a.ntaps);
  const int ct = (a.cstride + PK_C - 1) / PK_C, rt = (a.rows_pad + PK_R - 1) / PK_R;
  const int kt = ntaps * a.cstride, nld = PK_R * PK_C * khw;
  for (int tl = blockIdx.x; tl < rt * ct; tl += gridDim.x) {
    const int r0 = (tl / ct) * PK_R, c0 = (tl % ct) * PK_C;
    auto elem = [&](int e, int& li) -> float {  // source element e of the tile -> its value, LDS index
      const int k = e % khw, q = e / khw;
      int rl, cl;
      if (a.transposed) {  // src[c][r][tap]: runs of consecutive r per channel
        rl = q % PK_R;
        cl = q / PK_R;
      } else {  // src[r][c][tap]: runs of consecutive c per row
        cl = q % PK_C;
        rl = q / PK_C;
      }
      const int r = r0 + rl, c = c0 + cl;
      li = rl * PK_ROW + cl * 9 + k;
      return (r < rows && c < chans) ? a.src[(a.transposed ? ((size_t)c * a.d1 + r) : ((size_t)r * a.d1 + c)) * khw + k]
                                     : 0.f;
    };
    if constexpr (KHW > 0) {
      constexpr int PER = (PK_R * PK_C * KHW + 255) / 256;
      float v[PER];
      int li[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int e = threadIdx.x + 256 * u;
        v[u] = e < nld ? elem(e, li[u]) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < PER; ++u)
        if (threadIdx.x + 256 * u < nld) tile[li[u]] = v[u];
    } else {
      for (int e = threadIdx.x; e < nld; e += blockDim.x) {
        int li;
        const float v = elem(e, li);
        tile[li] = v;
      }
    }
    __syncthreads();
    const int cw = min(PK_C, a.cstride - c0);
    for (int e = threadIdx.x; e < PK_R * ntaps * PK_C; e += blockDim.x) {
      const int cl = e % PK_C, q = e / PK_C, t = q % ntaps, rl = q / ntaps;
      const int r = r0 + rl;
      const int tk = NT == 9 && KHW == 9 ? t : (NT == -9 && KHW == 9 ? 8 - t : (NT == 1 && KHW == 1 ? 0 : toff[t]));
      if (cl < cw && r < a.rows_pad) pack_store(a, r * a.k_pad + t * a.cstride + c0 + cl, tile[rl * PK_ROW + cl * 9 + tk], rflag);
    }
    if (c0 == 0)  // the row's k_pad tail
      for (int e = threadIdx.x; e < PK_R * (a.k_pad - kt); e += blockDim.x) {
        const int rl = e / (a.k_pad - kt), kk = kt + e % (a.k_pad - kt);
        if (r0 + rl < a.rows_pad) pack_store(a, (r0 + rl) * a.k_pad + kk, 0.f, rflag);
      }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_pack_multi(const zp_pack_job* __restrict__ jobs, unsigned* rflag, int forms) {
  const zp_pack_job& a = jobs[blockIdx.y];
  // tap offsets in LDS (a private copy of the job's tap arrays would live in scratch)
  __shared__ int toff[ZP_MAX_TAPS];
  __shared__ float tile[PK_R * PK_ROW];
  if ((int)threadIdx.x < a.ntaps) toff[threadIdx.x] = a.ky[threadIdx.x] * a.kw + a.kx[threadIdx.x];
  __syncthreads();
  const int rows = a.transposed ? a.d1 : a.d0;
  const int chans = a.transposed ? a.d0 : a.d1;
  if (a.kh * a.kw <= 9) {
    bool ident = true, rev = true;
    for (int t = 0; t < a.ntaps; ++t) {
      ident = ident && a.ky[t] * a.kw + a.kx[t] == t;
      rev = rev && a.ky[t] * a.kw + a.kx[t] == a.ntaps - 1 - t;
    }
    if (!forms) pack_tiled<0, 0>(a, toff, tile, rflag);  // (A/B: ZP_PACK_FORMS=0)
    else if (ident && a.kh * a.kw == 9 && a.ntaps == 9) pack_tiled<9, 9>(a, toff, tile, rflag);
    else if (rev && a.kh * a.kw == 9 && a.ntaps == 9) pack_tiled<9, -9>(a, toff, tile, rflag);
    else if (ident && a.kh * a.kw == 1 && a.ntaps == 1) pack_tiled<1, 1>(a, toff, tile, rflag);
    else pack_tiled<0, 0>(a, toff, tile, rflag);
    return;
  }
  const int pairs = a.rows_pad * a.cstride;
  const int kt = a.ntaps * a.cstride, khw = a.kh * a.kw;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < pairs; q += gridDim.x * blockDim.x) {
    const int r = q / a.cstride, c = q - r * a.cstride;
    const bool live = r < rows && c < chans;
    const float* sp = a.src + (a.transposed ? ((size_t)c * a.d1 + r) : ((size_t)r * a.d1 + c)) * khw;
    const int o = r * a.k_pad + c;
    if (a.ntaps <= 9) {  // all loads in flight before the stores
      float v[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) v[t] = (live && t < a.ntaps) ? sp[toff[t]] : 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (t < a.ntaps) pack_store(a, o + t * a.cstride, v[t], rflag);
    } else {
      for (int t = 0; t < a.ntaps; ++t) pack_store(a, o + t * a.cstride, live ? sp[toff[t]] : 0.f, rflag);
    }
    for (int kk = kt + c; kk < a.k_pad; kk += a.cstride) pack_store(a, r * a.k_pad + kk, 0.f, rflag);
  }
}

}  // namespace zp
using namespace zp;

extern "C" int zp_conv_rows_pad(int Cout) {
  int tc = Cout > 64 ? 128 : (Cout > 32 ? 64 : 32);
  return (Cout + tc - 1) / tc * tc;
}

extern "C" int zp_pack_weight(const float* src, int d0, int d1, int kh, int kw, int transposed, int ntaps, const int* ky,
                              const int* kx, int cstride, int dtype, void* dst, int rows_pad, int k_pad, void* stream) {
  ZP_CHECK_ARG(dtype == ZP_F32 || dtype == ZP_BF16 || dtype == ZP_F16 || dtype == ZP_F32X3 || dtype == ZP_F32H2,
               "zp_pack_weight: bad dtype %d", dtype);
  ZP_CHECK_ARG(src && dst && ky && kx, "zp_pack_weight: null pointer");
  ZP_CHECK_ARG(ntaps >= 1 && ntaps <= ZP_MAX_TAPS, "zp_pack_weight: ntaps %d", ntaps);
  ZP_CHECK_ARG(cstride >= (transposed ? d0 : d1) && (long)ntaps * cstride <= k_pad, "zp_pack_weight: cstride/k_pad");
  ZP_CHECK_ARG(rows_pad >= (transposed ? d1 : d0), "zp_pack_weight: rows_pad");
  PackArgs a;
  a.src = src; a.dst = dst; a.d0 = d0; a.d1 = d1; a.kh = kh; a.kw = kw; a.transposed = transposed;
  a.ntaps = ntaps; a.cstride = cstride; a.rows_pad = rows_pad; a.k_pad = k_pad;
  for (int t = 0; t < ntaps; ++t) {
    ZP_CHECK_ARG(ky[t] >= 0 && ky[t] < kh && kx[t] >= 0 && kx[t] < kw, "zp_pack_weight: tap %d out of range", t);
    a.ky[t] = (signed char)ky[t];
    a.kx[t] = (signed char)kx[t];
  }
  const dim3 grid(grid_for((long)rows_pad * k_pad));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == ZP_F32X3 || dtype == ZP_F32H2)
    by_planes(dtype, [&](auto npl) {
      hipLaunchKernelGGL(k_pack_split<npl.value>, grid, dim3(256), 0, st, a, npl.value == 2 ? range_flag() : nullptr);
    });
  else
    by_dtype(dtype, [&](auto tag) { hipLaunchKernelGGL(k_pack<typename decltype(tag)::type>, grid, dim3(256), 0, st, a); });
  ZP_LAUNCH_CHECK("zp_pack_weight");
  return ZP_OK;
}

extern "C" int zp_pack_weight_multi(int n, const zp_pack_job* jobs, const long long* prefix, long long total,
                                    void* stream) {
  ZP_CHECK_ARG(n >= 0 && n <= 65535 && total >= 0 && total < (1ll << 40) && (n == 0 || (jobs && prefix)),
               "zp_pack_weight_multi: bad args");
  if (n == 0 || total == 0) return ZP_OK;
  // blocks per job, each walking the job's 8-row x 64-channel tiles: 64 measured best of 32 / 64 / 128
  // / 256 on the training step's ~100 jobs (256: 170 us, most blocks of the small jobs empty; 64: 134
  // us; a flat tile space over all jobs, blocks scanning the jobs' tile counts, ran 228 us at 172
  // VGPRs); ZP_PACK_GX for A/B
  static const int gx = getenv("ZP_PACK_GX") ? atoi(getenv("ZP_PACK_GX")) : 64;
  static const int forms = getenv("ZP_PACK_FORMS") ? atoi(getenv("ZP_PACK_FORMS")) : 1;
  hipLaunchKernelGGL(k_pack_multi, dim3(gx > 0 ? gx : 64, n), dim3(256), 0, (hipStream_t)stream, jobs, range_flag(),
                     forms);
  ZP_LAUNCH_CHECK("zp_pack_weight_multi");
  return ZP_OK;
}
