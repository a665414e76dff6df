// BatchNorm on gfx950 (NHWC, 16-byte vectorised): the eval-mode fold, the train-mode statistics merge
// (three variants) and apply (two), the backward reduce / totals / apply, and the key-15 tuning switch.
#include "zp_elem.h"

namespace zp {

// ------------------------------------------------------------------ batch norm
__global__ void k_bn_fold(const float* g, const float* b, const float* m, const float* v, const float* bias, float eps,
                          int C, float* scale, float* shift) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  // PyTorch CPU eval: alpha = weight / sqrt(var + eps); out = in * alpha + (bias - mean * alpha)
  float inv = 1.f / sqrtf(v[c] + eps);
  float s = g[c] * inv;
  float sh = b[c] - m[c] * s;
  if (bias) sh += bias[c] * s;
  scale[c] = s;
  shift[c] = sh;
}

// Level 1 of the statistics merge: block (channel group, j) merges parts [j*R, (j+1)*R) with
// Chan's formula (f64 inside the block) and writes the merged (count, mean, M2) back in place into
// part j*R -- only this block reads that range, so the in-place write is race-free.  Level 2
// (k_bn_train_finalize) then reads every R-th part.  Two levels keep both kernels short: the
// conv epilogue emits one part per wave-half (8192 parts at 128x128, bs 32).
constexpr int BN_MERGE_R = 64;
__global__ void k_bn_stat_merge(float* __restrict__ part, int parts, int C) {
  __shared__ double sh[3][8][33];
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int k0 = blockIdx.y * BN_MERGE_R, k1 = min(parts, k0 + BN_MERGE_R);
  double n = 0, s = 0;
  if (c < C)
    for (int k = k0 + pl; k < k1; k += 8) {
      double nk = part[(size_t)k * C + c];
      n += nk;
      s += nk * (double)part[((size_t)parts + k) * C + c];
    }
  sh[0][pl][cl] = n;
  sh[1][pl][cl] = s;
  __syncthreads();
  double ntot = 0, stot = 0;
  for (int k = 0; k < 8; ++k) {
    ntot += sh[0][k][cl];
    stot += sh[1][k][cl];
  }
  const double mean = ntot > 0 ? stot / ntot : 0.0;
  double q = 0;
  if (c < C)
    for (int k = k0 + pl; k < k1; k += 8) {
      double nk = part[(size_t)k * C + c];
      double dm = (double)part[((size_t)parts + k) * C + c] - mean;
      q += (double)part[((size_t)2 * parts + k) * C + c] + nk * dm * dm;
    }
  sh[2][pl][cl] = q;
  __syncthreads();  // every read of this range precedes the write-back below
  if (pl != 0 || c >= C) return;
  for (int k = 1; k < 8; ++k) q += sh[2][k][cl];
  part[(size_t)k0 * C + c] = (float)ntot;
  part[((size_t)parts + k0) * C + c] = (float)mean;
  part[((size_t)2 * parts + k0) * C + c] = (float)q;
}

// Level 2 (one block = 32 channels x 8 part lanes; reads parts 0, R, 2R, ... (R = stride)):
// partials [0] count, [1] mean, [2] M2 (centred) per part, merged with Chan's formula in f64:
// n = sum n_k, mean = sum n_k mean_k / n, M2 = sum M2_k + sum n_k (mean_k - mean)^2; then the
// train-mode scale / shift, the saved statistics and the running-statistics update
struct BnFin {
  float eps, mom;
  const float *gamma, *beta, *bias;
  float *rm, *rv;
  int64_t* nbt;
  float *scale, *shift, *save;
};
__device__ __forceinline__ void bn_finalize_block(const float* __restrict__ part, int parts, int stride, int C, int cgrp,
                                                  const BnFin& f, double (&sh)[3][8][33]) {
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int c = cgrp * 32 + cl;
  double n = 0, s = 0;
  if (c < C)
    for (int k = pl * stride; k < parts; k += 8 * stride) {
      double nk = part[(size_t)k * C + c];
      n += nk;
      s += nk * (double)part[((size_t)parts + k) * C + c];
    }
  sh[0][pl][cl] = n;
  sh[1][pl][cl] = s;
  __syncthreads();
  double ntot = 0, stot = 0;
  for (int k = 0; k < 8; ++k) {
    ntot += sh[0][k][cl];
    stot += sh[1][k][cl];
  }
  const double mean = ntot > 0 ? stot / ntot : 0.0;
  double q = 0;
  if (c < C)
    for (int k = pl * stride; k < parts; k += 8 * stride) {
      double nk = part[(size_t)k * C + c];
      double dm = (double)part[((size_t)parts + k) * C + c] - mean;
      q += (double)part[((size_t)2 * parts + k) * C + c] + nk * dm * dm;
    }
  sh[2][pl][cl] = q;
  __syncthreads();
  if (pl != 0 || c >= C) return;
  for (int k = 1; k < 8; ++k) q += sh[2][k][cl];
  const double cntd = ntot;
  double var = cntd > 0 ? q / cntd : 0.0;
  if (var < 0) var = 0;
  float invstd = (float)(1.0 / sqrt(var + (double)f.eps));
  float sc = f.gamma[c] * invstd;
  const float shv = __builtin_fmaf(-(float)mean, sc, f.beta[c]);
  f.scale[c] = sc;
  f.shift[c] = shv;
  f.save[c] = (float)mean;
  f.save[C + c] = invstd;
  f.save[2 * C + c] = sc;  // the backward recomputes the ReLU mask from the raw conv output
  f.save[3 * C + c] = shv;
  double mt = mean + (f.bias ? (double)f.bias[c] : 0.0);
  double unb = cntd > 1 ? var * cntd / (cntd - 1.0) : var;
  f.rm[c] = (float)((1.0 - f.mom) * f.rm[c] + f.mom * mt);
  f.rv[c] = (float)((1.0 - f.mom) * f.rv[c] + f.mom * unb);
  if (c == 0 && f.nbt) f.nbt[0] += 1;
}

__global__ void k_bn_train_finalize(const float* __restrict__ part, int parts, int stride, int C, const BnFin f) {
  __shared__ double sh[3][8][33];
  bn_finalize_block(part, parts, stride, C, blockIdx.x, f, sh);
}

// Levels 1 and 2 in one launch (round 5; VERDICT r4 #4: the training step ran ~55 merge + ~55
// finalize launches of 5-7 us).  Block (channel group x, part range y) merges its range in place as
// k_bn_stat_merge does; then the blocks of a channel group hand off through an agent-scope counter
// (cdna_hip_programming.md Guideline 16, counter form: every wave drains its stores, the block's
// barrier, one lane's release fence + drain, relaxed agent fetch_add); the block that draws the last
// ticket acquires (fence, drain, barrier) and runs level 2 over the merged parts, then re-arms the
// counter for the next launch.  Correct for any placement of the blocks over XCDs; the parts are
// merged in the same fixed order as the two-launch form, so results are bit-identical to it.
__global__ void __launch_bounds__(256) k_bn_stat_merge_fin(float* __restrict__ part, int parts, int C,
                                                           unsigned* __restrict__ cnt, const BnFin f) {
  __shared__ double sh[3][8][33];
  __shared__ int last;
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int k0 = blockIdx.y * BN_MERGE_R, k1 = min(parts, k0 + BN_MERGE_R);
  double n = 0, s = 0;
  if (c < C)
    for (int k = k0 + pl; k < k1; k += 8) {
      double nk = part[(size_t)k * C + c];
      n += nk;
      s += nk * (double)part[((size_t)parts + k) * C + c];
    }
  sh[0][pl][cl] = n;
  sh[1][pl][cl] = s;
  __syncthreads();
  double ntot = 0, stot = 0;
  for (int k = 0; k < 8; ++k) {
    ntot += sh[0][k][cl];
    stot += sh[1][k][cl];
  }
  const double mean = ntot > 0 ? stot / ntot : 0.0;
  double q = 0;
  if (c < C)
    for (int k = k0 + pl; k < k1; k += 8) {
      double nk = part[(size_t)k * C + c];
      double dm = (double)part[((size_t)parts + k) * C + c] - mean;
      q += (double)part[((size_t)2 * parts + k) * C + c] + nk * dm * dm;
    }
  sh[2][pl][cl] = q;
  __syncthreads();  // every read of this range precedes the write-back below
  if (pl == 0 && c < C) {
    for (int k = 1; k < 8; ++k) q += sh[2][k][cl];
    part[(size_t)k0 * C + c] = (float)ntot;
    part[((size_t)parts + k0) * C + c] = (float)mean;
    part[((size_t)2 * parts + k0) * C + c] = (float)q;
  }
  // hand-off: publish this block's merged part, count it; the last block of the group continues
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned prev = __hip_atomic_fetch_add(cnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int l = prev == gridDim.y - 1;
    if (l) {
      __hip_atomic_store(cnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    last = l;
  }
  __syncthreads();
  if (!last) return;
  bn_finalize_block(part, parts, BN_MERGE_R, C, blockIdx.x, f, sh);
}

// One level for up to BN_MERGE1_MAX parts (round 5; with the strip tile's per-tile parts most layers
// of the bs 32 training step have 128): block = 8 channels x 128 part lanes, a lane's (at most 4) parts loaded once; the two passes of
// Chan's merge (n, sum n_k mean_k -> mean; sum M2_k + n_k (mean_k - mean)^2) read registers, each
// followed by a fixed pairwise tree over the 128 lanes in f64 (deterministic); then the finalize of
// bn_finalize_block.  One launch without the two-level form's counter hand-off, whose release /
// acquire fences and two dependent global passes per level held every merge near 10 us.
constexpr int BN_MERGE1_MAX = 512;
__global__ void __launch_bounds__(1024) k_bn_stat_merge1(const float* __restrict__ part, int parts, int C, const BnFin f) {
  __shared__ double sh[2][128][9];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + cl;
  constexpr int U = BN_MERGE1_MAX / 128;
  float pn[U], pm[U], pq[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k = pl + 128 * u;
    const bool in = c < C && k < parts;
    pn[u] = in ? part[(size_t)k * C + c] : 0.f;
    pm[u] = in ? part[((size_t)parts + k) * C + c] : 0.f;
    pq[u] = in ? part[((size_t)2 * parts + k) * C + c] : 0.f;
  }
  double n = 0, s = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    n += (double)pn[u];
    s += (double)pn[u] * (double)pm[u];
  }
  sh[0][pl][cl] = n;
  sh[1][pl][cl] = s;
  __syncthreads();
  for (int w = 64; w > 0; w >>= 1) {
    if (pl < w) {
      sh[0][pl][cl] += sh[0][pl + w][cl];
      sh[1][pl][cl] += sh[1][pl + w][cl];
    }
    __syncthreads();
  }
  const double ntot = sh[0][0][cl], stot = sh[1][0][cl];
  const double mean = ntot > 0 ? stot / ntot : 0.0;
  double q = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const double dm = (double)pm[u] - mean;
    q += (double)pq[u] + (double)pn[u] * dm * dm;  // (parts past the end: all three zero)
  }
  __syncthreads();  // every lane has read the pass-1 totals
  sh[0][pl][cl] = q;
  __syncthreads();
  for (int w = 64; w > 0; w >>= 1) {
    if (pl < w) sh[0][pl][cl] += sh[0][pl + w][cl];
    __syncthreads();
  }
  if (pl != 0 || c >= C) return;
  q = sh[0][0][cl];
  const double cntd = ntot;
  double var = cntd > 0 ? q / cntd : 0.0;
  if (var < 0) var = 0;
  float invstd = (float)(1.0 / sqrt(var + (double)f.eps));
  float sc = f.gamma[c] * invstd;
  const float shv = __builtin_fmaf(-(float)mean, sc, f.beta[c]);
  f.scale[c] = sc;
  f.shift[c] = shv;
  f.save[c] = (float)mean;
  f.save[C + c] = invstd;
  f.save[2 * C + c] = sc;
  f.save[3 * C + c] = shv;
  double mt = mean + (f.bias ? (double)f.bias[c] : 0.0);
  double unb = cntd > 1 ? var * cntd / (cntd - 1.0) : var;
  f.rm[c] = (float)((1.0 - f.mom) * f.rm[c] + f.mom * mt);
  f.rv[c] = (float)((1.0 - f.mom) * f.rv[c] + f.mom * unb);
  if (c == 0 && f.nbt) f.nbt[0] += 1;
}

// the fused merge's hand-off counters (one per channel group) live in the caller's partials buffer,
// past the [3][parts][C] statistics (ABI 4, zp_bn_finalize_floats), and are zeroed on the launch's
// stream before the merge: every launch has its own, whatever stream or hipGraph it runs in (ADVICE
// r5: one static array per device was shared by concurrent launches on different streams)
static int g_bn_fused = -1;  // zp_conv_tuning key 15: 1 the one-launch merge, 0 two launches (-1: ZP_BN_FUSED or 1)
int bn_fused_mode(int v) {
  const int old = g_bn_fused;
  g_bn_fused = v;
  return old;
}

// N consecutive per-channel floats (16-byte aligned: c and C are multiples of N)
template <int N>
__device__ __forceinline__ void load_chan(const float* __restrict__ p, float* v) {
#pragma unroll
  for (int i = 0; i < N; i += 4) {
    const float4 q = *(const float4*)(p + i);
    v[i] = q.x;
    v[i + 1] = q.y;
    v[i + 2] = q.z;
    v[i + 3] = q.w;
  }
}

// Pixel-row tiling of the per-pixel BN passes: block = 256 threads = lanes (16-byte channel chunks,
// at most 256) x R pixel rows; blockIdx.y = channel group.  A thread keeps one channel chunk, so its
// per-channel terms are loaded once, and walks K = pix / R pixels in batches of 4 with every load
// of a batch issued before any use.
struct BnTile {
  int lanes, R, cgroups, pix, blocks;
};
static inline BnTile bn_tile(long P, int C, int N, long min_blocks = 2048) {  // k_bn_bwd_apply
  BnTile t;
  const int CV = C / N;
  t.lanes = CV < 256 ? CV : 256;
  t.R = 256 / t.lanes;
  t.cgroups = CV > 256 ? CV / 256 : 1;
  int K = 16;  // pixels per thread: fewer (down to 4) while that leaves fewer than min_blocks blocks
  while (K > 4 && ((P + (long)t.R * K - 1) / ((long)t.R * K)) * t.cgroups < min_blocks) K >>= 1;
  t.pix = t.R * K;
  t.blocks = (int)((P + t.pix - 1) / t.pix);
  return t;
}

template <typename T>
__global__ void k_bn_apply(const T* __restrict__ x, long P, int C, const float* __restrict__ scale,
                           const float* __restrict__ shift, const T* __restrict__ res, int ldr, int cr0, int relu,
                           T* __restrict__ y, int ldy, int cy0) {
  // grid-stride over 16-byte chunks (measured faster here than bn_tile's pixel-row tiling)
  constexpr int N = V16<T>::N;
  const int CV = C / N;
  const long total = P * CV;
  int cur = -1;  // channel chunk whose scale / shift are in registers (16-byte loads)
  float sc[N], sh[N];
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long p = e / CV;
    int c = (int)(e - p * CV) * N;
    float v[N], r[N];
    V16<T>::load(x + p * C + c, v);
    if (res) V16<T>::load(res + p * ldr + cr0 + c, r);
    if (c != cur) {
      cur = c;
      load_chan<N>(scale + c, sc);
      load_chan<N>(shift + c, sh);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float o = __builtin_fmaf(v[i], sc[i], sh[i]);  // the backward's mask (relu mode 2) repeats this
      if (res) o += r[i];
      if (relu) o = fmaxf(o, 0.f);
      v[i] = o;
    }
    V16<T>::store(y + p * ldy + cy0 + c, v);
  }
}

// (round 5) the same pass with U chunks per thread in flight and 32-bit shift indexing, for C/N a
// power of two dividing 256: a block's chunk runs start at multiples of 256, so a thread's channel
// chunk is fixed (tid mod C/N) and its scale / shift are loaded once
template <typename T, int U>
__global__ void __launch_bounds__(256) k_bn_apply_u(const T* __restrict__ x, unsigned total, int cvs, int C,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    const T* __restrict__ res, int ldr, int cr0, int relu,
                                                    T* __restrict__ y, int ldy, int cy0) {
  constexpr int N = V16<T>::N;
  const unsigned tid = threadIdx.x;
  const int c = (int)(tid & ((1u << cvs) - 1u)) * N;
  float sc[N], sh[N];
  load_chan<N>(scale + c, sc);
  load_chan<N>(shift + c, sh);
  for (unsigned base = blockIdx.x * 256u * U; base < total; base += gridDim.x * 256u * U) {
    float v[U][N], r[U][N];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const unsigned e = base + k * 256u + tid;
      if (e < total) {
        const unsigned p = e >> cvs;
        V16<T>::load(x + (size_t)p * C + c, v[k]);
        if (res) V16<T>::load(res + (size_t)p * ldr + cr0 + c, r[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const unsigned e = base + k * 256u + tid;
      if (e >= total) break;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float o = __builtin_fmaf(v[k][i], sc[i], sh[i]);
        if (res) o += r[k][i];
        if (relu) o = fmaxf(o, 0.f);
        v[k][i] = o;
      }
      V16<T>::store(y + (size_t)(e >> cvs) * ldy + cy0 + c, v[k]);
    }
  }
}

// Pixels per partial slot of the backward reduction: 16 pixel rows per thread row, fewer (down to
// 4) while that leaves fewer than 512 slots -- 32x32 layers at 256-512 channels would otherwise
// run on 64 workgroups (more slots make the totals pass, which reads every slot, the slower one).  Rows per block assume 16-byte bf16 lanes (C/8 lanes, at most 256); any
// multiple of the kernel's row count works, the fp32 kernel included.
static inline int bn_bwd_pix(int P, int C) {
  const int lanes = C / 8 < 256 ? (C / 8 > 0 ? C / 8 : 1) : 256;
  const int R = 256 / lanes > 0 ? 256 / lanes : 1;
  int rows = 16;
  // large layers (up2 at bs 32: 4096 slots at 16 rows): up to 64 rows while >= 1024 slots remain --
  // fewer partials for the totals pass to read
  while (rows < 64 && (P + R * rows * 2 - 1) / (R * rows * 2) >= 1024) rows <<= 1;
  while (rows > 4 && (P + R * rows - 1) / (R * rows) < 512) rows >>= 1;
  return R * rows;
}

// block: 256 threads = (C/N) chunk lanes x R rows.  MODE: ReLU mask source (0 none, 1 the stored
// activation y, 2 recomputed from the raw x); HX: x given (sum g*xhat as well).  Templated so each
// instance holds only the registers its streams need (the runtime-mode kernel spilled at 128 VGPRs).
template <typename T, int MODE, bool HX>
__global__ void __launch_bounds__(256) k_bn_bwd_reduce(const T* __restrict__ dy, int lddy, int cdy0,
                                                       const T* __restrict__ y, int ldy, int cy0,
                                                       const T* __restrict__ x, long P, int C,
                                                       const float* __restrict__ save, float* __restrict__ part,
                                                       int parts, int pix) {
  constexpr int N = V16<T>::N;
  static_assert(MODE != 2 || HX, "mask from raw needs x");
  __shared__ float red[2][256][N];
  const int CV = C / N;
  const int lanes = CV < 256 ? CV : 256;  // chunk lanes per row
  const int R = 256 / lanes;
  const int cgi = blockIdx.y;
  const int cl = threadIdx.x % lanes, row = threadIdx.x / lanes;
  const int c = (cgi * lanes + cl) * N;
  const long p0 = (long)blockIdx.x * pix;
  const long p1 = min(P, p0 + pix);
  float sg[N], sgx[N], mean[N], inv[N], msc[N], msh[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    sg[i] = sgx[i] = 0.f;
    mean[i] = (HX && c < C) ? save[c + i] : 0.f;
    inv[i] = (HX && c < C) ? save[C + c + i] : 0.f;
    msc[i] = (MODE == 2 && c < C) ? save[2 * C + c + i] : 0.f;
    msh[i] = (MODE == 2 && c < C) ? save[3 * C + c + i] : 0.f;
  }
  if (row < R && c < C) {
    // U pixels per iteration with all loads issued before any use: the loop is otherwise
    // latency-bound (one dependent HBM round trip per pixel row)
    constexpr int U = 4;  // pixels in flight per thread (the pixel count per thread, pix / R, is 4, 8 or 16)
    auto body = [&](const uint4& gd, const uint4& yd, const uint4& xd, bool ok) {
      float g[N], yy[N], xx[N];
      V16<T>::load((const T*)&gd, g);
#pragma unroll
      for (int i = 0; i < N; ++i) g[i] = ok ? g[i] : 0.f;
      if (MODE == 1) {
        V16<T>::load((const T*)&yd, yy);
#pragma unroll
        for (int i = 0; i < N; ++i) g[i] = yy[i] > 0.f ? g[i] : 0.f;
      }
      if (HX) {
        V16<T>::load((const T*)&xd, xx);
        if (MODE == 2)
#pragma unroll
          for (int i = 0; i < N; ++i) g[i] = __builtin_fmaf(xx[i], msc[i], msh[i]) > 0.f ? g[i] : 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) sgx[i] += g[i] * (xx[i] - mean[i]) * inv[i];
      }
#pragma unroll
      for (int i = 0; i < N; ++i) sg[i] += g[i];
    };
    // batches of U rows with every load issued before any use; rows past the end load the last
    // row again (clamped address) and contribute zero
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (long pb = p0 + row; pb < p1; pb += U * R) {
      uint4 gd[U], yd[U], xd[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long pp = min(pb + u * R, p1 - 1);
        gd[u] = *(const uint4*)(dy + pp * lddy + cdy0 + c);
        yd[u] = MODE == 1 ? *(const uint4*)(y + pp * ldy + cy0 + c) : z;
        xd[u] = HX ? *(const uint4*)(x + pp * C + c) : z;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) body(gd[u], yd[u], xd[u], pb + u * R < p1);
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    red[0][threadIdx.x][i] = sg[i];
    red[1][threadIdx.x][i] = sgx[i];
  }
  __syncthreads();
  if (row == 0 && c < C) {
    for (int r = 1; r < R; ++r)
#pragma unroll
      for (int i = 0; i < N; ++i) {
        sg[i] += red[0][r * lanes + cl][i];
        sgx[i] += red[1][r * lanes + cl][i];
      }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      part[(size_t)blockIdx.x * C + c + i] = sg[i];
      part[((size_t)(parts + 1) + blockIdx.x) * C + c + i] = sgx[i];
    }
  }
}

// totals over parts -> part[0][parts][c], part[1][parts][c]; dgamma / dbeta
// block = 8 channels x 128 part lanes (1024 threads; C / 8 blocks: 8 for a 64-channel BN, where the
// former 32 x 32 layout ran 2 blocks for the whole GPU); each lane sums its parts (4 loads per
// stream in flight), then a fixed pairwise tree over the 128 lanes (deterministic)
// oparts: the totals go to rows oparts of both halves (the [2][oparts + 1][C] layout zp_bn_bwd_apply
// reads; oparts != parts after a zp_conv2d launch with bnr_part) -- only this block touches channel c,
// and it writes after every read of its parts
__global__ void __launch_bounds__(1024) k_bn_bwd_totals(float* __restrict__ part, int parts, int C, float* dgamma,
                                                        float* dbeta, int accumulate, int oparts) {
  __shared__ double sh[2][128][9];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + cl;
  double s = 0, q = 0;
  if (c < C)
    for (int k0 = pl; k0 < parts; k0 += 128 * 4) {
      // clamped, unconditional loads: no branch between them
      float a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = min(k0 + 128 * u, parts - 1);
        a[u] = part[(size_t)k * C + c];
        b[u] = part[((size_t)parts + 1 + k) * C + c];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = k0 + 128 * u < parts;
        s += in ? (double)a[u] : 0.0;
        q += in ? (double)b[u] : 0.0;
      }
    }
  sh[0][pl][cl] = s;
  sh[1][pl][cl] = q;
  __syncthreads();
  for (int w = 64; w > 0; w >>= 1) {
    if (pl < w) {
      sh[0][pl][cl] += sh[0][pl + w][cl];
      sh[1][pl][cl] += sh[1][pl + w][cl];
    }
    __syncthreads();
  }
  if (pl != 0 || c >= C) return;
  s = sh[0][0][cl];
  q = sh[1][0][cl];
  part[(size_t)oparts * C + c] = (float)s;
  part[((size_t)oparts + 1 + oparts) * C + c] = (float)q;
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)q : (float)q;
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)s : (float)s;
}

template <typename T, int relu>
__global__ void __launch_bounds__(256) k_bn_bwd_apply(const T* __restrict__ dy, int lddy, int cdy0,
                                                      const T* __restrict__ y, int ldy, int cy0,
                                                      const T* __restrict__ x, long P, int C,
                                                      const float* __restrict__ save, const float* __restrict__ part,
                                                      int parts, const float* __restrict__ gamma, T* __restrict__ dx,
                                                      T* __restrict__ dres, int lddres, int cdres0, int racc, int pix) {
  // pixel-row tiling (bn_tile)
  constexpr int N = V16<T>::N;
  constexpr int U = 4;
  const int CV = C / N;
  const int lanes = CV < 256 ? CV : 256;
  const int R = 256 / lanes;
  const int cl = threadIdx.x % lanes, row = threadIdx.x / lanes;
  const int c = (blockIdx.y * lanes + cl) * N;
  if (row >= R || c >= C) return;
  const long p0 = (long)blockIdx.x * pix;
  const long p1 = min(P, p0 + pix);
  const float invP = 1.f / (float)P;
  float mean[N], inv[N], sg[N], sgx[N], gm[N], msc[N], msh[N];
  if (dx) {
    load_chan<N>(save + c, mean);
    load_chan<N>(save + C + c, inv);
    if (relu == 2) {
      load_chan<N>(save + 2 * C + c, msc);
      load_chan<N>(save + 3 * C + c, msh);
    }
    load_chan<N>(part + (size_t)parts * C + c, sg);
    load_chan<N>(part + ((size_t)parts + 1 + parts) * C + c, sgx);
    load_chan<N>(gamma + c, gm);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      sg[i] *= invP;
      sgx[i] *= invP;
    }
  }
  // optional streams loaded under their (uniform) condition and read only under it -- a select
  // between the stream and a zero constant made the compiler load through a pointer select of
  // global and private memory (flat loads, a 32-byte private segment)
  const bool hx = dx != nullptr, hr = dres != nullptr && racc;
  for (long pb = p0 + row; pb < p1; pb += U * R) {
    uint4 gd[U], yd[U], xd[U], rd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long pp = min(pb + u * R, p1 - 1);
      gd[u] = *(const uint4*)(dy + pp * lddy + cdy0 + c);
      if constexpr (relu == 1) yd[u] = *(const uint4*)(y + pp * ldy + cy0 + c);
      if (hx) xd[u] = *(const uint4*)(x + pp * C + c);
      if (hr) rd[u] = *(const uint4*)(dres + pp * lddres + cdres0 + c);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long p = pb + u * R;
      if (p >= p1) break;
      float g[N], yy[N], xx[N], o[N];
      V16<T>::load((const T*)&gd[u], g);
      if (relu == 1) {
        V16<T>::load((const T*)&yd[u], yy);
#pragma unroll
        for (int i = 0; i < N; ++i) g[i] = yy[i] > 0.f ? g[i] : 0.f;
      }
      if (dx) {
        V16<T>::load((const T*)&xd[u], xx);
        if (relu == 2)
#pragma unroll
          for (int i = 0; i < N; ++i) g[i] = __builtin_fmaf(xx[i], msc[i], msh[i]) > 0.f ? g[i] : 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          float xh = (xx[i] - mean[i]) * inv[i];
          o[i] = gm[i] * inv[i] * (g[i] - sg[i] - xh * sgx[i]);
        }
        V16<T>::store(dx + p * C + c, o);
      }
      if (dres) {
        T* d = dres + p * lddres + cdres0 + c;
        if (racc) {
          float r[N];
          V16<T>::load((const T*)&rd[u], r);
#pragma unroll
          for (int i = 0; i < N; ++i) r[i] += g[i];
          V16<T>::store(d, r);
        } else {
          V16<T>::store(d, g);
        }
      }
    }
  }
}

}  // namespace zp
using namespace zp;

extern "C" long long zp_bn_finalize_floats(int parts, int C) {
  if (parts <= 0 || C <= 0) return 0;
  return 3LL * parts * C + (C + 31) / 32;  // statistics + the one-launch merge's counters (ABI 4)
}

extern "C" int zp_bn_fold(const float* g, const float* b, const float* m, const float* v, const float* bias, float eps,
                          int C, float* scale, float* shift, void* stream) {
  ZP_CHECK_ARG(g && b && m && v && scale && shift && C > 0, "zp_bn_fold: bad args");
  hipLaunchKernelGGL(k_bn_fold, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, b, m, v, bias, eps, C,
                     scale, shift);
  ZP_LAUNCH_CHECK("zp_bn_fold");
  return ZP_OK;
}

extern "C" int zp_bn_train_finalize(float* partials, int parts, int C, long long count, float eps, float momentum,
                                    const float* gamma, const float* beta, const float* conv_bias, float* running_mean,
                                    float* running_var, int64_t* nbt, float* scale, float* shift, float* save,
                                    void* stream) {
  ZP_CHECK_ARG(partials && gamma && beta && running_mean && running_var && scale && shift && save && parts > 0 &&
                   C > 0 && count > 0,
               "zp_bn_train_finalize: bad args");
  // count is only required to be positive: the merged count is the sum of the parts' own counts
  // (comparing the two would take a device read inside the training step)
  const BnFin f{eps, momentum, gamma, beta, conv_bias, running_mean, running_var, nbt, scale, shift, save};
  hipStream_t st = (hipStream_t)stream;
  // the partials buffer is the caller's scratch (zp_conv2d stats): level 1 merges in place
  if (parts <= BN_MERGE1_MAX) {  // (both key-15 modes: one level, one launch)
    hipLaunchKernelGGL(k_bn_stat_merge1, dim3((C + 7) / 8), dim3(1024), 0, st, partials, parts, C, f);
    ZP_LAUNCH_CHECK("zp_bn_train_finalize (one level)");
    return ZP_OK;
  }
  // more than BN_MERGE1_MAX (> 2 * BN_MERGE_R) parts: always two levels
  const int groups = (C + 31) / 32;
  static const int env = getenv("ZP_BN_FUSED") ? atoi(getenv("ZP_BN_FUSED")) : 1;
  const bool fused_on = (g_bn_fused >= 0 ? g_bn_fused : env) != 0;
  if (fused_on) {
    unsigned* cnt = (unsigned*)(partials + (size_t)3 * parts * C);
    if (hipMemsetAsync(cnt, 0, (size_t)groups * sizeof(unsigned), st) != hipSuccess) {
      set_error("zp_bn_train_finalize: counter reset failed");
      return ZP_ERR_HIP;
    }
    hipLaunchKernelGGL(k_bn_stat_merge_fin, dim3(groups, (parts + BN_MERGE_R - 1) / BN_MERGE_R), dim3(256), 0, st,
                       partials, parts, C, cnt, f);
    ZP_LAUNCH_CHECK("zp_bn_train_finalize (fused merge)");
    return ZP_OK;
  }
  hipLaunchKernelGGL(k_bn_stat_merge, dim3(groups, (parts + BN_MERGE_R - 1) / BN_MERGE_R), dim3(256), 0, st, partials,
                     parts, C);
  ZP_LAUNCH_CHECK("zp_bn_train_finalize merge");
  hipLaunchKernelGGL(k_bn_train_finalize, dim3(groups), dim3(256), 0, st, partials, parts, BN_MERGE_R, C, f);
  ZP_LAUNCH_CHECK("zp_bn_train_finalize");
  return ZP_OK;
}

extern "C" int zp_bn_apply(const void* x, int P, int C, const float* scale, const float* shift, const void* res, int ldr,
                           int cr0, int relu, int dtype, void* y, int ldy, int cy0, void* stream) {
  ZP_DTYPE_CHECK("zp_bn_apply", dtype);
  const int N = dtype == ZP_F32 ? 4 : 8;
  ZP_CHECK_ARG(x && y && scale && shift && P > 0 && C % N == 0 && ldy % N == 0 && cy0 % N == 0,
               "zp_bn_apply: bad args");
  if (res) ZP_CHECK_ARG(ldr % N == 0 && cr0 % N == 0, "zp_bn_apply: residual alignment");
  long total = (long)P * (C / N);
  const int CV = C / N;
  const char* ev = getenv("ZP_BN_APPLY_U");  // A/B knob (0: the grid-stride kernel), read per call
  const int use_u = ev ? atoi(ev) : 1;
  hipStream_t st = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (use_u && (CV & (CV - 1)) == 0 && 256 % CV == 0 && total < (1L << 31) - (1L << 20)) {
      constexpr int U = 4;
      const int cvs = __builtin_ctz((unsigned)CV);
      long g = (total + 256L * U - 1) / (256L * U);
      const dim3 grid((unsigned)(g > 65535 ? 65535 : g));
      hipLaunchKernelGGL((k_bn_apply_u<T, U>), grid, dim3(256), 0, st, (const T*)x, (unsigned)total, cvs, C, scale,
                         shift, (const T*)res, ldr, cr0, relu, (T*)y, ldy, cy0);
    } else {
      hipLaunchKernelGGL(k_bn_apply<T>, dim3(grid_for(total)), dim3(256), 0, st, (const T*)x, (long)P, C, scale, shift,
                         (const T*)res, ldr, cr0, relu, (T*)y, ldy, cy0);
    }
  });
  ZP_LAUNCH_CHECK("zp_bn_apply");
  return ZP_OK;
}

extern "C" int zp_bn_bwd_parts(int P, int C) {
  const int pix = bn_bwd_pix(P, C);
  return (P + pix - 1) / pix;
}

extern "C" int zp_bn_bwd_reduce(const void* dy, int lddy, int cdy0, const void* y, int ldy, int cy0, const void* x, int P,
                                int C, const float* save, int relu, int dtype, float* partials, float* dgamma,
                                float* dbeta, int accumulate, void* stream) {
  ZP_DTYPE_CHECK_TRAIN("zp_bn_bwd_reduce", dtype);
  const int N = dtype == ZP_F32 ? 4 : 8;
  ZP_CHECK_ARG(dy && partials && P > 0 && C % N == 0 && relu >= 0 && relu <= 2 && (relu != 1 || y) &&
                   (relu != 2 || x) && (!x || save),
               "zp_bn_bwd_reduce: bad args");
  ZP_CHECK_ARG(C / N <= 256 || (C / N) % 256 == 0, "zp_bn_bwd_reduce: C %d", C);
  // 16-byte loads at dy + p * lddy + cdy0 + c (and at y, where the mask reads it)
  ZP_CHECK_ARG(lddy % N == 0 && cdy0 % N == 0 && (relu != 1 || (ldy % N == 0 && cy0 % N == 0)),
               "zp_bn_bwd_reduce: slice alignment");
  const int parts = zp_bn_bwd_parts(P, C);
  const int CV = C / N;
  const int cgroups = CV > 256 ? CV / 256 : 1;
  const int pix = bn_bwd_pix(P, C);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(parts, cgroups);
  by_train_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto kernel = k_bn_bwd_reduce<T, 0, false>;  // the instance for the mask source and whether x is given
    if (relu == 2) kernel = k_bn_bwd_reduce<T, 2, true>;
    else if (relu == 1) kernel = x ? k_bn_bwd_reduce<T, 1, true> : k_bn_bwd_reduce<T, 1, false>;
    else if (x) kernel = k_bn_bwd_reduce<T, 0, true>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const T*)dy, lddy, cdy0, (const T*)y, ldy, cy0, (const T*)x,
                       (long)P, C, save, partials, parts, pix);
  });
  ZP_LAUNCH_CHECK("zp_bn_bwd_reduce");
  hipLaunchKernelGGL(k_bn_bwd_totals, dim3((C + 7) / 8), dim3(1024), 0, st, partials, parts, C, dgamma, dbeta,
                     accumulate, parts);
  ZP_LAUNCH_CHECK("zp_bn_bwd_reduce totals");
  return ZP_OK;
}

extern "C" int zp_bn_bwd_totals(float* partials, int parts, int C, int out_parts, float* dgamma, float* dbeta,
                                int accumulate, void* stream) {
  ZP_CHECK_ARG(partials && parts > 0 && out_parts > 0 && C > 0, "zp_bn_bwd_totals: bad args");
  hipLaunchKernelGGL(k_bn_bwd_totals, dim3((C + 7) / 8), dim3(1024), 0, (hipStream_t)stream, partials, parts, C,
                     dgamma, dbeta, accumulate, out_parts);
  ZP_LAUNCH_CHECK("zp_bn_bwd_totals");
  return ZP_OK;
}

extern "C" int zp_bn_bwd_apply(const void* dy, int lddy, int cdy0, const void* y, int ldy, int cy0, const void* x, int P,
                               int C, const float* save, const float* partials, const float* gamma, int relu, int dtype,
                               void* dx, void* dres, int lddres, int cdres0, int res_accumulate, void* stream) {
  ZP_DTYPE_CHECK_TRAIN("zp_bn_bwd_apply", dtype);
  const int N = dtype == ZP_F32 ? 4 : 8;
  ZP_CHECK_ARG(dy && P > 0 && C % N == 0 && relu >= 0 && relu <= 2 && (relu != 1 || y) && (relu != 2 || dx) &&
                   (!dx || (x && save && partials && gamma)),
               "zp_bn_bwd_apply: bad args");
  ZP_CHECK_ARG(C / N <= 256 || (C / N) % 256 == 0, "zp_bn_bwd_apply: C %d", C);
  // 16-byte loads / stores at dy, y (where the mask reads it) and dres
  ZP_CHECK_ARG(lddy % N == 0 && cdy0 % N == 0 && (relu != 1 || (ldy % N == 0 && cy0 % N == 0)) &&
                   (!dres || (lddres % N == 0 && cdres0 % N == 0)),
               "zp_bn_bwd_apply: slice alignment");
  const int parts = zp_bn_bwd_parts(P, C);
  const BnTile t = bn_tile(P, C, N);
  const dim3 grid(t.blocks, t.cgroups);
  hipStream_t st = (hipStream_t)stream;
  by_train_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto kernel = k_bn_bwd_apply<T, 0>;  // the instance for the mask source
    if (relu == 2) kernel = k_bn_bwd_apply<T, 2>;
    else if (relu == 1) kernel = k_bn_bwd_apply<T, 1>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const T*)dy, lddy, cdy0, (const T*)y, ldy, cy0, (const T*)x,
                       (long)P, C, save, partials, parts, gamma, (T*)dx, (T*)dres, lddres, cdres0, res_accumulate,
                       t.pix);
  });
  ZP_LAUNCH_CHECK("zp_bn_bwd_apply");
  return ZP_OK;
}
