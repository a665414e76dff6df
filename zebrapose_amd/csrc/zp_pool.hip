// Layout conversion and pooling on gfx950: NCHW -> NHWC, the split-fp32 stem im2col, the 3x3 / s2 max
// pool forward and backward, the global average pool, the H*W sums and broadcasts (plain and split-plane).
#include "zp_elem.h"

namespace zp {

// ------------------------------------------------------------------ layout / pooling
template <typename T>
__global__ void k_nchw_to_nhwc(const float* __restrict__ x, int B, int C, int H, int W, int cpad, T* __restrict__ y) {
  constexpr int N = V16<T>::N;
  const long HW = (long)H * W, total = (long)B * HW;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long b = e / HW, s = e - b * HW;
    T* o = y + e * cpad;
    if (cpad % N == 0) {  // one 16 B store per N channels (the network's input: 3 -> 8 bf16 = one store)
      for (int c0 = 0; c0 < cpad; c0 += N) {
        float v[N];
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = c0 + i < C ? x[(b * C + c0 + i) * HW + s] : 0.f;
        V16<T>::store(o + c0, v);
      }
    } else {
      for (int c = 0; c < cpad; ++c) o[c] = Elem<T>::cvt(c < C ? x[(b * C + c) * HW + s] : 0.f);
    }
  }
}

template <typename T>
__global__ void k_maxpool(const T* __restrict__ x, int B, int IH, int IW, int ldx, int cx0, int C, T* __restrict__ y,
                          int OH, int OW, int ldy, int cy0) {
  constexpr int N = V16<T>::N;
  const int CV = C / N;
  const long total = (long)B * OH * OW * CV;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long pix = e / CV;
    int c = (int)(e - pix * CV) * N;
    int ox = (int)(pix % OW);
    long t = pix / OW;
    int oy = (int)(t % OH), b = (int)(t / OH);
    float m[N];
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
      int iy = oy * 2 - 1 + ky;
      if ((unsigned)iy >= (unsigned)IH) continue;
      for (int kx = 0; kx < 3; ++kx) {
        int ix = ox * 2 - 1 + kx;
        if ((unsigned)ix >= (unsigned)IW) continue;
        float v[N];
        V16<T>::load(x + (((size_t)b * IH + iy) * IW + ix) * ldx + cx0 + c, v);
#pragma unroll
        for (int i = 0; i < N; ++i)
          if (v[i] > m[i] || isnan(v[i])) m[i] = v[i];  // PyTorch CPU max_pool2d rule
      }
    }
    V16<T>::store(y + pix * ldy + cy0 + c, m);
  }
}

// Split-fp32 stem im2col (zp_im2col_split): thread per (output pixel, 8-element chunk of the
// kpad-long patch row); taps gathered from the f32 NHWC image (L2-resident: each input pixel is
// read by <= 16 overlapping 7x7 / s2 windows), each element split into the NPL planes
template <int NPL>
__global__ void k_im2col_split(const float* __restrict__ x, int B, int H, int W, int ldx, int C, int k, int s, int p,
                               int OH, int OW, int kpad, unsigned short* __restrict__ y, unsigned* rflag) {
  const int KC = kpad / 8, KK = k * k * C;
  bool bad = false;
  const long total = (long)B * OH * OW * KC;
  const long plane = (long)B * OH * OW * kpad;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long pix = e / KC;
    const int kc = (int)(e - pix * KC);
    const int ox = (int)(pix % OW);
    const long t = pix / OW;
    const int oy = (int)(t % OH), b = (int)(t / OH);
    uint32_t w[NPL][4];
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
      unsigned short q[2][NPL];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int kk = kc * 8 + i + h;
        float v = 0.f;
        if (kk < KK) {
          const int tap = kk / C, c = kk - tap * C;
          const int ky = tap / k, kx = tap - ky * k;
          const int iy = oy * s - p + ky, ix = ox * s - p + kx;
          if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = x[(((long)b * H + iy) * W + ix) * ldx + c];
        }
        SplitF32<NPL>::split(v, q[h]);
        if constexpr (NPL == 2) bad |= h2_overflow(v);
      }
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) w[pl][i >> 1] = (uint32_t)q[0][pl] | ((uint32_t)q[1][pl] << 16);
    }
    unsigned short* yo = y + pix * kpad + kc * 8;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) *(uint4*)(yo + pl * plane) = make_uint4(w[pl][0], w[pl][1], w[pl][2], w[pl][3]);
  }
  if constexpr (NPL == 2) raise_range_flag(rflag, bad);
}

// Split-fp32 max pool (NPL planes, SplitF32<NPL>): the 3x3 window max of the joined f32 values
// (PyTorch CPU rule), stored split again (joining is exact, so the winner's value is reproduced
// exactly).  Planes: x + p * psx, y + p * psy.
template <int NPL>
__global__ void k_maxpool_split(const unsigned short* __restrict__ x, long psx, int B, int IH, int IW, int ldx, int cx0,
                                int C, unsigned short* __restrict__ y, long psy, int OH, int OW, int ldy, int cy0) {
  const int CV = C / 8;
  const long total = (long)B * OH * OW * CV;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long pix = e / CV;
    int c = (int)(e - pix * CV) * 8;
    int ox = (int)(pix % OW);
    long t = pix / OW;
    int oy = (int)(t % OH), b = (int)(t / OH);
    float m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
      int iy = oy * 2 - 1 + ky;
      if ((unsigned)iy >= (unsigned)IH) continue;
      for (int kx = 0; kx < 3; ++kx) {
        int ix = ox * 2 - 1 + kx;
        if ((unsigned)ix >= (unsigned)IW) continue;
        const size_t o = (((size_t)b * IH + iy) * IW + ix) * ldx + cx0 + c;
        uint32_t w[NPL][4];
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
          const uint4 q = *(const uint4*)(x + o + p * psx);
          w[p][0] = q.x;
          w[p][1] = q.y;
          w[p][2] = q.z;
          w[p][3] = q.w;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int s = (i & 1) * 16;
          unsigned short q[NPL];
#pragma unroll
          for (int p = 0; p < NPL; ++p) q[p] = (unsigned short)(w[p][i >> 1] >> s);
          const float v = SplitF32<NPL>::join(q);
          if (v > m[i] || isnan(v)) m[i] = v;
        }
      }
    }
    uint32_t o[NPL][4];
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
      unsigned short q0[NPL], q1[NPL];
      SplitF32<NPL>::split(m[i], q0);
      SplitF32<NPL>::split(m[i + 1], q1);
#pragma unroll
      for (int p = 0; p < NPL; ++p) o[p][i >> 1] = (uint32_t)q0[p] | ((uint32_t)q1[p] << 16);
    }
    unsigned short* yo = y + pix * ldy + cy0 + c;
#pragma unroll
    for (int p = 0; p < NPL; ++p) *(uint4*)(yo + p * psy) = make_uint4(o[p][0], o[p][1], o[p][2], o[p][3]);
  }
}

// Split-fp32 global average pool: block = (64 channels, image b); the joined values summed in
// double (CPU adaptive_avg_pool2d's accumulator) over 4 pixel lanes, combined in a fixed order; the
// f32 mean stored split into y [NPL][B][C]
template <int NPL>
__global__ void __launch_bounds__(256) k_avgpool_split(const unsigned short* __restrict__ x, long psx, int H, int W,
                                                       int ldx, int cx0, int C, unsigned short* __restrict__ y,
                                                       long psy) {
  __shared__ double red[4][64];
  const int b = blockIdx.y;
  const long HW = (long)H * W;
  const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s = 0.0;
  if (c < C)
    for (long p = sl; p < HW; p += 4) {
      const size_t o = ((size_t)b * HW + p) * ldx + cx0 + c;
      unsigned short q[NPL];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) q[pl] = x[o + pl * psx];
      s += (double)SplitF32<NPL>::join(q);
    }
  red[sl][cl] = s;
  __syncthreads();
  if (threadIdx.x < 64 && c < C) {
    const double t = red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl];
    unsigned short q[NPL];
    SplitF32<NPL>::split((float)(t / (double)HW), q);
    const size_t o = (size_t)b * C + c;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) y[o + pl * psy] = q[pl];
  }
}

// Split-fp32 global average pool, vectorised: block = (64 channels, image b), 256 threads = 8
// channel vectors (8 channels, 16 B per plane) x 32 pixel lanes; each thread sums every 32nd pixel
// in double (four pixels' loads in flight), the 32 lane sums meet in LDS in a fixed order.  Same
// sums as k_avgpool_split up to the (double) association; 16 B loads instead of 2 B
// (r03: k_avgpool_split read 67 MB in 71 us, 0.94 TB/s).
template <int NPL>
__global__ void __launch_bounds__(256) k_avgpool_split8(const unsigned short* __restrict__ x, long psx, int H, int W,
                                                        int ldx, int cx0, int C, unsigned short* __restrict__ y,
                                                        long psy) {
  __shared__ double red[32][65];
  const int b = blockIdx.y;
  const int HW = H * W;
  const int cv = threadIdx.x & 7, pl0 = threadIdx.x >> 3;
  const int c = blockIdx.x * 64 + cv * 8;
  double s[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) s[r] = 0.0;
  if (c < C) {
    const unsigned short* xb = x + (size_t)b * HW * ldx + cx0 + c;
    int p = pl0;
    for (; p + 96 < HW; p += 128) {
      uint4 q[4][NPL];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) q[u][pl] = *(const uint4*)(xb + (size_t)(p + 32 * u) * ldx + pl * psx);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          unsigned short h[NPL];
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) {
            const uint32_t w4[4] = {q[u][pl].x, q[u][pl].y, q[u][pl].z, q[u][pl].w};
            h[pl] = (unsigned short)(w4[r >> 1] >> ((r & 1) * 16));
          }
          s[r] += (double)SplitF32<NPL>::join(h);
        }
      }
    }
    for (; p < HW; p += 32) {
      uint4 q[NPL];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) q[pl] = *(const uint4*)(xb + (size_t)p * ldx + pl * psx);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        unsigned short h[NPL];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
          const uint32_t w4[4] = {q[pl].x, q[pl].y, q[pl].z, q[pl].w};
          h[pl] = (unsigned short)(w4[r >> 1] >> ((r & 1) * 16));
        }
        s[r] += (double)SplitF32<NPL>::join(h);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) red[pl0][cv * 8 + r] = s[r];
  __syncthreads();
  if (threadIdx.x < 64 && blockIdx.x * 64 + (int)threadIdx.x < C) {
    double t = 0.0;
    for (int k = 0; k < 32; ++k) t += red[k][threadIdx.x];
    unsigned short q[NPL];
    SplitF32<NPL>::split((float)(t / (double)HW), q);
    const size_t o = (size_t)b * C + blockIdx.x * 64 + threadIdx.x;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) y[o + pl * psy] = q[pl];
  }
}

// Window (oy, ox) of the 3x3 / stride-2 / pad-1 pool: per channel, the tap (ky*3+kx, -1 when the
// window lies outside the output) of its first maximum in (ky, kx) scan order (PyTorch CPU rule:
// `>` or NaN, the index starting at the window's first in-bounds tap, so a window of -inf alone sends
// its gradient there) and the window's dy.
template <typename T>
__device__ __forceinline__ void mp_window(const T* __restrict__ x, int ldx, int cx0, const T* __restrict__ dy,
                                          int lddy, int cdy0, int b, int c, int IH, int IW, int OH, int OW, int oy,
                                          int ox, int* pos, float* g) {
  constexpr int N = V16<T>::N;
#pragma unroll
  for (int i = 0; i < N; ++i) pos[i] = -1;
  if (oy >= OH || ox >= OW) return;
  float m[N];
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = -INFINITY;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = oy * 2 - 1 + ky;
    if ((unsigned)yy >= (unsigned)IH) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = ox * 2 - 1 + kx;
      if ((unsigned)xx >= (unsigned)IW) continue;
      float v[N];
      V16<T>::load(x + (((size_t)b * IH + yy) * IW + xx) * ldx + cx0 + c, v);
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (v[i] > m[i] || isnan(v[i]) || pos[i] < 0) {
          m[i] = v[i];
          pos[i] = ky * 3 + kx;
        }
    }
  }
  V16<T>::load(dy + (((size_t)b * OH + oy) * OW + ox) * lddy + cdy0 + c, g);
}

// Backward of the 3x3 / stride-2 / pad-1 max pool, gather form without atomics.  A thread owns the
// 2x2 input block (rows 2k, 2k+1; cols 2j, 2j+1) for one 16-byte channel vector, over a chunk of
// MP_ROWS consecutive k.  Row 2k lies only in window row k, row 2k+1 in window rows k and k+1 (same
// for columns), so the block needs windows (k|k+1, j|j+1); the k+1 pair is carried to the next k,
// i.e. two windows (18 loads) per block instead of a window walk per input pixel.  Contributions are
// added in (oy, ox) order, then the existing dx when accumulating.
constexpr int MP_ROWS = 4;
template <typename T>
__global__ void __launch_bounds__(256) k_maxpool_bwd(const T* __restrict__ x, int ldx, int cx0,
                                                     const T* __restrict__ dy, int lddy, int cdy0, int B, int IH,
                                                     int IW, int C, int OH, int OW, T* __restrict__ dx, int lddx,
                                                     int cdx0, int accumulate) {
  constexpr int N = V16<T>::N;
  const int CV = C / N, JP = (IW + 1) / 2, KP = (IH + 1) / 2, KC = (KP + MP_ROWS - 1) / MP_ROWS;
  const long total = (long)B * KC * JP * CV;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % CV) * N;
    long t = e / CV;
    const int j = (int)(t % JP);
    t /= JP;
    const int kc = (int)(t % KC), b = (int)(t / KC);
    const int k0 = kc * MP_ROWS, k1 = min(k0 + MP_ROWS, KP);
    int p00[N], p01[N], p10[N], p11[N];
    float g00[N], g01[N], g10[N], g11[N];
    mp_window(x, ldx, cx0, dy, lddy, cdy0, b, c, IH, IW, OH, OW, k0, j, p00, g00);
    mp_window(x, ldx, cx0, dy, lddy, cdy0, b, c, IH, IW, OH, OW, k0, j + 1, p01, g01);
    for (int k = k0; k < k1; ++k) {
      mp_window(x, ldx, cx0, dy, lddy, cdy0, b, c, IH, IW, OH, OW, k + 1, j, p10, g10);
      mp_window(x, ldx, cx0, dy, lddy, cdy0, b, c, IH, IW, OH, OW, k + 1, j + 1, p11, g11);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int iy = 2 * k + (q >> 1), ix = 2 * j + (q & 1);
        if (iy >= IH || ix >= IW) continue;
        float acc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
          float a = 0.f;
          // taps of (iy, ix) in windows (k, j), (k, j+1), (k+1, j), (k+1, j+1)
          if (q == 0) {
            if (p00[i] == 4) a += g00[i];
          } else if (q == 1) {
            if (p00[i] == 5) a += g00[i];
            if (p01[i] == 3) a += g01[i];
          } else if (q == 2) {
            if (p00[i] == 7) a += g00[i];
            if (p10[i] == 1) a += g10[i];
          } else {
            if (p00[i] == 8) a += g00[i];
            if (p01[i] == 6) a += g01[i];
            if (p10[i] == 2) a += g10[i];
            if (p11[i] == 0) a += g11[i];
          }
          acc[i] = a;
        }
        T* o = dx + (((size_t)b * IH + iy) * IW + ix) * lddx + cdx0 + c;
        if (accumulate) {
          float r[N];
          V16<T>::load(o, r);
#pragma unroll
          for (int i = 0; i < N; ++i) acc[i] += r[i];
        }
        V16<T>::store(o, acc);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
        p00[i] = p10[i];
        g00[i] = g10[i];
        p01[i] = p11[i];
        g01[i] = g11[i];
      }
    }
  }
}

// Per-channel sums over H*W: block = (image b, 64 channels), 256 threads = 64 channels x 4 pixel
// slices (coalesced 64-channel rows), slices combined through LDS in a fixed order.
template <typename T, typename ACC>
__device__ __forceinline__ ACC sum_hw_block(const T* __restrict__ x, long HW, int ld, int c0, int C, int b) {
  __shared__ ACC red[4][64];
  const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  ACC s = 0;
  if (c < C)
    for (long p = sl; p < HW; p += 4) s += (ACC)Elem<T>::ld(x + ((size_t)b * HW + p) * ld + c0 + c);
  red[sl][cl] = s;
  __syncthreads();
  return red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl];
}

// Vectorised form (C, c0, ld multiples of the 16 B vector width N): block = (image b, 64
// channels), 256 threads = (64 / N) chunk lanes x (256 N / 64) pixel lanes, 16 B loads; the pixel
// lanes are combined through LDS in a fixed order (deterministic).  MODE 0: mean over H*W in
// double, converted to T (CPU adaptive_avg_pool2d accumulates in double); MODE 1: float sum -> T.
template <typename T, int MODE>
__global__ void __launch_bounds__(256) k_hw_reduce_vec(const T* __restrict__ x, int H, int W, int ld, int c0, int C,
                                                       T* __restrict__ y) {
  constexpr int N = V16<T>::N;
  constexpr int CL = 64 / N, PL = 256 / CL;
  using ACC = typename std::conditional<MODE == 0, double, float>::type;
  __shared__ ACC red[PL][64];
  const int b = blockIdx.y;
  const long HW = (long)H * W;
  const int cl = threadIdx.x % CL, pl = threadIdx.x / CL;
  const int c = blockIdx.x * 64 + cl * N;
  ACC s[N];
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = 0;
  if (c < C) {
    const T* base = x + (size_t)b * HW * ld + c0 + c;
    long p = pl;
    for (; p + 3 * PL < HW; p += 4 * PL) {
      uint4 u[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = *(const uint4*)(base + (p + k * PL) * ld);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float v[N];
        V16<T>::load((const T*)&u[k], v);
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] += (ACC)v[i];
      }
    }
    for (; p < HW; p += PL) {
      float v[N];
      V16<T>::load(base + p * ld, v);
#pragma unroll
      for (int i = 0; i < N; ++i) s[i] += (ACC)v[i];
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) red[pl][cl * N + i] = s[i];
  __syncthreads();
  if (threadIdx.x < 64) {
    const int cc = blockIdx.x * 64 + threadIdx.x;
    ACC t = 0;
    for (int k = 0; k < PL; ++k) t += red[k][threadIdx.x];
    if (cc < C) {
      if (MODE == 0) y[(size_t)b * C + cc] = Elem<T>::cvt((float)((double)t / (double)HW));
      else y[(size_t)b * C + cc] = Elem<T>::cvt((float)t);
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) k_avgpool(const T* __restrict__ x, int H, int W, int ldx, int cx0, int C,
                                                 T* __restrict__ y) {
  const int b = blockIdx.y;
  const long HW = (long)H * W;
  // CPU adaptive_avg_pool2d accumulates in acc_type<float> = double
  double s = sum_hw_block<T, double>(x, HW, ldx, cx0, C, b);
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  if (threadIdx.x < 64 && c < C) y[(size_t)b * C + c] = Elem<T>::cvt((float)(s / (double)HW));
}

template <typename T>
__global__ void __launch_bounds__(256) k_sum_hw(const T* __restrict__ dy, int H, int W, int lddy, int cdy0, int C,
                                                T* __restrict__ out) {
  const int b = blockIdx.y;
  float s = sum_hw_block<T, float>(dy, (long)H * W, lddy, cdy0, C, b);
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  if (threadIdx.x < 64 && c < C) out[(size_t)b * C + c] = Elem<T>::cvt(s);
}

// y[b, p, cy0 + c] = src[b, c] for every pixel, one 16 B store per N channels (C, ldy, cy0
// multiples of N)
template <typename T>
__global__ void k_broadcast_vec(const T* __restrict__ src, int B, int C, T* __restrict__ y, int H, int W, int ldy,
                                int cy0) {
  constexpr int N = V16<T>::N;
  const int CV = C / N;
  const long HW = (long)H * W, total = (long)B * HW * CV;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long pix = e / CV;
    const int c = (int)(e - pix * CV) * N;
    const long b = pix / HW;
    *(uint4*)(y + pix * ldy + cy0 + c) = *(const uint4*)(src + b * C + c);
  }
}

template <typename T>
__global__ void k_broadcast(const T* __restrict__ src, int B, int C, float mul, T* __restrict__ y, int H, int W, int ldy,
                            int cy0, int accumulate, int convert) {
  const long HW = (long)H * W, total = (long)B * HW * C;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long pix = e / C;
    int c = (int)(e - pix * C);
    long b = pix / HW;
    T* o = y + pix * ldy + cy0 + c;
    if (!convert) {
      *o = src[b * C + c];
    } else {
      float v = Elem<T>::ld(src + b * C + c) * mul;
      if (accumulate) v += Elem<T>::ld(o);
      *o = Elem<T>::cvt(v);
    }
  }
}

}  // namespace zp
using namespace zp;

extern "C" int zp_im2col_split(const float* x, int B, int H, int W, int ldx, int C, int k, int s, int p, int OH,
                               int OW, int kpad, int dtype, void* y, void* stream) {
  ZP_CHECK_ARG(dtype == ZP_F32X3 || dtype == ZP_F32H2, "zp_im2col_split: dtype %d is not a split-fp32 form", dtype);
  ZP_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && C > 0 && ldx >= C && k > 0 && s > 0 && p >= 0 && OH > 0 &&
                   OW > 0 && kpad % 8 == 0 && kpad >= k * k * C,
               "zp_im2col_split: bad args");
  const long total = (long)B * OH * OW * (kpad / 8);
  by_planes(dtype, [&](auto npl) {
    hipLaunchKernelGGL(k_im2col_split<npl.value>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, B, H, W,
                       ldx, C, k, s, p, OH, OW, kpad, (unsigned short*)y, npl.value == 2 ? range_flag() : nullptr);
  });
  ZP_LAUNCH_CHECK("zp_im2col_split");
  return ZP_OK;
}

extern "C" int zp_nchw_to_nhwc(const float* x, int B, int C, int H, int W, int cpad, int dtype, void* y, void* stream) {
  ZP_DTYPE_CHECK("zp_nchw_to_nhwc", dtype);
  ZP_CHECK_ARG(x && y && B > 0 && C > 0 && cpad >= C, "zp_nchw_to_nhwc: bad args");
  by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(k_nchw_to_nhwc<T>, dim3(grid_for((long)B * H * W)), dim3(256), 0, (hipStream_t)stream, x, B, C,
                       H, W, cpad, (T*)y);
  });
  ZP_LAUNCH_CHECK("zp_nchw_to_nhwc");
  return ZP_OK;
}

extern "C" int zp_maxpool3s2(const void* x, int B, int IH, int IW, int ldx, int cx0, int C, int dtype, void* y, int OH,
                             int OW, int ldy, int cy0, void* stream) {
  const bool split = dtype == ZP_F32X3 || dtype == ZP_F32H2;
  if (!split) ZP_DTYPE_CHECK("zp_maxpool3s2", dtype);
  const int N = dtype == ZP_F32 ? 4 : 8;  // (the split planes hold 16-bit words: 8)
  ZP_CHECK_ARG(x && y && C % N == 0 && cx0 % N == 0 && ldx % N == 0 && cy0 % N == 0 && ldy % N == 0,
               "zp_maxpool3s2: bad args / alignment");
  ZP_CHECK_ARG(OH == (IH - 1) / 2 + 1 && OW == (IW - 1) / 2 + 1, "zp_maxpool3s2: OH/OW");
  const dim3 grid(grid_for((long)B * OH * OW * (C / N)));
  hipStream_t st = (hipStream_t)stream;
  if (split)
    by_planes(dtype, [&](auto npl) {
      hipLaunchKernelGGL(k_maxpool_split<npl.value>, grid, dim3(256), 0, st, (const unsigned short*)x,
                         (long)B * IH * IW * ldx, B, IH, IW, ldx, cx0, C, (unsigned short*)y, (long)B * OH * OW * ldy,
                         OH, OW, ldy, cy0);
    });
  else
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(k_maxpool<T>, grid, dim3(256), 0, st, (const T*)x, B, IH, IW, ldx, cx0, C, (T*)y, OH, OW, ldy,
                         cy0);
    });
  ZP_LAUNCH_CHECK("zp_maxpool3s2");
  return ZP_OK;
}

extern "C" int zp_maxpool3s2_bwd(const void* x, int ldx, int cx0, const void* dy, int lddy, int cdy0, int B, int IH,
                                 int IW, int C, int OH, int OW, int dtype, void* dx, int lddx, int cdx0, int accumulate,
                                 void* stream) {
  ZP_DTYPE_CHECK_TRAIN("zp_maxpool3s2_bwd", dtype);
  const int N = dtype == ZP_F32 ? 4 : 8;
  ZP_CHECK_ARG(x && dy && dx && C % N == 0 && cx0 % N == 0 && cdy0 % N == 0 && cdx0 % N == 0,
               "zp_maxpool3s2_bwd: bad args");
  ZP_CHECK_ARG(OH == (IH + 1) / 2 && OW == (IW + 1) / 2, "zp_maxpool3s2_bwd: OH/OW must be the 3x3 s2 p1 output");
  const long total = (long)B * (((IH + 1) / 2 + MP_ROWS - 1) / MP_ROWS) * ((IW + 1) / 2) * (C / N);
  by_train_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(k_maxpool_bwd<T>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx,
                       cx0, (const T*)dy, lddy, cdy0, B, IH, IW, C, OH, OW, (T*)dx, lddx, cdx0, accumulate);
  });
  ZP_LAUNCH_CHECK("zp_maxpool3s2_bwd");
  return ZP_OK;
}

extern "C" int zp_global_avgpool(const void* x, int B, int H, int W, int ldx, int cx0, int C, int dtype, void* y,
                                 void* stream) {
  const bool split = dtype == ZP_F32X3 || dtype == ZP_F32H2;
  if (!split) ZP_DTYPE_CHECK("zp_global_avgpool", dtype);
  ZP_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && C > 0, "zp_global_avgpool: bad args");
  const int N = dtype == ZP_F32 ? 4 : 8;
  const bool vec = C % N == 0 && cx0 % N == 0 && ldx % N == 0;  // 16-byte vectors
  const dim3 grid((C + 63) / 64, B);
  hipStream_t st = (hipStream_t)stream;
  if (split)  // y: [NPL][B][C]
    by_planes(dtype, [&](auto npl) {
      hipLaunchKernelGGL((vec ? k_avgpool_split8<npl.value> : k_avgpool_split<npl.value>), grid, dim3(256), 0, st,
                         (const unsigned short*)x, (long)B * H * W * ldx, H, W, ldx, cx0, C, (unsigned short*)y,
                         (long)B * C);
    });
  else
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((vec ? k_hw_reduce_vec<T, 0> : k_avgpool<T>), grid, dim3(256), 0, st, (const T*)x, H, W, ldx,
                         cx0, C, (T*)y);
    });
  ZP_LAUNCH_CHECK("zp_global_avgpool");
  return ZP_OK;
}

extern "C" int zp_broadcast_hw(const void* src, int B, int C, int dtype, void* y, int H, int W, int ldy, int cy0,
                               void* stream) {
  if (dtype == ZP_F32X3 || dtype == ZP_F32H2) {  // src [NPL][B][C] -> the planes of y [NPL][B, H, W, ldy]
    ZP_CHECK_ARG(src && y && B > 0 && C > 0 && C % 8 == 0 && ldy % 8 == 0 && cy0 % 8 == 0,
                 "zp_broadcast_hw: bad args / alignment");
    const long total = (long)B * H * W * C;
    const int npl = dtype == ZP_F32X3 ? 3 : 2;
    for (int p = 0; p < npl; ++p)
      hipLaunchKernelGGL(k_broadcast_vec<bf16_t>, dim3(grid_for(total / 8)), dim3(256), 0, (hipStream_t)stream,
                         (const bf16_t*)src + (long)p * B * C, B, C, (bf16_t*)y + (long)p * B * H * W * ldy, H, W,
                         ldy, cy0);
    ZP_LAUNCH_CHECK("zp_broadcast_hw");
    return ZP_OK;
  }
  ZP_DTYPE_CHECK("zp_broadcast_hw", dtype);
  ZP_CHECK_ARG(src && y && B > 0 && C > 0, "zp_broadcast_hw: bad args");
  long total = (long)B * H * W * C;
  by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    constexpr int N = V16<T>::N;
    if (C % N == 0 && ldy % N == 0 && cy0 % N == 0)
      hipLaunchKernelGGL(k_broadcast_vec<T>, dim3(grid_for(total / N)), dim3(256), 0, (hipStream_t)stream,
                         (const T*)src, B, C, (T*)y, H, W, ldy, cy0);
    else
      hipLaunchKernelGGL(k_broadcast<T>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const T*)src, B, C,
                         1.f, (T*)y, H, W, ldy, cy0, 0, 0);
  });
  ZP_LAUNCH_CHECK("zp_broadcast_hw");
  return ZP_OK;
}

extern "C" int zp_sum_hw(const void* dy, int B, int H, int W, int lddy, int cdy0, int C, int dtype, void* out,
                         void* stream) {
  ZP_DTYPE_CHECK_TRAIN("zp_sum_hw", dtype);
  ZP_CHECK_ARG(dy && out && B > 0 && C > 0, "zp_sum_hw: bad args");
  const int N = dtype == ZP_F32 ? 4 : 8;
  const bool vec = C % N == 0 && cdy0 % N == 0 && lddy % N == 0;
  by_train_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((vec ? k_hw_reduce_vec<T, 1> : k_sum_hw<T>), dim3((C + 63) / 64, B), dim3(256), 0,
                       (hipStream_t)stream, (const T*)dy, H, W, lddy, cdy0, C, (T*)out);
  });
  ZP_LAUNCH_CHECK("zp_sum_hw");
  return ZP_OK;
}

extern "C" int zp_add_broadcast_hw(const void* src, float mul, int B, int C, int dtype, void* y, int H, int W, int ldy,
                                   int cy0, int accumulate, void* stream) {
  ZP_DTYPE_CHECK_TRAIN("zp_add_broadcast_hw", dtype);
  ZP_CHECK_ARG(src && y && B > 0 && C > 0, "zp_add_broadcast_hw: bad args");
  by_train_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(k_broadcast<T>, dim3(grid_for((long)B * H * W * C)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)src, B, C, mul, (T*)y, H, W, ldy, cy0, accumulate, 1);
  });
  ZP_LAUNCH_CHECK("zp_add_broadcast_hw");
  return ZP_OK;
}
