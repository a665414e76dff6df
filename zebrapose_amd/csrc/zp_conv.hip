// Implicit-GEMM convolution for gfx950 (MI355X): forward / data-gradient (k_conv) in f32 / bf16 /
// fp16 (the weight gradient: zp_wgrad.hip; split fp32: zp_conv3*.hip).  NHWC activations, packed
// [rows][tap*Cin] weights.
//
// Replaces the cuDNN convolutions behind nn.Conv2d / nn.ConvTranspose2d at
// model/resnet.py:41-51, model/aspp.py:60-80, 89-112 and the torchvision ResNet
// children reused at resnet.py:191-199 (see include/zp.h).
//
// Forward tile: one workgroup of 2*NWP waves (2 cout x NWP pixel) computes TC (=32*WC)
// output channels x TP (=64*NWP) pixels.  The MFMA A operand is the weight tile (rows =
// output channels), B is the activation tile (cols = pixels), so each lane ends up with 4
// consecutive output channels of one pixel -> 8/16 B NHWC stores.  K steps are 128 bytes per
// row (64 bf16 / 32 f32) of one tap, staged global -> LDS by LDS-DMA through a STAGES-deep
// ring (XOR-swizzled 16 B chunks, one barrier per K step).
#include <type_traits>
#include "zp_common.h"
#include "zp_conv_kern.h"
#include "zp_conv3.h"

namespace zp {

// all-zero source for out-of-image / padding taps of the direct-to-LDS loads
__device__ uint4 g_zero_page[8];

// Conv epilogue shared by k_conv and k_conv_strip: BN scale/shift (+bias), residual, ReLU,
// NHWC (channel slice) / NCHW-head / f32 stores, or train-mode BN partial statistics.
template <typename T, int WC, int WP, int NWP, bool BNR = false>
__device__ __forceinline__ void conv_epilogue(const zp_conv_args& A, const zp_conv_sub& S, f32x4 (&acc)[WC][WP],
                                              const int p0, const int c0, const int wc, const int wp, const int lane,
                                              const int M, const int GHW, const int bx, const int zi,
                                              const int nz, unsigned* rflag = nullptr, float* red = nullptr) {
  // ---------------- epilogue ----------------
  // (zi, nz): this tile's sub-problem and the sub-problem count, for the statistics part index
  // (blockIdx.z / gridDim.z, except in k_conv_quad, whose tiles hold all four sub-pixel phases)
  // output pixel of (lane, j): one division for j = 0, then +16 pixels per j
  int pn[WP], poy[WP], pox[WP];
  bool pok[WP];
  {
    const int pw0 = p0 + wp * 16 * WP + (lane & 15);
    int n = pw0 / GHW, rr = pw0 - n * GHW;
    int gy = rr / A.GW, gx = rr - gy * A.GW;
    const bool fast = A.GW % 16 == 0;
#pragma unroll
    for (int j = 0; j < WP; ++j) {
      const int p = pw0 + j * 16;
      pok[j] = p < M;
      if (j > 0) {
        if (fast) {
          gx += 16;
          if (gx >= A.GW) {
            gx -= A.GW;
            if (++gy == A.GH) {
              gy = 0;
              ++n;
            }
          }
        } else {
          n = p / GHW;
          rr = p - n * GHW;
          gy = rr / A.GW;
          gx = rr - gy * A.GW;
        }
      }
      pn[j] = n;
      poy[j] = gy * S.oys + S.oyo;
      pox[j] = gx * S.oxs + S.oxo;
    }
  }
  // BNR (k_conv_strip2's bnr instance): the fused BN backward sums (zp.h bnr_*) are taken in the
  // paired store loop below, on its 8-channel lanes (16-byte raw loads, issued before the pixel loop)
  constexpr bool BPAIR = BNR && sizeof(T) == 2 && WC % 2 == 0;
  bool bdone = false;  // the paired loop took them
  if constexpr (BPAIR) {
    if (A.bnr_part) __syncthreads();  // red (the kernel's LDS): every wave's main loop has finished reading it
  }
  bool stored = false;
  if constexpr (sizeof(T) == 2 && WC % 2 == 0) {
    // bf16 NHWC fast path: v_permlane16_swap pairs lane groups (g, g + 1) so that each lane
    // holds 8 consecutive output channels of one pixel (tiles i and i + 1 exchange halves):
    // 16 B stores (and residual loads), half the store instructions
    if (A.out_mode == ZP_OUT_NHWC && A.Cout % 8 == 0 && S.ldy % 8 == 0 && S.cy0 % 8 == 0 &&
        (!A.res || (A.ldr % 8 == 0 && A.cr0 % 8 == 0))) {
      stored = true;
      const int g = lane >> 4;
#pragma unroll
      for (int i = 0; i < WC; i += 2) {
        const int cs = c0 + wc * 16 * WC + (i + (g & 1)) * 16 + (g >> 1) * 8;
        const bool cok = cs < A.Cout;
        float sc[8], sh[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          sc[r] = 1.f;
          sh[r] = 0.f;
        }
        const float* psc = S.scale + cs;
        const float* psh = S.shift + cs;
        if (ZP_ABL != 7 && cok && S.scale) {
          const float4 s0 = *(const float4*)psc, s1 = *(const float4*)(psc + 4);
          sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w;
          sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w;
        }
        if (ZP_ABL != 7 && cok && S.shift) {
          const float4 s0 = *(const float4*)psh, s1 = *(const float4*)(psh + 4);
          sh[0] = s0.x; sh[1] = s0.y; sh[2] = s0.z; sh[3] = s0.w;
          sh[4] = s1.x; sh[5] = s1.y; sh[6] = s1.z; sh[7] = s1.w;
        }
        // BPAIR: this lane's 8 channels' BN terms and the raw x of its WP pixels, loaded up front
        uint4 bx8[BPAIR ? WP : 1];
        float bm[8], bi[8], bsc[8], bsh[8], bs0[8], bs1[8];
        if constexpr (BPAIR) {
          if (A.bnr_part) {
#pragma unroll
            for (int j = 0; j < WP; ++j) {
              const size_t pix = ((size_t)pn[j] * S.OH + poy[j]) * S.OW + pox[j];
              bx8[j] = (pok[j] && cok) ? *(const uint4*)((const unsigned short*)A.bnr_x + pix * A.Cout + cs)
                                       : make_uint4(0u, 0u, 0u, 0u);
            }
            float4 q[8];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              q[2 * t] = cok ? *(const float4*)(A.bnr_save + t * A.Cout + cs) : make_float4(0.f, 0.f, 0.f, 0.f);
              q[2 * t + 1] = cok ? *(const float4*)(A.bnr_save + t * A.Cout + cs + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            float* dst[4] = {bm, bi, bsc, bsh};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              dst[t][0] = q[2 * t].x; dst[t][1] = q[2 * t].y; dst[t][2] = q[2 * t].z; dst[t][3] = q[2 * t].w;
              dst[t][4] = q[2 * t + 1].x; dst[t][5] = q[2 * t + 1].y; dst[t][6] = q[2 * t + 1].z; dst[t][7] = q[2 * t + 1].w;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) bs0[r] = bs1[r] = 0.f;
          }
        }
#pragma unroll
        for (int j = 0; j < WP; ++j) {
          float v[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) {  // all lanes active here (cross-lane op)
            const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][j][r]),
                                                             __float_as_uint(acc[i + 1][j][r]), false, false);
            v[r] = __uint_as_float(sw[0]);
            v[r + 4] = __uint_as_float(sw[1]);
          }
          if (!pok[j] || !cok) continue;
          const size_t pix = ((size_t)pn[j] * S.OH + poy[j]) * S.OW + pox[j];
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = v[r] * sc[r] + sh[r];
          if (A.res) {
            const uint4 rv = *(const uint4*)((const unsigned short*)A.res + pix * A.ldr + A.cr0 + cs);
            const uint32_t rw[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              v[2 * r] += H16<T>::from(rw[r] & 0xffffu);
              v[2 * r + 1] += H16<T>::from(rw[r] >> 16);
            }
          }
          if (A.relu) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = fmaxf(v[r], 0.f);
          }
          uint32_t o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = H16<T>::to(v[2 * r]) | (H16<T>::to(v[2 * r + 1]) << 16);
          if constexpr (BPAIR) {
            if (A.bnr_part) {  // g = the stored gradient; mask and xhat from the raw x (relu mode 2)
              const uint32_t xw[4] = {bx8[j].x, bx8[j].y, bx8[j].z, bx8[j].w};
#pragma unroll
              for (int r = 0; r < 8; ++r) {
                const float xx = H16<T>::from((r & 1) ? (xw[r >> 1] >> 16) : (xw[r >> 1] & 0xffffu));
                float g = H16<T>::from((r & 1) ? (o[r >> 1] >> 16) : (o[r >> 1] & 0xffffu));
                g = __builtin_fmaf(xx, bsc[r], bsh[r]) > 0.f ? g : 0.f;
                bs0[r] += g;
                bs1[r] += g * (xx - bm[r]) * bi[r];
              }
            }
          }
          if (ZP_ABL == 6 && o[0] != 0x3f803f80u) continue;  // diagnostic: no stores (unless a value pair is exactly 1, 1)
          if constexpr (ZP_ABL == 8) {  // diagnostic: non-temporal stores
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            u32x4* yp = (u32x4*)((unsigned short*)S.y + pix * S.ldy + S.cy0 + cs);
            __builtin_nontemporal_store((u32x4){o[0], o[1], o[2], o[3]}, yp);
          } else {
            *(uint4*)((unsigned short*)S.y + pix * S.ldy + S.cy0 + cs) = make_uint4(o[0], o[1], o[2], o[3]);
          }
        }
        if constexpr (BPAIR) {
          if (A.bnr_part) {
            bdone = true;
#pragma unroll
            for (int r = 0; r < 8; ++r) {  // over the 16 pixel lanes of this lane row (all lanes active)
              bs0[r] = row16_sum(bs0[r]);
              bs1[r] = row16_sum(bs1[r]);
            }
            if ((lane & 15) == 0) {  // red: [wp][sum][channel of the tile] (k_conv_strip2 passes it)
              const int ct = cs - c0;
              constexpr int TCB = 32 * WC;
              float* r0 = red + (wp * 2 + 0) * TCB + ct;
              float* r1 = red + (wp * 2 + 1) * TCB + ct;
              *(float4*)r0 = make_float4(bs0[0], bs0[1], bs0[2], bs0[3]);
              *(float4*)(r0 + 4) = make_float4(bs0[4], bs0[5], bs0[6], bs0[7]);
              *(float4*)r1 = make_float4(bs1[0], bs1[1], bs1[2], bs1[3]);
              *(float4*)(r1 + 4) = make_float4(bs1[4], bs1[5], bs1[6], bs1[7]);
            }
          }
        }
      }
    }
  }
  const int cbase = c0 + wc * 16 * WC + (lane >> 4) * 4;
#pragma unroll
  for (int j = 0; j < WP && !stored; ++j) {
    if (!pok[j]) continue;
    const int n = pn[j], oy = poy[j], ox = pox[j];
    size_t pix = ((size_t)n * S.OH + oy) * S.OW + ox;
#pragma unroll
    for (int i = 0; i < WC; ++i) {
      const int cf = cbase + i * 16;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int c = cf + r;
        float sc = (S.scale && c < A.Cout) ? S.scale[c] : 1.f;
        float sh = (S.shift && c < A.Cout) ? S.shift[c] : 0.f;
        v[r] = acc[i][j][r] * sc + sh;
      }
      if (A.res) {
        const T* R = (const T*)A.res + pix * A.ldr + A.cr0 + cf;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (cf + r < A.Cout) v[r] += Elem<T>::ld(R + r);
      }
      if (A.relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (A.out_mode == ZP_OUT_HEAD_NCHW) {
        const size_t plane = (size_t)S.OH * S.OW;
        const size_t sp = (size_t)oy * S.OW + ox;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int c = cf + r;
          if (c >= A.Cout) continue;
          if (c == 0)
            ((float*)S.y)[(size_t)n * plane + sp] = v[r];
          else
            ((float*)S.y2)[((size_t)n * (A.Cout - 1) + (c - 1)) * plane + sp] = v[r];
        }
        continue;
      }
      if constexpr (sizeof(T) == 4) {
        if (A.out_mode == ZP_OUT_NHWC_X3 || A.out_mode == ZP_OUT_NHWC_H2) {
          // f32 call writing a split-fp32 tensor (the split-mode stem)
          const long psy = (long)A.N * S.OH * S.OW * S.ldy;
          unsigned short* Y = (unsigned short*)S.y + pix * S.ldy + S.cy0 + cf;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (cf + r >= A.Cout) continue;
            if (A.out_mode == ZP_OUT_NHWC_X3) {
              unsigned short q[3];
              SplitF32<3>::split(v[r], q);
              Y[r] = q[0];
              Y[r + psy] = q[1];
              Y[r + 2 * psy] = q[2];
            } else {
              unsigned short q[2];
              SplitF32<2>::split(v[r], q);
              Y[r] = q[0];
              Y[r + psy] = q[1];
              raise_range_flag(rflag, h2_overflow(v[r]));
            }
          }
          continue;
        }
      }
      if (A.out_mode == ZP_OUT_NHWC_F32 || sizeof(T) == 4) {
        float* Y = (float*)S.y + pix * S.ldy + S.cy0 + cf;
        if (cf + 3 < A.Cout) {
          *(float4*)Y = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (cf + r < A.Cout) Y[r] = v[r];
        }
      } else {
        unsigned short b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          b[r] = (unsigned short)H16<T>::to(v[r]);
          v[r] = H16<T>::from(b[r]);  // statistics of the stored value
        }
        unsigned short* Y = (unsigned short*)S.y + pix * S.ldy + S.cy0 + cf;
        if (cf + 3 < A.Cout) {
          *(uint2*)Y = make_uint2((uint32_t)b[0] | ((uint32_t)b[1] << 16), (uint32_t)b[2] | ((uint32_t)b[3] << 16));
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (cf + r < A.Cout) Y[r] = b[r];
        }
      }
    }
  }
  if (A.stats) {
    // Train-mode BatchNorm statistics of the raw (stored) conv output, per wave half:
    // (count, mean, M2) with M2 centred on the local mean (two passes over the registers, no
    // E[x^2] - E[x]^2 cancellation); zp_bn_train_finalize merges the parts (Chan et al.).
    // red (k_conv_strip2, round 5): the NWP wave halves of a cout block are merged in LDS first, in
    // wave order (Chan's pairwise update in f32), and the tile writes one part
    // (zp_conv2d_stat_parts): a quarter of the partials for the merge to read -- at 128 x 128,
    // bs 32, 2048 parts instead of 8192 (that merge took 43 us)
    const int parts = red ? gridDim.x * nz : gridDim.x * nz * NWP;
    const int part = red ? zi * gridDim.x + bx : (zi * gridDim.x + bx) * NWP + wp;
    constexpr int TCS = 32 * WC;  // channels of the tile's cout block
    if (red) __syncthreads();  // every wave's last main-loop LDS read precedes the writes below
    float cnt = 0.f;
#pragma unroll
    for (int j = 0; j < WP; ++j) cnt += (p0 + wp * 16 * WP + j * 16 + (lane & 15) < M) ? 1.f : 0.f;
    if constexpr (sizeof(T) == 2) {
          cnt = row16_sum(cnt);
        } else {  // f32 parity mode: DPP temporaries pushed this 128-accumulator tile past 256 VGPRs
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) cnt += __shfl_xor(cnt, off);
        }
#pragma unroll
    for (int i = 0; i < WC; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float vv[WP];
        float sm = 0.f;
#pragma unroll
        for (int j = 0; j < WP; ++j) {
          const bool ok = p0 + wp * 16 * WP + j * 16 + (lane & 15) < M;
          float v = acc[i][j][r];
          if (sizeof(T) == 2 && A.out_mode != ZP_OUT_NHWC_F32) v = H16<T>::from(H16<T>::to(v));  // stored value
          vv[j] = ok ? v : 0.f;
          sm += vv[j];
        }
        if constexpr (sizeof(T) == 2) {
          sm = row16_sum(sm);
        } else {  // f32 parity mode: DPP temporaries pushed this 128-accumulator tile past 256 VGPRs
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) sm += __shfl_xor(sm, off);
        }
        const float mean = cnt > 0.f ? sm / cnt : 0.f;
        float m2 = 0.f;
#pragma unroll
        for (int j = 0; j < WP; ++j) {
          const bool ok = p0 + wp * 16 * WP + j * 16 + (lane & 15) < M;
          const float dlt = vv[j] - mean;
          m2 += ok ? dlt * dlt : 0.f;
        }
        if constexpr (sizeof(T) == 2) {
          m2 = row16_sum(m2);
        } else {  // f32 parity mode: DPP temporaries pushed this 128-accumulator tile past 256 VGPRs
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) m2 += __shfl_xor(m2, off);
        }
        const int c = cbase + i * 16 + r;
        if (red) {
          if ((lane & 15) == 0) {  // [wp][cnt, mean, m2][channel of the tile]
            red[(wp * 3 + 0) * TCS + c - c0] = cnt;
            red[(wp * 3 + 1) * TCS + c - c0] = mean;
            red[(wp * 3 + 2) * TCS + c - c0] = m2;
          }
        } else if ((lane & 15) == 0 && c < A.Cout) {
          A.stats[(size_t)part * A.Cout + c] = cnt;
          A.stats[((size_t)parts + part) * A.Cout + c] = mean;
          A.stats[((size_t)2 * parts + part) * A.Cout + c] = m2;
        }
      }
    if (red) {
      __syncthreads();
      const int t = wc * NWP * 64 + wp * 64 + lane;  // flat thread id: thread t merges channel c0 + t
      if (t < TCS && c0 + t < A.Cout) {
        float n = red[t], mu = red[TCS + t], q = red[2 * TCS + t];
#pragma unroll
        for (int w = 1; w < NWP; ++w) {
          const float nw = red[(w * 3 + 0) * TCS + t];
          if (nw > 0.f) {
            const float mw = red[(w * 3 + 1) * TCS + t], qw = red[(w * 3 + 2) * TCS + t];
            const float nn = n + nw, d = mw - mu;
            mu += d * (nw / nn);
            q += qw + d * d * (n * nw / nn);
            n = nn;
          }
        }
        A.stats[(size_t)part * A.Cout + c0 + t] = n;
        A.stats[((size_t)parts + part) * A.Cout + c0 + t] = mu;
        A.stats[((size_t)2 * parts + part) * A.Cout + c0 + t] = q;
      }
    }
  }
  if (A.bnr_part) {
    // Data gradient feeding a train-mode BN + ReLU backward (zp.h bnr_*): per wave half, the sums
    // zp_bn_bwd_reduce (relu mode 2) takes over the stored gradient g -- masked where the forward's
    // fma(x, scale, shift) was <= 0 -- and g * xhat, xhat = (x - mean) * invstd of the BN's raw
    // input x at the same pixel.  The zp_conv2d checks leave no scale / shift / residual / ReLU here:
    // the stored value is the accumulator (rounded to T).  BPAIR (bdone): the paired store loop
    // took them into red already; otherwise (k_conv / k_conv_quad dgrads, the f32 parity mode) this
    // pass, 4 channels per lane, loads issued per channel block before their use.
    // red (k_conv_strip2: its LDS, free after the main loop): the NWP wave halves of a cout block meet
    // there and the tile writes one part (zp_conv2d_bnr_parts) -- a quarter of the partials for the
    // totals pass to read
    const int parts = red ? gridDim.x * nz : gridDim.x * nz * NWP;
    const int part = red ? zi * gridDim.x + bx : (zi * gridDim.x + bx) * NWP + wp;
    constexpr int TCB = 32 * WC;  // channels of the tile's cout block (2 wave rows of 16 * WC)
    if (!bdone) {
      if (red) __syncthreads();  // every wave's last main-loop LDS read precedes the writes below
      const float* sv = A.bnr_save;
      using XV = typename std::conditional<sizeof(T) == 2, uint2, float4>::type;
#pragma unroll
      for (int i = 0; i < WC; ++i) {
        const int cf = cbase + i * 16;
        const bool cok = cf < A.Cout;  // (Cout % 4 == 0: all four channels or none)
        XV xr[WP];
#pragma unroll
        for (int j = 0; j < WP; ++j) {
          const size_t pix = ((size_t)pn[j] * S.OH + poy[j]) * S.OW + pox[j];
          xr[j] = (pok[j] && cok) ? *(const XV*)((const T*)A.bnr_x + pix * A.Cout + cf) : XV{};
        }
        float4 pm[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pm[q] = cok ? *(const float4*)(sv + q * A.Cout + cf) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float mean[4] = {pm[0].x, pm[0].y, pm[0].z, pm[0].w}, inv[4] = {pm[1].x, pm[1].y, pm[1].z, pm[1].w};
        const float msc[4] = {pm[2].x, pm[2].y, pm[2].z, pm[2].w}, msh[4] = {pm[3].x, pm[3].y, pm[3].z, pm[3].w};
        float sg[4] = {0.f, 0.f, 0.f, 0.f}, sgx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < WP; ++j) {
          float xx[4];
          if constexpr (sizeof(T) == 2) {
            xx[0] = H16<T>::from(xr[j].x & 0xffffu);
            xx[1] = H16<T>::from(xr[j].x >> 16);
            xx[2] = H16<T>::from(xr[j].y & 0xffffu);
            xx[3] = H16<T>::from(xr[j].y >> 16);
          } else {
            xx[0] = xr[j].x; xx[1] = xr[j].y; xx[2] = xr[j].z; xx[3] = xr[j].w;
          }
          const bool ok = pok[j] && cok;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float g = acc[i][j][r];
            if (sizeof(T) == 2 && A.out_mode != ZP_OUT_NHWC_F32) g = H16<T>::from(H16<T>::to(g));  // stored value
            g = (ok && __builtin_fmaf(xx[r], msc[r], msh[r]) > 0.f) ? g : 0.f;
            sg[r] += g;
            sgx[r] += g * (xx[r] - mean[r]) * inv[r];
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (sizeof(T) == 2) {
            sg[r] = row16_sum(sg[r]);
            sgx[r] = row16_sum(sgx[r]);
          } else {
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
              sg[r] += __shfl_xor(sg[r], off);
              sgx[r] += __shfl_xor(sgx[r], off);
            }
          }
        }
        if (red) {
          if ((lane & 15) == 0) {  // [wp][sum][channel of the tile]
            const int ct = cf - c0;
            *(float4*)(red + (wp * 2 + 0) * TCB + ct) = make_float4(sg[0], sg[1], sg[2], sg[3]);
            *(float4*)(red + (wp * 2 + 1) * TCB + ct) = make_float4(sgx[0], sgx[1], sgx[2], sgx[3]);
          }
        } else if ((lane & 15) == 0 && cok) {
          *(float4*)(A.bnr_part + (size_t)part * A.Cout + cf) = make_float4(sg[0], sg[1], sg[2], sg[3]);
          *(float4*)(A.bnr_part + ((size_t)parts + 1 + part) * A.Cout + cf) = make_float4(sgx[0], sgx[1], sgx[2], sgx[3]);
        }
      }
    }
    if (red) {
      __syncthreads();
      // the tile's sums over its NWP wave halves, in wave order: thread t < TCB sums channel t
      const int t = wc * NWP * 64 + wp * 64 + lane;  // flat thread id (wave = wc * NWP + wp)
      if (t < TCB && c0 + t < A.Cout) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int w = 0; w < NWP; ++w) {
          s0 += red[(w * 2 + 0) * TCB + t];
          s1 += red[(w * 2 + 1) * TCB + t];
        }
        A.bnr_part[(size_t)part * A.Cout + c0 + t] = s0;
        A.bnr_part[((size_t)parts + 1 + part) * A.Cout + c0 + t] = s1;
      }
    }
  }
}

// Staging: every K step moves TC weight rows + TP activation rows of 128 B each straight
// from global memory into LDS with global_load_lds_dwordx4 (one wave-instruction = 8 rows x
// 128 B, lane-linear in LDS).  The 16 B chunk swizzle (chunk ^ (row & 7), conflict-free
// ds_read_b128 of the MFMA fragments) is applied on the per-lane SOURCE address.  Out-of-
// image taps read g_zero_page.  STAGES LDS buffers: the loads of steps k+1..k+STAGES-1 are
// in flight while step k's MFMAs run; each step ends with a counted vmcnt wait (only the
// oldest step's loads) and a raw s_barrier.
template <typename T, int WC, int WP, int NWP, int STAGES, bool SMALLC>
__global__ void __launch_bounds__(128 * NWP) k_conv(const zp_conv_args A, const conv_taps TG, const int flags) {
  static_assert(STAGES == 2 || STAGES == 3, "2- or 3-deep LDS ring");
  constexpr int E = MfmaTraits<T>::E;
  constexpr int KE = 8 * E;  // elements per K step (128 B)
  constexpr int TC = 32 * WC, TP = 16 * WP * NWP;
  constexpr int NW = 2 * NWP;                 // waves
  constexpr int G = (TC + TP) / 8;            // 8-row groups per K step
  static_assert(G % NW == 0, "row groups must split evenly over the waves");
  constexpr int GPW = G / NW;                 // groups per wave
  // the first WPW groups of every wave are weight rows, the rest activation rows (group g = wid + NW*i
  // is a weight group iff i < WPW): compile-time, so per-pixel state exists only for pixel groups
  static_assert((TC / 8) % NW == 0, "weight groups must split evenly over the waves");
  constexpr int WPW = TC / 8 / NW;
  constexpr int LPS = ZP_ABL == 3 ? WPW : GPW;  // LDS-DMA instructions per wave per stage
  __shared__ uint4 lds0[(TC + TP) * 8];
  __shared__ uint4 lds1[(TC + TP) * 8];
  __shared__ uint4 lds2[STAGES == 3 ? (TC + TP) * 8 : 1];
  auto bufp = [&](auto i_c) -> uint4* {
    constexpr int i = decltype(i_c)::value;
    if constexpr (i == 0) return lds0;
    else if constexpr (i == 1) return lds1;
    else return lds2;
  };

  const zp_conv_sub& S = A.sub[blockIdx.z];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (scalar branches)
  const int wc = wid / NWP, wp = wid % NWP;
  const int GHW = A.GH * A.GW;
  const int M = A.N * GHW;
  // XCD-aware tile order (flags & 2): workgroups are dispatched round-robin over the
  // 8 XCDs, so consecutive linear ids land on different L2s.  Remap so that each XCD walks a
  // contiguous run of (pixel tile, cout tile) pairs, cout tiles fastest: the cout tiles of one
  // pixel tile (same activations) and neighbouring pixel tiles (shared halo rows) then meet in
  // the same L2.
  int bx = blockIdx.x, by = blockIdx.y;
  if (flags & 2) {
    const int total = gridDim.x * gridDim.y;
    const int bid = blockIdx.x + gridDim.x * blockIdx.y;
    const int lin = (total & 7) ? bid : (bid & 7) * (total >> 3) + (bid >> 3);
    bx = lin / gridDim.y;
    by = lin - bx * gridDim.y;
  }
  const int p0 = bx * TP, c0 = by * TC;
  const int lrow = lane >> 3;                  // row within the 8-row group
  const int csrc = (lane & 7) ^ lrow;          // source chunk (swizzle on the source side)

  // per group: weight row or activation row (pixel) of this lane
  int gpix_n[GPW], gpix_y[GPW], gpix_x[GPW];
  bool gvalid[GPW];
#pragma unroll
  for (int i = 0; i < GPW; ++i) {
    if (i < WPW) continue;
    const int r = (wid + NW * i) * 8 + lrow;
    int m = p0 + (r - TC);
    gvalid[i] = r >= TC && m < M;
    int mm = gvalid[i] ? m : 0;
    int n = mm / GHW, rr = mm - n * GHW;
    int gy = rr / A.GW, gx = rr - gy * A.GW;
    gpix_n[i] = n;
    gpix_y[i] = gy * A.sy;
    gpix_x[i] = gx * A.sx;
  }
  const T* __restrict__ X = (const T*)A.x;
  const T* __restrict__ Wt = (const T*)S.w;
  const int CB = SMALLC ? 1 : A.Cin / KE;
  int nK = SMALLC ? A.k_pad / KE : S.ntaps * CB;

  // ---- staging addresses (Cin >= 64 B-chunk path): buffer loads with per-lane 32-bit byte
  // offsets.  The tap walk (ty, tx, channel chunk) is scalar state advanced by one K step per
  // issue; per lane only the pixel's base offset and two validity bit masks (input row / column
  // in range, one bit per tap row / column) are kept.  Invalid taps use an offset past the
  // buffer's end, which the buffer unit returns as zeros: no address clamp, no select of a
  // zero page, no multiplies in the loop.
  const int tb = blockIdx.z;
  const int ny = TG.ny[tb], nx = TG.nx[tb], dty = TG.dty[tb], dtx = TG.dtx[tb];
  unsigned abase[GPW], ymask[GPW], xmask[GPW];
#pragma unroll
  for (int i = 0; i < GPW; ++i) {
    if (i < WPW) continue;
    const int y0 = gpix_y[i], x0 = gpix_x[i];
    abase[i] = (unsigned)(((((long)gpix_n[i] * A.IH + y0) * A.IW + x0) * A.ldx + A.cx0 + csrc * E) * sizeof(T));
    unsigned ym = 0, xm = 0;
    for (int q = 0; q < ny; ++q) ym |= (unsigned)((unsigned)(y0 + TG.ty0[tb] + q * dty) < (unsigned)A.IH) << q;
    for (int q = 0; q < nx; ++q) xm |= (unsigned)((unsigned)(x0 + TG.tx0[tb] + q * dtx) < (unsigned)A.IW) << q;
    ymask[i] = gvalid[i] ? ym : 0u;
    xmask[i] = xm;
  }
  // Tap-row trimming (flags & 16): a tap row whose input rows lie outside the image for every
  // output row of this tile only ever stages zeros.  A tile inside one image runs just the K
  // steps of tap rows [qlo, qhi] (the valid rows are contiguous: the row offset is monotonic in
  // q).  ASPP's dilation-12 / -18 convs at 32 x 32 run 6 of 9 taps on most 8-row tiles.  The
  // test is scalar (wave-uniform) and conservative: it never drops a row holding a valid tap.
  int qlo = 0, qhi = ny - 1;
  if (!SMALLC && (flags & 16) && ny > 1) {
    const int mlast = min(p0 + TP, M) - 1;
    const int n0 = p0 / GHW, n1 = mlast / GHW;
    if (n0 == n1) {
      const int ya = (p0 - n0 * GHW) / A.GW * A.sy, yb = (mlast - n1 * GHW) / A.GW * A.sy;
      int lo = ny, hi = -1;
      for (int q = 0; q < ny; ++q) {
        const int off = TG.ty0[tb] + q * dty;
        if (yb + off >= 0 && ya + off <= A.IH - 1) {
          lo = min(lo, q);
          hi = q;
        }
      }
      if (hi >= lo) {
        qlo = lo;
        qhi = hi;
        nK = (qhi - qlo + 1) * nx * CB;
      }
    }
  }
  const int kb0 = qlo * nx * CB;  // first K step (weights are tap-major: K = (q nx + r) CB + cb)
  const unsigned wbase = (unsigned)(((size_t)(c0 + wid * 8 + lrow) * A.k_pad + csrc * E) * sizeof(T));
  // scalar tap walk: the next K step to issue is (tap row tyi, tap column txi, chunk cb) with
  // act_off = ((ty * IW + tx) * ldx + cb * KE) * sizeof(T)
  int w_tyi = qlo, w_txi = 0, w_cb = 0;
  int act_off = (((TG.ty0[tb] + qlo * dty) * A.IW + TG.tx0[tb]) * A.ldx) * (int)sizeof(T);
  const int step_x = dtx * A.ldx * (int)sizeof(T), step_y = dty * A.IW * A.ldx * (int)sizeof(T);
  const int chunk_b = KE * (int)sizeof(T);
#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t xrsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)X, (short)0, (int)TG.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)Wt, (short)0, (int)TG.w_bytes[tb], 0x00020000);
#endif

  auto issue = [&](int ks, uint4* dst) {
    if constexpr (SMALLC) {
      // small Cin (stem): one K step mixes taps, per-lane tap decode
      const int kw_off = ks * KE;
      int k = ks * KE + csrc * E;
      int t = k / A.Cin;
      const int cc = k - t * A.Cin;
      const bool tok = t < S.ntaps;
      int kyy = t / S.kw;
      const int ty = kyy * S.dil - S.pad;
      const int tx = (t - kyy * S.kw) * S.dil - S.pad;
      const void* srcs[GPW];
#pragma unroll
      for (int i = 0; i < GPW; ++i) {
        const int g = wid + NW * i;
        const int r = g * 8 + lrow;
        const void* src;
        if (i < WPW) {
          src = Wt + (size_t)(c0 + r) * A.k_pad + kw_off + csrc * E;
        } else {
          int iy = gpix_y[i] + ty, ix = gpix_x[i] + tx;
          bool ok = tok && gvalid[i] && (unsigned)iy < (unsigned)A.IH && (unsigned)ix < (unsigned)A.IW;
          int iyc = min(max(iy, 0), A.IH - 1), ixc = min(max(ix, 0), A.IW - 1);
          const T* pv = X + (((size_t)gpix_n[i] * A.IH + iyc) * A.IW + ixc) * A.ldx + A.cx0 + cc;
          src = ok ? (const void*)pv : (const void*)&g_zero_page[lane & 7];
        }
        srcs[i] = src;
      }
#if defined(__HIP_DEVICE_COMPILE__)  // device-only builtin: the host pass would silently drop the kernel stubs
#pragma unroll
      for (int i = 0; i < GPW; ++i) {
        const int g = wid + NW * i;
        __builtin_amdgcn_global_load_lds(srcs[i], (__attribute__((address_space(3))) void*)&dst[g * 64], 16, 0, 0);
      }
#endif
    } else {
      // all offsets first (distinct registers), then the DMA issues back to back: hipcc waits
      // vmcnt(0) before it rewrites the address VGPRs of an in-flight LDS-DMA
      unsigned voff[GPW];
#pragma unroll
      for (int i = 0; i < GPW; ++i) {
        const int g = wid + NW * i;
        if (i < WPW) {  // weight group (compile-time)
          voff[i] = wbase + (unsigned)(NW * i * 8) * (unsigned)(A.k_pad * sizeof(T));
        } else {
          const bool ok = (ymask[i] >> w_tyi) & (xmask[i] >> w_txi) & 1u;
          voff[i] = ok ? abase[i] + (unsigned)act_off : 0x80000000u;
        }
      }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
      for (int i = 0; i < GPW; ++i) {
        const int g = wid + NW * i;
        auto* d = (__attribute__((address_space(3))) void*)&dst[g * 64];
        if (i < WPW)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, d, 16, voff[i], (kb0 + ks) * chunk_b, 0, 0);
        else if (ZP_ABL != 3)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, d, 16, voff[i], 0, 0, 0);
      }
#endif
      // advance the scalar tap walk to step ks + 1 (tap-major: chunks fastest)
      act_off += chunk_b;
      if (++w_cb == CB) {
        w_cb = 0;
        act_off += step_x - CB * chunk_b;
        if (++w_txi == nx) {
          w_txi = 0;
          act_off += step_y - nx * step_x;
          ++w_tyi;
        }
      }
    }
  };

  f32x4 acc[WC][WP];
#pragma unroll
  for (int i = 0; i < WC; ++i)
#pragma unroll
    for (int j = 0; j < WP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Three-stage ring: while step k computes from buffer k%3, the DMA of steps k+1 (issued one
  // step earlier) and k+2 (issued now) are in flight.  End of step k: counted vmcnt(GPW) (only
  // step k+2's loads may remain outstanding) + raw s_barrier -- never __syncthreads(), whose
  // vmcnt(0) would drain the ring.  Buffer indices are compile-time (loop unrolled by 3) and the
  // three buffers are distinct LDS objects, so hipcc can prove a ds_read never aliases an
  // in-flight global_load_lds and inserts no vmcnt wait in front of it.
  const bool pingpong = NW == 8 && !SMALLC && (flags & 8);
  // per-lane byte offsets of the MFMA fragments inside a stage buffer: row (lane & 15) of the
  // wave's first 16-row tile, 16 B chunk (s * 4 + lane / 16) swizzled by (row & 7) = (lane & 7);
  // tile i / j adds i * 16 rows = i * 2048 B (an immediate of the ds_read)
  unsigned aoff[2], boff[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const unsigned chunk = (unsigned)(((s2 * 4 + (lane >> 4)) ^ (lane & 7)) * 16);
    aoff[s2] = (unsigned)(wc * 16 * WC + (lane & 15)) * 128u + chunk;
    boff[s2] = (unsigned)(TC + wp * 16 * WP + (lane & 15)) * 128u + chunk;
  }
  auto step = [&](auto cur_c, auto nxt_c, int ks) {
    const bool more = ks + (STAGES - 1) < nK;
    // next stage's DMA first (its tap offsets come from scalar loads, whose lgkmcnt wait must
    // not also wait for this step's fragment reads)
    if constexpr (ZP_ABL != 1) {
      if (more) issue(ks + (STAGES - 1), bufp(nxt_c));
    }
    // fragment reads as inline asm: hipcc's waitcnt pass cannot prove across the loop back-edge
    // that they miss the in-flight LDS-DMA buffers and would put a vmcnt(0) in front of them
    const unsigned cb = lds_addr(bufp(cur_c));
    uint4 af[2][WC], bfr[2][WP];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const unsigned pa = cb + aoff[s2], pb = cb + boff[s2];
      static_for<WC>([&](auto i) { af[s2][i] = ds_read16<i * 2048>(pa); });
      static_for<WP>([&](auto j) { bfr[s2][j] = ds_read16<j * 2048>(pb); });
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (pingpong) {
      // end of the read section: fragments in registers (the other group may refill this
      // buffer after the barrier) and every load but the newest step's retired, so the next
      // step's buffer is complete once all waves have passed the barrier
      if (more) vm_wait<LPS * (STAGES - 2)>();
      else vm_wait<0>();
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    if (flags & 4) __builtin_amdgcn_s_setprio(1);
    if constexpr (ZP_ABL != 2) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int i = 0; i < WC; ++i)
#pragma unroll
          for (int j = 0; j < WP; ++j) MfmaTraits<T>::mma(acc[i][j], af[s2][i], bfr[s2][j]);
    } else {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int i = 0; i < WC; ++i) acc[i][0][0] += __uint_as_float(af[s2][i].x ^ bfr[s2][0].y);
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the MFMAs in front of the wait + barrier
    if (flags & 4) __builtin_amdgcn_s_setprio(0);
    if (!pingpong) {
      if (more) vm_wait<LPS * (STAGES - 2)>();
      else vm_wait<0>();
    }
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  issue(0, lds0);
  if (STAGES == 3 && nK > 1) {
    issue(1, lds1);
    vm_wait<LPS * (STAGES - 2)>();
  } else {
    vm_wait<0>();
  }
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  // Ping-pong (flags & 8, 8-wave tiles): every step is a read section (fragments + next DMA)
  // and an MFMA section, each closed by a barrier; waves 4-7 start one barrier late, so on
  // every SIMD (waves w and w+4 share one) one wave's MFMAs overlap the other's LDS reads.
  if (pingpong && wid >= 4) __builtin_amdgcn_s_barrier();
  if constexpr (STAGES == 3) {
    for (int ks = 0; ks < nK; ks += 3) {
      step(I0{}, I2{}, ks);
      if (ks + 1 >= nK) break;
      step(I1{}, I0{}, ks + 1);
      if (ks + 2 >= nK) break;
      step(I2{}, I1{}, ks + 2);
    }
  } else {
    for (int ks = 0; ks < nK; ks += 2) {
      step(I0{}, I1{}, ks);
      if (ks + 1 >= nK) break;
      step(I1{}, I0{}, ks + 1);
    }
  }

  if (pingpong && wid < 4) __builtin_amdgcn_s_barrier();  // same barrier count for both groups

  // (lds0 as the epilogue's LDS scratch: the BN partials of the tile's wave halves meet there)
  conv_epilogue<T, WC, WP, NWP>(A, S, acc, p0, c0, wc, wp, lane, M, GHW, bx, blockIdx.z, gridDim.z, TG.rflag,
                                (float*)lds0);
}

// ------------------------------------------------------------------------------------
// 3x3 stride-1 convolution with activation-strip reuse (bf16).  k_conv stages the activation
// rows of every tap separately: 9 shifted copies of nearly the same rows per channel chunk, and
// the L2 -> LDS stream (not the MFMA) bounds it (profiles/r01_conv_sweep.md ablations).  Here a
// tile is TR full image rows (TP = TR * W = 256 pixels) and, per (tap row, 64-channel chunk), ONE
// strip of TR x (W + 2d) input pixels is staged and read by the three taps of that row at column
// offsets 0, d, 2d: 3 strips + 9 weight tiles per chunk instead of 9 + 9 tiles.
// K steps run (tap row, chunk, tap column), tap column fastest.  Weights: STAGES-deep ring as
// k_conv; strips: 2-deep ring, each strip issued two steps ahead of its first use.  Every wave
// issues the same number of LDS-DMA instructions per step (padding rows load zeros), so the
// counted vmcnt waits stay exact.  Epilogue shared with k_conv.
// ------------------------------------------------------------------------------------
struct strip_geo {
  int W, TR, SW, SR, SPW;       // width, rows per tile, strip width W + 2d, strip rows, DMA instrs / wave
  int ty0, dty, tx0, dtx, pad;  // tap grid (3 x 3) and the halo width pad = max |offset|
  unsigned x_bytes, w_bytes;
};

template <typename T, int WC, int STAGES, int SPW>
__global__ void __launch_bounds__(512) k_conv_strip(const zp_conv_args A, const strip_geo SG, const int flags) {
  constexpr int WP = 4, NWP = 4, NW = 8;
  constexpr int TC = 32 * WC, TP = 256;
  constexpr int WPW = TC / 8 / NW;  // weight DMA instrs per wave per step
  constexpr int SRP = 64 * SPW;     // strip rows incl. padding (8 waves x SPW instrs x 8 rows)
  static_assert(STAGES == 2 || STAGES == 3, "weight ring");
  // weight ring and strip ring; slots are runtime indices (ks % STAGES, group & 1): the loop is
  // unrolled only over the 3 tap columns of a group (compile-time wait counts), which keeps the
  // 256-channel variant inside the register file
  __shared__ uint4 wring[STAGES * TC * 8];
  __shared__ uint4 sring[2 * SRP * 8];
  auto wbuf = [&](int slot) -> uint4* { return wring + slot * (TC * 8); };
  auto sbuf = [&](int slot) -> uint4* { return sring + slot * (SRP * 8); };
  const zp_conv_sub& S = A.sub[0];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wid / NWP, wp = wid % NWP;
  const int GHW = A.GH * A.GW;
  const int M = A.N * GHW;
  int bx = blockIdx.x, by = blockIdx.y;
  if (flags & 2) {
    // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs (bid % 8 share one L2).
    // Give each XCD a contiguous run of (pixel tile, cout tile) pairs, cout tiles fastest, so the
    // cout tiles of one pixel tile (same strip) and neighbouring pixel tiles (shared halo rows)
    // are served by the same L2 instead of each fetching its strip from beyond it.  Bijective for
    // any total (cdna_hip_programming.md T1).
    const int total = gridDim.x * gridDim.y;
    const int bid = blockIdx.x + gridDim.x * blockIdx.y;
    const int xcd = bid & 7, pos = bid >> 3, q = total >> 3, r = total & 7;
    const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
    bx = lin / gridDim.y;
    by = lin - bx * gridDim.y;
  }
  const int p0 = bx * TP, c0 = by * TC;
  const int n_img = p0 / GHW, y0 = (p0 - n_img * GHW) / SG.W;
  const int CB = A.Cin / 64;
  const int nK = 9 * CB;
  const int lrow = lane >> 3;
  const int csrc = (lane & 7) ^ lrow;  // weight rows: swizzle by (row & 7) = lrow

#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)A.x, (short)0, (int)SG.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)S.w, (short)0, (int)SG.w_bytes, 0x00020000);
#endif
  // weight rows of this lane: row c0 + (wid + NW*i)*8 + lrow
  const unsigned wbase = (unsigned)(((size_t)(c0 + wid * 8 + lrow) * A.k_pad + csrc * 8) * 2);
  // strip rows of this lane: s = (wid + 8 i) * 8 + lrow -> (tr, c); input (n, y0 + ty + tr, c - pad)
  // per strip instruction: the byte offset of the row's (tr, column) with tr packed into the low
  // 4 bits (offsets are 16-byte multiples; tr < 16), or -1 for padding rows / columns
  int sbase[SPW];
  const int rowb = A.IW * A.ldx * 2;  // bytes per input row
#pragma unroll
  for (int i = 0; i < SPW; ++i) {
    const int srow = (wid + 8 * i) * 8 + lrow;
    const int tr = srow / SG.SW, c = srow - tr * SG.SW;
    const int ix = c - SG.pad;
    const bool ok = srow < SG.SR && (unsigned)ix < (unsigned)A.IW;
    const int sw = (lane & 7) ^ (srow & 7);  // source-side chunk swizzle by the strip row
    sbase[i] = ok ? ((((n_img * A.IH + y0 + tr) * A.IW + ix) * A.ldx + A.cx0 + sw * 8) * 2) | tr : -1;
  }
  auto issue_w = [&](int ks, uint4* dst) {
    const int g = ks / 3, kx = ks - 3 * g, ky = g / CB, cb = g - ky * CB;
    const int koff = ((ky * 3 + kx) * A.Cin + cb * 64) * 2;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
      auto* d = (__attribute__((address_space(3))) void*)&dst[(wid + NW * i) * 64];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, d, 16, wbase + (unsigned)(NW * i * 8) * (unsigned)(A.k_pad * 2),
                                               koff, 0, 0);
    }
#endif
  };
  // strip pieces [I0, I1) of group g (all SPW pieces by default)
  auto issue_s = [&](int g, uint4* dst, auto i0_c, auto i1_c) {
    constexpr int I0 = decltype(i0_c)::value, I1 = decltype(i1_c)::value;
    const int ky = g / CB, cb = g - ky * CB;
    const int ty = SG.ty0 + ky * SG.dty;
    unsigned voff[SPW];
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      const int tr = sbase[i] & 15;
      const bool ok = sbase[i] >= 0 && (unsigned)(y0 + ty + tr) < (unsigned)A.IH;
      voff[i] = ok ? (unsigned)((sbase[i] & ~15) + ty * rowb + cb * 128) : 0x80000000u;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      auto* d = (__attribute__((address_space(3))) void*)&dst[(wid + 8 * i) * 64];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, d, 16, voff[i], 0, 0, 0);
    }
#endif
  };
  using C0 = std::integral_constant<int, 0>;
  using CS = std::integral_constant<int, SPW>;

  f32x4 acc[WC][WP];
#pragma unroll
  for (int i = 0; i < WC; ++i)
#pragma unroll
    for (int j = 0; j < WP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment offsets: A (weights) as in k_conv; B from the strip: pixel q = wp*64 + j*16 + (lane&15)
  // -> strip row tr*SW + x + (tx + pad), chunk swizzled by that row
  unsigned aoff[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
    aoff[s2] = (unsigned)(wc * 16 * WC + (lane & 15)) * 128u + (unsigned)(((s2 * 4 + (lane >> 4)) ^ (lane & 7)) * 16);
  // strip row of fragment j = bsrow0 + jdelta(j): the wave's 64 pixels are one image row when
  // W >= 64, two rows of 32 when W == 32
  int bsrow0;
  {
    const int q0 = wp * 16 * WP;
    const int tr = q0 / SG.W, x0 = q0 - tr * SG.W;
    bsrow0 = tr * SG.SW + x0 + (lane & 15) + SG.pad;
  }
  const int jrow = SG.W == 32 ? SG.SW - 32 : 0;  // extra offset for fragments 2, 3 when W == 32
  const bool pingpong = (flags & 8) != 0;
  // flags & 32 (3-stage ring only): the next group's strip DMA is spread over the three steps of the
  // current group (pieces [0,N0) | [N0,N0+N1) | [N0+N1,SPW)) instead of all SPW pieces in one step,
  // so no read section carries SPW + WPW LDS-DMA issues (~60-180 cycles each) at once
  const bool spread = STAGES == 3 && (flags & 32) != 0;
  constexpr int N0 = (SPW + 2) / 3, N1 = (SPW + 1) / 3;

  // step phase PH = ks % 3 = tap column (compile-time); weight slot ks % STAGES, strip slot g & 1
  auto step = [&](auto ph_c, int ks) {
    constexpr int PH = decltype(ph_c)::value;
    const bool more_w = ks + (STAGES - 1) < nK;
    const bool strip_next = ((PH + 2) % 3 == 0) && ks + 2 < nK;
    const int gnext = ks / 3 + 1;
    const bool has_next = gnext * 3 < nK;  // the next group exists (its strip is staged by this group)
    if (!spread) {
      // (diagnostic builds: ZP_ABL 1 = no DMA in the loop, 3 = weights only, 4 = strips only)
      if (ZP_ABL != 1 && ZP_ABL != 4 && more_w) issue_w(ks + (STAGES - 1), wbuf((ks + STAGES - 1) % STAGES));
      if (ZP_ABL != 1 && ZP_ABL != 3 && strip_next) issue_s((ks + 2) / 3, sbuf(((ks + 2) / 3) & 1), C0{}, CS{});
    } else if constexpr (PH == 0) {
      if (more_w) issue_w(ks + 2, wbuf((ks + 2) % 3));
      if (has_next) issue_s(gnext, sbuf(gnext & 1), C0{}, std::integral_constant<int, N0>{});
    } else if constexpr (PH == 1) {
      if (more_w) issue_w(ks + 2, wbuf((ks + 2) % 3));
      if (has_next) issue_s(gnext, sbuf(gnext & 1), std::integral_constant<int, N0>{},
                            std::integral_constant<int, N0 + N1>{});
    } else {
      if (has_next) issue_s(gnext, sbuf(gnext & 1), std::integral_constant<int, N0 + N1>{}, CS{});
      if (more_w) issue_w(ks + 2, wbuf((ks + 2) % 3));
    }
    const int g = ks / 3;
    const int txo = SG.tx0 + PH * SG.dtx;
    const unsigned cw = lds_addr(wbuf(ks % STAGES));
    const unsigned csb = lds_addr(sbuf(g & 1));
    // loads allowed to stay in flight at the end of this step: the ones issued for later steps
    constexpr int OUT_S2 = ((PH + 2) % 3 == 0) ? SPW : 0;  // strip issued this step (needed at ks + 2)
    constexpr int OUT = (STAGES == 3 ? WPW : 0) + OUT_S2;
    // (a step whose strip slot would have been refilled past the end issued no strip)
    auto wait_out = [&]() {
      if (spread) {
        // loads allowed in flight: this step's weights (for ks + 2) and the pieces of the next
        // strip issued after the weights of step ks + 1, except in the group's last step
        if constexpr (PH == 0) {
          if (more_w && has_next) vm_wait<WPW + N0>();
          else if (more_w) vm_wait<WPW>();
          else if (has_next) vm_wait<N0>();
          else vm_wait<0>();
        } else if constexpr (PH == 1) {
          if (more_w && has_next) vm_wait<WPW + N0 + N1>();
          else if (more_w) vm_wait<WPW>();
          else if (has_next) vm_wait<N0 + N1>();
          else vm_wait<0>();
        } else {
          if (more_w) vm_wait<WPW>();
          else vm_wait<0>();
        }
        return;
      }
      if (strip_next) vm_wait<OUT>();
      else if (more_w) vm_wait<OUT - OUT_S2>();
      else vm_wait<0>();
    };
    uint4 af[2][WC], bfr[2][WP];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const unsigned pa = cw + aoff[s2];
      static_for<WC>([&](auto i) { af[s2][i] = ds_read16<i * 2048>(pa); });
#pragma unroll
      for (int j = 0; j < WP; ++j) {
        const int sr = bsrow0 + txo + 16 * j + (j >= 2 ? jrow : 0);
        const unsigned pb = csb + (unsigned)sr * 128u + (unsigned)((((s2 * 4 + (lane >> 4)) ^ (sr & 7))) * 16);
        bfr[s2][j] = ds_read16<0>(pb);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (pingpong) {
      wait_out();
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(1);
    if constexpr (ZP_ABL != 2) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int i = 0; i < WC; ++i)
#pragma unroll
          for (int j = 0; j < WP; ++j) MfmaTraits<T>::mma(acc[i][j], af[s2][i], bfr[s2][j]);
    } else {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int i = 0; i < WC; ++i)
#pragma unroll
          for (int j = 0; j < WP; ++j) acc[i][j][0] += __uint_as_float(af[s2][i].x ^ bfr[s2][j].y);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    if (!pingpong) wait_out();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  // prologue: strip of group 0, weights of steps 0 .. STAGES-2; the strip of group 1 is issued
  // at step 1 (two steps ahead of step 3)
  issue_s(0, sbuf(0), C0{}, CS{});
  issue_w(0, wbuf(0));
  if (STAGES == 3) issue_w(1, wbuf(1));
  if (STAGES == 3) vm_wait<WPW>();  // strip(0) and weights(0) landed; weights(1) may be in flight
  else vm_wait<0>();
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if (pingpong && wid >= 4) __builtin_amdgcn_s_barrier();
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  for (int ks = 0; ks < nK; ks += 3) {  // nK = 9 CB: whole groups
    step(P0{}, ks);
    step(P1{}, ks + 1);
    step(P2{}, ks + 2);
  }
  if (pingpong && wid < 4) __builtin_amdgcn_s_barrier();
  conv_epilogue<T, WC, WP, NWP>(A, S, acc, p0, c0, wc, wp, lane, M, GHW, bx, blockIdx.z, gridDim.z);
}

// ------------------------------------------------------------------------------------
// k_conv_strip2: k_conv_strip's algorithm (same staging, same K order, bit-identical results)
// with a lean main loop.  Profiling k_conv_strip (256 -> 256 at 128 x 128, bs 32) showed the
// read section of every step -- not the MFMAs, not L2 / HBM -- as the critical path: the MFMA-free
// ablation ran exactly as long as the full kernel, and each step issued ~65 SALU (runtime
// divisions for the tap / chunk / slot of every DMA, a branch tree of counted waits) and ~70 VALU
// (per-step fragment and DMA address arithmetic, an SGPR-spilled buffer descriptor rebuilt with
// v_readlane) besides its 16 ds_reads and 2-7 LDS-DMAs.  Here:
//   * the loop is unrolled by group parity x tap column, so every LDS address is a per-lane base
//     register + an immediate (weight slot = tap column, strip slot = group parity) and every wait
//     count is a constant; the steady-state groups (all of whose steps prefetch) are separated
//     from the last group, so the loop body has no prefetch conditions;
//   * DMA offsets are per-lane registers computed once (weights: row offsets; strips: one per tap
//     row and piece) plus a scalar offset advanced by additions (no divisions);
//   * one __shared__ array (weights ring, then strip ring).
// ------------------------------------------------------------------------------------
template <typename T, int WC, int WP, int NWP>
__device__ __forceinline__ void head_epilogue16(const zp_conv_args& A, const zp_conv_sub& S, const zp_head_args& H,
                                                f32x4 (&acc)[WC][WP], int p0, int c0, int by, int wc, int wp,
                                                int lane, int M, uint4* lds);

// HEAD (zp_conv2d_head, 16-bit eval): the conv output is not stored; it feeds the fused 1x1 head's
// partial sums over this tile's channels (head_epilogue16)
template <typename T, int WC, int SPW, int DM, bool HEAD = false, bool BNR = false>
__global__ void __launch_bounds__(512) k_conv_strip2(const zp_conv_args A, const strip_geo SG, const int flags,
                                                     const zp_head_args H) {
  // DM: where the next group's strip DMA is issued.  0: the read section of tap column 1; 1: spread
  // over the read sections of the group's three steps; 2: between the MFMAs of tap column 0 (the
  // read sections then carry only the weight pieces: the LDS-DMA issue cost, ~60 cycles per piece
  // among bare MFMAs but 100-185 inside a read section already holding 16 ds_read_b128, leaves the
  // critical path of the ping-pong schedule, and the strip is issued one phase earlier)
  constexpr bool SPREAD = DM == 1, MSEC = DM == 2;
  constexpr int WP = 4, NWP = 4, NW = 8;
  constexpr int TC = 32 * WC, TP = 256;
  constexpr int WPW = TC / 8 / NW;  // weight DMA instrs per wave per step
  constexpr int SRP = 64 * SPW;     // strip rows incl. padding
  constexpr int WSLOT = TC * 128;   // bytes per weight slot (3 slots)
  constexpr int SSLOT = SRP * 128;  // bytes per strip slot (2 slots)
  static_assert(SSLOT < 65536 && 2 * WSLOT + 2048 * (WC - 1) < 65536, "ds_read immediate range");
  __shared__ uint4 lds[(3 * TC + 2 * SRP) * 8];
  const zp_conv_sub& S = A.sub[0];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wid / NWP, wp = wid % NWP;
  const int GHW = A.GH * A.GW;
  const int M = A.N * GHW;
  int bx = blockIdx.x, by = blockIdx.y;
  if (flags & 2) {  // XCD-aware order, as k_conv_strip
    const int total = gridDim.x * gridDim.y;
    const int bid = blockIdx.x + gridDim.x * blockIdx.y;
    const int xcd = bid & 7, pos = bid >> 3, q = total >> 3, r = total & 7;
    const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
    bx = lin / gridDim.y;
    by = lin - bx * gridDim.y;
  }
  const int p0 = bx * TP, c0 = by * TC;
  const int n_img = p0 / GHW, y0 = (p0 - n_img * GHW) / SG.W;
  const int CB = A.Cin / 64;
  const int lrow = lane >> 3;
  const int csrc = (lane & 7) ^ lrow;

#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)A.x, (short)0, (int)SG.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)S.w, (short)0, (int)SG.w_bytes, 0x00020000);
#endif
  // weight DMA: per-lane row offsets (piece i = rows (wid + NW i) * 8 + lrow); the K offset of a
  // step is scalar: koff = (ky * 3 + kx) * Cin * 2 + cb * 128
  unsigned wv[WPW];
#pragma unroll
  for (int i = 0; i < WPW; ++i)
    wv[i] = (unsigned)(((size_t)(c0 + (wid + NW * i) * 8 + lrow) * A.k_pad + csrc * 8) * 2);
  const int cin2 = A.Cin * 2;
  // strip DMA: per piece and tap row ky, the lane's source byte offset (chunk 0) or an offset past
  // the buffer end (zeros) for padding rows / columns; the chunk's cb * 128 goes in the scalar offset
  const int rowb = A.IW * A.ldx * 2;
  // pk[i]: the piece's 16-byte-aligned source offset for tap row 0 with a 3-bit "row inside the
  // image" mask per tap row in the low bits; svn[i]: the offsets for the next strip's tap row,
  // recomputed (a few VALU per piece) only when that tap row changes, i.e. 3 times per workgroup
  unsigned pk[SPW], svn[SPW];
#pragma unroll
  for (int i = 0; i < SPW; ++i) {
    const int srow = (wid + 8 * i) * 8 + lrow;
    const int tr = srow / SG.SW, c = srow - tr * SG.SW;
    const int ix = c - SG.pad;
    const bool ok = srow < SG.SR && (unsigned)ix < (unsigned)A.IW;
    const int sw = (lane & 7) ^ (srow & 7);
    const int base = (((n_img * A.IH + y0 + tr) * A.IW + ix) * A.ldx + A.cx0 + sw * 8) * 2 + SG.ty0 * rowb;
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      m |= (unsigned)(ok && (unsigned)(y0 + SG.ty0 + k * SG.dty + tr) < (unsigned)A.IH) << k;
    pk[i] = (unsigned)base | m;
  }
  const int dtyb = SG.dty * rowb;
  auto set_svn = [&](int k) {
#pragma unroll
    for (int i = 0; i < SPW; ++i)
      svn[i] = (pk[i] >> k) & 1u ? (pk[i] & ~15u) + (unsigned)(k * dtyb) : 0x80000000u;
  };
  const unsigned lds0 = lds_addr(lds);
  // fragment bases: A (weights) row wc*16*WC + (lane & 15), swizzled chunk; + slot * WSLOT + i * 2048
  unsigned aoff[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
    aoff[s2] = lds0 + (unsigned)(wc * 16 * WC + (lane & 15)) * 128u + (unsigned)(((s2 * 4 + (lane >> 4)) ^ (lane & 7)) * 16);
  // B (strip) per tap column PH, half s2, pixel fragment j; + parity * SSLOT
  unsigned bo[3][2][WP];
  {
    const int q0 = wp * 16 * WP;
    const int tr = q0 / SG.W, x0 = q0 - tr * SG.W;
    const int bsrow0 = tr * SG.SW + x0 + (lane & 15) + SG.pad;
    const int jrow = SG.W == 32 ? SG.SW - 32 : 0;
#pragma unroll
    for (int ph = 0; ph < 3; ++ph)
#pragma unroll
      for (int j = 0; j < WP; ++j) {
        const int sr = bsrow0 + SG.tx0 + ph * SG.dtx + 16 * j + (j >= 2 ? jrow : 0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
          bo[ph][s2][j] = lds0 + 3u * WSLOT + (unsigned)sr * 128u + (unsigned)(((s2 * 4 + (lane >> 4)) ^ (sr & 7)) * 16);
      }
  }
  const bool pingpong = (flags & 8) != 0;

  auto issue_w = [&](int slot, int koff) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
      auto* d = (__attribute__((address_space(3))) void*)&lds[(slot * TC + (wid + NW * i) * 8) * 8];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, d, 16, wv[i], koff, 0, 0);
    }
#endif
  };
  constexpr int N0 = (SPW + 2) / 3, N1 = (SPW + 1) / 3;  // SPREAD: pieces per step (PH 0 / 1 / 2 = rest)
  auto issue_s = [&](int slot, int cb, auto i0_c, auto i1_c) {  // pieces [I0, I1) of the strip svn holds
    constexpr int I0 = decltype(i0_c)::value, I1 = decltype(i1_c)::value;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      auto* d = (__attribute__((address_space(3))) void*)&lds[(3 * TC + slot * SRP + (wid + 8 * i) * 8) * 8];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, d, 16, svn[i], cb * 128, 0, 0);
    }
#endif
  };

  f32x4 acc[WC][WP];
#pragma unroll
  for (int i = 0; i < WC; ++i)
#pragma unroll
    for (int j = 0; j < WP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // one K step: tap column PH of a group with strip parity GP.  Prefetch (issued first): PH 0 the
  // weights of (this group, column 2) -> slot 2; PH 1 the weights of (next group, column 0) -> slot 0
  // and the next group's strip -> slot GP ^ 1; PH 2 the weights of (next group, column 1) -> slot 1.
  // Waits: what the next step reads must have landed.
  auto step = [&](auto gp_c, auto ph_c, auto steady_c, int koff_cur, int koff_next, int ncb) {
    constexpr int GP = decltype(gp_c)::value, PH = decltype(ph_c)::value;
    constexpr bool STEADY = decltype(steady_c)::value;
    using Z = std::integral_constant<int, 0>;
    using K0 = std::integral_constant<int, N0>;
    using K1 = std::integral_constant<int, N0 + N1>;
    using KS = std::integral_constant<int, SPW>;
    if constexpr (ZP_ABL == 1) {  // diagnostic build: no DMA in the loop
    } else if constexpr (!SPREAD) {
      if constexpr (PH == 0) {
        issue_w(2, koff_cur + 2 * cin2);
      } else if constexpr (STEADY && PH == 1) {
        issue_w(0, koff_next);
        if constexpr (!MSEC) issue_s(GP ^ 1, ncb, Z{}, KS{});
      } else if constexpr (STEADY && PH == 2) {
        issue_w(1, koff_next + cin2);
      }
    } else {
      // the next strip in three parts; issue order weights-then-strip (PH 0, 1), strip-then-weights
      // (PH 2) so each counted wait below retires exactly what the next step reads
      if constexpr (PH == 0) {
        issue_w(2, koff_cur + 2 * cin2);
        if constexpr (STEADY) issue_s(GP ^ 1, ncb, Z{}, K0{});
      } else if constexpr (STEADY && PH == 1) {
        issue_w(0, koff_next);
        issue_s(GP ^ 1, ncb, K0{}, K1{});
      } else if constexpr (STEADY && PH == 2) {
        issue_s(GP ^ 1, ncb, K1{}, KS{});
        issue_w(1, koff_next + cin2);
      }
    }
    uint4 af[2][WC], bfr[2][WP];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      static_for<WC>([&](auto i) { af[s2][i] = ds_read16<PH * WSLOT + i * 2048>(aoff[s2]); });
      static_for<WP>([&](auto j) { bfr[s2][j] = ds_read16<GP * SSLOT>(bo[PH][s2][j]); });
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    auto wait_out = [&]() {
      // (MSEC without ping-pong: the wait follows the MFMA section, i.e. this step's strip issue)
      if constexpr (MSEC && PH == 0 && STEADY) {
        if (pingpong) vm_wait<WPW>();
        else vm_wait<WPW + SPW>();
      } else if constexpr (PH == 0) vm_wait<WPW + (SPREAD && STEADY ? N0 : 0)>();
      else if constexpr (STEADY && PH == 1) vm_wait<WPW + (SPREAD ? N0 + N1 : SPW)>();
      else if constexpr (STEADY && PH == 2) vm_wait<WPW>();
      else vm_wait<0>();
    };
    if (pingpong) {
      wait_out();
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(1);
    if constexpr (ZP_ABL != 2) {
      // MSEC, tap column 0 of a steady group: strip piece k after MFMA SP (k + 1) - 1
      constexpr int NM = 2 * WC * WP, SP = NM / (SPW + 1);
      static_for<NM>([&](auto t_c) {
        constexpr int t = decltype(t_c)::value;
        constexpr int s2 = t / (WC * WP), i = (t / WP) % WC, j = t % WP;
        MfmaTraits<T>::mma(acc[i][j], af[s2][i], bfr[s2][j]);
        if constexpr (MSEC && PH == 0 && STEADY && ZP_ABL != 1 && (t + 1) % SP == 0 && (t + 1) / SP <= SPW) {
          constexpr int k = (t + 1) / SP - 1;
          __builtin_amdgcn_sched_barrier(0);  // pin the piece between MFMAs t and t + 1
          issue_s(GP ^ 1, ncb, std::integral_constant<int, k>{}, std::integral_constant<int, k + 1>{});
          __builtin_amdgcn_sched_barrier(0);
        }
      });
    } else {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int i = 0; i < WC; ++i)
#pragma unroll
          for (int j = 0; j < WP; ++j) acc[i][j][0] += __uint_as_float(af[s2][i].x ^ bfr[s2][j].y);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    if (!pingpong) wait_out();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  using G0 = std::integral_constant<int, 0>;
  using G1 = std::integral_constant<int, 1>;
  using ST = std::integral_constant<bool, true>;
  using TL = std::integral_constant<bool, false>;
  auto group = [&](auto gp_c, auto steady_c, int koff_cur, int koff_next, int ncb) {
    step(gp_c, P0{}, steady_c, koff_cur, koff_next, ncb);
    step(gp_c, P1{}, steady_c, koff_cur, koff_next, ncb);
    step(gp_c, P2{}, steady_c, koff_cur, koff_next, ncb);
  };

  // groups (ky, cb), cb fastest; koff of (ky, cb, kx = 0) = ky * 3 * Cin * 2 + cb * 128
  int ky = 0, cb = 0;
  auto koff_of = [&](int a, int b) { return a * 3 * cin2 + b * 128; };
  // the next group (its strip is staged during the current one); svn follows its tap row
  int nky = 0, ncb = 0;
  auto advance_next = [&]() {
    if (++ncb == CB) {
      ncb = 0;
      ++nky;
      if (nky < 3) set_svn(nky);
    }
  };
  // prologue: strip of group 0, weights of steps 0 and 1
  set_svn(0);
  issue_s(0, 0, std::integral_constant<int, 0>{}, std::integral_constant<int, SPW>{});
  issue_w(0, 0);
  issue_w(1, cin2);
  vm_wait<WPW>();
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if (pingpong && wid >= 4) __builtin_amdgcn_s_barrier();
  const int ng = 3 * CB;
  advance_next();
  int g = 0;
  for (; g + 2 <= ng - 1; g += 2) {
    group(G0{}, ST{}, koff_of(ky, cb), koff_of(nky, ncb), ncb);
    ky = nky;
    cb = ncb;
    advance_next();
    group(G1{}, ST{}, koff_of(ky, cb), koff_of(nky, ncb), ncb);
    ky = nky;
    cb = ncb;
    advance_next();
  }
  if (g < ng - 1) {
    group(G0{}, ST{}, koff_of(ky, cb), koff_of(nky, ncb), ncb);
    ky = nky;
    cb = ncb;
    ++g;
  }
  if (g & 1) group(G1{}, TL{}, koff_of(ky, cb), 0, 0);
  else group(G0{}, TL{}, koff_of(ky, cb), 0, 0);
  if (pingpong && wid < 4) __builtin_amdgcn_s_barrier();
  if constexpr (ZP_ABL == 5) {  // diagnostic build: no epilogue (one store only if a sum is exactly 1)
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < WC; ++i)
#pragma unroll
      for (int j = 0; j < WP; ++j) sm += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
    if (sm == 1.f) ((float*)S.y)[tid] = sm;
  } else if constexpr (HEAD) {
    head_epilogue16<T, WC, WP, NWP>(A, S, H, acc, p0, c0, by, wc, wp, lane, M, lds);
  } else {
    conv_epilogue<T, WC, WP, NWP, BNR>(A, S, acc, p0, c0, wc, wp, lane, M, GHW, bx, blockIdx.z, gridDim.z, nullptr,
                                       (float*)lds);
  }
}

// The fused head's epilogue for the 16-bit strip tile (ZP_BF16 / ZP_F16 eval; zp_conv2d_head): the
// tile's TC = 32 WC output channels of 256 pixels, after BN scale / shift, residual and ReLU and
// rounded to the storage type exactly as the unfused path stores them, are the B operand of the head's
// 16 x 16 x 32 MFMAs: the paired lane layout (v_permlane16_swap of cout blocks i, i + 1: a lane holds
// 8 consecutive channels of one pixel) is a B fragment when lane group g is read as k slot g, so the
// head weights are read with the same channel permutation (k slot g <-> channel (g & 1) * 16 +
// (g >> 1) * 8 of the 32-channel slice).  The first cout tile also adds x2 (x_128) at k = Cout + c.
// The two wave rows (wc) of a pixel quarter meet in LDS; the tile's partial sums (rows r < hcout,
// f32) go to H.ws[by][r][p]; k_head_combine16 adds the cout tiles in order, plus the bias.
template <typename T, int WC, int WP, int NWP>
__device__ __forceinline__ void head_epilogue16(const zp_conv_args& A, const zp_conv_sub& S, const zp_head_args& H,
                                                f32x4 (&acc)[WC][WP], int p0, int c0, int by, int wc, int wp,
                                                int lane, int M, uint4* lds) {
  static_assert(WC % 2 == 0, "paired cout blocks");
  using MT = MfmaTraits<T>;
  const int g = lane >> 4, lr = lane & 15;
  const int GHW = S.OH * S.OW;
  f32x4 hacc[2][WP];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int j = 0; j < WP; ++j) hacc[hb][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const T* W = (const T*)H.w;
  // head weight fragment: rows hb * 16 + lr, the 8 k of lane group g (k = kbase + perm)
  auto wfrag = [&](int hb, int k) -> uint4 { return *(const uint4*)(W + (size_t)(hb * 16 + lr) * H.k_pad + k); };
#pragma unroll
  for (int i = 0; i < WC; i += 2) {
    const int cs = c0 + wc * 16 * WC + (i + (g & 1)) * 16 + (g >> 1) * 8;  // this lane's 8 channels
    float sc[8], sh[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      sc[r] = S.scale ? S.scale[cs + r] : 1.f;
      sh[r] = S.shift ? S.shift[cs + r] : 0.f;
    }
    const uint4 w0 = wfrag(0, cs), w1 = wfrag(1, cs);
#pragma unroll
    for (int j = 0; j < WP; ++j) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // all lanes active (cross-lane op)
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][j][r]), __float_as_uint(acc[i + 1][j][r]),
                                                         false, false);
        v[r] = __uint_as_float(sw[0]);
        v[r + 4] = __uint_as_float(sw[1]);
      }
      const int p = p0 + wp * 16 * WP + j * 16 + lr;
      const bool ok = p < M;
      const size_t pix = ok ? (size_t)p : 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = v[r] * sc[r] + sh[r];
      if (A.res) {
        const uint4 rv = *(const uint4*)((const unsigned short*)A.res + pix * A.ldr + A.cr0 + cs);
        const uint32_t rw[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[2 * r] += H16<T>::from(rw[r] & 0xffffu);
          v[2 * r + 1] += H16<T>::from(rw[r] >> 16);
        }
      }
      if (A.relu) {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      uint32_t o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = ok ? (H16<T>::to(v[2 * r]) | (H16<T>::to(v[2 * r + 1]) << 16)) : 0u;
      const uint4 xb = make_uint4(o[0], o[1], o[2], o[3]);
      MT::mma(hacc[0][j], w0, xb);
      MT::mma(hacc[1][j], w1, xb);
    }
  }
  if (by == 0 && wc == 0) {  // x2 (the skip features, NHWC on the output grid), weights at k = Cout + c
    for (int q = 0; q < H.C2 / 32; ++q) {
      const uint4 w0 = wfrag(0, A.Cout + q * 32 + g * 8), w1 = wfrag(1, A.Cout + q * 32 + g * 8);
#pragma unroll
      for (int j = 0; j < WP; ++j) {
        const int p = p0 + wp * 16 * WP + j * 16 + lr;
        const uint4 xq = p < M ? *(const uint4*)((const unsigned short*)H.x2 + (size_t)p * H.ldx2 + H.cx20 + q * 32 + g * 8)
                               : make_uint4(0u, 0u, 0u, 0u);
        MT::mma(hacc[0][j], w0, xq);
        MT::mma(hacc[1][j], w1, xq);
      }
    }
  }
  // the wave rows' sums meet in LDS (free: every wave passed the main loop's last barrier)
  f32x4* red = (f32x4*)lds;  // [wp][hb][j][lane]
  if (wc != 0) {
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int j = 0; j < WP; ++j) red[((wp * 2 + hb) * WP + j) * 64 + lane] = hacc[hb][j];
  }
  __syncthreads();
  if (wc != 0) return;
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int j = 0; j < WP; ++j) {
      const f32x4 o = red[((wp * 2 + hb) * WP + j) * 64 + lane];
      const int p = p0 + wp * 16 * WP + j * 16 + lr;
      if (p >= M) continue;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int r = hb * 16 + g * 4 + qq;
        if (r < H.cout) H.ws[((size_t)by * 32 + r) * M + p] = hacc[hb][j][qq] + o[qq];
      }
    }
  (void)GHW;
}

// the fused 16-bit head's second launch: mask / code = ws[0] + ws[1] (the two cout tiles, in that
// order) + bias, f32 NCHW (one thread per output pixel)
__global__ void k_head_combine16(const float* __restrict__ ws, int M, int GHW, int hcout, const float* __restrict__ bias,
                                 float* __restrict__ mask, float* __restrict__ code) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= M) return;
  const int n = p / GHW, sp = p - n * GHW;
  for (int r = 0; r < hcout; ++r) {
    const float v = (ws[(size_t)r * M + p] + ws[((size_t)32 + r) * M + p]) + (bias ? bias[r] : 0.f);
    if (r == 0) mask[(size_t)n * GHW + sp] = v;
    else code[((size_t)n * (hcout - 1) + (r - 1)) * GHW + sp] = v;
  }
}

// ------------------------------------------------------------------------------------
// k_conv_quad: the four sub-pixel phases of a stride-2 transposed structure in ONE tile.
// ConvTranspose2d(3, s2, p1, op1) (model/aspp.py:60-80) -- and the data gradient of a 3x3 stride-2
// conv, which geometry.py plans the same way -- is four stride-1 sub-problems over the same input
// grid, output phase (py, px) at (2 gy + py, 2 gx + px), with 1 / 2 / 2 / 4 taps whose input offsets
// (dy, dx) all lie in {0, 1}^2.  k_conv runs them as four independent tiles (blockIdx.z) that each
// stage their own shifted copies of the input: 9 activation tiles per 64-channel chunk for the 9
// (phase, tap) pairs, and the four phases of one pixel tile land on different XCDs, so the re-staging
// goes to HBM (r01 PMC: 761 MB read per up2 launch against 85 MB algorithmic).
// Here a workgroup owns 256 grid points (TR = 256 / W full rows) x 64 output channels x ALL FOUR
// phases: per chunk it stages ONE strip of (TR + 1) x W input pixels (the +1 row / column of the
// (dy, dx) = 1 taps; column W is outside the image, so the lane that would read it gets zeros by a
// register select instead of a staged padding column) and the 9 weight taps, and every (phase, tap)
// reads its operand from the strip at offset dy * W + dx.
// Per chunk, 5 K steps grouped by input shift (B fragments read once per step):
//   step 0: shift 00, phases 0, 1   step 1: shift 00, phases 2, 3   step 2: shift 01, phases 1, 3
//   step 3: shift 10, phases 2, 3   step 4: shift 11, phase 3
// Weights: one 8 KB LDS slot per (phase, tap) (9 slots, 72 KB); at the start of step s the slots of
// step s - 1 are refilled with the next chunk's taps (4 steps of lead).  Strips: 2-slot ring, the
// next chunk's strip issued at step 0.  8 waves = 2 (32 channels) x 4 (64 grid points), each holding
// 4 phases x 2 x 4 MFMA tiles (128 accumulator registers).  Schedule (ping-pong wave groups, setprio,
// counted vmcnt waits, XCD-aware order) as k_conv_strip2.  Epilogue: k_conv's, once per phase.
// ------------------------------------------------------------------------------------
struct quad_geo {
  unsigned x_bytes, w_bytes;
  int koff[9];  // byte offset of the slot's tap in a packed weight row: local tap index * Cin * 2
};
// slot -> phase (sub-problem) and input shift (host table: quad_plan)
__host__ __device__ constexpr int quad_phase(int slot) { return slot == 0 ? 0 : slot == 1 || slot == 4 ? 1 : slot == 2 || slot == 6 ? 2 : 3; }

template <typename T, int W, bool MS>
__global__ void __launch_bounds__(512) k_conv_quad(const zp_conv_args A, const quad_geo QG, const int flags) {
  // MS (flags & 256, as k_conv_strip2's DM 2): the next chunk's strip DMA is issued between the MFMAs
  // of step 0 instead of in its read section
  constexpr int WC = 2, WP = 4, NWP = 4;
  constexpr int TC = 64, TP = 256, TR = TP / W;
  constexpr int SROWS = (TR + 1) * W;    // strip rows: TR + 1 image rows of W pixels
  constexpr int SPW = (SROWS + 63) / 64;  // strip DMA instructions per wave (8 waves x 8 rows each)
  constexpr int SRP = 64 * SPW;
  constexpr int WSLOT = TC * 128;         // bytes per weight slot (one tap)
  constexpr int SBASE = 9 * WSLOT;        // strip ring after the 9 weight slots
  constexpr int SSLOT = SRP * 128;
  static_assert(SPW == 5, "strip of 5 DMA instructions per wave (W 32 / 64)");
  static_assert(7 * WSLOT + 2048 < 65536 && SSLOT + W * 128 < 65536, "ds_read immediate range");
  __shared__ uint4 lds[(9 * TC + 2 * SRP) * 8];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wid / NWP, wp = wid % NWP;
  const int GHW = A.GH * A.GW;
  const int M = A.N * GHW;
  int bx = blockIdx.x, by = blockIdx.y;
  if (flags & 2) {  // XCD-aware order: the cout tiles of one pixel tile (same strip) on one L2
    const int total = gridDim.x * gridDim.y;
    const int bid = blockIdx.x + gridDim.x * blockIdx.y;
    const int xcd = bid & 7, pos = bid >> 3, q = total >> 3, r = total & 7;
    const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
    bx = lin / gridDim.y;
    by = lin - bx * gridDim.y;
  }
  const int p0 = bx * TP, c0 = by * TC;
  const int n_img = p0 / GHW, y0 = (p0 - n_img * GHW) / W;
  const int CB = A.Cin / 64;
  const int lrow = lane >> 3;

#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)A.x, (short)0, (int)QG.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t wrsrc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    wrsrc[s] = __builtin_amdgcn_make_buffer_rsrc((void*)A.sub[s].w, (short)0, (int)QG.w_bytes, 0x00020000);
#endif
  // weight DMA: row c0 + wid * 8 + lrow of the slot, source chunk swizzled by the row (lrow)
  const unsigned wv = (unsigned)(((size_t)(c0 + wid * 8 + lrow) * A.k_pad + ((lane & 7) ^ lrow) * 8) * 2);
  // strip DMA: piece i = strip rows (wid + 8 i) * 8 + lrow = (tr, x); rows past the strip or below the
  // image read past the buffer end (zeros)
  unsigned sv[SPW];
#pragma unroll
  for (int i = 0; i < SPW; ++i) {
    const int srow = (wid + 8 * i) * 8 + lrow;
    const int tr = srow / W, x = srow - tr * W;
    const bool ok = srow < SROWS && y0 + tr < A.IH;
    const int sw = (lane & 7) ^ (srow & 7);
    sv[i] = ok ? (unsigned)((((n_img * A.IH + y0 + tr) * A.IW + x) * A.ldx + A.cx0 + sw * 8) * 2) : 0x80000000u;
  }
  const unsigned lds0 = lds_addr(lds);
  unsigned aoff[2], aoff8[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    aoff[s2] = lds0 + (unsigned)(wc * 16 * WC + (lane & 15)) * 128u + (unsigned)(((s2 * 4 + (lane >> 4)) ^ (lane & 7)) * 16);
    aoff8[s2] = aoff[s2] + 8u * WSLOT;
  }
  // B fragment j of the wave: grid point q = wp * 64 + 16 j + (lane & 15) -> strip row tr * W + x + dx
  // (+ dy * W through the immediate offset, which keeps the row's swizzle); the lane at x = W - 1
  // reads garbage for dx = 1 and is zeroed after the read
  unsigned bo[2][2][WP];
#pragma unroll
  for (int dx = 0; dx < 2; ++dx)
#pragma unroll
    for (int j = 0; j < WP; ++j) {
      const int q = wp * 64 + 16 * j + (lane & 15);
      const int sr = (q / W) * W + (q % W) + dx;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
        bo[dx][s2][j] = lds0 + (unsigned)SBASE + (unsigned)sr * 128u + (unsigned)((((s2 * 4 + (lane >> 4)) ^ (sr & 7))) * 16);
    }
  const bool edge = (lane & 15) == 15;  // x = W - 1 in fragments j = 3 (W 64) / j odd (W 32)
  // the strip slot of the current chunk alternates: bo moves between the two slots once per chunk
  // (a runtime parity keeps ONE loop body and one tail, so the 128 accumulators stay in place)
  int sdelta = SSLOT;
  auto flip = [&]() {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < WP; ++j) bo[dx][s2][j] += (unsigned)sdelta;
    sdelta = -sdelta;
  };

  auto issue_w = [&](int slot, int cb) {
#if defined(__HIP_DEVICE_COMPILE__)
    auto* d = (__attribute__((address_space(3))) void*)&lds[(slot * TC + wid * 8) * 8];
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc[quad_phase(slot)], d, 16, wv, QG.koff[slot] + cb * 128, 0, 0);
#endif
  };
  auto issue_s = [&](int gslot, int cb) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < SPW; ++i) {
      auto* d = (__attribute__((address_space(3))) void*)&lds[(9 * TC + gslot * SRP + (wid + 8 * i) * 8) * 8];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, d, 16, sv[i], cb * 128, 0, 0);
    }
#endif
  };

  f32x4 acc[4][WC][WP];
#pragma unroll
  for (int ph = 0; ph < 4; ++ph)
#pragma unroll
    for (int i = 0; i < WC; ++i)
#pragma unroll
      for (int j = 0; j < WP; ++j) acc[ph][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // one K step S of chunk cb (strip slot gp); STEADY: a next chunk exists (prefetches issued)
  auto step = [&](auto s_c, auto steady_c, int cb, int gp) {
    constexpr int S = decltype(s_c)::value;
    constexpr bool STEADY = decltype(steady_c)::value;
    constexpr int NT = S == 4 ? 1 : 2;
    constexpr int DY = (S == 3 || S == 4) ? 1 : 0, DX = (S == 2 || S == 4) ? 1 : 0;
    if constexpr (ZP_ABL == 1) {  // diagnostic build: no DMA in the loop
    } else if constexpr (S == 0) {
      issue_w(8, cb);
      if constexpr (STEADY && !MS) issue_s(gp ^ 1, cb + 1);
    } else if constexpr (STEADY) {
      issue_w(2 * (S - 1), cb + 1);
      issue_w(2 * (S - 1) + 1, cb + 1);
    }
    uint4 af[NT][2][WC], bfr[2][WP];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      static_for<NT>([&](auto t) {
        constexpr int SL = 2 * S + decltype(t)::value;
        static_for<WC>([&](auto i) {
          if constexpr (SL < 8) af[t][s2][i] = ds_read16<SL * WSLOT + i * 2048>(aoff[s2]);
          else af[t][s2][i] = ds_read16<i * 2048>(aoff8[s2]);
        });
      });
      static_for<WP>([&](auto j) { bfr[s2][j] = ds_read16<DY * W * 128>(bo[DX][s2][j]); });
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (DX == 1) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < WP; ++j)
          if (W == 32 ? (j & 1) : (j == 3)) {
            bfr[s2][j].x = edge ? 0u : bfr[s2][j].x;
            bfr[s2][j].y = edge ? 0u : bfr[s2][j].y;
            bfr[s2][j].z = edge ? 0u : bfr[s2][j].z;
            bfr[s2][j].w = edge ? 0u : bfr[s2][j].w;
          }
    }
    // loads allowed in flight at the end of this step (issued after what the next step reads)
    auto wait_out = [&]() {
      if constexpr (STEADY) {
        if constexpr (S == 0 && MS) vm_wait<5>();  // the strip is issued after this wait
        else if constexpr (S <= 2) vm_wait<5 + SPW>();
        else if constexpr (S == 3) vm_wait<6 + SPW>();
        else vm_wait<6>();
      } else {
        if constexpr (S == 0) vm_wait<5>();
        else if constexpr (S == 1) vm_wait<3>();
        else if constexpr (S == 2) vm_wait<1>();
        else vm_wait<0>();
      }
    };
    // ping-pong: the two wave groups run one barrier apart (the second group's extra prologue
    // barrier), so one group's MFMAs overlap the other's LDS reads
    wait_out();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    static_for<NT>([&](auto t) {
      constexpr int PH = quad_phase(2 * S + decltype(t)::value);
      static_for<2 * WC * WP>([&](auto u_c) {
        constexpr int u = decltype(u_c)::value, s2 = u / (WC * WP), i = (u / WP) % WC, j = u % WP;
        if constexpr (ZP_ABL != 2) MfmaTraits<T>::mma(acc[PH][i][j], af[t][s2][i], bfr[s2][j]);
        else acc[PH][i][j][0] += __uint_as_float(af[t][s2][i].x ^ bfr[s2][j].y);  // diagnostic: no MFMA
        // MS: strip piece k after MFMA 5 (k + 1) - 1 of step 0 (32 MFMAs), pinned between MFMAs
        constexpr int m = decltype(t)::value * 2 * WC * WP + u;
        if constexpr (MS && S == 0 && STEADY && ZP_ABL != 1 && (m + 1) % 5 == 0 && (m + 1) / 5 <= SPW) {
          constexpr int k = (m + 1) / 5 - 1;
          __builtin_amdgcn_sched_barrier(0);
#if defined(__HIP_DEVICE_COMPILE__)
          auto* d = (__attribute__((address_space(3))) void*)&lds[(9 * TC + (gp ^ 1) * SRP + (wid + 8 * k) * 8) * 8];
          __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, d, 16, sv[k], (cb + 1) * 128, 0, 0);
#endif
          __builtin_amdgcn_sched_barrier(0);
        }
      });
    });
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  using ST = std::integral_constant<bool, true>;
  using TL = std::integral_constant<bool, false>;
  auto chunk = [&](auto steady_c, int cb) {
    const int gp = cb & 1;
    step(std::integral_constant<int, 0>{}, steady_c, cb, gp);
    step(std::integral_constant<int, 1>{}, steady_c, cb, gp);
    step(std::integral_constant<int, 2>{}, steady_c, cb, gp);
    step(std::integral_constant<int, 3>{}, steady_c, cb, gp);
    step(std::integral_constant<int, 4>{}, steady_c, cb, gp);
    flip();
  };
  // prologue: strip of chunk 0, then the weights of slots 0..7 (slot 8 is issued by step 0)
  issue_s(0, 0);
#pragma unroll
  for (int sl = 0; sl < 8; ++sl) issue_w(sl, 0);
  vm_wait<6>();  // strip(0) and slots 0, 1 landed
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if (wid >= 4) __builtin_amdgcn_s_barrier();
  for (int cb = 0; cb < CB - 1; ++cb) chunk(ST{}, cb);
  chunk(TL{}, CB - 1);
  if (wid < 4) __builtin_amdgcn_s_barrier();
  if constexpr (ZP_ABL == 5) {  // diagnostic build: no epilogue (one store only if a sum is exactly 1)
    float sm = 0.f;
    static_for<4>([&](auto ph) {
#pragma unroll
      for (int i = 0; i < WC; ++i)
#pragma unroll
        for (int j = 0; j < WP; ++j) sm += acc[ph][i][j][0] + acc[ph][i][j][1] + acc[ph][i][j][2] + acc[ph][i][j][3];
    });
    if (sm == 1.f) ((float*)A.sub[0].y)[tid] = sm;
  } else {
    static_for<4>([&](auto ph) {
      conv_epilogue<T, WC, WP, NWP>(A, A.sub[ph], acc[ph], p0, c0, wc, wp, lane, M, GHW, bx, ph, 4, nullptr,
                                    (float*)lds);
    });
  }
}

// ------------------------------------------------------------------------------------
// 1 x 1 conv with a narrow K and a wide output (the head's data gradient in training: 32 -> 320
// channels at 128 x 128, bs 32 -- 34 MB in, 335 MB out).  On k_conv's small-Cin tile it took 177 us
// (2.1 TB/s): one K step per 128 x 256 tile, so every workgroup was prologue + epilogue at one
// workgroup per CU.  Here a block stages the whole packed weight (Cout x Cin, <= 48 KB) in LDS in
// MFMA fragment order once, and each wave walks 16-pixel groups: one 16-byte activation load per lane
// and K step, Cout / 16 MFMAs from LDS fragments, the paired 8-channel epilogue's 16-byte stores.
// Same MFMAs over the same K order as k_conv (its extra K step of zero weights only adds zeros).
constexpr int C1N_MAXCB = 24;  // cout blocks of 16 (384 channels)
template <typename T, int NCB>  // NCB = Cout / 16 (compile-time: the accumulators stay in registers)
__global__ void __launch_bounds__(256) k_conv1x1n(const zp_conv_args A) {
  __shared__ uint4 wl[NCB * 2 * 64];
  const zp_conv_sub& S = A.sub[0];
  constexpr int ncb = NCB;
  const int nks = A.Cin / 32;
  for (int f = threadIdx.x; f < ncb * nks * 64; f += blockDim.x) {  // fragment (i, s), lane l
    const int l = f & 63, fs = f >> 6, i = fs / nks, ks = fs - i * nks;
    wl[f] = *(const uint4*)((const unsigned short*)S.w + (size_t)(i * 16 + (l & 15)) * A.k_pad + ks * 32 + (l >> 4) * 8);
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4;
  const long M = (long)A.N * A.GH * A.GW;
  const long ngroups = (M + 15) / 16;
  for (long grp = (long)blockIdx.x * 4 + wave; grp < ngroups; grp += (long)gridDim.x * 4) {
    const long p = grp * 16 + (lane & 15);
    const bool pok = p < M;
    uint4 b[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      b[ks] = (pok && ks < nks) ? *(const uint4*)((const unsigned short*)A.x + p * A.ldx + A.cx0 + ks * 32 + g * 8)
                                : make_uint4(0u, 0u, 0u, 0u);
    f32x4 acc[NCB];
#pragma unroll
    for (int i = 0; i < NCB; ++i) {
      acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      MfmaTraits<T>::mma(acc[i], wl[(i * nks) * 64 + lane], b[0]);
      if (nks > 1) MfmaTraits<T>::mma(acc[i], wl[(i * nks + 1) * 64 + lane], b[1]);
    }
    // (stride 1, one sub-problem on the input grid: output pixel = p)
    unsigned short* Y = (unsigned short*)S.y + p * S.ldy + S.cy0;
#pragma unroll
    for (int i = 0; i < NCB; i += 2) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // all lanes active (cross-lane op)
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][r]), __float_as_uint(acc[i + 1][r]), false,
                                                         false);
        v[r] = __uint_as_float(sw[0]);
        v[r + 4] = __uint_as_float(sw[1]);
      }
      if (!pok) continue;
      const int cs = (i + (g & 1)) * 16 + (g >> 1) * 8;
      uint32_t o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = H16<T>::to(v[2 * r]) | (H16<T>::to(v[2 * r + 1]) << 16);
      *(uint4*)(Y + cs) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

}  // namespace zp

using namespace zp;

// ------------------------------------------------------------------------------------ host
// Tuning overrides for sweeps (read once): ZP_CONV_TP=128|256 forces the pixel tile,
// ZP_CONV_STAGES=2|3 forces the LDS ring depth, ZP_CONV_TC256=0 disables the 256-channel tile.
// 0 = heuristic.
static bool conv_tc256_enabled() {
  static const bool v = getenv("ZP_CONV_TC256") ? env_int("ZP_CONV_TC256") != 0 : true;
  return v;
}
static int conv_tp_override() {
  static const int v = env_int("ZP_CONV_TP");
  return v;
}
static int conv_stages_override() {
  static const int v = env_int("ZP_CONV_STAGES");
  return v;
}
// runtime tuning knobs (zp_conv_tuning)
static int g_tc256_min_blocks = 1024;  // key 0: minimum workgroup count for the 256-channel tile
static int g_conv_flags = -1;          // key 1 (runtime A/B in one process); -1 = env / default
static int g_strip_c64 = 1;  // key 2: 64-channel layers on the strip kernel (TC 64; 27.5 -> 22.2 us at 64x64)
static int g_quad_min_blocks = 256;    // key 6: fewest workgroups k_conv_quad runs with

// conv schedule switches: bit 1 XCD-aware tile order, bit 2 s_setprio(1) around the MFMA
// cluster, bit 3 ping-pong (staggered wave groups), bit 4 tap-row trimming (tap rows that read only
// padding for a whole tile are skipped; k_conv and the split-fp32 k_conv3), bit 5 spread strip DMA (k_conv_strip only; slower), bit 6
// k_conv_strip2 instead of k_conv_strip, bit 7 k_conv_quad for the four phases of stride-2 transposed
// structures (ConvTranspose2d forward, stride-2 conv data gradient), bit 8 k_conv_strip2 issues the
// next strip's DMA between the MFMAs of a group's first step (DM 2).  Default (measured, profiles/r01_conv_sweep.md,
// profiles/r02_conv_ab.md): XCD order + setprio + ping-pong + trimming + k_conv_strip2 (94).
// ZP_CONV_FLAGS / zp_conv_tuning(1, .) override for sweeps.
static int conv_flags() {
  static const int v = getenv("ZP_CONV_FLAGS") ? env_int("ZP_CONV_FLAGS") : 94 + 128 + 256;
  return g_conv_flags >= 0 ? g_conv_flags : v;
}

// k_conv1x1n's geometry (ZP_CONV1X1N=0 turns it off)
static bool conv1x1n_ok(const zp_conv_args& a) {
  static const int en1n = getenv("ZP_CONV1X1N") ? env_int("ZP_CONV1X1N") : 1;
  const zp_conv_sub& S = a.sub[0];
  return en1n && (a.dtype == ZP_BF16 || a.dtype == ZP_F16) && a.nsub == 1 && S.ntaps == 1 && S.ty[0] == 0 &&
         S.tx[0] == 0 && (a.Cin == 32 || a.Cin == 64) && a.Cout % 64 == 0 && a.Cout / 16 <= C1N_MAXCB &&
         a.w_rows >= a.Cout && a.k_pad >= a.Cin && !a.stats && !a.bnr_part && !a.res && !a.relu &&
         a.out_mode == ZP_OUT_NHWC && !S.scale && !S.shift && S.ldy % 8 == 0 && S.cy0 % 8 == 0 && a.ldx % 8 == 0 &&
         a.cx0 % 8 == 0 && a.sy == 1 && a.sx == 1 && a.GH == a.IH && a.GW == a.IW && S.OH == a.GH && S.OW == a.GW &&
         S.oys == 1 && S.oxs == 1 && S.oyo == 0 && S.oxo == 0 && (long)a.N * a.GH * a.GW >= 65536;
}

// 3x3 stride-1 same-size 16-bit convs on full-width tiles (W 32 / 64 / 128) whose strip of
// TR x (W + 2 pad) pixels fits the 320-row LDS slot run k_conv_strip (256-pixel tiles).
// ZP_CONV_STRIP=0 disables.
static bool strip_eligible(const zp_conv_args& a, strip_geo* sg) {
  static const int en = getenv("ZP_CONV_STRIP") ? env_int("ZP_CONV_STRIP") : 1;
  if (!en || a.dtype == ZP_F32 || a.nsub != 1 || a.Cin % 64 != 0 || a.Cout % 64 != 0) return false;
  if (a.Cout <= 64 && !g_strip_c64) return false;
  if (a.sy != 1 || a.sx != 1 || a.GH != a.IH || a.GW != a.IW) return false;
  const zp_conv_sub& S = a.sub[0];
  if (S.ntaps != 9 || S.oys != 1 || S.oxs != 1 || S.oyo != 0 || S.oxo != 0 || S.OH != a.GH || S.OW != a.GW)
    return false;
  const int ty0 = S.ty[0], tx0 = S.tx[0], dty = S.ty[3] - S.ty[0], dtx = S.tx[1] - S.tx[0];
  for (int t = 0; t < 9; ++t)
    if (S.ty[t] != ty0 + (t / 3) * dty || S.tx[t] != tx0 + (t % 3) * dtx) return false;
  const int W = a.GW;
  if (W != 32 && W != 64 && W != 128) return false;
  if (((long)a.GH * a.GW) % 256 != 0) return false;
  int pad = 0;
  for (int k = 0; k < 3; ++k) {
    pad = max(pad, abs(ty0 + k * dty));
    pad = max(pad, abs(tx0 + k * dtx));
  }
  const int TR = 256 / W, SW = W + 2 * pad, SR = TR * SW;
  if (SR > 320) return false;
  sg->W = W;
  sg->TR = TR;
  sg->SW = SW;
  sg->SR = SR;
  sg->SPW = 5;
  sg->ty0 = ty0;
  sg->dty = dty;
  sg->tx0 = tx0;
  sg->dtx = dtx;
  sg->pad = pad;
  return true;
}
// strip tile width: 128 channels, or 64 when 128-channel tiles would leave part of the 256 CUs
// idle (128 -> 128 at 32x32, bs 32: 128 workgroups; 24.2 -> 22.7 us).  A 256-channel strip tile does
// not fit the register file (35 spilled VGPRs).
static int strip_tc(const zp_conv_args& a) {
  static const int en64 = getenv("ZP_STRIP_TC64") ? env_int("ZP_STRIP_TC64") : 1;
  if (a.Cout <= 64) return 64;
  if (!en64) return 128;
  const long tiles = (long)a.N * a.GH * a.GW / 256;
  if (tiles * ((a.Cout + 127) / 128) < 256) return 64;
  return 128;
}

// k_conv_quad eligibility: 16-bit, the four phases (py, px) = (0,0), (0,1), (1,0), (1,1) of a
// stride-2 transposed structure over an input the size of the grid (W 32 / 64), 1 / 2 / 2 / 4 taps
// at input offsets in {0,1}^2 (geometry.py _phases with k = 3, p = 1), channels in whole chunks, and
// enough workgroups to cover the CUs.  qg: the byte offset of each schedule slot's tap.
static bool quad_plan(const zp_conv_args& a, quad_geo* qg) {
  if (!(conv_flags() & 128)) return false;
  if (a.dtype == ZP_F32 || a.nsub != 4 || a.Cin % 64 != 0 || a.Cout % 64 != 0) return false;
  if (a.sy != 1 || a.sx != 1 || a.GH != a.IH || a.GW != a.IW) return false;
  if (a.GW != 32 && a.GW != 64) return false;
  if (((long)a.GH * a.GW) % 256 != 0) return false;
  if ((long)a.N * a.GH * a.GW / 256 * (a.Cout / 64) < g_quad_min_blocks) return false;
  static const int ntap[4] = {1, 2, 2, 4};
  for (int s = 0; s < 4; ++s) {
    const zp_conv_sub& S = a.sub[s];
    if (S.oys != 2 || S.oxs != 2 || S.oyo != s / 2 || S.oxo != s % 2 || S.ntaps != ntap[s]) return false;
    if (S.OH < 2 * a.GH || S.OW < 2 * a.GW) return false;
  }
  // slot -> (ty, tx) (the sub is quad_phase(slot))
  static const int shift[9][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 1}, {0, 1}, {1, 0}, {1, 0}, {1, 1}};
  int used[4] = {0, 0, 0, 0};
  for (int k = 0; k < 9; ++k) {
    const int ph = quad_phase(k);
    const zp_conv_sub& S = a.sub[ph];
    int t = 0;
    while (t < S.ntaps && !(S.ty[t] == shift[k][0] && S.tx[t] == shift[k][1])) ++t;
    if (t == S.ntaps || (used[ph] >> t) & 1) return false;
    used[ph] |= 1 << t;
    qg->koff[k] = t * a.Cin * 2;
  }
  return true;
}

// One launch's configuration: what zp_conv2d runs and what every query answers.
enum conv_kind { CONV_SPLIT, CONV_C1X1N, CONV_STRIP, CONV_STRIP2, CONV_QUAD, CONV_TILE };
struct conv_plan {
  conv_kind kind;
  int variant;         // zp_conv2d_config's label of the kernel (include/zp.h)
  int tc, tp, stages;  // cout tile, pixel tile, LDS ring depth
  bool smallc;         // k_conv's small-Cin form (Cin below one K step)
  int gx, gy, gz;      // grid of every kind but CONV_C1X1N (gx is zp_conv2d_grid's answer for all)
  int blocks;          // CONV_C1X1N: its persistent workgroups
  int stat_parts, bnr_parts;
  int dm;              // CONV_STRIP2: k_conv_strip2's DM
  bool ms;             // CONV_QUAD: k_conv_quad's MS
  int ncb;             // CONV_C1X1N: k_conv1x1n's NCB
  strip_geo sg;        // CONV_STRIP, CONV_STRIP2 (x_bytes / w_bytes: the launch fills them)
  quad_geo qg;         // CONV_QUAD (the same)
};

// k_conv's tile (CONV_TILE; CONV_C1X1N reports it too).
// cout tile: 256 (the whole layer: activations are staged once per pixel tile instead of once per
// 128-channel tile, and 64 MFMAs per wave per LDS step instead of 32) for bf16 layers with
// Cout % 256 == 0; else 128 / 64 / 32.
// Measured (R34 bs 32, profiles/r01_conv_sweep.md): a win when the launch still has >= 1024
// workgroups of 256 pixels (64x64 / 128x128 layers, the 64x64 transposed-conv phases: 1.1-1.2x),
// a loss on 32x32 layers (128 workgroups for 256 CUs), on the 32x32 transposed-conv phases (512
// workgroups: 78.7 us vs 70.7 us on the 128-channel tile) and on the ASPP launch, whose four
// sub-problems (1 vs 9 taps) are too unbalanced for 512 large tiles.
// pixel tile: 256 (8 waves) whenever the cout tile allows it.  Measured on MI355X (R34 bs32,
// profiles/r01_conv_sweep.md): the 8-wave 3-stage tile beats the 4-wave tiles even on the
// 32x32 layers where it leaves part of the chip idle (fewer workgroups, but 2x the MFMA work
// per LDS byte and deeper prefetch)
static void plan_tile(const zp_conv_args& a, conv_plan& p) {
  const long M = (long)a.N * a.GH * a.GW;
  p.tc = a.Cout > 64 ? 128 : (a.Cout > 32 ? 64 : 32);
  if (a.dtype != ZP_F32 && a.Cout % 256 == 0 && a.Cin >= 64 && conv_tc256_enabled()) {
    int tmin = ZP_MAX_TAPS, tmax = 0;
    for (int s = 0; s < a.nsub; ++s) {
      tmin = a.sub[s].ntaps < tmin ? a.sub[s].ntaps : tmin;
      tmax = a.sub[s].ntaps > tmax ? a.sub[s].ntaps : tmax;
    }
    if (ceil_div(M, 256) * (long)a.nsub >= g_tc256_min_blocks && tmax <= 4 * tmin) p.tc = 256;
  }
  const int ov = conv_tp_override();
  // Cout <= 128 (one cout tile): 128-pixel tiles double the workgroup count of the 32x32 / 64x64
  // layers (tools/conv_micro.py: 128->128 @32x32 36 -> 24 us, 64->64 @64x64 28.6 -> 26.3 us);
  // the small-Cin stem keeps 256
  const int E = a.dtype == ZP_F32 ? 4 : 8;
  if (p.tc == 32) p.tp = 128;  // 32 + 256 rows do not split over 8 waves in 8-row groups
  else if (p.tc == 256) p.tp = 256;  // the 256-channel tile exists only with 256-pixel tiles
  else if (ov == 128 || ov == 256) p.tp = ov;
  else p.tp = a.Cout <= 128 && a.Cin >= 8 * E ? 128 : 256;
}

// The order of precedence: narrow-K 1x1, strip, quad, k_conv's tile (split dtypes: zp_conv3*.hip's own).
static conv_plan plan_conv(const zp_conv_args& a) {
  conv_plan p{};
  const long M = (long)a.N * a.GH * a.GW;
  const int fl = conv_flags();
  p.smallc = a.Cin < (a.dtype == ZP_F32 ? 32 : 64);
  if (a.dtype == ZP_F32X3 || a.dtype == ZP_F32H2) {
    p.kind = CONV_SPLIT;  // k_conv3 / k_conv3s / k_conv3w
    p.tc = conv3_tc(a);
    p.tp = conv3_tp(a, p.tc);
    p.variant = p.tc == 256 ? 6 : conv3_nsplit(a) == 1 && conv3_strip_ok(a, p.tc) ? 5 : 4;
  } else if (conv1x1n_ok(a)) {
    p.kind = CONV_C1X1N;
    p.variant = 7;
    plan_tile(a, p);
    p.ncb = a.Cout / 16;
    const long want = ((M + 15) / 16 + 3) / 4;  // four 16-pixel groups per workgroup and pass
    p.blocks = (int)(want < 2L * num_cus() ? want : 2L * num_cus());  // (~200 VGPRs: 2 blocks per CU)
  } else if (strip_eligible(a, &p.sg)) {
    // k_conv_strip2 (lean main loop) or k_conv_strip; flags & 32: strip DMA spread over the group
    p.kind = (fl & 64) ? CONV_STRIP2 : CONV_STRIP;
    p.variant = (fl & 64) ? 2 : 1;
    p.tc = strip_tc(a);
    p.tp = 256;
    p.dm = (fl & 256) ? 2 : (fl & 32) ? 1 : 0;
  } else if (quad_plan(a, &p.qg)) {
    p.kind = CONV_QUAD;  // 64 channels x 4 phases
    p.variant = 3;
    p.tc = 64;
    p.tp = 256;
    p.ms = (fl & 256) != 0;
  } else {
    p.kind = CONV_TILE;
    plan_tile(a, p);
  }
  // LDS ring depth: 3, except for the two launches with very few or gather-bound K steps, where the
  // 2-deep ring's smaller LDS footprint (more resident workgroups) wins (R34 bs 32, layer report):
  // the small-Cin stem (7x7, per-lane tap gather: 100 -> 75 us) and the 32-channel-tile head
  // (1x1 320 -> 17 at 128x128, 5 K steps, HBM-bound: 99 -> 90 us).  Every other k_conv launch loses
  // with 2 stages (ASPP 217 -> 329 us).  The 256 x 256 tile: 64 KB per LDS stage, so a 2-deep ring.
  const int ov = conv_stages_override();
  p.stages = p.tc == 256 ? 2 : (ov == 2 || ov == 3) ? ov : (p.smallc || p.tc <= 32) ? 2 : 3;
  p.gx = ceil_div(M, p.tp);  // (strip, quad: whole 256-pixel tiles)
  p.gy = ceil_div(a.Cout, p.tc);
  p.gz = p.kind == CONV_STRIP || p.kind == CONV_STRIP2 || p.kind == CONV_QUAD ? 1 : a.nsub;
  // statistics parts: k_conv_strip2, k_conv_quad and k_conv merge their wave halves in LDS -- one
  // part per tile and sub (k_conv_quad's tiles hold the four phases); k_conv_strip and the split
  // forms keep one per wave half.  bnr_parts == stat_parts by construction: every kernel that takes
  // the fused BN backward reduce (bnr_part) emits its parts exactly as it emits the statistics.
  p.stat_parts = p.kind == CONV_SPLIT   ? (p.tp / 64) * p.gx * a.nsub
                 : p.kind == CONV_STRIP ? 4 * p.gx
                 : p.kind == CONV_QUAD  ? 4 * p.gx
                                        : p.gx * p.gz;
  p.bnr_parts = p.stat_parts;
  return p;
}

extern "C" int zp_conv2d_grid(const zp_conv_args* a) { return a ? plan_conv(*a).gx : 0; }
extern "C" int zp_conv2d_stat_parts(const zp_conv_args* a) { return a ? plan_conv(*a).stat_parts : 0; }
extern "C" int zp_conv2d_bnr_parts(const zp_conv_args* a) { return a ? plan_conv(*a).bnr_parts : 0; }

/* launch configuration zp_conv2d picks for these args (for kernel labels in reports) */
extern "C" int zp_conv2d_config(const zp_conv_args* a, int* tc, int* tp, int* stages, int* variant) {
  ZP_CHECK_ARG(a && tc && tp && stages && variant, "zp_conv2d_config: null args");
  const conv_plan p = plan_conv(*a);
  *tc = p.tc;
  *tp = p.tp;
  *stages = p.stages;
  *variant = p.variant;
  return ZP_OK;
}

template <typename T, int WC, int NWP, int STAGES>
static void launch_conv_st(const zp_conv_args& a, const conv_taps& tg, const conv_plan& p, hipStream_t st) {
  const dim3 grid(p.gx, p.gy, p.gz);
  if (p.smallc)
    hipLaunchKernelGGL((k_conv<T, WC, 4, NWP, STAGES, true>), grid, dim3(128 * NWP), 0, st, a, tg, conv_flags());
  else
    hipLaunchKernelGGL((k_conv<T, WC, 4, NWP, STAGES, false>), grid, dim3(128 * NWP), 0, st, a, tg, conv_flags());
}
template <typename T, int WC, int NWP>
static void launch_conv_nwp(const zp_conv_args& a, const conv_taps& tg, const conv_plan& p, hipStream_t st) {
  if (p.stages == 3) launch_conv_st<T, WC, NWP, 3>(a, tg, p, st);
  else launch_conv_st<T, WC, NWP, 2>(a, tg, p, st);
}
template <typename T>
static void launch_conv(const zp_conv_args& a, const conv_taps& tg, const conv_plan& p, hipStream_t st) {
  const int nwp = p.tp / 64;
  if (p.tc == 256) {  // (16-bit only)
    if constexpr (sizeof(T) == 2) hipLaunchKernelGGL((k_conv<T, 8, 4, 4, 2, false>), dim3(p.gx, p.gy, p.gz), dim3(512), 0, st, a, tg, conv_flags());
  } else if (p.tc == 128) {
    if (nwp == 4) launch_conv_nwp<T, 4, 4>(a, tg, p, st);
    else launch_conv_nwp<T, 4, 2>(a, tg, p, st);
  } else if (p.tc == 64) {
    if (nwp == 4) launch_conv_nwp<T, 2, 4>(a, tg, p, st);
    else launch_conv_nwp<T, 2, 2>(a, tg, p, st);
  } else {
    launch_conv_nwp<T, 1, 2>(a, tg, p, st);
  }
}

extern "C" int zp_conv2d(const zp_conv_args* ap, void* stream) {
  ZP_CHECK_ARG(ap != nullptr, "zp_conv2d: null args");
  const zp_conv_args& a = *ap;
  ZP_CHECK_ARG(a.dtype == ZP_F32 || a.dtype == ZP_BF16 || a.dtype == ZP_F16 || a.dtype == ZP_F32X3 ||
                   a.dtype == ZP_F32H2,
               "zp_conv2d: bad dtype %d", a.dtype);
  ZP_CHECK_ARG(a.nsub >= 1 && a.nsub <= ZP_MAX_SUB, "zp_conv2d: nsub %d", a.nsub);
  ZP_CHECK_ARG(a.x && a.N > 0 && a.GH > 0 && a.GW > 0 && a.IH > 0 && a.IW > 0 && a.Cout > 0,
               "zp_conv2d: bad geometry");
  ZP_CHECK_ARG(!a.bnr_part || (a.bnr_x && a.bnr_save && (a.dtype == ZP_F32 || a.dtype == ZP_BF16) && !a.stats &&
                                !a.res && !a.relu && a.out_mode == ZP_OUT_NHWC && a.Cout % 4 == 0),
               "zp_conv2d: bnr_* (fused BN backward reduce) needs a plain f32 / bf16 NHWC store (no stats, "
               "residual, ReLU), bnr_x and bnr_save, Cout %% 4 == 0");
  hipStream_t st = (hipStream_t)stream;
  const int fl = conv_flags();
  if (a.dtype == ZP_F32X3 || a.dtype == ZP_F32H2) return conv3_launch(a, st, fl);  // (plans itself: zp_conv3.hip)
  conv_plan p = plan_conv(a);
  const int E = a.dtype == ZP_F32 ? 4 : 8, KE = 8 * E;
  ZP_CHECK_ARG(a.Cin > 0 && a.Cin % E == 0 && (p.smallc || a.Cin % KE == 0),
               "zp_conv2d: Cin %d must be a multiple of %d (or < %d and a multiple of %d)", a.Cin, KE, KE, E);
  ZP_CHECK_ARG(a.ldx >= a.cx0 + a.Cin && a.cx0 % E == 0 && a.ldx % E == 0, "zp_conv2d: bad ldx/cx0");
  ZP_CHECK_ARG(a.k_pad % KE == 0, "zp_conv2d: k_pad %d not a multiple of %d", a.k_pad, KE);
  ZP_CHECK_ARG(a.w_rows % p.tc == 0 && a.w_rows >= a.Cout, "zp_conv2d: w_rows %d", a.w_rows);
  ZP_CHECK_ARG((a.out_mode >= 0 && a.out_mode <= 2) || ((a.out_mode == ZP_OUT_NHWC_X3 || a.out_mode == ZP_OUT_NHWC_H2) && a.dtype == ZP_F32 && !a.stats),
               "zp_conv2d: out_mode %d", a.out_mode);
  ZP_CHECK_ARG(!(a.stats || a.bnr_part) || (!a.res && !a.relu && a.out_mode != ZP_OUT_HEAD_NCHW && !a.sub[0].scale &&
                            !a.sub[0].shift),
               "zp_conv2d: stats are taken on the raw conv output (no scale/shift/residual/relu/head)");
  for (int s = 0; s < a.nsub; ++s) {
    const zp_conv_sub& S = a.sub[s];
    ZP_CHECK_ARG(S.w && S.y, "zp_conv2d: sub %d null w/y", s);
    ZP_CHECK_ARG(!a.bnr_part || (!S.scale && !S.shift), "zp_conv2d: bnr_* with a scale / shift epilogue");
    ZP_CHECK_ARG(S.ntaps >= 1 && S.ntaps <= ZP_MAX_TAPS, "zp_conv2d: ntaps %d", S.ntaps);
    if (p.smallc) {
      ZP_CHECK_ARG(S.kw > 0 && (long)S.ntaps * a.Cin <= a.k_pad, "zp_conv2d: small-Cin taps/k_pad");
    } else {
      ZP_CHECK_ARG((long)S.ntaps * a.Cin <= a.k_pad, "zp_conv2d: k_pad %d < ntaps*Cin", a.k_pad);
    }
    if (a.out_mode != ZP_OUT_HEAD_NCHW) {
      ZP_CHECK_ARG(S.ldy >= S.cy0 + a.Cout && S.cy0 % 4 == 0 && S.ldy % 4 == 0, "zp_conv2d: bad ldy/cy0");
    } else {
      ZP_CHECK_ARG(S.y2 || a.Cout == 1, "zp_conv2d: head needs y2");
    }
  }
  if (a.res) ZP_CHECK_ARG(a.ldr >= a.cr0 + a.Cout && a.cr0 % 4 == 0, "zp_conv2d: bad residual ld");
  conv_taps tg{};
  {
    const long long xb = (long long)a.N * a.IH * a.IW * a.ldx * (E == 8 ? 2 : 4);
    const long long wb = (long long)a.w_rows * a.k_pad * (E == 8 ? 2 : 4);
    ZP_CHECK_ARG(xb < (1ll << 31) && wb < (1ll << 31),
                 "zp_conv2d: input (%lld B) / weights (%lld B) must stay below 2 GiB per launch (split the batch)",
                 xb, wb);
    tg.x_bytes = (unsigned)xb;
    tg.rflag = a.out_mode == ZP_OUT_NHWC_H2 ? range_flag() : nullptr;
    for (int s = 0; s < a.nsub; ++s) {
      const zp_conv_sub& S = a.sub[s];
      tg.w_bytes[s] = (unsigned)wb;
      int nx = 1;
      while (nx < S.ntaps && S.ty[nx] == S.ty[0]) ++nx;
      const int ny = S.ntaps / nx;
      tg.ny[s] = ny;
      tg.nx[s] = nx;
      tg.ty0[s] = S.ty[0];
      tg.tx0[s] = S.tx[0];
      tg.dty[s] = ny > 1 ? S.ty[nx] - S.ty[0] : 0;
      tg.dtx[s] = nx > 1 ? S.tx[1] - S.tx[0] : 0;
      if (p.smallc) continue;  // the small-Cin path decodes (kw, dil, pad) per lane instead
      bool grid = ny * nx == S.ntaps && ny <= 32 && nx <= 32;
      for (int t = 0; grid && t < S.ntaps; ++t)
        grid = S.ty[t] == tg.ty0[s] + (t / nx) * tg.dty[s] && S.tx[t] == tg.tx0[s] + (t % nx) * tg.dtx[s];
      ZP_CHECK_ARG(grid, "zp_conv2d: sub %d taps must form a (row x column) grid of at most 32 x 32, rows outer", s);
    }
  }
  p.sg.x_bytes = p.qg.x_bytes = tg.x_bytes;
  p.sg.w_bytes = p.qg.w_bytes = tg.w_bytes[0];
  const dim3 grid(p.gx, p.gy, p.gz);
  const bool f16 = a.dtype == ZP_F16;
  switch (p.kind) {
    case CONV_C1X1N: {  // narrow-K 1x1 convs with a wide output (the head's data gradient in training)
#define ZP_C1N(NCB)                                                                                 \
  case NCB:                                                                                         \
    if (f16) hipLaunchKernelGGL((k_conv1x1n<f16_t, NCB>), dim3(p.blocks), dim3(256), 0, st, a);     \
    else hipLaunchKernelGGL((k_conv1x1n<bf16_t, NCB>), dim3(p.blocks), dim3(256), 0, st, a);        \
    break;
      switch (p.ncb) { ZP_C1N(4) ZP_C1N(8) ZP_C1N(12) ZP_C1N(16) ZP_C1N(20) ZP_C1N(24) }
#undef ZP_C1N
      ZP_LAUNCH_CHECK("zp_conv2d 1x1 narrow-K");
      return ZP_OK;
    }
    case CONV_STRIP2: {
      const zp_head_args H0{};
#define ZP_STRIP2(T, WC, BNR)                                                                                       \
  if (p.dm == 2) hipLaunchKernelGGL((k_conv_strip2<T, WC, 5, 2, false, BNR>), grid, dim3(512), 0, st, a, p.sg, fl, H0);      \
  else if (p.dm == 1) hipLaunchKernelGGL((k_conv_strip2<T, WC, 5, 1, false, BNR>), grid, dim3(512), 0, st, a, p.sg, fl, H0); \
  else hipLaunchKernelGGL((k_conv_strip2<T, WC, 5, 0, false, BNR>), grid, dim3(512), 0, st, a, p.sg, fl, H0);
      if (a.bnr_part) {  // (bf16 only: zp_conv2d's bnr check)
        if (p.tc == 64) { ZP_STRIP2(bf16_t, 2, true) } else { ZP_STRIP2(bf16_t, 4, true) }
      } else if (f16) {
        if (p.tc == 64) { ZP_STRIP2(f16_t, 2, false) } else { ZP_STRIP2(f16_t, 4, false) }
      } else {
        if (p.tc == 64) { ZP_STRIP2(bf16_t, 2, false) } else { ZP_STRIP2(bf16_t, 4, false) }
      }
#undef ZP_STRIP2
      ZP_LAUNCH_CHECK("zp_conv2d strip");
      return ZP_OK;
    }
    case CONV_STRIP:
      if (f16) {
        if (p.tc == 64) hipLaunchKernelGGL((k_conv_strip<f16_t, 2, 3, 5>), grid, dim3(512), 0, st, a, p.sg, fl);
        else hipLaunchKernelGGL((k_conv_strip<f16_t, 4, 3, 5>), grid, dim3(512), 0, st, a, p.sg, fl);
      } else {
        if (p.tc == 64) hipLaunchKernelGGL((k_conv_strip<bf16_t, 2, 3, 5>), grid, dim3(512), 0, st, a, p.sg, fl);
        else hipLaunchKernelGGL((k_conv_strip<bf16_t, 4, 3, 5>), grid, dim3(512), 0, st, a, p.sg, fl);
      }
      ZP_LAUNCH_CHECK("zp_conv2d strip");
      return ZP_OK;
    case CONV_QUAD:
#define ZP_QUAD(T)                                                                                              \
  if (a.GW == 32 && p.ms) hipLaunchKernelGGL((k_conv_quad<T, 32, true>), grid, dim3(512), 0, st, a, p.qg, fl);  \
  else if (a.GW == 32) hipLaunchKernelGGL((k_conv_quad<T, 32, false>), grid, dim3(512), 0, st, a, p.qg, fl);    \
  else if (p.ms) hipLaunchKernelGGL((k_conv_quad<T, 64, true>), grid, dim3(512), 0, st, a, p.qg, fl);           \
  else hipLaunchKernelGGL((k_conv_quad<T, 64, false>), grid, dim3(512), 0, st, a, p.qg, fl);
      if (f16) { ZP_QUAD(f16_t) } else { ZP_QUAD(bf16_t) }
#undef ZP_QUAD
      ZP_LAUNCH_CHECK("zp_conv2d quad");
      return ZP_OK;
    default:  // CONV_TILE
      if (a.dtype == ZP_BF16) launch_conv<bf16_t>(a, tg, p, st);
      else if (f16) launch_conv<f16_t>(a, tg, p, st);
      else launch_conv<float>(a, tg, p, st);
      ZP_LAUNCH_CHECK("zp_conv2d");
      return ZP_OK;
  }
}

// the 16-bit fused head: a 3x3 stride-1 conv on the 128-channel strip tile (k_conv_strip2, two cout
// tiles for Cout 256); ZP_F32H2: the wide two-plane tile, unsplit
static bool head_ok(const zp_conv_args& a, const conv_plan& p) {
  if (a.nsub != 1 || a.Cout != 256 || a.out_mode != ZP_OUT_NHWC) return false;
  if (a.dtype == ZP_F32H2) return p.tc == 256 && conv3w_tp_head(a) == 256 && conv3w_splitk(a) == 1;
  if ((a.dtype != ZP_BF16 && a.dtype != ZP_F16) || a.stats) return false;
  if (a.res && (a.ldr % 8 != 0 || a.cr0 % 8 != 0)) return false;
  return p.kind == CONV_STRIP2 && p.tc == 128;
}

extern "C" int zp_conv2d_head_ok(const zp_conv_args* a) { return a && head_ok(*a, plan_conv(*a)); }

extern "C" long long zp_conv2d_head_ws(const zp_conv_args* a) {
  if (!a || !(a->dtype == ZP_BF16 || a->dtype == ZP_F16)) return 0;
  return 2LL * 32 * (long long)a->N * a->GH * a->GW * 4;
}

extern "C" int zp_conv2d_head(const zp_conv_args* a, const zp_head_args* h, void* stream) {
  ZP_CHECK_ARG(a && h, "zp_conv2d_head: null args");
  conv_plan p = plan_conv(*a);
  ZP_CHECK_ARG(head_ok(*a, p), "zp_conv2d_head: not a fused-head geometry (zp_conv2d_head_ok)");
  if (a->dtype == ZP_F32H2) return conv3_launch(*a, (hipStream_t)stream, conv_flags(), h);
  // ZP_BF16 / ZP_F16: the strip kernel with the head epilogue, then the cout tiles' combine
  const zp_conv_args& A = *a;
  ZP_CHECK_ARG(h->w && h->mask && (h->code || h->cout == 1) && h->cout >= 1 && h->cout <= 32 && h->ws,
               "zp_conv2d_head: bad head (16-bit: needs ws, zp_conv2d_head_ws bytes)");
  ZP_CHECK_ARG(h->C2 >= 0 && h->C2 % 32 == 0 && h->k_pad % 8 == 0 && h->k_pad >= A.Cout + h->C2,
               "zp_conv2d_head: C2 %d / k_pad %d", h->C2, h->k_pad);
  ZP_CHECK_ARG(h->C2 == 0 || (h->x2 && h->ldx2 % 8 == 0 && h->cx20 % 8 == 0 && h->ldx2 >= h->cx20 + h->C2),
               "zp_conv2d_head: x2 layout");
  ZP_CHECK_ARG(A.Cin > 0 && A.Cin % 64 == 0 && A.ldx >= A.cx0 + A.Cin && A.cx0 % 8 == 0 && A.ldx % 8 == 0 &&
                   A.k_pad % 64 == 0 && A.w_rows % 128 == 0 && A.w_rows >= A.Cout && A.sub[0].w && A.sub[0].ntaps == 9,
               "zp_conv2d_head: conv operands");
  ZP_CHECK_ARG(A.sub[0].OH == A.GH && A.sub[0].OW == A.GW, "zp_conv2d_head: output grid");
  const long long xb = (long long)A.N * A.IH * A.IW * A.ldx * 2, wb = (long long)A.w_rows * A.k_pad * 2;
  ZP_CHECK_ARG(xb < (1ll << 31) && wb < (1ll << 31), "zp_conv2d_head: input / weights must stay below 2 GiB");
  ZP_CHECK_ARG(p.kind == CONV_STRIP2, "zp_conv2d_head: not a strip geometry");
  p.sg.x_bytes = (unsigned)xb;
  p.sg.w_bytes = (unsigned)wb;
  hipStream_t st = (hipStream_t)stream;
  const int fl = conv_flags();
  const dim3 grid(p.gx, p.gy, 1u);  // (two 128-channel cout tiles; always DM 2, whatever the flags say)
  if (A.dtype == ZP_F16) hipLaunchKernelGGL((k_conv_strip2<f16_t, 4, 5, 2, true>), grid, dim3(512), 0, st, A, p.sg, fl, *h);
  else hipLaunchKernelGGL((k_conv_strip2<bf16_t, 4, 5, 2, true>), grid, dim3(512), 0, st, A, p.sg, fl, *h);
  ZP_LAUNCH_CHECK("zp_conv2d_head (16-bit conv + head partials)");
  const int M = A.N * A.GH * A.GW;
  hipLaunchKernelGGL(k_head_combine16, dim3((M + 255) / 256), dim3(256), 0, st, h->ws, M, A.GH * A.GW, h->cout, h->bias,
                     h->mask, h->code);
  ZP_LAUNCH_CHECK("zp_conv2d_head (combine)");
  return ZP_OK;
}

/* split-fp32 split-K workspace: bytes of f32 slices zp_conv2d uses for these args when a.stats
 * points to that many (0: the launch is not split) */
extern "C" long long zp_conv2d_split_ws(const zp_conv_args* a) {
  if (!a || (a->dtype != ZP_F32X3 && a->dtype != ZP_F32H2)) return 0;
  const int ns = conv3_nsplit(*a);
  return ns > 1 ? (long long)ns * a->nsub * a->N * a->GH * a->GW * a->Cout * 4 : 0;
}

/* runtime tuning knobs: include/zp.h lists the keys.  Returns the previous value. */
extern "C" int zp_conv_tuning(int key, int value) {
  int* g = nullptr;
  switch (key) {
    case 0: g = &g_tc256_min_blocks; break;
    case 1: g = &g_conv_flags; break;
    case 2: g = &g_strip_c64; break;
    case 6: g = &g_quad_min_blocks; break;
    case 3:
    case 4:
    case 5: return wgrad_tuning(key, value);
    case 7: return conv3_strip_mode(value);
    case 8: return conv3_min_blocks(value);
    case 9: return conv3_splitk_mode(value);
    case 10: return conv3w_mode(value);
    case 11: return conv3w_min_blocks(value);
    case 12: return conv3w_splitk_mode(value);
    case 13: return conv3w_acc_mode(value);
    case 14: return conv3w_tp128_mode(value);
    case 15: return bn_fused_mode(value);
    case 16: return conv3_subint_mode(value);
    case 17: return conv3w_subint_mode(value);
    case 18: return conv3w_mf32_mode(value);
    case 19: return conv3_pipe_st_mode(value);
    case 20: return stem_wgs_mode(value);
    case 21: return conv3w_pfb_mode(value);
    case 22: return conv3w_pp_mode(value);
    default: return -1;
  }
  const int old = *g;
  *g = value;
  return old;
}
