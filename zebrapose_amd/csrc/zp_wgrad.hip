// Weight gradient of the implicit-GEMM convolutions of zp_conv.hip for gfx950 (MI355X): k_wgrad
// (register-staged; f32 parity mode), k_wgrad_lds and k_wgrad2 (bf16, LDS-DMA), k_wgrad_reduce (the
// deterministic split-K sum) and their launch plan.  NHWC activations; dw in the weight's own layout.
//
// Replaces autograd's weight gradients of the nn.Conv2d / nn.ConvTranspose2d modules zp_conv.hip
// lists (train_v6.py:337; see include/zp.h).
#include <algorithm>
#include <type_traits>
#include "zp_common.h"
#include "zp_conv_kern.h"
#include "zp_conv3.h"

namespace zp {

// ------------------------------------------------------------------------------------
// weight gradient:  ws[split][sub][co][col] = sum over the split's grid points of
//   dy[out pixel][co] * x[in pixel (tap of col)][ci of col],   col = t*Cin + ci
// K (pixels) is the MFMA reduction axis, so both LDS tiles [pixel][channel] are read
// transposed with ds_read_b64_tr_b16 (bf16) / per-lane b32 (f32).
// ------------------------------------------------------------------------------------
template <typename T> struct WgTraits;
template <> struct WgTraits<bf16_t> { static constexpr int KP = 32; };  // pixels per K step
template <> struct WgTraits<float> { static constexpr int KP = 16; };

constexpr int WG_TILE = 128;            // co x col tile
constexpr int WG_ROWB = 256 + 16;       // LDS row bytes (128 ch of bf16 / 64 of f32 -> see below)

template <typename T>
__global__ void __launch_bounds__(256) k_wgrad(const zp_wgrad_args A, float* __restrict__ ws, int pix_per_split,
                                                int col_tiles, int cols_max) {
  constexpr int KP = WgTraits<T>::KP;
  constexpr int CHE = 16 / sizeof(T);            // elements per 16 B chunk
  constexpr int NCH = WG_TILE / CHE;             // chunks per 128-channel row (16 bf16 / 32 f32)
  constexpr int ROWB = WG_TILE * sizeof(T) + 16; // padded LDS row bytes
  constexpr int TILEB = KP * ROWB;
  constexpr int LPT = KP * NCH / 256;            // chunk loads per thread per tile (2)
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][TILEB];

  const int sub = blockIdx.z;
  const auto& S = A.sub[sub];
  const int cols = S.ntaps * A.Cin;
  const int ct = blockIdx.y % col_tiles, cot = blockIdx.y / col_tiles;
  const int col0 = ct * WG_TILE, co0 = cot * WG_TILE;
  if (col0 >= cols) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wc = wid >> 1, wk = wid & 1;
  const int GHW = A.GH * A.GW;
  const int M = A.N * GHW;
  const int pbeg = blockIdx.x * pix_per_split;
  const int pend = min(M, pbeg + pix_per_split);

  // thread -> (row, chunk) of both tiles; chunk column fixed for the whole kernel
  const int qc = tid % NCH, qr = tid / NCH;      // rows qr + (256/NCH)*i
  constexpr int RSTEP = 256 / NCH;
  // dy channel of this chunk
  const int dco = co0 + qc * CHE;
  const bool dco_ok = dco < A.Cout;
  // x column of this chunk -> (tap, ci)
  const int xcol = col0 + qc * CHE;
  const bool xcol_ok = xcol < cols;
  const int xt = xcol_ok ? xcol / A.Cin : 0;
  const int xci = xcol - xt * A.Cin;
  const int xty = S.ty[xt], xtx = S.tx[xt];
  const T* __restrict__ X = (const T*)A.x;
  const T* __restrict__ DY = (const T*)S.dy;

  uint4 rd[LPT], rx[LPT];
  auto gload = [&](int pk) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      int p = pk + qr + RSTEP * i;
      uint4 vd = make_uint4(0, 0, 0, 0), vx = make_uint4(0, 0, 0, 0);
      if (p < pend) {
        int n = p / GHW, rr = p - n * GHW;
        int gy = rr / A.GW, gx = rr - gy * A.GW;
        if (dco_ok) {
          int oy = gy * S.oys + S.oyo, ox = gx * S.oxs + S.oxo;
          vd = *(const uint4*)(DY + (((size_t)n * S.OH + oy) * S.OW + ox) * S.lddy + S.cdy0 + dco);
        }
        int iy = gy * A.sy + xty, ix = gx * A.sx + xtx;
        if (xcol_ok && (unsigned)iy < (unsigned)A.IH && (unsigned)ix < (unsigned)A.IW)
          vx = *(const uint4*)(X + (((size_t)n * A.IH + iy) * A.IW + ix) * A.ldx + A.cx0 + xci);
      }
      rd[i] = vd;
      rx[i] = vx;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      int row = qr + RSTEP * i;
      *(uint4*)(&lds[buf][0][row * ROWB + qc * 16]) = rd[i];
      *(uint4*)(&lds[buf][1][row * ROWB + qc * 16]) = rx[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nsteps = pend > pbeg ? (pend - pbeg + KP - 1) / KP : 0;
  if (nsteps > 0) {
    gload(pbeg);
    sstore(0);
  }
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) gload(pbeg + (s + 1) * KP);
    const unsigned char* TD = lds[buf][0];
    const unsigned char* TX = lds[buf][1];
    if constexpr (sizeof(T) == 2) {
      // A[co][k] and B[k][col]: lane l of group g = l>>4 needs k = 8g..8g+7 of column (l & 15)
      typedef __attribute__((ext_vector_type(4))) short s4;
      const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
      bf16x8 af[4], bfm[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int cbase = wc * 64 + i * 16 + 4 * pp;
        const unsigned char* a0 = TD + (8 * g + q) * ROWB + cbase * 2;
        s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(a0));
        s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(a0 + 4 * ROWB));
        typedef __attribute__((ext_vector_type(8))) short s8;
        s8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        af[i] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int cbase = wk * 64 + j * 16 + 4 * pp;
        const unsigned char* b0 = TX + (8 * g + q) * ROWB + cbase * 2;
        s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(b0));
        s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(b0 + 4 * ROWB));
        typedef __attribute__((ext_vector_type(8))) short s8;
        s8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        bfm[j] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfm[j], acc[i][j], 0, 0, 0);
    } else {
      // f32: A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; 4 MFMAs of K=4 per 16-pixel step
      const int li = lane & 15, g = lane >> 4;
#pragma unroll
      for (int kk = 0; kk < KP; kk += 4) {
        float av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          av[i] = *(const float*)(TD + (kk + g) * ROWB + (wc * 64 + i * 16 + li) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bv[j] = *(const float*)(TX + (kk + g) * ROWB + (wk * 64 + j * 16 + li) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
      }
    }
    if (s + 1 < nsteps) sstore(buf ^ 1);
    __syncthreads();
  }
  // write partial tile: ws[((split*nsub + sub)*Cout + co)*cols_max + col]
  float* W = ws + ((size_t)blockIdx.x * A.nsub + sub) * (size_t)A.Cout * cols_max;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int col = col0 + wk * 64 + j * 16 + (lane & 15);
      if (col >= cols) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int co = co0 + wc * 64 + i * 16 + (lane >> 4) * 4 + r;
        if (co < A.Cout) W[(size_t)co * cols_max + col] = acc[i][j][r];
      }
    }
}

// ------------------------------------------------------------------------------------
// bf16 weight gradient, LDS-DMA version.  Same product and workspace layout as k_wgrad.
//
// A workgroup of 8 waves owns a (64*NA output channels) x (64*NB columns) tile; wave
// (a, b) = (w / NB, w % NB) computes a 64 x 64 block with 4 x 4 v_mfma_f32_16x16x32_bf16.
// Every K step covers KP consecutive grid points (pixels).  The stage image is NA + NB
// "panels" of [KP pixel rows][64 channels] (128 B rows): panels 0..NA-1 hold dy channels,
// panels NA.. hold x columns (tap, channel).  They are filled straight from global memory by
// buffer_load ... lds (one wave-instruction = 8 rows), STAGES-deep ring, counted vmcnt + raw
// barrier per step, exactly as k_conv does.
//
// The MFMA reduces over pixels, so both operands are read transposed with
// ds_read_b64_tr_b16: lane 4q+p of 16-lane group g supplies row (8g + q) and columns
// 4p..4p+3 of a 16-column block and receives one column (4 consecutive pixels).  Chunk
// swizzle: the 16 B chunk c of row R sits at chunk c ^ s(R), s(R) = 2 * (bit1(R) | bit3(R) << 1)
// (even, so the chunk pair of a 16-column block stays adjacent): the 8 rows a 32-lane half
// reads (two groups, rows 8g+q, q < 4) then cover all 64 banks once -- conflict-free.  The
// LDS-DMA writes are lane-linear, so the swizzle is applied on the per-lane SOURCE chunk.
//
// The tap walk is per lane: each lane always loads the same pixel row R of the tile (the
// instruction -> row-block map is wave-constant), so the grid point (n, gy, gx) advances
// incrementally by KP per issued step -- no divisions in the loop.
// ------------------------------------------------------------------------------------
struct wg_bounds {
  unsigned x_bytes, dy_bytes[ZP_MAX_SUB];
};

__device__ __forceinline__ int wg_swz(int r) { return (((r >> 1) & 1) | (((r >> 3) & 1) << 1)) << 1; }

template <int OFF>
__device__ __forceinline__ uint2 ds_read_tr8(unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset range");
  uint2 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}

template <int KP, int NA, int NB, int STAGES, int WN>
__global__ void __launch_bounds__(512) k_wgrad_lds(const zp_wgrad_args A, float* __restrict__ ws, int pix_per_split,
                                                   int col_tiles, int tiles_per_sub, int cols_max,
                                                   const wg_bounds WB) {
  static_assert(NA * NB == 8 * WN, "8 waves of 64 x (64 WN)");
  constexpr int NBW = NB / WN;           // wave columns
  static_assert(KP == 32 || KP == 64, "K step");
  static_assert(STAGES == 2 || STAGES == 3, "ring depth");
  constexpr int NP = NA + NB;            // panels per stage
  constexpr int PB = KP * 128;           // panel bytes
  constexpr int SB = NP * PB;            // stage bytes
  constexpr int IPP = KP / 8;            // wave-instructions per panel
  constexpr int NI = NP * IPP;           // wave-instructions per stage
  constexpr int JPW = (NI + 7) / 8;      // per wave (the last may be idle)
  static_assert(SB * STAGES <= 160 * 1024, "LDS");
  __shared__ uint4 lds0[SB / 16];
  __shared__ uint4 lds1[SB / 16];
  __shared__ uint4 lds2[STAGES == 3 ? SB / 16 : 1];
  auto bufp = [&](auto i_c) -> uint4* {
    constexpr int i = decltype(i_c)::value;
    if constexpr (i == 0) return lds0;
    else if constexpr (i == 1) return lds1;
    else return lds2;
  };

  // 1-D grid, XCD-aware: workgroups are dispatched round-robin over the 8 XCDs (separate L2s);
  // remap so that each XCD walks a contiguous range of (split, sub, tile) with the tiles
  // fastest -- every tile of one split reads the same dy / x pixel rows, which then meet in one
  // L2 instead of being fetched by all eight.
  const int total = gridDim.x;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, pos = bid >> 3, q8 = total >> 3, r8 = total & 7;  // bijective for any total
  const int lin = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  const int tiles = tiles_per_sub;
  const int tile = lin % tiles;
  const int rest = lin / tiles;
  const int sub = rest % A.nsub;
  const int split = rest / A.nsub;
  const auto& S = A.sub[sub];
  const int cols = S.ntaps * A.Cin;
  const int ct = tile % col_tiles, cot = tile / col_tiles;
  const int col0 = ct * 64 * NB, co0 = cot * 64 * NA;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wa = wid / NBW, wb = wid % NBW;  // wave (co panel, group of WN column panels)
  const int GHW = A.GH * A.GW;
  const int M = A.N * GHW;
  const int pbeg = split * pix_per_split;
  const int pend = min(M, pbeg + pix_per_split);
  const int nK = pend > pbeg ? (pend - pbeg + KP - 1) / KP : 0;

  // ---- staging state of this lane: pixel row R, source chunk of every panel
  const int rowblk = (KP == 64) ? wid : (wid & 3);
  // panel of this wave's j-th wave-instruction (instruction q = wid + 8 j, IPP per panel)
  auto panel_of = [&](int j) { return KP == 64 ? j : 2 * j + ((wid >> 2) & 1); };
  const int R = rowblk * 8 + (lane >> 3);
  const int lchunk = (lane & 7) ^ wg_swz(R);
  const int cout8 = (A.Cout + 7) & ~7;
  int poff[NP];        // per-panel lane offset (bytes; x panels: relative to the pixel base)
  int pty[NP], ptx[NP];
  bool pok[NP];
#pragma unroll
  for (int P = 0; P < NP; ++P) {
    if (P < NA) {
      const int ch = co0 + 64 * P + 8 * lchunk;
      pok[P] = ch < cout8;
      poff[P] = (S.cdy0 + ch) * 2;
      pty[P] = ptx[P] = 0;
    } else {
      const int col = col0 + 64 * (P - NA) + 8 * lchunk;
      pok[P] = col < cols;
      const int t = pok[P] ? col / A.Cin : 0;
      const int ci = col - t * A.Cin;
      pty[P] = S.ty[t];
      ptx[P] = S.tx[t];
      poff[P] = ((pty[P] * A.IW + ptx[P]) * A.ldx + A.cx0 + ci) * 2;
    }
  }
  // grid point of the next step to issue
  int pn, pgy, pgx;
  {
    const int p = min(pbeg + R, M - 1);
    pn = p / GHW;
    const int rr = p - pn * GHW;
    pgy = rr / A.GW;
    pgx = rr - pgy * A.GW;
  }
  int pnext = pbeg + R;
#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)A.x, (short)0, (int)WB.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t drsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)S.dy, (short)0, (int)WB.dy_bytes[sub], 0x00020000);
#endif

  auto issue = [&](uint4* dst) {
    const bool pv = pnext < pend;
    const unsigned dbase =
        (unsigned)((((pn * S.OH + pgy * S.oys + S.oyo) * S.OW + pgx * S.oxs + S.oxo) * S.lddy) * 2);
    const int iy0 = pgy * A.sy, ix0 = pgx * A.sx;
    const int xbase = (((pn * A.IH + iy0) * A.IW + ix0) * A.ldx) * 2;
    unsigned voff[JPW];
#pragma unroll
    for (int j = 0; j < JPW; ++j) {
      const int P = panel_of(j);  // wave-uniform (compile-time for KP 64)
      voff[j] = 0x80000000u;
      if (P < NA) {
        if (pv && pok[P]) voff[j] = dbase + (unsigned)poff[P];
      } else if (P < NP) {
        const int iy = iy0 + pty[P], ix = ix0 + ptx[P];
        if (pv && pok[P] && (unsigned)iy < (unsigned)A.IH && (unsigned)ix < (unsigned)A.IW)
          voff[j] = (unsigned)(xbase + poff[P]);
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int j = 0; j < JPW; ++j) {
      const int P = panel_of(j);
      if (P >= NP) continue;
      auto* d = (__attribute__((address_space(3))) void*)((unsigned char*)dst + P * PB + rowblk * 1024);
      if (P < NA) __builtin_amdgcn_raw_ptr_buffer_load_lds(drsrc, d, 16, voff[j], 0, 0, 0);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, d, 16, voff[j], 0, 0, 0);
    }
#endif
    pnext += KP;
    if (A.GW >= 16) {  // at most KP / 16 row wraps per step: predicated, no loop
      pgx += KP;
#pragma unroll
      for (int it = 0; it < KP / 16; ++it) {
        if (pgx >= A.GW) {
          pgx -= A.GW;
          if (++pgy == A.GH) {
            pgy = 0;
            ++pn;
          }
        }
      }
    } else {  // tiny grids (1x1 image-pool branch): divide
      const int p = min(pnext, M - 1);
      pn = p / GHW;
      const int rr = p - pn * GHW;
      pgy = rr / A.GW;
      pgx = rr - pgy * A.GW;
    }
  };

  f32x4 acc[4][4 * WN];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4 * WN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment read addresses: lane (g, 4q+p) -> row 8g + q, byte 8p of the 16-column block,
  // 16-column block ii at chunk pair 2*(ii ^ s'), s' = s(R) / 2 (independent of the +4 / +32
  // row offsets, which are immediates)
  const int g = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  const int sh = (((q4 >> 1) & 1) | ((g & 1) << 1));
  unsigned ra[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) ra[ii] = (unsigned)(wa * PB) + (unsigned)(128 * (8 * g + q4) + 8 * p4 + 32 * (ii ^ sh));
  // column panel w of this wave = panel NA + wb * WN + w: an immediate offset w * PB

  auto step = [&](auto cur_c, auto nxt_c, int ks) {
    const bool more = ks + (STAGES - 1) < nK;
    if constexpr (ZP_ABL != 1) {
      if (more) issue(bufp(nxt_c));
    }
    const unsigned cb = lds_addr(bufp(cur_c));
    unsigned pa[4], pb[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      pa[ii] = cb + ra[ii];
      pb[ii] = pa[ii] + (unsigned)((NA + wb * WN - wa) * PB);
    }
    static_for<KP / 32>([&](auto s2) {
      uint4 af[4], bfr[4 * WN];
      static_for<4>([&](auto ii) {
        const uint2 a0 = ds_read_tr8<s2 * 4096>(pa[ii]);
        const uint2 a1 = ds_read_tr8<s2 * 4096 + 512>(pa[ii]);
        af[ii] = make_uint4(a0.x, a0.y, a1.x, a1.y);
        static_for<WN>([&](auto w) {
          const uint2 b0 = ds_read_tr8<w * PB + s2 * 4096>(pb[ii]);
          const uint2 b1 = ds_read_tr8<w * PB + s2 * 4096 + 512>(pb[ii]);
          bfr[w * 4 + ii] = make_uint4(b0.x, b0.y, b1.x, b1.y);
        });
      });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      if constexpr (ZP_ABL != 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4 * WN; ++j) MfmaTraits<bf16_t>::mma(acc[i][j], af[i], bfr[j]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][0][0] += __uint_as_float(af[i].x ^ bfr[i].y);
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(0);
    });
    if (more) vm_wait<JPW * (STAGES - 2)>();
    else vm_wait<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  if (nK > 0) {
    issue(lds0);
    if (STAGES == 3 && nK > 1) {
      issue(lds1);
      vm_wait<JPW * (STAGES - 2)>();
    } else {
      vm_wait<0>();
    }
  }
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
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
  // partial tile -> ws[((split*nsub + sub)*Cout + co)*cols_max + col]
  float* W = ws + ((size_t)split * A.nsub + sub) * (size_t)A.Cout * cols_max;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4 * WN; ++j) {
      const int col = col0 + wb * WN * 64 + j * 16 + (lane & 15);
      if (col >= cols) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wa * 64 + i * 16 + g * 4 + r;
        if (co < A.Cout) W[(size_t)co * cols_max + col] = acc[i][j][r];
      }
    }
}

// ------------------------------------------------------------------------------------
// k_wgrad2: k_wgrad_lds's product (same tiles, same panels, same fragment reads, same partial
// layout) with a lean issue path for the common geometry: one sub-problem, stride 1, dy on the
// input grid (same-size convs: every 3x3 d-conv and 1x1 of the network), W in {32, 64, 128},
// images a multiple of the 64-pixel step, Cin and the dy channel slice 64-aligned.  Then the
// pixel offset of a lane's row in dy and x is LINEAR in the pixel index: the per-step offset is
// one scalar (p * ld * 2) added by the buffer unit; per lane only constant row / channel /
// tap offsets are kept, and a tap's row validity is wave-uniform per step (a 64-pixel step is
// one image row at W 64, half a row at W 128, two rows at W 32 whose halves are waves 0-3 and
// 4-7), its column validity a per-lane constant (W 128: one of two).  k_wgrad_lds, profiled on
// the 256->256 3x3 at 128x128 (bs 32), spent 1.4 VALU + 1.0 SALU per MFMA on per-step pixel
// arithmetic and ran the MFMA pipe 34% busy.
// Stride 2 (round 6; the input grid twice the output grid): a lane's x pixel is (S (gy + rh) + ty,
// S gx + tx) -- per lane (S rh + ty) IW + S gx + tx, per step the image and row (n IH + S gy) IW
// (+ S 64 for the second half of a W 128 row).  That covers the stride-2 convs and, with x and dy
// exchanged, the ConvTranspose2d(3, s2, p1, op1) weight gradient: dW[ci][co][ky][kx] = sum_g
// x[g][ci] dy[2 g + (ky, kx) - 1][co] is the weight gradient of the stride-2 conv over dy whose
// output gradient is x (geometry.convT_dgrad's plan; the engine's _wgrad).
// ------------------------------------------------------------------------------------
template <int NA, int NB, int STAGES, int WN>
__global__ void __launch_bounds__(512) k_wgrad2(const zp_wgrad_args A, float* __restrict__ ws, int pix_per_split,
                                                int col_tiles, int tiles_per_sub, int cols_max, const wg_bounds WB) {
  constexpr int KP = 64;
  static_assert(NA * NB == 8 * WN, "8 waves of 64 x (64 WN)");
  constexpr int NBW = NB / WN;
  constexpr int NP = NA + NB;   // panels per stage; wave w fills rows 8w..8w+7 of every panel
  constexpr int PB = KP * 128;  // panel bytes
  constexpr int SB = NP * PB;   // stage bytes
  static_assert(SB * STAGES <= 160 * 1024, "LDS");
  __shared__ uint4 lds[STAGES * SB / 16];

  // XCD-aware order (bijective for any total): each XCD walks a contiguous run of (split, tile),
  // tiles fastest, so the tiles of one split (same dy / x pixel rows) share an L2
  const int total = gridDim.x;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, pos = bid >> 3, q8 = total >> 3, r8 = total & 7;
  const int lin = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  const int tile = lin % tiles_per_sub;
  const int split = lin / tiles_per_sub;  // one sub-problem
  const auto& S = A.sub[0];
  const int cols = S.ntaps * A.Cin;
  const int ct = tile % col_tiles, cot = tile / col_tiles;
  const int col0 = ct * 64 * NB, co0 = cot * 64 * NA;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wa = wid / NBW, wb = wid % NBW;
  const int W = A.GW, GHW = A.GH * A.GW;
  const int M = A.N * GHW;
  const int pbeg = split * pix_per_split;
  const int pend = min(M, pbeg + pix_per_split);
  const int nK = pend > pbeg ? (pend - pbeg) / KP : 0;

  const int R = wid * 8 + (lane >> 3);  // this lane's pixel row within a step
  const int lchunk = (lane & 7) ^ wg_swz(R);
  const int cout8 = (A.Cout + 7) & ~7;
  const int rh = W == 32 ? (wid >> 2) : 0;  // image-row offset of this wave's rows (wave-uniform)
  const int gxl = W == 32 ? (R & 31) : R;   // column (W 128: + 64 * xh)
  const int SS = A.sy;                      // input stride (1, or 2 with IH = 2 GH, IW = 2 GW)
  // per panel: lane offsets (dy: row + channel; x: row + tap + channel, with column validity folded
  // in as an out-of-range offset), tap row of x panels (wave-uniform)
  unsigned vdy[NA];
  int vx[NB];                // x: row + tap + channel offset (bytes; may be negative, the step adds p)
  bool okx0[NB], okx1[NB];   // column validity (W 128: column half 0 / 1)
  int tyP[NB];
#pragma unroll
  for (int P = 0; P < NA; ++P) {
    const int ch = co0 + 64 * P + 8 * lchunk;
    vdy[P] = ch < cout8 ? (unsigned)((R * S.lddy + S.cdy0 + ch) * 2) : 0x80000000u;
  }
#pragma unroll
  for (int P = 0; P < NB; ++P) {
    const int col = col0 + 64 * P + 8 * lchunk;
    const bool ok = col < cols;
    const int t = ok ? col / A.Cin : 0;
    const int ci = col - t * A.Cin;
    const int ty = S.ty[t], tx = S.tx[t];
    tyP[P] = __builtin_amdgcn_readfirstlane(S.ty[(col0 + 64 * P) / A.Cin < S.ntaps ? (col0 + 64 * P) / A.Cin : 0]);
    vx[P] = ((SS * rh + ty) * A.IW + SS * gxl + tx) * A.ldx * 2 + (A.cx0 + ci) * 2;
    okx0[P] = ok && (unsigned)(SS * gxl + tx) < (unsigned)A.IW;
    okx1[P] = ok && (unsigned)(SS * (gxl + 64) + tx) < (unsigned)A.IW;
  }
#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)A.x, (short)0, (int)WB.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc((void*)S.dy, (short)0, (int)WB.dy_bytes[0], 0x00020000);
#endif
  // scalar walk: pixel p of the next step to issue, its image row gy and (W 128) column half xh
  int p_is = pbeg;
  int gy_is, xh_is, n_is = pbeg / GHW;
  {
    const int r = pbeg % GHW;
    gy_is = r / W;
    xh_is = W == 128 ? (r / 64) & 1 : 0;
  }
  const int ldy2 = S.lddy * 2, ldx2 = A.ldx * 2;
  auto issue = [&](auto slot_c) {
    constexpr int SL = decltype(slot_c)::value;
    const int sdy = p_is * ldy2;
    const int sx = ((n_is * A.IH + SS * gy_is) * A.IW + SS * 64 * xh_is) * ldx2;  // (S 1: p_is * ldx2)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int P = 0; P < NA; ++P) {
      auto* d = (__attribute__((address_space(3))) void*)((unsigned char*)lds + SL * SB + P * PB + wid * 1024);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(drsrc, d, 16, vdy[P], sdy, 0, 0);
    }
#pragma unroll
    for (int P = 0; P < NB; ++P) {
      // the full (non-negative when valid) offset in the VGPR: a lane offset below zero is never
      // handed to the buffer unit, whatever its range check does with the scalar part
      const bool rowok = (unsigned)(SS * (gy_is + rh) + tyP[P]) < (unsigned)A.IH;  // wave-uniform
      const bool ok = rowok && (xh_is ? okx1[P] : okx0[P]);
      const unsigned v = ok ? (unsigned)(vx[P] + sx) : 0x80000000u;
      auto* d = (__attribute__((address_space(3))) void*)((unsigned char*)lds + SL * SB + (NA + P) * PB + wid * 1024);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, d, 16, v, 0, 0, 0);
    }
#endif
    // advance one 64-pixel step (images are whole steps: GHW % 64 == 0)
    p_is += KP;
    if (W == 128) {
      xh_is ^= 1;
      if (xh_is == 0) ++gy_is;
    } else {
      gy_is += KP / W;
    }
    if (gy_is >= A.GH) {
      gy_is = 0;
      ++n_is;
    }
  };

  f32x4 acc[4][4 * WN];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4 * WN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  const int sh = (((q4 >> 1) & 1) | ((g & 1) << 1));
  const unsigned l0 = lds_addr(lds);
  unsigned pa[STAGES][4], pb[STAGES][4];  // per ring slot (slot offsets exceed the ds immediate)
#pragma unroll
  for (int sl = 0; sl < STAGES; ++sl)
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      pa[sl][ii] = l0 + (unsigned)(sl * SB + wa * PB) + (unsigned)(128 * (8 * g + q4) + 8 * p4 + 32 * (ii ^ sh));
      pb[sl][ii] = pa[sl][ii] + (unsigned)((NA + wb * WN - wa) * PB);
    }
  auto step = [&](auto cur_c, auto nxt_c, int ks) {
    constexpr int CUR = decltype(cur_c)::value;
    const bool more = ks + (STAGES - 1) < nK;
    if constexpr (ZP_ABL != 1) {
      if (more) issue(nxt_c);
    }
    static_for<KP / 32>([&](auto s2) {
      uint4 af[4], bfr[4 * WN];
      static_for<4>([&](auto ii) {
        const uint2 a0 = ds_read_tr8<s2 * 4096>(pa[CUR][ii]);
        const uint2 a1 = ds_read_tr8<s2 * 4096 + 512>(pa[CUR][ii]);
        af[ii] = make_uint4(a0.x, a0.y, a1.x, a1.y);
        static_for<WN>([&](auto w) {
          const uint2 b0 = ds_read_tr8<w * PB + s2 * 4096>(pb[CUR][ii]);
          const uint2 b1 = ds_read_tr8<w * PB + s2 * 4096 + 512>(pb[CUR][ii]);
          bfr[w * 4 + ii] = make_uint4(b0.x, b0.y, b1.x, b1.y);
        });
      });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      if constexpr (ZP_ABL != 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4 * WN; ++j) MfmaTraits<bf16_t>::mma(acc[i][j], af[i], bfr[j]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][0][0] += __uint_as_float(af[i].x ^ bfr[i].y);
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(0);
    });
    if (more) vm_wait<NP * (STAGES - 2)>();
    else vm_wait<0>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  if (nK > 0) {
    issue(I0{});
    if (STAGES == 3 && nK > 1) {
      issue(I1{});
      vm_wait<NP * (STAGES - 2)>();
    } else {
      vm_wait<0>();
    }
  }
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
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
  float* Wp = ws + (size_t)split * (size_t)A.Cout * cols_max;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4 * WN; ++j) {
      const int col = col0 + wb * WN * 64 + j * 16 + (lane & 15);
      if (col >= cols) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wa * 64 + i * 16 + g * 4 + r;
        if (co < A.Cout) Wp[(size_t)co * cols_max + col] = acc[i][j][r];
      }
    }
}

// ws (summed over splits) -> dw in the weight's own layout.  Per element the splits are summed into
// 8 partial sums (split k into q[k % 8] for the whole batches of 8, the rest into q[0]), combined as
// ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)): fixed order, deterministic.  (Round 5) up to 32
// splits' loads are issued before their adds (the same adds in the same order as batches of 8; one
// batch of 8 in flight left the launch bound by 3-4 dependent memory round trips per thread), and
// the element index is 32-bit.
__global__ void __launch_bounds__(256) k_wgrad_reduce(const zp_wgrad_args A, const float* __restrict__ ws, int splits,
                                                      int cols_max) {
  const int sub = blockIdx.y;
  const auto& S = A.sub[sub];
  const unsigned cols = (unsigned)(S.ntaps * A.Cin);
  const unsigned total = (unsigned)A.Cout * cols;
  const size_t stride = (size_t)A.nsub * A.Cout * cols_max;
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const unsigned co = e / cols, col = e - co * cols;
    const int t = (int)(col / (unsigned)A.Cin), ci = (int)col - t * A.Cin;
    const int ky = S.ky[t], kx = S.kx[t];
    if (ci >= A.Cw || ky < 0) continue;  // padded input channels / padding taps
    const float* p = ws + ((size_t)sub * A.Cout + co) * cols_max + col;
    float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 32 <= splits; k += 32) {
      float v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] += v[8 * b + u];
    }
    if (k + 16 <= splits) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] += v[8 * b + u];
      k += 16;
    }
    if (k + 8 <= splits) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] += v[u];
      k += 8;
    }
    {
      float v[7];  // the remaining < 8 splits, loaded together, added to q[0] in split order
#pragma unroll
      for (int u = 0; u < 7; ++u) v[u] = k + u < splits ? p[(size_t)(k + u) * stride] : 0.f;
#pragma unroll
      for (int u = 0; u < 7; ++u)
        if (k + u < splits) q[0] += v[u];
    }
    const float s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    size_t idx = A.transposed_w ? (((size_t)ci * A.Cout + co) * A.kh + ky) * A.kw + kx
                                : (((size_t)co * A.Cw + ci) * A.kh + ky) * A.kw + kx;
    if (A.accumulate) A.dw[idx] += s;
    else A.dw[idx] = s;
  }
}


// ------------------------------------------------------------------------------------ host
// zp_conv_tuning key 3: k_wgrad2 (0 disables it); key 4: its workgroup rounds over the CUs (default
// 1: fewer, longer workgroups than k_wgrad_lds's 1024 -- the split-K partial slabs are written and
// re-read in full -- and never a partial extra round; one round measured fastest); key 5:
// k_wgrad_lds's workgroup rounds (0: the older ~1024-workgroup target)
static int g_wgrad2 = 1, g_wgrad2_rounds = 1, g_wgrad_lds_rounds = 1;

int wgrad_tuning(int key, int v) {
  int& g = key == 3 ? g_wgrad2 : key == 4 ? g_wgrad2_rounds : g_wgrad_lds_rounds;
  const int old = g;
  g = key == 3 ? v : key == 4 ? (v > 0 ? v : 1) : (v >= 0 ? v : 1);
  return old;
}

// bf16: the LDS-DMA kernels.  ZP_WGRAD=0 selects the register-staged k_wgrad.
static bool wgrad_lds(const zp_wgrad_args& a) {
  static const int v = getenv("ZP_WGRAD") ? env_int("ZP_WGRAD") : 1;
  return a.dtype == ZP_BF16 && v != 0;
}
// k_wgrad2 (lean issue path) for the common geometry -- see the kernel's header comment
static bool wgrad2_eligible(const zp_wgrad_args& a) {
  if (!g_wgrad2 || a.dtype != ZP_BF16 || a.nsub != 1 || a.sy != a.sx || (a.sy != 1 && a.sy != 2)) return false;
  if (a.IH != a.sy * a.GH || a.IW != a.sx * a.GW || (a.GW != 32 && a.GW != 64 && a.GW != 128)) return false;
  if (((long)a.GH * a.GW) % 64 != 0 || a.Cin % 64 != 0) return false;
  const auto& S = a.sub[0];
  return S.oys == 1 && S.oxs == 1 && S.oyo == 0 && S.oxo == 0 && S.OH == a.GH && S.OW == a.GW;
}
// LDS-DMA tile: 0 = 64 co x 512 col (Cout <= 64), 1 = 128 x 256, 2 = 256 x 256 (Cout >= 256: fewer
// staged bytes per FLOP -- the L2 -> LDS stream, not the MFMA, bounds this kernel).  Round 5: a
// k_wgrad2 launch whose 256 x 256 plan would give each split under 2048 pixels takes 128 x 256
// instead -- few tiles (a 3x3 256 -> 256 at 32 x 32 has 9) mean ~28 splits, and each split writes a
// 256 KB f32 partial slab (64 MB per launch, re-read by k_wgrad_reduce) for 1216 pixels of MFMA
// work: measured 739 -> 679 us over layer4's 11 wgrads, the 1 x 1 convs 43 -> 32 us; the 128 x 128
// decoder / layer5 wgrads (18724 / 4681 pixels per split) stay on 256 x 256 (1116 vs 1328 us).
// ZP_WGRAD_BIG=0: always 128 x 256; 2: always 256 x 256 (A/B)
static int wgrad_cfg(const zp_wgrad_args& a, bool lean, int cols_max, long M) {
  static const int big = getenv("ZP_WGRAD_BIG") ? env_int("ZP_WGRAD_BIG") : 1;
  if (a.Cout <= 64) return 0;
  if (a.Cout < 256 || !big) return 1;
  // (round 6) a Cout the 256-row tiles would pad by more than the 128-row ones (320: 512 against
  // 384 rows -- the ConvT weight gradient as the stride-2 conv over dy) takes 128 x 256: measured
  // 276 -> 261 us for up2's ConvT (tools/wgrad_ab.py, profiles/r06_conv_ablations.md)
  if (big == 1 && (a.Cout + 255) / 256 * 256 > (a.Cout + 127) / 128 * 128) return 1;
  if (big == 1 && lean) {
    // (the 256 x 256 plan's requested splits, before rounding to whole K steps)
    const long tiles = (long)ceil_div(cols_max, 256) * ceil_div(a.Cout, 256);
    long sp = (long)g_wgrad2_rounds * num_cus() / tiles;
    const long maxsp = M / (16 * 64) > 0 ? M / (16 * 64) : 1;
    sp = sp < 1 ? 1 : (sp > maxsp ? maxsp : sp);
    if (M / sp < 2048) return 1;
  }
  return 2;
}

// One weight-gradient launch: the kernel, its tile and split-K shape, and the grid.  The workspace
// query and the launch both read it.
enum wgrad_kernel { WG_REG, WG_LDS, WG_LEAN };  // k_wgrad, k_wgrad_lds, k_wgrad2
struct wgrad_launch {
  wgrad_kernel kernel;
  int cfg, tco, tcol;  // LDS-DMA tile (wgrad_cfg): output channels x columns
  int splits, col_tiles, cols_max, pix_per;
  int tiles;  // (co x col) tiles per sub-problem
  dim3 grid;
};

static wgrad_launch plan_wgrad(const zp_wgrad_args& a) {
  wgrad_launch p{};
  const long M = (long)a.N * a.GH * a.GW;
  for (int s = 0; s < a.nsub; ++s) p.cols_max = std::max(p.cols_max, a.sub[s].ntaps * a.Cin);
  int KP, min_steps;  // pixels per K step, fewest K steps per split
  long sp;            // splits asked for
  if (!wgrad_lds(a)) {
    p.kernel = WG_REG;
    p.tco = p.tcol = WG_TILE;
    KP = a.dtype == ZP_BF16 ? 32 : 16;
    min_steps = 8;
  } else {
    // tile 128 co x 256 col (3 stages), 64 x 512 (2 stages) when Cout <= 64, or 256 x 256; KP 64.
    // One workgroup per CU (96-144 KB LDS), each with >= 16 K steps.
    const bool lean = wgrad2_eligible(a);
    p.kernel = lean ? WG_LEAN : WG_LDS;
    p.cfg = wgrad_cfg(a, lean, p.cols_max, M);
    p.tco = 64 << p.cfg;
    p.tcol = p.cfg == 0 ? 512 : 256;
    KP = 64;
    min_steps = 16;
  }
  p.col_tiles = ceil_div(p.cols_max, p.tcol);
  p.tiles = p.col_tiles * ceil_div(a.Cout, p.tco);
  const int tiles = p.tiles * a.nsub;
  // k_wgrad_lds's target workgroup count when key 5 is 0: 1024 (R34 bs 32 train step 19.93 ->
  // 19.71 ms vs 512; 2048: 19.81).  ZP_WGRAD_WG overrides for sweeps (read once)
  static const int target_lds = getenv("ZP_WGRAD_WG") ? env_int("ZP_WGRAD_WG") : 1024;
  // k_wgrad: aim for >= 1024 workgroups.  k_wgrad2: workgroups in whole rounds over the CUs -- a
  // grid one workgroup past a round costs a full extra workgroup lifetime (513 vs 512 ran 1.6x).
  // k_wgrad_lds: the same whole-round plan when zp_conv_tuning key 5 > 0, else ~target_lds workgroups
  const bool padded = p.kernel == WG_LDS && g_wgrad_lds_rounds <= 0;
  if (p.kernel == WG_REG) sp = (1024 + tiles - 1) / tiles;
  else if (p.kernel == WG_LEAN) sp = (long)g_wgrad2_rounds * num_cus() / tiles;
  else sp = padded ? (target_lds + tiles - 1) / tiles : (long)g_wgrad_lds_rounds * num_cus() / tiles;
  const long maxsp = std::max(1L, M / (min_steps * KP));
  sp = std::min(std::max(sp, 1L), std::min(maxsp, 256L));
  long pp = (M + sp - 1) / sp;
  pp = (pp + KP - 1) / KP * KP;
  sp = (M + pp - 1) / pp;  // never more than requested: pp only grew
  // k_wgrad_lds's older plan: pad the split count so the launch is a multiple of 8 workgroups (its
  // XCD-aware order needs it); padding splits have an empty pixel range and write zero partials
  if (padded)
    while ((sp * tiles) % 8) ++sp;
  p.splits = (int)sp;
  p.pix_per = (int)pp;
  p.grid = p.kernel == WG_REG ? dim3(p.splits, p.tiles, a.nsub) : dim3(p.splits * tiles);
  return p;
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_conv2d_wgrad_ws_bytes(const zp_wgrad_args* a) {
  if (!a || a->nsub < 1 || a->nsub > ZP_MAX_SUB) return -1;
  const wgrad_launch p = plan_wgrad(*a);
  return (long long)p.splits * a->nsub * a->Cout * (long long)p.cols_max * 4;
}

extern "C" int zp_conv2d_wgrad(const zp_wgrad_args* ap, void* ws, void* stream) {
  ZP_CHECK_ARG(ap && ws, "zp_conv2d_wgrad: null args/workspace");
  const zp_wgrad_args& a = *ap;
  ZP_CHECK_ARG(a.dtype == ZP_F32 || a.dtype == ZP_BF16, "zp_conv2d_wgrad: dtype");
  ZP_CHECK_ARG(a.nsub >= 1 && a.nsub <= ZP_MAX_SUB && a.dw && a.x, "zp_conv2d_wgrad: bad args");
  const int E = a.dtype == ZP_BF16 ? 8 : 4;
  ZP_CHECK_ARG(a.Cin % E == 0 && a.cx0 % E == 0 && a.ldx % E == 0, "zp_conv2d_wgrad: Cin/cx0/ldx alignment");
  ZP_CHECK_ARG(a.Cw >= 1 && a.Cw <= a.Cin, "zp_conv2d_wgrad: Cw");
  for (int s = 0; s < a.nsub; ++s) {
    ZP_CHECK_ARG(a.sub[s].dy && a.sub[s].ntaps >= 1 && a.sub[s].ntaps <= ZP_MAX_TAPS, "zp_conv2d_wgrad: sub %d", s);
    ZP_CHECK_ARG(a.sub[s].cdy0 % E == 0 && a.sub[s].lddy % E == 0 &&
                 a.sub[s].lddy >= a.sub[s].cdy0 + ((a.Cout + E - 1) / E) * E,
                 "zp_conv2d_wgrad: dy ld must cover Cout rounded to %d", E);
  }
  const wgrad_launch p = plan_wgrad(a);
  hipStream_t st = (hipStream_t)stream;
  if (p.kernel == WG_REG) {
    if (a.dtype == ZP_BF16)
      hipLaunchKernelGGL(k_wgrad<bf16_t>, p.grid, dim3(256), 0, st, a, (float*)ws, p.pix_per, p.col_tiles, p.cols_max);
    else
      hipLaunchKernelGGL(k_wgrad<float>, p.grid, dim3(256), 0, st, a, (float*)ws, p.pix_per, p.col_tiles, p.cols_max);
  } else {
    wg_bounds wb{};
    const long long xb = (long long)a.N * a.IH * a.IW * a.ldx * 2;
    ZP_CHECK_ARG(xb < (1ll << 31), "zp_conv2d_wgrad: input %lld B must stay below 2 GiB (split the batch)", xb);
    wb.x_bytes = (unsigned)xb;
    for (int s = 0; s < a.nsub; ++s) {
      const long long db = (long long)a.N * a.sub[s].OH * a.sub[s].OW * a.sub[s].lddy * 2;
      ZP_CHECK_ARG(db < (1ll << 31), "zp_conv2d_wgrad: dy %lld B must stay below 2 GiB", db);
      wb.dy_bytes[s] = (unsigned)db;
    }
#define ZP_WG(...) \
  hipLaunchKernelGGL((__VA_ARGS__), p.grid, dim3(512), 0, st, a, (float*)ws, p.pix_per, p.col_tiles, p.tiles, p.cols_max, wb)
    if (p.kernel == WG_LEAN) {
      if (p.cfg == 0) ZP_WG(k_wgrad2<1, 8, 2, 1>);
      else if (p.cfg == 1) ZP_WG(k_wgrad2<2, 4, 3, 1>);
      else ZP_WG(k_wgrad2<4, 4, 2, 2>);
    } else {
      if (p.cfg == 0) ZP_WG(k_wgrad_lds<64, 1, 8, 2, 1>);
      else if (p.cfg == 1) ZP_WG(k_wgrad_lds<64, 2, 4, 3, 1>);
      else ZP_WG(k_wgrad_lds<64, 4, 4, 2, 2>);
    }
#undef ZP_WG
  }
  ZP_LAUNCH_CHECK("zp_conv2d_wgrad");
  long tot = (long)a.Cout * p.cols_max;
  int rb = (int)((tot + 255) / 256);
  if (rb > 4096) rb = 4096;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3(rb, a.nsub), dim3(256), 0, st, a, (const float*)ws, p.splits, p.cols_max);
  ZP_LAUNCH_CHECK("zp_conv2d_wgrad reduce");
  return ZP_OK;
}
