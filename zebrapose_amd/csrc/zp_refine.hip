// Edge refinement on the device: the visible contour of a mask crop (zp_mask_contour) and one
// Gauss-Newton step of the pose against it (zp_edge_refine_step).
// Reference: test.py:300-307 (contour of the entire mask, filtered by the visible mask, mapped to the
// image) and edge_refine/examples/edge_refine.cpp:68-173 (render, silhouette contour, nearest-contour
// match, 6 x 6 normal equations, pose update).  The contracts are in include/zp.h; tests/refine_ref.py
// restates them in numpy.
//
// Both kernels run one workgroup per image and share the contour machinery.  A binary image lives
// in LDS as one bit per pixel, rows padded to whole 32-bit words (WW words a row), twice: the set
// pixels S and the outside O.
//   load:    a lane per pixel, one wave ballot per 64 pixels (coalesced reads), and the bounding box
//            of the set pixels.
//   fill:    O starts as the unset pixels on the perimeter of the bounding box grown by one (clipped
//            to the image: those are next to the ring of unset pixels the definition pads with, or
//            lie outside the tight box, where everything is unset and connected to the ring).  A
//            pass closes every row under left / right steps (a thread per row: a Kogge-Stone fill
//            inside a word, a carry between words) and then every column of words under up / down
//            steps (a thread per word column, 32 pixel columns at once).  Passes repeat until one
//            changes nothing; the fixed point is the 4-connected outside whatever the order.  The
//            pass count is capped at 4 (H + W): no input can spin the kernel.
//   border:  S & (O shifted to the four neighbours | the ring), written over S.
//   compact: popcount per thread chunk, a block scan, and the pixels in row-major order.
// The step keeps the first RF_BL border pixels in LDS and the rest in the workspace.  Matching is a
// thread per observed point over the whole border list (every lane reads the same entry: an LDS
// broadcast); squared distances are integers below 2^44 held exactly in f64.  H and b are summed per
// thread in point order, then by a shuffle tree per wave and a fixed tree over the eight waves: no
// floating-point atomics, so a rerun gives the same bits.  Lane 0 solves by Cholesky and updates.
// Built with -ffp-contract=off: the crop -> image mapping is a multiply then an add, as numpy does it.
#include <limits.h>
#include <math.h>
#include "zp_common.h"

namespace zp {

constexpr int RF_T = 512;              // threads per workgroup (8 waves; the ballots need a multiple of 64)
constexpr int RF_WAVES = RF_T / 64;
constexpr int RF_MAX_BITS = 1 << 19;   // padded bits per mask: 64 KB of LDS each
constexpr int RF_BL = 4096;            // border pixels kept in LDS; the rest go to the workspace
constexpr int RF_MIN_BORDER = 20;      // edge_refine.cpp:85-86
constexpr int RF_SAT = 1 << 20;        // observed coordinates saturate here
constexpr int RF_NACC = 27;            // upper triangle of H (21) + b (6)

struct Grid {
  int H, W, WW;
  uint32_t* S;
  uint32_t* O;
};

struct IsSetDepth {
  static __device__ __forceinline__ bool test(float v) { return v > 0.f; }
};
struct IsSetU8 {
  static __device__ __forceinline__ bool test(uint8_t v) { return v != 0; }
};

// img [H][W] -> bits dst [H][WW]; box (LDS, 4 ints: x0, y0, x1, y1; x1 = -1 when nothing is set) if asked for
template <typename T, typename P>
__device__ void load_mask(const T* __restrict__ img, const Grid& g, uint32_t* dst, int* box) {
  const int tid = threadIdx.x;
  if (box && tid < 4) box[tid] = tid < 2 ? INT_MAX : -1;
  __syncthreads();
  const int nbits = g.H * g.WW * 32, npad = (nbits + 63) & ~63;
  int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  for (int i = tid; i < npad; i += RF_T) {  // trip count is uniform over a wave
    const int wd = i >> 5, y = wd / g.WW, x = ((wd - y * g.WW) << 5) | (i & 31);
    bool set = false;
    if (i < nbits && x < g.W) set = P::test(img[(size_t)y * g.W + x]);
    const unsigned long long m = __ballot(set);
    if ((tid & 31) == 0 && i < nbits) dst[wd] = (uint32_t)(m >> (tid & 32));
    if (set) {
      x0 = min(x0, x), x1 = max(x1, x);
      y0 = min(y0, y), y1 = max(y1, y);
    }
  }
  if (box && x1 >= 0) {
    atomicMin(&box[0], x0);
    atomicMin(&box[1], y0);
    atomicMax(&box[2], x1);
    atomicMax(&box[3], y1);
  }
  __syncthreads();
}

// g: seeds, p: free pixels; every free run above (below) a seed, towards higher (lower) bits
__device__ __forceinline__ uint32_t fill_up(uint32_t g, uint32_t p) {
  g |= p & (g << 1), p &= p << 1;
  g |= p & (g << 2), p &= p << 2;
  g |= p & (g << 4), p &= p << 4;
  g |= p & (g << 8), p &= p << 8;
  g |= p & (g << 16);
  return g;
}
__device__ __forceinline__ uint32_t fill_down(uint32_t g, uint32_t p) {
  g |= p & (g >> 1), p &= p >> 1;
  g |= p & (g >> 2), p &= p >> 2;
  g |= p & (g >> 4), p &= p >> 4;
  g |= p & (g >> 8), p &= p >> 8;
  g |= p & (g >> 16);
  return g;
}

// The outside of S into O.  Returns true when the pass cap was hit (the same in every thread).
__device__ bool fill_outside(const Grid& g, const int* box, int pass_cap) {
  const int tid = threadIdx.x, WW = g.WW;
  for (int i = tid; i < g.H * WW; i += RF_T) g.O[i] = 0;
  const int x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
  __syncthreads();
  if (x1 < 0) return false;
  const int xe0 = max(x0 - 1, 0), xe1 = min(x1 + 1, g.W - 1), ye0 = max(y0 - 1, 0), ye1 = min(y1 + 1, g.H - 1);
  const int we0 = xe0 >> 5, we1 = xe1 >> 5, nw = we1 - we0 + 1, nrows = ye1 - ye0 + 1;
  const uint32_t m0 = ~0u << (xe0 & 31), m1 = ~0u >> (31 - (xe1 & 31));
  const uint32_t b0 = 1u << (xe0 & 31), b1 = 1u << (xe1 & 31);
  auto colmask = [&](int w) { return (w == we0 ? m0 : ~0u) & (w == we1 ? m1 : ~0u); };
  for (int i = tid; i < nrows * nw; i += RF_T) {
    const int y = ye0 + i / nw, w = we0 + i % nw;
    const uint32_t F = ~g.S[y * WW + w] & colmask(w);
    g.O[y * WW + w] = (y == ye0 || y == ye1) ? F : (F & ((w == we0 ? b0 : 0u) | (w == we1 ? b1 : 0u)));
  }
  __syncthreads();
  for (int pass = 0; pass < pass_cap; ++pass) {
    int ch = 0;
    for (int y = ye0 + tid; y <= ye1; y += RF_T) {
      uint32_t* o = g.O + y * WW;
      const uint32_t* s = g.S + y * WW;
      uint32_t carry = 0;
      for (int w = we0; w <= we1; ++w) {
        const uint32_t F = ~s[w] & colmask(w), old = o[w];
        const uint32_t v = fill_up(old | (F & carry), F);
        if (v != old) o[w] = v, ch = 1;
        carry = v >> 31;
      }
      carry = 0;
      for (int w = we1; w >= we0; --w) {
        const uint32_t F = ~s[w] & colmask(w), old = o[w];
        const uint32_t v = fill_down(old | (F & (carry << 31)), F);
        if (v != old) o[w] = v, ch = 1;
        carry = v & 1u;
      }
    }
    __syncthreads();
    for (int w = we0 + tid; w <= we1; w += RF_T) {
      const uint32_t cm = colmask(w);
      uint32_t prev = g.O[ye0 * WW + w];
      for (int y = ye0 + 1; y <= ye1; ++y) {
        const uint32_t F = ~g.S[y * WW + w] & cm, old = g.O[y * WW + w], v = old | (F & prev);
        if (v != old) g.O[y * WW + w] = v, ch = 1;
        prev = v;
      }
      prev = g.O[ye1 * WW + w];
      for (int y = ye1 - 1; y >= ye0; --y) {
        const uint32_t F = ~g.S[y * WW + w] & cm, old = g.O[y * WW + w], v = old | (F & prev);
        if (v != old) g.O[y * WW + w] = v, ch = 1;
        prev = v;
      }
    }
    if (!__syncthreads_or(ch)) return false;
  }
  return true;
}

// S <- the outer border of S: the set pixels with a 4-neighbour in O or in the ring around the image
__device__ void border_inplace(const Grid& g, const int* box) {
  const int WW = g.WW, y0 = box[1], y1 = box[3];
  if (box[2] >= 0) {
    const uint32_t ring_r = 1u << ((g.W - 1) & 31);
    for (int i = threadIdx.x; i < (y1 - y0 + 1) * WW; i += RF_T) {
      const int y = y0 + i / WW, w = i % WW;
      const uint32_t s = g.S[y * WW + w];
      if (!s) continue;
      const uint32_t o = g.O[y * WW + w];
      const uint32_t l = (o << 1) | (w > 0 ? g.O[y * WW + w - 1] >> 31 : 1u);
      const uint32_t r = (o >> 1) | (w < WW - 1 ? g.O[y * WW + w + 1] << 31 : 0u) | (w == WW - 1 ? ring_r : 0u);
      const uint32_t u = y > 0 ? g.O[(y - 1) * WW + w] : ~0u;
      const uint32_t d = y < g.H - 1 ? g.O[(y + 1) * WW + w] : ~0u;
      g.S[y * WW + w] = s & (l | r | u | d);
    }
  }
  __syncthreads();
}

// emit(index, x, y) for every bit of S in rows box.y0 .. box.y1, in row-major order; returns their number
template <class Emit>
__device__ int compact(const Grid& g, const int* box, int* scan, Emit emit) {
  const int tid = threadIdx.x, WW = g.WW, y0 = box[1], y1 = box[3];
  if (box[2] < 0) return 0;
  const int nwr = (y1 - y0 + 1) * WW, C = (nwr + RF_T - 1) / RF_T;
  const int lo = min(tid * C, nwr), hi = min(lo + C, nwr);
  const uint32_t* base = g.S + y0 * WW;
  int c = 0;
  for (int i = lo; i < hi; ++i) c += __popc(base[i]);
  scan[tid] = c;
  __syncthreads();
  for (int off = 1; off < RF_T; off <<= 1) {
    const int v = tid >= off ? scan[tid - off] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int total = scan[RF_T - 1];
  int pos = scan[tid] - c;
  for (int i = lo; i < hi; ++i) {
    uint32_t m = base[i];
    const int y = y0 + i / WW, xb = (i % WW) << 5;
    while (m) {
      emit(pos++, xb + __ffs(m) - 1, y);
      m &= m - 1;
    }
  }
  __threadfence();
  __syncthreads();
  return total;
}

__global__ void __launch_bounds__(RF_T) k_mask_contour(const uint8_t* __restrict__ entire,
                                                       const uint8_t* __restrict__ visible,
                                                       const int* __restrict__ bbox, int S, int WW, int cap,
                                                       int pass_cap, int* __restrict__ counts, int* __restrict__ xy) {
  extern __shared__ uint32_t dyn[];
  __shared__ int scan[RF_T];
  __shared__ int box[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Grid g{S, S, WW, dyn, dyn + S * WW};
  load_mask<uint8_t, IsSetU8>(entire + (size_t)b * S * S, g, g.S, box);
  if (fill_outside(g, box, pass_cap)) {
    if (tid == 0) counts[b] = -1;
    return;
  }
  border_inplace(g, box);
  // test.py:305: x > 0, y > 0 and any of visible[y-1 .. y][x-1 .. x]; the visible bits take O's place
  if (visible) load_mask<uint8_t, IsSetU8>(visible + (size_t)b * S * S, g, g.O, nullptr);
  if (box[2] >= 0) {
    const int y0 = box[1], y1 = box[3];
    for (int i = tid; i < (y1 - y0 + 1) * WW; i += RF_T) {
      const int y = y0 + i / WW, w = i % WW;
      uint32_t keep = g.S[y * WW + w];
      if (!keep) continue;
      if (w == 0) keep &= ~1u;
      if (y == 0) keep = 0;
      if (visible && keep) {
        const uint32_t v = g.O[y * WW + w] | g.O[(y - 1) * WW + w];
        const uint32_t c = w > 0 ? (g.O[y * WW + w - 1] | g.O[(y - 1) * WW + w - 1]) >> 31 : 0u;
        keep &= v | (v << 1) | c;
      }
      g.S[y * WW + w] = keep;
    }
  }
  __syncthreads();
  // mapping_pixel_position_to_original_position: f64 multiply, add, truncation toward zero
  const double bx = bbox[4 * b], by = bbox[4 * b + 1];
  const double rx = (double)bbox[4 * b + 2] / (double)S, ry = (double)bbox[4 * b + 3] / (double)S;
  int* out = xy + (size_t)b * cap * 2;
  const int total = compact(g, box, scan, [&](int idx, int x, int y) {
    if (idx < cap) {
      out[2 * idx] = (int)(rx * (double)x + bx);
      out[2 * idx + 1] = (int)(ry * (double)y + by);
    }
  });
  if (tid == 0) counts[b] = total;
}

__device__ __forceinline__ int sat_coord(int v) { return v < -RF_SAT ? -RF_SAT : (v > RF_SAT ? RF_SAT : v); }

__global__ void __launch_bounds__(RF_T) k_refine_step(
    const float* __restrict__ depth, int H, int W, int WW, const int* __restrict__ counts, const int* __restrict__ xy,
    int cap, const double* __restrict__ Rin, const double* __restrict__ tin, const double* __restrict__ Kin,
    double lambda_rot, double lambda_trans, int pass_cap, double* __restrict__ R_out, double* __restrict__ t_out,
    long long* __restrict__ cost, int* __restrict__ status, int* __restrict__ border_n, int* __restrict__ border_xy,
    int bcap, int* __restrict__ match, double* __restrict__ Hb, uint32_t* __restrict__ spill) {
  extern __shared__ uint32_t dyn[];
  __shared__ uint32_t bl[RF_BL];
  __shared__ int scan[RF_T];
  __shared__ int box[4];
  __shared__ double red[RF_WAVES][RF_NACC];
  __shared__ long long cred[RF_WAVES];
  __shared__ double tot[RF_NACC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Grid g{H, W, WW, dyn, dyn + H * WW};
  const float* dimg = depth + (size_t)b * H * W;
  uint32_t* sp = spill + (size_t)b * H * W;  // border pixels RF_BL .. of this pose

  load_mask<float, IsSetDepth>(dimg, g, g.S, box);
  const bool capped = fill_outside(g, box, pass_cap);
  int nb = 0;
  if (!capped) {
    border_inplace(g, box);
    int* bo = border_xy ? border_xy + (size_t)b * bcap * 2 : nullptr;
    nb = compact(g, box, scan, [&](int idx, int x, int y) {
      const uint32_t pk = (uint32_t)x | ((uint32_t)y << 16);
      if (idx < RF_BL) bl[idx] = pk;
      else sp[idx - RF_BL] = pk;
      if (bo && idx < bcap) bo[2 * idx] = x, bo[2 * idx + 1] = y;
    });
  }
  int n = counts[b];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const int st = capped ? 2 : ((nb < RF_MIN_BORDER || n == 0) ? 1 : 0);
  if (tid == 0) {
    status[b] = st;
    if (border_n) border_n[b] = nb;
  }
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rin[9 * (size_t)b + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = tin[3 * (size_t)b + k];

  if (st != 0) {  // the pose is copied through (edge_refine.cpp:96-100 returns)
    if (tid < 9) R_out[9 * (size_t)b + tid] = Rin[9 * (size_t)b + tid];
    if (tid < 3) t_out[3 * (size_t)b + tid] = tin[3 * (size_t)b + tid];
    if (tid == 0) cost[b] = 0;
    if (Hb && tid < RF_NACC) Hb[(size_t)b * RF_NACC + tid] = 0.0;
    if (match)
      for (int i = tid; i < cap; i += RF_T) match[(size_t)b * cap + i] = -1;
    return;
  }

  const double fx = Kin[4 * b], fy = Kin[4 * b + 1], cx = Kin[4 * b + 2], cy = Kin[4 * b + 3];
  const int* pxy = xy + (size_t)b * cap * 2;
  const int nl = nb < RF_BL ? nb : RF_BL;
  double acc[RF_NACC];
#pragma unroll
  for (int k = 0; k < RF_NACC; ++k) acc[k] = 0.0;
  long long csum = 0;
  for (int i = tid; i < n; i += RF_T) {
    const int px = sat_coord(pxy[2 * i]), py = sat_coord(pxy[2 * i + 1]);
    double best = INFINITY;
    int bj = 0;
    for (int j = 0; j < nl; ++j) {
      const uint32_t u = bl[j];
      const double dx = (double)(px - (int)(u & 0xffffu)), dy = (double)(py - (int)(u >> 16));
      const double d2 = dx * dx + dy * dy;
      if (d2 < best) best = d2, bj = j;
    }
    for (int j = RF_BL; j < nb; ++j) {
      const uint32_t u = sp[j - RF_BL];
      const double dx = (double)(px - (int)(u & 0xffffu)), dy = (double)(py - (int)(u >> 16));
      const double d2 = dx * dx + dy * dy;
      if (d2 < best) best = d2, bj = j;
    }
    if (match) match[(size_t)b * cap + i] = bj;
    const uint32_t u = bj < RF_BL ? bl[bj] : sp[bj - RF_BL];
    const int xc = (int)(u & 0xffffu), yc = (int)(u >> 16);
    csum += (long long)best;
    const double d = (double)dimg[(size_t)yc * W + xc];
    const double Xc[3] = {d * ((double)xc - cx) / fx, d * ((double)yc - cy) / fy, d};
    const double jc00 = -fx / d, jc02 = fx * Xc[0] / (d * d), jc11 = -fy / d, jc12 = fy * Xc[1] / (d * d);
    double J0[6], J1[6], Xb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      J0[3 + c] = jc00 * R[c] + jc02 * R[6 + c];
      J1[3 + c] = jc11 * R[3 + c] + jc12 * R[6 + c];
      Xb[c] = (R[c] * (Xc[0] - t[0]) + R[3 + c] * (Xc[1] - t[1])) + R[6 + c] * (Xc[2] - t[2]);
    }
    // Jr = -Jt [Xb]x
    J0[0] = -(J0[4] * Xb[2] - J0[5] * Xb[1]);
    J0[1] = -(J0[5] * Xb[0] - J0[3] * Xb[2]);
    J0[2] = -(J0[3] * Xb[1] - J0[4] * Xb[0]);
    J1[0] = -(J1[4] * Xb[2] - J1[5] * Xb[1]);
    J1[1] = -(J1[5] * Xb[0] - J1[3] * Xb[2]);
    J1[2] = -(J1[3] * Xb[1] - J1[4] * Xb[0]);
    const double e0 = (double)(px - xc), e1 = (double)(py - yc);
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) acc[k++] += J0[r] * J0[c] + J1[r] * J1[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[21 + r] -= J0[r] * e0 + J1[r] * e1;
  }
  if (match)
    for (int i = n + tid; i < cap; i += RF_T) match[(size_t)b * cap + i] = -1;

  // thread -> wave (shuffle tree) -> block (fixed tree over the eight waves)
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < RF_NACC; ++k) acc[k] += __shfl_down(acc[k], off);
    csum += __shfl_down(csum, off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < RF_NACC; ++k) red[wave][k] = acc[k];
    cred[wave] = csum;
  }
  __syncthreads();
  if (tid < RF_NACC) {
    const double v = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) +
                     ((red[4][tid] + red[5][tid]) + (red[6][tid] + red[7][tid]));
    tot[tid] = v;
    if (Hb) Hb[(size_t)b * RF_NACC + tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  {
    long long c = 0;
    for (int w = 0; w < RF_WAVES; ++w) c += cred[w];
    cost[b] = c;
  }

  // (diag(lambda) + H) theta = b by Cholesky, A = L L^T
  double A[6][6], th[6];
  {
    int k = 0;
    for (int r = 0; r < 6; ++r)
      for (int c = r; c < 6; ++c) A[r][c] = A[c][r] = tot[k++];
    for (int r = 0; r < 6; ++r) A[r][r] += r < 3 ? lambda_rot : lambda_trans;
  }
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    for (int k = 0; k < j; ++k) s -= A[j][k] * A[j][k];
    const double l = sqrt(s);
    A[j][j] = l;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
      A[i][j] = v / l;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double v = tot[21 + i];
    for (int k = 0; k < i; ++k) v -= A[i][k] * th[k];
    th[i] = v / A[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = th[i];
    for (int k = i + 1; k < 6; ++k) v -= A[k][i] * th[k];
    th[i] = v / A[i][i];
  }
  // E = exp([th_r]x) = I + a K + c K^2, a = sin(a) / a, c = (1 - cos(a)) / a^2 = 2 sin^2(a / 2) / a^2
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
  double E[9], Rn[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double k2 = (Kx[3 * r] * Kx[c] + Kx[3 * r + 1] * Kx[3 + c]) + Kx[3 * r + 2] * Kx[6 + c];
      E[3 * r + c] = ((r == c ? 1.0 : 0.0) + ca * Kx[3 * r + c]) + cc * k2;
    }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (R[3 * r] * E[c] + R[3 * r + 1] * E[3 + c]) + R[3 * r + 2] * E[6 + c];
  for (int k = 0; k < 9; ++k) R_out[9 * (size_t)b + k] = Rn[k];
  for (int r = 0; r < 3; ++r)
    t_out[3 * (size_t)b + r] = t[r] + ((Rn[3 * r] * th[3] + Rn[3 * r + 1] * th[4]) + Rn[3 * r + 2] * th[5]);
}

// WW for an H x W image, or 0 when it does not fit the 64 KB masks
static int refine_words(int B, int H, int W) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 32768 || W > 32768) return 0;
  const int WW = (W + 31) / 32;
  return (long long)H * WW * 32 <= RF_MAX_BITS ? WW : 0;
}

template <typename Kern>
static hipError_t allow_lds(Kern k, size_t bytes) {
  if (bytes <= 48 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace zp

using namespace zp;

extern "C" int zp_mask_contour(int B, int S, const uint8_t* entire, const uint8_t* visible, const int* bbox, int cap,
                               int* counts, int* xy, void* stream) {
  const int WW = refine_words(B, S, S);
  ZP_CHECK_ARG(WW > 0, "zp_mask_contour: sizes out of range: B %d, S %d", B, S);
  ZP_CHECK_ARG(cap >= 1 && (long long)B * cap < (1LL << 30), "zp_mask_contour: cap %d", cap);
  ZP_CHECK_ARG(entire && bbox && counts && xy, "zp_mask_contour: NULL pointer");
  const size_t lds = (size_t)2 * S * WW * 4;
  if (allow_lds(k_mask_contour, lds) != hipSuccess) {
    set_error("zp_mask_contour: %zu bytes of LDS refused", lds);
    return ZP_ERR_HIP;
  }
  hipLaunchKernelGGL(k_mask_contour, dim3(B), dim3(RF_T), lds, (hipStream_t)stream, entire, visible, bbox, S, WW, cap,
                     4 * (S + S), counts, xy);
  ZP_LAUNCH_CHECK("zp_mask_contour");
  return ZP_OK;
}

extern "C" long long zp_edge_refine_ws_bytes(int B, int H, int W) {
  if (!refine_words(B, H, W)) return -1;
  return (long long)B * H * W * 4;
}

extern "C" int zp_edge_refine_step(int B, int H, int W, const float* depth, const int* counts, const int* xy, int cap,
                                   const double* R, const double* t, const double* K, double lambda_rot,
                                   double lambda_trans, double* R_out, double* t_out, long long* cost, int* status,
                                   int* border_n, int* border_xy, int bcap, int* match, double* Hb, void* ws,
                                   void* stream) {
  const int WW = refine_words(B, H, W);
  ZP_CHECK_ARG(WW > 0, "zp_edge_refine_step: sizes out of range: B %d, %d x %d", B, H, W);
  ZP_CHECK_ARG(cap >= 1 && cap <= (1 << 20) && (long long)B * cap < (1LL << 30), "zp_edge_refine_step: cap %d", cap);
  ZP_CHECK_ARG(!border_xy || (bcap >= 1 && (long long)B * bcap < (1LL << 30)), "zp_edge_refine_step: bcap %d", bcap);
  ZP_CHECK_ARG(lambda_rot > 0 && lambda_trans > 0 && lambda_rot < INFINITY && lambda_trans < INFINITY,
               "zp_edge_refine_step: lambda_rot %g, lambda_trans %g must be positive and finite", lambda_rot,
               lambda_trans);
  ZP_CHECK_ARG(depth && counts && xy && R && t && K && R_out && t_out && cost && status && ws,
               "zp_edge_refine_step: NULL pointer");
  ZP_CHECK_ARG(R != R_out && t != t_out, "zp_edge_refine_step: the pose cannot be updated in place");
  const size_t lds = (size_t)2 * H * WW * 4;
  if (allow_lds(k_refine_step, lds) != hipSuccess) {
    set_error("zp_edge_refine_step: %zu bytes of LDS refused", lds);
    return ZP_ERR_HIP;
  }
  hipLaunchKernelGGL(k_refine_step, dim3(B), dim3(RF_T), lds, (hipStream_t)stream, depth, H, W, WW, counts, xy, cap, R,
                     t, K, lambda_rot, lambda_trans, 4 * (H + W), R_out, t_out, cost, status, border_n, border_xy, bcap,
                     match, Hb, (uint32_t*)ws);
  ZP_LAUNCH_CHECK("zp_edge_refine_step");
  return ZP_OK;
}
