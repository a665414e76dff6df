// Batched triangle rasteriser: GT code images, depth and masks from a mesh on the device.
// Reference: Binary_Code_GT_Generator/Render_GT_Color_Mesh_to_GT_Img -- rendering_GT_once /
// render_3D_GT_Model (render_related_source/opengl_render.cpp:164-206: clear to black, GL_LESS
// depth test, no culling, no antialiasing, one glDrawElements), the projection matrix of
// camera.hpp:29-59 (u = fx X / Z + cx with GL's pixel centres at half-integers) and the
// pass-through shaders shader_groundtruth.vs / .fs, as driven by
// generate_training_labels_for_BOP_v2.py:77-85.  An Instinct card has no graphics pipeline, so the
// draw is restated as exact integer geometry (tests/render_ref.py is the executable definition):
//
//   vertex    Xc = ((r0 x + r1 y) + r2 z) + tx (f64; likewise Yc, Zc), u = (fx Xc) / Zc + cx,
//             xi = rint(256 u) (half to even), saturated to +-2^28, so edge functions fit int64
//   triangle  dropped when a vertex has Zc < z_near (or a NaN projection), when its area in snapped
//             units is 0, or when an index lies outside the mesh; both windings draw
//   coverage  pixel (x, y) sampled at (256 x + 128, 256 y + 128); exact int64 edge functions; a sample
//             on an edge belongs to the triangle whose edge is a top or left one (image rows down)
//   depth     q = (E12 (1/Z0) + E20 (1/Z1)) + E01 (1/Z2), invz = f32(q / A): linear in 1/Z like GL's z
//   visible   the largest invz, then the lowest face index (GL_LESS under draw order): one u64 key per
//             pixel, invz_bits << 32 | (0xFFFFFFFF - face), merged by an unsigned atomic max, so the
//             image does not depend on the order triangles arrive in
//   colour    the winning face's face_bgr
//
// Deviations from GL: no near / far clipping (a triangle with a vertex nearer than z_near is
// dropped whole; GT poses lie in front of the camera), vertices snapped to 1/256 px whatever the
// image size, flat per-face colour (the reference interpolates per-vertex colours; its GT meshes
// give every face one colour), and GL's own choice for samples exactly on an edge is not pinned.
//
// Five passes on the caller's stream: clear the key plane, k_render_verts (one thread per vertex),
// k_render_tris (one thread per face: setup, boxes of <= 16 samples finished in the thread, larger
// ones appended to a list), k_render_big (one wave per list entry, 8 x 8 sample blocks), and
// k_render_resolve (one thread per pixel).  Every pixel loop runs over a box already clipped to
// the image.
#include "zp_render_core.h"

// the f64 steps are single IEEE operations in the order written (render_ref.py mirrors them): the
// Makefile compiles this file with -ffp-contract=off; the pragma covers other build routes
#pragma clang fp contract(off)

namespace zp {

constexpr double R_SAT = 268435456.0;  // 2^28
constexpr int R_SMALL = 16;            // boxes of at most this many samples are finished in k_render_tris

__global__ void __launch_bounds__(256) k_render_verts(const float* __restrict__ verts, int nv, int B,
                                                      const double* __restrict__ R, const double* __restrict__ t,
                                                      const double* __restrict__ K, double z_near,
                                                      RVert* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * nv) return;
  const int b = i / nv, v = i - b * nv;
  const double* r = R + 9 * b;
  const double x = verts[3 * (size_t)v], y = verts[3 * (size_t)v + 1], z = verts[3 * (size_t)v + 2];
  const double Xc = ((r[0] * x + r[1] * y) + r[2] * z) + t[3 * b];
  const double Yc = ((r[3] * x + r[4] * y) + r[5] * z) + t[3 * b + 1];
  const double Zc = ((r[6] * x + r[7] * y) + r[8] * z) + t[3 * b + 2];
  RVert o = {0, 0, 0.0};
  if (Zc >= z_near) {
    const double u = (K[4 * b] * Xc) / Zc + K[4 * b + 2];
    const double w = (K[4 * b + 1] * Yc) / Zc + K[4 * b + 3];
    if (u == u && w == w) {
      o.x = (int)fmin(fmax(rint(u * 256.0), -R_SAT), R_SAT);
      o.y = (int)fmin(fmax(rint(w * 256.0), -R_SAT), R_SAT);
      o.w = 1.0 / Zc;
    }
  }
  out[i] = o;
}

// coverage test and key update of pixel (x, y), which lies inside the image
__device__ __forceinline__ void sample(const RTri& T, u64* __restrict__ keys, int W, int x, int y) {
  const long long sx = 256LL * x + 128, sy = 256LL * y + 128;
  const long long E12 = edge_at(T, 0, sx, sy), E20 = edge_at(T, 1, sx, sy), E01 = edge_at(T, 2, sx, sy);
  if (T.s * E12 < T.thr[0] || T.s * E20 < T.thr[1] || T.s * E01 < T.thr[2]) return;
  const double q = ((double)E12 * T.w0 + (double)E20 * T.w1) + (double)E01 * T.w2;
  const float invz = (float)(q / (double)T.A);
  const u64 key = ((u64)__float_as_uint(invz) << 32) | (u64)(0xFFFFFFFFu - T.face);
  u64* p = keys + (size_t)y * W + x;
  // keys only grow: a stale read costs at most one redundant atomic
  if (*(volatile u64*)p < key) atomicMax(p, key);
}

__global__ void __launch_bounds__(256) k_render_tris(const RVert* __restrict__ verts, int nv,
                                                     const int* __restrict__ faces, int nf, int B, int H, int W,
                                                     u64* __restrict__ keys, unsigned* __restrict__ counter,
                                                     unsigned* __restrict__ list) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool big = false;
  if (i < B * nf) {
    const int b = i / nf, f = i - b * nf;
    RTri T;
    if (tri_setup(verts + (size_t)b * nv, faces, nv, f, H, W, T)) {
      const int bw = T.bx1 - T.bx0 + 1, bh = T.by1 - T.by0 + 1;
      if ((long long)bw * bh <= R_SMALL) {
        u64* kb = keys + (size_t)b * H * W;
        for (int y = T.by0; y <= T.by1; ++y)
          for (int x = T.bx0; x <= T.bx1; ++x) sample(T, kb, W, x, y);
      } else {
        big = true;
      }
    }
  }
  // one counter bump per wave: every lane arrives here
  const u64 m = __ballot(big);
  if (m) {
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(m));
    base = __shfl(base, leader);
    if (big) list[base + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = (unsigned)i;
  }
}

__global__ void __launch_bounds__(256) k_render_big(const RVert* __restrict__ verts, int nv,
                                                    const int* __restrict__ faces, int nf, int B, int H, int W,
                                                    u64* __restrict__ keys, const unsigned* __restrict__ counter,
                                                    const unsigned* __restrict__ list) {
  const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
  const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const unsigned n = min(*counter, (unsigned)(B * nf));
  for (unsigned e = wave; e < n; e += nwaves) {
    const unsigned id = list[e];
    if (id >= (unsigned)(B * nf)) continue;
    const int b = id / nf, f = id - b * nf;
    RTri T;
    if (!tri_setup(verts + (size_t)b * nv, faces, nv, f, H, W, T)) continue;
    u64* kb = keys + (size_t)b * H * W;
    for (int y0 = T.by0; y0 <= T.by1; y0 += 8) {
      const int y1 = min(y0 + 7, T.by1);
      for (int x0 = T.bx0; x0 <= T.bx1; x0 += 8) {
        const int x1 = min(x0 + 7, T.bx1);
        // trivial reject: the block's largest s * E over its samples is below the edge's threshold
        bool out = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const long long cx = 256LL * (T.s * T.ey[k] < 0 ? x1 : x0) + 128;
          const long long cy = 256LL * (T.s * T.ex[k] > 0 ? y1 : y0) + 128;
          out |= T.s * edge_at(T, k, cx, cy) < T.thr[k];
        }
        if (out) continue;
        const int x = x0 + lx, y = y0 + ly;
        if (x <= x1 && y <= y1) sample(T, kb, W, x, y);
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_render_resolve(const u64* __restrict__ keys, long long n,
                                                        const uint8_t* __restrict__ face_bgr, int nf,
                                                        uint8_t* __restrict__ color, float* __restrict__ depth,
                                                        uint8_t* __restrict__ mask, int* __restrict__ face_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 key = keys[i];
  const bool fg = key != 0;
  const unsigned f = 0xFFFFFFFFu - (unsigned)key;
  if (color) {
    uint8_t c0 = 0, c1 = 0, c2 = 0;
    if (fg && f < (unsigned)nf) {
      c0 = face_bgr[3 * (size_t)f];
      c1 = face_bgr[3 * (size_t)f + 1];
      c2 = face_bgr[3 * (size_t)f + 2];
    }
    color[3 * i] = c0;
    color[3 * i + 1] = c1;
    color[3 * i + 2] = c2;
  }
  if (depth) depth[i] = fg ? (float)(1.0 / (double)__uint_as_float((unsigned)(key >> 32))) : 0.f;
  if (mask) mask[i] = fg ? 255 : 0;
  if (face_out) face_out[i] = fg ? (int)f : -1;
}

int render_visibility(int B, const float* verts, int nv, const int* faces, int nf, const double* R, const double* t,
                      const double* K, int H, int W, double z_near, const RWs& w, hipStream_t st) {
  const long long npix = (long long)B * H * W;
  hipError_t e = hipMemsetAsync(w.keys, 0, (size_t)npix * 8 + 4, st);
  if (e != hipSuccess) {
    set_error("zp_render: clear failed: %s", hipGetErrorString(e));
    return ZP_ERR_HIP;
  }
  hipLaunchKernelGGL(k_render_verts, dim3(ceil_div((long)B * nv, 256)), dim3(256), 0, st, verts, nv, B, R, t, K, z_near,
                     w.verts);
  ZP_LAUNCH_CHECK("zp_render verts");
  const int tri_blocks = ceil_div((long)B * nf, 256);
  hipLaunchKernelGGL(k_render_tris, dim3(tri_blocks), dim3(256), 0, st, (const RVert*)w.verts, nv, faces, nf, B, H, W,
                     w.keys, w.counter, w.list);
  ZP_LAUNCH_CHECK("zp_render tris");
  const int big_blocks = min(ceil_div((long)B * nf, 4), num_cus() * 8);
  hipLaunchKernelGGL(k_render_big, dim3(big_blocks), dim3(256), 0, st, (const RVert*)w.verts, nv, faces, nf, B, H, W,
                     w.keys, (const unsigned*)w.counter, (const unsigned*)w.list);
  ZP_LAUNCH_CHECK("zp_render big");
  return ZP_OK;
}

int render_resolve(const RWs& w, long long npix, const uint8_t* face_bgr, int nf, uint8_t* color, float* depth,
                   uint8_t* mask, int* face_out, hipStream_t st) {
  hipLaunchKernelGGL(k_render_resolve, dim3(ceil_div(npix, 256)), dim3(256), 0, st, (const u64*)w.keys, npix, face_bgr,
                     nf, color, depth, mask, face_out);
  ZP_LAUNCH_CHECK("zp_render resolve");
  return ZP_OK;
}

}  // namespace zp

using namespace zp;

extern "C" long long zp_render_ws_bytes(int B, int nv, int nf, int H, int W) {
  if (!render_sizes_ok(B, nv, nf, H, W)) return -1;
  size_t total = 0;
  carve(nullptr, B, nv, nf, H, W, &total);
  return (long long)total;
}

extern "C" int zp_render(int B, const float* verts, int nv, const int* faces, int nf, const uint8_t* face_bgr,
                         const double* R, const double* t, const double* K, int H, int W, double z_near,
                         uint8_t* color, float* depth, uint8_t* mask, int* face_out, void* ws, void* stream) {
  ZP_CHECK_ARG(B >= 1 && nv >= 1 && nf >= 1 && H >= 1 && W >= 1, "zp_render: B %d nv %d nf %d H %d W %d must be >= 1",
               B, nv, nf, H, W);
  ZP_CHECK_ARG(render_sizes_ok(B, nv, nf, H, W), "zp_render: sizes B %d nv %d nf %d H %d W %d out of range", B, nv,
               nf, H, W);
  ZP_CHECK_ARG(z_near > 0, "zp_render: z_near must be > 0");
  ZP_CHECK_ARG(verts && faces && R && t && K && ws, "zp_render: NULL pointer (verts, faces, R, t, K, ws are required)");
  ZP_CHECK_ARG(face_bgr || !color, "zp_render: color needs face_bgr");
  if (!color && !depth && !mask && !face_out) return ZP_OK;
  hipStream_t st = (hipStream_t)stream;
  const RWs w = carve(ws, B, nv, nf, H, W, nullptr);
  const int rc = render_visibility(B, verts, nv, faces, nf, R, t, K, H, W, z_near, w, st);
  if (rc != ZP_OK) return rc;
  return render_resolve(w, (long long)B * H * W, face_bgr, nf, color, depth, mask, face_out, st);
}
