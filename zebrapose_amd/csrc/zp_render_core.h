// Device and host pieces of the rasteriser (zp_render.hip) that the shaded renderer (zp_shade.hip)
// shares: the snapped vertex, the workspace layout, triangle setup with its exact int64 edge
// functions, and the two host steps of a render (visibility passes, resolve).  The kernels
// themselves live in zp_render.hip.
#pragma once
#include "zp_common.h"

namespace zp {

typedef unsigned long long u64;

struct RVert {  // snapped vertex of one render; w = 1 / Zc, or 0 = discard every triangle using it
  int x, y;
  double w;
};

struct RWs {
  u64* keys;           // [B][H][W]
  unsigned* counter;   // entries in list
  RVert* verts;        // [B][nv]
  unsigned* list;      // [B * nf]: b * nf + face
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// keys, then the counter (one memset clears both), then vertices, then the list
inline RWs carve(void* ws, int B, int nv, int nf, int H, int W, size_t* total) {
  char* p = (char*)ws;
  RWs r;
  size_t o = 0;
  r.keys = (u64*)(p + o);
  o += (size_t)B * H * W * 8;
  r.counter = (unsigned*)(p + o);
  o = align256(o + 4);
  r.verts = (RVert*)(p + o);
  o = align256(o + (size_t)B * nv * sizeof(RVert));
  r.list = (unsigned*)(p + o);
  o = align256(o + (size_t)B * nf * 4);
  if (total) *total = o;
  return r;
}

// One triangle of one render after setup.  Edge k (12, 20, 01) evaluates at a sample (sx, sy) as
// E = ex[k] * (sy - oy[k]) - ey[k] * (sx - ox[k]); s = sign(A); a sample is inside when every
// s * E >= thr[k] (0 on a top / left edge, 1 elsewhere).
struct RTri {
  long long ex[3], ey[3], ox[3], oy[3], thr[3];
  long long A, s;
  double w0, w1, w2;
  int bx0, bx1, by0, by1;  // clipped pixel box, inclusive
  unsigned face;
};

__device__ __forceinline__ bool tri_setup(const RVert* __restrict__ vb, const int* __restrict__ faces, int nv, int f,
                                          int H, int W, RTri& T) {
  const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) return false;
  const RVert a = vb[i0], b = vb[i1], c = vb[i2];
  if (a.w == 0.0 || b.w == 0.0 || c.w == 0.0) return false;
  const long long x0 = a.x, y0 = a.y, x1 = b.x, y1 = b.y, x2 = c.x, y2 = c.y;
  T.A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
  if (T.A == 0) return false;
  T.s = T.A > 0 ? 1 : -1;
  T.bx0 = (int)max((min(min(x0, x1), x2) + 127) >> 8, 0LL);
  T.bx1 = (int)min((max(max(x0, x1), x2) - 128) >> 8, (long long)W - 1);
  T.by0 = (int)max((min(min(y0, y1), y2) + 127) >> 8, 0LL);
  T.by1 = (int)min((max(max(y0, y1), y2) - 128) >> 8, (long long)H - 1);
  if (T.bx0 > T.bx1 || T.by0 > T.by1) return false;
  const long long px[3] = {x1, x2, x0}, py[3] = {y1, y2, y0}, qx[3] = {x2, x0, x1}, qy[3] = {y2, y0, y1};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long dx = qx[k] - px[k], dy = qy[k] - py[k];
    T.ex[k] = dx;
    T.ey[k] = dy;
    T.ox[k] = px[k];
    T.oy[k] = py[k];
    const bool tl = T.s * dy < 0 || (dy == 0 && T.s * dx > 0);
    T.thr[k] = tl ? 0 : 1;
  }
  T.w0 = a.w;
  T.w1 = b.w;
  T.w2 = c.w;
  T.face = (unsigned)f;
  return true;
}

__device__ __forceinline__ long long edge_at(const RTri& T, int k, long long sx, long long sy) {
  return T.ex[k] * (sy - T.oy[k]) - T.ey[k] * (sx - T.ox[k]);
}

inline bool render_sizes_ok(int B, int nv, int nf, int H, int W) {
  const long long lim = 2147483647LL - 1024;  // flat thread indices (grid * 256) stay in int
  return B >= 1 && nv >= 1 && nf >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (long long)B * nv <= lim &&
         (long long)B * nf <= lim && (long long)B * H * W <= lim;
}

// the passes up to the key plane (clear, vertices, triangles, listed triangles) on `st`; w = carve(ws, ...)
int render_visibility(int B, const float* verts, int nv, const int* faces, int nf, const double* R, const double* t,
                      const double* K, int H, int W, double z_near, const RWs& w, hipStream_t st);
// the key plane -> colour, depth, mask, face index (each may be NULL)
int render_resolve(const RWs& w, long long npix, const uint8_t* face_bgr, int nf, uint8_t* color, float* depth,
                   uint8_t* mask, int* face_out, hipStream_t st);

}  // namespace zp
