// What the mesh tools share: zp_mesh_code (zp_meshcode.hip), zp_mesh_code_radix (zp_meshcode_radix.hip)
// and zp_mesh_subdivide (zp_subdiv.hip).  The size limits, the workspace carver and the budget for
// rocPRIM's temporary storage are written here once; so are the rocPRIM calls (zp_mesh_prim.hip, the one
// file that includes rocPRIM), the part of the workspace both coders use, the device helpers their
// kernels share, and the steps of their drivers that are the same (defined in zp_meshcode.hip).
#pragma once
#include "zp_common.h"

namespace zp {

typedef unsigned long long u64;

constexpr int M_IDX_BITS = 21;  // nv <= 2^21: a vertex index fits 21 bits of a sort key
constexpr u64 M_IDX_MASK = (1ull << M_IDX_BITS) - 1;
constexpr int M_MAX_NF = 1 << 24;

inline bool mesh_range_ok(int nv, int nf) { return nv <= (1 << M_IDX_BITS) && nf >= 1 && nf <= M_MAX_NF; }

// the share of a workspace set aside for rocPRIM's temporary storage over n elements
inline size_t prim_temp_bytes(size_t n) { return ((size_t)16 << 20) + 32 * n; }

// Hands out consecutive regions of a workspace, each rounded up to 256 bytes, so total() is a sum that
// does not depend on the order of the takes.  A null base measures only: every take returns null.
class Carver {
 public:
  explicit Carver(void* base) : base_((char*)base) {}
  template <class T> T* take(size_t count) {
    char* r = base_ ? base_ + off_ : nullptr;
    off_ += (count * sizeof(T) + 255) & ~(size_t)255;
    return (T*)r;
  }
  size_t total() const { return off_; }

 private:
  char* base_;
  size_t off_ = 0;
};

// ---- rocPRIM (zp_mesh_prim.hip) --------------------------------------------------------------------
// Each call asks rocPRIM for its temporary need, refuses if that exceeds temp_bytes, then runs on `st`;
// `who` names the entry point in the error text.  Returns ZP_OK or ZP_ERR_HIP.

// stable sort of n (key, value) pairs on key bits [0, end_bit); K is u64 or unsigned
template <typename K>
int sort_pairs(const K* kin, K* kout, const int* vin, int* vout, int n, int end_bit, void* temp, size_t temp_bytes,
               hipStream_t st, const char* who);
// out[i] = in[0] + .. + in[i], and the same without in[i]
int inclusive_scan(const int* in, int* out, int n, void* temp, size_t temp_bytes, hipStream_t st, const char* who);
int exclusive_scan(const int* in, int* out, int n, void* temp, size_t temp_bytes, hipStream_t st, const char* who);

// ---- the two coders ----------------------------------------------------------------------------

struct MeshWs {     // what both splits use; G = the last level's group count
  int4* q;          // [nv] grid coordinates (w unused)
  int* gid;         // [nv] group of vertex v at the next level
  unsigned* gs;     // [nv] group of sorted position p
  int* order;       // [nv] vertex at sorted position p
  int* iota;        // [max(nv, nf)] 0, 1, 2, ...
  u64* key;         // [nv] balance / peel keys (the d-ary seeding's running minimum before the peel)
  u64* key2;        // [nv] their sorted copy
  int* val2;        // [nv] the values sorted with them
  int* gstart;      // [G + 1]
  u64* comp;        // [G] compactness of the running attempt
  u64* bcomp;       // [G] of the best
  int* done;        // [G]
  unsigned* fkey2;  // [nf] face ids sorted
  int* fval2;       // [nf] faces in class order
  void* temp;       // rocPRIM's temporary storage
  size_t temp_bytes;
};

inline MeshWs carve_mesh(Carver& c, int nv, int nf, size_t G) {
  const size_t nmax = (size_t)(nv > nf ? nv : nf);
  MeshWs w;
  w.q = c.take<int4>(nv);
  w.gid = c.take<int>(nv);
  w.gs = c.take<unsigned>(nv);
  w.order = c.take<int>(nv);
  w.iota = c.take<int>(nmax);
  w.key = c.take<u64>(nv);
  w.key2 = c.take<u64>(nv);
  w.val2 = c.take<int>(nv);
  w.gstart = c.take<int>(G + 1);
  w.comp = c.take<u64>(G);
  w.bcomp = c.take<u64>(G);
  w.done = c.take<int>(G);
  w.fkey2 = c.take<unsigned>(nf);
  w.fval2 = c.take<int>(nf);
  w.temp_bytes = prim_temp_bytes(nmax);
  w.temp = c.take<char>(w.temp_bytes);
  return w;
}

// The driver steps both entry points enqueue (zp_meshcode.hip, beside their kernels); `who` is the
// entry point's name.  Each returns ZP_OK or the error it has set.
// the range of nv / nf and the arguments both entry points take; `pointers`: none of them is NULL
int mesh_check_args(const char* who, int nv, int nf, int attempts, int iterations, int grid_log2, long long eps2_q,
                    bool pointers);
// grid coordinates; one group of all vertices; iota; vertex_ids = 0
int mesh_prologue(const char* who, const MeshWs& w, const float* verts, int nv, int nf, int grid_log2,
                  int* vertex_ids, hipStream_t st);
// after a level: positions sorted by gid (end_bit key bits), then the bounds of the next level's G groups
int mesh_regroup(const char* who, const MeshWs& w, int nv, int end_bit, int G, hipStream_t st);
// face ids, the faces sorted by id (code_bits key bits), the LUT of 2^code_bits classes
int mesh_epilogue(const char* who, const MeshWs& w, const float* verts, int nv, const int* faces, int nf,
                  int code_bits, const int* vertex_ids, int* face_ids, double* lut, hipStream_t st);

// ---- device helpers ----------------------------------------------------------------------------

__device__ __forceinline__ int clamp_index(int i, int nv) { return i < 0 ? 0 : (i >= nv ? nv - 1 : i); }

__device__ __forceinline__ long long floor_div(long long a, long long b) {  // b > 0
  long long r = a / b;
  if (a % b != 0 && a < 0) --r;
  return r;
}

struct MPos {
  int g, v;
  int4 pt;
};

// sorted position p -> group, vertex, grid point; false when the group word is out of range
__device__ __forceinline__ bool load_pos(int p, int nv, int G, const unsigned* __restrict__ gs,
                                         const int* __restrict__ order, const int4* __restrict__ q, MPos& r) {
  const unsigned g = gs[p];
  if (g >= (unsigned)G) return false;
  int v = order[p];
  if ((unsigned)v >= (unsigned)nv) v = 0;
  r.g = (int)g;
  r.v = v;
  r.pt = q[v];
  return true;
}

// seed 0 of group g: the grid point of its vertex at rank (draw * n) >> 32
__device__ __forceinline__ int4 seed0(int g, int nv, const int* __restrict__ gstart, const int* __restrict__ order,
                                      const int4* __restrict__ q, const uint32_t* __restrict__ draws) {
  const int s = gstart[g];
  const long long n = (long long)gstart[g + 1] - s;
  long long pos = s + (long long)(((u64)draws[g] * (u64)(n > 0 ? n : 0)) >> 32);
  pos = pos < 0 ? 0 : (pos >= nv ? nv - 1 : pos);
  int v = order[pos];
  if ((unsigned)v >= (unsigned)nv) v = 0;
  return q[v];
}

// the grid point of the vertex a farthest-point key (d^2 << 21 | 2^21 - 1 - index) names
__device__ __forceinline__ int4 far_point(u64 key, int nv, const int4* __restrict__ q) {
  long long v = (long long)(M_IDX_MASK - (key & M_IDX_MASK));
  if (v >= nv) v = nv - 1;
  return q[v];
}

}  // namespace zp
