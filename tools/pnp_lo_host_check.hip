// Host-side run of the PnP local optimisation (zp_pnp_lo.hip's ZP_HD functions and its loop lo_run on
// the CPU, with serial sums):
//   tools/pnp_lo_host_check <in.bin> <out.bin>
// in:  int n, rounds, steps, pad; double reproj_err; double K[4]; double R[9]; double t[3];
//      float pw[n][3]; int uv[n][2]
// out: double R[9], t[3], cost, Hb[28]; int inliers, status, trace[rounds][2]
// Build with -ffp-contract=off, as the library builds that file.
// (tests/test_pnp_lo_host.py compares against tests/pnp_lo_ref.py; no GPU involved)
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../zebrapose_amd/csrc/zp_pnp_lo.hip"
namespace zp {
void set_error(const char*, ...) {}  // the library's error slot lives in zp_core.hip
}

struct HostCtx {
  int n;
  const float* pw;
  const int* uv;
  zp::LoCam K;
  std::vector<unsigned char> mask;

  void load(int i, double* p, double* u, double* v) const {
    for (int k = 0; k < 3; ++k) p[k] = (double)pw[3 * i + k];
    *u = (double)uv[2 * i];
    *v = (double)uv[2 * i + 1];
  }
  bool writer() const { return true; }
  void select(const zp::LoPose& P, double thr2, bool compare, int* count, int* changed) {
    *count = *changed = 0;
    for (int i = 0; i < n; ++i) {
      double p[3], u, v, Xc[3], e[2], r2;
      load(i, p, &u, &v);
      const bool in = zp::lo_project(P, K, p, u, v, Xc, e, &r2) && r2 <= thr2;
      *count += in;
      if (compare) *changed += (mask[i] != 0) != in;
      mask[i] = in;
    }
  }
  void normal(const zp::LoPose& P, double (&acc)[zp::LO_NACC]) {
    for (int k = 0; k < zp::LO_NACC; ++k) acc[k] = 0.0;
    for (int i = 0; i < n; ++i) {
      if (!mask[i]) continue;
      double p[3], u, v, Xc[3], e[2], r2;
      load(i, p, &u, &v);
      zp::lo_project(P, K, p, u, v, Xc, e, &r2);
      zp::lo_accum(K, Xc, e, r2, acc);
    }
  }
  double trial(const zp::LoPose& P) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      if (!mask[i]) continue;
      double p[3], u, v, Xc[3], e[2], r2;
      load(i, p, &u, &v);
      zp::lo_project(P, K, p, u, v, Xc, e, &r2);
      s += Xc[2] > 0.0 ? r2 : INFINITY;
    }
    return s;
  }
  void final(const zp::LoPose& P, double thr2, int* count, double* cost) {
    *count = 0;
    *cost = 0.0;
    for (int i = 0; i < n; ++i) {
      double p[3], u, v, Xc[3], e[2], r2;
      load(i, p, &u, &v);
      if (zp::lo_project(P, K, p, u, v, Xc, e, &r2) && r2 <= thr2) {
        *count += 1;
        *cost += r2;
      }
    }
  }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[4];
  double err, Kv[4];
  zp::LoPose in;
  if (fread(hd, 4, 4, f) != 4 || fread(&err, 8, 1, f) != 1 || fread(Kv, 8, 4, f) != 4 || fread(in.R, 8, 9, f) != 9 ||
      fread(in.t, 8, 3, f) != 3)
    return 3;
  const int n = hd[0], rounds = hd[1], steps = hd[2];
  if (n < 0 || n > (1 << 24) || rounds < 1 || rounds > 64 || steps < 1 || steps > 64) return 3;
  std::vector<float> pw(3 * (size_t)n + 1);
  std::vector<int> uv(2 * (size_t)n + 1);
  if (fread(pw.data(), 4, 3 * (size_t)n, f) != 3 * (size_t)n || fread(uv.data(), 4, 2 * (size_t)n, f) != 2 * (size_t)n)
    return 3;
  fclose(f);
  HostCtx cx{n, pw.data(), uv.data(), zp::LoCam{Kv[0], Kv[1], Kv[2], Kv[3]}, std::vector<unsigned char>((size_t)n + 1)};
  zp::LoPose out = in;
  std::vector<int> trace(2 * rounds, -1);
  double Hb[zp::LO_NACC] = {0}, cost = 0.0;
  int inliers = 0, status = 1;
  bool finite = true;
  for (int k = 0; k < 9; ++k) finite = finite && __builtin_isfinite(in.R[k]);
  for (int k = 0; k < 3; ++k) finite = finite && __builtin_isfinite(in.t[k]);
  if (n >= zp::LO_MIN_SET && finite) {
    zp::lo_run(cx, in, err * err, rounds, steps, out, &inliers, &cost, &status, trace.data(), Hb);
    if (status != 0) out = in;
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 2;
  fwrite(out.R, 8, 9, g);
  fwrite(out.t, 8, 3, g);
  fwrite(&cost, 8, 1, g);
  fwrite(Hb, 8, zp::LO_NACC, g);
  fwrite(&inliers, 4, 1, g);
  fwrite(&status, 4, 1, g);
  fwrite(trace.data(), 4, trace.size(), g);
  fclose(g);
  return 0;
}
