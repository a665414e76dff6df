// The library's global state: the per-thread error slot (set_error, zp_last_error), the ABI version
// and the per-device range-flag registry that every split-fp32 store site reads.
#include <stdarg.h>
#include <stdio.h>
#include "zp_common.h"

namespace zp {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

}  // namespace zp
using namespace zp;

// zp_split_range_flag registry: one word per device, set by the caller
static unsigned* g_range_flag[64];

unsigned* zp::range_flag() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return nullptr;
  return g_range_flag[d];
}

extern "C" int zp_split_range_flag(unsigned int* flag) {
  int d = 0;
  ZP_CHECK_ARG(hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64, "zp_split_range_flag: no current device");
  g_range_flag[d] = flag;
  return ZP_OK;
}

extern "C" int zp_abi_version(void) { return ZP_ABI_VERSION; }
extern "C" const char* zp_last_error(void) { return g_err; }
