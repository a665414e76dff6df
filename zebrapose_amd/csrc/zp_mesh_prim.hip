// The rocPRIM calls of the mesh tools (declared in zp_mesh.h): the stable radix sorts of the two coders
// and the subdivider, and the subdivider's integer scans.  rocPRIM is header-only; this is the one file
// that includes it, so each sort and scan is instantiated once.  Integer code only.
#include "zp_mesh.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace zp {

// call(tmp, need) is the rocPRIM call: with a null tmp it only reports the temporary storage it needs,
// which must fit the workspace's share
template <typename F>
static int prim_run(void* temp, size_t temp_bytes, const char* who, const char* what, F call) {
  size_t need = 0;
  hipError_t e = call(nullptr, need);
  if (e == hipSuccess && need > temp_bytes) {
    set_error("%s: %s needs %zu bytes of temporary storage, the workspace holds %zu", who, what, need, temp_bytes);
    return ZP_ERR_HIP;
  }
  if (e == hipSuccess) e = call(temp, need);
  if (e != hipSuccess) {
    set_error("%s: %s failed: %s", who, what, hipGetErrorString(e));
    return ZP_ERR_HIP;
  }
  return ZP_OK;
}

template <typename K>
int sort_pairs(const K* kin, K* kout, const int* vin, int* vout, int n, int end_bit, void* temp, size_t temp_bytes,
               hipStream_t st, const char* who) {
  return prim_run(temp, temp_bytes, who, "the sort", [&](void* tmp, size_t& need) {
    return rocprim::radix_sort_pairs(tmp, need, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)end_bit, st);
  });
}
template int sort_pairs<u64>(const u64*, u64*, const int*, int*, int, int, void*, size_t, hipStream_t, const char*);
template int sort_pairs<unsigned>(const unsigned*, unsigned*, const int*, int*, int, int, void*, size_t, hipStream_t,
                                  const char*);

int inclusive_scan(const int* in, int* out, int n, void* temp, size_t temp_bytes, hipStream_t st, const char* who) {
  return prim_run(temp, temp_bytes, who, "the scan", [&](void* tmp, size_t& need) {
    return rocprim::inclusive_scan(tmp, need, in, out, (size_t)n, rocprim::plus<int>(), st);
  });
}

int exclusive_scan(const int* in, int* out, int n, void* temp, size_t temp_bytes, hipStream_t st, const char* who) {
  return prim_run(temp, temp_bytes, who, "the scan", [&](void* tmp, size_t& need) {
    return rocprim::exclusive_scan(tmp, need, in, out, 0, (size_t)n, rocprim::plus<int>(), st);
  });
}

}  // namespace zp
