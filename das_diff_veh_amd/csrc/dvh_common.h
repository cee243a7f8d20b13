// Shared helpers of the libdvh C-ABI: export macro, the thread-local last-error string and the boundary code every
// entry point uses (launch status, dynamic LDS, the dtype and section-count dispatch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#define DVH_API extern "C" __attribute__((visibility("default")))

namespace dvh {
// Records `msg` as the calling thread's last error and returns `code` (negative).
int set_error(int code, const char* msg);
// Compute units of the current device (cached per device ordinal on first use; 256 if the query fails).
int cu_count();

// 0, or -3 with the HIP error string as the last error.
inline int hip_status(hipError_t e) { return e == hipSuccess ? 0 : set_error(-3, hipGetErrorString(e)); }
// The status of the launches since the last check.
inline int last_launch() { return hip_status(hipGetLastError()); }
// Allows `fn` to be launched with `bytes` of dynamic LDS.
inline int set_dynamic_lds(const void* fn, size_t bytes) {
  return hip_status(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// f(T()) with T = float (dtype 0) or double (dtype 1): `[&](auto t) { using T = decltype(t); ... return rc; }`.
template <typename F>
int with_float_type(int32_t dtype, F&& f) {
  if (dtype == 0) return f(float());
  if (dtype == 1) return f(double());
  return set_error(-2, "dtype must be 0 (float32) or 1 (float64)");
}

// f(std::integral_constant<int, n_sec>()) for 1 <= n_sec <= 16:
// `[&](auto ns) { constexpr int NS = decltype(ns)::value; ... return rc; }`.
template <int N = 1, typename F>
int with_section_count(int n_sec, F&& f) {
  if constexpr (N > 16)
    return set_error(-4, "unsupported number of second-order sections");
  else
    return n_sec == N ? f(std::integral_constant<int, N>()) : with_section_count<N + 1>(n_sec, f);
}
}  // namespace dvh
