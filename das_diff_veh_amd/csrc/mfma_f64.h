// The float64 matrix instruction and the LDS-DMA address spaces, shared by dvh_disp.hip and dvh_fv.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace dvh {

typedef double doublex4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void gbl_void;

// v_mfma_f64_16x16x4_f64 lane maps: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15],
// D[row = (l >> 4) + 4 r][col = l & 15] for r in [0, 4).
__device__ __forceinline__ doublex4 mfma_f64(double a, double b, doublex4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

}  // namespace dvh
