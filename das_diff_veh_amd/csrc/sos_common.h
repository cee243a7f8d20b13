// What the two forms of sosfiltfilt share: the cascade's coefficients and one-sample step, the filtered sequence of a
// row, the launch geometry, and the host functions through which dvh_sos.hip (the block recursion, the entry points)
// reaches the matrix-pipe form in dvh_sosm.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dvh {

constexpr int kMaxSec = 16;

// orders one wave's LDS stores and loads (a single-wave block: the fence keeps the compiler from moving them)
__device__ __forceinline__ void wave_barrier_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The cascade of n_sec transposed-direct-form-II sections (scipy's sosfilt).
template <int NS>
struct SosCoef {
  double b0[NS], b1[NS], b2[NS], a1[NS], a2[NS];
  __device__ __forceinline__ void load(const double* __restrict__ sos) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      b0[s] = sos[6 * s];
      b1[s] = sos[6 * s + 1];
      b2[s] = sos[6 * s + 2];
      a1[s] = sos[6 * s + 4];
      a2[s] = sos[6 * s + 5];
    }
  }
  // one sample through the cascade (scipy's sosfilt expressions)
  __device__ __forceinline__ double step(double (&z0)[NS], double (&z1)[NS], double v) const {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const double o = b0[s] * v + z0[s];
      z0[s] = b1[s] * v - a1[s] * o + z1[s];
      z1[s] = b2[s] * v - a2[s] * o;
      v = o;
    }
    return v;
  }
};

// The filtered sequence u of a row: the odd extension of x (forward pass) or the reversed forward output.
template <typename T, bool BWD>
struct SosInput {
  const T* row;      // forward: the row of x
  const double* y;   // backward: the row's forward output [n_ext]
  int64_t n_t, n_ext, padlen;
  double x0, xn;
  __device__ __forceinline__ double operator()(int64_t i) const {
    if (BWD) return y[n_ext - 1 - i];
    if (i < padlen) return 2.0 * x0 - (double)row[padlen - i];
    const int64_t j = i - padlen;
    if (j < n_t) return (double)row[j];
    return 2.0 * xn - (double)row[n_t - 2 - (j - n_t)];
  }
};

struct SosGeom {
  int64_t n_rows, row_stride;
  int32_t n_t, padlen, L, nb;
  int64_t n_ext;
};
// rows of n_t samples extended by padlen at either end, in blocks of L
inline SosGeom sos_geom_of(int64_t n_rows, int64_t row_stride, int32_t n_t, int32_t padlen, int32_t L) {
  SosGeom G{n_rows, row_stride, n_t, padlen, L, 0, (int64_t)n_t + 2 * padlen};
  G.nb = (int32_t)((G.n_ext + L - 1) / L);
  return G;
}

template <typename T, bool BWD>
__device__ __forceinline__ SosInput<T, BWD> sos_input(const T* x, const double* y, const SosGeom& G, int64_t r) {
  SosInput<T, BWD> u;
  u.row = x + r * G.row_stride;
  u.y = y + r * G.n_ext;
  u.n_t = G.n_t;
  u.n_ext = G.n_ext;
  u.padlen = G.padlen;
  if (!BWD) {
    u.x0 = (double)u.row[0];
    u.xn = (double)u.row[G.n_t - 1];
  } else {
    u.x0 = u.xn = 0.0;
  }
  return u;
}

// The matrix-pipe form (dvh_sosm.hip): blocks of 64 samples, 32-bit column indices (sosm_fits), a plan of
// sosm_plan_doubles operator values, and a workspace whose tail holds a plan when the caller brings none.
SosGeom sosm_geom(int64_t n_rows, int64_t row_stride, int32_t n_t, int32_t padlen);
bool sosm_fits(const SosGeom& G);
int64_t sosm_plan_doubles(int n_sec);
int64_t sosm_workspace_doubles(const SosGeom& G, int n_sec);
// Forms the plan of a filter for records of G's length (launches only: the caller checks them).
int sosm_make_plan(const double* sos, int n_sec, const double* zi, const SosGeom& G, double* plan, hipStream_t st);
// Filters the rows of x (dtype 0 / 1) in place; plan == nullptr: formed into the workspace's tail first.
int sosm_filtfilt(void* x, int32_t dtype, const SosGeom& G, const double* sos, int n_sec, const double* zi,
                  const double* plan, double* work, hipStream_t st);

}  // namespace dvh
