// The arithmetic of one (f, v) pair of the phase-shift transform, shared by the image kernels (dvh_slant.hip) and the
// ridge walk that evaluates pairs in place (dvh_slant_ridge.hip):
//
//   value(f, v) = (float) | sum_r D[r] w^r |,   w = exp(i theta),  theta = 2 pi f dx / v
//
// Every kernel goes through these functions, in this order: slant_steer once, then per row in ascending order
// slant_add_row with w^r and slant_next_power for w^(r+1), then slant_magnitude.  All of it is explicit float64 FMAs and
// products (nothing a contraction setting could fuse differently), so two kernels that hand the same D, f, dx and v to
// it store the same bits, whether a kernel keeps the powers in registers or runs them beside the sum.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace dvh {

// w = exp(i theta) = c + i s
__device__ __forceinline__ void slant_steer(double f, double dx, double v, double& c, double& s) {
  const double theta = 2.0 * M_PI * f * dx / v;
  sincos(theta, &s, &c);
}

// (ar, ai) += d (wr + i wi)
__device__ __forceinline__ void slant_add_row(const double2 d, double wr, double wi, double& ar, double& ai) {
  ar = fma(d.x, wr, ar);
  ar = fma(-d.y, wi, ar);
  ai = fma(d.x, wi, ai);
  ai = fma(d.y, wr, ai);
}

// (nr, ni) = (wr + i wi) (c + i s)
__device__ __forceinline__ void slant_next_power(double wr, double wi, double c, double s, double& nr, double& ni) {
  nr = fma(wr, c, -(wi * s));
  ni = fma(wr, s, wi * c);
}

__device__ __forceinline__ float slant_magnitude(double ar, double ai) { return (float)sqrt(fma(ar, ar, ai * ai)); }

// The whole pair over rows 0 .. n_row - 1, row(r) giving D[r] at the pair's frequency; the power runs with the sum.
template <class Row>
__device__ __forceinline__ float slant_pair(double f, double dx, double v, int n_row, Row row) {
  double c, s;
  slant_steer(f, dx, v, c, s);
  double ar = 0.0, ai = 0.0, wr = 1.0, wi = 0.0;
  for (int r = 0; r < n_row; ++r) {
    slant_add_row(row(r), wr, wi, ar, ai);
    double nr, ni;
    slant_next_power(wr, wi, c, s, nr, ni);
    wr = nr;
    wi = ni;
  }
  return slant_magnitude(ar, ai);
}

}  // namespace dvh
