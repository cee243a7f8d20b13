// The arithmetic of the phase-weighted stack ("Phase-weighted stack"), written once for the device kernels
// and the host entries of dvh_pws.hip.  Every output element is one sequential chain of operations in an order fixed by
// the shapes and the selection; the products that feed a sum are written as fma on both sides, so the device compile's
// contraction has nothing left to change.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DVH_PWS_HD __host__ __device__ inline
#else
#define DVH_PWS_HD inline
#endif

namespace dvh {
namespace pws {

constexpr int kMaxLen = 1024;  // DVH_PWS_MAX_LEN: a row and its tap table as float64 in LDS, 16 KB

// Tap n of the circular convolution that gives imag(scipy.signal.hilbert(x)) for a row of N samples:
//   N even: (2/N) cot(pi n / N) for odd n, 0 for even n
//   N odd:  (cot(pi n / N) - cos(pi n) / sin(pi n / N)) / N = cot(pi n / 2N) / N for odd n, -tan(pi n / 2N) / N for
//           even n (the half-angle forms have no cancellation)
// The taps are odd about N/2, k[N - n] = -k[n]: the tangent is taken at the smaller of n and N - n and, for even N,
// at the complement above pi/4, so its argument never passes pi/4 and carries the relative error of one product and
// one quotient.
DVH_PWS_HD double hilbert_tap(int n, int N) {
  if (n == 0) return 0.0;
  const int m = n <= N - n ? n : N - n;
  const double sign = m == n ? 1.0 : -1.0;
  const double pi = 3.141592653589793;
  if (N % 2 == 0) {
    if (m % 2 == 0) return 0.0;
    // cot(x) above pi/4 as tan(pi/2 - x), the difference taken in integers: the tap at N/2 is exactly 0
    const double c = 4 * m <= N ? 1.0 / tan(pi * (double)m / (double)N) : tan(pi * (double)(N - 2 * m) / (double)(2 * N));
    return sign * (2.0 / (double)N) * c;
  }
  const double t = tan(pi * (double)m / (double)(2 * N));
  return sign * (m % 2 ? 1.0 / t : -t) / (double)N;
}

DVH_PWS_HD bool is_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN

// H[t] = sum_n k[n] x[(t - n) mod N], taps in ascending order from +0, rounded once.  all_finite: whether every sample
// of the row is finite.  The transform carries one non-finite sample into every lag as NaN (inf - inf in its sums);
// the convolution alone would leave +-inf where the sample meets a non-zero tap, so such a row is NaN by decision.
DVH_PWS_HD float hilbert_at(const double* x, const double* k, int N, int t, bool all_finite) {
  if (!all_finite) return NAN;
  double acc = 0.0;
  for (int n = 0; n < N; ++n) {
    const int i = t - n;
    acc = fma(k[n], x[i < 0 ? i + N : i], acc);
  }
  return (float)acc;
}

// The three sums of one output element over the drawn passes, in draw order.
struct Sums {
  float g, re, im;
};
DVH_PWS_HD Sums start() { return Sums{-0.f, 0.f, 0.f}; }  // g as select_mean_one starts it: -0 + x == x for every x

// One pass: g joins the linear sum by the plain add of select_mean_one, the phasor (g + i h) / |g + i h| -- 0 where both
// vanish -- the two others.  The sum of squares is float32: it overflows above |a| = 1.8e19 (inv = 0: the sample drops
// out of c) and is subnormal below 1.1e-19, 0 below 2.6e-23 (the sample counts as dead); include/dvh.h states the range.
DVH_PWS_HD void add(Sums& s, float g, float h) {
  const float n2 = fmaf(h, h, g * g);
  const float inv = n2 > 0.f ? 1.f / sqrtf(n2) : 0.f;  // NaN fails the comparison: g * 0 and h * 0 keep it
  s.g += g;
  s.re = fmaf(g, inv, s.re);
  s.im = fmaf(h, inv, s.im);
}

// lin * c^power with lin = sum g / m and c = |sum of phasors| / m.  power 0 returns lin itself.
DVH_PWS_HD float finish(const Sums& s, int m, float power) {
  const float lin = s.g / (float)m;  // divide (not multiply by 1/m): sum / len as the reference evaluates it
  if (power == 0.f) return lin;
  const float c = sqrtf(fmaf(s.im, s.im, s.re * s.re)) / (float)m;
  if (power == 1.f) return lin * c;
  if (power == 2.f) return lin * (c * c);
  return lin * powf(c, power);
}

// power is 0 or at least 1 (NaN fails both)
DVH_PWS_HD bool power_ok(float power) { return power == 0.f || (power >= 1.f && power <= 3.4028234663852886e38f); }

}  // namespace pws
}  // namespace dvh
