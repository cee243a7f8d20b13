// The secular function of rayleigh.h together with its derivative along one direction, for the sensitivity kernel of
// dvh_rayleigh_sens.hip and the host entry dvh_rayleigh_tangent_host.
//
// At a root c of D(c, omega, layers) the implicit function theorem gives dc/dp = -D_p / D_c for a layer value p and
// dc/domega = -D_omega / D_c, hence the group velocity U = c / (1 - (omega / c) dc/domega).  secular() returns D
// divided by the norm of the solution space's Pluecker vector (the re-orthonormalised block): a smooth positive factor
// g, and at a root (g D)_p / (g D)_c = D_p / D_c, so the ratios may be taken through the same recurrences.
//
// tangent() carries (value, derivative) pairs through exactly the operations of secular(): the half-space start
// vectors, LayerStep's coefficients, apply and orthonormalise (whose derivative holds the projection and both norms,
// which the pair arithmetic below produces by itself).  The value parts are the same float64 operations in the same
// order as secular()'s, so the value returned is secular()'s.  The direction is
//   0             c
//   1             omega
//   2 + 4 l + q   column q (h, alpha, beta, rho) of layer l
// and any other number gives a zero derivative.  Rows with h = 0 are skipped as in secular(), so their four
// derivatives are 0; the half-space's h is never read, so its derivative is 0.  k_sub is the caller's and the sublayer
// counts come from the values alone: they do not depend on the direction.
//
// Two derivatives are not what the pair arithmetic would give:
//   C(x), S(x) of cosh_sinhc, x = nu^2 h_s^2:  dC/dx = S / 2,  dS/dx = (C - S) / (2 x), the second by its own power
//     series on the |x| < 1e-2 branch, where the quotient cancels to nothing;
//   sqrt(fmax(., 0)) of the half-space: differentiated only where its argument is positive.
#pragma once
#include "rayleigh.h"

namespace dvh {
namespace rayleigh {

struct Dual {
  double v, d;
};

DVH_RAYLEIGH_HD Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
DVH_RAYLEIGH_HD Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
DVH_RAYLEIGH_HD Dual operator-(Dual a) { return {-a.v, -a.d}; }
DVH_RAYLEIGH_HD Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
DVH_RAYLEIGH_HD Dual operator*(double a, Dual b) { return {a * b.v, a * b.d}; }
DVH_RAYLEIGH_HD Dual operator*(Dual a, double b) { return {a.v * b, a.d * b}; }
DVH_RAYLEIGH_HD Dual operator/(Dual a, Dual b) {
  const double q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
DVH_RAYLEIGH_HD Dual operator/(double a, Dual b) {
  const double q = a / b.v;
  return {q, -q * b.d / b.v};
}
DVH_RAYLEIGH_HD Dual operator/(Dual a, double b) { return {a.v / b, a.d / b}; }
DVH_RAYLEIGH_HD Dual sqrt_dual(Dual a) {
  const double r = ::sqrt(a.v);
  return {r, 0.5 * a.d / r};
}
// sqrt(fmax(a, 0)): flat where the argument is clamped
DVH_RAYLEIGH_HD Dual sqrt_clamped(Dual a) {
  const double r = ::sqrt(fmax(a.v, 0.0));
  return {r, a.v > 0.0 ? 0.5 * a.d / r : 0.0};
}

// cosh_sinhc of a pair: the values are cosh_sinhc's own
DVH_RAYLEIGH_HD void cosh_sinhc(Dual x, Dual& C, Dual& S) {
  cosh_sinhc(x.v, C.v, S.v);
  double dS;
  if (fabs(x.v) < 1e-2) {  // sum_n n x^(n - 1) / (2 n + 1)!; the next term, 7 x^6 / 15!, is below 1e-23
    const double z = x.v;
    dS = 1.0 / 6.0 * (1.0 + z / 10.0 * (1.0 + z / 28.0 * (1.0 + z / 54.0 * (1.0 + z / 88.0 * (1.0 + z / 130.0)))));
  } else {
    dS = (C.v - S.v) / (2.0 * x.v);
  }
  C.d = 0.5 * S.v * x.d;
  S.d = dS * x.d;
}

DVH_RAYLEIGH_HD void orthonormalise(Dual (&u)[4], Dual (&v)[4]) {
  const Dual nu = 1.0 / sqrt_dual(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]);
  for (int i = 0; i < 4; ++i) u[i] = u[i] * nu;
  const Dual p = u[0] * v[0] + u[1] * v[1] + u[2] * v[2] + u[3] * v[3];
  for (int i = 0; i < 4; ++i) v[i] = v[i] - p * u[i];
  const Dual nv = 1.0 / sqrt_dual(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
  for (int i = 0; i < 4; ++i) v[i] = v[i] * nv;
}

struct LayerStepDual {
  Dual k, mu, t, mk2, irw2, Ca, Sa, na2Sa, Cb, Sb, nb2Sb;
  DVH_RAYLEIGH_HD void apply(Dual (&y)[4]) const {
    const Dual mt = mu * t;
    const Dual a = (mk2 * y[0] + y[3]) * irw2;
    const Dual d = -(k * y[3] + mt * y[0]) * irw2;
    const Dual b = -(mt * y[1] + k * y[2]) * irw2;
    const Dual e = (y[2] + mk2 * y[1]) * irw2;
    const Dual a1 = a * Ca + b * Sa, b1 = b * Ca + a * na2Sa;
    const Dual e1 = e * Cb + d * Sb, d1 = d * Cb + e * nb2Sb;
    y[0] = k * a1 + d1;
    y[1] = b1 + k * e1;
    y[2] = -mk2 * b1 - mt * e1;
    y[3] = -mt * a1 - mk2 * d1;
  }
};

// D = secular(layers, n_layer, c, omega, k_sub) and dD, its derivative along direction `dir`.
DVH_RAYLEIGH_HD void tangent(const double* layers, int n_layer, double c_, double omega_, double k_sub, int dir,
                             double& D, double& dD) {
  const Dual c = {c_, dir == 0 ? 1.0 : 0.0}, omega = {omega_, dir == 1 ? 1.0 : 0.0};
  const Dual k = omega / c, k2 = k * k, w2 = omega * omega;
  Dual u[4], v[4];
  {
    const int at = 2 + 4 * (n_layer - 1);
    const double* L = layers + 4 * (n_layer - 1);
    const Dual al = {L[1], dir == at + 1 ? 1.0 : 0.0}, be = {L[2], dir == at + 2 ? 1.0 : 0.0};
    const Dual rho = {L[3], dir == at + 3 ? 1.0 : 0.0};
    const Dual mu = rho * be * be;
    const Dual na = sqrt_clamped(k2 - w2 / (al * al)), nb = sqrt_clamped(k2 - w2 / (be * be));
    const Dual mt = mu * (2.0 * k2 - w2 / (be * be));
    u[0] = k, u[1] = na, u[2] = -2.0 * mu * k * na, u[3] = -mt;
    v[0] = nb, v[1] = k, v[2] = -mt, v[3] = -2.0 * mu * k * nb;
    orthonormalise(u, v);
  }
  for (int l = n_layer - 2; l >= 0; --l) {
    const double* L = layers + 4 * l;
    const int at = 2 + 4 * l;
    if (!(L[0] > 0.0)) continue;
    const Dual h = {L[0], dir == at ? 1.0 : 0.0}, al = {L[1], dir == at + 1 ? 1.0 : 0.0};
    const Dual be = {L[2], dir == at + 2 ? 1.0 : 0.0}, rho = {L[3], dir == at + 3 ? 1.0 : 0.0};
    const double ns = ceil(k_sub * h.v / kSubKh);
    int n_sub = ns >= (double)kMaxSub ? kMaxSub : (ns >= 1.0 ? (int)ns : 1);
#if defined(__HIP_DEVICE_COMPILE__)
    n_sub = __builtin_amdgcn_readfirstlane(n_sub);  // k_sub and the layer are the wave's: the loop count is scalar
#endif
    const Dual hs = h / (double)n_sub;
    const Dual kb2 = w2 / (be * be), na2 = k2 - w2 / (al * al), nb2 = k2 - kb2;
    LayerStepDual s;
    s.k = k;
    s.mu = rho * be * be;
    s.t = 2.0 * k2 - kb2;
    s.mk2 = 2.0 * s.mu * k;
    s.irw2 = 1.0 / (rho * w2);
    cosh_sinhc(na2 * hs * hs, s.Ca, s.Sa);
    cosh_sinhc(nb2 * hs * hs, s.Cb, s.Sb);
    s.Sa = s.Sa * hs;
    s.Sb = s.Sb * hs;
    s.na2Sa = na2 * s.Sa;
    s.nb2Sb = nb2 * s.Sb;
    for (int i = 0; i < n_sub; ++i) {
      s.apply(u);
      s.apply(v);
      orthonormalise(u, v);
    }
  }
  const Dual r = u[2] * v[3] - u[3] * v[2];
  D = r.v;
  dD = r.d;
}

}  // namespace rayleigh
}  // namespace dvh
