// The Rayleigh-wave secular function of a stack of homogeneous isotropic elastic layers over a half-space, in real
// float64 arithmetic, for the device kernels of dvh_rayleigh.hip and for the host entry dvh_rayleigh_secular_host.
//
// A layer is (h, alpha, beta, rho) in km, km/s, km/s, g/cm^3; the last one is the half-space (its h is ignored).  With
// the motion-stress vector (r1, r2, r3, r4) of Aki & Richards eq. 7.28 (horizontal and vertical displacement, shear
// and normal traction; z downward) a P-SV solution of horizontal wavenumber k = omega / c is
//   r = (k a + d,  b + k e,  -2 mu k b - mu t e,  -mu t a - 2 mu k d),      t = 2 k^2 - omega^2 / beta^2,
// where (a, b) is the P part and (e, d) the SV part, and over a distance h upward
//   a' = a C_a + b S_a,   b' = b C_a + a nu_a^2 S_a,      C = cosh(nu h), S = sinh(nu h) / nu, nu^2 S = nu sinh(nu h),
//   e' = e C_b + d S_b,   d' = d C_b + e nu_b^2 S_b,      nu_a^2 = k^2 - omega^2 / alpha^2, nu_b^2 likewise with beta.
// C and S are functions of nu^2 h^2 alone: cosh and sinh where it is positive, cos and sin where it is negative, and
// their common power series near zero (a scan point may land exactly on a layer's alpha or beta).
//
// The two solutions that decay in the half-space start as the potentials' vectors
//   P: (k, nu_a, -2 mu k nu_a, -mu t)      SV: (nu_b, k, -mu t, -2 mu k nu_b)
// which fixes the sign of the determinant: it is continuous in c on [c_min, beta_halfspace).  They are carried up as
// a 4 x 2 block.  A layer is cut into n_sub = ceil(k_sub h / kSubKh) equal sublayers and after each one the two columns
// are re-orthonormalised by modified Gram-Schmidt (positive norms: column operations of positive determinant, so the
// sign of every 2 x 2 minor is kept, and |minor| <= 1).  The secular function is the minor of the two traction rows
// at the free surface, r3(1) r4(2) - r4(1) r3(2); its zeros in c are the modal phase velocities.  k_sub is the
// caller's: the device passes the largest k of a wave's 64 points so that no lane's sublayer loop diverges.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DVH_RAYLEIGH_HD __host__ __device__ inline
#else
#define DVH_RAYLEIGH_HD inline
#endif

namespace dvh {
namespace rayleigh {

constexpr int kMaxLayers = 32;
constexpr int kMaxModes = 16;
constexpr double kSubKh = 8.0;  // the longest k h carried between two orthonormalisations
constexpr int kMaxSub = 256;    // a sublayer count beyond this (k h > 2 048) is clamped: the loop is bounded on any input

// sin(y) and cos(y) for the arguments a sublayer has, 0 <= y <= kSubKh (|nu| h_sub <= k h_sub): y minus the nearest
// multiple of pi / 2 in three fused steps (pi / 2 split into three doubles), then fdlibm's kernel polynomials on
// [-pi / 4, pi / 4].  The absolute error stays below 3e-16 for y up to about 1e3 (the multiple below 2^10) and grows
// beyond, which only a clamped sublayer count reaches.  The library's sin and cos carry a reduction for arguments up
// to 1e308 that costs the modes kernel 65 vector registers and half of its occupancy; this does not.
DVH_RAYLEIGH_HD void sincos_sublayer(double y, double& s, double& c) {
  const double n = rint(y * 0.63661977236758134308);  // 2 / pi
  double r = fma(-n, 1.5707963267948966, y);
  r = fma(-n, 6.123233995736766e-17, r);
  r = fma(-n, -1.4973849048591698e-33, r);
  const double z = r * r;
  const double sp = -1.66666666666666324348e-01 +
                    z * (8.33333333332248946124e-03 +
                         z * (-1.98412698298579493134e-04 +
                              z * (2.75573137070700676789e-06 +
                                   z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
  const double cp = 4.16666666666666019037e-02 +
                    z * (-1.38888888888741095749e-03 +
                         z * (2.48015872894767294178e-05 +
                              z * (-2.75573143513906633035e-07 +
                                   z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
  const double sr = fma(r * z, sp, r), cr = fma(z * z, cp, fma(-0.5, z, 1.0));
  const int q = n < 2e9 ? (int)n & 3 : 0;  // a NaN or absurd argument takes no undefined conversion
  const double a = (q & 1) ? cr : sr, b = (q & 1) ? sr : cr;
  s = (q & 2) ? -a : a;
  c = (q == 1 || q == 2) ? -b : b;
}

// C = cosh(sqrt(x)) and S = sinh(sqrt(x)) / sqrt(x) for x = nu^2 h^2 of either sign.
DVH_RAYLEIGH_HD void cosh_sinhc(double x, double& C, double& S) {
  if (fabs(x) < 1e-2) {  // the next terms, x^7 / 14! and x^6 / 13!, are below 1e-24
    C = 1.0 + x / 2.0 * (1.0 + x / 12.0 * (1.0 + x / 30.0 * (1.0 + x / 56.0 * (1.0 + x / 90.0 * (1.0 + x / 132.0)))));
    S = 1.0 + x / 6.0 * (1.0 + x / 20.0 * (1.0 + x / 42.0 * (1.0 + x / 72.0 * (1.0 + x / 110.0))));
  } else if (x > 0.0) {
    const double y = sqrt(x), e = exp(y), ei = 1.0 / e;
    C = 0.5 * (e + ei);
    S = 0.5 * (e - ei) / y;
  } else {
    const double y = sqrt(-x);
    double sn;
    sincos_sublayer(y, sn, C);
    S = sn / y;
  }
}

// u <- u / |u|,  v <- (v - (u.v) u) / |..|
DVH_RAYLEIGH_HD void orthonormalise(double (&u)[4], double (&v)[4]) {
  const double nu = 1.0 / sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]);
  for (int i = 0; i < 4; ++i) u[i] *= nu;
  const double p = u[0] * v[0] + u[1] * v[1] + u[2] * v[2] + u[3] * v[3];
  for (int i = 0; i < 4; ++i) v[i] -= p * u[i];
  const double nv = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
  for (int i = 0; i < 4; ++i) v[i] *= nv;
}

struct LayerStep {
  double k, mu, t, mk2, irw2, Ca, Sa, na2Sa, Cb, Sb, nb2Sb;  // mk2 = 2 mu k, irw2 = 1 / (rho omega^2)
  DVH_RAYLEIGH_HD void apply(double (&y)[4]) const {
    const double mt = mu * t;
    const double a = (mk2 * y[0] + y[3]) * irw2;
    const double d = -(k * y[3] + mt * y[0]) * irw2;
    const double b = -(mt * y[1] + k * y[2]) * irw2;
    const double e = (y[2] + mk2 * y[1]) * irw2;
    const double a1 = a * Ca + b * Sa, b1 = b * Ca + a * na2Sa;
    const double e1 = e * Cb + d * Sb, d1 = d * Cb + e * nb2Sb;
    y[0] = k * a1 + d1;
    y[1] = b1 + k * e1;
    y[2] = -mk2 * b1 - mt * e1;
    y[3] = -mt * a1 - mk2 * d1;
  }
};

// The secular function at phase velocity c and angular frequency omega; layers [n_layer][4].  k_sub >= omega / c sets
// the sublayer counts (see above).
DVH_RAYLEIGH_HD double secular(const double* layers, int n_layer, double c, double omega, double k_sub) {
  const double k = omega / c, k2 = k * k, w2 = omega * omega;
  double u[4], v[4];
  {
    const double* L = layers + 4 * (n_layer - 1);
    const double al = L[1], be = L[2], mu = L[3] * be * be;
    const double na = sqrt(fmax(k2 - w2 / (al * al), 0.0)), nb = sqrt(fmax(k2 - w2 / (be * be), 0.0));
    const double mt = mu * (2.0 * k2 - w2 / (be * be));
    u[0] = k, u[1] = na, u[2] = -2.0 * mu * k * na, u[3] = -mt;
    v[0] = nb, v[1] = k, v[2] = -mt, v[3] = -2.0 * mu * k * nb;
    orthonormalise(u, v);
  }
  for (int l = n_layer - 2; l >= 0; --l) {
    const double* L = layers + 4 * l;
    const double h = L[0], al = L[1], be = L[2], rho = L[3];
    if (!(h > 0.0)) continue;
    const double ns = ceil(k_sub * h / kSubKh);
    int n_sub = ns >= (double)kMaxSub ? kMaxSub : (ns >= 1.0 ? (int)ns : 1);
#if defined(__HIP_DEVICE_COMPILE__)
    n_sub = __builtin_amdgcn_readfirstlane(n_sub);  // k_sub and the layer are the wave's: the loop count is scalar
#endif
    const double hs = h / (double)n_sub;
    const double kb2 = w2 / (be * be), na2 = k2 - w2 / (al * al), nb2 = k2 - kb2;
    LayerStep s;
    s.k = k;
    s.mu = rho * be * be;
    s.t = 2.0 * k2 - kb2;
    s.mk2 = 2.0 * s.mu * k;
    s.irw2 = 1.0 / (rho * w2);
    cosh_sinhc(na2 * hs * hs, s.Ca, s.Sa);
    cosh_sinhc(nb2 * hs * hs, s.Cb, s.Sb);
    s.Sa *= hs;
    s.Sb *= hs;
    s.na2Sa = na2 * s.Sa;
    s.nb2Sb = nb2 * s.Sb;
    for (int i = 0; i < n_sub; ++i) {
      s.apply(u);
      s.apply(v);
      orthonormalise(u, v);
    }
  }
  return u[2] * v[3] - u[3] * v[2];
}

}  // namespace rayleigh
}  // namespace dvh
