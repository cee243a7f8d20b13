// Rayleigh-wave forward model on the device (the inversion notebooks' surf96 / evodcinv stage):
//   dvh_rayleigh_modes         modal phase velocities of a batch of layered models at a set of periods: one wave per
//                              (model, period) scans the secular function of rayleigh.h at c_k = fma(k, dc, c_min),
//                              64 points a round, and refines every wanted sign change by 64-way sectioning.
//   dvh_curve_misfit           the weighted per-curve RMS misfit of those velocities against observed curves.
//   dvh_rayleigh_secular_host  the same secular function on the CPU over host memory (pins the arithmetic where there
//                              is no GPU; nothing computes curves with it).
// The scan is the definition of a mode: mode m is the (m + 1)-th sign change between consecutive scan points, so two
// roots closer than dc vanish as a pair, as in surf96's search.
#include <math.h>

#include "dvh_common.h"
#include "dvh.h"
#include "rayleigh.h"

namespace {
using dvh::set_error;
namespace ray = dvh::rayleigh;

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / 64;
constexpr int kMaxRounds = 1 << 10;  // scan rounds of 64 points a wave takes at most (65 536 points)
constexpr int kMaxRefine = 16;       // sectioning steps: five reach tol = 1e-9 from dc = 0.005

// The bracket (lo, hi) of one sign change, lo_neg the sign at lo, narrowed 65-fold a step until hi - lo <= tol lo: the
// lanes take the 64 interior points, the first lane whose sign differs from lo's closes the new bracket.  Every lane
// holds the same lo and hi throughout and returns the same midpoint.
__device__ double refine(const double* L, int n_layer, double omega, double lo, double hi, bool lo_neg, double tol,
                         int lane) {
  for (int it = 0; it < kMaxRefine && hi - lo > tol * lo; ++it) {
    const double w = (hi - lo) / 65.0;
    const double c = fma((double)(lane + 1), w, lo);
    const double f = ray::secular(L, n_layer, c, omega, omega / lo);
    const unsigned long long neg = __ballot(f < 0.0);
    const unsigned long long diff = lo_neg ? ~neg : neg;
    if (diff == 0ull) {
      lo = fma(64.0, w, lo);
    } else {
      const int j = __builtin_ctzll(diff);  // interior point j + 1 is the first on the other side
      const double nlo = j == 0 ? lo : fma((double)j, w, lo);
      hi = fma((double)(j + 1), w, lo);
      lo = nlo;
    }
  }
  return 0.5 * (lo + hi);
}

__global__ __launch_bounds__(kThreads) void rayleigh_modes_kernel(const double* __restrict__ layers, int n_wave,
                                                                  int n_layer, const double* __restrict__ periods,
                                                                  int n_period, const int32_t* __restrict__ need,
                                                                  double c_min, double dc, double tol, int n_mode,
                                                                  double* __restrict__ out_c,
                                                                  int32_t* __restrict__ out_count) {
  // the wave index through readfirstlane: the model's layers and the period are then read by scalar loads
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
  if (wave >= n_wave) return;
  const int lane = threadIdx.x & 63;
  const int model = wave / n_period, p = wave - model * n_period;
  const double* L = layers + (int64_t)model * n_layer * 4;
  int nd = need[p];
  nd = nd < 0 ? 0 : (nd > n_mode ? n_mode : nd);
  const double T = periods[p];
  const double beta_hs = L[4 * (n_layer - 1) + 2];
  int found = 0;
  double mine = NAN;  // lane m ends up holding mode m
  if (nd > 0 && T > 0.0) {
    const double omega = 2.0 * M_PI / T;
    unsigned long long prev_neg = 0ull, have_prev = 0ull;
    for (int round = 0; round < kMaxRounds && found < nd; ++round) {
      const int base = round * 64;
      const double c0 = fma((double)base, dc, c_min);  // the round's smallest c: its k sets the sublayer counts
      if (!(c0 < beta_hs)) break;
      const double c = fma((double)(base + lane), dc, c_min);
      const bool valid = c < beta_hs;
      const double f = ray::secular(L, n_layer, valid ? c : c0, omega, omega / c0);
      const unsigned long long vm = __ballot(valid), neg = __ballot(valid && f < 0.0);
      // bit l of pneg / pvm: the sign and validity of the point before lane l's (the carry is the last round's lane 63)
      const unsigned long long pneg = (neg << 1) | prev_neg, pvm = (vm << 1) | have_prev;
      unsigned long long change = (neg ^ pneg) & vm & pvm;
      while (change != 0ull && found < nd) {
        const int b = __builtin_ctzll(change);
        change &= change - 1ull;
        const double lo = fma((double)(base + b - 1), dc, c_min), hi = fma((double)(base + b), dc, c_min);
        const double root = refine(L, n_layer, omega, lo, hi, (pneg >> b) & 1ull, tol, lane);
        if (lane == found) mine = root;
        ++found;
      }
      prev_neg = neg >> 63;
      have_prev = vm >> 63;
    }
  }
  if (lane < n_mode) out_c[(int64_t)wave * n_mode + lane] = mine;
  if (lane == 0) out_count[wave] = found;
}

// One thread per model; every sum in table order.
__global__ __launch_bounds__(kThreads) void curve_misfit_kernel(const double* __restrict__ c, int n_model, int n_period,
                                                                int n_mode, const int32_t* __restrict__ sp,
                                                                const int32_t* __restrict__ sm,
                                                                const double* __restrict__ obs,
                                                                const double* __restrict__ sigma,
                                                                const int32_t* __restrict__ sc, int n_sample,
                                                                const double* __restrict__ cw, int n_curve,
                                                                double* __restrict__ out) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= n_model) return;
  const double* cm = c + (int64_t)m * n_period * n_mode;
  double num = 0.0, den = 0.0;
  for (int i = 0; i < n_curve; ++i) {
    double acc = 0.0;
    int n = 0;
    for (int j = 0; j < n_sample; ++j) {
      if (sc[j] != i) continue;
      const int pj = sp[j], mj = sm[j];
      const bool inside = pj >= 0 && pj < n_period && mj >= 0 && mj < n_mode;
      const double r = (obs[j] - (inside ? cm[(int64_t)pj * n_mode + mj] : NAN)) / sigma[j];
      acc += r * r;
      ++n;
    }
    num += cw[i] * sqrt(acc / (double)n);
    den += cw[i];
  }
  const double r = num / den;
  out[m] = isnan(r) ? INFINITY : r;
}

}  // namespace

DVH_API int dvh_rayleigh_modes(const double* layers, int32_t n_model, int32_t n_layer, const double* periods,
                               int32_t n_period, const int32_t* need, double c_min, double dc, double tol,
                               int32_t n_mode, double* out_c, int32_t* out_count, void* stream) {
  if (n_model < 0 || n_layer < 1 || n_period < 0 || n_mode < 1) return set_error(-2, "negative or empty count");
  if (!(dc > 0.0) || !(tol > 0.0) || !(c_min > 0.0) || !isfinite(dc) || !isfinite(tol) || !isfinite(c_min))
    return set_error(-2, "c_min, dc and tol must be positive and finite");
  if (n_layer > ray::kMaxLayers) return set_error(-4, "more than 32 layers");
  if (n_mode > ray::kMaxModes) return set_error(-4, "more than 16 modes");
  if (n_model == 0 || n_period == 0) return 0;
  if (!layers || !periods || !need || !out_c || !out_count) return set_error(-2, "null pointer argument");
  const int64_t n_wave = (int64_t)n_model * n_period;
  if (n_wave > 0x7fffffffLL - kWavesPerBlock) return set_error(-4, "too many (model, period) pairs for one launch");
  const unsigned blocks = (unsigned)((n_wave + kWavesPerBlock - 1) / kWavesPerBlock);
  rayleigh_modes_kernel<<<dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(
      layers, (int)n_wave, n_layer, periods, n_period, need, c_min, dc, tol, n_mode, out_c, out_count);
  return dvh::last_launch();
}

DVH_API int dvh_curve_misfit(const double* c, int32_t n_model, int32_t n_period, int32_t n_mode,
                             const int32_t* sample_period, const int32_t* sample_mode, const double* sample_obs,
                             const double* sample_sigma, const int32_t* sample_curve, int32_t n_sample,
                             const double* curve_weight, int32_t n_curve, double* out, void* stream) {
  if (n_model < 0 || n_period < 1 || n_mode < 1 || n_sample < 1 || n_curve < 1)
    return set_error(-2, "negative or empty count");
  if (n_model == 0) return 0;
  if (!c || !sample_period || !sample_mode || !sample_obs || !sample_sigma || !sample_curve || !curve_weight || !out)
    return set_error(-2, "null pointer argument");
  curve_misfit_kernel<<<dim3((unsigned)((n_model + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                        (hipStream_t)stream>>>(c, n_model, n_period, n_mode, sample_period, sample_mode, sample_obs,
                                               sample_sigma, sample_curve, n_sample, curve_weight, n_curve, out);
  return dvh::last_launch();
}

DVH_API int dvh_rayleigh_secular_host(const double* layers_host, int32_t n_layer, const double* c_host, int32_t n_c,
                                      double omega, double* out_host) {
  if (n_layer < 1 || n_c < 0) return set_error(-2, "negative or empty count");
  if (!(omega > 0.0) || !isfinite(omega)) return set_error(-2, "omega must be positive and finite");
  if (n_layer > ray::kMaxLayers) return set_error(-4, "more than 32 layers");
  if (n_c == 0) return 0;
  if (!layers_host || !c_host || !out_host) return set_error(-2, "null pointer argument");
  for (int l = 0; l < n_layer; ++l) {
    const double* L = layers_host + 4 * l;
    if (!(L[2] > 0.0) || !(L[1] > L[2]) || !(L[3] > 0.0) || !isfinite(L[1]) || !isfinite(L[3]) ||
        (l + 1 < n_layer && !(L[0] >= 0.0 && isfinite(L[0]))))
      return set_error(-2, "a layer needs h >= 0, alpha > beta > 0 and rho > 0");
  }
  for (int i = 0; i < n_c; ++i) {
    const double c = c_host[i];
    out_host[i] = c > 0.0 && isfinite(c) ? ray::secular(layers_host, n_layer, c, omega, omega / c) : NAN;
  }
  return 0;
}
