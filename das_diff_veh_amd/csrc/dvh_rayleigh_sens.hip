// Rayleigh sensitivity kernels and group velocity on the device (the "Sensitivity kernel" section of
// inversion_diff_weight.ipynb and the notebooks' surf96(..., itype=1, ...)):
//   dvh_rayleigh_sens          at every root of a dvh_rayleigh_modes result: one Newton step on the root, then
//                              dc/dp = -D_p / D_c for the selected layer columns and the group velocity
//                              U = c / (1 - (omega / c) dc/domega), dc/domega = -D_omega / D_c, with the derivatives
//                              of the secular function from rayleigh_tangent.h.  One wave per (model, period, mode),
//                              one tangent direction per lane.
//   dvh_rayleigh_tangent_host  the same header on the CPU over host memory (pins the arithmetic where there is no GPU).
#include <math.h>

#include "dvh_common.h"
#include "dvh.h"
#include "rayleigh_tangent.h"

namespace {
using dvh::set_error;
namespace ray = dvh::rayleigh;

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / 64;

// Slot s of a wave's directions: 0 is c, 1 is omega, 2 + j is the j-th selected (layer, column) pair in layer order.
// A slot past the last one gets -1, which tangent() answers with a zero derivative.
__device__ int direction_of(int s, int n_layer, int n_sel, unsigned sel_cols) {
  if (s < 2) return s;
  const int j = s - 2;
  if (n_sel == 0 || j >= n_layer * n_sel) return -1;
  const int layer = j / n_sel, q = (sel_cols >> (8 * (j - layer * n_sel))) & 0xff;
  return 2 + 4 * layer + q;
}

__global__ __launch_bounds__(kThreads) void rayleigh_sens_kernel(const double* __restrict__ layers, int n_wave,
                                                                 int n_layer, const double* __restrict__ periods,
                                                                 int n_period, const double* __restrict__ c_in,
                                                                 int n_mode, int par_mask, double tol,
                                                                 double* __restrict__ out_c,
                                                                 double* __restrict__ out_u,
                                                                 double* __restrict__ out_dcdp) {
  // the wave index through readfirstlane: the model's layers, the period and the root are then read by scalar loads
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
  if (wave >= n_wave) return;
  const int lane = threadIdx.x & 63;
  const int mp = wave / n_mode, model = mp / n_period, p = mp - model * n_period;
  const double* L = layers + (int64_t)model * n_layer * 4;
  double* dcdp = out_dcdp ? out_dcdp + (int64_t)wave * n_layer * 4 : nullptr;
  const double T = periods[p], c0 = c_in[wave];
  const bool ok = c0 > 0.0 && isfinite(c0) && T > 0.0 && isfinite(T);
  if (dcdp)  // every slot is written: NaN here, the selected columns of a wave that has a root below
    for (int i = lane; i < n_layer * 4; i += 64)
      if (!ok || !((par_mask >> (i & 3)) & 1)) dcdp[i] = NAN;
  if (!ok) {
    if (lane == 0) {
      if (out_c) out_c[wave] = NAN;
      if (out_u) out_u[wave] = NAN;
    }
    return;
  }
  const double omega = 2.0 * M_PI / T;
  // the selected columns, packed a byte each
  int n_sel = 0;
  unsigned sel_cols = 0u;
  if (dcdp)
    for (int q = 0; q < 4; ++q)
      if ((par_mask >> q) & 1) sel_cols |= (unsigned)q << (8 * n_sel++);
  const int n_dir = out_u || dcdp ? 2 + n_layer * n_sel : 0;
  // Round -1 is one Newton step on the root, the same on every lane, kept if it stays within the width the root was
  // refined to; the rounds from 0 on take the directions at that c, 64 a round (wave-uniform: at most three, for
  // 2 + 32 x 4 directions).  One loop, so that tangent() is expanded once.
  double c = c0, Dc = 0.0;
  for (int round = -1; round * 64 < n_dir; ++round) {
    const int dir = round < 0 ? 0 : direction_of(round * 64 + lane, n_layer, n_sel, sel_cols);
    double D, dD;
    ray::tangent(L, n_layer, c, omega, omega / c, dir, D, dD);
    if (round < 0) {
      const double c1 = c - D / dD;
      if (fabs(c1 - c) <= 4.0 * tol * c) c = c1;
      if (out_c && lane == 0) out_c[wave] = c;
      continue;
    }
    if (round == 0) Dc = __shfl(dD, 0);  // slot 0 is D_c at the polished root
    const double dc = 0.0 - dD / Dc;
    if (dir == 1) {
      if (out_u) out_u[wave] = c / (1.0 - omega / c * dc);
    } else if (dir >= 2) {
      dcdp[dir - 2] = dc;
    }
  }
}

}  // namespace

DVH_API int dvh_rayleigh_sens(const double* layers, int32_t n_model, int32_t n_layer, const double* periods,
                              int32_t n_period, const double* c, int32_t n_mode, int32_t par_mask, double tol,
                              double* out_c, double* out_u, double* out_dcdp, void* stream) {
  if (n_model < 0 || n_layer < 1 || n_period < 0 || n_mode < 1) return set_error(-2, "negative or empty count");
  if (!(tol > 0.0) || !isfinite(tol)) return set_error(-2, "tol must be positive and finite");
  if (par_mask < 0 || par_mask > 15) return set_error(-2, "par_mask selects columns by bits 0 .. 3");
  if (n_layer > ray::kMaxLayers) return set_error(-4, "more than 32 layers");
  if (n_mode > ray::kMaxModes) return set_error(-4, "more than 16 modes");
  if (n_model == 0 || n_period == 0) return 0;
  if (!layers || !periods || !c) return set_error(-2, "null pointer argument");
  if (!out_c && !out_u && !out_dcdp) return set_error(-2, "at least one output is needed");
  const int64_t n_wave = (int64_t)n_model * n_period * n_mode;
  if (n_wave > 0x7fffffffLL - kWavesPerBlock) return set_error(-4, "too many (model, period, mode) for one launch");
  const unsigned blocks = (unsigned)((n_wave + kWavesPerBlock - 1) / kWavesPerBlock);
  rayleigh_sens_kernel<<<dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(
      layers, (int)n_wave, n_layer, periods, n_period, c, n_mode, par_mask, tol, out_c, out_u, out_dcdp);
  return dvh::last_launch();
}

DVH_API int dvh_rayleigh_tangent_host(const double* layers_host, int32_t n_layer, const double* c_host, int32_t n_c,
                                      double omega, const int32_t* dirs_host, int32_t n_dir, double* out_D,
                                      double* out_dD) {
  if (n_layer < 1 || n_c < 0 || n_dir < 1) return set_error(-2, "negative or empty count");
  if (!(omega > 0.0) || !isfinite(omega)) return set_error(-2, "omega must be positive and finite");
  if (n_layer > ray::kMaxLayers) return set_error(-4, "more than 32 layers");
  if (n_c == 0) return 0;
  if (!layers_host || !c_host || !dirs_host || !out_D || !out_dD) return set_error(-2, "null pointer argument");
  for (int l = 0; l < n_layer; ++l) {
    const double* L = layers_host + 4 * l;
    if (!(L[2] > 0.0) || !(L[1] > L[2]) || !(L[3] > 0.0) || !isfinite(L[1]) || !isfinite(L[3]) ||
        (l + 1 < n_layer && !(L[0] >= 0.0 && isfinite(L[0]))))
      return set_error(-2, "a layer needs h >= 0, alpha > beta > 0 and rho > 0");
  }
  for (int j = 0; j < n_dir; ++j)
    if (dirs_host[j] < 0 || dirs_host[j] >= 2 + 4 * n_layer)
      return set_error(-2, "a direction is 0 (c), 1 (omega) or 2 + 4 layer + column");
  for (int i = 0; i < n_c; ++i) {
    const double c = c_host[i];
    const bool ok = c > 0.0 && isfinite(c);
    double D = NAN, dD = NAN;
    for (int j = 0; j < n_dir; ++j) {
      if (ok) ray::tangent(layers_host, n_layer, c, omega, omega / c, dirs_host[j], D, dD);
      out_dD[(int64_t)i * n_dir + j] = dD;
    }
    out_D[i] = D;  // the value part: the same for every direction
  }
  return 0;
}
