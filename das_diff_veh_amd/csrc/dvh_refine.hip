// Damped Gauss-Newton (Levenberg-Marquardt) refinement of inverted models ("Gauss-Newton refinement"):
//   dvh_lm_normal       misfit f, its gradient g and the Gauss-Newton matrix H in the unit cube of the bounds, from the
//                       roots and sensitivities of dvh_rayleigh_sens and the chain rule of the parameters.  One
//                       workgroup per model; an output entry is one thread's sum over the samples in table order.
//   dvh_lm_normal_sets  the same with an observation set per model: set_obs and set_sigma [n_set][n_sample], model m
//                       scored against set model_set[m], a NaN observation marking an absent sample.  The same kernel,
//                       compiled with the presence test in.
//   dvh_lm_solve        (H + lambda diag(d)) delta = -g over the free parameters by a float64 Cholesky factorisation
//                       in LDS, one wave per model.
//   dvh_lm_normal_host, dvh_lm_normal_sets_host, dvh_lm_solve_host   the same header (refine.h) on the CPU over host
//                       memory.
#include <math.h>

#include "dvh_common.h"
#include "dvh.h"
#include "rayleigh.h"
#include "refine.h"

namespace {
using dvh::set_error;
namespace ray = dvh::rayleigh;
namespace lm = dvh::refine;

constexpr int kThreads = 256;
constexpr int kTile = 32;                                                           // samples of J held in LDS
constexpr int kStage = 1024;                                                        // samples of a residual stage
constexpr int kMaxPairs = lm::kMaxParams * (lm::kMaxParams + 1) / 2;                // 4656
constexpr int kPairsPerThread = (kMaxPairs + kThreads - 1) / kThreads;              // 19
constexpr int kSolveThreads = 64;
constexpr int kRowsPerLane = (lm::kMaxParams + kSolveThreads - 1) / kSolveThreads;  // 2

struct NormalArgs {
  const double* c;
  const double* dcdp;
  const double* chain;
  int n_layer, n_param;
  lm::Table tab;  // with sets, obs and sigma are set_obs and set_sigma [n_set][n_sample]
  const int32_t* model_set;
  int n_set;
  const double* curve_weight;
  double rho_floor;
  double* out_f;
  double* out_g;
  double* out_H;
  int32_t* out_status;
};

template <bool kSets>
__global__ __launch_bounds__(kThreads) void lm_normal_kernel(NormalArgs a) {
  __shared__ double jt[kTile][lm::kMaxParams];  // the tile's rows of J
  __shared__ double wa[kTile], wr[kTile];       // a_s and a_s r_s of the tile's samples
  __shared__ double rho[lm::kMaxCurves], fac[lm::kMaxCurves], total_w;
  __shared__ int count[lm::kMaxCurves];
  __shared__ double r2[kStage];  // squared residuals and curves of a stage of samples
  __shared__ int curve_of[kStage];
  __shared__ bool here[kTile];  // sets: whether the tile's sample is present
  const int tid = threadIdx.x, model = blockIdx.x;
  lm::Table t = a.tab;
  const int D = a.n_param, K = 4 * a.n_layer, S = t.n_sample;
  const int64_t slots = (int64_t)t.n_period * t.n_mode;
  const double* cm = a.c + model * slots;
  const double* dm = a.dcdp + model * slots * K;
  const double* chain = a.chain + (int64_t)model * K * D;
  double* g = a.out_g + (int64_t)model * D;
  double* H = a.out_H + (int64_t)model * D * D;

  // 1. only sampled slots are read: a sample outside c, a root or a dcdp value that is not finite flags the model.
  // With sets the model's set is block-uniform (its rows are a scalar base), a set outside the table flags the model
  // before anything is read, and only present samples are looked at: theirs is the sigma that must be positive.
  int bad = 0;
  if (kSets && !lm::select_set(t, a.model_set[model], a.n_set)) bad = 1;
  if (!bad) {
    for (int s = tid; s < S; s += kThreads) {
      if (!lm::present<kSets>(t, s)) continue;
      const int64_t at = lm::slot_of(t, s);
      if (at < 0 || !lm::is_finite(cm[at])) bad = 1;
      if (kSets && !lm::sigma_ok(t.sigma[s])) bad = 1;
    }
    if (__syncthreads_or(bad) == 0) {
      for (int64_t e = tid; e < (int64_t)S * K; e += kThreads) {
        const int s = (int)(e / K);
        if (!lm::present<kSets>(t, s)) continue;
        if (!lm::is_finite(dm[lm::slot_of(t, s) * K + (e - (int64_t)s * K)])) bad = 1;
      }
      bad = __syncthreads_or(bad);
    } else {
      bad = 1;
    }
  }
  // 2. the curves: rho_i, n_i, then f and a_i.  The squared residuals are staged through LDS by all threads; thread i
  // then adds those of curve i in table order.  An absent sample is staged as curve -1, which nobody adds; a curve
  // without a sample flags the model; with sets it drops out of f and W, and only a set without any sample flags.
  if (!bad) {
    double acc = 0.0;
    int n = 0;
    for (int s0 = 0; s0 < S; s0 += kStage) {
      const int ns = min(kStage, S - s0);
      __syncthreads();
      for (int e = tid; e < ns; e += kThreads) {
        if (!lm::present<kSets>(t, s0 + e)) {
          curve_of[e] = -1;
          continue;
        }
        const double r = lm::residual(t, cm, s0 + e);
        r2[e] = r * r;
        curve_of[e] = t.curve[s0 + e];
      }
      __syncthreads();
      if (tid < t.n_curve)
        for (int e = 0; e < ns; ++e)
          if (curve_of[e] == tid) {
            acc += r2[e];
            ++n;
          }
    }
    if (tid < t.n_curve) {
      rho[tid] = lm::rms_of(acc, n);
      count[tid] = n;
      if (!kSets && n == 0) bad = 1;
    }
    bad = kSets ? !__syncthreads_or(tid < t.n_curve && n > 0) : __syncthreads_or(bad);
  }
  if (bad) {  // block-uniform
    for (int e = tid; e < D * D; e += kThreads) H[e] = 0.0;
    for (int e = tid; e < D; e += kThreads) g[e] = 0.0;
    if (tid == 0) {
      a.out_f[model] = INFINITY;
      a.out_status[model] = 1;
    }
    return;
  }
  if (tid == 0) {
    double W;
    a.out_f[model] = lm::misfit_of(a.curve_weight, rho, count, t.n_curve, W);
    a.out_status[model] = 0;
    total_w = W;
  }
  __syncthreads();
  for (int i = tid; i < t.n_curve; i += kThreads)
    fac[i] = lm::curve_factor(a.curve_weight[i], total_w, count[i], rho[i], a.rho_floor);
  // 3. g and the lower triangle of H: thread tid owns g[tid] and the pairs tid, tid + 256, ..
  const int n_pair = D * (D + 1) / 2;
  int pk[kPairsPerThread], pl[kPairsPerThread];
  double hacc[kPairsPerThread], gacc = 0.0;
#pragma unroll
  for (int q = 0; q < kPairsPerThread; ++q) {
    hacc[q] = 0.0;
    pk[q] = pl[q] = 0;
    if (tid + q * kThreads < n_pair) lm::pair_of(tid + q * kThreads, pk[q], pl[q]);
  }
  for (int s0 = 0; s0 < S; s0 += kTile) {
    const int ns = min(kTile, S - s0);
    __syncthreads();  // the tile before has been consumed (and fac is written)
    for (int e = tid; e < ns * D; e += kThreads) {
      const int i = e / D, k = e - i * D, s = s0 + i;
      if (!lm::present<kSets>(t, s)) continue;
      jt[i][k] = lm::jacobian_entry(dm + lm::slot_of(t, s) * K, chain, K, D, k, t.sigma[s]);
    }
    if (tid < ns) {
      const bool p = lm::present<kSets>(t, s0 + tid);
      if (kSets) here[tid] = p;
      if (p) {
        const double w = fac[t.curve[s0 + tid]];
        wa[tid] = w;
        wr[tid] = w * lm::residual(t, cm, s0 + tid);
      }
    }
    __syncthreads();
    for (int i = 0; i < ns; ++i) {
      if (kSets && !here[i]) continue;  // block-uniform: an absent sample adds no term
      if (tid < D) gacc = lm::add_g(gacc, wr[i], jt[i][tid]);
#pragma unroll
      for (int q = 0; q < kPairsPerThread; ++q)
        if (tid + q * kThreads < n_pair) hacc[q] = lm::add_h(hacc[q], wa[i], jt[i][pk[q]], jt[i][pl[q]]);
    }
  }
  if (tid < D) g[tid] = gacc;
#pragma unroll
  for (int q = 0; q < kPairsPerThread; ++q)
    if (tid + q * kThreads < n_pair) {
      H[pk[q] * D + pl[q]] = hacc[q];
      H[pl[q] * D + pk[q]] = hacc[q];
    }
}

__global__ __launch_bounds__(kSolveThreads) void lm_solve_kernel(const double* __restrict__ H_all,
                                                                 const double* __restrict__ g_all,
                                                                 const double* __restrict__ lambda,
                                                                 const int32_t* __restrict__ free_mask, int D,
                                                                 double* __restrict__ out_delta,
                                                                 int32_t* __restrict__ out_status) {
  __shared__ double L[kMaxPairs];
  __shared__ double y[lm::kMaxParams], step[lm::kMaxParams];
  __shared__ int idx[lm::kMaxParams];
  __shared__ int n_free, failed;
  __shared__ double hmax_s;
  const int lane = threadIdx.x, model = blockIdx.x;
  const double* H = H_all + (int64_t)model * D * D;
  const double* g = g_all + (int64_t)model * D;
  double* delta = out_delta + (int64_t)model * D;
  if (lane == 0) {  // the free parameters in order, and the largest diagonal entry among them
    int n = 0;
    double hmax = -INFINITY;
    for (int k = 0; k < D; ++k)
      if (free_mask[k] != 0) {
        idx[n++] = k;
        hmax = fmax(hmax, H[(int64_t)k * D + k]);
      }
    n_free = n;
    hmax_s = hmax;
    failed = n == 0;
  }
  __syncthreads();
  const int n = n_free;
  const double lam = lambda[model], hmax = hmax_s;
  for (int p = lane; p < n * (n + 1) / 2; p += kSolveThreads) {
    int i, j;
    lm::pair_of(p, i, j);
    const double h = H[(int64_t)idx[i] * D + idx[j]];
    L[p] = i == j ? lm::damped_diagonal(h, hmax, lam) : h;
  }
  for (int i = lane; i < n; i += kSolveThreads) y[i] = 0.0 - g[idx[i]];
  __syncthreads();
  // factorisation, a column a step: every row of the column reduces against the finished columns, then scales
  for (int j = 0; j < n; ++j) {
    double v[kRowsPerLane];
#pragma unroll
    for (int q = 0; q < kRowsPerLane; ++q) {
      const int i = j + lane + q * kSolveThreads;
      v[q] = i < n ? lm::chol_reduce(L, i, j) : 0.0;
    }
    if (lane == 0) {
      if (!lm::pivot_ok(v[0])) failed = 1;
      L[lm::tri(j, j)] = sqrt(v[0]);
    }
    __syncthreads();
    if (failed) break;  // block-uniform
    const double d = L[lm::tri(j, j)];
#pragma unroll
    for (int q = 0; q < kRowsPerLane; ++q) {
      const int i = j + lane + q * kSolveThreads;
      if (i > j && i < n) L[lm::tri(i, j)] = v[q] / d;
    }
    __syncthreads();
  }
  if (!failed) {
    for (int j = 0; j < n; ++j) {  // L z = -g
      if (lane == 0) y[j] = y[j] / L[lm::tri(j, j)];
      __syncthreads();
      const double z = y[j];
      for (int i = j + 1 + lane; i < n; i += kSolveThreads) y[i] -= L[lm::tri(i, j)] * z;
      __syncthreads();
    }
    for (int j = n - 1; j >= 0; --j) {  // L^T delta = z
      if (lane == 0) y[j] = y[j] / L[lm::tri(j, j)];
      __syncthreads();
      const double x = y[j];
      for (int i = lane; i < j; i += kSolveThreads) y[i] -= L[lm::tri(j, i)] * x;
      __syncthreads();
    }
    for (int i = lane; i < n; i += kSolveThreads)
      if (!lm::is_finite(y[i])) failed = 1;  // every writer stores the same value
    __syncthreads();
  }
  for (int k = lane; k < D; k += kSolveThreads) step[k] = 0.0;  // fixed parameters, and every one after a failure
  __syncthreads();
  if (!failed)
    for (int i = lane; i < n; i += kSolveThreads) step[idx[i]] = y[i];
  __syncthreads();
  for (int k = lane; k < D; k += kSolveThreads) delta[k] = step[k];
  if (lane == 0) out_status[model] = failed ? 2 : 0;
}

// model_set and n_set are asked of only with sets.
int check_normal(const void* c, const void* dcdp, const void* chain, int32_t n_model, int32_t n_period, int32_t n_mode,
                 int32_t n_layer, int32_t n_param, const void* sp, const void* sm, const void* so, const void* ss,
                 const void* sc, int32_t n_sample, const void* cw, int32_t n_curve, double rho_floor, const void* out_f,
                 const void* out_g, const void* out_H, const void* out_status, bool sets = false,
                 const void* model_set = nullptr, int32_t n_set = 1) {
  if (sets && n_set < 1) return set_error(-2, "negative or empty count");
  if (n_model < 0 || n_period < 1 || n_mode < 1 || n_layer < 1 || n_param < 1 || n_sample < 1 || n_curve < 1)
    return set_error(-2, "negative or empty count");
  if (!(rho_floor > 0.0) || !isfinite(rho_floor)) return set_error(-2, "rho_floor must be positive and finite");
  if (n_param > lm::kMaxParams) return set_error(-4, "more than 96 parameters");
  if (n_layer > ray::kMaxLayers) return set_error(-4, "more than 32 layers");
  if (n_mode > ray::kMaxModes) return set_error(-4, "more than 16 modes");
  if (n_curve > lm::kMaxCurves) return set_error(-4, "more than 64 curves");
  if (n_model == 0) return 1;
  if (!c || !dcdp || !chain || !sp || !sm || !so || !ss || !sc || !cw || !out_f || !out_g || !out_H || !out_status ||
      (sets && !model_set))
    return set_error(-2, "null pointer argument");
  return 0;
}

// dvh_lm_normal_host (kSets false: so and ss are the table's obs and sigma) and dvh_lm_normal_sets_host, after their
// checks.
template <bool kSets>
void normal_host(const double* c, const double* dcdp, const double* chain, int32_t n_model, const lm::Table& tab,
                 const int32_t* model_set, int32_t n_set, int32_t n_layer, int32_t n_param, const double* curve_weight,
                 double rho_floor, double* out_f, double* out_g, double* out_H, int32_t* out_status) {
  const int D = n_param, K = 4 * n_layer, S = tab.n_sample, n_curve = tab.n_curve;
  const int64_t slots = (int64_t)tab.n_period * tab.n_mode;
  double rho[lm::kMaxCurves], fac[lm::kMaxCurves], j[lm::kMaxParams];
  int count[lm::kMaxCurves];
  for (int model = 0; model < n_model; ++model) {
    const double* cm = c + model * slots;
    const double* dm = dcdp + model * slots * K;
    const double* ch = chain + (int64_t)model * K * D;
    double* g = out_g + (int64_t)model * D;
    double* H = out_H + (int64_t)model * D * D;
    for (int e = 0; e < D * D; ++e) H[e] = 0.0;
    for (int e = 0; e < D; ++e) g[e] = 0.0;
    lm::Table t = tab;
    bool bad = kSets && !lm::select_set(t, model_set[model], n_set);
    for (int s = 0; s < S && !bad; ++s) {
      if (!lm::present<kSets>(t, s)) continue;
      const int64_t at = lm::slot_of(t, s);
      bad = at < 0 || !lm::is_finite(cm[at]) || (kSets && !lm::sigma_ok(t.sigma[s]));
      for (int r = 0; r < K && !bad; ++r) bad = !lm::is_finite(dm[at * K + r]);
    }
    int n_present = 0;
    for (int i = 0; i < n_curve && !bad; ++i) {
      lm::curve_rms<kSets>(t, cm, i, rho[i], count[i]);
      n_present += count[i];
      bad = !kSets && count[i] == 0;
    }
    bad = bad || n_present == 0;
    out_status[model] = bad ? 1 : 0;
    if (bad) {
      out_f[model] = INFINITY;
      continue;
    }
    double W;
    out_f[model] = lm::misfit_of(curve_weight, rho, count, n_curve, W);
    for (int i = 0; i < n_curve; ++i) fac[i] = lm::curve_factor(curve_weight[i], W, count[i], rho[i], rho_floor);
    for (int s = 0; s < S; ++s) {
      if (!lm::present<kSets>(t, s)) continue;
      for (int k = 0; k < D; ++k) j[k] = lm::jacobian_entry(dm + lm::slot_of(t, s) * K, ch, K, D, k, t.sigma[s]);
      const double w = fac[t.curve[s]], wr = w * lm::residual(t, cm, s);
      for (int k = 0; k < D; ++k) {
        g[k] = lm::add_g(g[k], wr, j[k]);
        for (int l = 0; l <= k; ++l) H[k * D + l] = lm::add_h(H[k * D + l], w, j[k], j[l]);
      }
    }
    for (int k = 0; k < D; ++k)
      for (int l = 0; l < k; ++l) H[l * D + k] = H[k * D + l];
  }
}

int check_solve(const void* H, const void* g, const void* lambda, const void* free_mask, int32_t n_model,
                int32_t n_param, const void* out_delta, const void* out_status) {
  if (n_model < 0 || n_param < 1) return set_error(-2, "negative or empty count");
  if (n_param > lm::kMaxParams) return set_error(-4, "more than 96 parameters");
  if (n_model == 0) return 1;
  if (!H || !g || !lambda || !free_mask || !out_delta || !out_status) return set_error(-2, "null pointer argument");
  return 0;
}

}  // namespace

DVH_API int dvh_lm_normal(const double* c, const double* dcdp, const double* chain, int32_t n_model, int32_t n_period,
                          int32_t n_mode, int32_t n_layer, int32_t n_param, const int32_t* sample_period,
                          const int32_t* sample_mode, const double* sample_obs, const double* sample_sigma,
                          const int32_t* sample_curve, int32_t n_sample, const double* curve_weight, int32_t n_curve,
                          double rho_floor, double* out_f, double* out_g, double* out_H, int32_t* out_status,
                          void* stream) {
  const int rc = check_normal(c, dcdp, chain, n_model, n_period, n_mode, n_layer, n_param, sample_period, sample_mode,
                              sample_obs, sample_sigma, sample_curve, n_sample, curve_weight, n_curve, rho_floor,
                              out_f, out_g, out_H, out_status);
  if (rc) return rc < 0 ? rc : 0;
  NormalArgs a{c, dcdp, chain, n_layer, n_param,
               lm::Table{sample_period, sample_mode, sample_obs, sample_sigma, sample_curve, n_sample, n_curve,
                         n_period, n_mode},
               nullptr, 1, curve_weight, rho_floor, out_f, out_g, out_H, out_status};
  lm_normal_kernel<false><<<dim3((unsigned)n_model), dim3(kThreads), 0, (hipStream_t)stream>>>(a);
  return dvh::last_launch();
}

DVH_API int dvh_lm_normal_sets(const double* c, const double* dcdp, const double* chain, int32_t n_model,
                               int32_t n_period, int32_t n_mode, int32_t n_layer, int32_t n_param,
                               const int32_t* sample_period, const int32_t* sample_mode, const double* set_obs,
                               const double* set_sigma, const int32_t* model_set, int32_t n_set,
                               const int32_t* sample_curve, int32_t n_sample, const double* curve_weight,
                               int32_t n_curve, double rho_floor, double* out_f, double* out_g, double* out_H,
                               int32_t* out_status, void* stream) {
  const int rc = check_normal(c, dcdp, chain, n_model, n_period, n_mode, n_layer, n_param, sample_period, sample_mode,
                              set_obs, set_sigma, sample_curve, n_sample, curve_weight, n_curve, rho_floor, out_f,
                              out_g, out_H, out_status, true, model_set, n_set);
  if (rc) return rc < 0 ? rc : 0;
  NormalArgs a{c, dcdp, chain, n_layer, n_param,
               lm::Table{sample_period, sample_mode, set_obs, set_sigma, sample_curve, n_sample, n_curve, n_period,
                         n_mode},
               model_set, n_set, curve_weight, rho_floor, out_f, out_g, out_H, out_status};
  lm_normal_kernel<true><<<dim3((unsigned)n_model), dim3(kThreads), 0, (hipStream_t)stream>>>(a);
  return dvh::last_launch();
}

DVH_API int dvh_lm_solve(const double* H, const double* g, const double* lambda, const int32_t* free_mask,
                         int32_t n_model, int32_t n_param, double* out_delta, int32_t* out_status, void* stream) {
  const int rc = check_solve(H, g, lambda, free_mask, n_model, n_param, out_delta, out_status);
  if (rc) return rc < 0 ? rc : 0;
  lm_solve_kernel<<<dim3((unsigned)n_model), dim3(kSolveThreads), 0, (hipStream_t)stream>>>(
      H, g, lambda, free_mask, n_param, out_delta, out_status);
  return dvh::last_launch();
}

DVH_API int dvh_lm_normal_host(const double* c, const double* dcdp, const double* chain, int32_t n_model,
                               int32_t n_period, int32_t n_mode, int32_t n_layer, int32_t n_param,
                               const int32_t* sample_period, const int32_t* sample_mode, const double* sample_obs,
                               const double* sample_sigma, const int32_t* sample_curve, int32_t n_sample,
                               const double* curve_weight, int32_t n_curve, double rho_floor, double* out_f,
                               double* out_g, double* out_H, int32_t* out_status) {
  const int rc = check_normal(c, dcdp, chain, n_model, n_period, n_mode, n_layer, n_param, sample_period, sample_mode,
                              sample_obs, sample_sigma, sample_curve, n_sample, curve_weight, n_curve, rho_floor,
                              out_f, out_g, out_H, out_status);
  if (rc) return rc < 0 ? rc : 0;
  normal_host<false>(c, dcdp, chain, n_model,
                     lm::Table{sample_period, sample_mode, sample_obs, sample_sigma, sample_curve, n_sample, n_curve,
                               n_period, n_mode},
                     nullptr, 1, n_layer, n_param, curve_weight, rho_floor, out_f, out_g, out_H, out_status);
  return 0;
}

DVH_API int dvh_lm_normal_sets_host(const double* c, const double* dcdp, const double* chain, int32_t n_model,
                                    int32_t n_period, int32_t n_mode, int32_t n_layer, int32_t n_param,
                                    const int32_t* sample_period, const int32_t* sample_mode, const double* set_obs,
                                    const double* set_sigma, const int32_t* model_set, int32_t n_set,
                                    const int32_t* sample_curve, int32_t n_sample, const double* curve_weight,
                                    int32_t n_curve, double rho_floor, double* out_f, double* out_g, double* out_H,
                                    int32_t* out_status) {
  const int rc = check_normal(c, dcdp, chain, n_model, n_period, n_mode, n_layer, n_param, sample_period, sample_mode,
                              set_obs, set_sigma, sample_curve, n_sample, curve_weight, n_curve, rho_floor, out_f,
                              out_g, out_H, out_status, true, model_set, n_set);
  if (rc) return rc < 0 ? rc : 0;
  normal_host<true>(c, dcdp, chain, n_model,
                    lm::Table{sample_period, sample_mode, set_obs, set_sigma, sample_curve, n_sample, n_curve, n_period,
                              n_mode},
                    model_set, n_set, n_layer, n_param, curve_weight, rho_floor, out_f, out_g, out_H, out_status);
  return 0;
}

DVH_API int dvh_lm_solve_host(const double* H_all, const double* g_all, const double* lambda,
                              const int32_t* free_mask, int32_t n_model, int32_t n_param, double* out_delta,
                              int32_t* out_status) {
  const int rc = check_solve(H_all, g_all, lambda, free_mask, n_model, n_param, out_delta, out_status);
  if (rc) return rc < 0 ? rc : 0;
  const int D = n_param;
  static thread_local double L[kMaxPairs];
  double y[lm::kMaxParams], v[lm::kMaxParams];
  int idx[lm::kMaxParams];
  for (int model = 0; model < n_model; ++model) {
    const double* H = H_all + (int64_t)model * D * D;
    const double* g = g_all + (int64_t)model * D;
    double* delta = out_delta + (int64_t)model * D;
    int n = 0;
    double hmax = -INFINITY;
    for (int k = 0; k < D; ++k) {
      delta[k] = 0.0;
      if (free_mask[k] != 0) {
        idx[n++] = k;
        hmax = fmax(hmax, H[(int64_t)k * D + k]);
      }
    }
    bool failed = n == 0;
    for (int i = 0; i < n; ++i) {
      for (int j2 = 0; j2 <= i; ++j2) {
        const double h = H[(int64_t)idx[i] * D + idx[j2]];
        L[lm::tri(i, j2)] = i == j2 ? lm::damped_diagonal(h, hmax, lambda[model]) : h;
      }
      y[i] = 0.0 - g[idx[i]];
    }
    for (int j2 = 0; j2 < n && !failed; ++j2) {
      for (int i = j2; i < n; ++i) v[i] = lm::chol_reduce(L, i, j2);
      failed = !lm::pivot_ok(v[j2]);
      if (failed) break;
      const double d = L[lm::tri(j2, j2)] = sqrt(v[j2]);
      for (int i = j2 + 1; i < n; ++i) L[lm::tri(i, j2)] = v[i] / d;
    }
    if (!failed) {
      for (int j2 = 0; j2 < n; ++j2) {
        const double z = y[j2] = y[j2] / L[lm::tri(j2, j2)];
        for (int i = j2 + 1; i < n; ++i) y[i] -= L[lm::tri(i, j2)] * z;
      }
      for (int j2 = n - 1; j2 >= 0; --j2) {
        const double x = y[j2] = y[j2] / L[lm::tri(j2, j2)];
        for (int i = 0; i < j2; ++i) y[i] -= L[lm::tri(j2, i)] * x;
      }
      for (int i = 0; i < n; ++i) failed = failed || !lm::is_finite(y[i]);
    }
    if (!failed)
      for (int i = 0; i < n; ++i) delta[idx[i]] = y[i];
    out_status[model] = failed ? 2 : 0;
  }
  return 0;
}
