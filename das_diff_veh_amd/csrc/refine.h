// The arithmetic of the damped Gauss-Newton step ("Gauss-Newton refinement"), written once for the device
// kernels and the host entries of dvh_refine.hip.  Every output entry is one sequential chain of operations in an order
// fixed by the sample table and the shapes: the device gives an entry to one thread, the host to one loop, and the two
// differ only by the FMA contraction of the device compile.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DVH_HD __host__ __device__ inline
#else
#define DVH_HD inline
#endif

namespace dvh {
namespace refine {

constexpr int kMaxParams = 96;  // DVH_LM_MAX_PARAMS
constexpr int kMaxCurves = 64;  // DVH_LM_MAX_CURVES

// The sample table of dvh_curve_misfit, and the shape of c it indexes.
struct Table {
  const int32_t* period;
  const int32_t* mode;
  const double* obs;
  const double* sigma;
  const int32_t* curve;
  int n_sample, n_curve, n_period, n_mode;
};

DVH_HD bool is_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN

// The (period, mode) slot of sample s in c, or -1 if the sample indexes outside c or names no curve.
DVH_HD int64_t slot_of(const Table& t, int s) {
  const int p = t.period[s], m = t.mode[s], i = t.curve[s];
  if (p < 0 || p >= t.n_period || m < 0 || m >= t.n_mode || i < 0 || i >= t.n_curve) return -1;
  return (int64_t)p * t.n_mode + m;
}

// Whether sample s takes part.  With one observation table (kSets false) every sample does.  With observation sets
// (dvh_lm_normal_sets) t.obs and t.sigma are the rows of the model's set and a sample is present iff its observation
// is finite: NaN marks it absent, and nothing else of an absent sample is read.
template <bool kSets>
DVH_HD bool present(const Table& t, int s) {
  return !kSets || is_finite(t.obs[s]);
}
DVH_HD bool sigma_ok(double sigma) { return sigma > 0.0 && is_finite(sigma); }  // asked of a set's present samples

// The set's rows of set_obs and set_sigma [n_set][n_sample] in t, or false for a set outside 0 .. n_set - 1.
DVH_HD bool select_set(Table& t, int set, int n_set) {
  if (set < 0 || set >= n_set) return false;
  t.obs += (int64_t)set * t.n_sample;
  t.sigma += (int64_t)set * t.n_sample;
  return true;
}

DVH_HD double residual(const Table& t, const double* cm, int s) {
  return (cm[slot_of(t, s)] - t.obs[s]) / t.sigma[s];
}

DVH_HD double rms_of(double sum_of_squares, int n) { return sqrt(sum_of_squares / (double)n); }

// rho_i and n_i of curve i: the mean over its present samples in table order.  All of them must have a slot.
template <bool kSets>
DVH_HD void curve_rms(const Table& t, const double* cm, int i, double& rho, int& n) {
  double acc = 0.0;
  n = 0;
  for (int s = 0; s < t.n_sample; ++s) {
    if (!present<kSets>(t, s) || t.curve[s] != i) continue;
    const double r = residual(t, cm, s);
    acc += r * r;
    ++n;
  }
  rho = rms_of(acc, n);
}

// f = sum_i w_i rho_i / W and W, over the curves with a sample (n_i > 0) in order.  One observation table flags a
// model that has a curve without a sample before it comes here; a set leaves such a curve out of both sums.
DVH_HD double misfit_of(const double* w, const double* rho, const int* count, int n_curve, double& W) {
  double num = 0.0;
  W = 0.0;
  for (int i = 0; i < n_curve; ++i) {
    if (count[i] == 0) continue;
    num += w[i] * rho[i];
    W += w[i];
  }
  return num / W;
}

DVH_HD double curve_factor(double w, double W, int n, double rho, double rho_floor) {
  return w / (W * (double)n * fmax(rho, rho_floor));
}

// j_s[k]: row is dcdp's [4 n_layer] values at the sample's slot, chain is [4 n_layer][D].
DVH_HD double jacobian_entry(const double* row, const double* chain, int n_value, int D, int k, double sigma) {
  double acc = 0.0;
  for (int r = 0; r < n_value; ++r) acc += row[r] * chain[(int64_t)r * D + k];
  return acc / sigma;
}

// One sample's term of g_k (w = a r) and of H_kl (w = a).
DVH_HD double add_g(double acc, double w, double jk) { return acc + w * jk; }
DVH_HD double add_h(double acc, double w, double jk, double jl) { return acc + (w * jk) * jl; }

// Pair p of the lower triangle in row order: p = k (k + 1) / 2 + l, l <= k.
DVH_HD void pair_of(int p, int& k, int& l) {
  k = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while (k * (k + 1) / 2 > p) --k;
  while ((k + 1) * (k + 2) / 2 <= p) ++k;
  l = p - k * (k + 1) / 2;
}
DVH_HD int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

// d_k = max(H_kk, 1e-12 max_j H_jj) over the free parameters; the damped diagonal is H_kk + lambda d_k.
DVH_HD double damped_diagonal(double hkk, double hmax, double lambda) {
  return hkk + lambda * fmax(hkk, 1e-12 * hmax);
}

// The steps of the Cholesky solve on the packed lower triangle L (row order) and the right-hand side y.  Entry (i, j)
// takes its products in the order k = 0 .. j - 1; the solves subtract column by column, which is that same order for
// every entry of y.
DVH_HD double chol_reduce(const double* L, int i, int j) {
  double v = L[tri(i, j)];
  for (int k = 0; k < j; ++k) v -= L[tri(i, k)] * L[tri(j, k)];
  return v;
}
DVH_HD bool pivot_ok(double v) { return v > 0.0 && is_finite(v); }

// ---- chains of models (dvh_lm_solve_chain; DESIGN.md, "Laterally constrained refinement") ----
// Position k of a chain has the diagonal block A_k and, towards k + 1, the block B_k = -w_k diag(mu).  The block
// Cholesky keeps per position the packed lower triangle L_k and X_k = B_k L_k^-T, which is upper triangular and is
// packed as its transpose U: U[tri(p, i)] = X_k[i][p], i <= p.  Every sum below runs in index order in one thread.

// q_k[d] = mu_d [ w_{k-1} (u_k - u_{k-1}) - w_k (u_{k+1} - u_k) ], a term that has no neighbour left out.
DVH_HD double coupling_gradient(double mu, bool has_left, double w_left, double u_left, bool has_right, double w_right,
                                double u_right, double u_here) {
  double t = 0.0;
  if (has_left) t += w_left * (u_here - u_left);
  if (has_right) t -= w_right * (u_right - u_here);
  return mu * t;
}
// A_k's diagonal entry from dvh_lm_solve's damped one; a link that does not exist is passed as 0.
DVH_HD double coupled_diagonal(double damped, double w_left, double w_right, double mu) {
  return damped + (w_left + w_right) * mu;
}
DVH_HD double link_entry(double w, double mu) { return -(w * mu); }  // B_k's diagonal
DVH_HD double chain_rhs(double g, double q) { return 0.0 - (g + q); }

// (i, j), j <= i, of S_k = A_k - X_{k-1} X_{k-1}^T from v = A_k's entry and U of position k - 1.
DVH_HD double schur_reduce(double v, const double* U, int i, int j, int n) {
  for (int p = i; p < n; ++p) v -= U[tri(p, i)] * U[tri(p, j)];
  return v;
}
// Entry i of r_k - X_{k-1} y_{k-1}.
DVH_HD double carry_forward(double r, const double* U, const double* y_before, int i, int n) {
  for (int p = i; p < n; ++p) r -= U[tri(p, i)] * y_before[p];
  return r;
}
// Row i of X_k L_k^T = B_k by substitution along the row, b = B_k's entry (i, i); written into U.
DVH_HD void link_row(const double* L, double* U, int i, int n, double b) {
  U[tri(i, i)] = b / L[tri(i, i)];
  for (int j = i + 1; j < n; ++j) {
    double s = 0.0;
    for (int p = i; p < j; ++p) s -= U[tri(p, i)] * L[tri(j, p)];
    U[tri(j, i)] = s / L[tri(j, j)];
  }
}
// Entry p of y_k - X_k^T delta_{k+1}.
DVH_HD double carry_back(double t, const double* U, const double* delta_after, int p) {
  for (int i = 0; i <= p; ++i) t -= U[tri(p, i)] * delta_after[i];
  return t;
}

}  // namespace refine
}  // namespace dvh
