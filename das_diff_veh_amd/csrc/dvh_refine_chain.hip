// The damped Gauss-Newton step of chains of models tied by first differences ("Laterally constrained
// refinement"):
//   dvh_lm_solve_chain       per chain the block-tridiagonal system with diagonal blocks
//                            A_k = H_k + lambda diag(d_k) + (w_{k-1} + w_k) diag(mu) and off-diagonal blocks
//                            B_k = -w_k diag(mu), right-hand side -(g_k + q_k), by a float64 block Cholesky walked
//                            along the chain.  One workgroup per chain; the factors of a position are in LDS while it is
//                            worked on and in the caller's workspace for the back sweep.
//   dvh_lm_solve_chain_host  the same header (refine.h) on the CPU over host memory, in the same order.
// With one position, or with mu or the links all 0, a row's step is dvh_lm_solve's bit for bit.
#include <math.h>

#include "dvh_common.h"
#include "dvh.h"
#include "refine.h"

namespace {
using dvh::set_error;
namespace lm = dvh::refine;

constexpr int kThreads = 256;
constexpr int kMaxPairs = lm::kMaxParams * (lm::kMaxParams + 1) / 2;  // 4656

struct ChainArgs {
  const double* H;
  const double* g;
  const double* u;
  const double* lambda;
  const int32_t* free_mask;
  const double* mu;
  const double* link;
  int chain_len, n_param;
  double* work;  // [n_model][2][n_param (n_param + 1) / 2]: L_k, then U_k
  double* out_delta;
  int32_t* out_status;
};

DVH_HD int64_t pairs_of(int n_param) { return (int64_t)n_param * (n_param + 1) / 2; }

// The links of position k of chain c: whether it has a neighbour on either side, and the weights (0 where it has none).
struct Links {
  bool has_left, has_right;
  double w_left, w_right;
};
DVH_HD Links links_of(const double* link, int64_t chain, int len, int k) {
  Links l;
  l.has_left = k > 0;
  l.has_right = k + 1 < len;
  const double* w = link + chain * (len - 1);
  l.w_left = l.has_left ? w[k - 1] : 0.0;
  l.w_right = l.has_right ? w[k] : 0.0;
  return l;
}

// A stretch of positions between two cut links (w = 0) or chain ends that has no positive H_kk anywhere holds nothing
// but the coupling, which is singular (a common shift costs nothing): its last pivot is 0 up to rounding, so it is
// refused by this rule and not by the sign of a rounding error.  Position k closes the stretch before it when its
// left link is cut.  With one position this is dvh_lm_solve's own refusal (no positive d_k, no positive pivot).
struct Stretch {
  bool has_data = false;
};
DVH_HD bool stretch_ok(Stretch& s, const Links& l, double hmax) {  // false: the stretch that ends before k is empty
  const bool closes = l.has_left && !(l.w_left > 0.0);
  const bool ok = !closes || s.has_data;
  if (closes) s.has_data = false;
  s.has_data = s.has_data || hmax > 0.0;
  return ok;
}

// Entry (i, j) of S_k before its factorisation, from H of the position (row stride D) and U of the position before.
DVH_HD double block_entry(const double* H, int D, const int* idx, int i, int j, double hmax, double lam, const Links& l,
                          const double* mu, const double* U, int n) {
  double v = H[(int64_t)idx[i] * D + idx[j]];
  if (i == j) {
    v = lm::damped_diagonal(v, hmax, lam);
    if (l.has_left || l.has_right) v = lm::coupled_diagonal(v, l.w_left, l.w_right, mu[idx[i]]);
  }
  return l.has_left ? lm::schur_reduce(v, U, i, j, n) : v;
}

// Entry i of r_k - X_{k-1} y_{k-1}; u is the row of the position, D apart from its neighbours'.
DVH_HD double rhs_entry(const double* g, const double* u, int D, const int* idx, int i, const Links& l,
                        const double* mu, const double* U, const double* y_before, int n) {
  const int k = idx[i];
  if (!l.has_left && !l.has_right) return 0.0 - g[k];
  const double q = lm::coupling_gradient(mu[k], l.has_left, l.w_left, l.has_left ? u[k - D] : 0.0, l.has_right,
                                         l.w_right, l.has_right ? u[k + D] : 0.0, u[k]);
  const double r = lm::chain_rhs(g[k], q);
  return l.has_left ? lm::carry_forward(r, U, y_before, i, n) : r;
}

__global__ __launch_bounds__(kThreads) void lm_solve_chain_kernel(ChainArgs a) {
  __shared__ double L[kMaxPairs], U[kMaxPairs];
  __shared__ double y[lm::kMaxParams], y_before[lm::kMaxParams], after[lm::kMaxParams], step[lm::kMaxParams];
  __shared__ double diag[lm::kMaxParams];
  __shared__ int idx[lm::kMaxParams];
  __shared__ int n_free, failed;
  __shared__ double hmax_s;
  const int tid = threadIdx.x, D = a.n_param, len = a.chain_len;
  const int64_t chain = blockIdx.x, first = chain * len, P = pairs_of(D);
  if (tid == 0) {  // the free parameters in order
    int n = 0;
    for (int k = 0; k < D; ++k)
      if (a.free_mask[k] != 0) idx[n++] = k;
    n_free = n;
    failed = n == 0;
  }
  __syncthreads();
  const int n = n_free, n_pair = n * (n + 1) / 2;
  const double lam = a.lambda[chain];
  // forward along the chain: S_k, its factor, y_k, X_k
  Stretch stretch;
  bool empty = false;
  for (int k = 0; k < len && !failed; ++k) {  // failed is block-uniform here: read after a barrier
    const int64_t m = first + k;
    const double* H = a.H + m * D * D;
    const Links l = links_of(a.link, chain, len, k);
    for (int i = tid; i < n; i += kThreads) diag[i] = H[(int64_t)idx[i] * D + idx[i]];
    __syncthreads();
    if (tid == 0) {
      double hmax = -INFINITY;
      for (int i = 0; i < n; ++i) hmax = fmax(hmax, diag[i]);
      hmax_s = hmax;
    }
    __syncthreads();
    const double hmax = hmax_s;
    if (!stretch_ok(stretch, l, hmax)) {  // block-uniform: every thread sees the same links and hmax
      empty = true;
      break;
    }
    for (int p = tid; p < n_pair; p += kThreads) {
      int i, j;
      lm::pair_of(p, i, j);
      L[p] = block_entry(H, D, idx, i, j, hmax, lam, l, a.mu, U, n);
    }
    for (int i = tid; i < n; i += kThreads)
      y[i] = rhs_entry(a.g + m * D, a.u + m * D, D, idx, i, l, a.mu, U, y_before, n);
    __syncthreads();
    // factorisation, a column a step, as lm_solve_kernel's
    for (int j = 0; j < n; ++j) {
      const int i = j + tid;
      const double v = i < n ? lm::chol_reduce(L, i, j) : 0.0;
      if (tid == 0) {
        if (!lm::pivot_ok(v)) failed = 1;
        L[lm::tri(j, j)] = sqrt(v);
      }
      __syncthreads();
      if (failed) break;  // block-uniform
      const double d = L[lm::tri(j, j)];
      if (i > j && i < n) L[lm::tri(i, j)] = v / d;
      __syncthreads();
    }
    if (failed) break;             // block-uniform: nobody writes it between the barrier above and here
    for (int j = 0; j < n; ++j) {  // L_k y_k = r_k - X_{k-1} y_{k-1}
      if (tid == 0) y[j] = y[j] / L[lm::tri(j, j)];
      __syncthreads();
      const double z = y[j];
      for (int i = j + 1 + tid; i < n; i += kThreads) y[i] -= L[lm::tri(i, j)] * z;
      __syncthreads();
    }
    if (l.has_right)  // U_{k-1} has been consumed above
      for (int i = tid; i < n; i += kThreads) lm::link_row(L, U, i, n, lm::link_entry(l.w_right, a.mu[idx[i]]));
    __syncthreads();
    double* work = a.work + m * 2 * P;
    for (int p = tid; p < n_pair; p += kThreads) {
      work[p] = L[p];
      if (l.has_right) work[P + p] = U[p];
    }
    for (int i = tid; i < n; i += kThreads) {
      y_before[i] = y[i];
      a.out_delta[m * D + i] = y[i];  // y_k waits in its row for the back sweep
    }
    __syncthreads();
  }
  __syncthreads();
  if (empty || !stretch.has_data) failed = 1;  // block-uniform, and every writer stores the same value
  __syncthreads();
  // back along the chain: delta_k = L_k^-T (y_k - X_k^T delta_{k+1})
  if (!failed) {
    for (int k = len - 1; k >= 0; --k) {
      const int64_t m = first + k;
      const double* work = a.work + m * 2 * P;
      double* delta = a.out_delta + m * D;
      for (int p = tid; p < n_pair; p += kThreads) L[p] = work[p];
      for (int i = tid; i < n; i += kThreads) {
        const double t = delta[i];
        y[i] = k + 1 < len ? lm::carry_back(t, work + P, after, i) : t;
      }
      __syncthreads();
      for (int j = n - 1; j >= 0; --j) {
        if (tid == 0) y[j] = y[j] / L[lm::tri(j, j)];
        __syncthreads();
        const double x = y[j];
        for (int i = tid; i < j; i += kThreads) y[i] -= L[lm::tri(j, i)] * x;
        __syncthreads();
      }
      for (int i = tid; i < n; i += kThreads) {
        if (!lm::is_finite(y[i])) failed = 1;  // every writer stores the same value
        after[i] = y[i];
      }
      for (int e = tid; e < D; e += kThreads) step[e] = 0.0;  // fixed parameters
      __syncthreads();
      for (int i = tid; i < n; i += kThreads) step[idx[i]] = y[i];
      __syncthreads();
      for (int e = tid; e < D; e += kThreads) delta[e] = step[e];
      __syncthreads();
    }
  }
  __syncthreads();
  if (failed)  // block-uniform: the whole chain stays where it is
    for (int64_t e = tid; e < (int64_t)len * D; e += kThreads) a.out_delta[first * D + e] = 0.0;
  if (tid == 0) a.out_status[chain] = failed ? 2 : 0;
}

int check_chain(const void* H, const void* g, const void* u, const void* lambda, const void* free_mask, const void* mu,
                const void* link, int32_t n_chain, int32_t chain_len, int32_t n_param, const void* workspace,
                const void* out_delta, const void* out_status) {
  if (n_chain < 0 || chain_len < 1 || n_param < 1) return set_error(-2, "negative or empty count");
  if (n_param > lm::kMaxParams) return set_error(-4, "more than 96 parameters");
  if (n_chain == 0) return 1;
  if ((int64_t)n_chain * chain_len > INT32_MAX) return set_error(-2, "more than 2^31 - 1 models");
  if (!H || !g || !u || !lambda || !free_mask || !mu || !link || !workspace || !out_delta || !out_status)
    return set_error(-2, "null pointer argument");
  return 0;
}

}  // namespace

DVH_API int64_t dvh_lm_solve_chain_workspace(int32_t n_model, int32_t n_param) {
  if (n_model < 0 || n_param < 1 || n_param > lm::kMaxParams) return 0;
  return (int64_t)n_model * 2 * pairs_of(n_param) * (int64_t)sizeof(double);
}

DVH_API int dvh_lm_solve_chain(const double* H, const double* g, const double* u, const double* lambda,
                               const int32_t* free_mask, const double* mu, const double* link, int32_t n_chain,
                               int32_t chain_len, int32_t n_param, void* workspace, double* out_delta,
                               int32_t* out_status, void* stream) {
  const int rc = check_chain(H, g, u, lambda, free_mask, mu, link, n_chain, chain_len, n_param, workspace, out_delta,
                             out_status);
  if (rc) return rc < 0 ? rc : 0;
  ChainArgs a{H, g, u, lambda, free_mask, mu, link, chain_len, n_param, (double*)workspace, out_delta, out_status};
  lm_solve_chain_kernel<<<dim3((unsigned)n_chain), dim3(kThreads), 0, (hipStream_t)stream>>>(a);
  return dvh::last_launch();
}

DVH_API int dvh_lm_solve_chain_host(const double* H_all, const double* g_all, const double* u_all,
                                    const double* lambda, const int32_t* free_mask, const double* mu,
                                    const double* link, int32_t n_chain, int32_t chain_len, int32_t n_param,
                                    void* workspace, double* out_delta, int32_t* out_status) {
  const int rc = check_chain(H_all, g_all, u_all, lambda, free_mask, mu, link, n_chain, chain_len, n_param, workspace,
                             out_delta, out_status);
  if (rc) return rc < 0 ? rc : 0;
  const int D = n_param, len = chain_len;
  const int64_t P = pairs_of(D);
  static thread_local double U[kMaxPairs];
  double y[lm::kMaxParams], y_before[lm::kMaxParams], after[lm::kMaxParams], v[lm::kMaxParams];
  int idx[lm::kMaxParams];
  int n = 0;
  for (int k = 0; k < D; ++k)
    if (free_mask[k] != 0) idx[n++] = k;
  for (int64_t chain = 0; chain < n_chain; ++chain) {
    const int64_t first = chain * len;
    bool failed = n == 0;
    Stretch stretch;
    for (int k = 0; k < len && !failed; ++k) {
      const int64_t m = first + k;
      const double* H = H_all + m * D * D;
      double* L = (double*)workspace + m * 2 * P;
      const Links l = links_of(link, chain, len, k);
      double hmax = -INFINITY;
      for (int i = 0; i < n; ++i) hmax = fmax(hmax, H[(int64_t)idx[i] * D + idx[i]]);
      failed = !stretch_ok(stretch, l, hmax);
      if (failed) break;
      for (int i = 0; i < n; ++i) {
        for (int j = 0; j <= i; ++j)
          L[lm::tri(i, j)] = block_entry(H, D, idx, i, j, hmax, lambda[chain], l, mu, U, n);
        y[i] = rhs_entry(g_all + m * D, u_all + m * D, D, idx, i, l, mu, U, y_before, n);
      }
      for (int j = 0; j < n && !failed; ++j) {
        for (int i = j; i < n; ++i) v[i] = lm::chol_reduce(L, i, j);
        failed = !lm::pivot_ok(v[j]);
        if (failed) break;
        const double d = L[lm::tri(j, j)] = sqrt(v[j]);
        for (int i = j + 1; i < n; ++i) L[lm::tri(i, j)] = v[i] / d;
      }
      if (failed) break;
      for (int j = 0; j < n; ++j) {
        const double z = y[j] = y[j] / L[lm::tri(j, j)];
        for (int i = j + 1; i < n; ++i) y[i] -= L[lm::tri(i, j)] * z;
      }
      if (l.has_right) {
        for (int i = 0; i < n; ++i) lm::link_row(L, U, i, n, lm::link_entry(l.w_right, mu[idx[i]]));
        for (int p = 0; p < n * (n + 1) / 2; ++p) L[P + p] = U[p];
      }
      for (int i = 0; i < n; ++i) out_delta[m * D + i] = y_before[i] = y[i];
    }
    failed = failed || !stretch.has_data;
    for (int k = len - 1; k >= 0 && !failed; --k) {
      const int64_t m = first + k;
      const double* L = (const double*)workspace + m * 2 * P;
      double* delta = out_delta + m * D;
      for (int i = 0; i < n; ++i) y[i] = k + 1 < len ? lm::carry_back(delta[i], L + P, after, i) : delta[i];
      for (int j = n - 1; j >= 0; --j) {
        const double x = y[j] = y[j] / L[lm::tri(j, j)];
        for (int i = 0; i < j; ++i) y[i] -= L[lm::tri(j, i)] * x;
      }
      for (int i = 0; i < n; ++i) after[i] = y[i];
      for (int e = 0; e < D; ++e) delta[e] = 0.0;
      for (int i = n - 1; i >= 0; --i) delta[idx[i]] = y[i];
    }
    for (int64_t e = 0; e < (int64_t)len * D && !failed; ++e) failed = !lm::is_finite(out_delta[first * D + e]);
    if (failed)
      for (int64_t e = 0; e < (int64_t)len * D; ++e) out_delta[first * D + e] = 0.0;
    out_status[chain] = failed ? 2 : 0;
  }
  return 0;
}
