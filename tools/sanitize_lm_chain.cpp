// A stand-alone host program around dvh_lm_solve_chain_host for AddressSanitizer and UBSan (CPU only; no device is
// touched).  Three chains of 7 positions at D = 95 under a mixed free mask: a healthy one, one with a gap (H = 0,
// g = 0) in the middle, and one with an indefinite block, in exactly sized heap buffers.
//
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I das_diff_veh_amd/csrc -I include \
//       tools/sanitize_lm_chain.cpp das_diff_veh_amd/csrc/dvh_refine_chain.hip das_diff_veh_amd/csrc/dvh_common.cpp \
//       -o build/sanitize_lm_chain && build/sanitize_lm_chain
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "dvh.h"

int main() {
  const int C = 3, L = 7, D = 95, M = C * L;
  uint64_t state = 88172645463325252ull;
  auto uniform = [&state]() {  // xorshift64, in 0 .. 1
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  std::vector<double> H((size_t)M * D * D), g((size_t)M * D), u((size_t)M * D), lambda(C, 1e-3), mu(D);
  std::vector<double> link((size_t)C * (L - 1)), delta((size_t)M * D, -1.0), B((size_t)D * D);
  std::vector<int32_t> free_mask(D), status(C, -7);
  for (int k = 0; k < D; ++k) {
    free_mask[k] = k % 5 != 3;
    mu[k] = k % 4 == 1 ? 0.0 : 0.1 + 0.4 * uniform();
  }
  for (auto& w : link) w = 0.5 + 1.5 * uniform();
  for (int m = 0; m < M; ++m) {
    for (auto& b : B) b = uniform() - 0.5;
    double* Hm = H.data() + (size_t)m * D * D;
    for (int i = 0; i < D; ++i)
      for (int j = 0; j <= i; ++j) {
        double acc = i == j ? 0.05 : 0.0;
        for (int r = 0; r < D; ++r) acc += B[(size_t)i * D + r] * B[(size_t)j * D + r];
        Hm[(size_t)i * D + j] = Hm[(size_t)j * D + i] = acc;
      }
    for (int k = 0; k < D; ++k) {
      g[(size_t)m * D + k] = uniform() - 0.5;
      u[(size_t)m * D + k] = uniform();
    }
  }
  const int gap = 1 * L + 3, broken = 2 * L + 5;
  for (int e = 0; e < D * D; ++e) H[(size_t)gap * D * D + e] = 0.0;
  for (int k = 0; k < D; ++k) {
    g[(size_t)gap * D + k] = 0.0;
    if (free_mask[k] && mu[k] == 0.0) mu[k] = 0.2;  // a gap is carried only by coupled parameters
  }
  H[(size_t)broken * D * D] = -100.0;
  const int64_t bytes = dvh_lm_solve_chain_workspace(M, D);
  std::vector<double> work((size_t)bytes / sizeof(double));
  const int rc = dvh_lm_solve_chain_host(H.data(), g.data(), u.data(), lambda.data(), free_mask.data(), mu.data(),
                                         link.data(), C, L, D, work.data(), delta.data(), status.data());
  bool ok = rc == 0 && status[0] == 0 && status[1] == 0 && status[2] == 2;
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < D; ++k) {
      const double d = delta[(size_t)m * D + k];
      ok = ok && isfinite(d) && (free_mask[k] || d == 0.0) && (m < 2 * L || d == 0.0);
    }
  // one position, and an empty batch
  const int rc1 = dvh_lm_solve_chain_host(H.data(), g.data(), u.data(), lambda.data(), free_mask.data(), mu.data(),
                                          link.data(), 1, 1, D, work.data(), delta.data(), status.data());
  const int rc0 = dvh_lm_solve_chain_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, L, D,
                                          nullptr, nullptr, nullptr);
  ok = ok && rc1 == 0 && status[0] == 0 && rc0 == 0;
  printf("rc %d %d %d: %s\n", rc, rc1, rc0, ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}
