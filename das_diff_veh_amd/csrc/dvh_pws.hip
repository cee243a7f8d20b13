// Phase-weighted stacking of cached gathers on MI355X (gfx950): DESIGN.md, "Phase-weighted stack" (Schimmel &
// Paulssen 1997).
//
//   dvh_hilbert_rows        the imaginary part of every row's analytic signal, once per gather cache: one workgroup per
//                           row, the row and its tap table as float64 in LDS, a direct O(N^2) circular convolution
//                           (499 is prime: no transform of the build fits it)
//   dvh_select_pws          dvh_select_mean_var's draws, each stacked as lin * c^power: per read one g and one h, the
//                           phasor formed in registers, three sums in selection order
//   dvh_hilbert_rows_host, dvh_select_pws_host   the same header (pws.h) on the CPU over host memory
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <vector>

#include "dvh_common.h"
#include "dvh.h"
#include "pws.h"

namespace dvh {

// Row r of X -> row r of H.  N = row_len[r] (W without a table), clamped to [0, W]; lags N <= t < W are written 0.
// LDS: x and k, 8 KB each.  The inner loop reads k[n] at one address for the whole wave (a broadcast) and x at
// consecutive float64 for consecutive lanes, wrapped once: no bank conflict either way.
__global__ __launch_bounds__(256) void hilbert_rows_kernel(const float* __restrict__ X, int64_t row_stride, int32_t W,
                                                           const int32_t* __restrict__ row_len, float* __restrict__ H) {
  __shared__ double x[pws::kMaxLen];
  __shared__ double k[pws::kMaxLen];
  const int64_t base = (int64_t)blockIdx.x * row_stride;
  int N = row_len ? row_len[blockIdx.x] : W;
  N = N < 0 ? 0 : (N > W ? W : N);
  int bad = 0;
  for (int t = threadIdx.x; t < N; t += blockDim.x) {
    x[t] = (double)X[base + t];
    k[t] = pws::hilbert_tap(t, N);
    bad |= !pws::is_finite(x[t]);
  }
  const bool all_finite = !__syncthreads_or(bad);  // N is uniform over the block: every thread arrives
  for (int t = threadIdx.x; t < W; t += blockDim.x) H[base + t] = t < N ? pws::hilbert_at(x, k, N, t, all_finite) : 0.f;
}

// select_vec of dvh_boot.hip with H beside G: the float4 path needs every base 16-byte aligned and every stride and K a
// multiple of 4 floats.
__device__ __forceinline__ bool pws_vec(const float* G, const float* H, int64_t pass_stride, int64_t K,
                                        const float* out, int64_t out_stride) {
  return (K % 4 == 0) && (pass_stride % 4 == 0) && (out_stride % 4 == 0) &&
         ((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(H) | reinterpret_cast<uintptr_t>(out)) % 16 == 0);
}

// Resample b = blockIdx.y stacks the cnt[b] passes sel[off[b] ..) over the K-element block of each pass.  float4 per
// lane on the vector path, the g and h loads of 4 selections issued before their adds (in order): 8 reads of 16 bytes in
// flight per lane, as many as select_mean_one keeps.  The scalar path is a grid-stride loop.
__global__ __launch_bounds__(256) void select_pws_kernel(const float* __restrict__ G, const float* __restrict__ H,
                                                         int64_t pass_stride, int64_t K,
                                                         const int32_t* __restrict__ sel,
                                                         const int32_t* __restrict__ off,
                                                         const int32_t* __restrict__ cnt, float power,
                                                         float* __restrict__ out, int64_t out_stride) {
  const int b = blockIdx.y;
  const int32_t* s = sel + off[b];
  const int m = cnt[b];
  float* o = out + (int64_t)b * out_stride;
  if (pws_vec(G, H, pass_stride, K, out, out_stride)) {
    const int64_t k4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * k4 >= K) return;
    pws::Sums a[4] = {pws::start(), pws::start(), pws::start(), pws::start()};
    int j = 0;
    for (; j + 4 <= m; j += 4) {
      float4 g[4], h[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t p = (int64_t)s[j + u] * pass_stride;
        g[u] = reinterpret_cast<const float4*>(G + p)[k4];
        h[u] = reinterpret_cast<const float4*>(H + p)[k4];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        pws::add(a[0], g[u].x, h[u].x);
        pws::add(a[1], g[u].y, h[u].y);
        pws::add(a[2], g[u].z, h[u].z);
        pws::add(a[3], g[u].w, h[u].w);
      }
    }
    for (; j < m; ++j) {
      const int64_t p = (int64_t)s[j] * pass_stride;
      const float4 g = reinterpret_cast<const float4*>(G + p)[k4];
      const float4 h = reinterpret_cast<const float4*>(H + p)[k4];
      pws::add(a[0], g.x, h.x);
      pws::add(a[1], g.y, h.y);
      pws::add(a[2], g.z, h.z);
      pws::add(a[3], g.w, h.w);
    }
    reinterpret_cast<float4*>(o)[k4] = make_float4(pws::finish(a[0], m, power), pws::finish(a[1], m, power),
                                                   pws::finish(a[2], m, power), pws::finish(a[3], m, power));
  } else {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x) {
      pws::Sums a = pws::start();
      for (int j = 0; j < m; ++j) {
        const int64_t p = (int64_t)s[j] * pass_stride + k;
        pws::add(a, G[p], H[p]);
      }
      o[k] = pws::finish(a, m, power);
    }
  }
}

static int hilbert_args(const float* X, int64_t row_stride, int32_t n_row, int32_t W, const float* H) {
  if (!X || !H) return set_error(-2, "null pointer argument");
  if (n_row < 0 || W < 0 || row_stride < W) return set_error(-2, "invalid sizes");
  if (W > pws::kMaxLen) return set_error(-4, "row longer than 1024 lags");
  return 0;
}

static int select_args(const float* G, const float* H, int64_t K, const int32_t* sel, const int32_t* off,
                       const int32_t* cnt, int32_t B, float power, const float* out) {
  if (!G || !H || !sel || !off || !cnt || !out) return set_error(-2, "null pointer argument");
  if (K < 0 || B < 0) return set_error(-2, "invalid sizes");
  if (!pws::power_ok(power)) return set_error(-2, "power must be 0 or a finite value of at least 1");
  return 0;
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_hilbert_rows(const float* X, int64_t row_stride, int32_t n_row, int32_t W, const int32_t* row_len,
                             float* H, void* stream) {
  if (const int rc = hilbert_args(X, row_stride, n_row, W, H)) return rc;
  if (n_row == 0 || W == 0) return 0;
  hipLaunchKernelGGL(hilbert_rows_kernel, dim3((unsigned)n_row), dim3(256), 0, (hipStream_t)stream, X, row_stride, W,
                     row_len, H);
  return last_launch();
}

DVH_API int dvh_hilbert_rows_host(const float* X, int64_t row_stride, int32_t n_row, int32_t W, const int32_t* row_len,
                                  float* H) {
  if (const int rc = hilbert_args(X, row_stride, n_row, W, H)) return rc;
  for (int32_t r = 0; row_len && r < n_row; ++r)
    if (row_len[r] < 0 || row_len[r] > W) return set_error(-2, "row length outside [0, W]");
  std::vector<double> x(W > 0 ? W : 1), k(W > 0 ? W : 1);
  for (int32_t r = 0; r < n_row; ++r) {
    const int N = row_len ? row_len[r] : W;
    const int64_t base = (int64_t)r * row_stride;
    bool all_finite = true;
    for (int t = 0; t < N; ++t) {
      x[t] = (double)X[base + t];
      k[t] = pws::hilbert_tap(t, N);
      all_finite = all_finite && pws::is_finite(x[t]);
    }
    for (int t = 0; t < W; ++t) H[base + t] = t < N ? pws::hilbert_at(x.data(), k.data(), N, t, all_finite) : 0.f;
  }
  return 0;
}

DVH_API int dvh_select_pws(const float* G, const float* H, int64_t pass_stride, int64_t K, const int32_t* sel,
                           const int32_t* off, const int32_t* cnt, int32_t B, float power, float* out,
                           int64_t out_stride, void* stream) {
  if (const int rc = select_args(G, H, K, sel, off, cnt, B, power, out)) return rc;
  if (B == 0 || K == 0) return 0;
  if (B > 65535) return set_error(-4, "too many resamples for one launch");
  const int64_t blocks = (K / 4 + 255) / 256 + 1;
  hipLaunchKernelGGL(select_pws_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, G, H, pass_stride,
                     K, sel, off, cnt, power, out, out_stride);
  return last_launch();
}

DVH_API int dvh_select_pws_host(const float* G, const float* H, int64_t pass_stride, int64_t K, const int32_t* sel,
                                const int32_t* off, const int32_t* cnt, int32_t B, float power, float* out,
                                int64_t out_stride) {
  if (const int rc = select_args(G, H, K, sel, off, cnt, B, power, out)) return rc;
  if (B == 0 || K == 0) return 0;
  if (B > 65535) return set_error(-4, "too many resamples for one launch");
  for (int32_t b = 0; b < B; ++b)
    if (cnt[b] < 1) return set_error(-2, "a resample needs at least one pass");
  for (int32_t b = 0; b < B; ++b) {
    const int32_t* s = sel + off[b];
    for (int64_t k = 0; k < K; ++k) {
      pws::Sums a = pws::start();
      for (int j = 0; j < cnt[b]; ++j) {
        const int64_t p = (int64_t)s[j] * pass_stride + k;
        pws::add(a, G[p], H[p]);
      }
      out[(int64_t)b * out_stride + k] = pws::finish(a, cnt[b], power);
    }
  }
  return 0;
}
