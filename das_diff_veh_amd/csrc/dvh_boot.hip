// Bootstrap / convergence resampling on MI355X (gfx950): SURVEY §8(f) row 1.
//
// Replaces, for all resamples of a bootstrap run at once:
//   bootstrap_disp                 apis/imaging_classes.py:8-48 (per resample: VSG stack of
//                                  random.sample(range(1, n), bt_size) windows, compute_disp_image,
//                                  extract_ridge_ref_idx per mode)
//   extract_ridge_ref_idx          modules/utils.py:621-678
// The per-pass gathers are computed once (dvh_vsg_gathers); a resample's stack is the mean of its
// selected gathers (select_mean_kernel); the f-v images of all resamples run through the batched
// dispersion kernels (dvh_disp_*); ridge_kernel walks every (resample, mode) ridge in one wave.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "dvh_common.h"
#include "dvh.h"
#include "ridge_walk.h"

namespace dvh {

// out[b][k] = (sum_{j < m} G[sel[b][j]][k]) / m over the contiguous K-element block of each pass,
// summed in selection order (the reference's sum(images) / len(images); sum() takes the first image as it is,
// VirtualShotGather.__radd__, so the accumulator starts at -0: a +0 start would turn a -0 of it into +0).
// float4 per lane; the loads of 8 selections are issued before their adds (in order), so a lane keeps 8 gathers'
// reads in flight.
__device__ __forceinline__ void select_mean_one(const float* __restrict__ G, int64_t pass_stride, int64_t K,
                                                const int32_t* __restrict__ s, int32_t m, float* __restrict__ o,
                                                bool vec) {
  if (vec) {
    const int64_t k4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * k4 >= K) return;
    float4 acc = make_float4(-0.f, -0.f, -0.f, -0.f);  // -0 + x == x for every x: the sum starts AT the first pass
    int j = 0;
    for (; j + 8 <= m; j += 8) {
      float4 g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) g[u] = reinterpret_cast<const float4*>(G + (int64_t)s[j + u] * pass_stride)[k4];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc.x += g[u].x;
        acc.y += g[u].y;
        acc.z += g[u].z;
        acc.w += g[u].w;
      }
    }
    for (; j < m; ++j) {
      const float4 g = reinterpret_cast<const float4*>(G + (int64_t)s[j] * pass_stride)[k4];
      acc.x += g.x;
      acc.y += g.y;
      acc.z += g.z;
      acc.w += g.w;
    }
    // divide (not multiply by 1/m): sum / len as the reference evaluates it
    reinterpret_cast<float4*>(o)[k4] = make_float4(acc.x / (float)m, acc.y / (float)m, acc.z / (float)m, acc.w / (float)m);
  } else {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x) {
      float acc = -0.f;
      for (int j = 0; j < m; ++j) acc += G[(int64_t)s[j] * pass_stride + k];
      o[k] = acc / (float)m;
    }
  }
}

__device__ __forceinline__ bool select_vec(const float* G, int64_t pass_stride, int64_t K, const float* out,
                                           int64_t out_stride) {
  return (K % 4 == 0) && (pass_stride % 4 == 0) && (out_stride % 4 == 0) &&
         ((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(out)) % 16 == 0);
}

__global__ __launch_bounds__(256) void select_mean_kernel(const float* __restrict__ G, int64_t pass_stride, int64_t K,
                                                          const int32_t* __restrict__ sel, int32_t m,
                                                          float* __restrict__ out, int64_t out_stride) {
  const int b = blockIdx.y;
  select_mean_one(G, pass_stride, K, sel + (int64_t)b * m, m, out + (int64_t)b * out_stride, select_vec(G, pass_stride,
                  K, out, out_stride));
}

// The same for resamples of different sizes in one launch: resample b takes cnt[b] selections from sel + off[b]
// (convergence_test's bt_size = 1 .. 60 x 30 draws: one launch of 1 800 resamples instead of 60 of 30).
__global__ __launch_bounds__(256) void select_mean_var_kernel(const float* __restrict__ G, int64_t pass_stride,
                                                              int64_t K, const int32_t* __restrict__ sel,
                                                              const int32_t* __restrict__ off,
                                                              const int32_t* __restrict__ cnt, float* __restrict__ out,
                                                              int64_t out_stride) {
  const int b = blockIdx.y;
  select_mean_one(G, pass_stride, K, sel + off[b], cnt[b], out + (int64_t)b * out_stride,
                  select_vec(G, pass_stride, K, out, out_stride));
}

// argmax of column c over rows [r0, r1) (first max wins); -1 when the range is empty
__device__ __forceinline__ int column_argmax(const float* __restrict__ F, int nF, int c, int r0, int r1, int lane) {
  float best = 0.f;
  int row = -1;
  for (int r = r0 + lane; r < r1; r += 64) {
    const float v = F[(int64_t)r * nF + c];
    if (row < 0 || better(v, r, best, row)) {
      best = v;
      row = r;
    }
  }
  wave_argmax(best, row);
  return row;
}

// The columns of a stored image fv[b] ([nV][nF]) for ridge_walk: band column i is image column c0 + i.
struct ImageColumns {
  const float* F;
  int nF, c0, lane;
  __device__ __forceinline__ void first(int) {}
  __device__ __forceinline__ int argmax(int i, int, int r0, int r1) { return column_argmax(F, nF, c0 + i, r0, r1, lane); }
};

// One wave per (image b, ridge):  extract_ridge_ref_idx (modules/utils.py:621-678) on the band of
// columns [c0, c0 + nb) of fv[b] ([nV][nF], rows = velocities in descending order vel[r]); the modes and the walk
// are ridge_walk's (ridge_walk.h).
__global__ __launch_bounds__(64) void ridge_kernel(const float* __restrict__ fv, int64_t b_stride, int32_t nV,
                                                   int32_t nF, int32_t c0, int32_t nb, const double* __restrict__ vel,
                                                   int32_t ref, double sigma, double vel_max,
                                                   const double* __restrict__ vref, const double* __restrict__ sg,
                                                   int32_t sgl, double* __restrict__ out, int32_t* __restrict__ status,
                                                   double* __restrict__ picks) {
  __shared__ double pick[kMaxBand];
  const int b = blockIdx.x, lane = threadIdx.x;
  ImageColumns src{fv + (int64_t)b * b_stride, nF, c0, lane};
  ridge_walk(src, b, lane, nV, nb, vel, ref, sigma, vel_max, vref, sg, sgl, out, status, picks, pick);
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_select_mean(const float* G, int64_t pass_stride, int64_t K, const int32_t* sel, int32_t B, int32_t m,
                            float* out, int64_t out_stride, void* stream) {
  if (!G || !sel || !out) return set_error(-2, "null pointer argument");
  if (m <= 0 || K < 0 || B < 0) return set_error(-2, "invalid sizes");
  if (B == 0 || K == 0) return 0;
  if (B > 65535) return set_error(-4, "too many resamples for one launch");
  const int64_t blocks = (K / 4 + 255) / 256 + 1;
  hipLaunchKernelGGL(select_mean_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, G, pass_stride,
                     K, sel, m, out, out_stride);
  return last_launch();
}

DVH_API int dvh_select_mean_var(const float* G, int64_t pass_stride, int64_t K, const int32_t* sel, const int32_t* off,
                                const int32_t* cnt, int32_t B, float* out, int64_t out_stride, void* stream) {
  if (!G || !sel || !off || !cnt || !out) return set_error(-2, "null pointer argument");
  if (K < 0 || B < 0) return set_error(-2, "invalid sizes");
  if (B == 0 || K == 0) return 0;
  if (B > 65535) return set_error(-4, "too many resamples for one launch");
  const int64_t blocks = (K / 4 + 255) / 256 + 1;
  hipLaunchKernelGGL(select_mean_var_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, G,
                     pass_stride, K, sel, off, cnt, out, out_stride);
  return last_launch();
}

DVH_API int dvh_ridge(const float* fv, int64_t b_stride, int32_t B, int32_t nV, int32_t nF, int32_t c0, int32_t nb,
                      const double* vel, int32_t ref, double sigma, double vel_max, const double* vref,
                      const double* sg, int32_t sgl, double* out, int32_t* status, double* picks, void* stream) {
  if (!fv || !vel || !out || !status) return set_error(-2, "null pointer argument");
  if (nb <= 0 || c0 < 0 || c0 + nb > nF || nV <= 0) return set_error(-2, "invalid band");
  if (nb > kMaxBand) return set_error(-4, "band longer than 1024 frequencies");
  if (ref != INT32_MIN || vref) {
    if (!sg || sgl % 2 == 0 || sgl > nb) return set_error(-4, "savgol window must be odd and <= the band length");
    if (ref >= nb || ref < -nb) return set_error(-2, "reference index outside the band");
  }
  if (B <= 0) return 0;
  hipLaunchKernelGGL(ridge_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, fv, b_stride, nV, nF, c0, nb, vel,
                     ref, sigma, vel_max, vref, sg, sgl, out, status, picks);
  return last_launch();
}
