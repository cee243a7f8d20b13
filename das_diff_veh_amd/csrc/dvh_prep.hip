// Per-pass windowing and taper, and the record's trace clean-up, on MI355X (gfx950).  (The bandpass is dvh_sos.hip.)
//
//   dvh_mute_traj    SurfaceWaveWindow.mute_along_traj (apis/data_classes.py:49-72): column t is
//                    multiplied by a tukey taper placed along the vehicle trajectory (host tables).
//   dvh_mute_time    SurfaceWaveWindow.mute_along_time (apis/data_classes.py:100-104).
//   dvh_trace_cleanup  the rest of TimeLapseImaging._preprocessing_for_surface_waves
//                    (apis/timeLapseImaging.py:51-71) after the bandpass: find_noise_idx /
//                    impute_noisy_trace (modules/utils.py:316-329) for empty traces (L2 norm below
//                    the threshold) then noisy traces (max above it), then the per-trace L2 norm.
//   dvh_cut_windows  SurfaceWaveSelector.locate_windows' cut of all accepted passes at once.
// Data may be float32 (dtype 0) or float64 (dtype 1), modified in place.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>

#include "dvh_common.h"
#include "dvh.h"

namespace dvh {

// tab[(p * n_t + t) * 3 + {0,1,2}] = {start, end, taper_start}; element (x, t) of pass p is scaled by
// taper[taper_start + x - start] for start <= x < end and zeroed elsewhere.
template <typename T>
__global__ __launch_bounds__(256) void mute_traj_kernel(T* __restrict__ data, int64_t pass_stride, int32_t n_ch,
                                                         int32_t n_t, const int32_t* __restrict__ tab,
                                                         const double* __restrict__ taper) {
  const int p = blockIdx.z;
  const int x = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_t) return;
  const int32_t* e = tab + ((int64_t)p * n_t + t) * 3;
  T* v = data + (int64_t)p * pass_stride + (int64_t)x * n_t + t;
  const int s = e[0], end = e[1];
  if (x >= s && x < end) {
    *v = (T)((double)*v * taper[e[2] + x - s]);
  } else {
    *v = (T)((double)*v * 0.0);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mute_time_kernel(T* __restrict__ data, int64_t n_rows, int32_t n_t,
                                                         const double* __restrict__ taper) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows * n_t) return;
  data[i] = (T)((double)data[i] * taper[i % n_t]);
}

// ---------------------------------------------------------------------------------------------
// Trace clean-up of the continuous record (bandpassed, [n_rows][n_t] with row_stride).

constexpr int kStatBlock = 256;

// NaN-propagating max (np.max returns NaN for a row holding one)
__device__ __forceinline__ double nan_max(double a, double b) { return (isnan(a) || a > b) ? a : b; }

template <typename T>
__device__ __forceinline__ void block_row_stats(const T* __restrict__ row, int32_t n_t, double* __restrict__ out2) {
  __shared__ double ss[kStatBlock / 64], mx[kStatBlock / 64];
  double s = 0.0, m = -INFINITY;
  // 8 loads in flight per thread (one load per iteration left the block waiting out a memory latency per 256 samples:
  // a one-block impute round took 38 us)
  constexpr int U = 8;
  int t = threadIdx.x;
  for (; t + (U - 1) * kStatBlock < n_t; t += U * kStatBlock) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = row[t + u * kStatBlock];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double d = (double)v[u];
      s += d * d;
      m = nan_max(m, d);
    }
  }
  for (; t < n_t; t += kStatBlock) {
    const double v = (double)row[t];
    s += v * v;
    m = nan_max(m, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    m = nan_max(m, __shfl_xor(m, o));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    ss[w] = s;
    mx[w] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = -INFINITY;
    for (int k = 0; k < kStatBlock / 64; ++k) {
      a += ss[k];
      b = nan_max(b, mx[k]);
    }
    out2[0] = a;  // sum of squares
    out2[1] = b;  // max
  }
  __syncthreads();
}

// stats[r] = {sum x^2, max x} per trace
template <typename T>
__global__ __launch_bounds__(kStatBlock) void row_stats_kernel(const T* __restrict__ x, int64_t row_stride,
                                                                int32_t n_t, double* __restrict__ stats) {
  block_row_stats(x + (int64_t)blockIdx.x * row_stride, n_t, stats + 2 * (int64_t)blockIdx.x);
}

// One find_noise_idx + impute_noisy_trace round (one block): idx = np.argmax(cond) over traces
// (first true, 0 if none) with cond = ||x_r|| < thr (empty) or max(x_r) > thr (noisy); then
// x[idx] = x[idx-1] (last), x[1] (first) or x[idx-1] + x[idx+1] (a sum, as the reference does);
// the trace's stats are refreshed for the next round.
template <typename T>
__global__ __launch_bounds__(kStatBlock) void impute_kernel(T* __restrict__ x, int64_t n_rows, int64_t row_stride,
                                                             int32_t n_t, int32_t empty, double thr,
                                                             double* __restrict__ stats, int32_t* __restrict__ idx_out) {
  __shared__ int first;
  if (threadIdx.x == 0) first = INT32_MAX;
  __syncthreads();
  for (int64_t r = threadIdx.x; r < n_rows; r += blockDim.x) {
    const bool c = empty ? (sqrt(stats[2 * r]) < thr) : (stats[2 * r + 1] > thr);
    if (c) atomicMin(&first, (int)r);
  }
  __syncthreads();
  const int64_t idx = first == INT32_MAX ? 0 : first;
  if (threadIdx.x == 0 && idx_out) *idx_out = (int32_t)idx;
  if (n_rows < 2) return;  // x[0] = x[-1] is x[0] itself
  T* dst = x + idx * row_stride;
  const T* a = x + (idx + 1 == n_rows ? idx - 1 : (idx == 0 ? 1 : idx - 1)) * row_stride;
  const T* b = (idx > 0 && idx + 1 < n_rows) ? x + (idx + 1) * row_stride : nullptr;
  constexpr int U = 8;
  int t = threadIdx.x;
  for (; t + (U - 1) * kStatBlock < n_t; t += U * kStatBlock) {
    T va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      va[u] = a[t + u * kStatBlock];
      vb[u] = b ? b[t + u * kStatBlock] : (T)0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) dst[t + u * kStatBlock] = b ? (T)(va[u] + vb[u]) : va[u];
  }
  for (; t < n_t; t += kStatBlock) dst[t] = b ? (T)(a[t] + b[t]) : a[t];
  __syncthreads();
  block_row_stats(dst, n_t, stats + 2 * idx);
}

// data /= np.linalg.norm(data, axis=-1, keepdims=True)
template <typename T>
__global__ __launch_bounds__(256) void row_normalize_kernel(T* __restrict__ x, int64_t row_stride, int32_t n_t,
                                                            const double* __restrict__ stats) {
  const int64_t r = blockIdx.y;
  const double nrm = sqrt(stats[2 * r]);
  T* row = x + r * row_stride;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_t; t += gridDim.x * blockDim.x)
    row[t] = (T)((double)row[t] / nrm);
}

// the same with 16-byte accesses (rows 16-byte aligned): 4 floats or 2 doubles per lane
template <typename T>
__global__ __launch_bounds__(256) void row_normalize_vec_kernel(T* __restrict__ x, int64_t row_stride, int32_t n_t,
                                                                const double* __restrict__ stats) {
  constexpr int V = 16 / sizeof(T);
  using Vec = typename std::conditional<sizeof(T) == 4, float4, double2>::type;
  const int64_t r = blockIdx.y;
  const double nrm = sqrt(stats[2 * r]);
  T* row = x + r * row_stride;
  const int nv = n_t / V;
  Vec* rv = reinterpret_cast<Vec*>(row);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += gridDim.x * blockDim.x) {
    Vec v = rv[i];
    T* e = reinterpret_cast<T*>(&v);
#pragma unroll
    for (int k = 0; k < V; ++k) e[k] = (T)((double)e[k] / nrm);
    rv[i] = v;
  }
  for (int t = nv * V + blockIdx.x * blockDim.x + threadIdx.x; t < n_t; t += gridDim.x * blockDim.x)
    row[t] = (T)((double)row[t] / nrm);
}

template <typename T>
static int trace_cleanup(T* x, int64_t n_rows, int64_t row_stride, int32_t n_t, int32_t flags, double thr,
                         double* stats, int32_t* idx_out, hipStream_t s) {
  hipLaunchKernelGGL(row_stats_kernel<T>, dim3((unsigned)n_rows), dim3(kStatBlock), 0, s, x, row_stride, n_t, stats);
  if (flags & 1)
    hipLaunchKernelGGL(impute_kernel<T>, dim3(1), dim3(kStatBlock), 0, s, x, n_rows, row_stride, n_t, 1, thr, stats,
                       idx_out);
  if (flags & 2)
    hipLaunchKernelGGL(impute_kernel<T>, dim3(1), dim3(kStatBlock), 0, s, x, n_rows, row_stride, n_t, 0, thr, stats,
                       idx_out ? idx_out + 1 : nullptr);
  if (flags & 4) {
    constexpr int V = 16 / sizeof(T);
    if (reinterpret_cast<uintptr_t>(x) % 16 == 0 && row_stride % V == 0)
      hipLaunchKernelGGL(row_normalize_vec_kernel<T>, dim3((unsigned)((n_t / V + 255) / 256 + 1), (unsigned)n_rows),
                         dim3(256), 0, s, x, row_stride, n_t, stats);
    else
      hipLaunchKernelGGL(row_normalize_kernel<T>, dim3((unsigned)((n_t + 255) / 256), (unsigned)n_rows), dim3(256), 0,
                         s, x, row_stride, n_t, stats);
  }
  return last_launch();
}

// SurfaceWaveSelector.locate_windows' cut (apis/data_classes.py:208-209, deepcopy of
// data[x_start:x_start + n_ch, t_start[w]:t_start[w] + n_t]) for all accepted passes at once:
// out[w][c][t] (contiguous batch, converted to Out).  Reads are guarded against the record's
// extent; a window outside it sets *status and is left unwritten.
template <typename In, typename Out>
__global__ __launch_bounds__(256) void cut_windows_kernel(const In* __restrict__ rec, int64_t n_rows,
                                                          int64_t row_stride, int64_t rec_n_t,
                                                          const int64_t* __restrict__ t_start, int64_t x_start,
                                                          int32_t n_ch, int32_t n_t, Out* __restrict__ out,
                                                          int32_t* __restrict__ status) {
  const int64_t w = blockIdx.z;
  const int c = blockIdx.y;
  const int64_t ts = t_start[w];
  if (ts < 0 || ts + n_t > rec_n_t || x_start < 0 || x_start + n_ch > n_rows) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && c == 0 && status) atomicOr(status, 1);
    return;
  }
  const In* src = rec + (x_start + c) * row_stride + ts;
  Out* dst = out + (w * n_ch + c) * (int64_t)n_t;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_t; t += gridDim.x * blockDim.x) dst[t] = (Out)src[t];
}

template <typename In, typename Out>
static int cut_windows(const void* rec, int64_t n_rows, int64_t row_stride, int64_t rec_n_t, const int64_t* t_start,
                       int32_t n_win, int64_t x_start, int32_t n_ch, int32_t n_t, void* out, int32_t* status,
                       hipStream_t s) {
  const unsigned gx = (unsigned)((n_t + 255) / 256 < 64 ? (n_t + 255) / 256 : 64);
  for (int32_t w0 = 0; w0 < n_win; w0 += 65535) {  // gridDim.z limit
    const int32_t nw = n_win - w0 < 65535 ? n_win - w0 : 65535;
    hipLaunchKernelGGL((cut_windows_kernel<In, Out>), dim3(gx, n_ch, nw), dim3(256), 0, s, (const In*)rec, n_rows,
                       row_stride, rec_n_t, t_start + w0, x_start, n_ch, n_t,
                       (Out*)out + (int64_t)w0 * n_ch * n_t, status);
  }
  return last_launch();
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_trace_cleanup(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t, int32_t flags,
                              double noise_threshold, double* stats, int32_t* idx_out, void* stream) {
  if (!x || !stats) return set_error(-2, "null pointer argument");
  if (n_rows <= 0 || n_t <= 0) return 0;
  if (n_rows > 65535 && (flags & 4)) return set_error(-4, "too many traces for one launch");
  return with_float_type(dtype, [&](auto t) {
    return trace_cleanup((decltype(t)*)x, n_rows, row_stride, n_t, flags, noise_threshold, stats, idx_out,
                         (hipStream_t)stream);
  });
}

DVH_API int dvh_mute_traj(void* data, int32_t dtype, int32_t n_pass, int64_t pass_stride, int32_t n_ch, int32_t n_t,
                          const int32_t* tab, const double* taper, void* stream) {
  if (!data || !tab || !taper) return set_error(-2, "null pointer argument");
  if (n_pass <= 0 || n_ch <= 0 || n_t <= 0) return 0;
  if (n_ch > 65535 || n_pass > 65535)  // gridDim.y / gridDim.z limit
    return set_error(-4, "too many channels or passes for one launch");
  const dim3 grid((n_t + 255) / 256, n_ch, n_pass);
  return with_float_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mute_traj_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (T*)data, pass_stride, n_ch, n_t,
                       tab, taper);
    return last_launch();
  });
}

DVH_API int dvh_mute_time(void* data, int32_t dtype, int64_t n_rows, int32_t n_t, const double* taper, void* stream) {
  if (!data || !taper) return set_error(-2, "null pointer argument");
  if (n_rows <= 0 || n_t <= 0) return 0;
  const int64_t n = n_rows * n_t;
  const dim3 grid((unsigned)((n + 255) / 256));
  return with_float_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mute_time_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (T*)data, n_rows, n_t, taper);
    return last_launch();
  });
}

DVH_API int dvh_cut_windows(const void* rec, int32_t in_dtype, int64_t n_rows, int64_t row_stride, int64_t rec_n_t,
                            const int64_t* t_start, int32_t n_win, int64_t x_start, int32_t n_ch, int32_t n_t,
                            void* out, int32_t out_dtype, int32_t* status, void* stream) {
  if (!rec || !t_start || !out) return set_error(-2, "null pointer argument");
  if (n_win < 0 || n_ch < 0 || n_t < 0) return set_error(-2, "invalid sizes");
  if (n_win == 0 || n_ch == 0 || n_t == 0) return 0;
  if (n_ch > 65535) return set_error(-4, "too many channels for one launch");
  if (x_start < 0 || x_start + n_ch > n_rows || n_t > rec_n_t) return set_error(-2, "window outside the record");
  return with_float_type(in_dtype, [&](auto in) {
    return with_float_type(out_dtype, [&](auto o) {
      return cut_windows<decltype(in), decltype(o)>(rec, n_rows, row_stride, rec_n_t, t_start, n_win, x_start, n_ch, n_t,
                                                    out, status, (hipStream_t)stream);
    });
  });
}

