// Tracking-grid preprocessing of a continuous record (TimeLapseImaging._preprocess_for_tracking,
// apis/timeLapseImaging.py:74-102), the stages the other files do not already hold:
//   dvh_median_abs_gate  means = np.median(np.abs(data), axis=-1); data[means > noise_level] *= 0  (:76-77)
//   dvh_resample_rows_t  signal.resample_poly(data[:, ::subsamp_factor], up, down) (:88-91), written transposed
//                        so that the row-wise dvh_sosfiltfilt then runs along space (bandpass_data_space, :98)
//   dvh_transpose_f64    back to [n_out][n_t_out]
// The two band-passes are dvh_sosfiltfilt_planned and the imputation is dvh_trace_cleanup (dvh_prep.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "dvh.h"
#include "dvh_common.h"

namespace dvh {

// ---------------------------------------------------------------------------------------------
// Median of |x| per trace by radix select, and the gate.
//
// One 256-thread block per trace.  The bit pattern of |x| is a non-negative integer whose order is the value's
// order, so the k-th smallest |x| is found 8 bits at a time from the top: a 256-bin histogram (one per wave, in LDS)
// of the current byte over the samples that match the bytes already fixed, a block scan of the bins, and the bin
// holding rank k fixes the next byte.  The row is re-read every pass (4 passes for float32, 8 for float64): nothing
// of the row is kept in LDS, so any n_t works.  The last pass also gives the number of samples equal to the k-th
// value, which says whether the second middle value of an even-length row is the same value or the smallest
// pattern above it (one more pass, a min reduction).  A pattern above +inf's is a NaN: np.median is then NaN and
// `NaN > noise_level` is false.

constexpr int kSelBlock = 256;
constexpr int kSelWaves = kSelBlock / 64;

template <typename T>
struct AbsBits;
template <>
struct AbsBits<float> {
  using U = uint32_t;
  static constexpr U kInf = 0x7f800000u;
  static __device__ __forceinline__ U of(float v) { return __float_as_uint(v) & 0x7fffffffu; }
  static __device__ __forceinline__ double value(U p) { return (double)__uint_as_float(p); }
};
template <>
struct AbsBits<double> {
  using U = uint64_t;
  static constexpr U kInf = 0x7ff0000000000000ull;
  static __device__ __forceinline__ U of(double v) {
    return (U)__double_as_longlong(v) & 0x7fffffffffffffffull;
  }
  static __device__ __forceinline__ double value(U p) { return __longlong_as_double((long long)p); }
};

template <typename T>
__global__ __launch_bounds__(kSelBlock) void median_abs_gate_kernel(T* __restrict__ x, int64_t row_stride, int32_t n_t,
                                                                    double noise_level, double* __restrict__ med_out,
                                                                    int32_t* __restrict__ gated_out) {
  using B = AbsBits<T>;
  using U = typename B::U;
  constexpr int kBits = 8 * sizeof(U);
  __shared__ uint32_t hist[kSelWaves][256];
  __shared__ uint32_t wave_tot[kSelWaves];
  __shared__ uint32_t sel_bin, sel_rank, sel_cnt, has_nan;
  __shared__ unsigned long long min_above;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  T* row = x + (int64_t)blockIdx.x * row_stride;
  const uint32_t k_lo = (uint32_t)(n_t - 1) / 2, k_hi = (uint32_t)n_t / 2;  // the two middle ranks (equal: odd n_t)

  U prefix = 0;
  uint32_t rank = k_lo;   // rank of the wanted sample among those matching the prefix
  uint32_t below = 0;     // samples below the prefix range
  uint32_t n_eq = 0;      // after the last pass: samples equal to the k_lo-th value
  if (tid == 0) has_nan = 0;
  for (int shift = kBits - 8; shift >= 0; shift -= 8) {
    for (int i = tid; i < kSelWaves * 256; i += kSelBlock) (&hist[0][0])[i] = 0;
    __syncthreads();
    const bool first = shift == kBits - 8;
    bool nan_seen = false;
    for (int t = tid; t < n_t; t += kSelBlock) {
      const U p = B::of(row[t]);
      if (first) {
        nan_seen |= p > B::kInf;
        atomicAdd(&hist[wv][(uint32_t)(p >> shift)], 1u);
      } else if ((p >> (shift + 8)) == (prefix >> (shift + 8))) {
        atomicAdd(&hist[wv][(uint32_t)(p >> shift) & 255u], 1u);
      }
    }
    if (first && nan_seen) has_nan = 1;
    __syncthreads();
    if (has_nan) {  // uniform: written before the barrier
      if (tid == 0) {
        if (med_out) med_out[blockIdx.x] = __longlong_as_double(0x7ff8000000000000ll);
        if (gated_out) gated_out[blockIdx.x] = 0;
      }
      return;
    }
    // bin tid's count and the exclusive scan of the bins over the block
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < kSelWaves; ++w) c += hist[w][tid];
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(inc, o);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wv; ++w) base += wave_tot[w];
    const uint32_t exc = base + inc - c;
    if (c > 0 && exc <= rank && rank < exc + c) {  // exactly one bin holds the rank
      sel_bin = (uint32_t)tid;
      sel_rank = rank - exc;
      sel_cnt = c;
      min_above = ~0ull;
    }
    __syncthreads();
    prefix |= (U)sel_bin << shift;
    below += rank - sel_rank;
    rank = sel_rank;
    n_eq = sel_cnt;
    // the next pass's histogram reset is ordered after these reads by its own barrier; sel_* are rewritten only
    // after the barrier that follows the next histogram
  }
  const U a = prefix;
  U b = a;
  if (k_hi >= below + n_eq) {  // the second middle sample is the smallest pattern above a (it exists: k_hi < n_t)
    unsigned long long m = ~0ull;
    for (int t = tid; t < n_t; t += kSelBlock) {
      const U p = B::of(row[t]);
      if (p > a && (unsigned long long)p < m) m = p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long v = __shfl_xor(m, o);
      m = v < m ? v : m;
    }
    if (lane == 0) atomicMin(&min_above, m);
    __syncthreads();
    b = (U)min_above;
  }
  const double med = (B::value(a) + B::value(b)) / 2.0;  // np.mean of the two (odd n_t: a == b)
  const bool gate = med > noise_level;
  if (tid == 0) {
    if (med_out) med_out[blockIdx.x] = med;
    if (gated_out) gated_out[blockIdx.x] = gate ? 1 : 0;
  }
  if (gate)
    for (int t = tid; t < n_t; t += kSelBlock) row[t] = row[t] * (T)0;  // `*= 0`: -0.0 and NaN as numpy leaves them
}

// ---------------------------------------------------------------------------------------------
// Polyphase resampling along the channel axis, fused with the time decimation, written transposed:
//   out[t][m] = sum_k h[half_len + down m - up k] x[k][t t_step]
// A block owns kRsTM outputs m x kRsTT times.  The input rows its outputs read form one contiguous range of k; it is
// staged through LDS in chunks of kRsKC rows x kRsTT times (the loads run along t, the strided axis of the record:
// a wave reads two rows' spans), then lane = m accumulates its kRsTT times from LDS, and the stores run along m (a wave
// writes 64 consecutive doubles of one output row).  A filter coefficient depends on (m, k) only, so one load of h
// serves kRsTT multiply-adds.

constexpr int kRsTM = 256;  // outputs m per block = threads
constexpr int kRsTT = 16;   // times per block
constexpr int kRsKC = 64;   // input rows per LDS chunk

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {  // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

template <typename T>
__global__ __launch_bounds__(kRsTM) void resample_rows_t_kernel(const T* __restrict__ x, int32_t n_in,
                                                                 int64_t row_stride, int32_t t_step, int32_t n_t_out,
                                                                 const double* __restrict__ h, int32_t half_len,
                                                                 int32_t up, int32_t down, double* __restrict__ out,
                                                                 int64_t out_stride, int32_t n_out) {
  __shared__ double xs[kRsKC][kRsTT + 1];
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kRsTT;
  const int64_t m0 = (int64_t)blockIdx.y * kRsTM;
  const int64_t m = m0 + tid;
  const int64_t m_last = (m0 + kRsTM - 1 < n_out ? m0 + kRsTM - 1 : n_out - 1);
  // input rows of the block's outputs, and of this thread's output: 0 <= half_len + down m - up k <= 2 half_len
  int64_t kb0 = floor_div((int64_t)down * m0 - half_len + up - 1, up);
  int64_t kb1 = floor_div((int64_t)down * m_last + half_len, up);
  kb0 = kb0 < 0 ? 0 : kb0;
  kb1 = kb1 > n_in - 1 ? n_in - 1 : kb1;
  int64_t k0 = 0, k1 = -1;
  if (m < n_out) {
    k0 = floor_div((int64_t)down * m - half_len + up - 1, up);
    k1 = floor_div((int64_t)down * m + half_len, up);
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > n_in - 1 ? n_in - 1 : k1;
  }
  double acc[kRsTT];
#pragma unroll
  for (int j = 0; j < kRsTT; ++j) acc[j] = 0.0;

  for (int64_t kc = kb0; kc <= kb1; kc += kRsKC) {
    __syncthreads();  // the previous chunk has been consumed
    for (int i = tid; i < kRsKC * kRsTT; i += kRsTM) {
      const int r = i / kRsTT, j = i % kRsTT;
      const int64_t k = kc + r, t = t0 + j;
      xs[r][j] = (k <= kb1 && t < n_t_out) ? (double)x[k * row_stride + t * t_step] : 0.0;
    }
    __syncthreads();
    const int64_t ka = k0 > kc ? k0 : kc;
    const int64_t kz = k1 < kc + kRsKC - 1 ? k1 : kc + kRsKC - 1;
    for (int64_t k = ka; k <= kz; ++k) {
      const double hv = h[(int64_t)half_len + (int64_t)down * m - (int64_t)up * k];
      const double* xr = xs[k - kc];
#pragma unroll
      for (int j = 0; j < kRsTT; ++j) acc[j] = fma(hv, xr[j], acc[j]);
    }
  }
  if (m < n_out) {
#pragma unroll
    for (int j = 0; j < kRsTT; ++j)
      if (t0 + j < n_t_out) out[(t0 + j) * out_stride + m] = acc[j];
  }
}

// ---------------------------------------------------------------------------------------------
// dst[c][r] = src[r][c] through a 32 x 32 LDS tile (padded: no bank conflicts on the transposed read); loads run
// along src rows, stores along dst rows.

constexpr int kTrTile = 32;

__global__ __launch_bounds__(256) void transpose_f64_kernel(const double* __restrict__ src, int64_t n_rows,
                                                            int64_t n_cols, int64_t src_stride,
                                                            double* __restrict__ dst, int64_t dst_stride,
                                                            int64_t tiles_c) {
  __shared__ double tile[kTrTile][kTrTile + 1];
  const int64_t r0 = ((int64_t)blockIdx.x / tiles_c) * kTrTile, c0 = ((int64_t)blockIdx.x % tiles_c) * kTrTile;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < kTrTile; i += 8)
    if (r0 + i < n_rows && c0 + tx < n_cols) tile[i][tx] = src[(r0 + i) * src_stride + c0 + tx];
  __syncthreads();
  for (int i = ty; i < kTrTile; i += 8)
    if (c0 + i < n_cols && r0 + tx < n_rows) dst[(c0 + i) * dst_stride + r0 + tx] = tile[tx][i];
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_median_abs_gate(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t,
                                double noise_level, double* med_out, int32_t* gated_out, void* stream) {
  if (!x) return set_error(-2, "null pointer argument");
  if (dtype != 0 && dtype != 1) return set_error(-2, "dtype must be 0 (float32) or 1 (float64)");
  if (n_rows < 0 || n_t < 0 || row_stride < n_t) return set_error(-2, "invalid shape");
  if (n_rows == 0) return 0;
  if (n_t == 0) return set_error(-2, "the median of an empty trace is undefined");
  if (n_rows > 0x7fffffffLL) return set_error(-4, "too many traces for one launch");
  const hipStream_t s = (hipStream_t)stream;
  return with_float_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(median_abs_gate_kernel<T>, dim3((unsigned)n_rows), dim3(kSelBlock), 0, s, (T*)x, row_stride,
                       n_t, noise_level, med_out, gated_out);
    return last_launch();
  });
}

DVH_API int dvh_resample_rows_t(const void* x, int32_t dtype, int32_t n_in, int64_t row_stride, int32_t t_step,
                                int32_t n_t_out, const double* h, int32_t half_len, int32_t up, int32_t down,
                                double* out, int64_t out_stride, int32_t n_out, void* stream) {
  if (!x || !h || !out) return set_error(-2, "null pointer argument");
  if (dtype != 0 && dtype != 1) return set_error(-2, "dtype must be 0 (float32) or 1 (float64)");
  if (n_in < 0 || n_t_out < 0 || t_step < 1 || up < 1 || down < 1 || half_len < 0)
    return set_error(-2, "invalid shape or resampling ratio");
  if ((int64_t)n_out != ((int64_t)n_in * up + down - 1) / down)
    return set_error(-2, "n_out must be ceil(n_in * up / down)");
  if (out_stride < n_out) return set_error(-2, "out_stride is shorter than an output row");
  if (n_out == 0 || n_t_out == 0) return 0;
  const int64_t gy = ((int64_t)n_out + kRsTM - 1) / kRsTM;
  if (gy > 65535) return set_error(-4, "too many output rows for one launch");
  const dim3 grid((unsigned)(((int64_t)n_t_out + kRsTT - 1) / kRsTT), (unsigned)gy);
  const hipStream_t s = (hipStream_t)stream;
  return with_float_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(resample_rows_t_kernel<T>, grid, dim3(kRsTM), 0, s, (const T*)x, n_in, row_stride, t_step,
                       n_t_out, h, half_len, up, down, out, out_stride, n_out);
    return last_launch();
  });
}

DVH_API int dvh_transpose_f64(const double* src, int64_t n_rows, int64_t n_cols, int64_t src_stride, double* dst,
                              int64_t dst_stride, void* stream) {
  if (!src || !dst) return set_error(-2, "null pointer argument");
  if (n_rows < 0 || n_cols < 0 || src_stride < n_cols || dst_stride < n_rows) return set_error(-2, "invalid shape");
  if (n_rows == 0 || n_cols == 0) return 0;
  const int64_t tiles_c = (n_cols + kTrTile - 1) / kTrTile, tiles_r = (n_rows + kTrTile - 1) / kTrTile;
  if (tiles_c * tiles_r > 0x7fffffffLL) return set_error(-4, "too many tiles for one launch");
  hipLaunchKernelGGL(transpose_f64_kernel, dim3((unsigned)(tiles_c * tiles_r)), dim3(256), 0, (hipStream_t)stream, src,
                     n_rows, n_cols, src_stride, dst, dst_stride, tiles_c);
  return last_launch();
}
