// Vehicle tracking on the tracking grid (KF_tracking, apis/tracking.py:21-168):
//   dvh_find_peaks_rows  scipy.signal.find_peaks(sign * x[row], distance=, prominence=, wlen=)[0] of a strided set of
//                        rows (:36-39, :44, :122)
//   dvh_peak_likelihood  the detection curve of detect_in_one_section (:30-42; likelihood_1d,
//                        modules/car_tracking_utils.py:21-26)
//   dvh_kf_track         the association and Kalman loop of tracking_with_veh_base (:101-155), one thread per vehicle
// remove_unrealistic_tracking and interp_nan_value work on the small [n_veh, n_steps] result on the host
// (apis/tracking.py of this package).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dvh.h"
#include "dvh_common.h"

namespace dvh {

// ---------------------------------------------------------------------------------------------
// find_peaks of one row per 256-thread block, in SciPy's order: local maxima, distance, prominence.
//
// LDS (dynamic): the row times sign when n_t <= kPkStageMax (longer rows are read from global memory, the row then
// being cache resident), the candidate list cand[] (ascending sample indices, at most (n_t - 1) / 2 of them), eight
// words of bookkeeping and one state byte per candidate: 0 undecided, 2 removed, 3 kept.
//
// Local maxima (_local_maxima_1d): sample i starts a plateau when x[i-1] < x[i]; its thread walks to the plateau's
// end and the plateau is a peak at (left + right) / 2 when the next sample is lower.  Starts are independent (a
// sample inside or right after a plateau is no start), so every sample is tested by its own thread and the hits of a
// 256-sample tile are appended in order through a ballot and a scan of the wave totals.  Comparisons with NaN are
// false; the first and last sample are never tested, and a plateau reaching the last sample finds no lower one.
//
// Distance (_select_by_peak_distance): the serial rule "visit from the highest, a peak still kept removes all closer
// than `distance`" keeps a peak exactly when no kept higher one is closer than `distance`.  Rounds: an undecided peak
// that outranks every undecided peak closer than `distance` is kept (all that outrank it were removed, so the serial
// pass keeps it too), then every undecided peak closer than `distance` to a kept one is removed.  The global
// highest undecided peak is decided every round, so the rounds end.  Equal heights rank by index, larger first (a
// stable ascending sort visited from the top).  A kept peak is marked 3 at once: a neighbour that reads 3 in the
// same round knows it lost, one that still reads 0 compares ranks and loses as well, so the race is harmless.
//
// Prominence (_peak_prominences) of the peaks the distance rule kept: scans outward from the peak while
// x[i] <= x[peak] inside [peak - wlen / 2, peak + wlen / 2] clipped to the row (wlen 0: the whole row), tracking
// the minimum; prominence = x[peak] - max(left_min, right_min); kept when >= min_prominence.  One thread per peak, in
// the pass that also appends the survivors to the output in order.

constexpr int kPkBlock = 256;
constexpr int kPkWaves = kPkBlock / 64;
constexpr int kPkMisc = 8;         // int32 words of block bookkeeping in LDS
constexpr int kPkStageMax = 6000;  // 8 n_t + 5 (n_t / 2 + 1) + 32 bytes <= 63 037: inside the 64 KB a block may take

// Position of this thread's hit among the block's hits in thread order, after `base` earlier ones; base moves on by
// the block's count.  Two barriers: every thread of the block must call it.
__device__ __forceinline__ int block_append_pos(bool hit, int& base, uint32_t* wave_tot) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long b = __ballot(hit);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wv] = (uint32_t)__popcll(b);
  __syncthreads();
  int off = base, tot = 0;
#pragma unroll
  for (int w = 0; w < kPkWaves; ++w) {
    const int c = (int)wave_tot[w];
    if (w < wv) off += c;
    tot += c;
  }
  __syncthreads();
  base += tot;
  return off + before;
}

template <bool kStaged>
__global__ __launch_bounds__(kPkBlock) void find_peaks_rows_kernel(
    const double* __restrict__ x, int64_t row_stride, int32_t n_t, int64_t row0, int64_t row_step, double sign,
    int32_t dist, int32_t use_prom, double min_prom, int32_t wlen, int32_t* __restrict__ peaks, int32_t cap,
    int32_t* __restrict__ count, double* __restrict__ prom_out, int32_t* __restrict__ status) {
  // all LDS in the dynamic region, the doubles first: a static variable ahead of it would shift its base off the
  // 8-byte alignment the row's loads need
  extern __shared__ __attribute__((aligned(16))) double pk_smem[];
  const int tid = threadIdx.x;
  const int n_cmax = n_t / 2 + 1;
  const double* row = x + (row0 + (int64_t)blockIdx.x * row_step) * row_stride;
  double* xs = pk_smem;
  int32_t* cand = (int32_t*)(pk_smem + (kStaged ? n_t : 0));
  uint32_t* wave_tot = (uint32_t*)(cand + n_cmax);  // kPkWaves words, then `again`: kPkMisc words in all
  int& again = *(int*)(wave_tot + kPkWaves);
  uint8_t* st = (uint8_t*)(wave_tot + kPkMisc);
  auto val = [&](int i) -> double { return kStaged ? xs[i] : sign * row[i]; };

  if (kStaged) {
    for (int i = tid; i < n_t; i += kPkBlock) xs[i] = sign * row[i];
    __syncthreads();
  }

  // local maxima -> cand[0 .. n_c)
  int n_c = 0;
  for (int i0 = 0; i0 < n_t; i0 += kPkBlock) {
    const int i = i0 + tid;
    bool pk = false;
    int mid = 0;
    if (i >= 1 && i < n_t - 1) {
      const double v = val(i);
      if (val(i - 1) < v) {
        int a = i + 1;
        while (a < n_t - 1 && val(a) == v) ++a;
        if (val(a) < v) {
          pk = true;
          mid = (i + a - 1) / 2;
        }
      }
    }
    const int pos = block_append_pos(pk, n_c, wave_tot);
    if (pk) {  // pos < (n_t - 1) / 2 <= n_cmax: a peak needs a lower sample on either side
      cand[pos] = mid;
      st[pos] = 0;
    }
  }
  __syncthreads();

  if (dist > 0 && n_c > 1) {
    for (;;) {
      if (tid == 0) again = 0;
      __syncthreads();
      for (int j = tid; j < n_c; j += kPkBlock) {
        if (st[j] != 0) continue;
        const int pj = cand[j];
        const double hj = val(pj);
        bool win = true;
        for (int k = j - 1; win && k >= 0 && pj - cand[k] < dist; --k) {
          const int s = st[k];
          if (s == 3 || (s == 0 && val(cand[k]) > hj)) win = false;
        }
        for (int k = j + 1; win && k < n_c && cand[k] - pj < dist; ++k) {
          const int s = st[k];
          if (s == 3 || (s == 0 && val(cand[k]) >= hj)) win = false;  // equal heights: the larger index outranks
        }
        if (win) st[j] = 3;
      }
      __syncthreads();
      for (int j = tid; j < n_c; j += kPkBlock) {
        if (st[j] != 0) continue;
        const int pj = cand[j];
        bool lose = false;
        for (int k = j - 1; !lose && k >= 0 && pj - cand[k] < dist; --k) lose = st[k] == 3;
        for (int k = j + 1; !lose && k < n_c && cand[k] - pj < dist; ++k) lose = st[k] == 3;
        if (lose)
          st[j] = 2;
        else
          again = 1;
      }
      __syncthreads();
      const int more = again;
      __syncthreads();  // every thread has read `again` before thread 0 clears it
      if (!more) break;
    }
  }

  // prominence of the kept peaks and the ordered output
  const int64_t out0 = (int64_t)blockIdx.x * cap;
  const bool want_prom = use_prom != 0 || prom_out != nullptr;
  int n_out = 0;
  for (int j0 = 0; j0 < n_c; j0 += kPkBlock) {
    const int j = j0 + tid;
    bool ok = false;
    int p = 0;
    double prom = 0.0;
    if (j < n_c && st[j] != 2) {
      ok = true;
      p = cand[j];
      if (want_prom) {
        const double v = val(p);
        int lo = 0, hi = n_t - 1;
        if (wlen >= 2) {
          lo = p - wlen / 2 > lo ? p - wlen / 2 : lo;
          hi = p + wlen / 2 < hi ? p + wlen / 2 : hi;
        }
        double lmin = v, rmin = v;
        for (int i = p; i >= lo; --i) {
          const double xi = val(i);
          if (!(xi <= v)) break;
          lmin = xi < lmin ? xi : lmin;
        }
        for (int i = p; i <= hi; ++i) {
          const double xi = val(i);
          if (!(xi <= v)) break;
          rmin = xi < rmin ? xi : rmin;
        }
        prom = v - (lmin > rmin ? lmin : rmin);
        if (use_prom && !(prom >= min_prom)) ok = false;
      }
    }
    const int pos = block_append_pos(ok, n_out, wave_tot);
    if (ok && pos < cap) {
      peaks[out0 + pos] = p;
      if (prom_out) prom_out[out0 + pos] = prom;
    }
  }
  if (tid == 0) {
    count[blockIdx.x] = n_out < cap ? n_out : cap;
    if (status) status[blockIdx.x] = n_out > cap ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------
// out[t] = sum over rows (sum over the row's peaks of norm.pdf(t_axis[t], loc=t_axis[peak], scale=sigma)), one thread
// per t, in the reference's order: a row's peaks are summed first, then the row is added.  norm.pdf as SciPy
// evaluates it: exp(-z^2 / 2) / sqrt(2 pi) / sigma with z = (t - loc) / sigma.

__global__ __launch_bounds__(256) void peak_likelihood_kernel(const int32_t* __restrict__ peaks, int32_t cap,
                                                              const int32_t* __restrict__ count, int32_t n_rows,
                                                              const double* __restrict__ t_axis, int32_t n_t,
                                                              double sigma, double* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_t) return;
  const double tt = t_axis[t];
  const double sqrt_2pi = 2.5066282746310002;  // np.sqrt(2 * np.pi)
  double acc = 0.0;
  for (int r = 0; r < n_rows; ++r) {
    int c = count[r];
    c = c < cap ? c : cap;
    double row_acc = 0.0;
    for (int p = 0; p < c; ++p) {
      const int pk = peaks[(int64_t)r * cap + p];
      if (pk < 0 || pk >= n_t) continue;  // not a sample of this axis
      const double z = (tt - t_axis[pk]) / sigma;
      row_acc = row_acc + exp(-(z * z) / 2.0) / sqrt_2pi / sigma;
    }
    acc += row_acc;
  }
  out[t] = acc;
}

// ---------------------------------------------------------------------------------------------
// tracking_with_veh_base's loop, one thread per vehicle (vehicles do not interact), sequential over the steps.
// The arithmetic follows the reference's matrix products term by term and is not contracted into fused
// multiply-adds: the predicted arrival is truncated to an integer, so it is kept as close to NumPy's as it can be.

constexpr int kKfBlock = 64;

__global__ __launch_bounds__(kKfBlock) void kf_track_kernel(const int32_t* __restrict__ peaks, int32_t cap,
                                                            const int32_t* __restrict__ count, int32_t n_steps,
                                                            const double* __restrict__ x_sel,
                                                            const int32_t* __restrict__ veh_base, int32_t n_veh,
                                                            double sigma_a, double* __restrict__ veh_states) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * kKfBlock + threadIdx.x;
  if (v >= n_veh) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t base0 = veh_base[v];
  int cnt = 0;                       // matches so far
  double first_z = 0.0, first_x = 0.0;  // the first match and its position
  double T0 = 0.0, T1 = 0.0, P00 = 0.0, P01 = 0.0, P10 = 0.0, P11 = 0.0, xv = 0.0;  // filtered
  double Tp0 = 0.0, Tp1 = 0.0, Q00 = 0.0, Q01 = 0.0, Q10 = 0.0, Q11 = 0.0;          // predicted (Q..: Pk1k)
  double* out = veh_states + (int64_t)v * n_steps;
  for (int k = 0; k < n_steps; ++k) {
    const double xk = x_sel[k];
    int64_t base = base0;
    bool search = true;
    if (cnt == 1) {  // re-seeded every step while there is exactly one match
      T0 = first_z;
      T1 = 0.0;
      xv = first_x;
      P00 = P01 = P10 = P11 = 0.0;
    } else if (cnt >= 2) {
      const double dx = xk - xv;
      Tp0 = T0 + dx * T1;  // A = [[1, dx], [0, 1]]
      Tp1 = T1;
      const double a00 = P00 + dx * P10, a01 = P01 + dx * P11;  // A P
      const double dx2 = dx * dx;
      Q00 = (a00 + a01 * dx) + sigma_a * (0.25 * (dx2 * dx2));  // (A P) A^T + Q
      Q01 = a01 + sigma_a * (0.5 * (dx2 * dx));
      Q10 = (P10 + P11 * dx) + sigma_a * (0.5 * (dx2 * dx));
      Q11 = P11 + sigma_a * dx2;
      if (Tp0 > -1e9 && Tp0 < 1e9)
        base = (int64_t)Tp0;  // truncated toward zero: the reference stores it in an integer array
      else
        search = false;  // no sample index: nothing can match
    }
    // the nearest peak ahead within (0, 30], else the nearest within (-15, 0]: the row's peaks ascend, so both
    // sit next to the first peak above the base (a bisection: 6 dependent loads for 40 peaks instead of 40)
    int64_t ahead = 31, behind = -15;
    if (search) {
      int c = count[k];
      c = c < cap ? c : cap;
      const int32_t* pk = peaks + (int64_t)k * cap;
      int lo = 0, hi = c;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)pk[mid] > base)
          hi = mid;
        else
          lo = mid + 1;
      }
      if (lo < c) {
        const int64_t d = (int64_t)pk[lo] - base;
        if (d <= 30) ahead = d;
      }
      if (lo > 0) {
        const int64_t d = (int64_t)pk[lo - 1] - base;
        if (d > -15) behind = d;
      }
    }
    const bool matched = ahead <= 30 || behind > -15;
    const double z = ahead <= 30 ? (double)(base + ahead) : (double)(base + behind);
    out[k] = matched ? z : nan;
    if (!matched) continue;
    ++cnt;
    if (cnt == 1) {
      first_z = z;
      first_x = xk;
    } else if (cnt > 2) {  // R = 1, C = [1, 0]
      const double s = 1.0 + Q00;
      const double K0 = Q00 / s, K1 = Q10 / s;
      const double innov = z - Tp0;
      T0 = Tp0 + K0 * innov;
      T1 = Tp1 + K1 * innov;
      P00 = Q00 - K0 * Q00;
      P01 = Q01 - K0 * Q01;
      P10 = Q10 - K1 * Q00;
      P11 = Q11 - K1 * Q01;
      xv = xk;
    }
  }
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_find_peaks_rows(const double* x, int64_t row_stride, int32_t n_t, int64_t row0, int64_t row_step,
                                int32_t n_sel, int32_t sign, double distance, int32_t use_prominence,
                                double min_prominence, double wlen, int32_t* peaks, int32_t cap, int32_t* count,
                                double* prominences, int32_t* status, void* stream) {
  if (!x || !peaks || !count) return set_error(-2, "null pointer argument");
  if (n_t < 1 || row_stride < n_t || n_sel < 0 || row0 < 0 || row_step < 1 || cap < 1)
    return set_error(-2, "invalid shape");
  if (sign != 1 && sign != -1) return set_error(-2, "sign must be +1 or -1");
  if (distance != distance || min_prominence != min_prominence || wlen != wlen)
    return set_error(-2, "NaN argument");
  if (n_t > DVH_FIND_PEAKS_MAX_NT) return set_error(-4, "row longer than DVH_FIND_PEAKS_MAX_NT samples");
  if (n_sel == 0) return 0;
  // ceil() as SciPy takes them; beyond the row's length both mean "the whole row"
  const int32_t dist = distance > 0 ? (int32_t)fmin(ceil(distance), (double)n_t + 1.0) : 0;
  const int32_t wl = wlen > 1 ? (int32_t)fmin(ceil(wlen), 2.0 * (double)n_t + 2.0) : 0;
  const bool staged = n_t <= kPkStageMax;
  const size_t lds = (staged ? sizeof(double) * (size_t)n_t : 0) + (size_t)5 * (size_t)(n_t / 2 + 1) +
                     sizeof(int32_t) * kPkMisc;
  const hipStream_t s = (hipStream_t)stream;
  if (staged)
    hipLaunchKernelGGL(find_peaks_rows_kernel<true>, dim3((unsigned)n_sel), dim3(kPkBlock), lds, s, x, row_stride, n_t,
                       row0, row_step, (double)sign, dist, use_prominence, min_prominence, wl, peaks, cap, count,
                       prominences, status);
  else
    hipLaunchKernelGGL(find_peaks_rows_kernel<false>, dim3((unsigned)n_sel), dim3(kPkBlock), lds, s, x, row_stride,
                       n_t, row0, row_step, (double)sign, dist, use_prominence, min_prominence, wl, peaks, cap, count,
                       prominences, status);
  return last_launch();
}

DVH_API int dvh_peak_likelihood(const int32_t* peaks, int32_t cap, const int32_t* count, int32_t n_rows,
                                const double* t_axis, int32_t n_t, double sigma, double* out, void* stream) {
  if (!t_axis || !out || (n_rows > 0 && (!peaks || !count))) return set_error(-2, "null pointer argument");
  if (n_rows < 0 || n_t < 0 || cap < 1 || !(sigma > 0)) return set_error(-2, "invalid shape or sigma");
  if (n_t == 0) return 0;
  hipLaunchKernelGGL(peak_likelihood_kernel, dim3((unsigned)((n_t + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     peaks, cap, count, n_rows, t_axis, n_t, sigma, out);
  return last_launch();
}

DVH_API int dvh_kf_track(const int32_t* peaks, int32_t cap, const int32_t* count, int32_t n_steps, const double* x_sel,
                         const int32_t* veh_base, int32_t n_veh, double sigma_a, double* veh_states, void* stream) {
  if (n_veh < 0 || n_steps < 0 || cap < 1 || sigma_a != sigma_a) return set_error(-2, "invalid shape or sigma_a");
  if (n_veh == 0 || n_steps == 0) return 0;
  if (!peaks || !count || !x_sel || !veh_base || !veh_states) return set_error(-2, "null pointer argument");
  hipLaunchKernelGGL(kf_track_kernel, dim3((unsigned)((n_veh + kKfBlock - 1) / kKfBlock)), dim3(kKfBlock), 0,
                     (hipStream_t)stream, peaks, cap, count, n_steps, x_sel, veh_base, n_veh, sigma_a, veh_states);
  return last_launch();
}
