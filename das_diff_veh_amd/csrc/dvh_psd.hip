// Welch power spectra: scipy.signal.welch(x, fs, nperseg=P, nfft=F) with SciPy's defaults (periodic Hann window,
// noverlap = P / 2, detrend='constant', density scaling, one-sided) for float32 rows, averaged over the rows of a
// group (win_avg_psd, modules/utils.py:715-728; plot_psd_vs_offset, apis/virtual_shot_gather.py:45-89).
//
// Fast form, F in {256, 512, 1024, 2048, 4096}: one 64-lane wave owns a segment.  The raw segment goes to LDS by its
// logical sample index (16-byte loads where the address allows, single loads at an unaligned head and tail; the
// next segment's loads are in flight during the transform: a row's samples come once from HBM and once more from L2
// for the overlapping half), its mean is taken in float64, and the detrended, windowed samples are packed as z[n] = s[2n] + i s[2n+1] into one
// F / 2-point complex Stockham transform (fft_wave.h).  With A = Z[k], B = conj(Z[F/2 - k]), E = (A + B) / 2,
// O = -i (A - B) / 2 and w = exp(-2 pi i k / F) the real transform is X[k] = E + w O and X[F/2 - k] = conj(E - w O),
// so every lane forms a pair of bins.  The powers are summed in float64 registers over the wave's segments and rows.
// A 256-thread block owns up to kChunkRows rows of one group, wave v rows v, v + 4, ...; the four waves' sums are
// added in wave order, and a group of more rows leaves one partial per chunk that a second kernel adds in chunk
// order.  The order of every sum is therefore a function of the row's index in its group alone: a value does not
// depend on strides, alignment or the number of groups.
//
// Direct form, any other F (SciPy's clipped nperseg = n_t case): the segment is detrended and windowed in float64
// into LDS, and every thread sums one bin against the host's table exp(-2 pi i m / F), also in LDS.  All float64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dvh.h"
#include "dvh_common.h"
#include "fft_wave.h"

using dvh::set_error;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunkRows = 64;             // rows of a group one block sums
constexpr size_t kMaxLds = 160 * 1024;

struct Args {
  const float* x;
  int64_t group_stride, row_stride;
  const double* win;      // [P]
  const double2* tab;     // [F] (cos, -sin) of 2 pi m / F: the direct form
  double* out;            // [n_groups][F / 2 + 1]
  double* part;           // [n_groups][n_chunks][F / 2 + 1] when n_chunks > 1
  double scale;           // 1 / (fs sum win^2)
  int P, F, step, nseg, rows, n_chunks;
};

// The complex transform of the packed real one (the lengths fft_wave.h has no plan for are spelled out).
template <int N> struct HalfPlan { using T = typename dvh::FftPlan<N>::T; };
template <> struct HalfPlan<128> { using T = dvh::Stockham<128, 1, 4, 4, 4, 2>; };
template <> struct HalfPlan<256> { using T = dvh::Stockham<256, 1, 4, 4, 4, 4>; };

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

// The value of bin `bin` from the sum of |X|^2 over segments and rows: SciPy's scale, the one-sided fold (every bin
// but DC and, for even F, Nyquist is doubled) and the two means.
__device__ __forceinline__ double finish(double sum, int bin, const Args& a, bool bad) {
  if (bad) return __builtin_nan("");
  const bool single = bin == 0 || (a.F % 2 == 0 && bin == a.F / 2);
  return sum * (single ? a.scale : 2.0 * a.scale) / ((double)a.nseg * (double)a.rows);
}

// One segment on its way from global memory to LDS: IT 16-byte pieces per lane, held in registers so that a segment
// is requested before the transform of the one in front of it and written to LDS after it (the requests' latency
// hides behind that transform).  Whole 16-byte vectors inside the segment are loaded as such, an unaligned head and
// tail sample by sample; nothing outside [seg, seg + P) is read.  raw[e] receives sample e whatever the alignment.
template <int IT>
struct SegmentRegs {
  float4 q[IT];
  int mis;

  __device__ __forceinline__ void load(const float* __restrict__ seg, int P, int lane) {
    mis = (int)(((uintptr_t)seg >> 2) & 3);
    const int nvec = (mis + P + 3) >> 2;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int e = 4 * (lane + 64 * it) - mis;
      if (lane + 64 * it < nvec) {
        if (e >= 0 && e + 4 <= P) {
          q[it] = *(const float4*)(seg + e);
        } else {
          q[it].x = e >= 0 && e < P ? seg[e] : 0.f;
          q[it].y = e + 1 >= 0 && e + 1 < P ? seg[e + 1] : 0.f;
          q[it].z = e + 2 >= 0 && e + 2 < P ? seg[e + 2] : 0.f;
          q[it].w = e + 3 >= 0 && e + 3 < P ? seg[e + 3] : 0.f;
        }
      }
    }
  }

  __device__ __forceinline__ void store(float* raw, int P, int lane) const {
    const int nvec = (mis + P + 3) >> 2;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int e = 4 * (lane + 64 * it) - mis;
      if (lane + 64 * it < nvec) {
        if (mis == 0 && e + 4 <= P) {  // raw is 16-byte aligned
          *(float4*)(raw + e) = q[it];
        } else {
          if (e >= 0 && e < P) raw[e] = q[it].x;
          if (e + 1 >= 0 && e + 1 < P) raw[e + 1] = q[it].y;
          if (e + 2 >= 0 && e + 2 < P) raw[e + 2] = q[it].z;
          if (e + 3 >= 0 && e + 3 < P) raw[e + 3] = q[it].w;
        }
      }
    }
  }
};

template <int N>
constexpr size_t fft_lds_bytes() {
  return sizeof(float2) * (N + (N / 2 + 2) + (size_t)kWaves * 2 * N) + 16;
}

// N = F / 2.  LDS: twiddles of the N-point transform, exp(-2 pi i k / F) for k <= N / 2, two N-point buffers per
// wave, one flag per wave.
template <int N>
__global__ __launch_bounds__(kThreads) void welch_fft_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* tw = (float2*)smem;
  float2* twp = tw + N;
  float2* bufs = twp + (N / 2 + 2);
  int* flags = (int*)(bufs + kWaves * 2 * N);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int J = N / 128;  // bin pairs (k, N - k), k = lane + 64 j < N / 2, per lane

  dvh::init_twiddles<N>(tw);
  for (int k = tid; k <= N / 2; k += kThreads) {
    double s, c;
    sincospi((double)k / (double)N, &s, &c);
    twp[k] = make_float2((float)c, (float)(-s));
  }
  __syncthreads();

  float2* A = bufs + wave * 2 * N;
  float2* B = A + N;
  const int64_t g = blockIdx.x / a.n_chunks;
  const int chunk = blockIdx.x - (int)g * a.n_chunks;
  const int r0 = chunk * kChunkRows;
  const int r1 = r0 + kChunkRows < a.rows ? r0 + kChunkRows : a.rows;
  const int P = a.P;

  double lo[J], hi[J], mid = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j) lo[j] = hi[j] = 0.0;
  bool bad = false;

  // this wave's segments in order: rows r0 + wave, + kWaves, ..., each row's segments 0 .. nseg - 1
  const int n_tasks = r0 + wave < r1 ? ((r1 - r0 - wave + kWaves - 1) / kWaves) * a.nseg : 0;
  auto segment = [&](int t) {
    const int i = t / a.nseg, sg = t - i * a.nseg;
    return a.x + g * a.group_stride + (int64_t)(r0 + wave + kWaves * i) * a.row_stride + (int64_t)sg * a.step;
  };
  // The window samples this lane multiplies, 2 (lane + 64 i) and the next one, are the same for every segment: they
  // stay in registers, rounded to float32 like the products they form (the transform's input type).
  float2 wr[N / 64];
#pragma unroll
  for (int i = 0; i < N / 64; ++i) {
    const int e = 2 * (lane + 64 * i);
    wr[i] = make_float2(e < P ? (float)a.win[e] : 0.f, e + 1 < P ? (float)a.win[e + 1] : 0.f);
  }
  SegmentRegs<N / 128 + 1> regs;  // P <= 2 N samples at any alignment: at most N / 2 + 1 pieces
  if (n_tasks > 0) regs.load(segment(0), P, lane);
  for (int t = 0; t < n_tasks; ++t) {
    float* raw = (float*)B;  // 2 N floats: reads up to the next multiple of 4 past P stay inside, and are not used
    regs.store(raw, P, lane);
    dvh::wave_sync();
    double sum = 0.0;  // lane: samples 4 (lane + 64 i) .. + 3 in order, then the lanes by wave_sum
#pragma unroll 4
    for (int e = 4 * lane; e < P; e += 256) {
      const float4 r = *(const float4*)(raw + e);
      sum += (double)r.x;
      if (e + 1 < P) sum += (double)r.y;
      if (e + 2 < P) sum += (double)r.z;
      if (e + 3 < P) sum += (double)r.w;
    }
    const double mean = wave_sum(sum) / (double)P;
    bad |= !(mean - mean == 0.0);  // NaN or +-inf in the segment: SciPy's result is NaN in every bin
#pragma unroll
    for (int i = 0; i < N / 64; ++i) {
      const int n = lane + 64 * i, e = 2 * n;
      const float2 r = *(const float2*)(raw + e);
      const float re = e < P ? (float)(((double)r.x - mean) * (double)wr[i].x) : 0.f;
      const float im = e + 1 < P ? (float)(((double)r.y - mean) * (double)wr[i].y) : 0.f;
      A[n] = make_float2(re, im);
    }
    if (t + 1 < n_tasks) regs.load(segment(t + 1), P, lane);  // in flight during the transform
    dvh::wave_sync();
    const float2* Z = HalfPlan<N>::T::run(A, B, tw, lane);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int k = lane + 64 * j;
      const float2 zk = Z[k], zm = Z[(N - k) & (N - 1)], w = twp[k];
      const float ex = 0.5f * (zk.x + zm.x), ey = 0.5f * (zk.y - zm.y);
      const float ox = 0.5f * (zk.y + zm.y), oy = -0.5f * (zk.x - zm.x);
      const float tx = w.x * ox - w.y * oy, ty = w.x * oy + w.y * ox;
      const double px = (double)(ex + tx), py = (double)(ey + ty);
      const double qx = (double)(ex - tx), qy = (double)(ey - ty);
      lo[j] += px * px + py * py;
      hi[j] += qx * qx + qy * qy;
    }
    const float2 zh = Z[N / 2];
    mid += (double)zh.x * (double)zh.x + (double)zh.y * (double)zh.y;
    dvh::wave_sync();  // the next segment overwrites both buffers
  }

  // bins 0 .. N of this wave's sum into its own buffers, then the waves in order
  double* mine = (double*)A;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    mine[k] = lo[j];
    mine[N - k] = hi[j];
  }
  if (lane == 0) {
    mine[N / 2] = mid;
    flags[wave] = bad ? 1 : 0;
  }
  __syncthreads();
  const bool any_bad = (flags[0] | flags[1] | flags[2] | flags[3]) != 0;
  for (int bin = tid; bin <= N; bin += kThreads) {
    double v = ((const double*)bufs)[bin];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) v += ((const double*)(bufs + q * 2 * N))[bin];
    if (a.n_chunks == 1)
      a.out[g * (N + 1) + bin] = finish(v, bin, a, any_bad);
    else
      a.part[((int64_t)blockIdx.x) * (N + 1) + bin] = any_bad ? __builtin_nan("") : v;
  }
}

// out[g][bin] from the chunk partials, added in chunk order.
__global__ __launch_bounds__(kThreads) void welch_chunks_kernel(Args a) {
  const int bins = a.F / 2 + 1;
  const int64_t g = blockIdx.y;
  const int bin = blockIdx.x * kThreads + threadIdx.x;
  if (bin >= bins) return;
  const double* p = a.part + g * a.n_chunks * bins + bin;
  double v = p[0];
  for (int c = 1; c < a.n_chunks; ++c) v += p[(int64_t)c * bins];
  a.out[g * bins + bin] = finish(v, bin, a, false);  // a NaN partial stays NaN
}

__host__ __device__ constexpr size_t direct_lds_bytes(int P, int F) {
  return sizeof(double2) * (size_t)F + sizeof(double) * (size_t)(P + (P & 1)) + sizeof(double) * kWaves + 16;
}

// Block (tile, g): bins tile * 256 .. of group g.
__global__ __launch_bounds__(kThreads) void welch_direct_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double2* tab = (double2*)smem;
  double* v = (double*)(tab + a.F);
  double* red = v + a.P + (a.P & 1);
  int* flag = (int*)(red + kWaves);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = a.P, F = a.F, bins = F / 2 + 1;
  const int64_t g = blockIdx.y;
  const int bin = blockIdx.x * kThreads + tid;
  for (int m = tid; m < F; m += kThreads) tab[m] = a.tab[m];
  if (tid == 0) *flag = 0;
  double acc = 0.0;
  for (int r = 0; r < a.rows; ++r) {
    const float* row = a.x + g * a.group_stride + (int64_t)r * a.row_stride;
    for (int s = 0; s < a.nseg; ++s) {
      const float* seg = row + (int64_t)s * a.step;
      double sum = 0.0;
      for (int e = tid; e < P; e += kThreads) sum += (double)seg[e];
      sum = wave_sum(sum);
      __syncthreads();  // the last segment's sums are done with v and red
      if (lane == 0) red[wave] = sum;
      __syncthreads();
      const double mean = (((red[0] + red[1]) + red[2]) + red[3]) / (double)P;
      if (tid == 0 && !(mean - mean == 0.0)) *flag = 1;
      for (int e = tid; e < P; e += kThreads) v[e] = ((double)seg[e] - mean) * a.win[e];
      __syncthreads();
      if (bin < bins) {
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int n = 0; n < P; ++n) {
          const double2 t = tab[idx];
          re = __builtin_fma(v[n], t.x, re);
          im = __builtin_fma(v[n], t.y, im);
          idx += bin;
          if (idx >= F) idx -= F;
        }
        acc += re * re + im * im;
      }
    }
  }
  __syncthreads();
  if (bin < bins) a.out[g * bins + bin] = finish(acc, bin, a, *flag != 0);
}

bool fast_length(int F) { return F == 256 || F == 512 || F == 1024 || F == 2048 || F == 4096; }

int n_chunks_of(int rows) { return (rows + kChunkRows - 1) / kChunkRows; }

template <int N>
int launch_fft(const Args& a, int64_t n_groups, hipStream_t st) {
  constexpr size_t lds = fft_lds_bytes<N>();
  static_assert(lds <= kMaxLds, "LDS of one block");
  if (int rc = dvh::set_dynamic_lds((const void*)welch_fft_kernel<N>, lds)) return rc;
  welch_fft_kernel<N><<<dim3((unsigned)(n_groups * a.n_chunks)), dim3(kThreads), lds, st>>>(a);
  return dvh::last_launch();
}

}  // namespace

DVH_API int64_t dvh_welch_rows_workspace(int64_t n_groups, int32_t rows_per_group, int32_t nfft) {
  if (n_groups <= 0 || rows_per_group <= 0 || nfft <= 0 || !fast_length(nfft)) return 0;
  const int nc = n_chunks_of(rows_per_group);
  return nc == 1 ? 0 : (int64_t)sizeof(double) * n_groups * nc * (nfft / 2 + 1);
}

DVH_API int dvh_welch_rows(const float* x, int64_t n_groups, int64_t group_stride, int32_t rows_per_group,
                           int64_t row_stride, int32_t n_t, const double* win, int32_t nperseg, int32_t nfft,
                           double scale, const double* tab, double* out, void* ws, void* stream) {
  if (!x || !win || !out) return set_error(-2, "null pointer argument");
  if (n_groups < 0 || rows_per_group < 1 || n_t < 1) return set_error(-2, "invalid groups / rows / samples");
  if (nperseg < 1 || nperseg > n_t) return set_error(-4, "nperseg must be 1 .. n_t (the caller clips it as SciPy does)");
  if (nfft < nperseg) return set_error(-4, "nfft must be greater than or equal to nperseg");
  if (!(scale == scale)) return set_error(-2, "scale must be a number");
  if (rows_per_group > 1 && row_stride < n_t) return set_error(-2, "row stride shorter than a row");
  const int64_t group_span = (int64_t)(rows_per_group - 1) * (rows_per_group > 1 ? row_stride : 0) + n_t;
  if (n_groups > 1 && group_stride < group_span) return set_error(-2, "group stride shorter than a group");
  const bool fast = fast_length(nfft);
  if (!fast) {
    if (!tab) return set_error(-4, "this nfft takes the direct form, which needs the twiddle table");
    if ((uintptr_t)tab & 15) return set_error(-2, "the twiddle table must be 16-byte aligned");
    if (direct_lds_bytes(nperseg, nfft) > kMaxLds)
      return set_error(-4, "unsupported nfft: the direct form holds 16 nfft + 8 nperseg bytes in one block's LDS");
  }
  const int nc = fast ? n_chunks_of(rows_per_group) : 1;
  if (n_groups * nc > 0x7fffffffLL || ((!fast || nc > 1) && n_groups > 65535))
    return set_error(-4, "too many groups for one launch");
  if (n_groups == 0) return 0;
  const int bins = nfft / 2 + 1;
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out, wa = (uintptr_t)ws;
  const uintptr_t xe = xa + (uintptr_t)(((n_groups - 1) * (n_groups > 1 ? group_stride : 0) + group_span) * 4);
  const uintptr_t oe = oa + (uintptr_t)(n_groups * bins * 8);
  if (xa < oe && oa < xe) return set_error(-2, "x and out overlap");
  if (nc > 1) {
    if (!ws) return set_error(-2, "this many rows per group needs the workspace of dvh_welch_rows_workspace");
    const uintptr_t we = wa + (uintptr_t)(n_groups * nc * bins * 8);
    if ((xa < we && wa < xe) || (oa < we && wa < oe)) return set_error(-2, "the workspace overlaps x or out");
  }

  Args a;
  a.x = x;
  a.group_stride = n_groups > 1 ? group_stride : 0;
  a.row_stride = rows_per_group > 1 ? row_stride : 0;
  a.win = win;
  a.tab = (const double2*)tab;
  a.out = out;
  a.part = nc > 1 ? (double*)ws : nullptr;
  a.scale = scale;
  a.P = nperseg;
  a.F = nfft;
  const int noverlap = nperseg / 2;
  a.step = nperseg - noverlap;
  a.nseg = (n_t - noverlap) / a.step;
  a.rows = rows_per_group;
  a.n_chunks = nc;
  hipStream_t st = (hipStream_t)stream;
  if (!fast) {
    const size_t lds = direct_lds_bytes(nperseg, nfft);
    if (int rc = dvh::set_dynamic_lds((const void*)welch_direct_kernel, lds)) return rc;
    welch_direct_kernel<<<dim3((bins + kThreads - 1) / kThreads, (unsigned)n_groups), dim3(kThreads), lds, st>>>(a);
    return dvh::last_launch();
  }
  int rc = 0;
  switch (nfft) {
    case 256: rc = launch_fft<128>(a, n_groups, st); break;
    case 512: rc = launch_fft<256>(a, n_groups, st); break;
    case 1024: rc = launch_fft<512>(a, n_groups, st); break;
    case 2048: rc = launch_fft<1024>(a, n_groups, st); break;
    default: rc = launch_fft<2048>(a, n_groups, st); break;
  }
  if (rc || nc == 1) return rc;
  welch_chunks_kernel<<<dim3((bins + kThreads - 1) / kThreads, (unsigned)n_groups), dim3(kThreads), 0, st>>>(a);
  return dvh::last_launch();
}
