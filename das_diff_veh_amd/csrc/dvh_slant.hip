// Phase-shift (frequency-domain slant-stack) dispersion image on MI355X (gfx950): map_fv_FD_slant_stack of the
// reference (modules/utils.py:429-454), batched over gathers.
//
//   pout[f, v] = | sum_ix D[ix, f_idx(f)] * exp(+i 2 pi f (dx ix) / v) |,  D = fft(rows, n = nf) along time
// evaluated at the exact wavenumber k = f / v (map_fv samples a zero-padded k grid instead).  The time DFT at the
// bins the frequencies select is dvh_disp_tdft's; this file is the steering sum.  Everything is float64 -- sincos,
// the steering powers and the accumulation -- and the magnitude is rounded to float32 once, at the store.
//
// One lane per (f, v) pair, f fastest across the lanes: the D loads (16 B per lane) of neighbouring lanes fall into
// the same or the next bin and the fv stores are contiguous.  A lane builds w = exp(i theta), theta = 2 pi f dx / v,
// once, and its powers w^r by the recurrence w^r = w^(r-1) w; up to kSlRegRows rows the powers stay in registers and
// are reused by every gather of the lane's loop (4 FMAs per row and gather), above that the power runs inside the row
// loop (8 FMAs).  The rows are summed in ascending order by one lane, so an image does not depend on the batch it is
// part of or on the launch geometry.  Small f-v grids with many gathers split the gathers over gridDim.z.  The
// operations of one pair are slant_pair.h's, shared with the ridge walk that evaluates pairs in place
// (dvh_slant_ridge.hip) and must store the same bits.
//
// Measured (tools/bench_slant.py, DESIGN.md "Phase-shift dispersion"): 512 gathers of 19 rows on 512 x 1 000 pairs take
// 4.6 ms, 14-15 % of the float64 FMA floor (4.2 ms right after the time DFT wrote D).  The FMA pipe does not bound it:
// kernels with the same FMAs that read D differently took from 2.4 to 5.5 ms; what in the read path does has not been
// measured.  Two variants were timed, each in a run of its own, and not kept: the lanes' NR row offsets held as 32-bit
// registers beside the powers (5.5 ms at 124 VGPRs), and a per-block LDS copy of the columns the block's lanes share
// (3.5 ms there, but 53 us against 15 us on 3 gathers of 1 000 x 242).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <type_traits>

#include "dvh_common.h"
#include "dvh.h"
#include "slant_pair.h"

namespace dvh {

constexpr int kSlThreads = 256;
// Rows up to which the powers stay in registers (2 doubles = 4 VGPRs per row).  The compiled
// kernels take 94 VGPRs at 19 rows (5 waves per SIMD) and 124 at 21-24 rows (4 waves), none with scratch; the running
// power kernel takes 43 (8 waves).  The cut-over at 24 is the design's figure, not a measurement: only 19 rows have
// been timed.
constexpr int kSlRegRows = 24;
constexpr int kSlLoad = 8;      // rows loaded ahead of their FMAs (32 VGPRs)

struct SlantArgs {
  const double2* D;  // [B * nch][n_fb] complex
  int32_t B, nch, n_fb, row0, n_row;
  const int32_t* fb;
  const double* freqs;
  int32_t nF;
  const double* vels;
  int64_t n_pair, p0;
  double dx;
  float* fv;
  int64_t b_stride;
};

// (f, v) of the lane, exp(i theta) and the lane's column of D; false past the last pair.
__device__ __forceinline__ bool slant_lane(const SlantArgs& a, int64_t& p, double& c, double& s, const double2*& Dp) {
  p = a.p0 + (int64_t)blockIdx.x * kSlThreads + threadIdx.x;
  if (p >= a.n_pair) return false;
  const int64_t v = p / a.nF;
  const int32_t f = (int32_t)(p - v * a.nF);
  slant_steer(a.freqs[f], a.dx, a.vels[v], c, s);
  Dp = a.D + (int64_t)a.row0 * a.n_fb + a.fb[f];
  return true;
}

template <int NR>
__global__ __launch_bounds__(kSlThreads) void slant_reg_kernel(const SlantArgs a) {
  int64_t p;
  double c, s;
  const double2* Dp;
  if (!slant_lane(a, p, c, s, Dp)) return;
  double pr[NR], pi[NR];
  pr[0] = 1.0;
  pi[0] = 0.0;
#pragma unroll
  for (int r = 1; r < NR; ++r) slant_next_power(pr[r - 1], pi[r - 1], c, s, pr[r], pi[r]);
  const int64_t g_stride = (int64_t)a.nch * a.n_fb;
  for (int32_t b = blockIdx.z; b < a.B; b += gridDim.z) {
    const double2* Db = Dp + (int64_t)b * g_stride;
    double ar = 0.0, ai = 0.0;
    // kSlLoad rows' loads are issued before their FMAs, so their latencies overlap
#pragma unroll
    for (int r0 = 0; r0 < NR; r0 += kSlLoad) {
      double2 d[kSlLoad];
#pragma unroll
      for (int u = 0; u < kSlLoad; ++u)
        if (r0 + u < NR) d[u] = Db[(int64_t)(r0 + u) * a.n_fb];
#pragma unroll
      for (int u = 0; u < kSlLoad; ++u)
        if (r0 + u < NR) slant_add_row(d[u], pr[r0 + u], pi[r0 + u], ar, ai);
    }
    a.fv[(int64_t)b * a.b_stride + p] = slant_magnitude(ar, ai);
  }
}

// Any number of rows, 0 included (the sum is then empty and the image 0): the power runs with the row loop.
__global__ __launch_bounds__(kSlThreads) void slant_run_kernel(const SlantArgs a) {
  int64_t p;
  double c, s;
  const double2* Dp;
  if (!slant_lane(a, p, c, s, Dp)) return;
  const int64_t g_stride = (int64_t)a.nch * a.n_fb;
  for (int32_t b = blockIdx.z; b < a.B; b += gridDim.z) {
    const double2* Db = Dp + (int64_t)b * g_stride;
    double ar = 0.0, ai = 0.0, wr = 1.0, wi = 0.0;
    for (int r = 0; r < a.n_row; ++r) {
      slant_add_row(Db[(int64_t)r * a.n_fb], wr, wi, ar, ai);
      double nr, ni;
      slant_next_power(wr, wi, c, s, nr, ni);
      wr = nr;
      wi = ni;
    }
    a.fv[(int64_t)b * a.b_stride + p] = slant_magnitude(ar, ai);
  }
}

// The register-power kernel for n_row rows, 1 <= n_row <= kSlRegRows.
template <int N = 1>
const void* slant_reg_fn(int n_row) {
  if constexpr (N > kSlRegRows)
    return nullptr;
  else
    return n_row == N ? (const void*)slant_reg_kernel<N> : slant_reg_fn<N + 1>(n_row);
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_disp_slant(const double* D, int32_t B, int32_t nch, int32_t n_fb, int32_t row0, int32_t n_row,
                           const int32_t* fb, const double* freqs, int32_t nF, const double* vels, int32_t nV, double dx,
                           float* fv, int64_t b_stride, void* stream) {
  if (!D || !fb || !freqs || !vels || !fv) return set_error(-2, "null pointer argument");
  if (B < 0 || nch < 0 || row0 < 0 || n_row < 0 || nF < 0 || nV < 0) return set_error(-2, "negative count");
  if ((int64_t)row0 + n_row > nch) return set_error(-2, "rows [row0, row0 + n_row) leave the gather");
  if (n_fb <= 0) return set_error(-2, "n_fb must be positive");
  const int64_t n_pair = (int64_t)nF * nV;
  if (B > 1 && b_stride < n_pair) return set_error(-2, "images overlap: b_stride < nF * nV");
  if (B == 0 || n_pair == 0) return 0;
  const void* fn = (n_row >= 1 && n_row <= kSlRegRows) ? slant_reg_fn(n_row) : (const void*)slant_run_kernel;
  const int64_t gx = (n_pair + kSlThreads - 1) / kSlThreads;
  // fewer than 8 blocks per CU over the f-v grid alone: split the gathers over z (a lane's gathers z, z + gz, ...)
  int64_t gz = (8 * (int64_t)cu_count() + gx - 1) / gx;
  gz = gz < 1 ? 1 : gz;
  gz = gz > B ? B : gz;
  gz = gz > 65535 ? 65535 : gz;
  SlantArgs a{reinterpret_cast<const double2*>(D), B, nch, n_fb, row0, n_row, fb, freqs, nF, vels, n_pair, 0, dx, fv,
              b_stride};
  const int64_t max_x = 0x7fffffff;
  for (int64_t x0 = 0; x0 < gx; x0 += max_x) {  // f-v grids of more than 2^31 - 1 blocks: several launches
    const int64_t nx = gx - x0 < max_x ? gx - x0 : max_x;
    a.p0 = x0 * kSlThreads;
    void* args[] = {&a};
    if (int rc = hip_status(hipLaunchKernel(fn, dim3((unsigned)nx, 1, (unsigned)gz), dim3(kSlThreads), args, 0,
                                            (hipStream_t)stream)))
      return rc;
  }
  return 0;
}
