// Ridge walk on the phase-shift transform, evaluated in place, on MI355X (gfx950): extract_ridge_ref_idx
// (modules/utils.py:621-678) over the image map_fv_FD_slant_stack would give, without forming the image.
//
// A walk step compares the velocities inside (v_prev - sigma, v_prev + sigma) of one frequency column: 49-99 of the
// 1 000 rows of the notebooks' grid.  Each (f, v) value of the phase-shift image is an independent sum over the
// gather's rows, so the walk computes the values of the window it looks at and nothing else.
//
// One wave per (resample, walk), as ridge_kernel; the walk itself is ridge_walk's (ridge_walk.h), this file is its
// column source.  Per column: the lanes take the window's velocities in rounds of 64, each lane one pair through
// slant_pair (slant_pair.h), the arithmetic of dvh_disp_slant: a compared value equals, bit for bit, what the image
// kernels store for the same D.  The column's n_row spectrum values are the same for every lane: they sit in LDS (one
// 16-byte broadcast read per row), double-buffered; the walk's order is fixed, so the next column's global loads
// (lane r loads row r) are issued before the current column's sums and land in the other buffer after them.  The
// picks stay in LDS for the Savitzky-Golay finish.  LDS: 32 n_row + 8 nb bytes (1.5 KB at 19 rows x 116 columns).
//
// Compiled for gfx950: 154 VGPRs (32 of them the velocity axis VelAxis keeps in registers), 106 SGPRs, no scratch,
// 3 waves per SIMD.  Asking for 4 waves (128 VGPRs) spills 44 bytes per lane and was not kept.
//
// Measured (tools/bench_boot_slant.py, profiles/boot_slant.json): a convergence test of 1 800 resamples of 19 x 500 on
// 1 000 x 242, four modes (bands of 116, 50, 50, 40 columns): 2.27 ms with this kernel against 11.69 ms through
// stored images, the same ridges; the four launches take 0.27-1.07 ms each side by side (kernel trace), where the
// image kernel alone takes 9.83 ms and the four walks on it 0.14-0.42 ms.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "dvh_common.h"
#include "dvh.h"
#include "ridge_walk.h"
#include "slant_pair.h"

namespace dvh {

constexpr int kSrMaxRows = 1024;  // two column buffers of 16 KB beside 8 KB of picks: inside the 64 KB default

// The columns of the phase-shift image of one resample for ridge_walk, computed where the walk looks.
struct SlantColumns {
  const double2* Db;  // the resample's spectra [n_row][n_fb]
  int n_row, n_fb, c0, lane;
  const int32_t* __restrict__ fb;
  const double* __restrict__ freqs;
  const double* __restrict__ vel;
  double dx;
  double2* col;  // LDS [2][n_row]
  int cur;

  // row `lane` of band column i (the load that is issued ahead of the sums)
  __device__ __forceinline__ double2 fetch(int i) const {
    return lane < n_row ? Db[(int64_t)lane * n_fb + fb[c0 + i]] : make_double2(0.0, 0.0);
  }
  // band column i into buffer k: row `lane` from d0 = fetch(i), rows lane + 64, ... (gathers of more than 64 rows) here
  __device__ __forceinline__ void stash(int k, int i, double2 d0) {
    double2* c = col + k * n_row;
    if (lane < n_row) c[lane] = d0;
    for (int r = lane + 64; r < n_row; r += 64) c[r] = Db[(int64_t)r * n_fb + fb[c0 + i]];
  }
  __device__ __forceinline__ void first(int i) {
    cur = 0;
    stash(0, i, fetch(i));
    __syncthreads();
  }
  __device__ __forceinline__ int argmax(int i, int nxt, int r0, int r1) {
    double2 dn = make_double2(0.0, 0.0);
    if (nxt >= 0) dn = fetch(nxt);  // in flight during the sums below
    const double f = freqs[c0 + i];
    const double2* c = col + cur * n_row;
    float best = 0.f;
    int row = -1;
    for (int r = r0 + lane; r < r1; r += 64) {
      const float v = slant_pair(f, dx, vel[r], n_row, [c](int k) { return c[k]; });
      if (row < 0 || better(v, r, best, row)) {
        best = v;
        row = r;
      }
    }
    wave_argmax(best, row);
    if (nxt >= 0) stash(cur ^ 1, nxt, dn);
    __syncthreads();  // the other buffer is written, this one is read to the end
    cur ^= 1;
    return row;
  }
};

// One wave per resample b = blockIdx.x.  Dynamic LDS: double2 col[2][n_row], double pick[nb].
__global__ __launch_bounds__(64) void slant_ridge_kernel(const double2* __restrict__ D, int32_t n_row, int32_t n_fb,
                                                         const int32_t* __restrict__ fb,
                                                         const double* __restrict__ freqs, double dx, int32_t c0,
                                                         int32_t nb, const double* __restrict__ vel, int32_t nV,
                                                         int32_t ref, double sigma, double vel_max,
                                                         const double* __restrict__ vref,
                                                         const double* __restrict__ sg, int32_t sgl,
                                                         double* __restrict__ out, int32_t* __restrict__ status,
                                                         double* __restrict__ picks) {
  extern __shared__ double2 slant_ridge_lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  double* pick = reinterpret_cast<double*>(slant_ridge_lds + 2 * n_row);
  SlantColumns src{D + (int64_t)b * n_row * n_fb, n_row, n_fb, c0, lane, fb, freqs, vel, dx, slant_ridge_lds, 0};
  ridge_walk(src, b, lane, nV, nb, vel, ref, sigma, vel_max, vref, sg, sgl, out, status, picks, pick);
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_slant_ridge(const double* D, int32_t B, int32_t n_row, int32_t n_fb, const int32_t* fb,
                            const double* freqs, int32_t nF, double dx, int32_t c0, int32_t nb, const double* vel,
                            int32_t nV, int32_t ref, double sigma, double vel_max, const double* vref,
                            const double* sg, int32_t sgl, double* out, int32_t* status, double* picks,
                            void* stream) {
  if (!D || !fb || !freqs || !vel || !out || !status) return set_error(-2, "null pointer argument");
  if (B < 0 || n_row < 0 || nF < 0 || nV < 0) return set_error(-2, "negative count");
  if (n_fb <= 0) return set_error(-2, "n_fb must be positive");
  if (nb <= 0 || c0 < 0 || (int64_t)c0 + nb > nF || nV <= 0) return set_error(-2, "invalid band");
  if (nb > kMaxBand) return set_error(-4, "band longer than 1024 frequencies");
  if (n_row > kSrMaxRows) return set_error(-4, "more than 1024 rows");
  if (ref != INT32_MIN || vref) {
    if (!sg || sgl % 2 == 0 || sgl > nb) return set_error(-4, "savgol window must be odd and <= the band length");
    if (ref >= nb || ref < -nb) return set_error(-2, "reference index outside the band");
  }
  if (B == 0) return 0;
  const size_t lds = (size_t)2 * n_row * sizeof(double2) + (size_t)nb * sizeof(double);
  hipLaunchKernelGGL(slant_ridge_kernel, dim3((unsigned)B), dim3(64), lds, (hipStream_t)stream,
                     reinterpret_cast<const double2*>(D), n_row, n_fb, fb, freqs, dx, c0, nb, vel, nV, ref, sigma,
                     vel_max, vref, sg, sgl, out, status, picks);
  return last_launch();
}
