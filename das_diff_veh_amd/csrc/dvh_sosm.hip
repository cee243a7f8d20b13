// The matrix-pipe form of sosfiltfilt on MI355X (gfx950): the operator table (the plan), the tile kernels, the three
// state scans, and the plan / run functions that dvh_sos.hip calls (declared in sos_common.h).  No entry point lives
// here: dvh_sos.hip holds them and the choice between this form and the block recursion.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dvh_common.h"
#include "sos_common.h"

namespace dvh {

// ---------------------------------------------------------------------------------------------
// sosfiltfilt on the float64 matrix pipe (round 5).  With blocks of kSmL = 64 samples the phases A and C of the block
// recursion (dvh_sos.hip) are GEMMs whose operands are the block's samples and the filter's block operators, formed on the device from the
// filter's own recursion (sosm_mats_kernel):
//   h[t]       the cascade's impulse response (zero state, unit sample at step 0), t < L
//   Hm[t][m]   its output at step t from the unit state e_m and zero input
//   g[t][m]    its state after step t from the unit sample at step 0 (zero state)
//   M = A^L    the zero-input transition of L samples, Mzi = M zi, MQ = M^Q (the scan's group transition)
// A block of L samples u_0..u_{L-1} filtered from start state s gives
//   outputs   y_i = sum_{j <= i} h[i - j] u_j + sum_m Hm[i][m] s_m            (lower-triangular Toeplitz + L x 2NS)
//   end state s' = M s + sum_j g[L - 1 - j] u_j                                 (2NS x L)
// and the backward pass over the reversed forward output, in forward indexing i of the same block (backward
// blocks aligned with the forward ones; the partial last forward block is the first backward block):
//   outputs   v_i = sum_{i'' >= i} h[i'' - i] y_i'' + sum_m Hm[L - 1 - i][m] s_m  (upper-triangular Toeplitz)
//   end state s' = M s + sum_i g[i] y_i
// The products are v_mfma_f64_16x16x4_f64 tiles over 16 blocks (columns, 1 024 samples).  A tile's samples are moved
// by coalesced loads (issued one tile ahead, under the previous tile's MFMAs) into an LDS image [block][sample]
// (row stride 65 doubles: the B-operand reads are conflict-free), and its outputs leave through the same image by
// coalesced stores.  The GEMMs fed from the image take their k index in the order sample = 16 (l >> 4) + kk, those
// fed from accumulators (the backward end states) in the accumulator order sample = 4 kk + (l >> 4); the operator
// (A) values are read from small LDS tables (h zero-extended for the Toeplitz factors, Hm, g) by lane-constant
// offsets.  Launches:
//   sosm_mats   the operators (one wave per record)
//   sosm_fa     forward zero-state end states E_f (block 0 plus M zi x_ext[0]: its true end state)
//   sosm_scan   true forward end states (two-level, below)
//   sosm_fc     forward outputs y from the true start states, written once, and from the same accumulators the
//               backward zero-state end states E_b of every full block (the backward phase A, fused)
//   sosm_bf     the first backward block (the partial last forward block) by the recursion, one lane per row
//   sosm_scan   true backward end states
//   sosm_bc     backward outputs from the true start states, trimmed into the row
// The outputs equal the recursion's up to rounding (sums of <= 84 products per output instead of the cascade's chain;
// a float64 model of this scheme matches scipy.signal.sosfiltfilt to 1e-13); tests/test_prep_gpu.py holds them to
// scipy at 1e-10 (float64) / 2e-6 (float32).
constexpr int kSmL = 64;     // samples per block: four 16-row MFMA tiles
constexpr int kSmLd = 65;  // LDS image row stride (doubles), odd: the B-operand reads (column li, sample 4 kk + q),
                           // which the compiler pairs into ds_read2_b64 (16-lane groups, 32 banks), and the
                           // accumulator stores (ds_write_b64, 16-lane groups) of the 16 columns land on 16 distinct
                           // bank pairs (at 66 they fell on 8: 2-way conflicts; conflict cycles per LDS instruction
                           // fa / fc / bc 1.73 / 3.44 / 2.51 -> 0.23 / 0.22 / 0.15, profiles/r6_pmc_prep_sosm.json)
constexpr int kSmOcc = 3;  // sosm_fa / sosm_bc: waves per SIMD the registers are sized for (their LDS allows 3 blocks
                           // of 4 waves per CU; sosm_fc's 65 KB and 220 registers hold it at 2)
constexpr int kSmRows = 32;  // state rows of the MFMA tiles (2 NS <= 32)
typedef double doublex4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ doublex4_t mfma_f64x4(double a, double b, doublex4_t c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// offsets (doubles) of the filter operators in the MFMA path's table (the "plan")
template <int NS>
struct SosmMats {
  static constexpr int NST = 2 * NS;
  static constexpr int h = 0, Hm = kSmL, g = Hm + kSmL * NST, M = g + kSmL * NST, Mzi = M + NST * NST,
                       MQ = Mzi + NST, MQ16 = MQ + NST * NST, Qk = MQ16 + NST * NST, size = Qk + 2;
};
// + the key (Q, Q16) the group transitions MQ / MQ16 were formed for: a scan whose own Q differs (a plan built for
// another record length) uses a NaN transition, so that the mismatch shows in the output instead of a wrong filter
int64_t sosm_plan_doubles(int n_sec) {
  return kSmL + 2 * kSmL * (2 * n_sec) + 3 * (2 * n_sec) * (2 * n_sec) + 2 * n_sec + 2;
}
// M^Q from the plan for a scan of group length Q: NaN when the plan's key is another Q
template <int NS>
__device__ __forceinline__ double sosm_mq(const double* __restrict__ mats, bool q16, int32_t Q, int idx) {
  using O = SosmMats<NS>;
  const double v = mats[(q16 ? O::MQ16 : O::MQ) + idx];
  return mats[O::Qk + (q16 ? 1 : 0)] == (double)Q ? v : __builtin_nan("");
}

// Lanes e < NST: unit state e_e, zero input (Hm[:, e], M[:, e]); lane NST: zero state, unit sample (h, g).  Then
// Mzi = M zi, MQ = M^Q and MQ16 = M^Q16 by repeated products (threads (row, col) of the NST x NST result, LDS): the
// group transitions of the 8-group scans (sosm_scan_kernel, sosm_scanr_kernel) and the 16-group one (sosm_scanm).
// One thread per element of the products: 512 threads up to 11 sections (22 x 22), 1 024 above (32 x 32 at 16).
__host__ __device__ constexpr int sosm_mats_threads(int ns) { return 4 * ns * ns <= 512 ? 512 : 1024; }
template <int NS>
__global__ __launch_bounds__(sosm_mats_threads(NS)) void sosm_mats_kernel(const double* __restrict__ sos, const double* __restrict__ zi,
                                                        int32_t Q, int32_t Q16, double* __restrict__ mats) {
  using O = SosmMats<NS>;
  constexpr int NST = 2 * NS;
  static_assert(NST * NST <= sosm_mats_threads(NS), "one thread per element of the NST x NST products");
  __shared__ double P[NST * NST], R[NST * NST], M0[NST * NST];
  const int e = threadIdx.x;
  if (e <= NST) {
    SosCoef<NS> c;
    c.load(sos);
    double z0[NS], z1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      z0[s] = (2 * s == e) ? 1.0 : 0.0;
      z1[s] = (2 * s + 1 == e) ? 1.0 : 0.0;
    }
    for (int t = 0; t < kSmL; ++t) {
      const double o = c.step(z0, z1, (e == NST && t == 0) ? 1.0 : 0.0);
      if (e == NST) {
        mats[O::h + t] = o;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          mats[O::g + t * NST + 2 * s] = z0[s];
          mats[O::g + t * NST + 2 * s + 1] = z1[s];
        }
      } else {
        mats[O::Hm + t * NST + e] = o;
      }
    }
    if (e < NST) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        P[(2 * s) * NST + e] = z0[s];
        P[(2 * s + 1) * NST + e] = z1[s];
      }
    }
  }
  __syncthreads();
  const int row = e / NST, col = e % NST;
  const bool act = e < NST * NST;
  if (act) {
    mats[O::M + e] = P[e];
    M0[e] = P[e];
  }
  if (e < NST) {
    double a = 0.0;
    for (int j = 0; j < NST; ++j) a += P[e * NST + j] * zi[j];
    mats[O::Mzi + e] = a;
  }
  // M^q by binary powering: R *= P when the bit is set, P = P P (P restarts from M)
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
    if (act) {
      P[e] = M0[e];
      R[e] = row == col ? 1.0 : 0.0;  // R = M^0
    }
    for (int q = pass == 0 ? Q : Q16; q > 0; q >>= 1) {
      __syncthreads();
      if (q & 1) {
        double a = 0.0;
        if (act)
          for (int j = 0; j < NST; ++j) a += R[row * NST + j] * P[j * NST + col];
        __syncthreads();
        if (act) R[e] = a;
        __syncthreads();
      }
      if (q > 1) {
        double a = 0.0;
        if (act)
          for (int j = 0; j < NST; ++j) a += P[row * NST + j] * P[j * NST + col];
        __syncthreads();
        if (act) P[e] = a;
      }
    }
    __syncthreads();
    if (act) mats[(pass == 0 ? O::MQ : O::MQ16) + e] = R[e];
  }
  if (e < 2) mats[O::Qk + e] = (double)(e == 0 ? Q : Q16);
}

// sample i of row r of the forward pass's sequence: the odd extension of x (0 past n_ext)
template <typename T>
__device__ __forceinline__ double sosm_ext(const T* __restrict__ x, const SosGeom& G, int64_t r, int64_t i) {
  if (r >= G.n_rows || i >= G.n_ext) return 0.0;  // padding columns of a record's last tile: nothing to read
  const T* row = x + r * G.row_stride;
  const int64_t j = i - G.padlen;
  if (j >= 0 && j < G.n_t) return (double)row[j];
  if (j < 0) return 2.0 * (double)row[0] - (double)row[-j];
  return 2.0 * (double)row[G.n_t - 1] - (double)row[2 * (G.n_t - 1) - j];
}

// Operator tables in LDS, laid out so that the lane-constant A-operand reads of a 32-lane group spread over the banks
// (k index = sample 4 kk + q, or state KS q + q'):
//   hq[q][64 + d] = h[d] (0 for d < 0) and hr[q][64 + d] = h[-d], one copy per lane group q at stride 145: the
//     Toeplitz factors T[i][j] = h[i - j] = hq[q][64 + i - j] and U[i][j] = h[j - i] = hr[q][64 + i - j]
//   hm[i][m] = Hm[i][m], stride sosm_hm_ld: the 4 KS state slots a row is read at (KS = ceil(2 NS / 4) per lane
//     group; slots m >= 2 NS zero) and odd, 21 up to 10 sections, 33 at 16
//   ga[j][m] = g[L - 1 - j][m], stride 33;  gb[m][i] = g[i][m], stride 65  (rows m >= 2 NS zero)
constexpr int kHq = 145, kGaLd = 33, kGbLd = kSmLd;
__host__ __device__ constexpr int sosm_hm_ld(int nst) { return nst <= 20 ? 21 : (4 * ((nst + 3) / 4)) | 1; }
template <int NS>
__device__ __forceinline__ void sosm_tables(const double* __restrict__ mats, double* hq, double* hr, double* hm, double* ga,
                                            double* gb) {
  using O = SosmMats<NS>;
  constexpr int NST = 2 * NS, kHmLd = sosm_hm_ld(NST);
  static_assert(kHmLd >= 4 * ((NST + 3) / 4) && NST <= kSmRows && NST < kGaLd, "operator tables narrower than the state");
  for (int v = threadIdx.x; v < 4 * kHq; v += blockDim.x) {
    const int d = v % kHq - kSmL;
    if (hq) hq[v] = (d >= 0 && d < kSmL) ? mats[O::h + d] : 0.0;
    if (hr) hr[v] = (d <= 0 && -d < kSmL) ? mats[O::h - d] : 0.0;
  }
  if (hm)
    for (int v = threadIdx.x; v < kSmL * kHmLd; v += blockDim.x) {
      const int i = v / kHmLd, m = v % kHmLd;
      hm[v] = m < NST ? mats[O::Hm + i * NST + m] : 0.0;
    }
  if (ga)
    for (int v = threadIdx.x; v < kSmL * kGaLd; v += blockDim.x) {
      const int j = v / kGaLd, m = v % kGaLd;
      ga[v] = m < NST ? mats[O::g + (kSmL - 1 - j) * NST + m] : 0.0;
    }
  if (gb)
    for (int v = threadIdx.x; v < kSmRows * kGbLd; v += blockDim.x) {
      const int m = v / kGbLd, i = v % kGbLd;
      gb[v] = (m < NST && i < kSmL) ? mats[O::g + i * NST + m] : 0.0;
    }
}

// A tile: 16 consecutive columns c0 .. c0 + 15 of an [n_rows][ncpr] column grid (block k of row r = column r ncpr + k;
// 32-bit: the host checks n_rows * nb < 2^31).  Its 1 024 samples in registers: lane l, step u holds sample l of
// column u (the LDS image [column][sample] is filled from these).
struct SosmTile {
  int c0, r0, k0;
  bool one_row;  // all 16 columns in row r0
};
__device__ __forceinline__ SosmTile sosm_tile(int tile, int n_rows, int ncpr) {
  SosmTile t;
  t.c0 = tile * 16;
  t.r0 = t.c0 / ncpr;
  t.k0 = t.c0 - t.r0 * ncpr;
  t.one_row = t.k0 + 16 <= ncpr && t.r0 < n_rows;
  return t;
}
// (row, block) of column u of a tile
__device__ __forceinline__ void sosm_col(const SosmTile& t, int u, int ncpr, int& r, int& k) {
  if (t.one_row) {
    r = t.r0;
    k = t.k0 + u;
  } else {
    const int c = t.c0 + u;
    r = c / ncpr;
    k = c - r * ncpr;
  }
}

// forward sequence (odd extension of x) of a tile's columns (blocks of the ext, ncpr = nb), in two halves so that the
// loads of the next tile stay in flight under this tile's MFMAs: sosm_fetch_x issues them into registers of x's own
// type (the samples each lane's sample index reflects to, plus the two reflection centres, x[0] of the last column's
// row and x[n_t - 1] of the first's), sosm_expand_x forms the extension from them when the tile is consumed.  (A
// conversion or sum right after a load makes the compiler wait for it there: the prefetch would be a plain load.)
__device__ __forceinline__ bool sosm_interior(const SosGeom& G, const SosmTile& t) {  // all 16 columns inside x's row
  const int64_t e0 = (int64_t)t.k0 * kSmL;
  return t.one_row && e0 >= G.padlen && e0 + 16 * kSmL <= G.padlen + G.n_t;
}
template <typename T>
struct SosmXRaw {
  T v[16];
  T xl, xr;
};
template <typename T>
__device__ __forceinline__ void sosm_fetch_x(const T* __restrict__ x, const SosGeom& G, const SosmTile& t, int lane,
                                             SosmXRaw<T>& raw) {
  const int nr = (int)G.n_rows;
  {
    int rl, kl;
    sosm_col(t, 15, G.nb, rl, kl);
    raw.xl = x[(int64_t)min(rl, nr - 1) * G.row_stride];
    raw.xr = x[(int64_t)min(t.r0, nr - 1) * G.row_stride + G.n_t - 1];
  }
  if (sosm_interior(G, t)) {  // one contiguous run of x
    const T* p = x + (int64_t)t.r0 * G.row_stride + ((int64_t)t.k0 * kSmL - G.padlen) + lane;
#pragma unroll
    for (int u = 0; u < 16; ++u) raw.v[u] = p[64 * u];
  } else {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      int r, k;
      sosm_col(t, u, G.nb, r, k);
      const int64_t j = (int64_t)k * kSmL + lane - G.padlen;
      int64_t src = j < 0 ? -j : (j < G.n_t ? j : 2 * ((int64_t)G.n_t - 1) - j);
      src = src < 0 ? 0 : (src >= G.n_t ? G.n_t - 1 : src);  // past the extension: any valid sample (unused)
      raw.v[u] = x[(int64_t)min(r, nr - 1) * G.row_stride + src];
    }
  }
}
// the tile's extension samples from its fetched raw values; a column whose reflection centre is not in the raw set
// (a tile over more than two rows: records of under 16 blocks) reads x directly
template <typename T>
__device__ __forceinline__ void sosm_expand_x(const T* __restrict__ x, const SosGeom& G, const SosmTile& t, int lane,
                                              const SosmXRaw<T>& raw, double (&v)[16]) {
  if (sosm_interior(G, t)) {
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = (double)raw.v[u];
  } else {
    int rl, kl;
    sosm_col(t, 15, G.nb, rl, kl);
    const double xl = (double)raw.xl, xr = (double)raw.xr;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      int r, k;
      sosm_col(t, u, G.nb, r, k);
      const int64_t i = (int64_t)k * kSmL + lane, j = i - G.padlen;
      const double a = (double)raw.v[u];
      double e = 0.0;  // padding columns (r >= n_rows) and samples past the extension are zero, and read nothing
      if (r < G.n_rows && i < G.n_ext) {
        if (j >= 0 && j < G.n_t)
          e = a;
        else if (j < 0)
          e = r == rl ? 2.0 * xl - a : sosm_ext(x, G, r, i);
        else
          e = r == t.r0 ? 2.0 * xr - a : sosm_ext(x, G, r, i);
      }
      v[u] = e;
    }
  }
}

// forward output y of a tile's columns (ncpr = nb - 1: blocks k < nb - 1 of each row, all full)
__device__ __forceinline__ void sosm_load_y(const double* __restrict__ y, const SosGeom& G, const SosmTile& t, int lane,
                                            double (&v)[16]) {
  if (t.one_row) {  // one contiguous run of the row's y (every column a full block)
    const double* p = y + (int64_t)t.r0 * G.n_ext + (int64_t)t.k0 * kSmL + lane;
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[64 * u];
    return;
  }
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    int r, k;
    sosm_col(t, u, G.nb - 1, r, k);
    v[u] = r < G.n_rows ? y[(int64_t)r * G.n_ext + (int64_t)k * kSmL + lane] : 0.0;
  }
}

// register samples -> the wave's LDS image [column][sample]
__device__ __forceinline__ void sosm_to_lds(double* img, int lane, const double (&v)[16]) {
#pragma unroll
  for (int u = 0; u < 16; ++u) img[u * kSmLd + lane] = v[u];
}

// accumulator rows (row i = 16 t + 4 rr + (l >> 4) of column l & 15) -> the LDS image
__device__ __forceinline__ void sosm_acc_to_lds(double* img, int lane, const doublex4_t (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) img[(lane & 15) * kSmLd + 16 * t + 4 * rr + (lane >> 4)] = acc[t][rr];
}

// state accumulators (rows m = 16 t + 4 rr + (l >> 4)) -> the LDS image as [column][sosm_stp(NST)]: an odd row
// stride, so that the 16 columns of a write land in 16 distinct bank pairs (at NST = 20 they fell on 4: 4-way
// conflicts); element (column, m) is read back at sosm_sv(v) for v = column NST + m
__host__ __device__ constexpr int sosm_stp(int nst) { return nst | 1; }
template <int NST>
__device__ __forceinline__ int sosm_sv(int v) { return (v / NST) * sosm_stp(NST) + v % NST; }
template <int NST>
__device__ __forceinline__ void sosm_states_out(double* img, int lane, const doublex4_t (&e)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int m = 16 * t + 4 * rr + (lane >> 4);
      if (m < NST) img[(lane & 15) * sosm_stp(NST) + m] = e[t][rr];
    }
}

// B operand of k-step kk (sample 4 kk + q of column li) and the Toeplitz A operands
#define SOSM_B(kk) bsrc[4 * (kk)]

// Forward phase A: E_f[c] = G u_block for k < nb - 1 (block 0: + M zi u_0, its true end state).
template <typename T, int NS>
__global__ __launch_bounds__(256, kSmOcc) void sosm_fa_kernel(const T* __restrict__ x, SosGeom G, const double* __restrict__ mats,
                                                      double* __restrict__ Sf) {
  using O = SosmMats<NS>;
  constexpr int NST = 2 * NS;
  __shared__ double ga[kSmL * kGaLd], imgs[4][16 * kSmLd];
  sosm_tables<NS>(mats, nullptr, nullptr, nullptr, ga, nullptr);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* img = imgs[wave];
  const int q = lane >> 4, li = lane & 15;
  const int nr = (int)G.n_rows;
  const int n_tiles = (nr * G.nb + 15) / 16, stride = gridDim.x * 4;
  int tile = blockIdx.x * 4 + wave;
  // M zi rows m = 16 t + 4 rr + q of this lane (block 0's true end state adds M zi u_0)
  double mzi[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int m = 16 * t + 4 * rr + q;
      mzi[t][rr] = m < NST ? mats[O::Mzi + m] : 0.0;
    }
  SosmXRaw<T> raw;
  if (tile < n_tiles) sosm_fetch_x(x, G, sosm_tile(tile, nr, G.nb), lane, raw);
  for (; tile < n_tiles; tile += stride) {
    const SosmTile tl = sosm_tile(tile, nr, G.nb);
    {
      double v[16];
      sosm_expand_x(x, G, tl, lane, raw, v);
      wave_barrier_lds();
      sosm_to_lds(img, lane, v);
    }
    if (tile + stride < n_tiles) sosm_fetch_x(x, G, sosm_tile(tile + stride, nr, G.nb), lane, raw);  // next tile
    wave_barrier_lds();
    doublex4_t acc[2] = {doublex4_t{0.0, 0.0, 0.0, 0.0}, doublex4_t{0.0, 0.0, 0.0, 0.0}};
    const double* bsrc = img + li * kSmLd + q;               // B: sample 4 kk + q of column li
    const double* asrc = ga + q * kGaLd + li;  // A: G[16 t + li][4 kk + q] = ga[4 kk + q][16 t + li]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const double b = SOSM_B(kk);
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = mfma_f64x4(asrc[4 * kk * kGaLd + 16 * t], b, acc[t]);
    }
    // block 0 of a row: its true end state M zi u_0 + E (u_0: the column's sample 0, in the image)
    int r, k;
    sosm_col(tl, li, G.nb, r, k);
    const double u0 = (k == 0 && r < nr) ? img[li * kSmLd] : 0.0;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) acc[t][rr] += u0 * mzi[t][rr];
    wave_barrier_lds();
    sosm_states_out<NST>(img, lane, acc);
    wave_barrier_lds();
    // 16 x NST states, element v = column * NST + m; only full blocks (k < nb - 1) keep an end state
    if (tl.one_row && tl.k0 + 16 <= G.nb - 1) {  // one contiguous run of Sf
      double* sp = Sf + ((int64_t)tl.r0 * G.nb + tl.k0) * NST;
#pragma unroll
      for (int u = 0; u < (16 * NST + 63) / 64; ++u) {
        const int v = lane + 64 * u;
        if (v < 16 * NST) sp[v] = img[sosm_sv<NST>(v)];
      }
    } else {
#pragma unroll
      for (int u = 0; u < (16 * NST + 63) / 64; ++u) {
        const int v = lane + 64 * u;
        if (v < 16 * NST) {
          int rc, kc;
          sosm_col(tl, v / NST, G.nb, rc, kc);
          if (rc < nr && kc < G.nb - 1) Sf[((int64_t)rc * G.nb + kc) * NST + v % NST] = img[sosm_sv<NST>(v)];
        }
      }
    }
  }
}

// Forward phase C + backward phase A: y = T u + Hm s (s: the true start state, zi u_0 for block 0), then
// E_b = Gb y from the accumulators, stored at the backward block index nb - 1 - k (full blocks only).
template <typename T, int NS>
__global__ __launch_bounds__(256) void sosm_fc_kernel(const T* __restrict__ x, SosGeom G, const double* __restrict__ mats,
                                                      const double* __restrict__ zi, const double* __restrict__ Sf,
                                                      double* __restrict__ y, double* __restrict__ Sb) {
  constexpr int NST = 2 * NS, KS = (NST + 3) / 4, kHmLd = sosm_hm_ld(NST);
  __shared__ double hq[4 * kHq], hm[kSmL * kHmLd], gb[kSmRows * kGbLd], imgs[4][16 * kSmLd];
  sosm_tables<NS>(mats, hq, nullptr, hm, nullptr, gb);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* img = imgs[wave];
  const int q = lane >> 4, li = lane & 15;
  const int nr = (int)G.n_rows;
  const int n_tiles = (nr * G.nb + 15) / 16, stride = gridDim.x * 4;
  int tile = blockIdx.x * 4 + wave;
  // the start state of column li, states m = KS q + q' (q' < KS) in this lane: contiguous in Sf (raw loads, block 0's
  // zi u_0 formed at use, u_0 from the image)
  auto load_s = [&](const SosmTile& t, double (&s)[KS]) {
    int r, k;
    sosm_col(t, li, G.nb, r, k);
    const double* sp = Sf + ((int64_t)min(r, nr - 1) * G.nb + max(k - 1, 0)) * NST;
#pragma unroll
    for (int qq = 0; qq < KS; ++qq) s[qq] = sp[min(KS * q + qq, NST - 1)];
  };
  double zim[KS];
#pragma unroll
  for (int qq = 0; qq < KS; ++qq) zim[qq] = KS * q + qq < NST ? zi[KS * q + qq] : 0.0;
  SosmXRaw<T> raw;
  double ns[KS];
  if (tile < n_tiles) {
    const SosmTile t0 = sosm_tile(tile, nr, G.nb);
    sosm_fetch_x(x, G, t0, lane, raw);
    load_s(t0, ns);
  }
  for (; tile < n_tiles; tile += stride) {
    const SosmTile tl = sosm_tile(tile, nr, G.nb);
    {
      double v[16];
      sosm_expand_x(x, G, tl, lane, raw, v);
      wave_barrier_lds();
      sosm_to_lds(img, lane, v);
    }
    double sv[KS];
    {
      int r, k;
      sosm_col(tl, li, G.nb, r, k);
      const bool ok = r < nr;
      wave_barrier_lds();
      const double u0 = img[li * kSmLd];
#pragma unroll
      for (int qq = 0; qq < KS; ++qq) {
        const bool real = ok && KS * q + qq < NST;
        sv[qq] = !real ? 0.0 : (k == 0 ? zim[qq] * u0 : ns[qq]);
      }
    }
    if (tile + stride < n_tiles) {  // the next tile's samples and start states, in flight under this tile's MFMAs
      const SosmTile tn = sosm_tile(tile + stride, nr, G.nb);
      sosm_fetch_x(x, G, tn, lane, raw);
      load_s(tn, ns);
    }
    wave_barrier_lds();
    doublex4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = doublex4_t{0.0, 0.0, 0.0, 0.0};
    const double* bsrc = img + li * kSmLd + q;          // B: sample 4 kk + q of column li
    const double* tsrc = hq + q * kHq + kSmL + li - q;  // A: T[16 t + li][4 kk + q] = hq[q][64 + 16 t + li - 4 kk - q]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const double b = SOSM_B(kk);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (kk <= 4 * t + 3) acc[t] = mfma_f64x4(tsrc[16 * t - 4 * kk], b, acc[t]);  // the lower triangle's k-steps
    }
    const double* msrc = hm + li * kHmLd + KS * q;   // A: Hm[16 t + li][KS q + q']
#pragma unroll
    for (int qq = 0; qq < KS; ++qq)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma_f64x4(msrc[16 * t * kHmLd + qq], sv[qq], acc[t]);
    // backward zero-state end state Gb y: y (rows = samples) as the B operand straight from the accumulators
    // (register rr of tile t is k-step 4 t + rr: sample 16 t + 4 rr + q)
    doublex4_t e[2] = {doublex4_t{0.0, 0.0, 0.0, 0.0}, doublex4_t{0.0, 0.0, 0.0, 0.0}};
    const double* gsrc = gb + li * kGbLd + q;        // A: gb[16 t' + li][4 kk + q]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int t = 0; t < 2; ++t) e[t] = mfma_f64x4(gsrc[16 * t * kGbLd + 4 * kk], acc[kk >> 2][kk & 3], e[t]);
    // y through the image: coalesced row runs
    wave_barrier_lds();
    sosm_acc_to_lds(img, lane, acc);
    wave_barrier_lds();
    const bool full = tl.one_row && tl.k0 + 16 <= G.nb - 1;  // 16 full blocks of one row: plain runs
    if (full) {
      double* yp = y + (int64_t)tl.r0 * G.n_ext + (int64_t)tl.k0 * kSmL + lane;
#pragma unroll
      for (int u = 0; u < 16; ++u) yp[64 * u] = img[u * kSmLd + lane];
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        int r, k;
        sosm_col(tl, u, G.nb, r, k);
        const int64_t i = (int64_t)k * kSmL + lane;
        if (r < nr && i < G.n_ext) y[(int64_t)r * G.n_ext + i] = img[u * kSmLd + lane];
      }
    }
    // E_b of full blocks at backward index nb - 1 - k
    wave_barrier_lds();
    sosm_states_out<NST>(img, lane, e);
    wave_barrier_lds();
    if (full) {  // column c at backward index nb - 1 - k0 - c: descending runs of NST
      double* sp = Sb + ((int64_t)tl.r0 * G.nb + (G.nb - 1 - tl.k0)) * NST;
#pragma unroll
      for (int u = 0; u < (16 * NST + 63) / 64; ++u) {
        const int v = lane + 64 * u;
        if (v < 16 * NST) sp[v % NST - (v / NST) * NST] = img[sosm_sv<NST>(v)];
      }
    } else {
#pragma unroll
      for (int u = 0; u < (16 * NST + 63) / 64; ++u) {
        const int v = lane + 64 * u;
        if (v < 16 * NST) {
          int rc, kc;
          sosm_col(tl, v / NST, G.nb, rc, kc);
          if (rc < nr && kc < G.nb - 1) Sb[((int64_t)rc * G.nb + (G.nb - 1 - kc)) * NST + v % NST] = img[sosm_sv<NST>(v)];
        }
      }
    }
  }
}

// The first backward block (forward block nb - 1, P = n_ext - (nb - 1) L samples) by the recursion from zi y[-1],
// one lane per row: its outputs (trimmed) and the backward state after it (Sb[r][0]).  The block's samples are loaded
// 16 at a time ahead of the recursion that consumes them.
template <typename T, int NS>
__global__ __launch_bounds__(64) void sosm_bf_kernel(T* __restrict__ x, SosGeom G, const double* __restrict__ sos,
                                                     const double* __restrict__ zi, const double* __restrict__ y,
                                                     double* __restrict__ Sb) {
  constexpr int NST = 2 * NS;
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= G.n_rows) return;
  SosCoef<NS> c;
  c.load(sos);
  const double* yr = y + r * G.n_ext;
  const double ul = yr[G.n_ext - 1];
  double z0[NS], z1[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    z0[q] = zi[2 * q] * ul;
    z1[q] = zi[2 * q + 1] * ul;
  }
  const int64_t start = (int64_t)(G.nb - 1) * kSmL;
  double cur[16];
  for (int64_t i0 = G.n_ext - 1; i0 >= start; i0 -= 16) {
#pragma unroll
    for (int t = 0; t < 16; ++t) cur[t] = i0 - t >= start ? yr[i0 - t] : 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int64_t i = i0 - t;
      if (i >= start) {
        const double v = c.step(z0, z1, cur[t]);
        const int64_t j = i - G.padlen;
        if (j >= 0 && j < G.n_t) x[r * G.row_stride + j] = (T)v;
      }
    }
  }
  double* sb = Sb + r * G.nb * NST;
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    sb[2 * q] = z0[q];
    sb[2 * q + 1] = z1[q];
  }
}

// Backward phase C for backward blocks k' >= 1 (forward blocks k = nb - 1 - k' < nb - 1, columns (r, k) of an
// [n_rows][nb - 1] grid): v = U y + Hrev s with s the true backward state before the block, trimmed into the row.
template <typename T, int NS>
__global__ __launch_bounds__(256, kSmOcc) void sosm_bc_kernel(T* __restrict__ x, SosGeom G, const double* __restrict__ mats,
                                                      const double* __restrict__ y, const double* __restrict__ Sb) {
  constexpr int NST = 2 * NS, KS = (NST + 3) / 4, kHmLd = sosm_hm_ld(NST);
  __shared__ double hr[4 * kHq], hm[kSmL * kHmLd], imgs[4][16 * kSmLd];
  sosm_tables<NS>(mats, nullptr, hr, hm, nullptr, nullptr);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* img = imgs[wave];
  const int q = lane >> 4, li = lane & 15;
  const int nr = (int)G.n_rows, nc = G.nb - 1;
  const int n_tiles = (nr * nc + 15) / 16, stride = gridDim.x * 4;
  int tile = blockIdx.x * 4 + wave;
  auto load_s = [&](const SosmTile& t, double (&s)[KS]) {  // backward state before block k: Sb[r][nb - 2 - k]
    int r, k;
    sosm_col(t, li, nc, r, k);
    const bool ok = r < nr;
    const double* sp = Sb + ((int64_t)r * G.nb + (G.nb - 2 - k)) * NST;
#pragma unroll
    for (int qq = 0; qq < KS; ++qq) {
      const int m = KS * q + qq;
      s[qq] = (ok && m < NST) ? sp[m] : 0.0;
    }
  };
  double ny[16], ns[KS];
  if (tile < n_tiles) {
    const SosmTile t0 = sosm_tile(tile, nr, nc);
    sosm_load_y(y, G, t0, lane, ny);
    load_s(t0, ns);
  }
  for (; tile < n_tiles; tile += stride) {
    const SosmTile tl = sosm_tile(tile, nr, nc);
    double sv[KS];
#pragma unroll
    for (int qq = 0; qq < KS; ++qq) sv[qq] = ns[qq];
    wave_barrier_lds();
    sosm_to_lds(img, lane, ny);
    if (tile + stride < n_tiles) {
      const SosmTile tn = sosm_tile(tile + stride, nr, nc);
      sosm_load_y(y, G, tn, lane, ny);
      load_s(tn, ns);
    }
    wave_barrier_lds();
    doublex4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = doublex4_t{0.0, 0.0, 0.0, 0.0};
    const double* bsrc = img + li * kSmLd + q;          // B: sample 4 kk + q of column li
    const double* usrc = hr + q * kHq + kSmL + li - q;  // A: U[16 t + li][4 kk + q] = hr[q][64 + 16 t + li - 4 kk - q]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const double b = SOSM_B(kk);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (kk >= 4 * t) acc[t] = mfma_f64x4(usrc[16 * t - 4 * kk], b, acc[t]);  // the upper triangle's k-steps
    }
    const double* msrc = hm + (kSmL - 1 - li) * kHmLd + KS * q;  // A: Hm[L - 1 - (16 t + li)][KS q + q']
#pragma unroll
    for (int qq = 0; qq < KS; ++qq)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma_f64x4(msrc[-16 * t * kHmLd + qq], sv[qq], acc[t]);
    wave_barrier_lds();
    sosm_acc_to_lds(img, lane, acc);
    wave_barrier_lds();
    // v at ext index k L + i -> x[j = k L + i - padlen] when 0 <= j < n_t
    const int64_t j0 = (int64_t)tl.k0 * kSmL - G.padlen;
    if (tl.one_row && j0 >= 0 && j0 + 16 * kSmL <= G.n_t) {  // one contiguous run of x
      T* xp = x + (int64_t)tl.r0 * G.row_stride + j0 + lane;
#pragma unroll
      for (int u = 0; u < 16; ++u) xp[64 * u] = (T)img[u * kSmLd + lane];
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        int r, k;
        sosm_col(tl, u, nc, r, k);
        const int64_t j = (int64_t)k * kSmL + lane - G.padlen;
        if (r < nr && j >= 0 && j < G.n_t) x[(int64_t)r * G.row_stride + j] = (T)img[u * kSmLd + lane];
      }
    }
  }
}
#undef SOSM_B

// The state scan S[k] = S[k] + M S[k - 1], k = 1 .. K - 1 (K = nb - 1 end states; S[0] already true; S[k] holds
// the zero-state end state E[k] on entry), two-level: one 256-thread block per row, 8 half-waves (lane j = state
// component j; every row's block resident at once on a 1 024-row record).  The steps are cut into NG <= 8 groups of Q
// (q covers k in [1 + q Q, 1 + (q + 1) Q)):
//   1  every group runs the scan from a zero start (group 0 from S[0]): Z[k] = E[k] + M Z[k - 1] (into S[k]);
//   2  the carries, in order: C_q = Z[last of q] + M^Q C_{q - 1} (C_0 = Z[last of 0], already true);
//   3  every group q >= 1 adds the carried part: D = M D from D = C_{q - 1}, S[k] = Z[k] + D.
// 2 Q + NG dependent steps instead of K - 1 (record of 1 024 x 60 s: 68 instead of 235; 16 half-waves per row gave 46
// steps but two rounds of blocks).  A step is one LDS round trip: the state and the step's own operand come from the
// LDS in one batch of reads (the 16 steps' operands of a batch are staged there from HBM at once), its result goes
// to the LDS slot and to HBM by stores nothing waits for.  (Operands held in registers instead left room for two
// reads in flight: five round trips per step, 43 us per scan.)
constexpr int kScanHW = 8, kScanPF = 16;
__host__ __device__ constexpr int sosm_scan_q(int nb) { return nb > 2 ? (nb - 2 + kScanHW - 1) / kScanHW : 1; }
// the 16-group scan on the matrix pipe (sosm_scanm_kernel): its group length, at most kScanMQ steps
constexpr int kScanMG = 16, kScanMQ = 16;
__host__ __device__ constexpr int sosm_scan_q16(int nb) { return nb > 2 ? (nb - 2 + kScanMG - 1) / kScanMG : 1; }

template <int NS>
__global__ __launch_bounds__(32 * kScanHW, 4) void sosm_scan_kernel(SosGeom G, const double* __restrict__ mats, int32_t Q,
                                                        double* __restrict__ S) {
  using O = SosmMats<NS>;
  constexpr int NST = 2 * NS;
  __shared__ __attribute__((aligned(16))) double sv[kScanHW][32];
  __shared__ double zb[kScanHW][kScanPF][NST];  // the batch's operands, then its results
  __shared__ double carry[kScanHW][NST], zlast[kScanHW][NST];
  const int hw = threadIdx.x >> 5, j = threadIdx.x & 31;
  const bool act = j < NST;
  const int jc = act ? j : 0;
  double* Sr = S + (int64_t)blockIdx.x * G.nb * NST;
  const int K = G.nb - 1;
  const int k0 = 1 + hw * Q, k1 = min(1 + (hw + 1) * Q, K);  // this half-wave's group [k0, k1)
  const int ng = K > 1 ? (K - 1 + Q - 1) / Q : 0;              // non-empty groups
  // add + sum_i A[i] x_i (row j of the matrix), x from the LDS slot: every read of the step issued together
  auto matvec = [&](const double* A, double add) {
    wave_barrier_lds();
    const double2* v2 = reinterpret_cast<const double2*>(sv[hw]);
    double2 u[NST / 2];
#pragma unroll
    for (int i = 0; i < NST / 2; ++i) u[i] = v2[i];
    double pa[4] = {add, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NST / 2; ++i) {
      pa[(2 * i) & 3] += A[2 * i] * u[i].x;
      pa[(2 * i + 1) & 3] += A[2 * i + 1] * u[i].y;
    }
    return (pa[0] + pa[1]) + (pa[2] + pa[3]);
  };
  auto put = [&](double v) {
    wave_barrier_lds();
    sv[hw][j] = v;
  };
  double m[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) {
    const double v = mats[O::M + jc * NST + i];
    m[i] = act ? v : 0.0;
  }
  // rows kb .. kb + 15 of this group into zb[hw] (zeros past the group; loads unconditional, clamped, so that the
  // compiler issues them together instead of one under each lane test)
  auto stage = [&](int kb) {
    double v[kScanPF];
#pragma unroll
    for (int t = 0; t < kScanPF; ++t) v[t] = Sr[(int64_t)min(kb + t, K - 1) * NST + jc];
#pragma unroll
    for (int t = 0; t < kScanPF; ++t)
      if (act) zb[hw][t][j] = kb + t < k1 ? v[t] : 0.0;
  };
  // level 1: zero-start scans of the groups (group 0 from the true S[0]); every half-wave runs Q steps rounded up to
  // whole batches (steps past the group compute on zeros or run on past its end, and store nothing)
  {
    const double s0 = Sr[jc];
    put((hw == 0 && act) ? s0 : 0.0);
  }
  double zl = 0.0;
  for (int kb = k0; kb < k0 + Q; kb += kScanPF) {
    stage(kb);
#pragma unroll
    for (int t = 0; t < kScanPF; ++t) {
      const double z = matvec(m, act ? zb[hw][t][j] : 0.0);
      zl = kb + t == k1 - 1 ? z : zl;  // the group's last Z, for the carries
      put(z);
      if (act) zb[hw][t][j] = z;
      if (act && kb + t < k1) Sr[(int64_t)(kb + t) * NST + j] = z;
    }
  }
  if (act) zlast[hw][j] = zl;
  __syncthreads();
  // level 2: carries by one half-wave (M^Q rows from HBM: six steps)
  if (hw == 0) {
    double mq[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const double v = sosm_mq<NS>(mats, false, Q, jc * NST + i);
      mq[i] = act ? v : 0.0;
    }
    double c = act ? zlast[0][j] : 0.0;
    if (act) carry[0][j] = c;
    for (int g = 1; g + 1 < ng; ++g) {
      put(c);
      c = matvec(mq, act ? zlast[g][j] : 0.0);
      if (act) carry[g][j] = c;
    }
  }
  __syncthreads();
  // level 3: the carried part of groups q >= 1 (Z from the LDS when the group fits one batch, else from HBM again)
  if (hw >= 1 && hw < ng) {
    double d = act ? carry[hw - 1][j] : 0.0;
    for (int kb = k0; kb < k1; kb += kScanPF) {
      if (Q > kScanPF) stage(kb);
#pragma unroll
      for (int t = 0; t < kScanPF; ++t) {
        put(d);
        d = matvec(m, 0.0);
        if (act && kb + t < k1) Sr[(int64_t)(kb + t) * NST + j] = zb[hw][t][j] + d;
      }
    }
  }
}

// The same scan with the row's states resident in the LDS (records of up to kScanCap / NST end states: 240 blocks of
// 64 samples at NS = 10, 61 s at 250 Hz): the row's E[0 .. K) come in by one coalesced batch of 16-byte loads, level 1
// turns them into Z in place, level 3 stores S = Z + D straight from there.  HBM sees each state read once and written
// once (the staged kernel above reads E, writes Z, reads Z again and writes S: twice the bytes, in bursts that no
// step overlaps).
constexpr int kScanCap = 4800;  // doubles: 37.5 KB, with the carries and the broadcast slots 40 KB (4 rows per CU)
template <int NS>
__global__ __launch_bounds__(32 * kScanHW, 4) void sosm_scanr_kernel(SosGeom G, const double* __restrict__ mats,
                                                                    int32_t Q, double* __restrict__ S) {
  using O = SosmMats<NS>;
  constexpr int NST = 2 * NS;
  __shared__ __attribute__((aligned(16))) double zf[kScanCap];
  __shared__ __attribute__((aligned(16))) double sv[kScanHW][NST + (NST & 1)];
  __shared__ double carry[kScanHW][NST];
  const int hw = threadIdx.x >> 5, j = threadIdx.x & 31;
  const bool act = j < NST;
  const int jc = act ? j : 0;
  double* Sr = S + (int64_t)blockIdx.x * G.nb * NST;
  const int K = G.nb - 1;
  const int k0 = 1 + hw * Q, k1 = min(1 + (hw + 1) * Q, K);  // this half-wave's group [k0, k1)
  const int ng = K > 1 ? (K - 1 + Q - 1) / Q : 0;              // non-empty groups
  double m[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) {
    const double v = mats[O::M + jc * NST + i];
    m[i] = act ? v : 0.0;
  }
  // E[0 .. K) -> zf: K NST doubles by LDS-DMA (16 bytes per lane, no registers: M stays in them)
  {
    const int n16 = K * NST / 2;  // NST even
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = 0; c * 32 * kScanHW < n16; ++c) {
      const int e0 = c * 32 * kScanHW + w * 64, e = e0 + lane;
      if (e < n16)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Sr + 2 * e),
                                         (__attribute__((address_space(3))) void*)(zf + 2 * e0), 16, 0, 0);
    }
  }
  __syncthreads();
  // add + sum_i A[i] x_i, x = the NST doubles at xs (LDS, broadcast): every read of the step issued together
  auto matvec = [&](const double* A, const double* xs, double add) {
    const double2* v2 = reinterpret_cast<const double2*>(xs);
    double2 u[NST / 2];
#pragma unroll
    for (int i = 0; i < NST / 2; ++i) u[i] = v2[i];
    double pa[4] = {add, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NST / 2; ++i) {
      pa[(2 * i) & 3] += A[2 * i] * u[i].x;
      pa[(2 * i + 1) & 3] += A[2 * i + 1] * u[i].y;
    }
    return (pa[0] + pa[1]) + (pa[2] + pa[3]);
  };
  // level 1: Z[k] = E[k] + M Z[k - 1] in place (group 0 from the true S[0]; the others from zero: their first step
  // takes E alone, the product with the neighbouring group's row discarded)
#pragma unroll 1
  for (int k = k0; k < k1; ++k) {
    wave_barrier_lds();
    const double z = matvec(m, zf + (k - 1) * NST, zf[k * NST + jc]);
    const double e = zf[k * NST + jc];
    wave_barrier_lds();
    if (act) zf[k * NST + j] = (k == k0 && hw > 0) ? e : z;
  }
  __syncthreads();
  // level 2: the carries C_g (true state at the end of group g), in order, by one half-wave
  if (hw == 0) {
    double mq[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const double v = sosm_mq<NS>(mats, false, Q, jc * NST + i);
      mq[i] = act ? v : 0.0;
    }
    double c = act ? zf[(min(1 + Q, K) - 1) * NST + j] : 0.0;
    if (act) carry[0][j] = c;
#pragma unroll 1
    for (int g = 1; g + 1 < ng; ++g) {
      if (act) sv[0][j] = c;
      wave_barrier_lds();
      c = matvec(mq, sv[0], act ? zf[(min(1 + (g + 1) * Q, K) - 1) * NST + j] : 0.0);
      wave_barrier_lds();
      if (act) carry[g][j] = c;
    }
  }
  __syncthreads();
  // level 3: S[k] = Z[k] + M^(k - k0 + 1) C_(q - 1) for groups q >= 1, S[k] = Z[k] for group 0, stored to HBM (M
  // again from memory, L2-resident: holding it over level 2 beside M^Q would spill; the pointer is laundered so that
  // the compiler does not reuse the first loads' registers instead)
  const double* mats3 = mats;
  asm volatile("" : "+s"(mats3));
#pragma unroll
  for (int i = 0; i < NST; ++i) {
    const double v = mats3[O::M + jc * NST + i];
    m[i] = act ? v : 0.0;
  }
  double d = (hw >= 1 && hw < ng && act) ? carry[hw - 1][j] : 0.0;
#pragma unroll 1
  for (int k = k0; k < k1; ++k) {
    if (hw >= 1) {
      if (act) sv[hw][j] = d;
      wave_barrier_lds();
      d = matvec(m, sv[hw], 0.0);
      wave_barrier_lds();
    }
    if (act) Sr[(int64_t)k * NST + j] = zf[k * NST + j] + d;
  }
}

// The same scan on the float64 matrix pipe, one wave per row: its 16 groups of Q16 <= 16 blocks are the 16 columns
// of v_mfma_f64_16x16x4_f64 GEMMs, so a step of all 16 groups is M [NST x NST] times their states [NST x 16]: 2 row
// tiles x KS k-steps.  Lane l holds fragment kk of column c = l & 15, state row 4 kk + (l >> 4), which is at once the
// step's accumulator (tile kk / 4, register kk % 4) and the next step's B operand (k-step kk): the recurrence never
// leaves the registers (the LDS broadcast of the VALU scans was their bound).  Level 1 keeps every group's Z in
// registers (Q16 x KS doubles per lane), level 2 (the carries through M^Q16) runs on lanes 0 .. NST - 1 through the
// LDS, level 3 adds M^(s + 1) C to the registers' Z and stores S as it goes.  E is read once (all loads of a lane
// issued together at the start), S written once.  (Staging E and S through the LDS for whole-line transfers measured
// slower, 31.5 against 28.1 us: the stores no longer overlap the steps.)
template <int NS>
__global__ __launch_bounds__(64, 1) void sosm_scanm_kernel(SosGeom G, const double* __restrict__ mats, int32_t Q,
                                                          double* __restrict__ S) {
  using O = SosmMats<NS>;
  constexpr int NST = 2 * NS, KS = (NST + 3) / 4, TT = (NST + 15) / 16;
  __shared__ __attribute__((aligned(16))) double zl[kScanMG][NST + (NST & 1)];
  __shared__ __attribute__((aligned(16))) double carry[kScanMG][NST + (NST & 1)];
  __shared__ __attribute__((aligned(16))) double slot[NST + (NST & 1)];
  const int l = threadIdx.x, c = l & 15, q4 = l >> 4;
  double* Sr = S + (int64_t)blockIdx.x * G.nb * NST;
  const int K = G.nb - 1;
  const int k0 = 1 + c * Q, k1 = min(1 + (c + 1) * Q, K);  // group c = [k0, k1)
  const int len = max(k1 - k0, 0);
  const int ng = K > 1 ? (K - 1 + Q - 1) / Q : 0;
  // A operands: M[16 t + c][4 kk + q4] (zero outside NST x NST)
  double a[TT][KS];
#pragma unroll
  for (int t = 0; t < TT; ++t)
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int r = 16 * t + c, k = 4 * kk + q4;
      const double v = mats[O::M + min(r, NST - 1) * NST + min(k, NST - 1)];
      a[t][kk] = (r < NST && k < NST) ? v : 0.0;
    }
  // E of every step of the group, fragment kk = row 4 kk + q4 (rows past NST and steps past the group: any finite
  // value of the row, never used)
  double z[kScanMQ][KS];
#pragma unroll
  for (int st = 0; st < kScanMQ; ++st)
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int k = min(k0 + st, K - 1), r = min(4 * kk + q4, NST - 1);
      z[st][kk] = Sr[(int64_t)k * NST + r];
    }
  double b[KS];  // the state entering the step (B operand): S[0] for group 0, zero for the others
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    const double v = Sr[min(4 * kk + q4, NST - 1)];
    b[kk] = (c == 0 && 4 * kk + q4 < NST) ? v : 0.0;
  }
  auto step = [&](double (&v)[KS], const double* cin) {  // v = cin + M b (cin: KS fragments, or zero), b = v
    doublex4_t acc[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) acc[t][rr] = (cin && 4 * t + rr < KS) ? cin[4 * t + rr] : 0.0;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
      for (int t = 0; t < TT; ++t) acc[t] = mfma_f64x4(a[t][kk], b[kk], acc[t]);
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      v[kk] = acc[kk >> 2][kk & 3];
      b[kk] = v[kk];
    }
  };
  // level 1: Z in place of E
#pragma unroll
  for (int st = 0; st < kScanMQ; ++st)
    if (st < Q) step(z[st], z[st]);
  // the groups' last Z -> LDS
#pragma unroll
  for (int st = 0; st < kScanMQ; ++st)
    if (st == len - 1)
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
        if (4 * kk + q4 < NST) zl[c][4 * kk + q4] = z[st][kk];
  __syncthreads();
  // level 2: C_0 = Z_last(0), C_g = Z_last(g) + M^Q16 C_(g - 1), lanes j < NST
  if (l < NST) {
    double mq[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) mq[i] = sosm_mq<NS>(mats, true, Q, l * NST + i);
    double cv = zl[0][l];
    carry[0][l] = cv;
    for (int g = 1; g + 1 < ng; ++g) {
      slot[l] = cv;
      wave_barrier_lds();
      double acc = zl[g][l];
#pragma unroll
      for (int i = 0; i < NST; ++i) acc += mq[i] * slot[i];
      wave_barrier_lds();
      cv = acc;
      carry[g][l] = cv;
    }
  }
  __syncthreads();
  // level 3: D = M^(s + 1) C_(c - 1) (zero for group 0), S = Z + D
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    const int r = 4 * kk + q4;
    const double v = carry[c > 0 ? c - 1 : 0][min(r, NST - 1)];
    b[kk] = (c > 0 && c < ng && r < NST) ? v : 0.0;
  }
#pragma unroll
  for (int st = 0; st < kScanMQ; ++st) {
    if (st < Q) {
      double d[KS];
      step(d, nullptr);
      if (st < len)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
          if (4 * kk + q4 < NST) Sr[(int64_t)(k0 + st) * NST + 4 * kk + q4] = z[st][kk] + d[kk];
    }
  }
}

template <int NS>
static void sosm_scan(const SosGeom& G, const double* plan, int Q, double* S, hipStream_t st) {
  if (G.nb <= 2) return;
  if (sosm_scan_q16(G.nb) <= kScanMQ)  // the matrix-pipe scan where its 16 groups of <= 16 blocks cover the row
    hipLaunchKernelGGL(sosm_scanm_kernel<NS>, dim3((unsigned)G.n_rows), dim3(64), 0, st, G, plan,
                       (int32_t)sosm_scan_q16(G.nb), S);
  else if ((int64_t)(G.nb - 1) * 2 * NS <= kScanCap)
    hipLaunchKernelGGL(sosm_scanr_kernel<NS>, dim3((unsigned)G.n_rows), dim3(32 * kScanHW), 0, st, G, plan, Q, S);
  else
    hipLaunchKernelGGL(sosm_scan_kernel<NS>, dim3((unsigned)G.n_rows), dim3(32 * kScanHW), 0, st, G, plan, Q, S);
}

SosGeom sosm_geom(int64_t n_rows, int64_t row_stride, int32_t n_t, int32_t padlen) {
  return sos_geom_of(n_rows, row_stride, n_t, padlen, kSmL);
}

// workspace of the MFMA path: y [n_rows][n_ext] + Sf, Sb [n_rows][nb][2 n_sec] + the plan (operator table), doubles
int64_t sosm_workspace_doubles(const SosGeom& G, int n_sec) {
  const int64_t nst = 2 * n_sec;
  return ((G.n_rows * G.n_ext + 1) & ~1LL) + 2 * G.n_rows * G.nb * nst + sosm_plan_doubles(n_sec);  // Sf 16-byte aligned
}
// the MFMA path's column indices are 32-bit
bool sosm_fits(const SosGeom& G) { return G.n_rows * (int64_t)G.nb < (1LL << 31) - 16; }

template <int NS>
static void sosm_plan(const double* sos, const double* zi, const SosGeom& G, double* plan, hipStream_t st) {
  hipLaunchKernelGGL(sosm_mats_kernel<NS>, dim3(1), dim3(sosm_mats_threads(NS)), 0, st, sos, zi, (int32_t)sosm_scan_q(G.nb),
                     (int32_t)sosm_scan_q16(G.nb), plan);
}

template <typename T, int NS>
static int sosm_run(T* x, const SosGeom& G, const double* sos, const double* zi, const double* plan, double* work,
                    hipStream_t st) {
  constexpr int NST = 2 * NS;
  double* y = work;
  double* Sf = y + ((G.n_rows * G.n_ext + 1) & ~1LL);  // 16-byte aligned (the scans' 16-byte loads)
  double* Sb = Sf + G.n_rows * G.nb * NST;
  const int Q = sosm_scan_q(G.nb);
  // persistent grids: the blocks that are resident at once (LDS and registers), each wave looping over tiles, so
  // that every block forms its operator tables once for many tiles
  const int64_t tiles = (G.n_rows * G.nb + 15) / 16;
  static int occ_fa = 0, occ_fc = 0, occ_bc = 0;  // blocks per CU of each kernel, queried once
  auto resident = [](int& occ, const void* fn) {
    if (!occ && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 256, 0) != hipSuccess || occ <= 0)) occ = 1;
    return (unsigned)(occ * cu_count());
  };
  auto grid_of = [](int64_t tiles_, unsigned res) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles_ + 3) / 4, res)); };
  const unsigned gfa = grid_of(tiles, resident(occ_fa, (const void*)sosm_fa_kernel<T, NS>));
  const unsigned gfc = grid_of(tiles, resident(occ_fc, (const void*)sosm_fc_kernel<T, NS>));
  if (G.nb > 1) hipLaunchKernelGGL((sosm_fa_kernel<T, NS>), dim3(gfa), dim3(256), 0, st, (const T*)x, G, plan, Sf);
  sosm_scan<NS>(G, plan, Q, Sf, st);
  hipLaunchKernelGGL((sosm_fc_kernel<T, NS>), dim3(gfc), dim3(256), 0, st, (const T*)x, G, plan, zi,
                     (const double*)Sf, y, Sb);
  hipLaunchKernelGGL((sosm_bf_kernel<T, NS>), dim3((unsigned)((G.n_rows + 63) / 64)), dim3(64), 0, st, x, G, sos, zi,
                     (const double*)y, Sb);
  if (G.nb > 1) {
    sosm_scan<NS>(G, plan, Q, Sb, st);
    const int64_t tb = (G.n_rows * (G.nb - 1) + 15) / 16;
    const unsigned gbc = grid_of(tb, resident(occ_bc, (const void*)sosm_bc_kernel<T, NS>));
    hipLaunchKernelGGL((sosm_bc_kernel<T, NS>), dim3(gbc), dim3(256), 0, st, x, G, plan, (const double*)y,
                       (const double*)Sb);
  }
  return last_launch();
}

int sosm_make_plan(const double* sos, int n_sec, const double* zi, const SosGeom& G, double* plan, hipStream_t st) {
  return with_section_count(n_sec, [&](auto ns) {
    sosm_plan<decltype(ns)::value>(sos, zi, G, plan, st);
    return 0;
  });
}

// plan == nullptr: formed into the workspace's tail first; else the caller's (dvh_sosfiltfilt_planned)
int sosm_filtfilt(void* x, int32_t dtype, const SosGeom& G, const double* sos, int n_sec, const double* zi,
                  const double* plan, double* work, hipStream_t st) {
  return with_float_type(dtype, [&](auto t) {
    using T = decltype(t);
    return with_section_count(n_sec, [&](auto ns) {
      constexpr int NS = decltype(ns)::value;
      const double* p = plan;
      if (!p) {
        double* tail = work + ((G.n_rows * G.n_ext + 1) & ~1LL) + 2 * G.n_rows * G.nb * (2 * NS);
        sosm_plan<NS>(sos, zi, G, tail, st);
        p = tail;
      }
      return sosm_run<T, NS>((T*)x, G, sos, zi, p, work, st);
    });
  });
}

}  // namespace dvh
