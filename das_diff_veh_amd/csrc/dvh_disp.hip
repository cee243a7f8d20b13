// Dispersion (f-v) image on MI355X (gfx950): map_fv of the reference, batched over gathers.
//
// Replaces fk (modules/utils.py:236-248) + map_fv (:457-475) + Dispersion (:383-426):
//   FK = |fftshift(fft2(data, s=[nk, nf]))| sampled bilinearly at (k = f / v, f) with the queries
//   clamped to the grid (interp2d(kind='linear') == FITPACK degree-1 spline), stored as float32,
//   then savgol_filter(25, 4, axis=0, mode='interp') along frequency, output [Nvel, Nfreq].
// Only the FK bins the queries touch are computed, as two GEMMs on the float64 MFMA pipe
// (v_mfma_f64_16x16x4_f64): |FK| then tracks the reference's float64 fft2 to ~1e-13, so the
// float32 f-v map (and its argmax pick) comes out as the reference's for exact inputs.
//   1. time DFT   D[r, q]  = sum_t data[r, t] * exp(-2 pi i nu_q t / nf)      (r = gather x channel)
//      real GEMM  [B*nch x nt] . [nt x 2*n_fb]  (cos | -sin float64 twiddles prepared on the host)
//   2. channel contraction  Z[m, q] = sum_x exp(-2 pi i kappa_m x / nk) D[x, q]  per gather,
//      complex GEMM as the real block GEMM [[Er, -Ei], [Ei, Er]] . [Dr; Di], then |Z| -> FK grid
//      (optionally accumulated per class slot with a weight: the f-v image is linear in |FK|)
//   3. f-v sampling: bilinear (FITPACK basis, double) -> float32 -> Savitzky-Golay operator (double)
// Steps 1 and 2 are here; step 3 is dvh_fv.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdlib.h>

#include "dvh_common.h"
#include "dvh.h"
#include "mfma_f64.h"

namespace dvh {

// ---------------------------------------------------------------------------------------------
// 1. time-DFT GEMM: C[r, n] = scale[r] * sum_k A[r, k] W[k, n]   (float64 MFMA, fp32 data)
// One wave per 32 x 32 output tile and K slice (split-K): the problem is small (tens of gather rows
// x a few hundred bins), so K is split to put hundreds of waves on the chip; the slices are summed
// with float64 atomics into C (zeroed by the launcher).
constexpr int kGT = 32;

__global__ __launch_bounds__(64) void tdft_gemm_kernel(const float* __restrict__ data, int64_t b_stride,
                                                        int64_t ch_stride, int32_t nch, int32_t M, int32_t K,
                                                        const double* __restrict__ W, int32_t N,
                                                        const float* __restrict__ row_scale, int32_t kslice,
                                                        double* __restrict__ C) {
  const int lane = threadIdx.x;
  const int m0 = blockIdx.y * kGT, n0 = blockIdx.x * kGT;
  const int k0 = blockIdx.z * kslice, k1 = min(K, k0 + kslice);
  const float* rowp[2];
  bool rok[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int r = m0 + f * 16 + (lane & 15);
    rok[f] = r < M;
    const int rr = rok[f] ? r : 0;
    rowp[f] = data + (int64_t)(rr / nch) * b_stride + (int64_t)(rr % nch) * ch_stride;
  }
  doublex4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = doublex4{0.0, 0.0, 0.0, 0.0};
  // kTU k-steps of 4 per round: all of the round's operand loads are issued before its MFMAs, so
  // their latency overlaps (one k-step at a time left the wave waiting on every load)
  constexpr int kTU = 4;
  for (int k = k0; k < k1; k += 4 * kTU) {
    double a[kTU][2], b[kTU][2];
#pragma unroll
    for (int u = 0; u < kTU; ++u) {
      const int kk = k + 4 * u + (lane >> 4);
      const bool kok = kk < k1;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        a[u][f] = (kok && rok[f]) ? (double)rowp[f][kk] : 0.0;
        const int c = n0 + f * 16 + (lane & 15);
        b[u][f] = (kok && c < N) ? W[(int64_t)kk * N + c] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < kTU; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_f64(a[u][i], b[u][j], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + i * 16 + (lane >> 4) + 4 * r;
        const int col = n0 + j * 16 + (lane & 15);
        if (row < M && col < N)
          atomicAdd(C + (int64_t)row * N + col, acc[i][j][r] * (row_scale ? (double)row_scale[row] : 1.0));
      }
}

// 1b. The same GEMM with the twiddle operand staged in LDS and reused across the rows of a block:
// a block (4 waves) owns 64 rows x kTdNT 16-column tiles; each wave 16 rows x all kTdNT tiles, so one A
// operand (the gather samples, float4 loads: lane (i, q) holds rows i, k = k0 + 8 q + s for the chunk's
// 8 k-steps s -- the same k permutation on both operands) feeds kTdNT MFMAs.  The block stages the
// twiddle chunk W[k0 .. k0 + 32)[c0 .. c0 + 16 kTdNT) by LDS-DMA (16 B per lane) into a double buffer,
// the next chunk's while this one is multiplied; chunk row 8 q + s sits in LDS row 4 s + q, so the four
// lane groups of one B-operand read hit rows next to each other (other bank halves), not 8 rows apart
// (the same banks; measured the same, 96-101 us either way).  No split-K: the tile is stored, not
// accumulated.  512 gathers of 25 x 500: 176 -> 96 us against the split-K kernel.
constexpr int kTdNT = 7;   // 16-column tiles per block (112 columns)
constexpr int kTdKC = 32;  // k per chunk
constexpr int kTdRows = 64;
// Small problems (a few class stacks: configs[1]'s six class images make a handful of blocks of the form above, each
// a chain of 32 chunk round trips, 56 us) split K over G wave groups of one block instead: group g multiplies the chunks
// kc = g (mod G), the groups' sums are added in group order through LDS (deterministic, no atomics); 2 tiles per
// block keep the 16-wave block within 128 VGPRs (4 tiles spilled 14).
constexpr int kTdNTs = 2, kTdGs = 4;

__host__ __device__ constexpr size_t tdft_rows_lds(int NT, int G) {
  // the groups' staging buffers, or (after the loop) their partial sums, whichever is larger
  return sizeof(double) * (size_t)G * ((size_t)2 * kTdKC * NT * 16 > (size_t)4 * NT * 4 * 64
                                           ? (size_t)2 * kTdKC * NT * 16
                                           : (size_t)4 * NT * 4 * 64);
}

template <int NT, int G>
__global__ __launch_bounds__(256 * G) void tdft_rows_kernel(const float* __restrict__ data, int64_t b_stride,
                                                            int64_t ch_stride, int32_t nch, int32_t M, int32_t K,
                                                            const double* __restrict__ W, int32_t N,
                                                            const float* __restrict__ row_scale, double* __restrict__ C) {
  extern __shared__ __attribute__((aligned(16))) double wsm_all[];  // per group [2][kTdKC][NT * 16]
  constexpr int NC = NT * 16, CH = kTdKC * NC;
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, grp = G > 1 ? (tid >> 8) : 0;
  double* wsm = wsm_all + (size_t)grp * 2 * CH;
  const int m0 = blockIdx.x * kTdRows + wave * 16, c0 = blockIdx.y * NC;
  const int li = lane & 15, q = lane >> 4;
  const int row = m0 + li;
  const bool rok = row < M;
  const float* rowp = data + (rok ? (int64_t)(row / nch) * b_stride + (int64_t)(row % nch) * ch_stride : 0);
  const bool vec4 = ((b_stride | ch_stride) & 3) == 0 && (reinterpret_cast<uintptr_t>(data) & 15) == 0;
  // LDS-DMA of twiddle chunk kc into buffer buf: doubles e = r * NC + c (linear), 2 per lane per piece
  const int n_chunk = (K + kTdKC - 1) / kTdKC;
  const int n_step = (n_chunk + G - 1) / G;  // every group runs n_step steps (the barriers), idle past n_chunk
  auto stage = [&](int kc, int buf) {
    if (kc >= n_chunk) return;
    for (int p = wave; p < CH / 128; p += 4) {
      const int e = p * 128 + 2 * lane;
      const int rho = e / NC, c = e - rho * NC;
      const int r = 8 * (rho & 3) + (rho >> 2);  // LDS row rho = 4 s + q holds chunk row k = 8 q + s
      const int kr = min(kc * kTdKC + r, K - 1), cc = min(c0 + c, N - 2);
      __builtin_amdgcn_global_load_lds((gbl_void*)(W + (int64_t)kr * N + cc), (lds_void*)(wsm + buf * CH + p * 128), 16,
                                       0, 0);
    }
  };
  // A operand of chunk kc: a[s] = data[row][k0 + 8 q + s] (0 past K or M)
  auto load_a = [&](int kc, double (&a)[8]) {
    const int kb = kc * kTdKC + 8 * q;
    if (vec4 && kb + 8 <= K && rok) {
      const float4 u = *reinterpret_cast<const float4*>(rowp + kb);
      const float4 v = *reinterpret_cast<const float4*>(rowp + kb + 4);
      a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w; a[4] = v.x; a[5] = v.y; a[6] = v.z; a[7] = v.w;
    } else {
#pragma unroll
      for (int s = 0; s < 8; ++s) a[s] = (rok && kb + s < K) ? (double)rowp[kb + s] : 0.0;
    }
  };
  doublex4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = doublex4{0.0, 0.0, 0.0, 0.0};
  double a[8];
  stage(grp, 0);
  load_a(grp, a);
  for (int st = 0; st < n_step; ++st) {
    const int kc = grp + G * st, kn = kc + G;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this chunk's twiddles have landed (and a)
    __syncthreads();  // ... for every wave; the other buffer's last readers are done
    double an[8];
    if (kn < n_chunk) {
      stage(kn, (st + 1) & 1);
      load_a(kn, an);
    }
    if (kc < n_chunk) {
      // rows beyond K in a partial chunk multiply a = 0 with finite (clamped) twiddles
      const double* Wc = wsm + (st & 1) * CH;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma_f64(a[s], Wc[(4 * s + q) * NC + t * 16 + li], acc[t]);
      }
    }
    if (kn < n_chunk) {
#pragma unroll
      for (int s = 0; s < 8; ++s) a[s] = an[s];
    }
  }
  if constexpr (G > 1) {  // group sums in group order: red[g][wave][t][r][lane]
    __syncthreads();       // every group's last chunk is read
    double* red = wsm_all;
    if (grp > 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(((size_t)grp * 4 + wave) * NT + t) * 256 + r * 64 + lane] = acc[t][r];
    }
    __syncthreads();
    if (grp > 0) return;
#pragma unroll
    for (int g = 1; g < G; ++g)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] += red[(((size_t)g * 4 + wave) * NT + t) * 256 + r * 64 + lane];
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = c0 + t * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = m0 + q + 4 * r;
      if (rr < M && col < N) C[(int64_t)rr * N + col] = acc[t][r] * (row_scale ? (double)row_scale[rr] : 1.0);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 2. channel contraction + magnitude (float64 MFMA).  A (host table, global/L2) is [2*MT][K2],
// K2 = 2*nch rounded up to a multiple of 4: rows [0, MT) give Re Z, rows [MT, 2MT) give Im Z.
// One block = (gather b, 32 f-bins).
constexpr int kFN = 32;

__global__ __launch_bounds__(256) void fk_contract_kernel(const double* __restrict__ D, int32_t nch, int32_t n_fb,
                                                           const double* __restrict__ Atab, int32_t MT, int32_t K2,
                                                           int32_t n_kb, double* __restrict__ FK,
                                                           const int32_t* __restrict__ slot,
                                                           const float* __restrict__ weight, int32_t n_slot) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int M2 = 2 * MT;
  double* Bs = sm;                      // [K2][kFN + 1]
  double* Cs = Bs + K2 * (kFN + 1);     // [M2][kFN + 1]
  const int b = blockIdx.y, q0 = blockIdx.x * kFN;
  const double* Db = D + (int64_t)b * nch * 2 * n_fb;
  for (int e = threadIdx.x; e < K2 * kFN; e += 256) {
    const int kk = e / kFN, n = e % kFN;
    const int q = q0 + n;
    double v = 0.0;
    if (q < n_fb && kk < 2 * nch) {
      const int x = kk < nch ? kk : kk - nch;
      v = Db[(int64_t)x * 2 * n_fb + 2 * q + (kk < nch ? 0 : 1)];
    }
    Bs[kk * (kFN + 1) + n] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_mt = M2 / 16, n_nt = kFN / 16;
  for (int t = wave; t < n_mt * n_nt; t += 4) {
    const int mt = t / n_nt, nt = t % n_nt;
    doublex4 acc = {0.0, 0.0, 0.0, 0.0};
    const double* arow = Atab + (int64_t)(mt * 16 + (lane & 15)) * K2;
    for (int kk = 0; kk < K2; kk += 4) {
      const double a = arow[kk + (lane >> 4)];
      const double bb = Bs[(kk + (lane >> 4)) * (kFN + 1) + nt * 16 + (lane & 15)];
      acc = mfma_f64(a, bb, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = mt * 16 + (lane >> 4) + 4 * r;
      Cs[row * (kFN + 1) + nt * 16 + (lane & 15)] = acc[r];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n_kb * kFN; e += 256) {
    const int m = e / kFN, n = e % kFN, q = q0 + n;
    if (q >= n_fb) continue;
    const double mag = hypot(Cs[m * (kFN + 1) + n], Cs[(MT + m) * (kFN + 1) + n]);
    if (slot) {
      const int sl = slot[b];
      if (sl >= 0 && sl < n_slot)  // the host rejects such slots; never write outside FK
        atomicAdd(FK + ((int64_t)sl * n_kb + m) * n_fb + q, mag * (double)weight[b]);
    } else {
      FK[((int64_t)b * n_kb + m) * n_fb + q] = mag;
    }
  }
}

// 2b. The same contraction for tables too large for one block's LDS (more than ~128 channels, or the full
// grid of the public fk() from 65 channels on): one block = (gather b, kFtM wavenumbers m, 32 f-bins).  It holds
// the Re and the Im rows of its m (rows m and MT + m of A) as 2 * kFtM / 16 x 2 MFMA tiles, four per wave,
// accumulated in registers while the channel dimension passes through LDS in chunks of kFtK rows of [Dr; Di].
// Each element is summed over k in the order of fk_contract_kernel.
constexpr int kFtM = 64;  // wavenumbers per block
constexpr int kFtK = 64;  // rows of [Dr; Di] per LDS chunk
constexpr int kFtT = 2 * (kFtM / 16) * (kFN / 16) / 4;  // MFMA tiles per wave

__global__ __launch_bounds__(256) void fk_contract_tiled_kernel(const double* __restrict__ D, int32_t nch, int32_t n_fb,
                                                                 const double* __restrict__ Atab, int32_t MT, int32_t K2,
                                                                 int32_t n_kb, int32_t n_ft, double* __restrict__ FK,
                                                                 const int32_t* __restrict__ slot,
                                                                 const float* __restrict__ weight, int32_t n_slot) {
  __shared__ double Bs[kFtK * (kFN + 1)];      // [kFtK][kFN + 1]
  __shared__ double Cs[2 * kFtM * (kFN + 1)];  // [Re rows | Im rows][kFN + 1]
  const int b = blockIdx.y, q0 = (blockIdx.x % n_ft) * kFN, m0 = (blockIdx.x / n_ft) * kFtM;
  const double* Db = D + (int64_t)b * nch * 2 * n_fb;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int n_nt = kFN / 16, n_half = (kFtM / 16) * n_nt;  // tiles of one half (Re or Im)
  doublex4 acc[kFtT];
  const double* arow[kFtT];
  bool tok[kFtT];
#pragma unroll
  for (int i = 0; i < kFtT; ++i) {
    acc[i] = doublex4{0.0, 0.0, 0.0, 0.0};
    const int t = wave + 4 * i, im = t / n_half, ml = (t % n_half) / n_nt;
    tok[i] = m0 + ml * 16 < MT;  // MT is a multiple of 16: a 16-row tile lies inside the table or outside it
    arow[i] = Atab + (int64_t)(tok[i] ? im * MT + m0 + ml * 16 + (lane & 15) : 0) * K2;
  }
  for (int k0 = 0; k0 < K2; k0 += kFtK) {
    const int kc = min(kFtK, K2 - k0);  // a multiple of 4, as K2 is
    __syncthreads();                    // the last chunk's readers are done
    for (int e = threadIdx.x; e < kc * kFN; e += 256) {
      const int kk = k0 + e / kFN, n = e % kFN;
      const int q = q0 + n;
      double v = 0.0;
      if (q < n_fb && kk < 2 * nch) {
        const int x = kk < nch ? kk : kk - nch;
        v = Db[(int64_t)x * 2 * n_fb + 2 * q + (kk < nch ? 0 : 1)];
      }
      Bs[(e / kFN) * (kFN + 1) + n] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kFtT; ++i) {
      if (!tok[i]) continue;
      const int nt = (wave + 4 * i) % n_nt;
      for (int kk = 0; kk < kc; kk += 4) {
        const double a = arow[i][k0 + kk + (lane >> 4)];
        const double bb = Bs[(kk + (lane >> 4)) * (kFN + 1) + nt * 16 + (lane & 15)];
        acc[i] = mfma_f64(a, bb, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kFtT; ++i) {
    const int t = wave + 4 * i, im = t / n_half, ml = (t % n_half) / n_nt, nt = t % n_nt;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = im * kFtM + ml * 16 + (lane >> 4) + 4 * r;
      Cs[row * (kFN + 1) + nt * 16 + (lane & 15)] = acc[i][r];  // zeros where the tile lies outside the table
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kFtM * kFN; e += 256) {
    const int ml = e / kFN, n = e % kFN, q = q0 + n, m = m0 + ml;
    if (q >= n_fb || m >= n_kb) continue;
    const double mag = hypot(Cs[ml * (kFN + 1) + n], Cs[(kFtM + ml) * (kFN + 1) + n]);
    if (slot) {
      const int sl = slot[b];
      if (sl >= 0 && sl < n_slot)  // the host rejects such slots; never write outside FK
        atomicAdd(FK + ((int64_t)sl * n_kb + m) * n_fb + q, mag * (double)weight[b]);
    } else {
      FK[((int64_t)b * n_kb + m) * n_fb + q] = mag;
    }
  }
}

// per-row L1 norms -> 1 / ||row||_1 (map_fv norm=True: data / norm(data, ord=1, axis=-1))
__global__ __launch_bounds__(256) void row_l1_kernel(const float* __restrict__ data, int64_t b_stride,
                                                      int64_t ch_stride, int32_t nch, int32_t nt,
                                                      float* __restrict__ inv_l1) {
  const int r = blockIdx.x;
  const int b = r / nch, x = r % nch;
  const float* row = data + (int64_t)b * b_stride + (int64_t)x * ch_stride;
  double s = 0.0;
  for (int t = threadIdx.x; t < nt; t += blockDim.x) s += fabs((double)row[t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) inv_l1[r] = (float)(1.0 / (part[0] + part[1] + part[2] + part[3]));
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_disp_row_l1(const float* data, int64_t b_stride, int64_t ch_stride, int32_t B, int32_t nch,
                            int32_t nt, float* inv_l1, void* stream) {
  if (!data || !inv_l1) return set_error(-2, "null pointer argument");
  if (B * nch <= 0) return 0;
  hipLaunchKernelGGL(row_l1_kernel, dim3(B * nch), dim3(256), 0, (hipStream_t)stream, data, b_stride, ch_stride, nch,
                     nt, inv_l1);
  return last_launch();
}

DVH_API int dvh_disp_tdft(const float* data, int64_t b_stride, int64_t ch_stride, int32_t B, int32_t nch,
                          int32_t nt, const double* wt, int32_t n_fb, const float* row_scale, double* D,
                          void* stream) {
  if (!data || !wt || !D) return set_error(-2, "null pointer argument");
  const int M = B * nch, N = 2 * n_fb;
  if (M <= 0 || N <= 0) return 0;
  if ((reinterpret_cast<uintptr_t>(wt) & 15) == 0) {  // N = 2 n_fb is even: 16-byte twiddle pieces
    const int64_t blocks = (int64_t)((M + kTdRows - 1) / kTdRows) * ((N + kTdNT * 16 - 1) / (kTdNT * 16));
    // fewer blocks than a quarter of the CUs: the K-split form (16 waves per block)
    const bool split = blocks * 4 < cu_count();
    const void* fn = split ? (const void*)tdft_rows_kernel<kTdNTs, kTdGs> : (const void*)tdft_rows_kernel<kTdNT, 1>;
    const int NT = split ? kTdNTs : kTdNT, G = split ? kTdGs : 1;
    const size_t lds = tdft_rows_lds(NT, G);
    if (int rc = set_dynamic_lds(fn, lds)) return rc;
    dim3 grid((M + kTdRows - 1) / kTdRows, (N + NT * 16 - 1) / (NT * 16));
    void* args[] = {(void*)&data, &b_stride, &ch_stride, &nch, (void*)&M, &nt, (void*)&wt, (void*)&N, (void*)&row_scale, &D};
    return hip_status(hipLaunchKernel(fn, grid, dim3(256 * G), args, lds, (hipStream_t)stream));
  }
  if (int rc = hip_status(hipMemsetAsync(D, 0, sizeof(double) * (size_t)M * N, (hipStream_t)stream))) return rc;
  const int tiles = ((M + kGT - 1) / kGT) * ((N + kGT - 1) / kGT);
  // enough K slices for ~1024 waves, at least 64 samples each (more slices measured no faster on
  // 512 gathers: 4 096 / 8 192-wave targets 187 / 188 us vs 167)
  int splits = (1024 + tiles - 1) / tiles;
  int kslice = (nt + splits - 1) / splits;
  kslice = kslice < 64 ? 64 : ((kslice + 3) / 4) * 4;
  splits = (nt + kslice - 1) / kslice;
  dim3 grid((N + kGT - 1) / kGT, (M + kGT - 1) / kGT, splits);
  hipLaunchKernelGGL(tdft_gemm_kernel, grid, dim3(64), 0, (hipStream_t)stream, data, b_stride, ch_stride, nch, M, nt,
                     wt, N, row_scale, kslice, D);
  return last_launch();
}

DVH_API int dvh_disp_fk_as(const double* D, int32_t B, int32_t nch, int32_t n_fb, const double* atab, int32_t MT,
                           int32_t K2, int32_t n_kb, double* FK, const int32_t* slot, const float* weight,
                           int32_t n_slot, int32_t form, void* stream) {
  if (!D || !atab || !FK) return set_error(-2, "null pointer argument");
  if ((slot == nullptr) != (weight == nullptr)) return set_error(-2, "slot and weight go together");
  if (slot && n_slot <= 0) return set_error(-2, "slot accumulation needs n_slot > 0");
  if (MT % 16 || n_kb > MT || K2 < 2 * nch || K2 % 4) return set_error(-2, "invalid contraction table shape");
  if (form < DVH_FK_FORM_AUTO || form > DVH_FK_FORM_TILED) return set_error(-2, "unknown contraction form");
  if (B <= 0 || n_fb <= 0) return 0;
  const size_t lds = sizeof(double) * ((size_t)K2 * (kFN + 1) + (size_t)2 * MT * (kFN + 1));
  if (form == DVH_FK_FORM_ONE_BLOCK && lds > 160 * 1024) return set_error(-4, "contraction table too large for one block");
  // the operand and the result no longer fit one block: tile m, chunk the channels
  if (lds > 160 * 1024 || form == DVH_FK_FORM_TILED) {
    const int64_t n_ft = (n_fb + kFN - 1) / kFN, n_mt = (n_kb + kFtM - 1) / kFtM;
    if (n_ft * n_mt > 0x7fffffff) return set_error(-4, "FK grid too large for one launch");
    hipLaunchKernelGGL(fk_contract_tiled_kernel, dim3((unsigned)(n_ft * n_mt), B), dim3(256), 0, (hipStream_t)stream, D,
                       nch, n_fb, atab, MT, K2, n_kb, (int32_t)n_ft, FK, slot, weight, n_slot);
    return last_launch();
  }
  if (int rc = set_dynamic_lds((const void*)fk_contract_kernel, lds)) return rc;
  dim3 grid((n_fb + kFN - 1) / kFN, B);
  hipLaunchKernelGGL(fk_contract_kernel, grid, dim3(256), lds, (hipStream_t)stream, D, nch, n_fb, atab, MT, K2, n_kb,
                     FK, slot, weight, n_slot);
  return last_launch();
}

DVH_API int dvh_disp_fk(const double* D, int32_t B, int32_t nch, int32_t n_fb, const double* atab, int32_t MT,
                        int32_t K2, int32_t n_kb, double* FK, const int32_t* slot, const float* weight,
                        int32_t n_slot, void* stream) {
  return dvh_disp_fk_as(D, B, nch, n_fb, atab, MT, K2, n_kb, FK, slot, weight, n_slot, DVH_FK_FORM_AUTO, stream);
}

