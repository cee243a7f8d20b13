// Dispersion (f-v) image on MI355X (gfx950), step 3 of the chain described in dvh_disp.hip: the |FK| grid sampled
// bilinearly at (k = f / v, f) (FITPACK degree-1 basis, double) -> float32 -> Savitzky-Golay operator along
// frequency (double).  Five kernels, chosen by shape in fv_pick below and in das_diff_veh_amd/disp.py; the
// arithmetic they share is fv_common.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdlib.h>

#include "dvh_common.h"
#include "dvh.h"
#include "fv_common.h"
#include "mfma_f64.h"

namespace dvh {

// ---------------------------------------------------------------------------------------------
// 3. f-v sampling + Savitzky-Golay.  One block = (gather b, 16 velocity rows), all frequencies.
constexpr int kVC = 4;        // velocities per block: 750 blocks for one set of 3 images of 1000 x 242
constexpr int kVS = kVC + 1;  // LDS row stride: the f-consecutive FIR reads hit distinct banks

__global__ __launch_bounds__(256) void fv_kernel(const double* __restrict__ FK, int32_t n_kb, int32_t n_fb,
                                                  const double* __restrict__ kgrid, double kmin, double kmax,
                                                  const double* __restrict__ kq, int32_t nF, int32_t nV,
                                                  const int32_t* __restrict__ fj, const double* __restrict__ fw,
                                                  const double* __restrict__ sg, int32_t sgl,
                                                  float* __restrict__ fv) {
  extern __shared__ __attribute__((aligned(16))) float raw[];  // [nF][kVS]
  const int b = blockIdx.y, v0 = blockIdx.x * kVC;
  const double* F = FK + (int64_t)b * n_kb * n_fb;
  const double k0 = kgrid[0], inv_dk = 1.0 / (kgrid[1] - kgrid[0]);
  for (int e = threadIdx.x; e < nF * kVC; e += blockDim.x) {
    const int f = e / kVC, iv = e % kVC, v = v0 + iv;
    float val = 0.f;
    if (v < nV) {
      double hx0, hx1;
      const int m = fv_query(kq[(int64_t)f * nV + v], kgrid, n_kb, k0, inv_dk, kmin, kmax, hx0, hx1);
      const int j = fj[f];
      const double hy0 = fw[2 * f], hy1 = fw[2 * f + 1];
      const double z00 = F[m * n_fb + j], z01 = F[m * n_fb + j + 1];
      const double z10 = F[(m + 1) * n_fb + j], z11 = F[(m + 1) * n_fb + j + 1];
      val = fv_bilinear(z00, z01, z10, z11, hx0, hx1, hy0, hy1);
    }
    raw[f * kVS + iv] = val;
  }
  __syncthreads();
  const int half = sgl / 2;
  const double* h = sg;                        // interior taps, h[t] multiplies x[f - half + t]
  const double* el = sg + sgl;                 // [half][sgl] left edge (fit to x[0:sgl])
  const double* er = el + half * sgl;          // [half][sgl] right edge (fit to x[nF-sgl:nF])
  for (int e = threadIdx.x; e < nF * kVC; e += blockDim.x) {
    const int iv = e / nF, f = e % nF, v = v0 + iv;
    if (v >= nV) continue;
    double acc = 0.0;
    if (f < half) {
      for (int t = 0; t < sgl; ++t) acc += el[f * sgl + t] * (double)raw[t * kVS + iv];
    } else if (f >= nF - half) {
      const int r = f - (nF - half);
      for (int t = 0; t < sgl; ++t) acc += er[r * sgl + t] * (double)raw[(nF - sgl + t) * kVS + iv];
    } else {
      for (int t = 0; t < sgl; ++t) acc += h[t] * (double)raw[(f - half + t) * kVS + iv];
    }
    fv[((int64_t)b * nV + v) * nF + f] = (float)acc;
  }
}

// 3b. Batched f-v sampling (many images of one plan): one 1024-thread block = (VC velocities, all
// frequencies) x G consecutive images.  The bilinear weights depend on (f, v) only, so each thread
// computes them ONCE (frequency f = tid % nF, velocities 4 g .. 4 g + 3 of the chunk, g = tid / nF)
// and keeps them in registers across the G images.  Per image: the image's FK grid is staged in LDS
// (n_kb x n_fb doubles), the float32 samples go to an LDS row per velocity padded by kSgPad zeros on
// both sides, and the Savitzky-Golay pass gives every thread 4 consecutive outputs of one velocity
// (28 inputs read as 7 x 16 B, 25 taps each in double, the same tap order as fv_kernel).  Bound:
// float64 FMA issue (25 per output) and the 4 B/output HBM write.
constexpr int kFvPre = 4;  // FK doubles prefetched per thread: grids up to 4 x 1024 bins

__global__ __launch_bounds__(kFvThreads) void fv_batch_kernel(
    const double* __restrict__ FK, int32_t B, int32_t G, int32_t n_kb, int32_t n_fb,
    const double* __restrict__ kgrid, double kmin, double kmax, const double* __restrict__ kq, int32_t nF,
    int32_t nV, int32_t n_grp, const int32_t* __restrict__ fj, const double* __restrict__ fw,
    const double* __restrict__ sg, int32_t sgl, float* __restrict__ fv) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int nfk = n_kb * n_fb;
  const FvLds lds = fv_batch_lds(nfk, sgl, n_grp, nF);
  const int nfk2 = lds.fk;
  double* fks = smem;                                      // 2 x [n_kb][n_fb] (double buffer)
  const int VC = kFvVT * n_grp, S = fv_row_stride(nF);
  double* sgs = smem + lds.taps;                           // Savitzky-Golay taps + edge fits
  float* raw = reinterpret_cast<float*>(smem + lds.rows);  // [VC][S], x[f] at kSgPad + f
  const int v0 = blockIdx.x * VC, tid = threadIdx.x;

  // sampling ownership and weights (fv_kernel's expressions, computed once)
  const int g = tid / nF, f = tid - g * nF;
  const bool own = g < n_grp;
  int base[kFvVT];
  double hx0[kFvVT], hx1[kFvVT], hy0 = 0.0, hy1 = 0.0;
  {
    const double k0 = kgrid[0], inv_dk = 1.0 / (kgrid[1] - kgrid[0]);
    const int j = own ? fj[f] : 0;
    if (own) {
      hy0 = fw[2 * f];
      hy1 = fw[2 * f + 1];
    }
#pragma unroll
    for (int i = 0; i < kFvVT; ++i) {
      const int v = v0 + kFvVT * g + i;
      base[i] = -1;
      hx0[i] = hx1[i] = 0.0;
      if (own && v < nV)
        base[i] = fv_query(kq[(int64_t)f * nV + v], kgrid, n_kb, k0, inv_dk, kmin, kmax, hx0[i], hx1[i]) * n_fb + j;
    }
  }
  // zero pads (never written afterwards)
  for (int e = tid; e < VC * S; e += kFvThreads) {
    const int c = e % S;
    if (c < kSgPad || c >= kSgPad + nF) raw[e] = 0.f;
  }
  const int half = sgl / 2;
  for (int e = tid; e < sgl * sgl; e += kFvThreads) sgs[e] = sg[e];  // sgl + 2 * half * sgl = sgl^2 entries
  const double* h = sgs;
  const double* el = sgs + sgl;
  const double* er = el + half * sgl;
  const int nb4 = (nF + 3) >> 2;
  // FK grids are software-pipelined: image it + 1's grid is loaded into registers (kFvPre per
  // thread) while image it is sampled, and stored to the other LDS buffer before its filter pass
  const int b0 = blockIdx.y * G;
  const int n_img = min(G, B - b0);
  double pre[kFvPre];
#pragma unroll
  for (int k = 0; k < kFvPre; ++k) {
    const int e = tid + k * kFvThreads;
    if (e < nfk) fks[e] = FK[(int64_t)b0 * nfk + e];
  }
  for (int it = 0; it < n_img; ++it) {
    const int b = b0 + it;
    const double* fk_cur = fks + (it & 1) * nfk2;
    lds_barrier();  // fk_cur stored, raw free
    const bool more = it + 1 < n_img;
    if (more) {
#pragma unroll
      for (int k = 0; k < kFvPre; ++k) {
        const int e = min(tid + k * kFvThreads, nfk - 1);  // unconditional load: no register zeroing
        pre[k] = FK[(int64_t)(b + 1) * nfk + e];
      }
    }
    if (own) {
#pragma unroll
      for (int i = 0; i < kFvVT; ++i) {
        if (base[i] < 0) continue;
        const int m = base[i];
        const double z00 = fk_cur[m], z01 = fk_cur[m + 1], z10 = fk_cur[m + n_fb], z11 = fk_cur[m + n_fb + 1];
        raw[(kFvVT * g + i) * S + kSgPad + f] = fv_bilinear(z00, z01, z10, z11, hx0[i], hx1[i], hy0, hy1);
      }
    }
    if (more) {  // next image's grid -> the other LDS buffer (last read in the previous image's sampling)
      double* fk_next = fks + ((it + 1) & 1) * nfk2;
#pragma unroll
      for (int k = 0; k < kFvPre; ++k) {
        const int e = tid + k * kFvThreads;
        if (e < nfk) fk_next[e] = pre[k];
      }
    }
    lds_barrier();
    for (int task = tid; task < VC * nb4; task += kFvThreads) {
      const int r = task / nb4, f0 = (task - r * nb4) * 4, v = v0 + r;
      if (v >= nV) continue;
      const float* row = raw + r * S + kSgPad;  // row[x] = sample at frequency x (zero outside [0, nF))
      double acc[4];
      sg_pass4(row, nF, sgl, f0, nF, (gbl_cdouble)sg, h, el, er, acc);
      fv_store4(fv + ((int64_t)b * nV + v) * nF + f0, nF, f0, nF, acc);
    }
  }
}

// 3c. Frequency-tiled f-v sampling: one 256-thread block = (a tile of TO output frequencies, 4
// velocities) x G images, so that several independent blocks share a CU (the 1 024-thread
// fv_batch_kernel leaves the SIMDs idle at every barrier).  The block samples the tile's
// frequencies plus a kSgPad halo on each side (clamped to the record; the last tile keeps at least
// the 25 samples the right-edge fit reads), so the Savitzky-Golay pass of its outputs is local.
// Only the FK columns the tile's frequencies touch are staged per image.  The halo covers windows up to
// kSgFast = 2 * kSgPad + 1; the host refuses the tiled form for a wider one (fv_tile_geometry).
constexpr int kTileVT = 4;  // velocities per fv_tile block (8: more outputs per barrier pair, more registers)

// kCells: instead of every FK row of the columns the tile touches, the block stages only the cells its
// bilinear stencils read (host tables of DispPlan.cell_tables, per (velocity chunk, tile) ct: the cells'
// FK offsets, column-major, and per (frequency, velocity) the compact indices b0 of (m, j) and b1 of
// (m, j + 1) and the FITPACK interval m) -- a few rows per column instead of all n_kb.
template <int VT, bool kCells>
__global__ __launch_bounds__(kTileThreads) void fv_tile_kernel(
    const double* __restrict__ FK, int32_t B, int32_t G, int32_t n_kb, int32_t n_fb,
    const double* __restrict__ kgrid, double kmin, double kmax, const double* __restrict__ kq, int32_t nF,
    int32_t nV, int32_t TO, const int32_t* __restrict__ fj, const double* __restrict__ fw,
    const double* __restrict__ sg, int32_t sgl, float* __restrict__ fv, const int32_t* __restrict__ cell_off,
    const int32_t* __restrict__ n_cell, int32_t max_cell, const int4* __restrict__ qidx) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int S = kTileRow;
  const int tid = threadIdx.x;
  const int f_lo = blockIdx.x * TO, f_hi = min(nF, f_lo + TO);
  const int half = sgl / 2;
  const int s0 = max(0, f_lo - kSgPad);
  const int s1 = min(nF, max(f_hi + kSgPad, sgl));
  const int v0 = blockIdx.y * VT;
  const int f = s0 + tid;
  const bool own = f < s1;
  const int ct = blockIdx.y * gridDim.x + blockIdx.x;  // (velocity chunk, tile) of the cell tables
  int jlo = 0, ncol = 0, nsub = 0;
  if constexpr (kCells) {
    nsub = n_cell[ct];
  } else {
    __shared__ int jr[2];
    if (tid == 0) {
      jr[0] = 1 << 30;
      jr[1] = -1;
    }
    __syncthreads();
    if (own) {
      atomicMin(&jr[0], fj[f]);
      atomicMax(&jr[1], fj[f]);
    }
    __syncthreads();
    jlo = jr[0];
    ncol = jr[1] + 2 - jr[0];  // columns jlo .. jhi + 1
    nsub = n_kb * ncol;
  }
  const FvLds lds = fv_tile_lds(kCells ? max_cell : n_kb * n_fb, sgl, VT);
  double* fks = smem;                                      // [n_kb][ncol], or the compact cells
  double* sgs = smem + lds.taps;                           // taps + edge fits
  float* raw = reinterpret_cast<float*>(smem + lds.rows);  // [VT][S]
  for (int e = tid; e < sgl * sgl; e += kTileThreads) sgs[e] = sg[e];
  for (int e = tid; e < VT * S; e += kTileThreads) raw[e] = 0.f;
  const double* h = sgs;
  const double* el = sgs + sgl;
  const double* er = el + half * sgl;

  int base[VT], base1[VT];
  double hx0[VT], hx1[VT], hy0 = 0.0, hy1 = 0.0;
  {
    const double k0 = kgrid[0], inv_dk = 1.0 / (kgrid[1] - kgrid[0]);
    const int j = own && !kCells ? fj[f] - jlo : 0;
    if (own) {
      hy0 = fw[2 * f];
      hy1 = fw[2 * f + 1];
    }
#pragma unroll
    for (int i = 0; i < VT; ++i) {
      const int v = v0 + i;
      base[i] = -1;
      hx0[i] = hx1[i] = 0.0;
      if (own && v < nV) {
        const double q = kq[(int64_t)f * nV + v];
        if constexpr (kCells) {  // the interval comes with the table
          const int4 ix = qidx[((int64_t)ct * kTileThreads + tid) * VT + i];
          fv_weights(fv_clamp(q, kmin, kmax), kgrid, ix.z, hx0[i], hx1[i]);
          base[i] = ix.x;
          base1[i] = ix.y;
        } else {
          base[i] = fv_query(q, kgrid, n_kb, k0, inv_dk, kmin, kmax, hx0[i], hx1[i]) * ncol + j;
          base1[i] = base[i] + 1;
        }
      }
    }
  }
  const int nb4 = (f_hi - f_lo + 3) >> 2;
  const int b0 = blockIdx.z * G;
  const int n_img = min(G, B - b0);
  // the sub-grid element -> FK offset map is the same for every image: computed once
  constexpr int kStage = 3;  // elements per thread held as offsets (sub-grids up to 768 bins)
  int goff[kStage];
#pragma unroll
  for (int q = 0; q < kStage; ++q) {
    const int e = tid + q * kTileThreads;
    if constexpr (kCells) {
      goff[q] = e < nsub ? cell_off[(int64_t)ct * max_cell + e] : -1;
    } else {
      const int m = e / ncol;
      goff[q] = e < nsub ? m * n_fb + (e - m * ncol) : -1;
    }
  }
  // filter tasks (velocity row, 4 outputs): tid and, for VT = 8, tid + kTileThreads
  constexpr int kTasks = (VT * 64 + kTileThreads - 1) / kTileThreads;  // task slots per thread (nb4 <= 64)
  // Two barriers per image: the next image's FK sub-grid is staged into fks while this image is
  // filtered (fks is free once every thread has sampled), and its first kStage elements come from
  // registers loaded one image earlier, so the FK fetch latency is not exposed between barriers.
  const int64_t img_stride = (int64_t)n_kb * n_fb;
  double pre[kStage];
  auto stage_img = [&](int it_s) {  // pre (image it_s) -> fks; the rest of the sub-grid from global
    const double* F = FK + (int64_t)(b0 + it_s) * img_stride + jlo;
#pragma unroll
    for (int q = 0; q < kStage; ++q)
      if (goff[q] >= 0) fks[tid + q * kTileThreads] = pre[q];
    for (int e = tid + kStage * kTileThreads; e < nsub; e += kTileThreads) {
      if constexpr (kCells) {
        fks[e] = F[cell_off[(int64_t)ct * max_cell + e]];
      } else {
        const int m = e / ncol, c = e - m * ncol;
        fks[e] = F[m * n_fb + c];
      }
    }
  };
  auto load_pre = [&](int it_l) {
    const double* F = FK + (int64_t)(b0 + it_l) * img_stride + jlo;
#pragma unroll
    for (int q = 0; q < kStage; ++q)
      if (goff[q] >= 0) pre[q] = F[goff[q]];
  };
  if (n_img > 0) {
    load_pre(0);
    stage_img(0);
    if (n_img > 1) load_pre(1);
  }
  for (int it = 0; it < n_img; ++it) {
    const int b = b0 + it;
    lds_barrier();  // fks holds image it; the previous image's filter is done with raw
    if (own) {
#pragma unroll
      for (int i = 0; i < VT; ++i) {
        if (base[i] < 0) continue;
        // (m, j), (m, j + 1), (m + 1, j), (m + 1, j + 1): row-major sub-grid, or compact column-major cells
        const int m = base[i], m1 = base1[i];
        const double z00 = fks[m], z01 = kCells ? fks[m1] : fks[m + 1];
        const double z10 = kCells ? fks[m + 1] : fks[m + ncol], z11 = kCells ? fks[m1 + 1] : fks[m + ncol + 1];
        raw[i * S + kSgPad + tid] = fv_bilinear(z00, z01, z10, z11, hx0[i], hx1[i], hy0, hy1);
      }
    }
    lds_barrier();  // raw holds image it; fks is free
    if (it + 1 < n_img) {
      stage_img(it + 1);
      if (it + 2 < n_img) load_pre(it + 2);
    }
    // VT * nb4 filter tasks over the block's threads (TO + 2 kSgPad <= kTileThreads)
#pragma unroll
    for (int ts = 0; ts < kTasks; ++ts) {
      const int task = tid + ts * kTileThreads;
      const int t_r = task / nb4, t_f0 = f_lo + (task - t_r * nb4) * 4;
      if (!(task < VT * nb4 && v0 + t_r < nV)) continue;
      const int r = t_r, f0 = t_f0, v = v0 + r;
      const float* row = raw + r * S + kSgPad - s0;  // row[x] = sample at frequency x
      double acc[4];
      sg_pass4(row, nF, sgl, f0, f_hi, (gbl_cdouble)sg, h, el, er, acc);
      fv_store4(fv + ((int64_t)b * nV + v) * nF + f0, nF, f0, f_hi, acc);
    }
  }
}

// 3d. f-v sampling with the Savitzky-Golay filter on the matrix pipe.  The filter is a banded Toeplitz
// operator along frequency, so a (16 velocities x 16 frequencies) output tile is one float64 MFMA GEMM
//   out[v][f0 + j] = sum_{k < 40} x[v][f0 - 12 + k] * H[k][j],   H[k][j] = sg[k - j] (0 <= k - j < 25)
// with the samples x as the A operand (A[i = v][k] on lane (v, k & 3)) and the band as B: 10 K-steps of
// v_mfma_f64_16x16x4_f64 per tile (40 / 25 of the filter's FMAs, on the MFMA pipe, beside the VALU that
// samples).  A wave owns 16 velocities of GI images (GI independent accumulation chains) and walks the
// frequency axis tile by tile; tile t + 1 shares 24 of its 40 inputs with tile t, so each lane keeps its
// samples in a register ring per image (step g = frequency 4 g - 12 + (lane >> 4), slot g & 15) and
// samples 4 new ones per tile: their table loads one tile ahead, their arithmetic during the tile before
// the MFMAs that consume them.  The first tile (left polynomial fit rows f < 12) and a last tile at
// f0 = nF - 16 (right fit) take their B operands from the operator in LDS; the regular tiles write rows
// f < nF - 16 only.  The block (4 waves, 64 velocities) stages the GI images' compact FK grids in LDS
// with LDS-DMA (global_load_lds_dword, no VGPRs).
// Sampling per (f, v) is fv_kernel's arithmetic with the image-independent parts from plan tables
// (DispPlan.mfma_tables), loaded once per sample for the GI images: the FITPACK weights hx[f][v] =
// {fx (khi - q), fx (q - klo)} of the clamped query and the cell offset cb[f][v] = m * n_fb + fj[f],
// bit-identical to what the other kernels compute.  (Forming the weights in the kernel from the query and
// LDS tables of the k grid and fw measured slower: 1 207 vs 704 us for one image per wave, the LDS
// bandwidth of the extra reads.)  Two images per wave (GI = 2) measured 673 vs 724 us for one.
constexpr int kMfGI = 2;   // images per wave in lock step
constexpr int kMfWpe = 2;  // waves per SIMD the kernel is register-budgeted for
constexpr int kMfV = 16;      // velocities per wave
constexpr int kMfWaves = 4;   // waves per block

__device__ __forceinline__ double sg_coef(const double* sgs, int nF, int f, int xi) {
  constexpr int L = 2 * kSgPad + 1, half = kSgPad;
  int t;
  const double* c;
  if (f < half) {  // left fit: x[0, L)
    t = xi;
    c = sgs + L + f * L;
  } else if (f >= nF - half) {  // right fit: x[nF - L, nF)
    t = xi - (nF - L);
    c = sgs + L + half * L + (f - (nF - half)) * L;
  } else {
    t = xi - f + half;
    c = sgs;
  }
  return (t >= 0 && t < L) ? c[t] : 0.0;
}

// LDS bytes of fv_mfma_kernel<GI>
__host__ __device__ inline size_t fv_mfma_lds(int GI, int nfk) {
  const int nbuf = (nfk + 31) & ~31;
  constexpr int L = 2 * kSgPad + 1;
  return sizeof(double) * ((size_t)GI * nbuf + (size_t)L * L + 64);
}

template <int GI>
__global__ __launch_bounds__(kMfWaves * 64) __attribute__((amdgpu_waves_per_eu(kMfWpe, kMfWpe))) void fv_mfma_kernel(
    const double* __restrict__ FK, int32_t B, int32_t G, int32_t n_kb, int32_t n_fb, const double2* __restrict__ hx,
    const int32_t* __restrict__ cb, int32_t nF, int32_t nV, const double2* __restrict__ fw, const double* __restrict__ sg,
    float* __restrict__ fv, int32_t n_vb, int32_t xcd_map) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int L = 2 * kSgPad + 1;
  const int nfk = n_kb * n_fb;
  const int nbuf = ((nfk + 31) & ~31);  // doubles of an FK buffer: whole 256-byte LDS-DMA pieces
  double* fks = smem;                   // [GI][nbuf]
  double* sgs = smem + GI * nbuf;       // taps + edge fits (L * L)
  double* bpad = sgs + L * L;           // [64]: taps at 16 .. 40, zeros around (the interior band)
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the lane index formed afresh where it is used (mbcnt of an opaque zero: no value kept live, or spilled,
  // across the image loop)
  auto lane_now = []() {
    unsigned z = 0;
    asm volatile("" : "+v"(z));
    return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
  };
  // block -> (velocity block, image group); XCD-aware when the velocity blocks split evenly over the 8
  // XCDs (blocks are dealt round robin): every block of a velocity block then runs on one XCD and its
  // (f, v) table slice stays in that XCD's L2
  int vb, ig;
  {
    const int L0 = blockIdx.x;
    if (xcd_map) {
      const int per = n_vb >> 3, x = L0 & 7, k = L0 >> 3;
      vb = x + 8 * (k % per);
      ig = k / per;
    } else {
      vb = L0 % n_vb;
      ig = L0 / n_vb;
    }
  }
  const int b0 = ig * G, n_img = min(G, B - b0);
  const int vw = vb * (kMfWaves * kMfV) + wave * kMfV;  // the wave's first velocity (uniform)

  // LDS-DMA of image `img`'s FK grid into buffer `buf` (256-byte pieces dealt over the waves; lanes past
  // the grid re-read its last dword, landing in the buffer's pad)
  const int n_piece = (2 * nfk + 63) >> 6;
  auto stage = [&](int img, int buf) {
    const float* src = reinterpret_cast<const float*>(FK + (int64_t)img * nfk);
    const int lane = lane_now();
    for (int p = wave; p < n_piece; p += kMfWaves) {
      const int e = min(p * 64 + lane, 2 * nfk - 1);
      __builtin_amdgcn_global_load_lds((gbl_void*)(src + e), (lds_void*)(fks + buf * nbuf + p * 32), 4, 0, 0);
    }
  };
  for (int e = tid; e < L * L; e += kMfWaves * 64) sgs[e] = sg[e];
  for (int e = tid; e < 64; e += kMfWaves * 64) bpad[e] = (e >= 16 && e < 16 + L) ? sg[e - 16] : 0.0;
  const int t_reg = (nF - kMfV + kMfV - 1) / kMfV;  // regular tiles: rows [16 t, min(16 t + 16, nF - 16))

  for (int it = 0; it < n_img; it += GI) {
    const int ng = min(GI, n_img - it);  // images of this pass (a lone last image runs as a pair with itself)
    // the previous pass's reads are done (first barrier), the DMA has landed (vmcnt, second barrier)
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GI; ++g) stage(b0 + it + min(g, ng - 1), g);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the lane indices and sizes are laundered per pass: the first and last tiles' samples, band values
    // and store addresses do not depend on the images, and hoisting them out of the image loop would hold
    // ~200 registers; recomputing them is a few VALU per tile
    int li_, kk_, nF_, nV_, va_, vc_, fl_, boff;
    bool vok_;
    auto launder = [&]() {  // also before the last tile: no common subexpression with tile 0 lives across the loop
      const int ln = lane_now();
      li_ = ln & 15;
      kk_ = ln >> 4;
      nF_ = nF;
      nV_ = nV;
      asm volatile("" : "+v"(li_), "+v"(kk_), "+s"(nF_), "+s"(nV_));
      boff = 16 + kk_ - li_;  // interior band B[k][j] of K-step s = bpad[boff + 4 s] = sg[4 s + k - j]
      va_ = vw + li_;
      vok_ = va_ < nV_;
      vc_ = min(va_, nV_ - 1);
      fl_ = nF_ - kMfV;  // the last tile's first row
    };
    launder();
    // one sample of this lane for the GI images, branch-free (indices clamped, values zeroed outside the
    // grid): x[va_][f] rounded to float32 as map_fv's interp2d output.  Two stages for the regular
    // tiles: the table loads (tload) one tile before the weights, corners and arithmetic (tfinish).
    struct Pend {
      double2 w;
      int base, fc;
      bool in;
    };
    auto tload = [&](int f) -> Pend {
      Pend p;
      p.in = vok_ && f >= 0 && f < nF_;
      p.fc = min(max(f, 0), nF_ - 1);
      const int qi = p.fc * nV_ + vc_;
      p.w = hx[qi];
      p.base = cb[qi];
      return p;
    };
    auto tfinish = [&](const Pend& p, double* xo) {
      const double2 y = fw[p.fc];  // per frequency: 16 lanes share it (an LDS copy measured slower: the
                                   // corner reads already load the LDS, 700 vs 673 us)
      // the corner pairs are merged into ds_read2_b64 (8 LDS cycles against 2 + 2 for single reads, but
      // four opaque single reads measured slower: 743-751 vs 731 us)
      const int i00 = p.base, i01 = p.base + 1, i10 = p.base + n_fb, i11 = p.base + n_fb + 1;
#pragma unroll
      for (int g = 0; g < GI; ++g) {
        const double* F = fks + g * nbuf;
        const double z00 = F[i00], z01 = F[i01], z10 = F[i10], z11 = F[i11];
        const double val = (double)fv_bilinear(z00, z01, z10, z11, p.w.x, p.w.y, y.x, y.y);
        xo[g] = p.in ? val : 0.0;
      }
    };
    auto sample = [&](int f, double* xo) { tfinish(tload(f), xo); };
    auto store = [&](const doublex4* acc, int f0, int f_end) {
      const int f = f0 + li_;
      if (f >= f_end) return;
#pragma unroll
      for (int g = 0; g < GI; ++g) {
        if (g >= ng) break;
        float* out_b = fv + (int64_t)(b0 + it + g) * nV_ * nF_;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int v = vw + kk_ + 4 * r;
          if (v < nV_) out_b[(int64_t)v * nF_ + f] = (float)acc[g][r];
        }
      }
    };
    // rings of samples: step g (frequency 4 g - 12 + kk) in slot g & 15; steps 4 t + 10 .. 4 t + 13 (tile
    // t + 1's new ones) are finished during tile t from table loads issued during tile t - 1
    double x[16][GI];
#pragma unroll
    for (int g = 0; g < GI; ++g) x[0][g] = x[1][g] = 0.0;  // frequencies < -4
#pragma unroll
    for (int s = 2; s < 14; ++s) {  // in groups of 4 loads in flight: the next group's addresses wait on
      sample(4 * s - 12 + kk_, x[s]);  // this group's samples (an opaque dependency the compiler keeps)
      if (s % 4 == 1) asm volatile("" : "+v"(kk_) : "v"(x[s - 3][0]), "v"(x[s - 2][0]), "v"(x[s - 1][0]), "v"(x[s][0]));
    }
#pragma unroll
    for (int s = 10; s < 14; ++s)  // every image's tile-1 samples finished here, not deferred past tile 0
#pragma unroll
      for (int g = 0; g < GI; ++g) asm volatile("" : "+v"(x[s][g]));
    Pend pd[4];  // table loads of steps 14 .. 17 (tile 2's new ones), in flight during tiles 0 and 1
#pragma unroll
    for (int i = 0; i < 4; ++i) pd[i] = tload(4 * (14 + i) - 12 + kk_);
    {  // tile 0: left-fit rows, B operands from the fit matrices in LDS
      doublex4 acc[GI];
#pragma unroll
      for (int g = 0; g < GI; ++g) acc[g] = doublex4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 10; ++s) {
        const double bs = sg_coef(sgs, nF_, li_, 4 * s - 12 + kk_);
#pragma unroll
        for (int g = 0; g < GI; ++g) acc[g] = mfma_f64(x[s][g], bs, acc[g]);
      }
      store(acc, 0, min(kMfV, fl_));
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(pd[i].base));  // corner reads not hoisted above tile 0
    // regular tiles t = 1 .. t_reg - 1, four per iteration so that the ring slots are static.  Tile t
    // consumes steps 4 t .. 4 t + 9; during it, steps 4 t + 10 .. 4 t + 13 are finished from pd (loaded
    // during tile t - 1) and steps 4 t + 14 .. 4 t + 17 are loaded into pd.
    for (int t0 = 1; t0 < t_reg; t0 += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u;
        if (t >= t_reg) break;
        Pend nx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) nx[i] = tload(16 * t + 44 + 4 * i + kk_);
        // steps 4 t + 10 + i -> slot (4 (u + 1) + 10 + i) & 15  (t = t0 + u, t0 = 1 mod 4)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          tfinish(pd[i], x[(4 * (u + 1) + 10 + i) & 15]);
        }
        doublex4 acc[GI];
#pragma unroll
        for (int g = 0; g < GI; ++g) acc[g] = doublex4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 10; ++s) {
          const double bs = bpad[boff + 4 * s];
#pragma unroll
          for (int g = 0; g < GI; ++g) {
            acc[g] = mfma_f64(x[(4 * (u + 1) + s) & 15][g], bs, acc[g]);
          }
        }
        store(acc, kMfV * t, fl_);
#pragma unroll
        for (int i = 0; i < 4; ++i) pd[i] = nx[i];
        // one tile per scheduling region, its samples finished in it
        asm volatile("" ::"v"(x[(4 * (u + 1) + 10) & 15][0]), "v"(x[(4 * (u + 1) + 11) & 15][0]),
                     "v"(x[(4 * (u + 1) + 12) & 15][0]), "v"(x[(4 * (u + 1) + 13) & 15][0]));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    launder();
    {  // last tile: rows nF - 16 .. nF - 1 (right fit), fresh samples in two groups of 5
      doublex4 acc[GI];
#pragma unroll
      for (int g = 0; g < GI; ++g) acc[g] = doublex4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 10; ++s) {
        const int xi = fl_ - 12 + 4 * s + kk_;
        double xs[GI];
        sample(xi, xs);
        const double bs = sg_coef(sgs, nF_, fl_ + li_, xi);
#pragma unroll
        for (int g = 0; g < GI; ++g) acc[g] = mfma_f64(xs[g], bs, acc[g]);
        if (s == 4) asm volatile("" : "+v"(kk_) : "v"(xs[0]));
      }
      store(acc, fl_, nF_);
    }
  }
}

}  // namespace dvh

using namespace dvh;

namespace {

// What dvh_disp_fv_as launches for one shape: the kernel, its images per block and its launch figures.
struct FvPick {
  int form;    // DVH_FV_TILED, DVH_FV_BATCHED or DVH_FV_PER_IMAGE
  int G;       // images per block (0: the per-image kernel)
  int TO, nt;  // tiled: outputs per tile, tiles
  int n_grp;   // batched: velocity groups per block
  size_t lds;
};

// The structural conditions of fv_tile_kernel for n_tile tiles of TO outputs (a multiple of 4) that cover the nF
// frequencies: nullptr, or what fails.  A block samples its tile and a kSgPad halo, so the window is at most
// kSgFast; the sampled span fits the block's threads, the outputs its 64 four-output tasks per row; and the last
// of several tiles holds, with its halo, the sgl samples the right-edge fit reads.
const char* fv_tile_geometry(int nF, int sgl, int TO, int n_tile) {
  if (sgl > kSgFast) return "savgol window wider than a tile's halo covers (25)";
  for (int t = 0; t < n_tile; ++t) {
    const int f_lo = t * TO, f_hi = nF < f_lo + TO ? nF : f_lo + TO;
    const int s0 = f_lo - kSgPad > 0 ? f_lo - kSgPad : 0;
    const int e1 = f_hi + kSgPad > sgl ? f_hi + kSgPad : sgl, s1 = nF < e1 ? nF : e1;
    if (s1 - s0 > kTileThreads || (f_hi - f_lo + 3) / 4 > 64) return "tile wider than the block";
  }
  if (n_tile > 1 && nF - (n_tile - 1) * TO < kSgPad + 1) return "last tile too narrow";
  return nullptr;
}

// Images per block of the tiled and the cell-staged launch: ~8 k blocks, at most 64 images each
int fv_tile_images(int64_t tile_chunk_pairs, int B, int images_per_block) {
  if (images_per_block > 0) return images_per_block;
  const int64_t G = (tile_chunk_pairs * B + 8191) / 8192;
  return G < 1 ? 1 : (G > 64 ? 64 : (int)G);
}

// The choice among the three kernels of dvh_disp_fv, host arithmetic only.  `form` DVH_FV_AUTO takes each kernel
// where it pays; a forced form drops the size thresholds (work, B * nvc) but never the structural conditions (LDS,
// tile geometry, the window a tile's halo covers): where those fail the chain goes on, tiled -> batched ->
// per-image.  images_per_block > 0 sets G of the forced kernel (DVH_FV_TILED, DVH_FV_BATCHED).
FvPick fv_pick(int B, int n_kb, int n_fb, int nF, int nV, int sgl, int form, int images_per_block) {
  // a grid of more bins than kFvMaxStage fits no block's LDS: the per-image kernel reads it from global memory
  const bool staged = (int64_t)n_kb * n_fb <= kFvMaxStage;
  const int nfk = staged ? n_kb * n_fb : 0;
  // frequency-tiled kernel: tiles of TO outputs (multiple of 4, ~200)
  if (staged && (form == DVH_FV_AUTO || form == DVH_FV_TILED)) {
    const int nt = (nF + 199) / 200;
    int TO = (nF + nt - 1) / nt;
    TO = (TO + 3) & ~3;
    // large batches of long frequency axes only: on few images (the bench's 3 class stacks of
    // 1 000 x 242) the per-image kernel measured faster (1.100 vs 1.125 ms per bench step), and with
    // tiles under 160 outputs (nF = 242: 2 x 124) half the block idles -- the batched kernel packs
    // 4 velocity groups there (sliding bench 16.2 vs 17.6 ms per step)
    const int64_t work = (int64_t)B * nt * ((nV + kFvVT - 1) / kFvVT);  // in 4-velocity units
    if (((work >= 8192 && TO >= 160) || form == DVH_FV_TILED) && !fv_tile_geometry(nF, sgl, TO, nt)) {
      const size_t lds_t = fv_tile_lds(nfk, sgl, kTileVT).bytes;
      if (lds_t <= 64 * 1024) {
        const int nvc = (nV + kTileVT - 1) / kTileVT;
        const int G = fv_tile_images((int64_t)nt * nvc, B, form == DVH_FV_TILED ? images_per_block : 0);
        return {DVH_FV_TILED, G, TO, nt, 0, lds_t};
      }
    }
  }
  // batched kernel: weights computed once per (f, v) and reused over G images of the block
  int n_grp = nF <= kFvThreads ? kFvThreads / nF : 0;
  n_grp = n_grp > 8 ? 8 : n_grp;
  if (staged && n_grp > 0 && form != DVH_FV_PER_IMAGE) {
    const int VC = kFvVT * n_grp;
    const size_t lds_b = fv_batch_lds(nfk, sgl, n_grp, nF).bytes;
    if (nfk <= kFvPre * kFvThreads && lds_b <= 150 * 1024) {
      const int nvc = (nV + VC - 1) / VC;
      // images per block: 1 024 blocks (4 per CU) amortise the per-block weights best (measured
      // G = 64 > 16 > 4 on 512 images of 512 x 1000); below ~1 024 (v-chunk, image) pairs the
      // per-image kernel's 256-thread blocks fill the chip better
      int G = (int)(((int64_t)B * nvc + 1023) / 1024);
      G = G < 1 ? 1 : (G > 64 ? 64 : G);
      // (a named kernel stays named down the chain: a refused DVH_FV_TILED runs batched at any size)
      if ((int64_t)B * nvc < 1024 && form != DVH_FV_BATCHED && form != DVH_FV_TILED) G = 0;
      if (form == DVH_FV_BATCHED && images_per_block > 0) G = images_per_block;
      if (G > 0) return {DVH_FV_BATCHED, G, 0, 0, n_grp, lds_b};
    }
  }
  return {DVH_FV_PER_IMAGE, 0, 0, 0, 0, sizeof(float) * (size_t)nF * kVS};
}

int fv_check(int32_t n_kb, int32_t n_fb, int32_t nF, int32_t sgl, int32_t form) {
  if (n_kb < 2 || n_fb < 2) return set_error(-2, "FK grid needs at least 2 x 2 bins");
  if (sgl < 1 || sgl % 2 == 0 || sgl > nF)
    return set_error(-4, "savgol window must be odd and <= number of frequencies");
  if (form < DVH_FV_AUTO || form > DVH_FV_TILED) return set_error(-2, "unknown f-v form");
  return 0;
}

}  // namespace

DVH_API int dvh_disp_fv_pick(int32_t B, int32_t n_kb, int32_t n_fb, int32_t nF, int32_t nV, int32_t sgl, int32_t form,
                             int32_t images_per_block, int32_t* form_out, int32_t* G_out) {
  if (!form_out || !G_out) return set_error(-2, "null pointer argument");
  if (int rc = fv_check(n_kb, n_fb, nF, sgl, form)) return rc;
  *form_out = DVH_FV_AUTO;  // no images or no velocities: nothing would run
  *G_out = 0;
  if (B <= 0 || nV <= 0) return 0;
  const FvPick p = fv_pick(B, n_kb, n_fb, nF, nV, sgl, form, images_per_block);
  if (p.form == DVH_FV_PER_IMAGE && p.lds > 160 * 1024) return set_error(-4, "too many frequencies for one block");
  *form_out = p.form;
  *G_out = p.G;
  return 0;
}

DVH_API int dvh_disp_fv_as(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* kgrid, double kmin,
                           double kmax, const double* kq, int32_t nF, int32_t nV, const int32_t* fj, const double* fw,
                           const double* sg, int32_t sgl, float* fv, int32_t form, int32_t images_per_block,
                           void* stream) {
  if (!FK || !kgrid || !kq || !fj || !fw || !sg || !fv) return set_error(-2, "null pointer argument");
  if (int rc = fv_check(n_kb, n_fb, nF, sgl, form)) return rc;
  if (B <= 0 || nV <= 0) return 0;
  const FvPick p = fv_pick(B, n_kb, n_fb, nF, nV, sgl, form, images_per_block);
  const int G = p.G;
  if (p.form == DVH_FV_TILED) {
    constexpr int VT = kTileVT;
    if (int rc = set_dynamic_lds((const void*)fv_tile_kernel<VT, false>, p.lds)) return rc;
    dim3 grid(p.nt, (nV + VT - 1) / VT, (B + G - 1) / G);
    hipLaunchKernelGGL((fv_tile_kernel<VT, false>), grid, dim3(kTileThreads), p.lds, (hipStream_t)stream, FK, B, G,
                       n_kb, n_fb, kgrid, kmin, kmax, kq, nF, nV, p.TO, fj, fw, sg, sgl, fv, nullptr, nullptr, 0,
                       nullptr);
    return last_launch();
  }
  if (p.form == DVH_FV_BATCHED) {
    if (int rc = set_dynamic_lds((const void*)fv_batch_kernel, p.lds)) return rc;
    const int VC = kFvVT * p.n_grp;
    dim3 grid((nV + VC - 1) / VC, (B + G - 1) / G);
    hipLaunchKernelGGL(fv_batch_kernel, grid, dim3(kFvThreads), p.lds, (hipStream_t)stream, FK, B, G, n_kb, n_fb,
                       kgrid, kmin, kmax, kq, nF, nV, p.n_grp, fj, fw, sg, sgl, fv);
    return last_launch();
  }
  if (p.lds > 160 * 1024) return set_error(-4, "too many frequencies for one block");
  if (int rc = set_dynamic_lds((const void*)fv_kernel, p.lds)) return rc;
  dim3 grid((nV + kVC - 1) / kVC, B);
  hipLaunchKernelGGL(fv_kernel, grid, dim3(256), p.lds, (hipStream_t)stream, FK, n_kb, n_fb, kgrid, kmin, kmax, kq, nF,
                     nV, fj, fw, sg, sgl, fv);
  return last_launch();
}

DVH_API int dvh_disp_fv(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* kgrid, double kmin,
                        double kmax, const double* kq, int32_t nF, int32_t nV, const int32_t* fj, const double* fw,
                        const double* sg, int32_t sgl, float* fv, void* stream) {
  return dvh_disp_fv_as(FK, B, n_kb, n_fb, kgrid, kmin, kmax, kq, nF, nV, fj, fw, sg, sgl, fv, DVH_FV_AUTO, 0, stream);
}

DVH_API int dvh_disp_fv_cells_as(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* kgrid,
                                 double kmin, double kmax, const double* kq, int32_t nF, int32_t nV, const double* fw,
                                 const double* sg, int32_t sgl, int32_t TO, int32_t n_tile, int32_t VT,
                                 int32_t max_cell, const int32_t* cell_off, const int32_t* n_cell, const int32_t* qidx,
                                 float* fv, int32_t images_per_block, void* stream) {
  if (!FK || !kgrid || !kq || !fw || !sg || !fv || !cell_off || !n_cell || !qidx)
    return set_error(-2, "null pointer argument");
  if (int rc = fv_check(n_kb, n_fb, nF, sgl, DVH_FV_AUTO)) return rc;
  if (VT != kFvVT) return set_error(-4, "cell tables are built for 4 velocities per block");
  if (TO <= 0 || TO % 4 || n_tile <= 0 || (int64_t)(n_tile - 1) * TO >= nF || (int64_t)n_tile * TO < nF)
    return set_error(-2, "tile width / count do not cover the frequencies");
  if (max_cell <= 0 || max_cell > 8192) return set_error(-4, "cell table wider than 8192 cells");
  if (const char* why = fv_tile_geometry(nF, sgl, TO, n_tile)) return set_error(-4, why);
  if (B <= 0 || nV <= 0) return 0;
  const size_t lds = fv_tile_lds(max_cell, sgl, kFvVT).bytes;
  if (int rc = set_dynamic_lds((const void*)fv_tile_kernel<kFvVT, true>, lds)) return rc;
  const int nvc = (nV + kFvVT - 1) / kFvVT;
  const int G = fv_tile_images((int64_t)n_tile * nvc, B, images_per_block);
  dim3 grid(n_tile, nvc, (B + G - 1) / G);
  hipLaunchKernelGGL((fv_tile_kernel<kFvVT, true>), grid, dim3(kTileThreads), lds, (hipStream_t)stream, FK, B, G, n_kb,
                     n_fb, kgrid, kmin, kmax, kq, nF, nV, TO, (const int32_t*)nullptr, fw, sg, sgl, fv, cell_off, n_cell,
                     max_cell, (const int4*)qidx);
  return last_launch();
}

DVH_API int dvh_disp_fv_cells(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* kgrid, double kmin,
                              double kmax, const double* kq, int32_t nF, int32_t nV, const double* fw, const double* sg,
                              int32_t sgl, int32_t TO, int32_t n_tile, int32_t VT, int32_t max_cell,
                              const int32_t* cell_off, const int32_t* n_cell, const int32_t* qidx, float* fv,
                              void* stream) {
  return dvh_disp_fv_cells_as(FK, B, n_kb, n_fb, kgrid, kmin, kmax, kq, nF, nV, fw, sg, sgl, TO, n_tile, VT, max_cell,
                              cell_off, n_cell, qidx, fv, 0, stream);
}

DVH_API int dvh_disp_fv_mfma(const double* FK, int32_t B, int32_t n_kb, int32_t n_fb, const double* hx,
                             const int32_t* cb, int32_t nF, int32_t nV, const double* fw, const double* sg, int32_t sgl,
                             int32_t G, float* fv, void* stream) {
  if (!FK || !hx || !cb || !fw || !sg || !fv) return set_error(-2, "null pointer argument");
  if (n_kb < 2 || n_fb < 2) return set_error(-2, "FK grid needs at least 2 x 2 bins");
  if (sgl != 2 * kSgPad + 1) return set_error(-4, "the MFMA f-v kernel is built for savgol window 25");
  if (nF < 2 * kMfV) return set_error(-4, "the MFMA f-v kernel needs at least 32 frequencies");
  if ((int64_t)n_kb * n_fb > 8192) return set_error(-4, "FK grid larger than 8192 bins");
  if ((int64_t)nF * nV > 0x7fffffff) return set_error(-4, "f-v grid larger than 2^31 points");
  if (B <= 0 || nV <= 0) return 0;
  constexpr int GI = kMfGI;
  const size_t lds = fv_mfma_lds(GI, n_kb * n_fb);
  if (int rc = set_dynamic_lds((const void*)fv_mfma_kernel<GI>, lds)) return rc;
  const int n_vb = (nV + kMfWaves * kMfV - 1) / (kMfWaves * kMfV);
  if (G <= 0) {  // ~2 k blocks, at most 16 images each, a multiple of GI
    G = (int)(((int64_t)n_vb * B) / 2048);
    G = G < GI ? GI : (G > 16 ? 16 : G);
  }
  G = (G + GI - 1) / GI * GI;
  const int n_ig = (B + G - 1) / G;
  const int xcd_map = (n_vb % 8 == 0) ? 1 : 0;
  const int64_t n_blk = (int64_t)n_vb * n_ig;
  if (n_blk > 0x7fffffff) return set_error(-4, "grid too large");
  hipLaunchKernelGGL(fv_mfma_kernel<GI>, dim3((unsigned)n_blk), dim3(kMfWaves * 64), lds, (hipStream_t)stream, FK, B, G,
                     n_kb, n_fb, (const double2*)hx, cb, nF, nV, (const double2*)fw, sg, fv, n_vb, xcd_map);
  return last_launch();
}
