// What the f-v sampling kernels of dvh_fv.hip share: the FITPACK query step, the bilinear sample, the
// Savitzky-Golay pass over four consecutive outputs, the output store, and the LDS layouts of the batched and the
// frequency-tiled kernel as the host and the kernels both compute them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dvh {

constexpr int kFvThreads = 1024;
constexpr int kFvVT = 4;          // velocities per thread in the batched kernel's sampling phase
constexpr int kTileThreads = 256;
constexpr int kSgPad = 12;        // zero pad per side of an LDS row, and the halo of a frequency tile
constexpr int kSgFast = 2 * kSgPad + 1;  // the window of the unrolled filter paths; the widest a tile's halo covers

// Workgroup barrier for LDS hand-offs only.  __syncthreads() also orders global memory (a
// workgroup-scope release: s_waitcnt vmcnt(0)), which would stall every image on the previous
// image's f-v stores; the fv stores are never read back by the block.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------------------------
// The query step of FITPACK's fpbisp on the k axis, degree 1.
__device__ __forceinline__ double fv_clamp(double q, double kmin, double kmax) {
  return q < kmin ? kmin : (q > kmax ? kmax : q);  // fpbisp clamps to [t_b, t_e]
}

// fpbspl, degree 1: the weights of the clamped query q on its interval [kgrid[m], kgrid[m + 1])
__device__ __forceinline__ void fv_weights(double q, const double* kgrid, int m, double& hx0, double& hx1) {
  const double klo = kgrid[m], khi = kgrid[m + 1];
  const double fx = 1.0 / (khi - klo);
  hx0 = fx * (khi - q);
  hx1 = fx * (q - klo);
}

// Clamp, find the interval m (a guess from the uniform spacing inv_dk = 1 / (kgrid[1] - kgrid[0]), k0 = kgrid[0],
// walked to kgrid[m] <= q < kgrid[m + 1], m <= n_kb - 2), and form the weights.  Returns m.
__device__ __forceinline__ int fv_query(double q, const double* kgrid, int n_kb, double k0, double inv_dk,
                                        double kmin, double kmax, double& hx0, double& hx1) {
  q = fv_clamp(q, kmin, kmax);
  int m = (int)floor((q - k0) * inv_dk);
  m = m < 0 ? 0 : (m > n_kb - 2 ? n_kb - 2 : m);
  while (m < n_kb - 2 && q >= kgrid[m + 1]) ++m;
  while (m > 0 && q < kgrid[m]) --m;
  fv_weights(q, kgrid, m, hx0, hx1);
  return m;
}

// The bilinear sample, rounded to float32 as map_fv's interp2d output.  Every kernel samples through this one
// expression: their results are bit-identical.
__device__ __forceinline__ float fv_bilinear(double z00, double z01, double z10, double z11, double hx0, double hx1,
                                             double hy0, double hy1) {
  return (float)(z00 * hx0 * hy0 + z01 * hx0 * hy1 + z10 * hx1 * hy0 + z11 * hx1 * hy1);
}

// ---------------------------------------------------------------------------------------------
// Savitzky-Golay outputs f0 .. f0 + 3 (those below f_end) of one sample row: row[x] is the float32 sample at
// frequency x, readable (zero, or a neighbour's sample) kSgPad places to either side of what the outputs use.
// sg is the operator in global memory (uniform loads of the interior taps), h / el / er its LDS copy: interior
// taps, h[t] multiplies x[f - half + t]; [half][sgl] left-edge fit to x[0, sgl); [half][sgl] right-edge fit to
// x[nF - sgl, nF).  Outputs at or past f_end stay 0.
// sg carries its address space: the optimiser simplifies this function before it is inlined, and with a plain
// pointer it merges the edge block's loads from sg and from the LDS fits into flat loads (2 registers more in
// fv_tile_kernel, 3 waves per SIMD instead of 4).
typedef const __attribute__((address_space(1))) double* gbl_cdouble;

__device__ __forceinline__ void sg_pass4(const float* row, int nF, int sgl, int f0, int f_end, gbl_cdouble sg,
                                         const double* h, const double* el, const double* er, double (&acc)[4]) {
  const int half = sgl / 2;
  const bool fast_taps = (sgl == kSgFast);
#pragma unroll
  for (int o = 0; o < 4; ++o) acc[o] = 0.0;
  if (fast_taps && f0 >= half && f0 + 3 < nF - half && f0 + 3 < f_end) {
    // 28 inputs read as 7 x 16 B, 25 taps each in double, the tap order of fv_kernel
    float x[28];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const float4 t4 = *reinterpret_cast<const float4*>(row + f0 - kSgPad + 4 * q);
      x[4 * q] = t4.x; x[4 * q + 1] = t4.y; x[4 * q + 2] = t4.z; x[4 * q + 3] = t4.w;
    }
#pragma unroll
    for (int t = 0; t < kSgFast; ++t) {
      const double ht = sg[t];  // uniform: scalar loads, SGPR operands
#pragma unroll
      for (int o = 0; o < 4; ++o) acc[o] += ht * (double)x[o + t];
    }
  } else if (fast_taps) {
    // edge (or partial) block: the edge fits read x[0, 25) or x[nF - 25, nF) -- loaded once, all loops
    // unrolled so the LDS reads are batched (a rolled loop here stalls the whole block at the
    // next barrier: one dependent LDS round trip per tap)
    constexpr int L = kSgFast;
    const float* src = f0 < half ? row : row + nF - L;
    float y[L];
#pragma unroll
    for (int t = 0; t < L; ++t) y[t] = src[t];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int ff = f0 + o;
      if (ff >= f_end) break;
      double a = 0.0;
      if (ff < half || ff >= nF - half) {
        const double* c = ff < half ? el + ff * L : er + (ff - (nF - half)) * L;
#pragma unroll
        for (int t = 0; t < L; ++t) a += c[t] * (double)y[t];
      } else {
#pragma unroll
        for (int t = 0; t < L; ++t) a += sg[t] * (double)row[ff - half + t];
      }
      acc[o] = a;
    }
  } else {  // any other window: reads half <= kSgPad places around the outputs
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int ff = f0 + o;
      if (ff >= f_end) break;
      double a = 0.0;
      if (ff < half) {
        for (int t = 0; t < sgl; ++t) a += el[ff * sgl + t] * (double)row[t];
      } else if (ff >= nF - half) {
        const int rr = ff - (nF - half);
        for (int t = 0; t < sgl; ++t) a += er[rr * sgl + t] * (double)row[nF - sgl + t];
      } else {
        for (int t = 0; t < sgl; ++t) a += h[t] * (double)row[ff - half + t];
      }
      acc[o] = a;
    }
  }
}

// The four outputs to out = &fv[..][f0] (f0 a multiple of 4): one 16-byte store where the rows are 16-byte
// aligned and all four lie below f_end, else those below f_end one by one.
__device__ __forceinline__ void fv_store4(float* out, int nF, int f0, int f_end, const double (&acc)[4]) {
  if ((nF & 3) == 0 && f0 + 3 < f_end) {
    *reinterpret_cast<float4*>(out) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (f0 + o < f_end) out[o] = (float)acc[o];
  }
}

// ---------------------------------------------------------------------------------------------
// Dynamic LDS of a kernel: the FK buffer(s) at 0, then the Savitzky-Golay operator (sgl * sgl doubles: taps and
// the two edge fits), then the float32 sample rows.  fk, taps and rows count doubles.  The grids are those a block
// can stage (the host asks for at most kFvMaxStage bins), so int arithmetic holds.
struct FvLds {
  int fk;          // one FK buffer (even)
  int taps, rows;  // offsets of the operator and of the sample rows
  size_t bytes;
};
constexpr int kFvMaxStage = 8192;

// fv_batch_kernel: two FK buffers of nfk = n_kb * n_fb bins, rows [kFvVT * n_grp][fv_row_stride(nF)]
__host__ __device__ inline int fv_row_stride(int nF) { return ((nF + 3) & ~3) + 2 * kSgPad; }

__host__ __device__ inline FvLds fv_batch_lds(int nfk, int sgl, int n_grp, int nF) {
  FvLds l;
  l.fk = (nfk + 1) & ~1;
  l.taps = 2 * l.fk;
  l.rows = l.taps + ((sgl * sgl + 1) & ~1);
  l.bytes = sizeof(double) * (size_t)l.rows + sizeof(float) * (size_t)kFvVT * n_grp * fv_row_stride(nF);
  return l;
}

// fv_tile_kernel<VT, kCells>: one FK buffer of n_stage doubles (kCells: the widest block's cells, max_cell;
// else the whole grid, n_kb * n_fb), rows [VT][kTileRow]
constexpr int kTileRow = 2 * kSgPad + kTileThreads + 4;  // row stride (floats), multiple of 4

__host__ __device__ inline FvLds fv_tile_lds(int n_stage, int sgl, int VT) {
  FvLds l;
  l.fk = (n_stage + 1) & ~1;
  l.taps = l.fk;
  l.rows = l.taps + ((sgl * sgl + 1) & ~1);
  l.bytes = sizeof(double) * (size_t)l.rows + sizeof(float) * (size_t)VT * kTileRow;
  return l;
}

}  // namespace dvh
