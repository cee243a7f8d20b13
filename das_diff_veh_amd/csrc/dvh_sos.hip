// The bandpass on MI355X (gfx950): the block-recursion form of sosfiltfilt, the choice between it and the matrix-pipe
// form (dvh_sosm.hip, reached through sos_common.h), and the sosfiltfilt entry points.
//
//   dvh_sosfiltfilt  bandpass_data (modules/utils.py:179-189): scipy.signal.sosfiltfilt(sos, x, axis=1)
//                    = odd extension by padlen, sosfilt with zi * x_ext[0], reverse, sosfilt with
//                    zi * y[-1], reverse, trim.  Float64 recursion, time-parallel over blocks of each
//                    trace (zero-state block filters + a state scan + re-filter, below).
// Data may be float32 (dtype 0) or float64 (dtype 1), modified in place.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "dvh_common.h"
#include "sos_common.h"
#include "dvh.h"

namespace dvh {

// ---------------------------------------------------------------------------------------------
// sosfiltfilt, time-parallel.  The cascade of n_sec transposed-direct-form-II sections (scipy's sosfilt:
// o = b0 v + z0; z0 = b1 v - a1 o + z1; z1 = b2 v - a2 o) is linear in its 2 n_sec states, so a sequence
// u[0, n_ext) cut into blocks of L samples is filtered block-parallel in three phases:
//   A  every block except the last is filtered from ZERO state (block 0 from the true initial state
//      zi * u[0]), keeping only its end state e_k;
//   B  per row, the true end states follow by a scan over the blocks, s_k = e_k + M s_{k-1} with
//      M = A^L the zero-input state transition of L samples (sos_transition_kernel forms it on the
//      device with the filter's own arithmetic);
//   C  every block is filtered again from its true start state s_{k-1} and writes its outputs.
// sosfiltfilt = the forward pass over the odd extension ext(x) (zi * ext[0]), then the backward pass over
// the reversed forward output y (zi * y[-1]), trimmed by padlen.  One lane per (row, block): n_rows x n_ext
// / L lanes instead of n_rows (a 1 024-trace record filled 16 of the chip's 1 024 SIMDs with one lane per
// trace).  The poles of the order-10 band (1.2 Hz at fs = 250 Hz) sit about 1e-2 inside the unit circle,
// so M is a contraction and the scan is well conditioned.

// M[j][m] (row-major, 2 NS states ordered z0[0], z1[0], z0[1], ...): the state after L zero-input samples
// from the unit state e_m.  One wave, lane m < 2 NS.
template <int NS>
__global__ __launch_bounds__(64) void sos_transition_kernel(const double* __restrict__ sos, int32_t L,
                                                             double* __restrict__ M) {
  constexpr int NST = 2 * NS;
  const int m = threadIdx.x;
  if (m >= NST) return;
  SosCoef<NS> c;
  c.load(sos);
  double z0[NS], z1[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    z0[s] = (2 * s == m) ? 1.0 : 0.0;
    z1[s] = (2 * s + 1 == m) ? 1.0 : 0.0;
  }
  for (int i = 0; i < L; ++i) c.step(z0, z1, 0.0);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    M[(2 * s) * NST + m] = z0[s];
    M[(2 * s + 1) * NST + m] = z1[s];
  }
}

// Phases A (OUT = false: end states of blocks k < nb - 1 into S) and C (OUT = true: filter from the true start
// state S[k - 1] and write the outputs: y[i] forward, the trimmed row backward).  One wave per 64 consecutive
// lanes g = r * nb + k.  A lane's block is a run of L samples at its own address, so direct per-lane loads
// would touch 64 cache lines per instruction; instead the wave moves its 64 runs in chunks of kSosCh samples
// through an LDS tile: cooperative loads (16 lanes per run: each instruction reads 4 contiguous runs of 16
// samples), the recursion on the lane's own tile row, and (phase C) the outputs written back into the same
// tile slots and stored cooperatively, again 16 contiguous samples per 16 lanes.
constexpr int kSosCh = 16;           // samples per chunk (L is a multiple of 32)
constexpr int kSosLd = kSosCh + 1;   // tile row stride in doubles: conflict-free own-row reads
template <typename T, int NS, bool BWD, bool OUT>
__global__ __launch_bounds__(64) void sos_block_kernel(T* __restrict__ x, double* __restrict__ y, SosGeom G,
                                                        const double* __restrict__ sos, const double* __restrict__ zi,
                                                        double* __restrict__ S) {
  constexpr int NST = 2 * NS;
  __shared__ double tile[64 * kSosLd];
  const int lane = threadIdx.x;
  const int64_t n_lanes = G.n_rows * G.nb;
  const int64_t g0 = (int64_t)blockIdx.x * 64;
  const int64_t g = g0 + lane;
  const bool act = g < n_lanes && (OUT || (g % G.nb) != G.nb - 1);  // phase A: no end state of the last block
  const int64_t r = act ? g / G.nb : 0;
  const int k = act ? (int)(g - r * G.nb) : 0;
  const int64_t i0 = (int64_t)k * G.L, i1 = act ? min(i0 + G.L, G.n_ext) : i0;
  // this lane's part of the cooperative moves: runs s = 4 m + (lane >> 4), samples e = lane & 15 of a chunk
  const int e = lane & 15;
  SosCoef<NS> c;
  c.load(sos);
  double z0[NS], z1[NS];
  double* Sr = S + g * NST;  // S[r][k]
  if (act && k == 0) {
    const SosInput<T, BWD> u = sos_input<T, BWD>(x, y, G, r);
    const double u0 = u(0);
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      z0[q] = zi[2 * q] * u0;
      z1[q] = zi[2 * q + 1] * u0;
    }
  } else if (act && OUT) {
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      z0[q] = Sr[-NST + 2 * q];
      z1[q] = Sr[-NST + 2 * q + 1];
    }
  } else {
#pragma unroll
    for (int q = 0; q < NS; ++q) z0[q] = z1[q] = 0.0;
  }
  // the longest run of the wave (every block but a row's last has L samples)
  int64_t n_chunks = 0;
  {
    const int64_t len = i1 - i0;
    int64_t mx = len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (int64_t)__shfl_xor((long long)mx, o));
    n_chunks = (mx + kSosCh - 1) / kSosCh;
  }
  // run s = 4 m + (lane >> 4) of the wave is lane g0 + s: its (row, block) by stepping 4 lanes per m
  const int l4 = lane >> 4;
  const int64_t gl = g0 + l4;
  const int64_t r_l = gl / G.nb;
  const int k_l = (int)(gl - r_l * G.nb);
  // sample i of run (rs, ks): the sequence the pass filters (forward: the odd extension of x; backward: the
  // forward output reversed)
  auto in_at = [&](int64_t rs, int64_t i) -> double {
    if (BWD) return y[rs * G.n_ext + (G.n_ext - 1 - i)];
    const T* row = x + rs * G.row_stride;
    const int64_t j = i - G.padlen;
    if (j >= 0 && j < G.n_t) return (double)row[j];
    if (j < 0) return 2.0 * (double)row[0] - (double)row[-j];                    // i < padlen
    return 2.0 * (double)row[G.n_t - 1] - (double)row[2 * (G.n_t - 1) - j];     // past the end
  };
  // cooperative load of chunk ch into registers (this lane's 16 values: runs 4 m + l4, sample e)
  double pv[16];
  auto coop_load = [&](int64_t cbase) {
    int64_t rs = r_l;
    int ks = k_l;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      double v = 0.0;
      if (g0 + 4 * m + l4 < n_lanes) {
        const int64_t i = (int64_t)ks * G.L + cbase + e;
        if (i < min((int64_t)(ks + 1) * G.L, G.n_ext)) v = in_at(rs, i);
      }
      pv[m] = v;
      ks += 4;
      while (ks >= G.nb) {
        ks -= G.nb;
        ++rs;
      }
    }
  };
  if (n_chunks > 0) coop_load(0);
  for (int64_t ch = 0; ch < n_chunks; ++ch) {
    const int64_t cbase = ch * kSosCh;
#pragma unroll
    for (int m = 0; m < 16; ++m) tile[(4 * m + l4) * kSosLd + e] = pv[m];
    __syncthreads();
    if (ch + 1 < n_chunks) coop_load(cbase + kSosCh);  // the next chunk's loads in flight under this one's recursion
    const int64_t nn = min((int64_t)kSosCh, i1 - i0 - cbase);
    if (OUT) {
      for (int t = 0; t < nn; ++t) tile[lane * kSosLd + t] = c.step(z0, z1, tile[lane * kSosLd + t]);
    } else {
      for (int t = 0; t < nn; ++t) c.step(z0, z1, tile[lane * kSosLd + t]);
    }
    __syncthreads();
    if (OUT) {  // cooperative store of the outputs
      int64_t rs = r_l;
      int ks = k_l;
#pragma unroll 4
      for (int m = 0; m < 16; ++m) {
        const int sidx = 4 * m + l4;
        if (g0 + sidx < n_lanes) {
          const int64_t i = (int64_t)ks * G.L + cbase + e;
          if (i < min((int64_t)(ks + 1) * G.L, G.n_ext)) {
            const double v = tile[sidx * kSosLd + e];
            if (!BWD) {
              y[rs * G.n_ext + i] = v;
            } else {
              // reversed index i is sample n_ext - 1 - i of the extension; the row keeps [padlen, padlen + n_t)
              const int64_t j = G.n_ext - 1 - i - G.padlen;
              if (j >= 0 && j < G.n_t) x[rs * G.row_stride + j] = (T)v;
            }
          }
        }
        ks += 4;
        while (ks >= G.nb) {
          ks -= G.nb;
          ++rs;
        }
      }
      __syncthreads();
    }
  }
  if (!OUT && act) {
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      Sr[2 * q] = z0[q];
      Sr[2 * q + 1] = z1[q];
    }
  }
}

// Phase B: s_k = e_k + M s_{k-1} for k = 1 .. nb - 2 (s_0 = e_0 is already the true state).  Two rows per
// wave (lanes 0-31 / 32-63), lane j = state component j.  Each step's state goes through LDS: one 8-byte store
// per lane, then every lane reads the half's whole state with broadcast 16-byte reads (no per-element
// cross-lane shuffles on the step's critical path).
template <int NS>
__global__ __launch_bounds__(64) void sos_scan_kernel(SosGeom G, const double* __restrict__ M, double* __restrict__ S) {
  constexpr int NST = 2 * NS;
  __shared__ __attribute__((aligned(16))) double sv[2][32];
  const int half = threadIdx.x >> 5, j = threadIdx.x & 31;
  const int64_t r = 2 * (int64_t)blockIdx.x + half;
  const bool act = r < G.n_rows && j < NST;
  double m[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) m[i] = act ? M[j * NST + i] : 0.0;
  double* Sr = S + (act ? r : 0) * (int64_t)G.nb * NST;
  sv[half][j] = act ? Sr[j] : 0.0;
  // the zero-state end states e_k come from memory 8 steps at a time, the next 8 loaded under this group's
  // arithmetic (a load per step would put one memory latency on the critical path of every step)
  constexpr int PF = 8;
  const int kend = G.nb - 1;  // steps k = 1 .. nb - 2
  double cur[PF], nxt[PF];
#pragma unroll
  for (int t = 0; t < PF; ++t) cur[t] = (act && 1 + t < kend) ? Sr[(int64_t)(1 + t) * NST + j] : 0.0;
  for (int kb = 1; kb < kend; kb += PF) {
#pragma unroll
    for (int t = 0; t < PF; ++t) {
      const int k = kb + PF + t;
      nxt[t] = (act && k < kend) ? Sr[(int64_t)k * NST + j] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < PF; ++t) {
      const int k = kb + t;
      if (k < kend) {
        wave_barrier_lds();
        const double2* v2 = reinterpret_cast<const double2*>(sv[half]);
        double x[NST];
#pragma unroll
        for (int i = 0; i < NST / 2; ++i) {
          const double2 u = v2[i];
          x[2 * i] = u.x;
          x[2 * i + 1] = u.y;
        }
        // M s in four partial sums (a 5-deep instead of a 20-deep chain of dependent FMAs per step)
        double pa[4] = {cur[t], 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < NST; ++i) pa[i & 3] += m[i] * x[i];
        const double acc = (pa[0] + pa[1]) + (pa[2] + pa[3]);
        if (act) Sr[(int64_t)k * NST + j] = acc;
        wave_barrier_lds();
        sv[half][j] = acc;
      }
    }
#pragma unroll
    for (int t = 0; t < PF; ++t) cur[t] = nxt[t];
  }
}

// block length: enough (row, block) lanes for ~4 waves per SIMD, blocks of 32 .. 4096 samples
static int sos_block_len(int64_t n_rows, int64_t n_ext) {
  const int64_t target = 256LL * 4 * 4 * 64;
  int64_t L = (n_rows * n_ext + target - 1) / target;
  L = (L + 31) / 32 * 32;
  return (int)std::min<int64_t>(std::max<int64_t>(L, 32), 4096);
}

static SosGeom sos_geom(int64_t n_rows, int64_t row_stride, int32_t n_t, int32_t padlen) {
  return sos_geom_of(n_rows, row_stride, n_t, padlen, sos_block_len(n_rows, (int64_t)n_t + 2 * padlen));
}

// workspace: y [n_rows][n_ext] + S [n_rows][nb][2 n_sec] + M [2 n_sec]^2, doubles
static int64_t sos_workspace_doubles(const SosGeom& G, int n_sec) {
  const int64_t nst = 2 * n_sec;
  return G.n_rows * G.n_ext + G.n_rows * G.nb * nst + nst * nst;
}

template <typename T, int NS>
static int sosfiltfilt_blocks(T* x, const SosGeom& G, const double* sos, const double* zi, double* work,
                              hipStream_t st) {
  constexpr int NST = 2 * NS;
  double* y = work;
  double* S = y + G.n_rows * G.n_ext;
  double* M = S + G.n_rows * G.nb * NST;
  const int64_t lanes = G.n_rows * G.nb;
  const dim3 grid((unsigned)((lanes + 63) / 64)), scan_grid((unsigned)((G.n_rows + 1) / 2));
  hipLaunchKernelGGL(sos_transition_kernel<NS>, dim3(1), dim3(64), 0, st, sos, G.L, M);
  // forward pass over the odd extension -> y
  hipLaunchKernelGGL((sos_block_kernel<T, NS, false, false>), grid, dim3(64), 0, st, x, y, G, sos, zi, S);
  if (G.nb > 2) hipLaunchKernelGGL(sos_scan_kernel<NS>, scan_grid, dim3(64), 0, st, G, (const double*)M, S);
  hipLaunchKernelGGL((sos_block_kernel<T, NS, false, true>), grid, dim3(64), 0, st, x, y, G, sos, zi, S);
  // backward pass over reversed y -> the trimmed row
  hipLaunchKernelGGL((sos_block_kernel<T, NS, true, false>), grid, dim3(64), 0, st, x, y, G, sos, zi, S);
  if (G.nb > 2) hipLaunchKernelGGL(sos_scan_kernel<NS>, scan_grid, dim3(64), 0, st, G, (const double*)M, S);
  hipLaunchKernelGGL((sos_block_kernel<T, NS, true, true>), grid, dim3(64), 0, st, x, y, G, sos, zi, S);
  return last_launch();
}

}  // namespace dvh

using namespace dvh;

DVH_API int64_t dvh_sosfiltfilt_workspace(int64_t n_rows, int32_t n_t, int32_t n_sec, int32_t padlen) {
  if (n_rows <= 0 || n_t <= 0 || n_sec <= 0 || n_sec > kMaxSec || padlen < 0) return 0;
  return 8 * std::max(sosm_workspace_doubles(sosm_geom(n_rows, n_t, n_t, padlen), n_sec),
                      sos_workspace_doubles(sos_geom(n_rows, n_t, n_t, padlen), n_sec));
}

DVH_API double dvh_sos_pole_radius(const double* sos, int32_t n_sec) {
  if (!sos || n_sec <= 0) return -1.0;
  double r = 0.0;
  for (int s = 0; s < n_sec; ++s) {
    const double a0 = sos[6 * s + 3], a1 = sos[6 * s + 4] / a0, a2 = sos[6 * s + 5] / a0;
    const double disc = a1 * a1 - 4.0 * a2;
    if (disc < 0.0) {
      r = std::max(r, std::sqrt(a2));
    } else {
      const double q = std::sqrt(disc);
      r = std::max(r, std::max(std::fabs(0.5 * (-a1 + q)), std::fabs(0.5 * (-a1 - q))));
    }
  }
  return r;
}

DVH_API int64_t dvh_sosfiltfilt_plan_bytes(int32_t n_sec) {
  if (n_sec <= 0 || n_sec > kMaxSec) return 0;
  return 8 * sosm_plan_doubles(n_sec);
}

DVH_API int dvh_sosfiltfilt_plan(const double* sos, int32_t n_sec, const double* zi, int32_t n_t, int32_t padlen,
                                 double* plan, void* stream) {
  if (!sos || !zi || !plan) return set_error(-2, "null pointer argument");
  if (n_sec <= 0 || n_sec > kMaxSec) return set_error(-4, "unsupported number of second-order sections");
  if (padlen < 0 || n_t < 2) return set_error(-2, "invalid padlen / length");
  const SosGeom G = sosm_geom(1, n_t, n_t, padlen);
  if (int rc = sosm_make_plan(sos, n_sec, zi, G, plan, (hipStream_t)stream)) return rc;
  return last_launch();
}

DVH_API int dvh_sosfiltfilt_planned(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t,
                                    const double* sos, int32_t n_sec, int32_t padlen, const double* zi, const double* plan,
                                    double* work, void* stream) {
  if (!x || !sos || !zi || !work) return set_error(-2, "null pointer argument");  // plan NULL: the recursion
  if (reinterpret_cast<uintptr_t>(work) % 16) return set_error(-2, "work must be 16-byte aligned");
  if (n_sec <= 0 || n_sec > kMaxSec) return set_error(-4, "unsupported number of second-order sections");
  if (n_t <= padlen) return set_error(-4, "The length of the input vector x must be greater than padlen");
  if (padlen < 0 || n_t < 2) return set_error(-2, "invalid padlen / length");
  if (n_rows <= 0) return 0;
  // MFMA path (a plan given and the 32-bit column indices fit) or the VALU block recursion.  The block GEMMs add the
  // contributions of states that grow like 1 / (1 - r) for the filter's largest pole radius r, so their rounding grows
  // with it: relative error 1e-13 at r = 0.9956 (1.2-30 Hz at 250 Hz), 5e-10 at r = 0.99973 (0.08-1 Hz); callers
  // plan the matrix form only for r <= DVH_SOS_MFMA_MAX_POLE (dvh_sos_pole_radius) and take the recursion otherwise.
  const hipStream_t st = (hipStream_t)stream;
  const SosGeom Gm = sosm_geom(n_rows, row_stride, n_t, padlen);
  if (plan && sosm_fits(Gm)) return sosm_filtfilt(x, dtype, Gm, sos, n_sec, zi, plan, work, st);
  const SosGeom Gb = sos_geom(n_rows, row_stride, n_t, padlen);
  return with_float_type(dtype, [&](auto t) {
    return with_section_count(n_sec, [&](auto ns) {
      return sosfiltfilt_blocks<decltype(t), decltype(ns)::value>((decltype(t)*)x, Gb, sos, zi, work, st);
    });
  });
}

// without a plan: the same checks, and the recursion
DVH_API int dvh_sosfiltfilt(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t,
                            const double* sos, int32_t n_sec, int32_t padlen, const double* zi, double* work,
                            void* stream) {
  return dvh_sosfiltfilt_planned(x, dtype, n_rows, row_stride, n_t, sos, n_sec, padlen, zi, nullptr, work, stream);
}
