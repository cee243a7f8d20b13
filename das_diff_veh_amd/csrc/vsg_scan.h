// Window validity scan of the VSG stack launches (gfx950): device code shared by the validated stack kernel
// (dvh_vsg.hip: vsg_stackv_kernel) and the scan's own kernels.
//
// The reference divides every window by ||data||_F
// (preprocessing_window, apis/virtual_shot_gather.py:125): a NaN or inf anywhere in the window, or
// an all-zero window, makes the whole gather NaN (norm / norm_amp divide by a NaN or zero maximum
// afterwards), and so its class mean.  Deciding that needs every sample of the window, 4x - 130x the
// bytes the correlations read.  In the validated stack launch, besides the correlation waves, one
// to three waves per block (the launch's shape: dvh_vsg.hip, pick_vstack) stream the windows (16 x 16-byte loads per
// lane in flight) and keep the maximum
// of |x| as a bit pattern, max(bits & 0x7fffffff): >= 0x7f800000 means a NaN / inf, 0 means all
// zero.  Work is pulled in units of kScanRows channel rows from a global counter, by the scan waves
// from the start and by the correlation waves once their row tasks are done, so the HBM-bound scan
// runs under the VALU-bound transforms.  vsg_invalid_fill_kernel then sets the class slots holding an
// invalid pass to NaN.
//
// Scan windows: by default window s is pass s (win + s * pass_stride, n_ch rows), scanned in the
// correlation's class-sorted order so that both fronts start on the same passes (3.51 vs 3.53 ms per
// synth10k launch).  A unit launch (plan.UnitPlan: (pass, pivot) units over one flattened record) names
// its windows instead: scan_tab[s] = first record row of window s, and unit_scan[u] = the window whose
// flag unit u takes, so a pass imaged at several pivots is validated once per launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vsg_engines.h"

namespace dvh {

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

// the next index from a global work counter (one atomic per wave)
__device__ __forceinline__ int pull_unit(uint32_t* counter, int lane) {
  int u = 0;
  if (lane == 0) u = (int)atomicAdd(counter, 1u);
  return __builtin_amdgcn_readfirstlane(__shfl(u, 0));
}

constexpr int kScanRows = 16;
constexpr int kScanDepth = 16;  // 16-byte loads per lane in flight (8 / 12 / 24 measured no better)
constexpr int kScanAux = 2;     // cache policy of the scan's buffer loads (nt; allocating loads measured 4 % slower on
                                // synth10k)

__device__ __forceinline__ uint32_t absbits(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7fffffffu; }


// Buffer descriptor over [p, p + bytes) built from wave-uniform values (no waterfall loops around the
// loads); out-of-range loads return 0, which leaves a max |x| unchanged.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t scan_rsrc(const void* p, uint32_t bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  void* pu = reinterpret_cast<void*>(((uint64_t)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(pu, 0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// max |x| bit pattern over nf4 consecutive float4 (16-byte aligned): unconditional 16-byte buffer
// loads, kScanDepth per lane in flight (the descriptor's range check zeroes the tail)
template <int D = kScanDepth>
__device__ __forceinline__ uint32_t scan_span(const float* __restrict__ q, int nf4, int lane) {
  const __amdgpu_buffer_rsrc_t rs = scan_rsrc(q, (uint32_t)nf4 * 16u);
  const int nsteps = (nf4 + 63) >> 6;
  uint32_t m = 0;
  int off = lane * 16;
  u32x4 r[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    r[d] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, kScanAux);
    off += 1024;
  }
  for (int s0 = 0; s0 < nsteps; s0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const u32x4 v = r[d] & 0x7fffffffu;
      m = max(m, max(max(v.x, v.y), max(v.z, v.w)));
      r[d] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, kScanAux);
      off += 1024;
    }
  }
  return m;
}

// rows [c0, c1) of a window (n_t samples each): max |x| bit pattern over the wave
template <int D = kScanDepth>
__device__ __forceinline__ uint32_t scan_rows(const float* __restrict__ base, int64_t ch_stride, int c0, int c1,
                                              int n_t, bool vec, int lane) {
  uint32_t m = 0;
  if (vec && ch_stride == n_t) {  // the unit's rows are one contiguous span
    m = scan_span<D>(base + (int64_t)c0 * ch_stride, ((c1 - c0) * n_t) >> 2, lane);
  } else if (vec) {
    for (int c = c0; c < c1; ++c) m = max(m, scan_span<D>(base + (int64_t)c * ch_stride, n_t >> 2, lane));
  } else {
    for (int c = c0; c < c1; ++c)
      for (int t = lane; t < n_t; t += 64) m = max(m, absbits(base[(int64_t)c * ch_stride + t]));
  }
  return wave_max_u32(m);
}

struct ScanArgs {
  const int32_t* tab;  // nullptr: window s = pass s; else first record row of window s
  int32_t n_win;       // scan windows
  int32_t n_ch, n_t;   // rows and samples of one window
};

// ---- covered-span scan: the scan leaves out, per gather row, the float4s inside the row's correlated slices
// [a, a + (nwin - 1) hop + w) (both sides), which the correlation waves load and validate themselves (non-finite
// samples reach their spectra, or are checked where a sub-window is not transformed: FusedOps::check_untransformed).
// A row's remaining float4s are at most three spans; the wave streams them as one virtual index range, each lane's
// load address mapped past the skipped ranges (two compares), with kScanDepth loads in flight across row boundaries.
// Windows whose flag ends at 0 (nothing non-zero in the scanned part) or kSuspect are rescanned whole afterwards
// (window_fixup_kernel), so all-zero windows and non-finite spectra without a pass stay exact.
struct SpanRow {
  uint32_t base;  // byte offset of the row in the window (windows < 4 GiB)
  int U;         // float4s to scan
  int t0, d0;    // virtual index of the first skipped range, its length (float4)
  int s1, d1;    // start (real float4 index) and length of the second
};
// float4 range wholly inside side (a, L)'s correlated slices (empty when hop > w leaves gaps)
__device__ __forceinline__ void covered4(int a, int L, int w, int hop, int& b, int& e) {
  const int nw = n_subwin(L, w, hop);
  b = e = 0;
  if (nw <= 0 || hop > w) return;
  b = (a + 3) >> 2;
  e = (a + (nw - 1) * hop + w) >> 2;
  if (e < b) b = e = 0;
}
__device__ __forceinline__ SpanRow span_row(const VsgArgs& A, int p, int row0, int c, int n4) {
  SpanRow r;
  r.base = (uint32_t)((int64_t)c * A.ch_stride * 4);
  int b0 = 0, e0 = 0, b1 = 0, e1 = 0;
  const int i = c - row0;
  if (i >= 0 && i < A.R) {
    const int32_t* seg = A.seg_tab + ((int64_t)p * A.R + i) * 4;
    covered4(sld(seg), sld(seg + 1), A.w, A.hop, b0, e0);
    if (A.flags & kFlagOtherSide) covered4(sld(seg + 2), sld(seg + 3), A.w, A.hop, b1, e1);
  }
  if (e0 <= b0) b0 = e0 = n4;  // empty ranges sit past the row
  if (e1 <= b1) b1 = e1 = n4;
  if (b1 < b0) {  // ordered
    int t = b0; b0 = b1; b1 = t;
    t = e0; e0 = e1; e1 = t;
  }
  if (b1 < e0) {  // overlapping ranges merge
    e0 = max(e0, e1);
    b1 = e1 = n4;
  }
  e0 = min(e0, n4);
  e1 = min(e1, n4);
  r.t0 = b0;
  r.d0 = e0 - b0;
  r.s1 = b1;
  r.d1 = e1 - b1;
  r.U = n4 - r.d0 - r.d1;
  if (r.U == 0) r.U = 1;  // a wholly covered row reads one float4 again: no row is empty (one row switch per load)
  return r;
}
// rows [c0, c1) of pass p's window (n_t % 4 == 0, 16-byte aligned rows): max |x| bit pattern over the wave
// D: loads per lane in flight (the kernel's registers are sized for its correlation waves: EngF500's 128 VGPRs take
// 11, 12 spill)
template <int D>
__device__ __forceinline__ uint32_t scan_rows_span(const VsgArgs& A, const ScanArgs& S, int p, int c0, int c1, int lane) {
  const float* base = A.win + (int64_t)p * A.pass_stride;
  const int64_t wbytes = ((int64_t)(S.n_ch - 1) * A.ch_stride + S.n_t) * 4;  // < 0xfffffff0 (host)
  const __amdgpu_buffer_rsrc_t rs = scan_rsrc(base, (uint32_t)wbytes);
  const int row0 = sld(A.pass_tab + 2 * p), n4 = S.n_t >> 2;
  constexpr uint32_t kOut = 0xfffffff0u;  // past the descriptor's range: the load returns 0
  int c = c0, k = 0;
  SpanRow cur = span_row(A, p, row0, c, n4);
  auto issue = [&]() -> uint32_t {
    if (c < c1 && k * 64 >= cur.U) {  // next row (the loads in flight cover its table reads)
      ++c;
      k = 0;
      if (c < c1) cur = span_row(A, p, row0, c, n4);
    }
    if (c >= c1) return kOut;
    const int v = k * 64 + lane;
    ++k;
    int o = v + (v >= cur.t0 ? cur.d0 : 0);
    o += o >= cur.s1 ? cur.d1 : 0;
    return v < cur.U ? cur.base + (uint32_t)o * 16u : kOut;
  };
  uint32_t m = 0;
  u32x4 r[D];
#pragma unroll
  for (int d = 0; d < D; ++d) r[d] = __builtin_amdgcn_raw_buffer_load_b128(rs, issue(), 0, kScanAux);
  while (c < c1) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const u32x4 v = r[d] & 0x7fffffffu;
      m = max(m, max(max(v.x, v.y), max(v.z, v.w)));
      r[d] = __builtin_amdgcn_raw_buffer_load_b128(rs, issue(), 0, kScanAux);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const u32x4 v = r[d] & 0x7fffffffu;
    m = max(m, max(max(v.x, v.y), max(v.z, v.w)));
  }
  return wave_max_u32(m);
}

// Windows the covered-span scan could not decide -- flag 0 (the scanned part all zero: the slices may not be) or
// kSuspect -- are rescanned whole: one block per window, nothing to do for the usual flag.
__global__ __launch_bounds__(256) void window_fixup_kernel(VsgArgs A, ScanArgs S, uint32_t* __restrict__ vflag) {
  const int s = blockIdx.x;
  const uint32_t f0 = vflag[s];
  if (f0 != 0 && !(f0 & kSuspect)) return;
  __shared__ uint32_t part[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* base = A.win + (int64_t)s * A.pass_stride;
  uint32_t m = 0;
  for (int c = wave; c < S.n_ch; c += 4)
    for (int t = lane; t < S.n_t; t += 64) m = max(m, absbits(base[(int64_t)c * A.ch_stride + t]));
  m = wave_max_u32(m);
  if (lane == 0) part[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) vflag[s] = max(max(part[0], part[1]), max(part[2], part[3]));
}

// Pull scan units (window, kScanRows channel rows) until none is left; atomicMax into vflag[window].  span: the
// covered-span scan (default windows of a launch whose chunks list every pass), DS loads per lane in flight.
template <int D = kScanDepth, int DS = 8>
__device__ __forceinline__ void scan_units(const VsgArgs& A, const ScanArgs& S, uint32_t* __restrict__ vflag,
                                           uint32_t* __restrict__ counter, int lane,
                                           const int32_t* __restrict__ sorder = nullptr, bool span = false) {
  const int upp = (S.n_ch + kScanRows - 1) / kScanRows;  // units per window
  const int n_units = S.n_win * upp;
  const bool vec = (S.n_t % 4 == 0) && (A.ch_stride % 4 == 0) && (A.pass_stride % 4 == 0) &&
                   (reinterpret_cast<uintptr_t>(A.win) % 16 == 0);
  int u = pull_unit(counter, lane);
  while (u < n_units) {
    const int un = pull_unit(counter, lane);  // the next unit's index, fetched under this unit's loads
    const int q = u / upp, c0 = (u - q * upp) * kScanRows;
    const int s = (sorder && !S.tab) ? sld(sorder + q) : q;
    const float* base = S.tab ? A.win + (int64_t)sld(S.tab + s) * A.ch_stride : A.win + (int64_t)s * A.pass_stride;
    const uint32_t m = span ? scan_rows_span<DS>(A, S, s, c0, min(c0 + kScanRows, S.n_ch), lane)
                            : scan_rows<D>(base, A.ch_stride, c0, min(c0 + kScanRows, S.n_ch), S.n_t, vec, lane);
    if (lane == 0) atomicMax(vflag + s, m);
    u = un;
  }
}

// The validity scan alone (correlation engines without a validated stack kernel).
__global__ __launch_bounds__(256) void window_scan_kernel(VsgArgs A, ScanArgs S, uint32_t* __restrict__ vflag,
                                                          uint32_t* __restrict__ counter) {
  scan_units(A, S, vflag, counter, threadIdx.x & 63);
}

}  // namespace dvh
