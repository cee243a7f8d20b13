// Per-wave correlation engines of the VSG kernels (gfx950).
//
// An engine turns one gather row task (pass p, row i) into the raw circular correlations of both
// sides, c_f[k] and c_o[k] (k < w), summed over the row's sub-windows and scaled by N * nwin:
//   for every sub-window, z = pivot + i * receiver -> one complex FFT -> cross spectrum
//   P conj(R) = (i/4)(Z[f] + conj Z[-f]) conj(Z[f] - conj Z[-f]) accumulated per side in registers,
//   then ONE inverse FFT of Cf + i Co (real part -> forward side, imaginary -> other side).
// The cross spectra of real correlations are Hermitian, so only bins f <= N/2 are accumulated
// (NH per lane, f = lane + 64 j); the inverse writes both W[f] and W[N - f].
// A sub-window whose pivot or receiver slice is identically zero contributes exactly zero in the
// reference; the engines test every loaded sample (bit pattern, so NaN counts as non-zero) and skip
// such sub-windows, and report per side whether anything was accumulated (live_f / live_o), so that
// an all-zero side is exactly zero (and yields the reference's 0/0 = NaN where it normalises).
//
//   EngStockham<N, PAD>  any supported N: LDS ping-pong Stockham transform (fft_wave.h), sub-window
//                        loads staged in registers one sub-window ahead.  PAD: N >= 2w - 1 zero padded,
//                        linear correlation folded back to circular in c().
//   EngF500              N = w = 500 (wlen = 2 s at 250 Hz, the reference's operating point): the
//                        10 x 10 x 5 Stockham transform with its first and last stages in registers.
//   EngP1024             w <= 512 without an exact engine (w = 499): zero-padded 4^5 transform, first and
//                        last stages in registers, as EngF500 (pivot-slice table, cross-pass packing).
// (Engine variants measured and not kept are listed in DESIGN.md.)
//
// Each engine states its own facts once, as constants the kernels and the host's engine table (dvh_vsg.hip) read:
//   NFFT       the transform length;
//   kExact     NFFT = w (stackf_tasks), else NFFT >= 2w - 1 zero padded (stackp_tasks, the fold in corr_at());
//   kFused     a FusedOps engine: takes the pivot-slice table and packs single-sided tasks across passes;
//   kDeckLoop  (fused engines) the stack kernels' pass loop takes its table words from the task deck;
//   kOcc       waves / SIMD its scales and gather kernels are compiled for;
//   kOccStack  waves / SIMD its plain stack kernel is compiled for;
//   kWaves     waves per block;  NJ: lags per lane in the epilogues;  NH: half-spectrum slots per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_wave.h"
#include "tw_tables.h"


namespace dvh {


enum : int32_t {
  kFlagOtherSide = 1,
  kFlagNorm = 2,
  kFlagNormAmp = 4,
};

struct VsgArgs {
  const float* win;
  int64_t pass_stride;
  int64_t ch_stride;
  const int32_t* pass_tab;
  const int32_t* seg_tab;
  int32_t n_pass;
  int32_t R;
  int32_t w;
  int32_t hop;
  int32_t flags;
};

__device__ __forceinline__ int pmod(int a, int m) {
  const int r = a % m;
  return r < 0 ? r + m : r;
}

__device__ __forceinline__ int n_subwin(int L, int w, int hop) { return (L >= w) ? (L - w) / hop + 1 : 0; }

// Wave-uniform value (keeps table indices and table entries in SGPRs -> scalar loads).
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float unif(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// Wave-uniform load through the scalar cache (s_load).  The tables the kernels read (pass / segment / chunk
// tables, order, scales, weights, the pivot-spectra table) are written only by earlier launches, so the
// constant address space is safe; it keeps these dependent loads off the vector memory pipe, where they
// queued behind the receiver loads.  The address must be wave-uniform.
template <class T>
__device__ __forceinline__ T sld(const T* p) {
  return *(const __attribute__((address_space(4))) T*)p;
}

// Everything a row task needs, wave-uniform.
struct RowTask {
  const float* piv;
  const float* rcv;
  int a_f, nwin_f, a_o, nwin_o;
  int ch, pivot;
  int p, row0;
};

__device__ __forceinline__ RowTask make_task(const VsgArgs& A, int p, int i) {
  p = uni(p);
  i = uni(i);
  RowTask t;
  const int row0 = sld(A.pass_tab + 2 * p);
  t.p = p;
  t.row0 = row0;
  t.pivot = sld(A.pass_tab + 2 * p + 1);
  t.ch = row0 + i;
  const float* base = A.win + (int64_t)p * A.pass_stride;
  t.piv = base + (int64_t)t.pivot * A.ch_stride;
  t.rcv = base + (int64_t)t.ch * A.ch_stride;
  const int32_t* seg = A.seg_tab + ((int64_t)p * A.R + i) * 4;
  t.a_f = sld(seg);
  t.nwin_f = n_subwin(sld(seg + 1), A.w, A.hop);
  const bool other = (A.flags & kFlagOtherSide) != 0;
  t.a_o = sld(seg + 2);
  t.nwin_o = other ? n_subwin(sld(seg + 3), A.w, A.hop) : 0;
  return t;
}

// Opaque copy of a per-lane value: index arithmetic derived from it stays where it is used instead
// of being hoisted to the kernel entry (where, for per-task paths, it only occupies registers across the
// whole task loop and gets spilled once per wave).
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// |x| != 0 as a bit mask (NaN included); OR-accumulate, test once per sub-window
__device__ __forceinline__ uint32_t nzbits(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7fffffffu; }
// OR-accumulated non-zero bits of the loaded samples (one v_and_or per sample)
__device__ __forceinline__ uint32_t maxbits(uint32_t b, float x) { return b | nzbits(x); }
// Validity flags of the covered-span scan (vsg_scan.h): per pass the max |x| bit pattern of the samples the scan
// read (>= kInfBits: a NaN / inf), or'ed with kSuspect when a correlation wave saw a non-finite spectrum it cannot
// attribute to one pass (the window is then rescanned whole).
constexpr uint32_t kInfBits = 0x7f800000u, kSuspect = 0x80000000u;

__device__ __forceinline__ void accumulate_cross(float2 Az, float2 Bc, float2& C) {
  // P = (A + B) / 2, R = (A - B) / 2i with B = conj(Bc)  ->  P conj(R) = (i / 4) (A + B) conj(A - B)
  const float bx = Bc.x, by = -Bc.y;
  C.x += 0.5f * (bx * Az.y - by * Az.x);
  C.y += 0.25f * ((Az.x * Az.x + Az.y * Az.y) - (bx * bx + by * by));
}

// conj(W) for W = Cf + i Co over all N bins from the half spectra held in the engine's slots
// (slot j of a lane is bin E::bin(lane, j) <= N/2, or -1): the input of the inverse transform
// conj(FFT(conj(W))).  W[N - f] = conj(Cf[f]) + i conj(Co[f]).
template <class E>
__device__ __forceinline__ void store_conj_hermitian(float2* buf, const float2 (&Cf)[E::NH], const float2 (&Co)[E::NH],
                                                     int lane_) {
  constexpr int N = E::NFFT;
  const int lane = opaque(lane_);
#pragma unroll
  for (int j = 0; j < E::NH; ++j) {
    const int f = E::bin(lane, j);
    if (f >= 0) {
      buf[f] = make_float2(Cf[j].x - Co[j].y, -(Cf[j].y + Co[j].x));
      if (f > 0 && f < N / 2) buf[N - f] = make_float2(Cf[j].x + Co[j].y, Cf[j].y - Co[j].x);
    }
  }
}

// One row task's correlations: the accumulated cross spectra of both sides, then the one inverse transform.
// Returns Y with Y[k].x = N * IDFT(Cf)[k], -Y[k].y = N * IDFT(Co)[k], read through E::c().
template <class E>
__device__ __forceinline__ const float2* correlate(E& eng, const RowTask& t, int w, int hop) {
  float2 Cf[E::NH], Co[E::NH];
  eng.spectra(t, w, hop, Cf, Co);
  return eng.inverse(Cf, Co);
}

// (N * sum_s c_f[k], N * sum_s c_o[k]) at lag k of the inverse transform's output Y.  PAD: the linear correlation
// of the zero-padded sub-windows folded to the circular one of period w.
template <int N, bool PAD>
__device__ __forceinline__ float2 corr_at(const float2* Y, int k, int w) {
  float2 v = Y[k];
  if (PAD && k > 0) {
    const float2 u = Y[N - w + k];
    v.x += u.x;
    v.y += u.y;
  }
  return make_float2(v.x, -v.y);
}

// ------------------------------------------------------------------------------------------------
template <int N, bool PAD>
struct EngStockham {
  static constexpr int NFFT = N;
  static constexpr int kWaves = 4;
  static constexpr bool kExact = !PAD;
  static constexpr bool kFused = false;
  static constexpr int kOcc = 3;  // register-limited to 3 waves / SIMD
  // plain stack kernel: 4 for the exact transforms up to N = 500 (their spills at 128 VGPRs sit in the rare
  // time-domain fallback only); the padded N >= 1024 hold two accumulated side spectra besides the sub-window's
  // and would spill at 3
  static constexpr int kOccStack = PAD ? (N >= 1024 ? 2 : kOcc) : (N <= 500 ? 4 : kOcc);
  static constexpr int NJ = (N + 63) / 64;
  static constexpr int NH = (N / 2 + 1 + 63) / 64;
  static_assert(N % 2 == 0, "Hermitian half spectra assume an even length");
  static constexpr size_t kBlockBytes = sizeof(float2) * N;        // twiddle table
  static constexpr size_t kWaveBytes = sizeof(float2) * 2 * N;     // ping-pong buffers
  float2* tw;
  float2* bufA;
  float2* bufB;
  int lane;
  bool live_f, live_o;  // some sub-window of the side had non-zero pivot and receiver slices

  __device__ EngStockham(char* lds, int wave, int lane_) : lane(lane_), live_f(false), live_o(false) {
    tw = reinterpret_cast<float2*>(lds);
    bufA = reinterpret_cast<float2*>(lds + kBlockBytes + (size_t)wave * kWaveBytes);
    bufB = bufA + N;
  }
  static __device__ void block_init(char* lds) { init_twiddles<N>(reinterpret_cast<float2*>(lds)); }

  // sub-window samples staged in registers; a padded transform (w <= N / 2) only has samples n < N / 2, the
  // upper half of its input is zero (stored once per sub-window, no registers)
  static constexpr int NZ = PAD ? (N / 2 + 63) / 64 : NJ;
  __device__ void load(const RowTask& t, int a, int w, float2 (&z)[NZ]) const {
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      const int n = lane + 64 * j;
      z[j] = (n < w) ? make_float2(t.piv[a + n], t.rcv[a + n]) : make_float2(0.f, 0.f);
    }
  }

  // accumulated cross spectra of both sides: Cf[j], Co[j] at bins f = lane + 64 j
  __device__ void spectra(const RowTask& t, int w, int hop, float2 (&Cf)[NH], float2 (&Co)[NH]) {
    const int nq = t.nwin_f + t.nwin_o;
    float2 z[NZ];
#pragma unroll
    for (int j = 0; j < NH; ++j) {
      Cf[j] = make_float2(0.f, 0.f);
      Co[j] = make_float2(0.f, 0.f);
    }
    live_f = live_o = false;
    if (nq > 0) load(t, t.nwin_f > 0 ? t.a_f : t.a_o, w, z);
    for (int q = 0; q < nq; ++q) {
      uint32_t bp = 0, br = 0;
#pragma unroll
      for (int j = 0; j < NZ; ++j) {
        const int n = lane + 64 * j;
        if (n < N) bufA[n] = z[j];
        bp |= nzbits(z[j].x);
        br |= nzbits(z[j].y);
      }
      if (PAD) {
#pragma unroll
        for (int j = NZ; j < NJ; ++j) {
          const int n = lane + 64 * j;
          if (n < N) bufA[n] = make_float2(0.f, 0.f);
        }
      }
      const bool live = (__ballot(bp != 0) != 0) && (__ballot(br != 0) != 0);
      if (q + 1 < nq) {
        const int qn = q + 1;
        load(t, qn < t.nwin_f ? t.a_f + qn * hop : t.a_o + (qn - t.nwin_f) * hop, w, z);
      }
      if (!live) continue;  // exactly zero in the reference
      if (q < t.nwin_f) live_f = true;
      else live_o = true;
      wave_sync();
      const float2* X = FftPlan<N>::T::run(bufA, bufB, tw, lane);
      if (q < t.nwin_f) {
#pragma unroll
        for (int j = 0; j < NH; ++j) {
          const int f = lane + 64 * j;
          if (f <= N / 2) accumulate_cross(X[f], X[f == 0 ? 0 : N - f], Cf[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < NH; ++j) {
          const int f = lane + 64 * j;
          if (f <= N / 2) accumulate_cross(X[f], X[f == 0 ? 0 : N - f], Co[j]);
        }
      }
      wave_sync();
    }
  }

  // half-spectrum slot j of a lane holds bin f = lane + 64 j (f <= N/2)
  static __device__ __forceinline__ int bin(int lane, int j) {
    const int f = lane + 64 * j;
    return f <= N / 2 ? f : -1;
  }

  // Y with Y[k].x = N * IDFT(Cf)[k], -Y[k].y = N * IDFT(Co)[k] (read through c())
  __device__ const float2* inverse(const float2 (&Cf)[NH], const float2 (&Co)[NH]) {
    store_conj_hermitian<EngStockham>(bufA, Cf, Co, lane);
    wave_sync();
    return FftPlan<N>::T::run(bufA, bufB, tw, lane);
  }

  // twiddle exp(-2 pi i m / N), m in [0, N)
  __device__ float2 twiddle(int m) const { return tw[m]; }

  __device__ float2 c(const float2* Y, int k, int w) const { return corr_at<N, PAD>(Y, k, w); }
};

// ------------------------------------------------------------------------------------------------
// Per-pass table of pivot-slice spectra (FusedOps::spectra_tab).  A pass's rows read the pivot channel at
// few distinct slices: every row of a shared side (channel <= pivot forward, >= pivot other side,
// apis/virtual_shot_gather.py:145-180) at the pivot's own time window, and the trajectory rows whose
// trajectory time lies outside the record at the clamped window (argmax of an all-False mask is 0,
// virtual_shot_gather.py:29, so they all slice [0, nsamp)).  Entry e of pass p holds the spectra of the
// slices [start_e + q hop, + w), q < nwin_e:
//   e = 0: the forward shared window (the pivot row's forward slice), e = 1: the other side's,
//   e = 2: the forward trajectory window of the last gather row, e = 3: the other-side trajectory window
//   of the first gather row (the far rows' clamped windows).
// A row side whose (start, nwin) equals its entry's transforms only its receivers, two per complex FFT.
// An entry holds kTabSub = 3 sub-windows (the reference's default time_window_to_xcorr = 2 wlen: nwin = 3).
// A pass with a longer side is marked unusable in the head (every nwin = -1; tab_usable() is false) and
// its row tasks take the plain path.  BINS (per engine): the half-spectrum bins f <= N / 2 of P / 2 (the
// halving of z's separation folded in, exact), and at [BINS - 1].x a 1 when the slice has a non-zero sample.
constexpr int kTabEnt = 4;
constexpr int kTabSub = 3;

template <int BINS>
__device__ __forceinline__ const float2* tab_slice(const float2* tab, int p, int e, int q) {
  return tab + (((int64_t)p * kTabEnt + e) * kTabSub + q) * BINS;
}
template <int BINS>
constexpr int64_t tab_pass_f2() {
  return (int64_t)kTabEnt * kTabSub * BINS;  // float2 per pass
}
// (start, nwin) of every entry: int32 [n_pass][kTabEnt][2] after the spectra
template <int BINS>
__device__ __forceinline__ const int32_t* tab_head(const float2* tab, int n_pass) {
  return reinterpret_cast<const int32_t*>(tab + (int64_t)n_pass * tab_pass_f2<BINS>());
}

// ------------------------------------------------------------------------------------------------
// FusedOps<E>: the row-task logic of the engines whose first and last transform stages run in registers
// (EngF500, EngP1024).  E provides the transform: NFFT, kNJ (E::kNZ, the sample registers per lane; not E::NJ, the
// lags per lane of the epilogues in dvh_vsg.hip), NH (half-spectrum slots per lane), kTabBins, bin(l, j),
// load_ri() (a sub-window's samples into registers), stage1() (registers -> LDS), finish_with(acc) (the remaining stages, then acc(j, Z[f], Z[N - f]) for every half-spectrum slot j
// of the lane), inverse() and c() (the correlation at lag k after the inverse).  FusedOps holds the per-wave
// state and the three ways a row task forms its accumulated cross spectra:
//   spectra():     one complex transform per sub-window, z = pivot + i receiver;
//   spectra_tab(): the sub-windows whose pivot slices the pass table holds cost only their receivers, two
//                  per transform (z = R_a + i R_b, separated in the last stage and multiplied into the
//                  table's P conj(R)); the others keep z = P + i R.  On the configs[2] geometry that is 2
//                  transforms for a row whose only side is shared and 3 for a far row with both sides,
//                  against 3 and 6;
//   direct_task(): a task whose passes have only a table-served forward side packs receivers two per
//                  transform ACROSS its passes.
template <class E, int kNJ, int kNH>
struct FusedOps {
  float2* tw;
  float2* bufA;
  float2* bufB;
  int lane;
  bool live_f, live_o;
  const float2* tab = nullptr;  // the pass table of pivot spectra (stack kernels), or none
  int w;                        // sub-window length: the padded engines load samples n < w
  uint32_t* vflag = nullptr;    // validated launch with the covered-span scan: the passes' validity flags, to which
                                // the correlation reports the non-finite samples it loads (the scan leaves them out)

  __device__ FusedOps(char* lds, int wave, int lane_, int w_) : lane(lane_), live_f(false), live_o(false), w(w_) {
    tw = reinterpret_cast<float2*>(lds);
    bufA = reinterpret_cast<float2*>(lds + E::kBlockBytes + (size_t)wave * E::kWaveBytes);
    bufB = bufA + E::kBufA;
  }
  __device__ __forceinline__ const E& self() const { return *static_cast<const E*>(this); }

  __device__ __forceinline__ void load(const RowTask& t, int a, float2 (&z)[kNJ]) const {
    self().load_ri(t.piv + a, t.rcv + a, z);
  }
  // the stages after stage 1 of the transform whose stage-1 output is in bufB; cross spectra into C
  __device__ __forceinline__ void finish(float2 (&C)[kNH]) const {
    self().finish_with([&](int j, float2 a, float2 b) { accumulate_cross(a, b, C[j]); });
  }

  // Covered-span scan: a loaded sub-window that is not transformed (a zero pivot or receiver slice) is checked here
  // for non-finite samples (rare); a transformed one carries them into the accumulated spectra, which the stack
  // tasks test.  p2 < 0: both halves of z belong to pass p; else the real half to p, the imaginary half to p2.
  __device__ void check_untransformed(const float2 (&z)[kNJ], int p, int p2 = -1) const {
    if (!vflag) return;
    uint32_t ma = 0, mb = 0;
#pragma unroll
    for (int j = 0; j < kNJ; ++j) {
      ma = max(ma, nzbits(z[j].x));
      mb = max(mb, nzbits(z[j].y));
    }
    const bool ba = __ballot(ma >= kInfBits) != 0, bb = __ballot(mb >= kInfBits) != 0;
    if (lane == 0) {
      if (p2 < 0) {
        if (ba || bb) atomicMax(vflag + p, kInfBits);
      } else {
        if (ba) atomicMax(vflag + p, kInfBits);
        if (bb) atomicMax(vflag + p2, kInfBits);
      }
    }
  }

  // the pass's table entries hold all its sub-windows (head nwin of entry 0 >= 0)
  __device__ __forceinline__ bool tab_usable(int p, int n_pass) const {
    return sld(tab_head<E::kTabBins>(tab, n_pass) + (int64_t)p * kTabEnt * 2 + 1) >= 0;
  }

  // Sub-window q's pivot and receiver samples are loaded one sub-window ahead.
  __device__ void spectra(const RowTask& t, int, int hop, float2 (&Cf)[kNH], float2 (&Co)[kNH]) {
    constexpr int NH_ = kNH;
    const int nq = t.nwin_f + t.nwin_o;
#pragma unroll
    for (int j = 0; j < NH_; ++j) {
      Cf[j] = make_float2(0.f, 0.f);
      Co[j] = make_float2(0.f, 0.f);
    }
    live_f = live_o = false;
    auto start = [&](int q) { return q < t.nwin_f ? t.a_f + q * hop : t.a_o + (q - t.nwin_f) * hop; };
    float2 z[kNJ];
    if (nq > 0) load(t, start(0), z);
    for (int q = 0; q < nq; ++q) {
      uint32_t bp = 0, br = 0;
#pragma unroll
      for (int j = 0; j < kNJ; ++j) {
        bp = maxbits(bp, z[j].x);
        br = maxbits(br, z[j].y);
      }
      const bool live = (__ballot(bp != 0) != 0) && (__ballot(br != 0) != 0);
      if (live) self().stage1(z);
      else check_untransformed(z, t.p);
      if (q + 1 < nq) load(t, start(q + 1), z);
      if (!live) continue;  // exactly zero in the reference
      if (q < t.nwin_f) {
        live_f = true;
        finish(Cf);
      } else {
        live_o = true;
        finish(Co);
      }
    }
  }

  // ---- spectra_tab: the sub-windows whose pivot slices the table holds cost only their receivers ----
  // Transforms of a row task (wave-uniform): jobs k < npair pack the table-served receivers h = 2k, 2k + 1
  // (h < nrf: forward side, sub-window h, entry ef; then the other side, entry eo); the remaining nt
  // trajectory sub-windows (side ts, start at) are z = P + i R as in spectra().
  struct TabJobs {
    int nrf, nr, ef, eo, ts, at, nt, npair;
  };
  // a trajectory side matches its far-row entry (head words 4..7) when its slices are the same
  static __device__ __forceinline__ bool far_match(int a, int nwin, int start, int count) {
    return nwin > 0 && a == start && nwin == count;
  }
  // farf / faro: far_match() of the row's forward / other side
  static __device__ __forceinline__ TabJobs tab_jobs(const RowTask& t, bool farf, bool faro) {
    TabJobs J;
    const bool shf = t.ch <= t.pivot, sho = t.ch >= t.pivot;
    const bool mf = shf || farf;
    const bool mo = sho || faro;
    J.ef = shf ? 0 : 2;
    J.eo = sho ? 1 : 3;
    J.nrf = mf ? t.nwin_f : 0;
    J.nr = J.nrf + (mo ? t.nwin_o : 0);
    J.ts = !mf ? 0 : 1;
    J.nt = !mf ? t.nwin_f : (!mo ? t.nwin_o : 0);
    J.at = J.ts == 0 ? t.a_f : t.a_o;
    J.npair = (J.nr + 1) >> 1;
    return J;
  }
  // table-served receiver h: side, sub-window, slice start
  __device__ __forceinline__ void tab_half(const RowTask& t, const TabJobs& J, int h, int hop, int& side, int& q,
                                           int& a) const {
    side = h < J.nrf ? 0 : 1;
    q = h < J.nrf ? h : h - J.nrf;
    a = (side == 0 ? t.a_f : t.a_o) + q * hop;
  }
  __device__ __forceinline__ void tab_load(const RowTask& t, const TabJobs& J, int k, int hop,
                                           float2 (&z)[kNJ]) const {
    if (k < J.npair) {
      int s0, q0, a0, s1, q1, a1;
      tab_half(t, J, 2 * k, hop, s0, q0, a0);
      tab_half(t, J, 2 * k + 1, hop, s1, q1, a1);
      self().load_ri(t.rcv + a0, 2 * k + 1 < J.nr ? t.rcv + a1 : nullptr, z);
    } else {
      const int a = J.at + (k - J.npair) * hop;
      self().load_ri(t.piv + a, t.rcv + a, z);
    }
  }

  // The non-zero flags of the table slices a row can use, bit side * kTabSub + q (side 0: entry ef, 1: entry
  // eo), read from the table one by one (a task without a deck).
  __device__ __forceinline__ uint32_t tab_flags(const RowTask& t, const TabJobs& J) const {
    constexpr int BINS = E::kTabBins;
    // all loads issued together (one scalar round trip); a slice the row does not use reads slice 0's flag instead
    float v[2 * kTabSub];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int q = 0; q < kTabSub; ++q) {
        const bool on = q < (s == 0 ? J.nrf : J.nr - J.nrf);
        v[s * kTabSub + q] = sld(&tab_slice<BINS>(tab, t.p, s == 0 ? J.ef : J.eo, on ? q : 0)[BINS - 1].x);
      }
    }
    uint32_t fl = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int q = 0; q < kTabSub; ++q) {
        const bool on = q < (s == 0 ? J.nrf : J.nr - J.nrf);
        if (on && v[s * kTabSub + q] != 0.f) fl |= 1u << (s * kTabSub + q);
      }
    }
    return fl;
  }

  // fl: the slices' non-zero flags (tab_flags(), or the deck's)
  __device__ void spectra_tab(const RowTask& t, const TabJobs& J, uint32_t fl, int hop, float2 (&Cf)[kNH],
                              float2 (&Co)[kNH]) {
    constexpr int NH_ = kNH, BINS = E::kTabBins;
#pragma unroll
    for (int j = 0; j < NH_; ++j) {
      Cf[j] = make_float2(0.f, 0.f);
      Co[j] = make_float2(0.f, 0.f);
    }
    live_f = live_o = false;
    const int nj = J.npair + J.nt;
    float2 z[kNJ];
    if (nj > 0) tab_load(t, J, 0, hop, z);
    for (int k = 0; k < nj; ++k) {
      const bool pairjob = k < J.npair;
      uint32_t bp = 0, br = 0;
#pragma unroll
      for (int j = 0; j < kNJ; ++j) {
        bp = maxbits(bp, z[j].x);
        br = maxbits(br, z[j].y);
      }
      const bool nzp = __ballot(bp != 0) != 0, nzr = __ballot(br != 0) != 0;
      int s0 = 0, q0 = 0, a0 = 0, s1 = 0, q1 = 0, a1 = 0;
      bool la = false, lb = false;
      const float2 *Pa = nullptr, *Pb = nullptr;
      if (pairjob) {
        tab_half(t, J, 2 * k, hop, s0, q0, a0);
        tab_half(t, J, 2 * k + 1, hop, s1, q1, a1);
        Pa = tab_slice<BINS>(tab, t.p, s0 == 0 ? J.ef : J.eo, q0);
        Pb = tab_slice<BINS>(tab, t.p, s1 == 0 ? J.ef : J.eo, q1);
        // a receiver slice or its pivot slice identically zero: exactly zero in the reference
        la = nzp && ((fl >> (s0 * kTabSub + q0)) & 1u) != 0;
        lb = (2 * k + 1 < J.nr) && nzr && ((fl >> (s1 * kTabSub + q1)) & 1u) != 0;
      }
      const bool live = pairjob ? (la || lb) : (nzp && nzr);
      if (live) self().stage1(z);
      else check_untransformed(z, t.p);
      if (k + 1 < nj) tab_load(t, J, k + 1, hop, z);
      if (!live) continue;
      if (pairjob) {
        // the table's P at this lane's bins, loaded under the middle stages
        float2 pa[NH_], pb[NH_];
#pragma unroll
        for (int j = 0; j < NH_; ++j) {
          const int f = max(E::bin(lane, j), 0);
          pa[j] = Pa[f];
          pb[j] = Pb[f];
        }
        if (la) {
          if (s0 == 0) live_f = true;
          else live_o = true;
        }
        if (lb) {
          if (s1 == 0) live_f = true;
          else live_o = true;
        }
        const bool fa = s0 == 0, fb = s1 == 0;
        self().finish_with([&](int j, float2 za, float2 zc) {
          // z = R_a + i R_b: R_a = (Z[f] + conj Z[-f]) / 2, R_b = (Z[f] - conj Z[-f]) / 2i; P conj(R)
          if (la) {
            const float2 r = make_float2(za.x + zc.x, za.y - zc.y);  // 2 R_a (the table holds P / 2)
            const float2 c = make_float2(pa[j].x * r.x + pa[j].y * r.y, pa[j].y * r.x - pa[j].x * r.y);
            float2& C = fa ? Cf[j] : Co[j];
            C.x += c.x;
            C.y += c.y;
          }
          if (lb) {
            const float2 r = make_float2(za.y + zc.y, zc.x - za.x);  // 2 R_b
            const float2 c = make_float2(pb[j].x * r.x + pb[j].y * r.y, pb[j].y * r.x - pb[j].x * r.y);
            float2& C = fb ? Cf[j] : Co[j];
            C.x += c.x;
            C.y += c.y;
          }
        });
      } else if (J.ts == 0) {
        live_f = true;
        finish(Cf);
      } else {
        live_o = true;
        finish(Co);
      }
    }
  }

  // ---- The task deck: everything the passes of one (chunk, row) task need from the tables, lane k = pass
  // order[b + k], loaded together at the start of the task (one dependent round after `order`, and the slices'
  // non-zero flags one round later, when the row's table entries are known) and handed out by readlane:
  // direct_task takes the whole deck, the pass loop of an engine with kDeckLoop a hand of it (below), and no
  // table load is left in that loop or in the job loops.  A task with more than 64 passes, or a side with
  // kDeckNwin sub-windows or more, has no deck (n = 0) and reads its tables pass by pass.
  static constexpr int kDeckNwBits = 11, kDeckNwin = 1 << kDeckNwBits;
  enum : uint32_t {
    kDeckUsable = 1u << (2 * kDeckNwBits),  // tab_usable()
    kDeckFarF = kDeckUsable << 1,           // far_match() of the forward / other side
    kDeckFarO = kDeckUsable << 2,
    kDeckFlag0 = 2 * kDeckNwBits + 3,       // first bit of the slices' non-zero flags (tab_flags() order)
  };
  struct Deck {
    int n = 0;
    int p = 0, ch = 0, pivot = 0, a_f = 0, a_o = 0;
    uint32_t word = 0;  // nwin_f | nwin_o << kDeckNwBits | kDeckUsable.. | flags << kDeckFlag0
    float sf = 0.f, so = 0.f, wp = 0.f;
  };
  __device__ Deck deal(const VsgArgs& A, const float* __restrict__ scales, const int32_t* __restrict__ order,
                       const float* __restrict__ weight, int b, int e, int i) const {
    constexpr int BINS = E::kTabBins;
    Deck D;
    const int n = e - b;
    if (!tab || n < 1 || n > 64) return D;
    const bool other = (A.flags & kFlagOtherSide) != 0;
    const int ln = opaque(lane);  // per-task addresses formed here, not held across the task loop
    const bool act = ln < n;
    int row0 = 0, L = 0, Lo = 0, h1 = -1, h4 = -1, h5 = -1, h6 = -1, h7 = -1;
    if (act) {
      D.p = order[b + ln];
      row0 = A.pass_tab[2 * D.p];
      D.pivot = A.pass_tab[2 * D.p + 1];
      const int32_t* seg = A.seg_tab + ((int64_t)D.p * A.R + i) * 4;
      D.a_f = seg[0];
      L = seg[1];
      D.a_o = seg[2];
      Lo = seg[3];
      const int32_t* head = tab_head<BINS>(tab, A.n_pass) + (int64_t)D.p * kTabEnt * 2;
      h1 = head[1];
      h4 = head[4];
      h5 = head[5];
      h6 = head[6];
      h7 = head[7];
      D.sf = scales[2 * D.p];
      D.so = scales[2 * D.p + 1];
      D.wp = weight[D.p];
    }
    D.ch = row0 + i;
    const int nwf = n_subwin(L, A.w, A.hop), nwo = other ? n_subwin(Lo, A.w, A.hop) : 0;
    if (__ballot(nwf >= kDeckNwin || nwo >= kDeckNwin) != 0) return D;
    const bool usable = act && h1 >= 0;
    uint32_t word = (uint32_t)nwf | (uint32_t)nwo << kDeckNwBits;
    if (usable) {
      word |= kDeckUsable;
      if (far_match(D.a_f, nwf, h4, h5)) word |= kDeckFarF;
      if (far_match(D.a_o, nwo, h6, h7)) word |= kDeckFarO;
      // a usable pass's table holds kTabSub slices per entry (absent ones zero, flag 0)
      const float2* Pf = tab_slice<BINS>(tab, D.p, D.ch <= D.pivot ? 0 : 2, 0);
      const float2* Po = tab_slice<BINS>(tab, D.p, D.ch >= D.pivot ? 1 : 3, 0);
      float ff[kTabSub], fo[kTabSub];
#pragma unroll
      for (int q = 0; q < kTabSub; ++q) {
        ff[q] = Pf[q * BINS + BINS - 1].x;
        fo[q] = Po[q * BINS + BINS - 1].x;
      }
#pragma unroll
      for (int q = 0; q < kTabSub; ++q) {
        if (ff[q] != 0.f) word |= 1u << (kDeckFlag0 + q);
        if (fo[q] != 0.f) word |= 1u << (kDeckFlag0 + kTabSub + q);
      }
    }
    D.word = word;
    D.n = n;
    return D;
  }
  // A hand: kHand passes of a deck, kHandPer fields to a register (field f of pass k in lane kHand (f % kHandPer)
  // + k of register f / kHandPer), which is what the pass loop holds: two registers instead of the deck's nine
  // (the deck itself lives only from deal() to direct_task()).  A task with more passes deals a new hand every
  // kHand passes.
  static constexpr int kHand = 8, kHandPer = 64 / kHand;  // passes of a hand, fields to a register
  enum { kHP, kHCh, kHPivot, kHWord, kHAf, kHAo, kHSf, kHSo, kHWp, kHFields };
  struct Hand {
    int n = 0;  // passes held; 0: none
    int first = 0;  // index into `order` of pass 0
    int v[(kHFields + kHandPer - 1) / kHandPer] = {};
  };
  __device__ Hand hand(const Deck& D, int first) const {
    Hand H;
    if (D.n == 0) return H;
    const int ln = opaque(lane);
    const int src = ln & (kHand - 1), grp = ln / kHand;
    const int f[kHFields] = {D.p, D.ch, D.pivot, (int)D.word, D.a_f, D.a_o, __builtin_bit_cast(int, D.sf),
                             __builtin_bit_cast(int, D.so), __builtin_bit_cast(int, D.wp)};
#pragma unroll
    for (int r = 0; r < (kHFields + kHandPer - 1) / kHandPer; ++r) {
      int v = 0;
#pragma unroll
      for (int g = 0; g < kHandPer; ++g) {
        if (kHandPer * r + g < kHFields) {
          const int x = __shfl(f[kHandPer * r + g], src);
          v = grp == g ? x : v;
        }
      }
      H.v[r] = v;
    }
    H.n = min(D.n, kHand);
    H.first = first;
    return H;
  }
  // field f of pass k of the hand (wave-uniform)
  __device__ __forceinline__ int hand_i(const Hand& H, int f, int k) const {
    return __builtin_amdgcn_readlane(H.v[f / kHandPer], (f % kHandPer) * kHand + k);
  }
  __device__ __forceinline__ float hand_f(const Hand& H, int f, int k) const {
    return __builtin_bit_cast(float, hand_i(H, f, k));
  }
  // pass k's row task (make_task's values); word: its kHWord
  __device__ __forceinline__ RowTask hand_task(const VsgArgs& A, const Hand& H, int k, uint32_t word) const {
    RowTask t;
    t.p = hand_i(H, kHP, k);
    t.ch = hand_i(H, kHCh, k);
    t.pivot = hand_i(H, kHPivot, k);
    t.row0 = 0;
    const float* base = A.win + (int64_t)t.p * A.pass_stride;
    t.piv = base + (int64_t)t.pivot * A.ch_stride;
    t.rcv = base + (int64_t)t.ch * A.ch_stride;
    t.a_f = hand_i(H, kHAf, k);
    t.a_o = hand_i(H, kHAo, k);
    t.nwin_f = (int)(word & (kDeckNwin - 1));
    t.nwin_o = (int)((word >> kDeckNwBits) & (kDeckNwin - 1));
    return t;
  }
  __device__ __forceinline__ TabJobs deck_jobs(const RowTask& t, uint32_t word) const {
    return tab_jobs(t, (word & kDeckFarF) != 0, (word & kDeckFarO) != 0);
  }

  // ---- direct_task: a row task whose passes have only a table-served forward side ----
  // (no row norm; every pass's other side empty, its forward slices in the table, the same sub-window count
  // W and shared/far-window kind on every pass, finite factors).  The passes' receivers are then packed two
  // per transform ACROSS passes -- ceil(W n / 2) transforms for n passes instead of n ceil(W / 2) -- and each
  // pass's weight w_p = weight / W * scale is applied per half:  U = sum_p w_p sum_q P_pq conj(R_pq).
  // RAMP (exact engines): Gh += (-1)^lane ramp(U), the forward epilogue of stackf_tasks (ok = false: no
  // other side) summed over the passes; otherwise (padded engines) Gh += U, the forward side's accumulated
  // spectrum, and *shared = the passes' common lag convention.  On the configs[2] geometry these are the
  // rows below the pivot (3 receivers per pass).  Returns false (nothing done) when the task does not qualify.
  template <bool RAMP>
  __device__ bool direct_task(const VsgArgs& A, const Deck& D, float2 (&Gh)[kNH], bool* shared = nullptr) {
    constexpr int NH_ = kNH, BINS = E::kTabBins;
    const int n = D.n;
    if (n <= 1) return false;
    // lane k < n: pass order[b + k], from the task deck
    const bool act = lane < n;
    const int p = D.p, ch = D.ch, a = D.a_f;
    const int nwf = (int)(D.word & (kDeckNwin - 1)), nwo = (int)((D.word >> kDeckNwBits) & (kDeckNwin - 1));
    const bool shf = ch <= D.pivot;
    const int W = uni(nwf);
    const bool shf0 = uni(shf ? 1 : 0) != 0;
    const bool mf = shf || (D.word & kDeckFarF) != 0;
    // the epilogue's forward factor: ff = 1 / nwin_f, times the scale (side_scale), times the class weight
    float wgt = 0.f;
    if (W > 0) {
      float ff = 1.0f / (float)W;
      ff *= D.sf;
      wgt = D.wp * ff;
    }
    const bool good = !act || ((D.word & kDeckUsable) != 0 && nwo == 0 && nwf == W && shf == shf0 && mf && isfinite(wgt));
    if (__ballot(!good) != 0) return false;
    if (shared) *shared = shf0;
    if (W == 0) return true;  // no sub-windows on any pass: the row adds nothing
    // per-pass sources in lane k: receiver slice and table slice of sub-window 0, factor
    const uint64_t rp = reinterpret_cast<uint64_t>(A.win + (int64_t)p * A.pass_stride + (int64_t)ch * A.ch_stride + a);
    const uint64_t pp = reinterpret_cast<uint64_t>(tab_slice<BINS>(tab, p, shf ? 0 : 2, 0));
    // (the slices' non-zero flags ride in the low bits of the 8-byte aligned table pointer: no register of their own)
    static_assert(kTabSub <= 3, "flag bits in the low bits of a float2 pointer");
    const uint32_t rlo = (uint32_t)rp, rhi = (uint32_t)(rp >> 32), phi = (uint32_t)(pp >> 32);
    const uint32_t plo = (uint32_t)pp | ((D.word >> kDeckFlag0) & ((1u << kTabSub) - 1));
    const uint32_t wv = __builtin_bit_cast(uint32_t, wgt);
    // halves in order: pass k, sub-window s (cursor of the next half to hand out)
    int hk = 0, hs = 0;
    auto take = [&](const float*& r, const float2*& P, float& wt, bool& nz) {
      const int k = hk;
      r = reinterpret_cast<const float*>(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)rhi, k) << 32) |
                                         (uint32_t)__builtin_amdgcn_readlane((int)rlo, k)) + hs * A.hop;
      const uint32_t pl = (uint32_t)__builtin_amdgcn_readlane((int)plo, k);
      nz = ((pl >> hs) & 1u) != 0;  // the pivot slice's non-zero flag
      P = reinterpret_cast<const float2*>(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)phi, k) << 32) |
                                          (pl & ~7u)) + hs * BINS;
      wt = __builtin_bit_cast(float, __builtin_amdgcn_readlane((int)wv, k));
      if (++hs == W) {
        hs = 0;
        ++hk;
      }
    };
    const int M = W * n, nj = (M + 1) >> 1;
    float2 U[NH_];
#pragma unroll
    for (int j = 0; j < NH_; ++j) U[j] = make_float2(0.f, 0.f);
    const float *ra, *rb;
    const float2 *Pa, *Pb;
    float wa, wb = 0.f;
    bool fa, fb = false;
    take(ra, Pa, wa, fa);
    bool hb = hk < n;
    if (hb) take(rb, Pb, wb, fb);
    else {
      rb = ra;
      Pb = Pa;
    }
    float2 z[kNJ];
    self().load_ri(ra, rb, z);
    for (int jb = 0; jb < nj; ++jb) {
      uint32_t bp = 0, br = 0;
#pragma unroll
      for (int j = 0; j < kNJ; ++j) {
        bp = maxbits(bp, z[j].x);
        br = maxbits(br, z[j].y);
      }
      // a receiver slice or its pivot slice identically zero: exactly zero in the reference
      const bool la = (__ballot(bp != 0) != 0) && fa;
      const bool lb = hb && (__ballot(br != 0) != 0) && fb;
      const bool live = la || lb;
      if (live) self().stage1(z);
      else check_untransformed(z, __builtin_amdgcn_readlane(p, (2 * jb) / W),
                               hb ? __builtin_amdgcn_readlane(p, (2 * jb + 1) / W) : __builtin_amdgcn_readlane(p, (2 * jb) / W));
      const float2 *Pa_c = Pa, *Pb_c = Pb;
      const float wa_c = wa, wb_c = wb;
      if (jb + 1 < nj) {  // the next pair's samples, loaded under this transform
        take(ra, Pa, wa, fa);
        hb = hk < n;
        if (hb) take(rb, Pb, wb, fb);
        else {
          rb = ra;
          Pb = Pa;
        }
        self().load_ri(ra, rb, z);
      }
      if (!live) continue;
      float2 pa[NH_], pb[NH_];
#pragma unroll
      for (int j = 0; j < NH_; ++j) {
        const int f = max(E::bin(lane, j), 0);
        pa[j] = Pa_c[f];
        pb[j] = Pb_c[f];
      }
      self().finish_with([&](int j, float2 za, float2 zc) {
        // z = R_a + i R_b: R_a = (Z[f] + conj Z[-f]) / 2, R_b = (Z[f] - conj Z[-f]) / 2i; w P conj(R)
        if (la) {
          const float2 r = make_float2(za.x + zc.x, za.y - zc.y);  // 2 R_a (the table holds P / 2)
          U[j].x += wa_c * (pa[j].x * r.x + pa[j].y * r.y);
          U[j].y += wa_c * (pa[j].y * r.x - pa[j].x * r.y);
        }
        if (lb) {
          const float2 r = make_float2(za.y + zc.y, zc.x - za.x);  // 2 R_b
          U[j].x += wb_c * (pb[j].x * r.x + pb[j].y * r.y);
          U[j].y += wb_c * (pb[j].y * r.x - pb[j].x * r.y);
        }
      });
    }
    if (vflag) {  // a non-finite sample of some pass reached U: each of the task's passes is rescanned whole
      bool nf = false;
#pragma unroll
      for (int j = 0; j < NH_; ++j) nf |= !isfinite(U[j].x) || !isfinite(U[j].y);
      if (__ballot(nf) != 0 && act) atomicOr(vflag + p, kSuspect);
    }
    if constexpr (RAMP) {
      // Gh = (-1)^lane (conj on the shared window) U conj(tw[f])
      const int ln = opaque(lane);
      const float sg = (ln & 1) ? -1.f : 1.f;
#pragma unroll
      for (int j = 0; j < NH_; ++j) {
        const int f = E::bin(ln, j);
        if (f >= 0) {
          const float2 t = tw[f];
          const float2 x = cmul(shf0 ? make_float2(U[j].x, -U[j].y) : U[j], make_float2(t.x, -t.y));
          Gh[j].x += sg * x.x;
          Gh[j].y += sg * x.y;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NH_; ++j) {
        Gh[j].x += U[j].x;
        Gh[j].y += U[j].y;
      }
    }
    return true;
  }
};

// ------------------------------------------------------------------------------------------------
// EngF500: N = w = 500 Stockham (10 x 10 x 5) with the first and last stages fused into registers.
//   stage 1 (radix 10, span 1) reads its inputs straight from the prefetched sub-window samples (lane i < 50
//     holds samples i + 50 t, t < 10, of both slices) -- no LDS store of the raw window; one Good-Thomas 2 x 5
//     butterfly per lane, its outputs X[10 i .. 10 i + 9] stored as five 16-byte pieces (buffer B);
//   stage 2 (radix 10, span 10: 50 butterflies, one round) goes through LDS, two twiddle reads per butterfly
//     (w, w^5), into buffer A padded by kPad entries after every 100, which makes its 8-byte stores conflict free
//     (unpadded, the lanes of a 16-lane store group that straddle i / 10 land 800 B apart: 25 of 32 banks shared);
//   stage 3 (radix 5, span 100) runs butterflies k and 100 - k in the same lane (l <= 50), so the
//     lane holds X[k + 100 q] and its Hermitian partners X[N - f] and forms the cross spectra of its
//     five bins in registers -- no LDS write of the spectrum and no partner reads.
// Per forward transform: 2 LDS round trips and 3 wave barriers, 5 ds_write_b128 + 10 ds_write_b64, 10 + 2 LDS reads
// in the middle stage, one round of 64 lanes per stage (4 x 5 x 5 x 5, the previous plan: 3 round trips, 4
// barriers, 4 + 20 stores, 20 + 4 reads, 2 / 2 + 2 rounds; DESIGN.md has both measured).
// The padded buffer A is 4 kPad entries longer than the 500 of buffer B behind it and overlaps B's first entries:
// the middle stage has read all of B before its first store, and B is rewritten only by the next stage 1.
// Half-spectrum slots per lane l: j < 3 -> f = l + 100 j (l <= 50); j = 3, 4 -> f = 100 - l + 100 (j - 3)
// (1 <= l <= 49): each of the 251 bins f <= 250 exactly once.
struct EngF500 : FusedOps<EngF500, 10, 5> {
  static constexpr int NFFT = 500;
  static constexpr int NJ = 8;   // lags per lane in the epilogues (dvh_vsg.hip)
  static constexpr int kNZ = 10;  // sample registers per lane: samples i + 50 t
  static constexpr int NH = 5;
  static constexpr int kWaves = 4;
  static constexpr bool kExact = true;
  static constexpr bool kFused = true;
  static constexpr bool kDeckLoop = true;
  static constexpr int kOcc = 4;       // fits 4 waves / SIMD (the LDS Stockham engines are register-limited to 3)
  static constexpr int kOccStack = 4;  // as the exact Stockham engines up to N = 500
  static constexpr int kTabBins = 256;  // bins f <= 250; [255].x: the slice's non-zero flag
  static constexpr size_t kBlockBytes = sizeof(float2) * NFFT;     // twiddle table
  static constexpr size_t kWaveBytes = sizeof(float2) * 2 * NFFT;  // ping-pong buffers
  static constexpr int kBufA = NFFT;                               // bufB = bufA + kBufA
  static constexpr int kPad = 6;  // 2 (100 + kPad) = 20 mod 32 dwords: the 20-dword runs of consecutive i / 10 abut

  __device__ EngF500(char* lds, int wave, int lane_) : FusedOps<EngF500, kNZ, 5>(lds, wave, lane_, NFFT) {}
  static __device__ void block_init(char* lds) { init_twiddles<NFFT>(reinterpret_cast<float2*>(lds)); }

  static __device__ __forceinline__ int bin(int l, int j) {
    if (j < 3) return l <= 50 ? l + 100 * j : -1;
    return (l >= 1 && l <= 49) ? 100 - l + 100 * (j - 3) : -1;
  }

  // stage-1 operands z[t] = (re, im)[i + 50 t], t < 10, i = min(lane, 49), of the slices starting at re / im.
  // Branch-free: lanes past the 50 stage-1 butterflies load lane 49's samples again, which stage1() does not
  // store and which leave the non-zero tests unchanged; with im == nullptr the receiver is loaded into both
  // halves (the second half's result is discarded).
  __device__ __forceinline__ void load_ri(const float* re, const float* im, float2 (&z)[kNZ]) const {
    const float* ip = im ? im : re;
    const int i = min(lane, 49);
#pragma unroll
    for (int t = 0; t < kNZ; ++t) {
      const int n = i + 50 * t;
      z[t] = make_float2(re[n], ip[n]);
    }
  }

  __device__ __forceinline__ void stage1(const float2 (&z)[kNZ]) const {
    const int i = opaque(lane);
    if (i < 50) {
      float2 a[10];
#pragma unroll
      for (int t = 0; t < 10; ++t) a[t] = z[t];
      Dft<10>::run(a);
      // X[10 i .. 10 i + 9] as five 16-byte stores: the 80-byte lane stride tiles the 32 banks within each
      // 8-lane store group (20 i mod 32 = 0, 20, 8, 28, 16, 4, 24, 12), no swizzle needed
      float4* d = reinterpret_cast<float4*>(bufB + 10 * i);
#pragma unroll
      for (int q = 0; q < 10; q += 2) d[q >> 1] = make_float4(a[q].x, a[q].y, a[q + 1].x, a[q + 1].y);
    }
  }

  // stages 2-3 of the transform whose stage-1 output is in bufB; for every half-spectrum slot j of
  // the lane (compile-time j, valid slots only), acc(j, Z[f], Z[N - f]) with f = bin(lane, j)
  template <class F>
  __device__ __forceinline__ void finish_with(F&& acc) const {
    wave_sync();
    stockham_stage_any<NFFT, 10, 10, 0, kPad>(bufB, bufA, tw, opaque(lane));
    wave_sync();
    const int ln = opaque(lane);  // the stage's addresses formed per call, not held in registers between calls
    if (ln <= 50) {
      float2 XA[5], XB[5];
      const bool pair = ln >= 1 && ln <= 49;
      last_bfly_from(bufA, ln, XA);
      if (pair) last_bfly_from(bufA, 100 - ln, XB);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        // partner X[N - f] of f = l + 100 j is X[(100 - l) + 100 (4 - j)]
        const float2 p0 = XA[(5 - j) % 5], p50 = XA[4 - j], pb = XB[4 - j];
        float2 pa;  // value selects (a select of array elements would become a scratch pointer)
        pa.x = ln == 0 ? p0.x : (ln == 50 ? p50.x : pb.x);
        pa.y = ln == 0 ? p0.y : (ln == 50 ? p50.y : pb.y);
        acc(j, XA[j], pa);
      }
      if (pair) {
#pragma unroll
        for (int q = 0; q < 2; ++q) acc(3 + q, XB[q], XA[4 - q]);
      }
    }
    wave_sync();
  }

  // radix-5 butterfly k of the last stage (span 100): X[k + 100 q], q < 5, from the padded buffer
  __device__ __forceinline__ void last_bfly_from(const float2* src, int k, float2 (&x)[5]) const {
#pragma unroll
    for (int t = 0; t < 5; ++t) x[t] = lds_ld(src, k + (100 + kPad) * t);
    const float2 w1 = tw[k];
    float2 wt = w1;
#pragma unroll
    for (int t = 1; t < 5; ++t) {
      x[t] = cmul(x[t], wt);
      if (t < 4) wt = cmul(wt, w1);
    }
    Dft<5>::run(x);
  }

  __device__ const float2* inverse(const float2 (&Cf)[NH], const float2 (&Co)[NH]) {
    // 10 x 10 x 5 as the forward transform: B -> A -> padded B -> A.  The padded buffer starts 4 kPad entries
    // before B, over the end of A: the middle stage has read all of A before its first store, and the last stage
    // writes those entries of A (X[476..499], its second round) after its first round has read the overlapped
    // inputs (padded entries < 24).
    float2* const bufP = bufB - 4 * kPad;
    store_conj_hermitian<EngF500>(bufB, Cf, Co, lane);
    wave_sync();
    stockham_stage_any<NFFT, 1, 10>(bufB, bufA, tw, opaque(lane));
    wave_sync();
    stockham_stage_any<NFFT, 10, 10, 0, kPad>(bufA, bufP, tw, opaque(lane));
    wave_sync();
    stockham_stage_any<NFFT, 100, 5, kPad, 0>(bufP, bufA, tw, opaque(lane));
    wave_sync();
    return bufA;
  }

  __device__ float2 twiddle(int m) const { return tw[m]; }

  __device__ float2 c(const float2* Y, int k, int w_) const { return corr_at<NFFT, !kExact>(Y, k, w_); }
};


// ------------------------------------------------------------------------------------------------
// EngP1024: zero-padded N = 1024 Stockham for the window lengths without an exact engine, w <= 512 (w = int(wlen /
// dt) = 499 at the reference's other operating point, dt = 0.004000000000001336): the linear correlation of the
// zero-padded sub-windows (N >= 2w - 1) is folded back to the circular one in c().  The transform is fused like
// EngF500's:
//   the first stage from the prefetched samples: a lane holds z[j] = x[lane + 64 j], j < 8 (only samples n < w <=
//     512 can be non-zero: half the registers of a 1 024-sample stage), and its butterflies drop the zero inputs;
//   the last stage (radix 4, span 256) runs butterflies k and 256 - k in one lane -- round A: (l, 256 - l) for l >= 1
//     and (0, 128) on lane 0, both self-partnered; round B: (64 + l, 192 - l) -- so each lane holds X[f] and X[N - f]
//     of its bins and forms their cross spectra in registers.
// Half-spectrum slots per lane l (each bin f <= 512 exactly once):
//   j = 0, 1: l, l + 256;  j = 2, 3: 256 - l, 512 - l (lane 0: 128, 384);  j = 4..7: 64 + l, 320 + l, 192 - l,
//   448 - l;  j = 8: 512 (lane 0 only).
// The transforms run as radix-16 stages: forward = radix 16 (span 1, from the registers, zero-padded half) -> LDS A ->
// radix 16 (span 16) -> LDS B -> the paired radix-4 last stage (span 256) in registers; inverse = radix 4 (span 1,
// from the registers) -> LDS B -> radix 16 (span 4) -> LDS A -> radix 16 (span 64) -> Y in LDS B.  Two LDS round trips
// per transform instead of four radix-4 ones, one wave synchronisation per stage boundary, and the twiddle products of
// two radix-4 stages merged into one radix-16 stage.  Buffer A is padded (the span-1 forward stage's 16 outputs per
// lane at n + n / 16, the span-4 inverse stage's at n + 4 (n / 64)), so the stores and reads of every stage are
// conflict free; buffer B is plain.  (An XOR-swizzled radix-4 layout cut the conflicts further but cost 25 % more VALU
// for no gain)
struct EngP1024 : FusedOps<EngP1024, 8, 9> {
  static constexpr int NFFT = 1024;
  static constexpr int NJ = 8;   // lags per lane in the epilogues (dvh_vsg.hip): w <= 512
  static constexpr int kNZ = 8;  // sample registers per lane: samples lane + 64 j < NFFT / 2
  static constexpr int NH = 9;
  static constexpr int kWaves = 4;
  static constexpr bool kExact = false;
  static constexpr bool kFused = true;
  // its stack kernels sit at the 256-register limit of 2 waves / SIMD: a hand in the pass loop spills (20 B)
  static constexpr bool kDeckLoop = false;
  static constexpr int kOcc = 3;  // register-limited to 3 waves / SIMD
  // the plain stack kernel holds two accumulated side spectra besides the sub-window's (4 x 9 complex per lane)
  // and would spill at 3 waves / SIMD
  static constexpr int kOccStack = 2;
  static constexpr int kTabBins = 520;  // bins f <= 512; [519].x: the slice's non-zero flag
  static constexpr int kBufA = NFFT + NFFT / 16;
  static constexpr size_t kWaveBytes = sizeof(float2) * (kBufA + NFFT);  // buffers A and B
  // Radix-16 stage twiddles, contiguous per stage after the main table: stage Ls holds w^k, w^4k, w^8k (w = e^(-2 pi
  // i Ls' / N), Ls' = N / (16 Ls)) for k < Ls at r16_tw(Ls) + {0, Ls, 2 Ls} + k, so that a stage's reads by lanes of
  // consecutive k are consecutive (read from the main table at stride 4 k, 16 k, 32 k they cost 1.6 bank-conflict
  // cycles per LDS instruction of the whole launch).
  static constexpr int kR16Tw = NFFT;
  static constexpr int kR16TwEntries = 3 * (16 + 4 + 64);
  static constexpr int r16_tw(int Ls) { return kR16Tw + (Ls == 16 ? 0 : (Ls == 4 ? 48 : 60)); }
  static constexpr size_t kBlockBytes = sizeof(float2) * (NFFT + kR16TwEntries);

  __device__ EngP1024(char* lds, int wave, int lane_) : FusedOps<EngP1024, kNZ, 9>(lds, wave, lane_, NFFT / 2) {}
  static __device__ void block_init(char* lds) {
    float2* t = reinterpret_cast<float2*>(lds);
    init_twiddles<NFFT>(t);
    for (int e = threadIdx.x; e < kR16TwEntries; e += blockDim.x) {
      const int Ls = e < 48 ? 16 : (e < 60 ? 4 : 64), o = e - (Ls == 16 ? 0 : (Ls == 4 ? 48 : 60));
      const int j = o / Ls, k = o % Ls, mult = j == 0 ? 1 : (j == 1 ? 4 : 8);
      const int m = mult * k * (NFFT / (16 * Ls));
      double sn, cs;
      sincospi(2.0 * (double)m / (double)NFFT, &sn, &cs);  // init_twiddles' formula: the same float values as tw[m]
      t[kR16Tw + e] = make_float2((float)cs, (float)(-sn));
    }
  }

  static __device__ __forceinline__ int bin(int l, int j) {
    switch (j) {
      case 0: return l;
      case 1: return l + 256;
      case 2: return l == 0 ? 128 : 256 - l;
      case 3: return l == 0 ? 384 : 512 - l;
      case 4: return 64 + l;
      case 5: return 320 + l;
      case 6: return 192 - l;
      case 7: return 448 - l;
      default: return l == 0 ? 512 : -1;
    }
  }

  // z[j] = (re, im)[lane + 64 j], j < 8, zero past the sub-window (n >= w); im == nullptr: the receiver in
  // both halves (the second half's result is discarded)
  __device__ __forceinline__ void load_ri(const float* re, const float* im, float2 (&z)[kNZ]) const {
    const float* ip = im ? im : re;
#pragma unroll
    for (int j = 0; j < kNZ; ++j) {
      const int n = lane + 64 * j;
      z[j] = n < w ? make_float2(re[n], ip[n]) : make_float2(0.f, 0.f);
    }
  }

  // the four outputs of radix-4 butterfly i of a span-1 stage (out[4 i + q]) as two 16-byte stores at a 32-byte
  // lane stride; lanes with i & 4 store their second pair first so that every 8-lane store group tiles the 32 banks
  static __device__ __forceinline__ void store4(float2* out, int i, float2 x0, float2 x1, float2 x2, float2 x3) {
    const bool sw = (i & 4) != 0;
    const int o = sw ? 2 : 0;
    float4* d = reinterpret_cast<float4*>(out + 4 * i);
    d[o >> 1] = sw ? make_float4(x2.x, x2.y, x3.x, x3.y) : make_float4(x0.x, x0.y, x1.x, x1.y);
    d[(2 - o) >> 1] = sw ? make_float4(x0.x, x0.y, x1.x, x1.y) : make_float4(x2.x, x2.y, x3.x, x3.y);
  }

  __device__ __forceinline__ void stage1(const float2 (&z)[kNZ]) const {
    // radix-16 butterfly i = lane of x[i + 64 t], t < 16: the prefetched z[t] for t < 8, zero above; outputs
    // out[16 i + q] at the padded index 17 i + q (16 lanes of a store group: 16 distinct banks)
    float2 a[16];
#pragma unroll
    for (int t = 0; t < kNZ; ++t) a[t] = z[t];
    dft16<true>(a);
    float2* o = bufA + 17 * lane;
#pragma unroll
    for (int q = 0; q < 16; ++q) o[q] = a[q];
  }

  // radix-16 Stockham stage (span Ls = 16, 4 or 64) of butterfly i = lane: inputs in[ia(i + 64 t)], twiddles
  // w^t with w = tw[k N / (16 Ls)] (k = i % Ls), outputs out[oa((i - k) 16 + k + Ls q)]
  template <int Ls, class IA, class OA>
  __device__ __forceinline__ void stage16(const float2* in, float2* out, IA ia, OA oa) const {
    const int i = lane, k = i % Ls;
    float2 a[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) a[t] = lds_ld(in, ia(i + 64 * t));
    const float2* st = tw + r16_tw(Ls);
    twiddle16(a, st[k], st[Ls + k], st[2 * Ls + k]);
    dft16<false>(a);
    const int base = (i - k) * 16 + k;
#pragma unroll
    for (int q = 0; q < 16; ++q) out[oa(base + Ls * q)] = a[q];
  }

  // radix-4 butterfly k of the last stage (span 256): X[k + 256 q], q < 4
  __device__ __forceinline__ void last_bfly_from(const float2* src, int k, float2 (&x)[4]) const {
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = lds_ld(src, k + 256 * t);
    const float2 w1 = tw[k];
    float2 wt = w1;
#pragma unroll
    for (int t = 1; t < 4; ++t) {
      x[t] = cmul(x[t], wt);
      if (t < 3) wt = cmul(wt, w1);
    }
    Dft<4>::run(x);
  }

  static __device__ __forceinline__ float2 sel(bool c, float2 a, float2 b) {
    return make_float2(c ? a.x : b.x, c ? a.y : b.y);  // value selects (no scratch pointer)
  }

  // stages 2-5 of the transform whose stage-1 output is in bufB; acc(j, Z[f], Z[N - f]) for every valid
  // half-spectrum slot j of the lane (compile-time j)
  template <class F>
  __device__ __forceinline__ void finish_with(F&& acc) const {
    wave_sync();
    stage16<16>(bufA, bufB, [](int n) { return n + (n >> 4); }, [](int n) { return n; });
    const float2* src = bufB;  // the span-256 stage's input
    wave_sync();
    const int ln = opaque(lane);  // the stage's addresses formed per call, not held in registers between calls
    const bool l0 = ln == 0;
    {
      float2 XA[4], XB[4];
      last_bfly_from(src, ln, XA);
      last_bfly_from(src, l0 ? 128 : 256 - ln, XB);
      acc(0, XA[0], sel(l0, XA[0], XB[3]));
      acc(1, XA[1], sel(l0, XA[3], XB[2]));
      acc(2, XB[0], sel(l0, XB[3], XA[3]));
      acc(3, XB[1], sel(l0, XB[2], XA[2]));
      if (l0) acc(8, XA[2], XA[2]);
    }
    {
      float2 XA[4], XB[4];
      last_bfly_from(src, 64 + ln, XA);
      last_bfly_from(src, 192 - ln, XB);
      acc(4, XA[0], XB[3]);
      acc(5, XA[1], XB[2]);
      acc(6, XB[0], XA[3]);
      acc(7, XB[1], XA[2]);
    }
    wave_sync();
  }

  // The inverse transform conj(FFT(conj(W))) of W = Cf + i Co (W[N - f] = conj Cf[f] + i conj Co[f]).  Its first
  // stage (span 1: butterfly i of x[i + 256 t], t < 4, no twiddles) runs from the registers: the inputs of each
  // butterfly are four of ONE lane's half-spectrum slots or their Hermitian partners -- lane l >= 1 holds those of
  // butterflies l, 64 + l, 192 - l and 256 - l, lane 0 those of 0, 64, 128 and 192 -- so the spectrum is never
  // stored and re-read; then stages 2-5 in the swizzled layout.  Returns Y (bufB), read through c().
  __device__ const float2* inverse(const float2 (&Cf)[NH], const float2 (&Co)[NH]) {
    const int ln = opaque(lane);
    const bool l0 = ln == 0;
    // x[f] = conj W[f] = A(j), x[N - f] = conj W[N - f] = B(j) for slot j's bin f
    auto A = [&](int j) { return make_float2(Cf[j].x - Co[j].y, -(Cf[j].y + Co[j].x)); };
    auto B = [&](int j) { return make_float2(Cf[j].x + Co[j].y, Cf[j].y - Co[j].x); };
    auto bfly = [&](int i, float2 a0, float2 a1, float2 a2, float2 a3) {
      float2 a[4] = {a0, a1, a2, a3};
      Dft<4>::run(a);
      store4(bufB, i, a[0], a[1], a[2], a[3]);
    };
    // lane 0: x[512] is bin 512 itself (slot 8), x[768] the partner of bin 256 (slot 1); lanes >= 1: partners of
    // 512 - l (slot 3) and 256 - l (slot 2)
    bfly(ln, A(0), A(1), l0 ? A(8) : B(3), l0 ? B(1) : B(2));
    bfly(64 + ln, A(4), A(5), B(7), B(6));
    // lanes >= 1: butterflies 192 - l and 256 - l; lane 0: 128 and 192 (value selects, no divergent branch)
    bfly(l0 ? 128 : 192 - ln, sel(l0, A(2), A(6)), sel(l0, A(3), A(7)), sel(l0, B(3), B(5)), sel(l0, B(2), B(4)));
    bfly(l0 ? 192 : 256 - ln, sel(l0, A(6), A(2)), sel(l0, A(7), A(3)), sel(l0, B(5), B(1)), sel(l0, B(4), B(0)));
    wave_sync();
    stage16<4>(bufB, bufA, [](int n) { return n; }, [](int n) { return n + 4 * (n >> 6); });
    wave_sync();
    stage16<64>(bufA, bufB, [](int n) { return n + 4 * (n >> 6); }, [](int n) { return n; });
    wave_sync();
    return bufB;
  }

  __device__ float2 twiddle(int m) const { return tw[m]; }

  __device__ float2 c(const float2* Y, int k, int w_) const { return corr_at<NFFT, !kExact>(Y, k, w_); }
};

}  // namespace dvh
