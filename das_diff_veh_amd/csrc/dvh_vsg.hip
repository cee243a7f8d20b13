// Virtual-shot-gather cross-correlation + class stacking on MI355X (gfx950).
//
// Replaces, for a whole batch of vehicle passes at once:
//   XCORR_vshot                      modules/utils.py:289-314
//   XCORR_two_traces / repeat1d      modules/utils.py:250-270
//   xcorr_two_traces_based_on_traj   apis/virtual_shot_gather.py:14-43
//   post_processing_XCF              apis/virtual_shot_gather.py:129-142
//   construct_shot_gather[_other_side] + the two-sided average   apis/virtual_shot_gather.py:145-192
//   sum(images) / len(images)        apis/imaging_classes.py:106-107 (VirtualShotGather.__add__/__truediv__)
//
// Work unit: one (pass, gather row).  One wave64 computes BOTH sides of the row:
//   for each side, for each of the nwin sub-windows of its time slice, z = pivot + i*receiver is
//   transformed by one complex FFT (LDS Stockham), the cross spectrum P*conj(R) is extracted from
//   Z[f], conj(Z[-f]) and accumulated in registers; then ONE inverse FFT of Cf + i*Co yields both
//   sides' correlations (real and imaginary parts).  The epilogue applies each row type's lag
//   permutation (roll(w//2), time flip on the forward side), the per-pass amplitude normalisation
//   (1 / max of the pivot autocorrelation, from vsg_scales_kernel), the optional row L2 norm, and
//   the two-sided average rule (rows whose other side is finite and non-zero).
// Lag conventions, with c[k] = sum_n p[(n+k) % w] r[n] and h = w // 2:
//   forward, channel <= pivot (shared pivot window):   F[j] = c[(w-1-j-h) mod w]
//   forward, channel >  pivot (trajectory window):     F[j] = c[(j+h+1) mod w]
//   other,   channel >= pivot (shared, reverse=True):  O[j] = c[(h-1-j) mod w]
//   other,   channel <  pivot (trajectory window):     O[j] = c[(j-h) mod w]
//
// Windows are fp32, channel-major: sample (pass p, channel c, time t) at
//   win[p * pass_stride + c * ch_stride + t].
// seg_tab[((p * R + i) * 2 + side) * 2 + {0,1}] = {slice start, slice length} for gather row i
// (channel row0[p] + i) on side 0 = forward, 1 = other; pass_tab[p * 2 + {0,1}] = {row0, pivot}.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <algorithm>

#include "vsg_engines.h"
#include "vsg_scan.h"
#include "dvh_common.h"
#include "dvh.h"

namespace dvh {

constexpr int kBlock = 512;  // sumsq kernel

// Per-kernel engine setup of the fused-stage engines (E::kFused: they take a per-pass pivot-slice spectra table in
// the stack kernels and pack single-sided tasks across passes): the sub-window length (the padded engines mask
// their loads with it) and the pivot-slice table (stack kernels; nullptr elsewhere).
template <class E>
__device__ __forceinline__ void bind_engine(E& e, const VsgArgs& A, const float2* tab) {
  if constexpr (E::kFused) {
    e.w = A.w;
    e.tab = tab;
  }
}

// The per-task state of a stack wave's pass loop.  Fused engines: the task deck (FusedOps::Deck, consumed by
// direct_task) and the hand of passes the loop holds (FusedOps::Hand; n = 0: none, the tables are read pass by
// pass).
struct NoDeck {
  int n = 0;
};
template <class E, bool FUSED = E::kFused>
struct PassLoop {
  using Deck = NoDeck;
  using Hand = NoDeck;
};
template <class E>
struct PassLoop<E, true> {
  using Deck = typename E::Deck;
  using Hand = typename E::Hand;
};

template <class E>
__device__ __forceinline__ typename PassLoop<E>::Deck engine_deal(E& eng, const VsgArgs& A, const float* scales,
                                                                   const int32_t* order, const float* weight, int b,
                                                                   int e, int i) {
  if constexpr (E::kFused) return eng.deal(A, scales, order, weight, b, e, i);
  else return NoDeck{};
}
template <class E>
__device__ __forceinline__ typename PassLoop<E>::Hand engine_hand(E& eng, const typename PassLoop<E>::Deck& D, int b) {
  if constexpr (E::kFused) {
    if constexpr (E::kDeckLoop) return eng.hand(D, b);
    else return typename E::Hand{};
  } else {
    return NoDeck{};
  }
}

// Pass order[q] of a task of row i whose passes end at e: its row task, factors and cross spectra.  With a hand
// everything comes from it by readlane (a new hand is dealt when q runs past it).  Without one (other engines,
// tasks of more than 64 passes, an engine without kDeckLoop) the tables are read here.
template <class E>
__device__ __forceinline__ void engine_pass(E& eng, const VsgArgs& A, const float* __restrict__ scales,
                                            const int32_t* __restrict__ order, const float* __restrict__ weight,
                                            typename PassLoop<E>::Hand& H, int e, int q, int i, RowTask& task,
                                            float& sf, float& so, float& wp, float2 (&Cf)[E::NH],
                                            float2 (&Co)[E::NH]) {
  if constexpr (E::kFused) {
    if (H.n && q >= H.first + H.n) H = eng.hand(eng.deal(A, scales, order, weight, q, min(e, q + E::kHand), i), q);
    if (H.n) {
      const int k = uni(q - H.first);
      const uint32_t word = (uint32_t)eng.hand_i(H, E::kHWord, k);
      task = eng.hand_task(A, H, k, word);
      if (word & E::kDeckUsable) {
        eng.spectra_tab(task, eng.deck_jobs(task, word), word >> E::kDeckFlag0, A.hop, Cf, Co);
      } else {
        eng.spectra(task, A.w, A.hop, Cf, Co);
      }
      sf = eng.hand_f(H, E::kHSf, k);
      so = eng.hand_f(H, E::kHSo, k);
      wp = eng.hand_f(H, E::kHWp, k);
      return;
    }
  }
  const int p = sld(order + q);
  task = make_task(A, p, i);
  bool tabbed = false;
  if constexpr (E::kFused) {
    if (eng.tab && eng.tab_usable(p, A.n_pass)) {
      const int32_t* head = tab_head<E::kTabBins>(eng.tab, A.n_pass) + (int64_t)p * kTabEnt * 2;
      const auto J = E::tab_jobs(task, E::far_match(task.a_f, task.nwin_f, sld(head + 4), sld(head + 5)),
                                 E::far_match(task.a_o, task.nwin_o, sld(head + 6), sld(head + 7)));
      eng.spectra_tab(task, J, eng.tab_flags(task, J), A.hop, Cf, Co);
      tabbed = true;
    }
  }
  if (!tabbed) eng.spectra(task, A.w, A.hop, Cf, Co);
  sf = sld(scales + 2 * p);
  so = sld(scales + 2 * p + 1);
  wp = sld(weight + p);
}

// A row task whose passes have only a table-served forward side, transformed across passes.  RAMP: the exact
// engines' output-spectrum form; otherwise the forward spectrum sum (*shared: its lag convention).
template <class E, bool RAMP>
__device__ __forceinline__ bool engine_direct(E& eng, const VsgArgs& A, const typename PassLoop<E>::Deck& D,
                                              float2 (&Gh)[E::NH], bool* shared = nullptr) {
  if constexpr (E::kFused) {
    return eng.tab && eng.template direct_task<RAMP>(A, D, Gh, shared);
  } else {
    return false;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// XCD-aware block order (blocks are dealt round robin over the 8 XCDs, each with its own L2):
// consecutive logical blocks -- the row tasks of one pass chunk, which all read that chunk's pivot
// channel -- run on the same XCD.  A bijection on [0, gridDim.x).
__device__ __forceinline__ int xcd_block() {
  const int G = gridDim.x, b = blockIdx.x;
  const int q = G / 8, r = G % 8, x = b % 8, k = b / 8;
  return x < r ? x * (q + 1) + k : r * (q + 1) + (x - r) * q + k;
}

// The row tasks of a stack launch as one wave takes them: a static stride (t0, t0 + stride, ...), or pulled
// from a global counter (pull_unit, vsg_scan.h).  (Eight per-XCD counters, each XCD draining its own eighth of the
// tasks before the others' leftovers, measured no faster on the padded engine: w = 499 synth10k launch 15.05 vs 14.99 ms, weights 1.80-1.83
// vs 1.81-1.83 ms.)
struct TaskSource {
  uint32_t* q = nullptr;  // nullptr: static stride
  int64_t stride = 1;
  __device__ int64_t first(int64_t t0, int lane) { return q ? pull_unit(q, lane) : t0; }
  __device__ int64_t next(int64_t t, int lane) { return q ? pull_unit(q, lane) : t + stride; }
};

template <class E>
__device__ __forceinline__ E make_engine(char* lds) {
  E::block_init(lds);
  __syncthreads();
  return E(lds, threadIdx.x >> 6, threadIdx.x & 63);
}

// The reference divides every window by ||data||_F first (preprocessing_window,
// apis/virtual_shot_gather.py:125): a window holding a NaN / inf, or all zero (0 / 0), turns the
// whole gather into NaN.  With win_sumsq = ||data||_F^2 given, such a pass gets NaN scales, which
// the gather / stack kernels carry into every computed row exactly as that division does.
__device__ __forceinline__ bool window_invalid(const double* __restrict__ sumsq, int p) {
  if (!sumsq) return false;
  const double s = sumsq[p];
  return !(s > 0.0) || !isfinite(s);
}

// Per-pass scale of each side: 1 / max(pivot autocorrelation row) after the optional row norm
// (post_processing_XCF with norm_amp=True); 1 / ||window||_F^2 when neither norm is requested.
template <class E>
__global__ __launch_bounds__(64 * E::kWaves, E::kOcc) void vsg_scales_kernel(VsgArgs A, const double* __restrict__ sumsq,
                                                           float* __restrict__ scales) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  E eng = make_engine<E>(lds);
  bind_engine(eng, A, nullptr);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const bool other = (A.flags & kFlagOtherSide) != 0;
  const bool norm = (A.flags & kFlagNorm) != 0;
  const bool norm_amp = (A.flags & kFlagNormAmp) != 0;
  constexpr int NJ = E::NJ;
  const int stride = gridDim.x * E::kWaves;
  for (int p = blockIdx.x * E::kWaves + wave; p < A.n_pass; p += stride) {
    if (!norm_amp || window_invalid(sumsq, p)) {
      if (lane == 0) {
        const float s = window_invalid(sumsq, p) ? NAN : (norm ? 1.0f : (float)(1.0 / sumsq[p]));
        scales[2 * p] = s;
        scales[2 * p + 1] = s;
      }
      continue;
    }
    const RowTask t = make_task(A, p, uni(A.pass_tab[2 * p + 1] - A.pass_tab[2 * p]));  // the pivot row
    const float2* Y = correlate(eng, t, A.w, A.hop);
    float mf = -INFINITY, mo = -INFINITY, sf = 0.f, so = 0.f;
    bool nanf = false, nano = false;
    // a side with nothing accumulated is exactly zero in the reference (the packed inverse FFT
    // would otherwise leak the other side's rounding into it)
    const float2 live = make_float2(eng.live_f ? 1.f : 0.f, eng.live_o ? 1.f : 0.f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int k = lane + 64 * j;
      if (k < A.w) {
        float2 c = eng.c(Y, k, A.w);
        c.x *= live.x;
        c.y *= live.y;
        nanf |= isnan(c.x);
        nano |= isnan(c.y);
        mf = fmaxf(mf, c.x);
        mo = fmaxf(mo, c.y);
        sf += c.x * c.x;
        so += c.y * c.y;
      }
    }
    wave_sync();
    mf = wave_max(mf);
    mo = wave_max(mo);
    const bool anynanf = __ballot(nanf) != 0, anynano = __ballot(nano) != 0;
    float amax_f, amax_o;
    if (norm) {
      sf = wave_sum(sf);
      so = wave_sum(so);
      amax_f = mf / sqrtf(sf);
      amax_o = mo / sqrtf(so);
    } else {
      amax_f = t.nwin_f > 0 ? mf / ((float)E::NFFT * (float)t.nwin_f) : 0.f;
      amax_o = t.nwin_o > 0 ? mo / ((float)E::NFFT * (float)t.nwin_o) : 0.f;
    }
    if (anynanf) amax_f = NAN;
    if (anynano) amax_o = NAN;
    if (lane == 0) {
      scales[2 * p] = 1.0f / amax_f;
      scales[2 * p + 1] = other ? 1.0f / amax_o : 0.f;
    }
  }
}

// Applies the per-pass scales to the row factors.  With neither norm the reference scales the DATA
// (data / ||data||, virtual_shot_gather.py:124), so a side without sub-windows stays exactly 0 even
// when the window is all zero or holds a NaN; otherwise the scale divides the finished row and
// 0 * (1 / amax) reproduces its 0 / amax.
__device__ __forceinline__ void side_scale(int flags, const RowTask& t, float sf, float so, float& ff, float& fo) {
  if (!(flags & (kFlagNorm | kFlagNormAmp))) {
    ff = t.nwin_f > 0 ? ff * sf : 0.f;
    fo = t.nwin_o > 0 ? fo * so : 0.f;
  } else {
    ff *= sf;
    fo *= so;
  }
}

// Time-domain epilogue of a row: lag permutation, per-pass scales, optional row norm, two-sided
// average -> G[m] for output lag j = lane + 64 m (post_processing_XCF + VirtualShotGather.__init__).

template <class E>
__device__ __forceinline__ void row_epilogue(const E& eng, const VsgArgs& A, const float2* Y, const RowTask& t,
                                             float sf, float so, int lane_, float (&G)[E::NJ]) {
  constexpr int NJ = E::NJ;
  const int lane = opaque(lane_);  // cold path (norms / NaN fallback): keep its index math local
  const bool other = (A.flags & kFlagOtherSide) != 0;
  const bool norm = (A.flags & kFlagNorm) != 0;
  const int w = A.w, h = w / 2;
  // a side with nothing accumulated is exactly zero in the reference (see vsg_scales_kernel)
  const float2 live = make_float2(eng.live_f ? 1.f : 0.f, eng.live_o ? 1.f : 0.f);
  float ff, fo;
  if (norm) {
    float s2f = 0.f, s2o = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int k = lane + 64 * j;
      if (k < w) {
        float2 c = eng.c(Y, k, w);
        c.x *= live.x;
        c.y *= live.y;
        s2f += c.x * c.x;
        s2o += c.y * c.y;
      }
    }
    ff = 1.0f / sqrtf(wave_sum(s2f));
    fo = 1.0f / sqrtf(wave_sum(s2o));
  } else {
    ff = t.nwin_f > 0 ? 1.0f / ((float)E::NFFT * (float)t.nwin_f) : 0.f;
    fo = t.nwin_o > 0 ? 1.0f / ((float)E::NFFT * (float)t.nwin_o) : 0.f;
  }
  side_scale(A.flags, t, sf, so, ff, fo);
  const bool fwd_shared = t.ch <= t.pivot;
  const bool oth_shared = t.ch >= t.pivot;
  float O[NJ];
  bool nan_o = false, nz_o = false;
#pragma unroll
  for (int m = 0; m < NJ; ++m) {
    const int j = lane + 64 * m;
    G[m] = 0.f;
    O[m] = 0.f;
    if (j < w) {
      const int kf = fwd_shared ? pmod(w - 1 - j - h, w) : pmod(j + h + 1, w);
      G[m] = (eng.c(Y, kf, w).x * live.x) * ff;
      if (other) {
        const int ko = oth_shared ? pmod(h - 1 - j, w) : pmod(j - h, w);
        O[m] = (eng.c(Y, ko, w).y * live.y) * fo;
        nan_o |= isnan(O[m]);
        nz_o |= (O[m] != 0.f);
      }
    }
  }
  wave_sync();
  if (other) {
    // ||other row|| > 0 in the reference: finite-or-inf, not NaN, and not identically zero
    const bool ok = (__ballot(nan_o) == 0) && (__ballot(nz_o) != 0);
    if (ok) {
#pragma unroll
      for (int m = 0; m < NJ; ++m) G[m] = (G[m] + O[m]) * 0.5f;
    }
  }
}

template <class E>
__device__ __forceinline__ void gather_row(E& eng, const VsgArgs& A, const float* __restrict__ scales, int p,
                                           const RowTask& t, int lane, float (&G)[E::NJ]) {
  const float2* Y = correlate(eng, t, A.w, A.hop);
  row_epilogue<E>(eng, A, Y, t, sld(scales + 2 * p), sld(scales + 2 * p + 1), lane, G);
}

template <class E>
__global__ __launch_bounds__(64 * E::kWaves, E::kOcc) void vsg_gather_kernel(VsgArgs A, const float* __restrict__ scales,
                                                           float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  E eng = make_engine<E>(lds);
  bind_engine(eng, A, nullptr);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int NJ = E::NJ;
  const int64_t n_task = (int64_t)A.n_pass * A.R;
  const int64_t stride = (int64_t)gridDim.x * E::kWaves;
  for (int64_t t = (int64_t)xcd_block() * E::kWaves + wave; t < n_task; t += stride) {
    const int p = uni((int)(t / A.R)), i = uni((int)(t % A.R));
    const RowTask task = make_task(A, p, i);
    float G[NJ];
    gather_row<E>(eng, A, scales, p, task, lane, G);
    float* o = out + t * A.w;
#pragma unroll
    for (int m = 0; m < NJ; ++m) {
      const int j = lane + 64 * m;
      if (j < A.w) o[j] = G[m];
    }
  }
}

// Stack mode, exact transforms (N == w): every pass's contribution is accumulated directly as the
// spectrum of its output row, Ghat[m] += w_p (alpha f_f Phase_F(Cf) + beta f_o Phase_O(Co)), where
// each lag convention of the reference is a conjugation and a phase ramp:
//   c[(a - j) mod w]  ->  W^(a m) conj(C[m]),      c[(j + b) mod w]  ->  W^(-b m) C[m]
// (alpha, beta) = (1/2, 1/2) when the other side is finite and non-zero, else (1, 0).  One inverse
// transform per (chunk, row) replaces the per-pass inverse transform and epilogue.  Passes with a
// non-finite scale or NaN data go through the exact time-domain path (row_epilogue) instead.
// The row tasks t0, t0 + stride, ... < n_chunk * R of one wave (task = (chunk, row)).
template <class E>
__device__ __forceinline__ void stackf_tasks(E& eng, const VsgArgs& A, const float* __restrict__ scales,
                                             const int32_t* __restrict__ order, const int32_t* __restrict__ chunk_tab,
                                             int32_t n_chunk, const float* __restrict__ weight,
                                             float* __restrict__ stack, int64_t t0, TaskSource src) {
  const int lane_ = threadIdx.x & 63;
  constexpr int NJ = E::NJ;
  constexpr int NH = E::NH;
  constexpr int N = E::NFFT;
  const bool other = (A.flags & kFlagOtherSide) != 0;
  const bool norm = (A.flags & kFlagNorm) != 0;
  const int h = N / 2;
  const int64_t n_task = (int64_t)n_chunk * A.R;
  // tasks from src (static stride or pulled); the next index fetched at the top of the task so that `continue`
  // moves on
  const int lane_t = threadIdx.x & 63;
  int64_t tn = src.first(t0, lane_t);
  for (int64_t t = tn; t < n_task; t = tn) {
    tn = src.next(t, lane_t);
    const int c = uni((int)(t / A.R)), i = uni((int)(t % A.R));
    const int b = sld(chunk_tab + 3 * c), e = sld(chunk_tab + 3 * c + 1), slot = sld(chunk_tab + 3 * c + 2);
    float* o = stack + ((int64_t)slot * A.R + i) * A.w;
    float2 Gh[NH];
#pragma unroll
    for (int m = 0; m < NH; ++m) Gh[m] = make_float2(0.f, 0.f);
    const auto D = engine_deal(eng, A, scales, order, weight, b, e, i);
    const bool direct = !norm && engine_direct<E, true>(eng, A, D, Gh);
    typename PassLoop<E>::Hand H;  // (the deck is dead once direct_task has run)
    if (!direct) H = engine_hand(eng, D, b);
    for (int q = direct ? e : b; q < e; ++q) {
      RowTask task;
      float2 Cf[NH], Co[NH];
      float sf, so, wp;
      engine_pass(eng, A, scales, order, weight, H, e, q, i, task, sf, so, wp, Cf, Co);
      const int p = task.p;
      // per-pass bin / twiddle-index math recomputed here (hoisted, it only spills)
      const int lane = opaque(lane_);
      // sums of |.| over the half spectra: NaN iff some bin is NaN (sums of non-negative values never
      // turn infinities into NaN); the other side is non-zero iff its sum is
      float af = 0.f, ao = 0.f;
#pragma unroll
      for (int m = 0; m < NH; ++m) {
        if (E::bin(lane, m) >= 0) {
          af += fabsf(Cf[m].x) + fabsf(Cf[m].y);
          ao += fabsf(Co[m].x) + fabsf(Co[m].y);
        }
      }
      const bool bad = __ballot(isnan(af + ao)) != 0;
      const bool nzo = other && (__ballot(ao != 0.f) != 0);
      if constexpr (E::kFused) {  // covered-span scan: a non-finite sample among this pass's loaded slices
        if (eng.vflag && __ballot(!isfinite(af + ao)) != 0 && lane_ == 0) atomicMax(eng.vflag + p, kInfBits);
      }
      float ff, fo;
      if (norm) {  // ||c||^2 = sum_m |C[m]|^2 / N (Parseval over all N bins: interior bins count twice)
        float s2f = 0.f, s2o = 0.f;
#pragma unroll
        for (int m = 0; m < NH; ++m) {
          const int f = E::bin(lane, m);
          if (f >= 0) {
            const float wgt = (f == 0 || f == h) ? 1.f : 2.f;
            s2f += wgt * (Cf[m].x * Cf[m].x + Cf[m].y * Cf[m].y);
            s2o += wgt * (Co[m].x * Co[m].x + Co[m].y * Co[m].y);
          }
        }
        ff = sqrtf((float)N) / sqrtf(wave_sum(s2f));
        fo = sqrtf((float)N) / sqrtf(wave_sum(s2o));
      } else {
        ff = task.nwin_f > 0 ? 1.0f / (float)task.nwin_f : 0.f;
        fo = task.nwin_o > 0 ? 1.0f / (float)task.nwin_o : 0.f;
      }
      side_scale(A.flags, task, sf, so, ff, fo);
      if (bad || !isfinite(ff) || (nzo && !isfinite(fo))) {
        // exact time-domain path (NaN / inf semantics of the reference), added straight to the stack
        const float2* Y = eng.inverse(Cf, Co);
        float G[NJ];
        row_epilogue<E>(eng, A, Y, task, sf, so, lane, G);
#pragma unroll
        for (int m = 0; m < NJ; ++m) {
          const int j = lane + 64 * m;
          if (j < A.w) atomicAdd(o + j, G[m] * wp);
        }
        wave_sync();
      } else {
        // other row finite and not identically zero (row_epilogue's test)
        const bool ok = nzo && fo != 0.f;
        // lag shifts as phase ramps W^(s f): forward s = h - 1 on both row types (conj on the shared
        // window), other side s = h - 1 (shared, conj) or h (trajectory window).  W^(h f) = (-1)^f and
        // every engine's bins have the lane's parity, so W^((h-1) f) = (-1)^lane conj(tw[f]).
        const float sg = (lane & 1) ? -1.f : 1.f;
        const float cf = sg * wp * (ok ? 0.5f : 1.f) * ff;
        const float co = ok ? sg * wp * 0.5f * fo : 0.f;
        const bool fwd_shared = task.ch <= task.pivot;
        const bool oth_shared = task.ch >= task.pivot;
#pragma unroll
        for (int m = 0; m < NH; ++m) {
          const int f = E::bin(lane, m);
          if (f >= 0) {
            const float2 t = eng.twiddle(f);
            const float2 tc = make_float2(t.x, -t.y);
            float2 x = fwd_shared ? make_float2(Cf[m].x, -Cf[m].y) : Cf[m];
            x = cmul(x, tc);
            Gh[m].x += cf * x.x;
            Gh[m].y += cf * x.y;
            if (ok) {
              float2 y = Co[m];
              if (oth_shared) y = cmul(make_float2(y.x, -y.y), tc);
              Gh[m].x += co * y.x;
              Gh[m].y += co * y.y;
            }
          }
        }
      }
    }
    float2 Z[NH];
#pragma unroll
    for (int m = 0; m < NH; ++m) Z[m] = make_float2(0.f, 0.f);
    const float2* Y = eng.inverse(Gh, Z);
    const float inv_n = 1.0f / (float)N;
    const int lane = opaque(lane_);  // per-task addresses formed here, not held across the task loop
#pragma unroll
    for (int m = 0; m < NJ; ++m) {
      const int j = lane + 64 * m;
      if (j < A.w) atomicAdd(o + j, eng.c(Y, j, A.w).x * inv_n);
    }
    wave_sync();
  }
}

// Stack mode, zero-padded transforms (N >= 2w - 1, w without an exact engine, e.g. w = 499 on real time axes):
// the circular correlation is the fold c[k] = lin[k] + lin[k - w] of the linear one, so it cannot be phase-
// ramped in the N-point domain; but folding, the lag permutations and the class sum are linear.  The passes of
// a (chunk, row) task whose row has the same lag conventions as the chunk's first pass (every pass but those
// whose pivot row lies on the other side of this row) accumulate their weighted side spectra in registers,
//   Af += w_p alpha_p f_f,p Cf_p,   Ao += w_p beta_p f_o,p Co_p,
// then ONE inverse transform of Af + i Ao per task yields both sides' summed, folded correlations, which the
// epilogue permutes with the chunk's conventions and adds to the stack.  Passes with a row norm (the row's
// norm needs its own folded correlation), NaN data, non-finite factors or other conventions take the exact
// per-pass time-domain path.
template <class E>
__device__ __forceinline__ void stackp_tasks(E& eng, const VsgArgs& A, const float* __restrict__ scales,
                                             const int32_t* __restrict__ order, const int32_t* __restrict__ chunk_tab,
                                             int32_t n_chunk, const float* __restrict__ weight,
                                             float* __restrict__ stack, int64_t t0, TaskSource src) {
  const int lane_ = threadIdx.x & 63;
  constexpr int NJ = E::NJ;
  constexpr int NH = E::NH;
  constexpr int N = E::NFFT;
  const bool other = (A.flags & kFlagOtherSide) != 0;
  const bool norm = (A.flags & kFlagNorm) != 0;
  const int w = A.w, h = w / 2;
  const int64_t n_task = (int64_t)n_chunk * A.R;
  // tasks from src (static stride or pulled); the next index fetched at the top of the task so that `continue`
  // moves on
  const int lane_t = threadIdx.x & 63;
  int64_t tn = src.first(t0, lane_t);
  for (int64_t t = tn; t < n_task; t = tn) {
    tn = src.next(t, lane_t);
    const int c = uni((int)(t / A.R)), i = uni((int)(t % A.R));
    const int b = sld(chunk_tab + 3 * c), e = sld(chunk_tab + 3 * c + 1), slot = sld(chunk_tab + 3 * c + 2);
    float* o = stack + ((int64_t)slot * A.R + i) * A.w;
    float2 Af[NH], Ao[NH];
#pragma unroll
    for (int m = 0; m < NH; ++m) Af[m] = Ao[m] = make_float2(0.f, 0.f);
    bool fs0 = false, os0 = false, any = false, anyo = false;
    const auto D = engine_deal(eng, A, scales, order, weight, b, e, i);
    if (b < e) {
      int ch0 = 0, pivot0 = 0;
      if constexpr (E::kFused) {
        if (D.n) {
          ch0 = __builtin_amdgcn_readfirstlane(D.ch);
          pivot0 = __builtin_amdgcn_readfirstlane(D.pivot);
        }
      }
      if (!D.n) {
        const int p0 = sld(order + b);
        ch0 = sld(A.pass_tab + 2 * p0) + i;
        pivot0 = sld(A.pass_tab + 2 * p0 + 1);
      }
      fs0 = ch0 <= pivot0;
      os0 = ch0 >= pivot0;
    }
    // single-sided tasks with table-served forward slices: receivers packed across passes (fused engines)
    bool dshared = fs0;
    const bool direct = !norm && engine_direct<E, false>(eng, A, D, Af, &dshared);
    if (direct) {
      fs0 = dshared;
      any = true;
    }
    typename PassLoop<E>::Hand H;  // (the deck is dead once direct_task has run)
    if (!direct) H = engine_hand(eng, D, b);
    for (int q = direct ? e : b; q < e; ++q) {
      RowTask task;
      float2 Cf[NH], Co[NH];
      float sf, so, wp;
      engine_pass(eng, A, scales, order, weight, H, e, q, i, task, sf, so, wp, Cf, Co);
      const int p = task.p;
      const int lane = opaque(lane_);
      float af = 0.f, ao = 0.f;
#pragma unroll
      for (int m = 0; m < NH; ++m) {
        if (E::bin(lane, m) >= 0) {
          af += fabsf(Cf[m].x) + fabsf(Cf[m].y);
          ao += fabsf(Co[m].x) + fabsf(Co[m].y);
        }
      }
      const bool bad = __ballot(isnan(af + ao)) != 0;
      const bool nzo = other && eng.live_o && (__ballot(ao != 0.f) != 0);
      if constexpr (E::kFused) {  // covered-span scan: a non-finite sample among this pass's loaded slices
        if (eng.vflag && __ballot(!isfinite(af + ao)) != 0 && lane_ == 0) atomicMax(eng.vflag + p, kInfBits);
      }
      float ff = task.nwin_f > 0 ? 1.0f / (float)task.nwin_f : 0.f;
      float fo = task.nwin_o > 0 ? 1.0f / (float)task.nwin_o : 0.f;
      side_scale(A.flags, task, sf, so, ff, fo);
      const bool same = (task.ch <= task.pivot) == fs0 && (task.ch >= task.pivot) == os0;
      if (norm || bad || !same || !isfinite(ff) || (nzo && !isfinite(fo))) {
        // exact per-pass time-domain path, added straight to the stack
        const float2* Y = eng.inverse(Cf, Co);
        float G[NJ];
        row_epilogue<E>(eng, A, Y, task, sf, so, lane, G);
#pragma unroll
        for (int m = 0; m < NJ; ++m) {
          const int j = lane + 64 * m;
          if (j < A.w) atomicAdd(o + j, G[m] * wp);
        }
        wave_sync();
        continue;
      }
      // other row finite and not identically zero (row_epilogue's test): the two-sided average
      const bool ok = nzo && fo != 0.f;
      const float cf = wp * (ok ? 0.5f : 1.f) * ff, co = ok ? wp * 0.5f * fo : 0.f;
#pragma unroll
      for (int m = 0; m < NH; ++m) {
        Af[m].x += cf * Cf[m].x;
        Af[m].y += cf * Cf[m].y;
        Ao[m].x += co * Co[m].x;
        Ao[m].y += co * Co[m].y;
      }
      any = true;
      anyo |= ok;
    }
    if (!any) continue;
    // N * (sum of folded forward correlations, sum of folded other-side correlations) at lag k: eng.c(Y, k, w)
    const float2* Y = eng.inverse(Af, Ao);
    const float inv_n = 1.0f / (float)N;
#pragma unroll
    for (int m = 0; m < NJ; ++m) {
      const int j = lane_ + 64 * m;
      if (j < w) {
        const int kf = fs0 ? pmod(w - 1 - j - h, w) : pmod(j + h + 1, w);
        float g = eng.c(Y, kf, w).x;
        if (other && anyo) {  // (an all-zero Ao's inverse is rounding noise, not the exact 0 the reference adds)
          const int ko = os0 ? pmod(h - 1 - j, w) : pmod(j - h, w);
          g += eng.c(Y, ko, w).y;
        }
        atomicAdd(o + j, g * inv_n);
      }
    }
    wave_sync();
  }
}

// The plain stack kernels: stackp for the padded engines, stackf for the exact ones (E::kExact).
template <class E>
__global__ __launch_bounds__(64 * E::kWaves, E::kOccStack) void vsg_stackp_kernel(
    VsgArgs A, const float* __restrict__ scales, const int32_t* __restrict__ order,
    const int32_t* __restrict__ chunk_tab, int32_t n_chunk, const float* __restrict__ weight,
    float* __restrict__ stack, const float2* __restrict__ ptab) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  E eng = make_engine<E>(lds);
  bind_engine(eng, A, ptab);
  const int wave = threadIdx.x >> 6;
  TaskSource src;
  src.stride = (int64_t)gridDim.x * E::kWaves;
  stackp_tasks<E>(eng, A, scales, order, chunk_tab, n_chunk, weight, stack, (int64_t)xcd_block() * E::kWaves + wave, src);
}

template <class E>
__global__ __launch_bounds__(64 * E::kWaves, E::kOccStack) void vsg_stackf_kernel(
    VsgArgs A, const float* __restrict__ scales, const int32_t* __restrict__ order,
    const int32_t* __restrict__ chunk_tab, int32_t n_chunk, const float* __restrict__ weight,
    float* __restrict__ stack, const float2* __restrict__ ptab) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  E eng = make_engine<E>(lds);
  bind_engine(eng, A, ptab);
  const int wave = threadIdx.x >> 6;
  TaskSource src;
  src.stride = (int64_t)gridDim.x * E::kWaves;
  stackf_tasks<E>(eng, A, scales, order, chunk_tab, n_chunk, weight, stack, (int64_t)xcd_block() * E::kWaves + wave, src);
}

// The pivot-slice spectra table of every pass (FusedOps::spectra_tab) for engine E: one wave per pass forms the
// entries' (start, nwin) from the pivot row and the first / last gather rows and transforms their slices
// pairwise with the engine's transform (zero-padded past w for the padded engines), writing P[f] / 2, f <= N / 2,
// and each slice's non-zero flag at bin kTabBins - 1.
template <class E>
__global__ __launch_bounds__(256) void vsg_pivot_table_kernel(VsgArgs A, float2* __restrict__ tab) {
  constexpr int N = E::NFFT, BINS = E::kTabBins;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float2* tw = reinterpret_cast<float2*>(lds);
  init_twiddles<N>(tw);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float2* bufA = reinterpret_cast<float2*>(lds + sizeof(float2) * N + (size_t)wave * sizeof(float2) * 2 * N);
  float2* bufB = bufA + N;
  int32_t* head = reinterpret_cast<int32_t*>(tab + (int64_t)A.n_pass * tab_pass_f2<BINS>());
  for (int p = blockIdx.x * 4 + wave; p < A.n_pass; p += gridDim.x * 4) {
    const int row0 = sld(A.pass_tab + 2 * p), pivot = sld(A.pass_tab + 2 * p + 1);
    const RowTask tp = make_task(A, p, pivot - row0), tl = make_task(A, p, A.R - 1), t0 = make_task(A, p, 0);
    int st0 = tp.a_f, st1 = tp.a_o, st2 = tl.a_f, st3 = t0.a_o;
    int nw0 = tp.nwin_f, nw1 = tp.nwin_o, nw2 = tl.ch > pivot ? tl.nwin_f : 0, nw3 = t0.ch < pivot ? t0.nwin_o : 0;
    // an entry holds kTabSub sub-windows: a pass with more (time_window_to_xcorr > 2 wlen) is marked unusable
    // (every head nwin = -1, nothing transformed) and its row tasks take the plain z = P + i R path
    static_assert(kTabEnt == 4, "entries: pivot forward / other side, far-row forward / other side");
    if (!(nw0 <= kTabSub && nw1 <= kTabSub && nw2 <= kTabSub && nw3 <= kTabSub)) nw0 = nw1 = nw2 = nw3 = -1;
    // entry values by selects among scalars (a run-time index into a stack array went to scratch)
    auto pick = [](int e, int a0, int a1, int a2, int a3) { return e == 0 ? a0 : e == 1 ? a1 : e == 2 ? a2 : a3; };
    if (lane < 2 * kTabEnt)
      head[(int64_t)p * 2 * kTabEnt + lane] = (lane & 1) ? pick(lane >> 1, nw0, nw1, nw2, nw3) : pick(lane >> 1, st0, st1, st2, st3);
    // the slices (e, q), q < kTabSub, two per transform; absent ones are zero.  The next pair's samples are loaded
    // before this pair's transform (one load latency per pass instead of one per transform)
    constexpr int NL = (N + 63) / 64;
    auto load_pair = [&](int s0, float (&v0)[NL], float (&v1)[NL], bool& h0, bool& h1) {
      const int e0 = s0 / kTabSub, q0 = s0 % kTabSub, e1 = (s0 + 1) / kTabSub, q1 = (s0 + 1) % kTabSub;
      h0 = q0 < pick(e0, nw0, nw1, nw2, nw3);
      h1 = q1 < pick(e1, nw0, nw1, nw2, nw3);
      const float* x0 = tp.piv + pick(e0, st0, st1, st2, st3) + q0 * A.hop;
      const float* x1 = tp.piv + pick(e1, st0, st1, st2, st3) + q1 * A.hop;
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        const int n = lane + 64 * k;
        const bool in = n < A.w;  // the padded engines' zeros past the sub-window (and n < N, as A.w <= N)
        v0[k] = (h0 && in) ? x0[n] : 0.f;
        v1[k] = (h1 && in) ? x1[n] : 0.f;
      }
    };
    float c0[NL], c1[NL];
    bool ch0, ch1;
    load_pair(0, c0, c1, ch0, ch1);
#pragma unroll 1
    for (int s0 = 0; s0 < kTabSub * kTabEnt; s0 += 2) {
      const int e0 = s0 / kTabSub, q0 = s0 % kTabSub, e1 = (s0 + 1) / kTabSub, q1 = (s0 + 1) % kTabSub;
      const bool h0 = ch0, h1 = ch1;
      uint32_t nz0 = 0, nz1 = 0;
      const float2* X = nullptr;
      if (h0 || h1) {
#pragma unroll
        for (int k = 0; k < NL; ++k) {
          const int n = lane + 64 * k;
          nz0 |= nzbits(c0[k]);
          nz1 |= nzbits(c1[k]);
          if (n < N) bufA[n] = make_float2(c0[k], c1[k]);
        }
      }
      if (s0 + 2 < kTabSub * kTabEnt) load_pair(s0 + 2, c0, c1, ch0, ch1);
      if (h0 || h1) {
        wave_sync();
        X = FftPlan<N>::T::run(bufA, bufB, tw, lane);
      }
      const bool l0 = __ballot(nz0 != 0) != 0, l1 = __ballot(nz1 != 0) != 0;
      float2* o0 = tab + (((int64_t)p * kTabEnt + e0) * kTabSub + q0) * BINS;
      float2* o1 = tab + (((int64_t)p * kTabEnt + e1) * kTabSub + q1) * BINS;
      for (int f = lane; f < BINS; f += 64) {
        float2 p0 = make_float2(0.f, 0.f), p1 = p0;
        if (X && f <= N / 2) {
          const float2 za = X[f], zc = X[f == 0 ? 0 : N - f];
          // P / 2 of each slice (the consumers separate 2 R from their own transforms)
          p0 = make_float2(0.25f * (za.x + zc.x), 0.25f * (za.y - zc.y));
          p1 = make_float2(0.25f * (za.y + zc.y), -0.25f * (za.x - zc.x));
        }
        if (f == BINS - 1) {
          p0 = make_float2(l0 ? 1.f : 0.f, 0.f);
          p1 = make_float2(l1 ? 1.f : 0.f, 0.f);
        }
        o0[f] = p0;
        o1[f] = p1;
      }
      wave_sync();
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The validated stack launch: the correlation waves and the window validity scan (vsg_scan.h) in one kernel.
// correlation waves raise their issue priority while they correlate (scan waves stay at 0);
// 1 / 2 / 3 all measured 127.7 k -> 136 k windows/s on synth10k (at
// 7 + 1 waves, when the correlation was the launch's longer half; not re-measured for the 5 + 3 shape)
constexpr int kCorrPrio = 2;

// The row tasks of a stack launch: frequency-domain stacking with the engine's exact (N = w) transforms, or
// with a zero-padded one (stackp_tasks).
template <class E>
__device__ __forceinline__ void stack_tasks(E& eng, const VsgArgs& A, const float* __restrict__ scales,
                                            const int32_t* __restrict__ order, const int32_t* __restrict__ chunk_tab,
                                            int32_t n_chunk, const float* __restrict__ weight, float* __restrict__ stack,
                                            int64_t t0, TaskSource src) {
  if constexpr (E::kExact) stackf_tasks<E>(eng, A, scales, order, chunk_tab, n_chunk, weight, stack, t0, src);
  else stackp_tasks<E>(eng, A, scales, order, chunk_tab, n_chunk, weight, stack, t0, src);
}

// Persistent validated stack launch: blocks of kFft correlation waves + kScan scan waves (EngF500: two per CU;
// the 1 024-point engines' LDS and registers allow one).  EXACT repeats E::kExact: it is part of the kernels'
// symbol names, which the benchmark and the committed profiles look up.
template <class E, int kFft, int kScan, int kOcc, bool EXACT = true, int kDepth = kScanDepth, int kSpanDepth = 8>
__global__ __launch_bounds__(64 * (kFft + kScan), kOcc) void vsg_stackv_kernel(
    VsgArgs A, const float* __restrict__ scales, const int32_t* __restrict__ order,
    const int32_t* __restrict__ chunk_tab, int32_t n_chunk, const float* __restrict__ weight,
    float* __restrict__ stack, ScanArgs S, uint32_t* __restrict__ vflag, uint32_t* __restrict__ counter,
    const float2* __restrict__ ptab, int32_t span_req) {
  static_assert(EXACT == E::kExact, "EXACT repeats the engine's constant");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  E eng = make_engine<E>(lds);
  bind_engine(eng, A, ptab);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // the chunks cover order[0, end of the last chunk): scan in that order when it lists every pass
  const int32_t* sorder = (n_chunk > 0 && sld(chunk_tab + 3 * (n_chunk - 1) + 1) == A.n_pass) ? order : nullptr;
  // covered-span scan (the host checked window layout and alignment): every pass's slices are loaded by the
  // correlation only when the chunks list every pass
  const bool span = E::kFused && span_req && sorder && !S.tab;
  if constexpr (E::kFused) {
    if (span) eng.vflag = vflag;
  }
  // the padded engines' correlation waves pull row tasks (w = 499: fused launch 4.80 -> 3.99 ms, their task costs vary
  // with the pivot-slice table's coverage); the exact ones keep the static stride (pulled, synth10k / weights measured
  // no better: balanced waves all join the scan at once)
  TaskSource src;
  src.stride = (int64_t)gridDim.x * kFft;
  if constexpr (!E::kExact) src.q = counter + 1;
  if (wave < kFft) {
    __builtin_amdgcn_s_setprio(kCorrPrio);  // correlation waves issue first when both are ready
    stack_tasks<E>(eng, A, scales, order, chunk_tab, n_chunk, weight, stack, (int64_t)xcd_block() * kFft + wave, src);
    __builtin_amdgcn_s_setprio(0);
  }
  scan_units<kDepth, kSpanDepth>(A, S, vflag, counter, lane, sorder, span);
}

// stack[slot] = NaN for every slot holding a pass whose window is invalid (vflag NaN / inf or 0).
// Block (slot, part): the slot's passes are found through chunk_tab; part j fills elements
// [j * 4096, (j + 1) * 4096) of the slot.
constexpr int kFillBlock = 256;
__global__ __launch_bounds__(kFillBlock) void vsg_invalid_fill_kernel(const int32_t* __restrict__ order,
                                                                      const int32_t* __restrict__ chunk_tab,
                                                                      int32_t n_chunk, const uint32_t* __restrict__ vflag,
                                                                      const int32_t* __restrict__ unit_scan,
                                                                      float* __restrict__ stack, int64_t slot_elems) {
  const int slot = blockIdx.y;
  int bad = 0;
  for (int c = threadIdx.x; c < n_chunk; c += kFillBlock) {
    if (chunk_tab[3 * c + 2] != slot) continue;
    for (int q = chunk_tab[3 * c]; q < chunk_tab[3 * c + 1]; ++q) {
      const int p = order[q];
      const uint32_t f = vflag[unit_scan ? unit_scan[p] : p];
      bad |= (f >= 0x7f800000u) || (f == 0u);
    }
  }
  if (!__syncthreads_or(bad)) return;
  float* o = stack + (int64_t)slot * slot_elems;
  const int64_t e0 = (int64_t)blockIdx.x * 4096;
  for (int64_t k = e0 + threadIdx.x; k < min(e0 + 4096, slot_elems); k += kFillBlock) o[k] = NAN;
}

// Sum of squares of each pass window (np.linalg.norm(window.data) ** 2), for norm=norm_amp=False.
// One block per pass; wave k takes rows k, k + 8, ...; 16-byte loads, 4 in flight per lane, fp64
// accumulation in a fixed order (deterministic run to run).
constexpr int kSumWaves = kBlock / 64;
__global__ __launch_bounds__(kBlock) void window_sumsq_kernel(const float* __restrict__ win, int64_t pass_stride,
                                                               int64_t ch_stride, int32_t n_ch, int32_t n_t,
                                                               double* __restrict__ out) {
  __shared__ double part[kSumWaves];
  const int p = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* base = win + (int64_t)p * pass_stride;
  const bool vec = (n_t % 4 == 0) && (ch_stride % 4 == 0) && (pass_stride % 4 == 0) &&
                   (reinterpret_cast<uintptr_t>(win) % 16 == 0);
  double s0 = 0.0, s1 = 0.0;
  for (int c = wave; c < n_ch; c += kSumWaves) {
    const float* row = base + (int64_t)c * ch_stride;
    if (vec) {
      const float4* r4 = reinterpret_cast<const float4*>(row);
      const int n4 = n_t / 4;
      int t = lane;
      for (; t + 192 < n4; t += 256) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = r4[t + 64 * u];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          s0 += (double)v[u].x * v[u].x + (double)v[u].y * v[u].y;
          s1 += (double)v[u].z * v[u].z + (double)v[u].w * v[u].w;
        }
      }
      for (; t < n4; t += 64) {
        const float4 v = r4[t];
        s0 += (double)v.x * v.x + (double)v.y * v.y;
        s1 += (double)v.z * v.z + (double)v.w * v.w;
      }
    } else {
      for (int t = lane; t < n_t; t += 64) {
        const double v = row[t];
        s0 += v * v;
      }
    }
  }
  double s = s0 + s1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < kSumWaves; ++k) t += part[k];
    out[p] = t;
  }
}

// ------------------------------------------------------------------------------------------------
// The host's engine table: one descriptor per transform length, built from the engine type (engine_row), and the
// one function from a window length to its descriptor (engine_for).  Everything the entry points launch or size
// comes from the descriptor; nothing below the table names a transform length or an engine type.

// The validated (correlation + validity scan) launch of a transform length: kernel, correlation / scan waves per
// block, blocks per CU, LDS per block.  fn == nullptr: no fused form (the scan is its own launch).
struct VStack {
  const void* fn;
  int fft, scan, bpc;
  size_t lds;
};
template <class E, int F, int SC, int OCC, int DEPTH = kScanDepth, int SPAN = 8>
static VStack vstack(int bpc) {
  return VStack{(const void*)vsg_stackv_kernel<E, F, SC, OCC, E::kExact, DEPTH, SPAN>, F, SC, bpc,
                E::kBlockBytes + F * E::kWaveBytes};
}

struct VsgEngine {
  int nfft;                             // transform length
  bool exact;                           // serves w == nfft; else every w with 2w - 1 <= nfft (zero padded)
  const void *scales, *gather, *stack;  // scales, gather and plain stack kernels: `waves` waves, `lds` bytes a block
  int waves;
  size_t lds;
  VStack v;                  // validated launch
  VStack vs;                 // its shape for a launch held by its scan (pick_vstack), if the engine has one
  const void* table;         // pivot-slice table kernel (the fused-stage engines), or nullptr
  size_t table_lds;          // the engine's block tables + 4 waves' buffers (EngP1024's padded buffer A included)
  int64_t table_pass_bytes;  // table workspace per pass: the entries' spectra and their (start, nwin) head
  bool span;                 // the covered-span scan may be requested
};

template <class E>
static VsgEngine engine_row(VStack v = VStack{}, bool span = false, VStack vs = VStack{}) {
  VsgEngine d{};
  d.nfft = E::NFFT;
  d.exact = E::kExact;
  d.scales = (const void*)vsg_scales_kernel<E>;
  d.gather = (const void*)vsg_gather_kernel<E>;
  if constexpr (E::kExact) d.stack = (const void*)vsg_stackf_kernel<E>;
  else d.stack = (const void*)vsg_stackp_kernel<E>;
  d.waves = E::kWaves;
  d.lds = E::kBlockBytes + E::kWaves * E::kWaveBytes;
  d.v = v;
  d.vs = vs;
  if constexpr (E::kFused) {
    d.table = (const void*)vsg_pivot_table_kernel<E>;
    d.table_lds = E::kBlockBytes + 4 * E::kWaveBytes;
    d.table_pass_bytes = tab_pass_f2<E::kTabBins>() * (int64_t)sizeof(float2) + 2 * kTabEnt * (int64_t)sizeof(int32_t);
  }
  d.span = span;
  return d;
}

// Validated launch shapes.  EngF500: blocks of 7 correlation + 1 scan waves, 2 blocks per CU (4 waves per SIMD, the
// registers sized for it by the launch bounds); a launch held by its scan runs 5 + 3 instead (pick_vstack).  With the
// covered-span scan and the 10 x 10 x 5 engine synth10k is such a launch: 12.49-12.51 ms at 7 + 1 -> 11.09 ms at
// 5 + 3 (72.7 GB: 6.56 TB/s); weights, held by its correlation, would pay 1-3 % (1.20-1.21 -> 1.22-1.25 ms) and
// stays at 7 + 1 (profiles/eng500_wave_mix.json).  The correlation waves' task stride is grid x the
// correlation waves per block: 6 + 2 and 4 + 4 give strides of 3 and 2 rows modulo synth10k's 1 023 gather rows, a
// wave then stays among rows of one cost, and both measured slower than 7 + 1 (13.3-13.5 ms).
// EngP1024: 7 + 1 waves, one block per CU (LDS, registers), its scan
// waves keeping 32 loads per lane in flight (w = 499 synth10k launch 14.70 vs 15.08 ms at 16, 14.92 at 48).
constexpr int kVsFft = 7, kVsScan = 1, kVsBpc = 2, kVsOcc = 4;
constexpr int kVsHeavyFft = 5, kVsHeavyScan = 3;
// A launch takes the scan-heavy shape when it scans at least this many window bytes per (pass, gather row) it
// correlates.  One (pass, row) costs the 14 correlation waves of a CU 3.4 ns of the launch on synth10k (corr7 7.0 ms,
// rows served by the pivot-slice table) and 5.1-5.4 ns on weights (corr7 0.93-0.97 ms, 48 rows); in those times a
// 6.4 TB/s stream moves 22 and 33-34 KB: below the first a launch is held by its correlation whatever its rows cost,
// above the second by its scan.  The entry point does not see what a launch's rows cost, so the threshold sits
// between the two workloads: synth10k scans 32.8 KB per (pass, row), weights 27.5 KB.
constexpr int64_t kVsHeavyBytes = 30000;
constexpr int kVsSpan = 11;  // the covered-span scan's loads per lane in flight in the EngF500 launch: the most without
                             // spills (12 spill; 11 vs 8: synth10k 13.06 vs 13.09-13.13 ms, profiles/r6_ab)
constexpr int kP1Fft = 7, kP1Scan = 1, kP1Depth = 32;

// The engine of window length w: exact mixed-radix when available, else a zero-padded power of two >= 2w - 1 (linear
// correlation folded back to circular).  nullptr if unsupported.
// The covered-span scan is requested for EngF500 only: synth10k launch 13.27-13.28 -> 13.06-13.13 ms, weights
// 1.304-1.312 -> 1.263-1.289 ms; on the padded engine it lost (w = 499 synth10k 14.8-15.0 -> 16.3-17.1 ms at 8 or 16
// loads per lane in flight against the whole-window scan's 32).
static const VsgEngine* engine_for(int w) {
  static const VsgEngine rows[] = {
      engine_row<EngStockham<250, false>>(),
      engine_row<EngF500>(vstack<EngF500, kVsFft, kVsScan, kVsOcc, kScanDepth, kVsSpan>(kVsBpc), /*span=*/true,
                          vstack<EngF500, kVsHeavyFft, kVsHeavyScan, kVsOcc, kScanDepth, kVsSpan>(kVsBpc)),
      engine_row<EngStockham<1000, false>>(),
      engine_row<EngStockham<512, true>>(vstack<EngStockham<512, true>, 7, 1, 2>(1)),
      engine_row<EngP1024>(vstack<EngP1024, kP1Fft, kP1Scan, 2, kP1Depth>(1)),
      engine_row<EngStockham<2048, true>>(),
  };
  for (const VsgEngine& e : rows)  // the exact rows first
    if (e.exact ? w == e.nfft : 2 * w - 1 <= e.nfft) return &e;
  return nullptr;
}

// The validated launch shape of one launch: the engine's scan-heavy one when it has one and the launch scans at least
// kVsHeavyBytes of windows (n_win of n_ch x n_t floats) per (pass, gather row) it correlates.
static const VStack& pick_vstack(const VsgEngine& e, int64_t n_win, int64_t n_ch, int64_t n_t, int64_t n_pass,
                                 int64_t R) {
  const bool heavy = e.vs.fn && n_win * n_ch * n_t * (int64_t)sizeof(float) >= kVsHeavyBytes * n_pass * R;
  return heavy ? e.vs : e.v;
}

static int check_common(const VsgArgs& A) {
  if (!A.win || !A.pass_tab || !A.seg_tab) return set_error(-2, "null pointer argument");
  if (A.n_pass < 0 || A.R <= 0 || A.w < 2 || A.hop < 1) return set_error(-2, "invalid geometry (R, w, hop)");
  return 0;
}

static int launch(const void* fn, int grid, int waves, size_t lds, void** args, hipStream_t s) {
  if (grid <= 0) return 0;
  if (int rc = set_dynamic_lds(fn, lds)) return rc;
  return hip_status(hipLaunchKernel(fn, dim3(grid), dim3(64 * waves), args, lds, s));
}

// The entry points' common start: the geometry, then the entry point's own argument check (arg_error: its message,
// or nullptr), then the engine of the window length -- refused before anything is launched or zeroed.
struct VsgCall {
  VsgArgs A;
  const VsgEngine* eng;
  int rc;
};
static VsgCall vsg_begin(const VsgArgs& A, const char* arg_error) {
  VsgCall c{A, nullptr, 0};
  if ((c.rc = check_common(A))) return c;
  if (arg_error) c.rc = set_error(-2, arg_error);
  else if (!(c.eng = engine_for(A.w))) c.rc = set_error(-4, "unsupported correlation window length");
  return c;
}

// blocks of `waves` waves, one task per wave (the launches stride over what the clamp leaves)
static int task_grid(int64_t tasks, int waves) {
  const int64_t grid = (tasks + waves - 1) / waves;
  return (int)(grid > (1 << 30) ? (1 << 30) : grid);
}

static int launch_table(const VsgEngine& e, VsgArgs& A, float2* tab, hipStream_t s) {
  const int grid = (int)std::min<int64_t>(((int64_t)A.n_pass + 3) / 4, 8 * (int64_t)cu_count());
  void* args[] = {&A, &tab};
  return launch(e.table, grid, 4, e.table_lds, args, s);
}

// The pivot-slice table if one is given, then the plain stack launch.
static int launch_stack(const VsgEngine& e, VsgArgs& A, const float* scales, const int32_t* order,
                        const int32_t* chunk_tab, int32_t n_chunk, const float* weight, float* stack, float2* tab,
                        hipStream_t s) {
  if (tab)
    if (int rc = launch_table(e, A, tab, s)) return rc;
  void* args[] = {&A, &scales, &order, &chunk_tab, &n_chunk, &weight, &stack, &tab};
  return launch(e.stack, task_grid((int64_t)n_chunk * A.R, e.waves), e.waves, e.lds, args, s);
}

}  // namespace dvh

using namespace dvh;

DVH_API int dvh_vsg_fft_length(int32_t w) {
  const VsgEngine* e = engine_for(w);
  return e ? e->nfft : 0;
}

DVH_API int dvh_vsg_stack_validated_waves(int32_t w, int32_t n_win, int32_t n_ch, int32_t n_t, int32_t n_pass,
                                          int32_t R) {
  const VsgEngine* e = engine_for(w);
  if (!e || !e->v.fn) return 0;
  const VStack& v = pick_vstack(*e, n_win, n_ch, n_t, n_pass, R);
  return 16 * v.fft + v.scan;
}

DVH_API int dvh_window_sumsq(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass, int32_t n_ch,
                             int32_t n_t, double* out, void* stream) {
  if (!win || !out) return set_error(-2, "null pointer argument");
  if (n_pass <= 0) return 0;
  hipLaunchKernelGGL(window_sumsq_kernel, dim3(n_pass), dim3(kBlock), 0, (hipStream_t)stream, win, pass_stride,
                     ch_stride, n_ch, n_t, out);
  return last_launch();
}

DVH_API int dvh_vsg_scales(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass,
                           const int32_t* pass_tab, const int32_t* seg_tab, int32_t R, int32_t w, int32_t hop,
                           int32_t flags, const double* win_sumsq, float* scales, void* stream) {
  VsgCall c = vsg_begin({win, pass_stride, ch_stride, pass_tab, seg_tab, n_pass, R, w, hop, flags},
                        !scales ? "null scales"
                        : (!(flags & kFlagNormAmp) && !(flags & kFlagNorm) && !win_sumsq)
                            ? "win_sumsq required when norm and norm_amp are both off"
                            : nullptr);
  if (c.rc) return c.rc;
  const VsgEngine& e = *c.eng;
  void* args[] = {&c.A, &win_sumsq, &scales};
  return launch(e.scales, task_grid(n_pass, e.waves), e.waves, e.lds, args, (hipStream_t)stream);
}

DVH_API int dvh_vsg_gathers(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass,
                            const int32_t* pass_tab, const int32_t* seg_tab, int32_t R, int32_t w, int32_t hop,
                            int32_t flags, const float* scales, float* out, void* stream) {
  VsgCall c = vsg_begin({win, pass_stride, ch_stride, pass_tab, seg_tab, n_pass, R, w, hop, flags},
                        (!scales || !out) ? "null pointer argument" : nullptr);
  if (c.rc) return c.rc;
  const VsgEngine& e = *c.eng;
  void* args[] = {&c.A, &scales, &out};
  return launch(e.gather, task_grid((int64_t)n_pass * R, e.waves), e.waves, e.lds, args, (hipStream_t)stream);
}

DVH_API int64_t dvh_vsg_stack_workspace(int32_t n_pass, int32_t w) {
  const VsgEngine* e = engine_for(w);
  if (n_pass <= 0 || !e || !e->table) return 0;
  return n_pass * e->table_pass_bytes;
}

DVH_API int dvh_vsg_stack_validated(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass,
                                    int32_t n_ch, int32_t n_t, const int32_t* pass_tab, const int32_t* seg_tab, int32_t R,
                                    int32_t w, int32_t hop, int32_t flags, const float* scales, const int32_t* order,
                                    const int32_t* chunk_tab, int32_t n_chunk, int32_t n_slot, const float* weight,
                                    float* stack, const int32_t* scan_tab, int32_t n_scan, const int32_t* unit_scan,
                                    uint32_t* work, void* spec_ws, void* stream) {
  VsgCall c = vsg_begin(
      {win, pass_stride, ch_stride, pass_tab, seg_tab, n_pass, R, w, hop, flags},
      (!scales || !order || !chunk_tab || !weight || !stack || !work) ? "null pointer argument"
      : !(flags & (kFlagNorm | kFlagNormAmp))
          ? "validated stacking needs norm or norm_amp (raw scales need ||data||_F: dvh_window_sumsq)"
      : (n_ch < R || n_t <= 0)                             ? "window smaller than the gather"
      : ((scan_tab == nullptr) != (unit_scan == nullptr)) ? "scan_tab and unit_scan go together"
      : (scan_tab && n_scan <= 0)                          ? "a scan table needs n_scan > 0"
                                                           : nullptr);
  if (c.rc) return c.rc;
  const VsgEngine& e = *c.eng;
  VsgArgs& A = c.A;
  const ScanArgs S{scan_tab, scan_tab ? n_scan : n_pass, n_ch, n_t};
  hipStream_t s = (hipStream_t)stream;
  uint32_t* vflag = work;
  uint32_t* counter = work + S.n_win;
  float2* tab = (e.table && spec_ws) ? reinterpret_cast<float2*>(spec_ws) : nullptr;
  if (int rc = hip_status(hipMemsetAsync(work, 0, sizeof(uint32_t) * ((size_t)S.n_win + 2), s))) return rc;
  // the covered-span scan: an engine that allows it, default windows, 16-byte aligned rows (the kernel also needs the
  // chunks to list every pass, and falls back to the whole-window scan otherwise)
  int32_t span = (e.span && !scan_tab && n_t % 4 == 0 && ch_stride % 4 == 0 && pass_stride % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(win) % 16 == 0 &&
                  ((int64_t)(n_ch - 1) * ch_stride + n_t) * 4 < 0xfffffff0LL) ? 1 : 0;
  if (e.v.fn) {
    if (tab)
      if (int rc = launch_table(e, A, tab, s)) return rc;
    const VStack& v = pick_vstack(e, S.n_win, n_ch, n_t, n_pass, R);
    const int64_t need = ((int64_t)n_chunk * R + v.fft - 1) / v.fft;
    const int grid = (int)(need < v.bpc * cu_count() ? (need > 0 ? need : 1) : v.bpc * cu_count());
    void* args[] = {&A, &scales, &order, &chunk_tab, &n_chunk, &weight, &stack, (void*)&S, &vflag, &counter, &tab, &span};
    if (int rc = launch(v.fn, grid, v.fft + v.scan, v.lds, args, s)) return rc;
    if (span && S.n_win > 0) {  // the windows the covered-span scan could not decide, rescanned whole
      hipLaunchKernelGGL(window_fixup_kernel, dim3((unsigned)S.n_win), dim3(256), 0, s, A, S, vflag);
      if (int rc = last_launch()) return rc;
    }
  } else {  // no fused form: the scan as its own launch, then the plain stack launch
    void* sargs[] = {&A, (void*)&S, &vflag, &counter};
    if (int rc = launch((const void*)window_scan_kernel, 4 * cu_count(), 4, 0, sargs, s)) return rc;
    if (int rc = launch_stack(e, A, scales, order, chunk_tab, n_chunk, weight, stack, tab, s)) return rc;
  }
  if (n_slot <= 0 || n_chunk <= 0) return 0;
  const int64_t slot_elems = (int64_t)R * w;
  hipLaunchKernelGGL(vsg_invalid_fill_kernel, dim3((unsigned)((slot_elems + 4095) / 4096), n_slot), dim3(kFillBlock), 0,
                     s, order, chunk_tab, n_chunk, (const uint32_t*)vflag, unit_scan, stack, slot_elems);
  return last_launch();
}

DVH_API int dvh_vsg_stack(const float* win, int64_t pass_stride, int64_t ch_stride, int32_t n_pass,
                          const int32_t* pass_tab, const int32_t* seg_tab, int32_t R, int32_t w, int32_t hop,
                          int32_t flags, const float* scales, const int32_t* order, const int32_t* chunk_tab,
                          int32_t n_chunk, const float* weight, float* stack, void* spec_ws, void* stream) {
  VsgCall c = vsg_begin({win, pass_stride, ch_stride, pass_tab, seg_tab, n_pass, R, w, hop, flags},
                        (!scales || !order || !chunk_tab || !weight || !stack) ? "null pointer argument" : nullptr);
  if (c.rc) return c.rc;
  float2* tab = (c.eng->table && spec_ws) ? reinterpret_cast<float2*>(spec_ws) : nullptr;
  return launch_stack(*c.eng, c.A, scales, order, chunk_tab, n_chunk, weight, stack, tab, (hipStream_t)stream);
}
