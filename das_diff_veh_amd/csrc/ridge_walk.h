// The ridge walk of extract_ridge_ref_idx (modules/utils.py:621-678) for one wave, over a column source: shared by
// ridge_kernel (dvh_boot.hip), whose columns are a stored f-v image, and slant_ridge_kernel (dvh_slant_ridge.hip), which
// computes the values of a column's window where the walk looks.  The walk's rules -- strict window bounds, np.argmax
// order, the Python-index loop order, the empty-window status, the Savitzky-Golay finish -- are written once, here.
//
// A column source has
//   void first(int i)                          the walk starts at band column i
//   int  argmax(int i, int nxt, int r0, int r1) row of the first maximum of band column i over rows [r0, r1), -1 when
//                                              the range is empty; nxt is the band column the walk visits next (-1:
//                                              none), known before the pick because the walk's order is fixed
// and is called by all 64 lanes together with wave-uniform arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace dvh {

// np.argmax order over (value, row): a NaN beats any number, the first row wins ties
__device__ __forceinline__ bool better(float a, int ra, float b, int rb) {
  const bool na = isnan(a), nb = isnan(b);
  if (na != nb) return na;
  if (na || a == b) return ra < rb;
  return a > b;
}

__device__ __forceinline__ void wave_argmax(float& v, int& r) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o);
    const int r2 = __shfl_xor(r, o);
    if (r2 >= 0 && (r < 0 || better(v2, r2, v, r))) {
      v = v2;
      r = r2;
    }
  }
}

// first row r (of nV, velocities descending) with vel[r] < x: rows [0, r) have vel >= x
__device__ __forceinline__ int first_below(const double* __restrict__ vel, int nV, double x) {
  int lo = 0, hi = nV;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (vel[mid] < x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// first row r with vel[r] <= x
__device__ __forceinline__ int first_at_or_below(const double* __restrict__ vel, int nV, double x) {
  int lo = 0, hi = nV;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (vel[mid] <= x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The velocity axis of a walk held in the wave's registers (nV <= 1024: lane l holds rows l S .. l S + S - 1,
// S = ceil(nV / 64)), so that each step's two window bounds and its pick's velocity cost no memory round trip (the
// binary searches over vel[] were 2 x 10 dependent loads per step, the walk's critical path).  Same results as
// first_below / first_at_or_below / vel[r] on a descending axis; larger axes use those.
struct VelAxis {
  static constexpr int kMaxS = 16;
  const double* vel;
  int nV, S, lane;
  bool regs;
  double v[kMaxS];
  __device__ VelAxis(const double* vel_, int nV_, int lane_) : vel(vel_), nV(nV_), S((nV_ + 63) / 64), lane(lane_) {
    regs = nV <= 64 * kMaxS;
#pragma unroll
    for (int k = 0; k < kMaxS; ++k) {
      const int r = lane * S + k;
      v[k] = (regs && k < S && r < nV) ? vel[r] : 0.0;
    }
  }
  // first row whose velocity satisfies the monotone predicate (rows past nV count as satisfying it), nV if none
  template <class P>
  __device__ __forceinline__ int first(P pred) const {
    int f = S;
#pragma unroll
    for (int k = 0; k < kMaxS; ++k) {
      const int r = lane * S + k;
      if (k < S && f == S && (r >= nV || pred(v[k]))) f = k;
    }
    const uint64_t m = __ballot(f < S);
    if (m == 0) return nV;
    const int L = __ffsll((unsigned long long)m) - 1;
    return min(L * S + __shfl(f, L), nV);
  }
  __device__ __forceinline__ int below(double x) const {  // first_below
    return regs ? first([x](double u) { return u < x; }) : first_below(vel, nV, x);
  }
  __device__ __forceinline__ int at_or_below(double x) const {  // first_at_or_below
    return regs ? first([x](double u) { return u <= x; }) : first_at_or_below(vel, nV, x);
  }
  __device__ __forceinline__ double at(int r) const {  // vel[r] for a wave-uniform row r
    if (!regs) return vel[r];
    const int k = r % S;
    double u = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxS; ++j) u = j == k ? v[j] : u;
    return __shfl(u, r / S);
  }
};

constexpr int kMaxBand = 1024;

// One wave's ridge of resample b on the band's nb columns (rows = velocities in descending order vel[r]).
//   ref == INT32_MIN:  vel_max mode (ref_freq_idx=None), raw picks over rows at/after
//             argmin |vel_max - vel| (no smoothing)
//   vref:     per-column reference velocities (ref_vel(freq)), window (vref - sigma, vref + sigma)
//   else:     pick at column ref over all rows, then walk backward / forward with the window
//             (v_prev - sigma, v_prev + sigma); -nb <= ref < 0 is a Python index with the reference's
//             loop order (below); savgol(sgl, 2, mode='interp') of the picks.
// status[b] = 0, or 1 when a window holds no velocity (np.argmax of an empty slice raises).
// pick: nb doubles of LDS.
template <class Src>
__device__ __forceinline__ void ridge_walk(Src& src, int b, int lane, int32_t nV, int32_t nb,
                                           const double* __restrict__ vel, int32_t ref, double sigma, double vel_max,
                                           const double* __restrict__ vref, const double* __restrict__ sg, int32_t sgl,
                                           double* __restrict__ out, int32_t* __restrict__ status,
                                           double* __restrict__ picks, double* pick) {
  double* o = out + (int64_t)b * nb;
  int err = 0;
  if (ref == INT32_MIN) {
    // max_idx = argmin |vel_max - vel| (first of equal distances)
    double bd = INFINITY;
    int bi = nV;
    for (int r = lane; r < nV; r += 64) {
      const double d = fabs(vel_max - vel[r]);
      if (d < bd || (d == bd && r < bi)) {
        bd = d;
        bi = r;
      }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const double d2 = __shfl_xor(bd, s);
      const int i2 = __shfl_xor(bi, s);
      if (d2 < bd || (d2 == bd && i2 < bi)) {
        bd = d2;
        bi = i2;
      }
    }
    src.first(0);
    for (int i = 0; i < nb; ++i) {
      const int r = src.argmax(i, i + 1 < nb ? i + 1 : -1, bi, nV);
      if (lane == 0) {
        o[i] = r >= 0 ? vel[r] : NAN;
        if (picks) picks[(int64_t)b * nb + i] = o[i];  // nothing is smoothed here: the raw picks are the result
      }
      err |= r < 0;
    }
    if (lane == 0) status[b] = err;
    return;
  }
  const VelAxis ax(vel, nV, lane);
  // the walk over columns i_begin, i_begin + dir, ... (i_end excluded) from the pick velocity v, `after` being the
  // column visited after the last of them; returns the last pick
  auto walk = [&](int i_begin, int i_end, int dir, double v, int after) {
    for (int i = i_begin; i != i_end; i += dir) {
      const int r0 = ax.below(v + sigma), r1 = ax.at_or_below(v - sigma);
      const int r = src.argmax(i, i + dir != i_end ? i + dir : after, r0, r1);
      err |= r < 0;
      v = r >= 0 ? ax.at(r) : NAN;  // (r is wave-uniform: every lane takes part in the shuffle)
      if (lane == 0) pick[i] = v;
    }
    return v;
  };
  if (vref) {
    src.first(0);
    for (int i = 0; i < nb; ++i) {
      const int r0 = ax.below(vref[i] + sigma), r1 = ax.at_or_below(vref[i] - sigma);
      const int r = src.argmax(i, i + 1 < nb ? i + 1 : -1, r0, r1);
      err |= r < 0;
      const double pv = r >= 0 ? ax.at(r) : NAN;
      if (lane == 0) pick[i] = pv;
    }
  } else if (ref < 0) {
    // a negative reference index is a Python index: out[ref] is column nb + ref, the backward loop
    // range(ref - 1, -1, -1) is empty, and range(ref + 1, len(freq)) walks columns nb + ref + 1 ..
    // nb - 1 and then 0 .. nb - 1 again, seeded by out[-1] (modules/utils.py:662-671)
    const int k0 = nb + ref;
    src.first(k0);
    const int rr = src.argmax(k0, k0 + 1 < nb ? k0 + 1 : 0, 0, nV);
    const double v = rr >= 0 ? ax.at(rr) : NAN;
    if (lane == 0) pick[k0] = v;
    walk(0, nb, 1, walk(k0 + 1, nb, 1, v, 0), -1);
  } else {
    const int fwd = ref + 1 < nb ? ref + 1 : -1;  // the forward walk's first column
    src.first(ref);
    const int rr = src.argmax(ref, ref > 0 ? ref - 1 : fwd, 0, nV);
    const double vr = rr >= 0 ? ax.at(rr) : NAN;  // wave-uniform (every lane holds the reduced row)
    if (lane == 0) pick[ref] = vr;
    walk(ref - 1, -1, -1, vr, fwd);  // backward
    walk(ref + 1, nb, 1, vr, -1);    // forward
  }
  __syncthreads();
  if (picks)  // the raw picks before smoothing (parity checks of each pick)
    for (int i = lane; i < nb; i += 64) picks[(int64_t)b * nb + i] = pick[i];
  // savgol_filter(picks, sgl, 2) with mode='interp': interior taps h, edge fits el / er
  const int half = sgl / 2;
  const double* h = sg;
  const double* el = sg + sgl;
  const double* er = el + half * sgl;
  for (int i = lane; i < nb; i += 64) {
    double acc = 0.0;
    if (i < half) {
      for (int t = 0; t < sgl; ++t) acc += el[i * sgl + t] * pick[t];
    } else if (i >= nb - half) {
      for (int t = 0; t < sgl; ++t) acc += er[(i - (nb - half)) * sgl + t] * pick[nb - sgl + t];
    } else {
      for (int t = 0; t < sgl; ++t) acc += h[t] * pick[i - half + t];
    }
    o[i] = acc;
  }
  if (lane == 0) status[b] = err;
}

}  // namespace dvh
