"""The association and Kalman loop of tracking_with_veh_base (apis/tracking.py:101-155) in exact rational arithmetic
(fractions.Fraction).  Test support only: the product never imports it.

It restates tests/tracker_ref.kf_track step by step, with every float64 operation replaced by the exact one: x_sel and
sigma_a enter as the exact rationals of their float64 values, the matches are integers, and the filter state, its
covariance, the gain and the predicted arrival are rationals that are never rounded.  The only non-rational step of
the loop is the one the reference has as well: the predicted arrival is truncated toward zero to give the search base.

What it is for: a float64 implementation (NumPy's or the device's) can differ from this one only where its rounded
prediction truncates to another integer, that is where the exact prediction lies within the implementation's rounding
error of an integer.  exact() therefore returns, next to the matches, the exact predictions and their distance from
the nearest integer, and decided() says for which steps any implementation whose prediction is within DELTA of the
exact one must find the same base:

  * the prediction is an integer and the slope state is exactly 0 (the two-match state, and sigma_a = 0, where the gain
    is 0): the float64 prediction is T0 + dx * 0 = T0, the same integer, with no rounding at all; or
  * the prediction lies more than DELTA from every integer.

A step without a prediction (fewer than two matches so far: the base is veh_base) is decided trivially."""
from fractions import Fraction

import numpy as np

AHEAD, BEHIND = 30, 15   # a match lies in (base - BEHIND, base + AHEAD]
DELTA = 1e-6


def _trunc(q):
    """Fraction -> int, toward zero (int() of a float does the same)."""
    return int(q)   # Fraction.__trunc__


class Exact:
    """states [n_veh, n_steps] float64 (a peak index or NaN); pred[v][k] the exact predicted arrival (Fraction) of a
    step that had one, else None; slope0[v, k] whether the slope state was exactly 0 at that prediction; gap[v, k]
    the prediction's distance from the nearest integer as a float (NaN where there is no prediction)."""

    def __init__(self, states, pred, slope0):
        self.states, self.pred, self.slope0 = states, pred, slope0
        self.gap = np.full(states.shape, np.nan)
        for v, row in enumerate(pred):
            for k, p in enumerate(row):
                if p is not None:
                    self.gap[v, k] = float(abs(p - round(p)))

    def decided(self, delta=DELTA):
        none = np.isnan(self.gap)
        return none | ((self.gap == 0.0) & self.slope0) | (self.gap > delta)

    def closest_undetermined(self):
        """The smallest distance from an integer among the predictions that are not exact integers with slope 0
        (inf when there is none): the margin the float64 implementations have."""
        g = self.gap[~np.isnan(self.gap) & ~((self.gap == 0.0) & self.slope0)]
        return float(g.min()) if g.size else float("inf")

    def match_counts(self):
        """Matches up to and including each step, [n_veh, n_steps]."""
        return np.cumsum(~np.isnan(self.states), axis=1)


def exact(peak_lists, x_sel, veh_base, sigma_a=0.01):
    n_veh, n_steps = len(veh_base), len(peak_lists)
    xs = [Fraction(float(x)) for x in x_sel]
    sa = Fraction(float(sigma_a))
    states = np.full((n_veh, n_steps), np.nan)
    pred = [[None] * n_steps for _ in range(n_veh)]
    slope0 = np.zeros((n_veh, n_steps), dtype=bool)
    half, quarter = Fraction(1, 2), Fraction(1, 4)
    rows = [[int(p) for p in row] for row in peak_lists]
    for v in range(n_veh):
        base0 = int(veh_base[v])
        count = 0
        first = None                      # (match, position) of the first match
        t0 = t1 = Fraction(0)             # filtered state: arrival sample, samples per metre
        p00 = p01 = p10 = p11 = Fraction(0)
        xv = Fraction(0)                  # position of the last update
        for k in range(n_steps):
            if count == 0:
                base = base0
            elif count == 1:              # re-seeded every step while there is exactly one match
                t0, t1 = Fraction(first[0]), Fraction(0)
                xv = first[1]
                p00 = p01 = p10 = p11 = Fraction(0)
                base = base0
            else:
                dx = xs[k] - xv
                tp0, tp1 = t0 + dx * t1, t1                     # A = [[1, dx], [0, 1]]
                a00, a01 = p00 + dx * p10, p01 + dx * p11       # A P
                q00 = a00 + a01 * dx + sa * quarter * dx ** 4   # A P A^T + Q
                q01 = a01 + sa * half * dx ** 3
                q10 = p10 + p11 * dx + sa * half * dx ** 3
                q11 = p11 + sa * dx ** 2
                pred[v][k] = tp0
                slope0[v, k] = t1 == 0
                base = _trunc(tp0)
            ahead = [p - base for p in rows[k] if 0 < p - base <= AHEAD]
            behind = [p - base for p in rows[k] if -BEHIND < p - base <= 0]
            if ahead:
                z = base + min(ahead)
            elif behind:
                z = base + max(behind)
            else:
                continue
            states[v, k] = z
            count += 1
            if count == 1:
                first = (z, xs[k])
            elif count > 2:               # R = 1, C = [1, 0]
                s = 1 + q00
                k0, k1 = q00 / s, q10 / s
                innov = z - tp0
                t0, t1 = tp0 + k0 * innov, tp1 + k1 * innov
                p00, p01, p10, p11 = q00 - k0 * q00, q01 - k0 * q01, q10 - k1 * q00, q11 - k1 * q01
                xv = xs[k]
    return Exact(states, pred, slope0)


def prediction_gap(ex, trace):
    """max |float64 prediction - exact prediction| over the steps that have one; trace[v, k] is the float64
    prediction (NaN where there is none), as tracker_ref.kf_track(..., trace=) records it.  The two must have
    predictions at the same steps."""
    worst = 0.0
    for v, row in enumerate(ex.pred):
        for k, p in enumerate(row):
            assert (p is None) == bool(np.isnan(trace[v, k])), (v, k)
            if p is not None:
                worst = max(worst, float(abs(Fraction(float(trace[v, k])) - p)))
    return worst
