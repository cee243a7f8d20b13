"""NumPy restatement of the vehicle-class chain (das_diff_veh_amd.classes, dvh_qs_curves):

    m      = (x[0] + x[1] + ... + x[n_ch - 1]) / n_ch                  channel order, one division (d.mean(0))
    y      = savgol_filter(m, W, P) as the three maps (h, el, er)      tests/ingest_ref.smooth64
    z      = y - (slope a + icpt),  a[t] = (t + 1) / n_t               scipy.signal.detrend in closed form
    curve  = z - z[0],  peak = max |curve|

in float64, or in longdouble with ``longdouble=True`` (the maps stay SciPy's float64 coefficients: the switch measures
the rounding of the evaluation, not of the design).  Also the NumPy form of the record functions (aligned_states_table
and the gather it stands for), which are this project's own definition.

``bound`` is the derived tolerance the tests hold the chain to; its docstring carries the derivation.
"""
from __future__ import annotations

import numpy as np

from tests import ingest_ref

U = 2.0 ** -53  # unit roundoff of float64


def operator(window_length=101, polyorder=3):
    return ingest_ref.operator(window_length, polyorder)


def channel_mean(x, dtype=np.float64):
    """(sum_c x[c]) / n_ch with the rows added in order, x [..., n_ch, n_t]."""
    x = np.asarray(x).astype(dtype)
    acc = np.zeros(x.shape[:-2] + x.shape[-1:], dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(x.shape[-2]):
            acc = acc + x[..., c, :]
        return acc / dtype(x.shape[-2])


def _savgol(m, h, el, er, dtype):
    if dtype == np.float64:
        return ingest_ref.smooth64(m, h, el, er)
    W, half, n_t = len(h), len(h) // 2, m.shape[-1]
    if n_t < W:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    h, el, er = (a.astype(dtype) for a in (h, el, er))
    out = np.zeros(m.shape, dtype=dtype)
    n_int = n_t - 2 * half
    for j in range(W):
        out[..., half:n_t - half] += h[j] * m[..., j:j + n_int]
    for t in range(half):
        out[..., t] = (el[t] * m[..., :W]).sum(-1)
        out[..., n_t - half + t] = (er[t] * m[..., n_t - W:]).sum(-1)
    return out


def detrend(y, dtype=np.float64):
    """y minus its least-squares line on [(t + 1) / n_t, 1] (scipy.signal.detrend, type='linear') in closed form:
    slope = sum (a - abar) y / sum (a - abar)^2 with abar = (n_t + 1) / (2 n_t) and sum (a - abar)^2 =
    (n_t^2 - 1) / (12 n_t); icpt = sum y / n_t - slope abar."""
    y = np.asarray(y, dtype=dtype)
    n_t = y.shape[-1]
    n = dtype(n_t)
    a = np.arange(1, n_t + 1).astype(dtype) / n
    abar = (n + dtype(1)) / (dtype(2) * n)
    with np.errstate(invalid="ignore", over="ignore"):
        s0 = y.sum(-1, keepdims=True)
        s1 = ((a - abar) * y).sum(-1, keepdims=True)
        slope = s1 / ((n * n - dtype(1)) / (dtype(12) * n))
        icpt = s0 / n - slope * abar
        return y - (slope * a + icpt)


def curves(x, h, el, er, longdouble=False):
    """x [..., n_ch, n_t] (float32 values are upcast exactly) -> (curve [..., n_t], peak [...]).  A pass holding a
    non-finite value gets a NaN peak."""
    dtype = np.longdouble if longdouble else np.float64
    m = channel_mean(x, dtype)
    y = _savgol(m, h, el, er, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        z = detrend(y, dtype)
        c = z - z[..., :1]
        bad = ~np.isfinite(c).all(-1)
        peak = np.where(bad, np.nan, np.abs(c).max(-1))
    return c, peak


def scipy_chain(d):
    """The notebooks' cell: detrend(savgol_filter(d.mean(0), 101, 3)), minus its first sample."""
    import scipy.signal
    c = scipy.signal.detrend(scipy.signal.savgol_filter(d.mean(0), 101, 3))
    return c - c[0]


def bound(n_t, h, el, er, amax):
    """The tolerance on |curve - curve'| between two float64 evaluations of the chain (the restatement against SciPy,
    the kernel against the restatement), as a multiple of u = 2^-53 and X = amax = max |x|.  Every term is a
    worst-case forward bound formed from the coefficient magnitudes of the linear maps, none from a measured error:

      mean     both sides add the rows in channel order and divide once: identical bits, |m| <= X.
      savgol   an output is a W-term dot product with a coefficient row r, sum |r| <= S_sg = max(sum |h|, max row sum
               of |el|, |er|) (1.32, 2.48, 2.48 at (101, 3)).  In any order, with or without fma, it errs by at most
               gamma_W sum |r_j m_j| <= W u S_sg X; two evaluations differ by at most 2 W u S_sg X.  At the edges
               SciPy does not apply rows: it fits a cubic to the W samples (np.polyfit: least squares on the
               column-scaled Vandermonde matrix, condition number K_fit = 84 at W = 101) and evaluates it.  el / er
               are that same procedure on unit vectors, so both sides carry a fit error, to first order
               K_fit u ||x_w||_2 <= K_fit sqrt(W) u X each on the coefficients' side, passed on with the map's gain
               S_sg.  Together:  e_sg = (2 W + 2 K_fit sqrt(W)) S_sg u X,  |y| <= Y = S_sg X.
      detrend  z = (I - P) y, P the projection on span{a, 1}: P[t][s] = 1 / N + (a_t - abar)(a_s - abar) / D.  Its
               absolute row sums are at most S_P = 1 + max|a_t - abar| sum_s |a_s - abar| / D <= 1 + (1/2)(N/4)(12/N)
               = 2.5, so the savgol error passes through with gain 1 + S_P = 3.5.  Its own rounding: the two N-term
               sums err by at most gamma_N sum |.| <= N u N Y in any order (SciPy's are a LAPACK least-squares solve
               of a 2-column system of condition < 4, bounded the same way), which moves the line by at most
               S_P N u Y per side; the line's evaluation and the subtraction add 4 u (1 + S_P) Y per side.
               e_dt = 3.5 e_sg + 2 (S_P N + 4 (1 + S_P)) u Y.
      shift    curve = z - z[0] carries two z errors and one rounding:  e = 2 e_dt + 2 u (1 + S_P) Y.

    At (n_t, W) = (1500, 101) this is 7.0e4 u X = 7.8e-12 X (3.6e4 u X = 4.0e-12 X at n_t = 101); the measured
    differences are 2.8e-15 X (against SciPy) and 5.5e-16 X (float64 against longdouble): the bound is a worst case
    over summation orders and signs, and an indexing or coefficient mistake misses it by ten orders of magnitude."""
    W = len(h)
    s_sg = max(np.abs(h).sum(), np.abs(el).sum(1).max(), np.abs(er).sum(1).max())
    v = np.vander(np.arange(float(W)), min(4, W))
    k_fit = np.linalg.cond(v / np.sqrt((v * v).sum(0)))
    s_p = 2.5
    y_max = s_sg * amax
    e_sg = (2 * W + 2 * k_fit * np.sqrt(W)) * s_sg * U * amax
    e_dt = (1 + s_p) * e_sg + 2 * (s_p * n_t + 4 * (1 + s_p)) * U * y_max
    return 2 * e_dt + 2 * U * (1 + s_p) * y_max


# ---------------------------------------------------------------------------------------------- record functions

def first_at_or_above(axis, value):
    return int(np.argmax(np.asarray(axis) >= value))


def linear_interp(xp, yp, xq):
    """interp1d(kind='linear', fill_value='extrapolate') on ascending xp."""
    xp, yp, xq = (np.asarray(a, dtype=np.float64) for a in (xp, yp, xq))
    i = np.clip(np.searchsorted(xp, xq), 1, xp.size - 1)
    slope = (yp[i] - yp[i - 1]) / (xp[i] - xp[i - 1])
    return slope * (xq - xp[i - 1]) + yp[i - 1]


def states_table(x_axis, t_axis, track, start_x, end_x, n_t):
    """-> (ch0, n_ch, t_start, valid) by plain loops: the definition of aligned_states_table."""
    ch0, ch1 = first_at_or_above(x_axis, start_x), first_at_or_above(x_axis, end_x)
    t_start, valid = [], ch1 > ch0
    for c in range(ch0, ch1):
        t_c = float(linear_interp(track[0], track[1], x_axis[c]))
        above = [i for i in range(len(t_axis)) if t_axis[i] >= t_c]
        if not above or t_c > t_axis[-1]:
            valid = False
            t_start.append(len(t_axis) - n_t // 2)
            continue
        t_start.append(above[0] - n_t // 2)
        if t_start[-1] < 0 or t_start[-1] + n_t > len(t_axis):
            valid = False
    return ch0, ch1 - ch0, np.array(t_start, dtype=np.int64), valid


def gather_states(record, ch0, n_ch, t_start, n_t):
    """The [n_ch, n_t] block a table stands for."""
    return np.stack([record[ch0 + c, t_start[c]:t_start[c] + n_t] for c in range(n_ch)])


def track_speed(veh_state, dist_trk, t_trk, start_x_tracking, start_x, end_x):
    """1 / slope of the least-squares line t(x) over the vehicle's finite samples in [start_x, end_x]; NaN for fewer
    than two samples or a zero slope."""
    i0 = int(np.abs(start_x_tracking - np.asarray(dist_trk)).argmin())
    xs, ts = [], []
    for j, s in enumerate(veh_state):
        if i0 + j < len(dist_trk) and np.isfinite(s) and start_x <= dist_trk[i0 + j] <= end_x:
            xs.append(dist_trk[i0 + j])
            ts.append(t_trk[int(s)])
    if len(xs) < 2:
        return np.nan
    xm, tm = sum(xs) / len(xs), sum(ts) / len(ts)
    slope = sum((x - xm) * (t - tm) for x, t in zip(xs, ts)) / sum((x - xm) ** 2 for x in xs)
    return 1.0 / slope if slope != 0 else np.nan
