"""NumPy / SciPy restatement of the reference's vehicle tracker (KF_tracking, apis/tracking.py:21-168, with
likelihood_1d, remove_unrealistic_tracking and interp_nan_value of modules/car_tracking_utils.py:21-66) that runs on
current NumPy.  Test support only: the product never imports it.  tests/test_tracker_ref.py pins it to the reference's
own outputs (tests/golden/tracker_*.npz); the GPU tests and tools/bench_tracker.py use it as the CPU statement of
the chain and of its stages."""
import numpy as np
import scipy.signal
import scipy.stats

FACTOR = 3          # every third grid row is tracked
AHEAD, BEHIND = 30, 15   # a match lies in (base - BEHIND, base + AHEAD]
DEFAULT_DETECT = dict(minprominence=0.2, minseparation=50, prominenceWindow=600)


def row_peaks(row, detect):
    return scipy.signal.find_peaks(row, prominence=detect["minprominence"], wlen=detect["prominenceWindow"],
                                   distance=detect["minseparation"])[0]


def distance_order_free(row, distance):
    """True when find_peaks' distance rule on this row does not depend on the order in which equal heights are
    visited (SciPy takes it from an unstable np.argsort): every local maximum that has an equally high one closer
    than `distance` also has a strictly higher kept one that close, so it is removed before its turn whatever the
    order (by induction from the top, the kept set above a height is unique)."""
    row = np.asarray(row)
    cand = scipy.signal.find_peaks(row)[0]
    kept = scipy.signal.find_peaks(row, distance=distance)[0]
    near = np.abs(cand[:, None] - cand[None, :]) < distance
    tied = near & (row[cand][:, None] == row[cand][None, :]) & ~np.eye(len(cand), dtype=bool)
    covered = ((np.abs(cand[:, None] - kept[None, :]) < distance) & (row[kept][None, :] > row[cand][:, None])).any(1)
    return not (tied.any(1) & ~covered).any()


def likelihood(peak_lists, t_axis, sigma):
    """The detection curve: per row the sum over its peaks of norm.pdf centred on the peak's time, rows added in
    order."""
    out = np.zeros(len(t_axis))
    for peaks in peak_lists:
        row = np.zeros(len(t_axis))
        for p in peaks:
            row = row + scipy.stats.norm.pdf(t_axis, loc=t_axis[p], scale=sigma)
        out += row
    return out


def detect(data, t_axis, x_axis, start_x, detect_args=DEFAULT_DETECT, nx=15, sigma=0.1):
    """detect_in_one_section -> (veh_base, peak_erode, the nx peak lists)."""
    i0 = int(np.argmin(np.abs(start_x - x_axis)))
    lists = [row_peaks(data[i0 + i], detect_args) for i in range(nx)]
    erode = likelihood(lists, t_axis, sigma)
    base = scipy.signal.find_peaks(erode, height=0.0, distance=detect_args["minseparation"])[0]
    return base, erode, lists


def kf_track(peak_lists, x_sel, veh_base, sigma_a=0.01, trace=None):
    """The association and Kalman loop over the tracked rows' peak lists (positions x_sel) ->
    veh_states [n_veh, n_steps], NaN or a peak index.  ``trace``, a [n_veh, n_steps] float64 array, receives the
    float64 predicted arrival of every step that has one (the rest is left as it is); the result does not depend
    on it."""
    n_veh, n_steps = len(veh_base), len(peak_lists)
    states = np.full((n_veh, n_steps), np.nan)
    T = np.zeros((n_veh, 2))       # filtered state: arrival sample, samples per metre
    P = np.zeros((n_veh, 2, 2))
    Tp = np.zeros((n_veh, 2))      # predicted
    Pp = np.zeros((n_veh, 2, 2))
    xv = np.zeros(n_veh)
    count = np.zeros(n_veh, int)
    for k in range(n_steps):
        peaks = np.asarray(peak_lists[k], dtype=np.int64)
        for v in range(n_veh):
            if count[v] == 0:
                base = int(veh_base[v])
            elif count[v] == 1:
                j = int(np.flatnonzero(~np.isnan(states[v]))[0])
                T[v] = (states[v, j], 0.0)
                xv[v] = x_sel[j]
                P[v] = 0.0
                base = int(veh_base[v])
            else:
                dx = x_sel[k] - xv[v]
                A = np.array([[1.0, dx], [0.0, 1.0]])
                Q = sigma_a * np.array([[0.25 * dx ** 4, 0.5 * dx ** 3], [0.5 * dx ** 3, dx ** 2]])
                Tp[v] = A @ T[v]
                Pp[v] = A @ P[v] @ A.T + Q
                if trace is not None:
                    trace[v, k] = Tp[v, 0]
                base = int(Tp[v, 0])   # truncated toward zero, as the reference's integer array does
            dist = peaks - base
            ahead = dist[(dist > 0) & (dist <= AHEAD)]
            behind = dist[(dist > -BEHIND) & (dist <= 0)]
            if len(ahead):
                states[v, k] = base + ahead.min()
            elif len(behind):
                states[v, k] = base + behind.max()
            if not np.isnan(states[v, k]):
                count[v] += 1
                if count[v] > 2:
                    K = Pp[v][:, 0] / (1.0 + Pp[v][0, 0])
                    T[v] = Tp[v] + K * (states[v, k] - Tp[v, 0])
                    P[v] = Pp[v] - np.outer(K, Pp[v][0])
                    xv[v] = x_sel[k]
    return states


def remove_unrealistic(states, adjacency_lim=20):
    """remove_unrealistic_tracking on the [n_veh, n_steps] matches -> (kept rows with their > 20-sample jumps set to
    NaN, indices of the kept vehicles).  The vehicle is judged before its jumps are removed."""
    states = np.array(states, dtype=np.float64, copy=True)
    n = states.shape[1]
    keep = []
    for v, s in enumerate(states):
        idx = np.flatnonzero(~np.isnan(s))
        m = s[idx]
        d = np.diff(m)
        adjacent = int(np.sum(np.diff(np.flatnonzero(np.isnan(s))) == 1))
        bad = len(m) < 0.3 * n
        bad = bad or bool(np.sum(np.convolve(d, np.ones(20), mode="valid") <= -15))
        bad = bad or abs(np.sum(d)) < 30 * (len(m) / n)
        bad = bad or adjacent >= adjacency_lim
        if not bad:
            keep.append(v)
        s[idx[np.flatnonzero(np.abs(d) > 20) + 1]] = np.nan
    return states[keep], np.array(keep, dtype=np.int64)


def spread_and_interp(tracked, factor=FACTOR):
    """The matches on every factor-th column of a [n, n_steps * factor] array, the rest (and the removed matches)
    filled by np.interp, constant past the first and last match."""
    full = np.full((tracked.shape[0], tracked.shape[1] * factor), np.nan)
    full[:, ::factor] = tracked
    for s in full:
        nan = np.isnan(s)
        s[nan] = np.interp(np.flatnonzero(nan), np.flatnonzero(~nan), s[~nan])
    return full


def track(data, t_axis, x_axis, start_x, end_x, veh_base, detect_args=DEFAULT_DETECT, sigma_a=0.01):
    """tracking_with_veh_base -> (tracks, veh_states before the rejection, the tracked rows' peak lists)."""
    i0 = int(np.argmin(np.abs(start_x - x_axis)))
    i1 = int(np.argmin(np.abs(end_x - x_axis)))
    rows = range(i0, i1 + 1, FACTOR)
    lists = [row_peaks(data[i], detect_args) for i in rows]
    raw = kf_track(lists, np.asarray(x_axis)[i0:i1 + 1:FACTOR], veh_base, sigma_a)
    tracked, _ = remove_unrealistic(raw)
    return spread_and_interp(tracked), raw, lists


def chain(data, t_axis, x_axis, start_x, end_x, detect_args=DEFAULT_DETECT, nx=15, sigma=0.08, sigma_a=0.01):
    """track_cars: detection, then the tracks."""
    base, _, _ = detect(data, t_axis, x_axis, start_x, detect_args, nx, sigma)
    return base, track(data, t_axis, x_axis, start_x, end_x, base, detect_args, sigma_a)[0]
