"""Vehicle classes: the quasi-static curve and peak of every pass on the device, and the notebooks' class split.

The first live stage of the four imaging notebooks (imaging_diff_speed.ipynb cells 5, 6, 8, 9, 11 and
imaging_diff_weight.ipynb cells 5, 7, 8, 9, 11; the ``_600`` notebooks do the same):

    das_veh_states[k] [n_ch, n_t] -> mean over channels -> savgol_filter(., 101, 3) -> detrend -> minus first sample
                                  -> peaks[k] = max |curve|                                  quasi_static_curves
    peaks, veh_speed -> histogram mode / mean +- std thresholds                              peak_majority,
                     -> majority filter, fast / mid / slow, heavy / mid / light              speed_majority,
                                                                                             speed_classes, weight_classes
    per-class mean and std curves (cell 11)                                                  class_curve_stats

The per-pass chain is device work (dvh_qs_curves, float64 throughout); the thresholds on a few thousand peaks and
speeds are host NumPy with the notebooks' own expressions, so the same inputs give the same index arrays.  The class
images are then ``engine.stacked([windows[i] for i in sel], prm, slots, n_slot)`` with ``sel, slots, n_slot =
split.subset()``.

The reference ships ``das_veh_states`` and ``veh_speed`` only as pickles and holds no code that makes them, so
``aligned_states_table``, ``quasi_static_curves_from_record`` and ``track_speeds`` are this project's own definition
of those inputs (pinned to a NumPy restatement, tests/classes_ref.py, not to the reference).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .device import default_device
from .modules.utils import _first_at_or_above
from .plan import interp1d_extrap
from .preprocess import _savgol_device, savgol_interp_operator

QS_TILE = 512       # DVH_QS_TILE: interior outputs per block of the kernel's Savitzky-Golay stage
QS_MAX_WLEN = 255   # DVH_QS_MAX_WLEN: the longest window dvh_qs_curves takes

_SHORT = "If mode is 'interp', window_length must be less than or equal to the size of x."
_NONFINITE = "array must not contain infs or NaNs"


def _check_table(off, n_t, numel):
    """The host-side check of a row table: every row's n_t samples lie inside the buffer."""
    off = np.asarray(off)
    if off.size and (int(off.min()) < 0 or int(off.max()) + n_t > numel):
        raise ValueError("row table reaches outside the data")


def _launch(x, row_off, n_pass, n_ch, n_t, window_length, polyorder, want_curves=True):
    """dvh_qs_curves on the flat device tensor x -> (curves [n_pass, n_t] or None, peaks, status), device tensors."""
    dev = x.device
    h, el, er = _savgol_device(window_length, polyorder, dev)
    curves = torch.empty((n_pass, n_t), dtype=torch.float64, device=dev) if want_curves else None
    peaks = torch.empty(n_pass, dtype=torch.float64, device=dev)
    status = torch.zeros(n_pass, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().dvh_qs_curves_workspace(n_pass, n_t) // 8, dtype=torch.float64, device=dev)
    _lib.call("dvh_qs_curves", _lib.ptr(x), 0 if x.dtype == torch.float32 else 1, _lib.ptr(row_off), n_pass, n_ch, n_t,
              _lib.ptr(h), int(window_length), _lib.ptr(el), _lib.ptr(er), _lib.ptr(curves), n_t, _lib.ptr(peaks),
              _lib.ptr(status), _lib.ptr(ws), _lib.stream_of(dev))
    return curves, peaks, status


def _failures(status, skip_failed, index=None):
    """{pass: reason} of the passes whose status is set; raises for the first of them unless skip_failed."""
    bad = np.flatnonzero(status)
    if index is not None:
        bad = np.asarray(index)[bad]
    bad = sorted(int(b) for b in bad)
    if bad and not skip_failed:
        raise ValueError(f"{_NONFINITE} (pass {bad[0]})")
    return {b: _NONFINITE for b in bad}


def _as_batches(states):
    """-> (on_device, [(pass indices, tensor-or-array [n, n_ch, n_t])]) grouped by shape and dtype in first-seen order.
    float32 and float64 are kept, every other dtype goes to float64 on the host, as SciPy does."""
    def norm(a):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            if a.dtype not in (torch.float32, torch.float64):
                raise TypeError("device states must be float32 or float64")
            return a
        a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)
        return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)

    if isinstance(states, (torch.Tensor, np.ndarray)):
        a = norm(states)
        if a.ndim != 3:
            raise ValueError("states must be [n_pass, n_ch, n_t] or a list of [n_ch, n_t] arrays")
        return isinstance(a, torch.Tensor), [(np.arange(a.shape[0]), a)], a.shape[0]
    items = [norm(a) for a in states]
    if any(a.ndim != 2 for a in items):
        raise ValueError("states must be [n_pass, n_ch, n_t] or a list of [n_ch, n_t] arrays")
    on_device = bool(items) and all(isinstance(a, torch.Tensor) for a in items)
    if not on_device:
        items = [a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in items]
    groups = {}
    for i, a in enumerate(items):
        groups.setdefault((tuple(a.shape), str(a.dtype)), []).append(i)
    stack = torch.stack if on_device else np.stack
    return on_device, [(np.asarray(idx), stack([items[i] for i in idx])) for idx in groups.values()], len(items)


def quasi_static_curves(states, window_length=101, polyorder=3, skip_failed=False):
    """The notebooks' quasi-static curves and peaks (speed notebook cell 5, weight notebook cells 7-8):

        curve[k] = detrend(savgol_filter(states[k].mean(0), window_length, polyorder));  curve[k] -= curve[k][0]
        peaks[k] = max |curve[k]|

    ``states``: a device tensor or NumPy array [n_pass, n_ch, n_t], or the notebooks' list of [n_ch, n_t] arrays.
    Mixed shapes are grouped by shape, one launch per shape, and returned in the caller's order: ``curves`` is
    [n_pass, n_t] when every pass has the same length, else a list of curves.  float32 and float64 are taken as they
    are (every sum is float64 on the exact values), anything else is converted to float64 on the host first, as SciPy
    does.  The results are float64: device tensors for a device input, NumPy arrays for a host input.

    Errors are the reference chain's own: n_t < window_length raises savgol_filter's ValueError, a pass holding a
    non-finite value raises detrend's ``ValueError("array must not contain infs or NaNs")`` with the first such pass
    named.  ``skip_failed=True`` does not raise for those: their peaks are NaN and a third value {pass: reason} lists
    them."""
    W = int(window_length)
    savgol_interp_operator(W, polyorder)  # the design's own errors (even window, polyorder >= window_length)
    on_device, batches, n_pass = _as_batches(states)
    if any(b.shape[-1] < W for _, b in batches):
        raise ValueError(_SHORT)
    if any(b.shape[1] < 1 for _, b in batches):
        raise ValueError("a pass needs at least one channel")
    lengths = {b.shape[-1] for _, b in batches}
    curves = [None] * n_pass
    dev = batches[0][1].device if on_device else (default_device() if n_pass else None)
    peaks = torch.empty(n_pass, dtype=torch.float64, device=dev) if n_pass else None
    status = np.zeros(n_pass, dtype=np.int32)
    for idx, b in batches:
        n, n_ch, n_t = b.shape
        if n == 0:
            continue
        x = b.contiguous() if on_device else torch.from_numpy(np.ascontiguousarray(b)).to(dev)
        off = torch.arange(n * n_ch, dtype=torch.int64, device=dev) * n_t
        c, p, st = _launch(x, off, n, n_ch, n_t, W, polyorder)
        peaks[torch.from_numpy(idx).to(dev)] = p
        status[idx] = st.cpu().numpy()
        for j, i in enumerate(idx):
            curves[i] = c[j]
    if n_pass == 0:
        peaks = torch.empty(0, dtype=torch.float64)
        curves_out = torch.empty((0, 0), dtype=torch.float64)
        if on_device:
            curves_out, peaks = curves_out.to(states.device), peaks.to(states.device)
    elif len(lengths) == 1:
        curves_out = c if len(batches) == 1 else torch.stack(curves)
    else:
        curves_out = curves
    failed = _failures(status, skip_failed)
    if not on_device:
        peaks = peaks.cpu().numpy()
        curves_out = [c.cpu().numpy() for c in curves_out] if isinstance(curves_out, list) else curves_out.cpu().numpy()
    return (curves_out, peaks, failed) if skip_failed else (curves_out, peaks)


# ------------------------------------------------------------------------------------------------ the split (host)

@dataclass
class ClassSplit:
    """One notebook cell's split: ``names`` of the classes, ``indices`` (the notebooks' ``np.where(...)[0]`` arrays, in
    the same order) and the ``thresholds`` the cell computed."""
    names: tuple
    indices: tuple
    thresholds: dict

    def __getitem__(self, name):
        return self.indices[self.names.index(name)]

    def subset(self):
        """-> (sel, slots, n_slot): ``sel`` the ascending union of the classes' indices, ``slots`` [len(sel)] the class
        of every selected pass (the position of its class in ``names``), for
        ``engine.stacked([windows[i] for i in sel], prm, slots, n_slot)``."""
        n_slot = len(self.names)
        if not n_slot:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 0
        idx = np.concatenate([np.asarray(i, dtype=np.int64) for i in self.indices])
        cls = np.concatenate([np.full(len(i), k, dtype=np.int64) for k, i in enumerate(self.indices)])
        order = np.argsort(idx, kind="stable")
        return idx[order], cls[order], n_slot


def peak_majority(peaks, width=0.3):
    """Speed notebook cell 6: the passes whose peak lies within ``width`` standard deviations of the histogram's mode
    (the left edge of the fullest of 100 bins), bounds inclusive."""
    peaks = np.asarray(peaks)
    hist, bins = np.histogram(peaks, bins=100)
    mode_peak = bins[np.argmax(hist)]
    sigma = np.std(peaks)
    lower_limit = mode_peak - width*sigma
    upper_limit = mode_peak + width*sigma
    peak_idx = np.where((peaks >= lower_limit) & (peaks <= upper_limit))[0]
    return ClassSplit(("majority",), (peak_idx,), dict(mode_peak=mode_peak, sigma=sigma, lower_limit=lower_limit,
                                                       upper_limit=upper_limit))


def speed_majority(veh_speed):
    """Weight notebook cell 5: the passes whose speed lies within one standard deviation of the mean, inclusive."""
    veh_speed = np.asarray(veh_speed)
    lower_limit = np.mean(veh_speed) - 1*np.std(veh_speed)
    upper_limit = np.mean(veh_speed) + 1*np.std(veh_speed)
    speed_idx = np.where((veh_speed >= lower_limit) & (veh_speed <= upper_limit))[0]
    return ClassSplit(("majority",), (speed_idx,), dict(lower_limit=lower_limit, upper_limit=upper_limit))


def speed_classes(veh_speed):
    """Speed notebook cell 8: fast > mu + sigma, mid <= mu + sigma and > mu - sigma, slow <= mu - sigma."""
    veh_speed = np.asarray(veh_speed)
    threshold_1 = np.mean(veh_speed) + np.std(veh_speed)
    threshold_2 = np.mean(veh_speed) - np.std(veh_speed)
    fast_idx = np.where(veh_speed > threshold_1)[0]
    mid_idx = np.where((veh_speed <= threshold_1) & (veh_speed > threshold_2))[0]
    slow_idx = np.where(veh_speed <= threshold_2)[0]
    return ClassSplit(("fast", "mid", "slow"), (fast_idx, mid_idx, slow_idx),
                      dict(threshold_1=threshold_1, threshold_2=threshold_2))


def weight_classes(peaks, threshold_1=1.2):
    """Weight notebook cell 8: heavy > threshold_1, mid <= threshold_1 and > mode, light <= mode, the mode being the
    left edge of the fullest of 100 histogram bins."""
    peaks = np.asarray(peaks)
    n, bins = np.histogram(peaks, bins=100)
    mode_peak = bins[np.argmax(n)]
    threshold_2 = mode_peak
    heavy_idx = np.where(peaks > threshold_1)[0]
    mid_idx = np.where((peaks <= threshold_1) & (peaks > threshold_2))[0]
    light_idx = np.where(peaks <= threshold_2)[0]
    return ClassSplit(("heavy", "mid", "light"), (heavy_idx, mid_idx, light_idx),
                      dict(threshold_1=threshold_1, threshold_2=threshold_2))


def class_curve_stats(curves, split):
    """Cell 11's curves: per class of ``split`` the mean and the population std of its passes' curves, per sample
    (np.mean(state, axis=0), np.std(state, axis=0)), through dvh_class_curve_stats -> (mean, std [n_class, n_t],
    count [n_class]).  The speed notebook's cell 11 takes np.std of the already averaged curve for two of its classes,
    which is one scalar; the per-sample std, which the weight notebook plots, is returned for every class.  An empty
    class gives NaN rows.  Device curves give device tensors, host curves NumPy arrays."""
    on_device = isinstance(curves, torch.Tensor) and curves.is_cuda
    c = curves if on_device else torch.from_numpy(np.ascontiguousarray(np.asarray(curves, dtype=np.float64))).to(
        default_device())
    if c.dim() != 2 or c.dtype != torch.float64:
        raise ValueError("curves must be float64 [n_pass, n_t]")
    if c.stride(1) != 1 or (c.shape[0] > 1 and c.stride(0) < c.shape[1]):
        c = c.contiguous()
    n_pass, n_t = c.shape
    n_slot = len(split.names)
    slots = np.full(n_pass, -1, dtype=np.int32)
    for k, idx in enumerate(split.indices):
        slots[np.asarray(idx, dtype=np.int64)] = k
    dev = c.device
    mean = torch.empty((n_slot, n_t), dtype=torch.float64, device=dev)
    std = torch.empty((n_slot, n_t), dtype=torch.float64, device=dev)
    count = torch.empty(n_slot, dtype=torch.int32, device=dev)
    _lib.call("dvh_class_curve_stats", _lib.ptr(c), c.stride(0) if n_pass > 1 else n_t,
              _lib.ptr(torch.from_numpy(slots).to(dev)), n_pass, n_t, n_slot, _lib.ptr(mean), _lib.ptr(std),
              _lib.ptr(count), _lib.stream_of(dev))
    if on_device:
        return mean, std, count
    return mean.cpu().numpy(), std.cpu().numpy(), count.cpu().numpy()


# ------------------------------------------------------------------------------------- from a record (build-defined)

def _trajectory(window_or_track):
    if hasattr(window_or_track, "trajectory"):
        return window_or_track.trajectory()
    vx, vt = window_or_track
    return interp1d_extrap(vx, vt)


def aligned_states_table(x_axis, t_axis, window_or_track, start_x, end_x, n_t=1500):
    """The rows of one pass's vehicle-aligned state block in a record (this project's definition; the reference ships
    the blocks as pickles only) -> (ch0, n_ch, t_start [n_ch] int64):

      channels  from the first ``x_axis >= start_x`` up to, not including, the first ``x_axis >= end_x``
      per row   i_c = the first index with ``t_axis >= f(x_c)``, f the pass's trajectory (a window's
                ``trajectory()`` or (veh_state_x, veh_state_t): interp1d_extrap, as the VSG path uses it);
                ``t_start[c] = i_c - n_t // 2``

    The pass is valid (``states_table_valid``) only if every row lies inside the record and f(x_c) <= t_axis[-1]; where
    the vehicle passes a channel after the record's end, i_c is len(t_axis), which puts the row outside."""
    x_axis = np.asarray(x_axis)
    t_axis = np.asarray(t_axis)
    ch0 = _first_at_or_above(x_axis, start_x)
    ch1 = _first_at_or_above(x_axis, end_x)
    n_ch = ch1 - ch0
    if n_ch < 1:
        raise ValueError("no channel in [start_x, end_x)")
    t_at = _trajectory(window_or_track)(x_axis[ch0:ch1])
    i_c = np.searchsorted(t_axis, t_at, side="left").astype(np.int64)
    return ch0, n_ch, i_c - int(n_t) // 2


def states_table_valid(t_start, n_t, rec_n_t):
    """Every row of an aligned_states_table lies inside a record of rec_n_t samples."""
    t_start = np.asarray(t_start)
    return bool(t_start.size) and bool(t_start.min() >= 0) and bool(t_start.max() + int(n_t) <= int(rec_n_t))


def quasi_static_curves_from_record(record, x_axis, t_axis, tracks, start_x, end_x, n_t=1500, window_length=101,
                                    polyorder=3, skip_failed=False, return_curves=True):
    """quasi_static_curves of the vehicle-aligned blocks of ``tracks`` (windows, or (veh_state_x, veh_state_t) pairs)
    read straight from the record [n_ch_rec, n_t_rec] (device tensor, float32 or float64; a host array is uploaded)
    through the row table of aligned_states_table: no [n_pass, n_ch, n_t] batch is made -> (curves, peaks, valid).
    ``valid`` [len(tracks)] bool: the passes whose block lies inside the record; the others are left out of curves
    and peaks (which follow the valid passes in order).  A valid pass holding a non-finite value raises as
    quasi_static_curves does, with the track's index; ``skip_failed=True`` returns {track index: reason} as a fourth
    value instead.  This is the project's own definition of ``das_veh_states`` (see the module docstring)."""
    W = int(window_length)
    savgol_interp_operator(W, polyorder)
    n_t = int(n_t)
    if n_t < W:
        raise ValueError(_SHORT)
    on_device = isinstance(record, torch.Tensor) and record.is_cuda
    if on_device:
        rec = record
        if rec.dtype not in (torch.float32, torch.float64):
            raise TypeError("a device record must be float32 or float64")
    else:
        host = np.asarray(record.detach().cpu() if isinstance(record, torch.Tensor) else record)
        if host.dtype not in (np.float32, np.float64):
            host = host.astype(np.float64)
        rec = torch.from_numpy(np.ascontiguousarray(host)).to(default_device())
    if rec.dim() != 2 or len(x_axis) != rec.shape[0] or len(t_axis) != rec.shape[1]:
        raise ValueError("record must be [len(x_axis), len(t_axis)]")
    if rec.stride(1) != 1 or rec.stride(0) < rec.shape[1]:
        rec = rec.contiguous()
    dev = rec.device
    rec_n_t, row_stride = rec.shape[1], rec.stride(0)
    valid = np.zeros(len(tracks), dtype=bool)
    rows = []
    ch0 = n_ch = 0
    for k, trk in enumerate(tracks):
        ch0, n_ch, t_start = aligned_states_table(x_axis, t_axis, trk, start_x, end_x, n_t)
        valid[k] = states_table_valid(t_start, n_t, rec_n_t)
        if valid[k]:
            rows.append((ch0 + np.arange(n_ch, dtype=np.int64)) * row_stride + t_start)
    index = np.flatnonzero(valid)
    n_pass = len(rows)
    if n_pass:
        off = np.stack(rows)
        _check_table(off, n_t, (rec.shape[0] - 1) * row_stride + rec_n_t)
        curves, peaks, status = _launch(rec, torch.from_numpy(off).to(dev), n_pass, n_ch, n_t, W, polyorder,
                                        want_curves=return_curves)
        status = status.cpu().numpy()
    else:
        curves = torch.empty((0, n_t), dtype=torch.float64, device=dev) if return_curves else None
        peaks = torch.empty(0, dtype=torch.float64, device=dev)
        status = np.zeros(0, dtype=np.int32)
    failed = _failures(status, skip_failed, index)
    if not on_device:
        curves = None if curves is None else curves.cpu().numpy()
        peaks = peaks.cpu().numpy()
    return (curves, peaks, valid, failed) if skip_failed else (curves, peaks, valid)


def track_speeds(veh_states, distance_along_fiber_tracking, t_axis_tracking, start_x_tracking, start_x, end_x):
    """Speed [m/s] of every tracked vehicle over [start_x, end_x] (host NumPy; this project's definition of the
    notebooks' ``veh_speed``): veh_states [n_veh, n_x] holds tracking-time indices per tracking channel (NaN where
    untracked), column j at distance ``distance_along_fiber_tracking[i0 + j]`` with i0 the channel nearest
    start_x_tracking, as SurfaceWaveWindow reads it.  Per vehicle: 1 / slope of the least-squares line t(x) over its
    finite samples with start_x <= x <= end_x; fewer than two samples, or a zero slope, gives NaN."""
    vs = np.atleast_2d(np.asarray(veh_states, dtype=np.float64))
    dist = np.asarray(distance_along_fiber_tracking, dtype=np.float64)
    t_trk = np.asarray(t_axis_tracking, dtype=np.float64)
    i0 = int(np.abs(start_x_tracking - dist).argmin())
    x_all = dist[i0:i0 + vs.shape[1]]
    out = np.full(vs.shape[0], np.nan)
    for v in range(vs.shape[0]):
        row = vs[v, :x_all.size]
        ok = np.isfinite(row) & (x_all >= start_x) & (x_all <= end_x)
        if ok.sum() < 2:
            continue
        x = x_all[ok]
        t = t_trk[row[ok].astype(int)]
        dx = x - x.mean()
        den = np.sum(dx * dx)
        slope = np.sum(dx * (t - t.mean())) / den if den > 0 else 0.0
        if slope != 0.0:
            out[v] = 1.0 / slope
    return out
