"""KF_tracking — apis/tracking.py:12-168 on the device.

  detect_in_one_section   :21-63    find_peaks of nx grid rows (dvh_find_peaks_rows), the detection likelihood
                                    (dvh_peak_likelihood), find_peaks of that curve -> veh_base
  tracking_with_veh_base  :65-168   find_peaks of every third row of the span (one dvh_find_peaks_rows launch), the
                                    association / Kalman loop (dvh_kf_track, one thread per vehicle), then on the host
                                    remove_unrealistic_tracking and interp_nan_value
                                    (modules/car_tracking_utils.py:28-66) on the [n_veh, n_steps] result
``data`` is the tracking grid [n_x, n_t]: a float64 device tensor is used in place (rows may be strided), anything
else is copied to the device as float64.  ``sign=-1`` tracks the peaks of ``-data`` without forming it (the reference's
track_cars passes ``-data_for_tracking``).  The returns are the reference's: veh_base an integer array, the tracks a
host float64 array [n_valid, n_steps * 3].

Kept from the reference as it is: a vehicle searches from veh_base until it has two matches, and is re-seeded from its
single match every step before that; the predicted arrival is truncated toward zero; a match lies in (-15, 30] of the
search base, ahead first; the rejection looks at the match count, a 20-tap moving sum of the differences (NumPy's
``convolve(..., 'valid')``, which for fewer than 20 differences gives their whole sum), the net motion and the number of
adjacent misses, and only afterwards cuts jumps of more than 20 samples; the returned width is n_steps * 3, which can
exceed the span's rows.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib
from ..device import default_device

FACTOR = 3  # tracking_with_veh_base follows every third row


def remove_unrealistic_tracking(veh_states, adjacency_nan_count_lim=20):
    """modules/car_tracking_utils.py:38-66 on the matches of the tracked rows [n_veh, n_steps] -> the kept vehicles'
    rows, their jumps of more than 20 samples set to NaN (after the vehicle was judged)."""
    s = np.array(veh_states, dtype=np.float64, copy=True)
    n = s.shape[1]
    keep = np.zeros(len(s), dtype=bool)
    for v, row in enumerate(s):
        idx = np.flatnonzero(~np.isnan(row))
        m = row[idx]
        d = np.diff(m)
        adjacent = np.count_nonzero(np.diff(np.flatnonzero(np.isnan(row))) == 1)
        keep[v] = not (len(m) < 0.3 * n
                       or np.any(np.convolve(d, np.ones(20), mode="valid") <= -15)
                       or abs(d.sum()) < 30 * (len(m) / n)
                       or adjacent >= adjacency_nan_count_lim)
        row[idx[1:][np.abs(d) > 20]] = np.nan
    return s[keep]


def interp_nan_value(veh_states):
    """modules/car_tracking_utils.py:28-35, in place: NaN -> np.interp over the row's other samples."""
    for row in veh_states:
        nan = np.isnan(row)
        row[nan] = np.interp(np.flatnonzero(nan), np.flatnonzero(~nan), row[~nan])


class KF_tracking:
    def __init__(self, data, t_axis, x_axis, args, sign=1):
        if sign not in (1, -1):
            raise ValueError("sign must be +1 or -1")
        if isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.float64 and data.dim() == 2 \
                and data.stride(1) == 1:
            self.data = data
        else:
            host = data.detach().cpu().numpy() if isinstance(data, torch.Tensor) else np.asarray(data)
            if host.ndim != 2:
                raise ValueError("data must be [n_x, n_t]")
            self.data = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float64)).to(default_device())
        self.sign = int(sign)
        self.t_axis = np.asarray(t_axis)
        self.x_axis = np.asarray(x_axis)
        if self.data.shape != (len(self.x_axis), len(self.t_axis)):
            raise ValueError("data must be [len(x_axis), len(t_axis)]")
        self.dx = self.x_axis[1] - self.x_axis[0]
        self.args = args
        self._t_dev = torch.from_numpy(np.ascontiguousarray(self.t_axis, dtype=np.float64)).to(self.data.device)

    # ------------------------------------------------------------------------------------------ device pieces

    @staticmethod
    def _detect_args(detection_args):
        return (float(detection_args["minprominence"]), float(detection_args["minseparation"]),
                float(detection_args["prominenceWindow"]))

    def find_peaks_rows(self, row0, row_step, n_sel, detection_args):
        """find_peaks(sign * data[row0 + k * row_step], prominence=, wlen=, distance=) for k < n_sel ->
        (peaks [n_sel, cap] int32, count [n_sel] int32) on the device."""
        pmin, sep, wlen = self._detect_args(detection_args)
        d = self.data
        n_x, n_t = d.shape
        if n_sel < 0 or row0 < 0 or (n_sel and row0 + (n_sel - 1) * row_step >= n_x):
            raise IndexError("rows outside the grid")
        return _find_peaks(d, n_t, row0, row_step, n_sel, self.sign, sep, True, pmin, wlen)

    def detect_in_one_section(self, start_x, nx=15, detection_args=None, sigma=0.1, pclip=98, show_plot=False,
                              plt_xlim=1000, _events=None):
        if show_plot:
            raise NotImplementedError("plotting is outside the accelerated path; use the reference's KF_tracking "
                                      "on the host copy of the grid")
        if not detection_args:
            detection_args = self.args["detect"]
        ev = _recorder(_events)
        start_x_idx = int(np.argmin(np.abs(start_x - self.x_axis)))
        if start_x_idx + nx > len(self.x_axis):
            raise IndexError(f"index {start_x_idx + nx - 1} is out of bounds for axis 0 with size {len(self.x_axis)}")
        dev = self.data.device
        st = _lib.stream_of(dev)
        ev("detect_start")
        peaks, count = self.find_peaks_rows(start_x_idx, 1, nx, detection_args)
        ev("detect_peaks")
        n_t = len(self.t_axis)
        erode = torch.empty(n_t, dtype=torch.float64, device=dev)
        _lib.call("dvh_peak_likelihood", _lib.ptr(peaks), peaks.shape[1], _lib.ptr(count), nx, _lib.ptr(self._t_dev),
                  n_t, float(sigma), _lib.ptr(erode), st)
        ev("likelihood")
        self.peak_erode = erode
        sep = self._detect_args(detection_args)[1]
        base, n_base = _find_peaks(erode.view(1, n_t), n_t, 0, 1, 1, 1, sep, False, 0.0, 0.0)
        ev("bases")
        return base[0, :int(n_base[0])].cpu().numpy().astype(np.int64)

    def tracking_with_veh_base(self, start_x, end_x, veh_base, sigma_a=0.01, detection_args=None, _events=None):
        if detection_args is None:
            detection_args = self.args["detect"]
        ev = _recorder(_events)
        start_x_idx = int(np.argmin(np.abs(start_x - self.x_axis)))
        end_x_idx = int(np.argmin(np.abs(end_x - self.x_axis)))
        veh_base = np.asarray(veh_base)
        n_veh = len(veh_base)
        n_steps = len(range(start_x_idx, end_x_idx + 1, FACTOR))
        dev = self.data.device
        st = _lib.stream_of(dev)
        ev("track_start")
        peaks, count = self.find_peaks_rows(start_x_idx, FACTOR, n_steps, detection_args)
        ev("track_peaks")
        self.row_peaks, self.row_counts = peaks, count
        x_sel = torch.from_numpy(np.ascontiguousarray(self.x_axis[start_x_idx:end_x_idx + 1:FACTOR],
                                                      dtype=np.float64)).to(dev)
        base_dev = torch.from_numpy(np.ascontiguousarray(veh_base, dtype=np.int32)).to(dev)
        states = torch.empty((n_veh, n_steps), dtype=torch.float64, device=dev)
        ev("kf_start")
        _lib.call("dvh_kf_track", _lib.ptr(peaks), peaks.shape[1], _lib.ptr(count), n_steps, _lib.ptr(x_sel),
                  _lib.ptr(base_dev), n_veh, float(sigma_a), _lib.ptr(states), st)
        ev("kf")
        self.veh_states_raw = states.cpu().numpy()
        tracked_v = remove_unrealistic_tracking(self.veh_states_raw)
        tracked_v_full = np.full((tracked_v.shape[0], n_steps * FACTOR), np.nan)
        tracked_v_full[:, ::FACTOR] = tracked_v
        interp_nan_value(tracked_v_full)
        return tracked_v_full

    # ------------------------------------------------------------------------------------------ plotting

    def _no_plot(self, *args, **kwargs):
        raise NotImplementedError("plotting is outside the accelerated path; use the reference's KF_tracking on "
                                  "the host copy of the grid")

    tracking_visulization_one_section = plot_data = show_detection_example = _no_plot


def _recorder(events):
    if events is None:
        return lambda k: None

    def record(k):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events[k] = e
    return record


def _find_peaks(x, n_t, row0, row_step, n_sel, sign, distance, use_prominence, min_prominence, wlen):
    """dvh_find_peaks_rows with a cap no row can exceed: (n_t - 1) // 2 local maxima at the most, and with the
    distance on, kept peaks at least ceil(distance) apart."""
    dev = x.device
    cap = max((n_t - 1) // 2, 1)
    if distance > 0:
        cap = min(cap, (n_t - 1) // max(int(math.ceil(distance)), 1) + 1)
    peaks = torch.empty((n_sel, cap), dtype=torch.int32, device=dev)
    count = torch.empty(n_sel, dtype=torch.int32, device=dev)
    if n_sel == 0:
        return peaks, count
    row_stride = x.stride(0) if x.shape[0] > 1 else n_t   # a single row's stride is arbitrary
    _lib.call("dvh_find_peaks_rows", _lib.ptr(x), row_stride, n_t, row0, row_step, n_sel, sign, float(distance),
              1 if use_prominence else 0, float(min_prominence), float(wlen), _lib.ptr(peaks), cap, _lib.ptr(count),
              None, None, _lib.stream_of(dev))
    return peaks, count
