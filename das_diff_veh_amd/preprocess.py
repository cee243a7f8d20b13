"""Per-pass windowing / taper / bandpass on device (host side builds the small index tables).

  bandpass_inplace  bandpass_data (modules/utils.py:179-189): butter(10, [flo, fhi] / fNy, 'band',
                    output='sos') designed on the host (filter design, 10 x 6 coefficients), the
                    zero-phase filtering itself in dvh_sosfiltfilt
  mute_along_traj   apis/data_classes.py:49-72: per time sample the taper placement
                    (argmax(x > car(t) - offset/2 + delta_x), clipped) is tabulated on the host with
                    the reference's float64 expressions; the multiply runs in dvh_mute_traj
  mute_along_time   apis/data_classes.py:100-104 -> dvh_mute_time
  surface_wave_preprocessing  TimeLapseImaging._preprocessing_for_surface_waves (apis/timeLapseImaging.py:
                    51-71): bandpass + empty / noisy trace imputation + per-trace L2 norm
  tracking_preprocessing  TimeLapseImaging._preprocess_for_tracking (apis/timeLapseImaging.py:74-102): median
                    gate, empty-trace imputation, 0.08-1 Hz bandpass, 204/25 polyphase resampling onto the
                    1 m x 50 Hz tracking grid, spatial bandpass (dvh_median_abs_gate, dvh_resample_rows_t,
                    dvh_transpose_f64 with the kernels above)
  savgol_smooth     ImagingIO.__getitem__'s savgol_filter(data, 21, 15) and ``data /= scale`` (modules/imaging_IO.py:
                    44-46) in one pass: SciPy's mode='interp' filter as three host-designed linear maps
                    (savgol_interp_operator), evaluated by dvh_savgol_rows
"""
from __future__ import annotations

import numpy as np
import scipy.signal
import torch

from . import _lib
from .device import default_device
from .plan import interp1d_extrap


def butter_bandpass_sos(dt, flo, fhi, order=10):
    fny = 0.5 / dt
    return scipy.signal.butter(order, [flo / fny, fhi / fny], analog=False, btype="band", output="sos")


def _padlen(sos):
    return 3 * (2 * len(sos) + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


def tukey(n, alpha):
    """scipy.signal.windows.tukey(n, alpha) (sym=True)."""
    return scipy.signal.windows.tukey(n, alpha)


class _DeviceView:
    """Device tensor for a host array or tensor, written back in place on exit."""

    def __init__(self, data):
        self.data = data
        if isinstance(data, torch.Tensor) and data.is_cuda:
            self.t = data if data.is_contiguous() else data.contiguous()
        else:
            host = np.asarray(data.detach().cpu() if isinstance(data, torch.Tensor) else data)
            if host.dtype not in (np.float32, np.float64):
                raise TypeError("data must be float32 or float64")
            self.t = torch.from_numpy(np.ascontiguousarray(host)).to(default_device())
        if self.t.dtype not in (torch.float32, torch.float64):
            raise TypeError("data must be float32 or float64")
        self.dtype = 0 if self.t.dtype == torch.float32 else 1

    def write_back(self):
        d = self.data
        if isinstance(d, torch.Tensor):
            if d.data_ptr() != self.t.data_ptr():
                d.copy_(self.t)
        else:
            d[...] = self.t.to("cpu").numpy()


_DESIGNS = {}


def _design(dt, flo, fhi, dev):
    """(sos, zi, padlen) of bandpass_data's filter and their device copies, cached per (dt, band, device):
    the design is a pure function of its arguments (the reference redesigns it per call)."""
    key = (float(dt), float(flo), float(fhi), str(dev))
    if key not in _DESIGNS:
        sos = butter_bandpass_sos(dt, flo, fhi)
        zi = scipy.signal.sosfilt_zi(sos)
        _DESIGNS[key] = (sos, _padlen(sos), torch.from_numpy(np.ascontiguousarray(sos, dtype=np.float64)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(zi, dtype=np.float64)).to(dev))
    return _DESIGNS[key]


_PLANS = {}
SOS_MFMA_MAX_POLE = 0.999  # include/dvh.h DVH_SOS_MFMA_MAX_POLE


def _plan(key, n_t, sos, padlen, sos_t, zi_t, dev):
    """dvh_sosfiltfilt_plan's block operators of the design, per record length (formed once; the reference
    redesigns the same filter for every record); None (the block recursion) for a design whose largest pole
    radius exceeds SOS_MFMA_MAX_POLE, where the matrix form's rounding would pass 1e-10 of the output."""
    k = key + (int(n_t),)
    if k not in _PLANS:
        s64 = np.ascontiguousarray(sos, dtype=np.float64)
        if _lib.load().dvh_sos_pole_radius(s64.ctypes.data, len(sos)) > SOS_MFMA_MAX_POLE:
            _PLANS[k] = None
            return None
        plan = torch.empty(int(_lib.load().dvh_sosfiltfilt_plan_bytes(len(sos))) // 8, dtype=torch.float64, device=dev)
        _lib.call("dvh_sosfiltfilt_plan", _lib.ptr(sos_t), len(sos), _lib.ptr(zi_t), int(n_t), padlen, _lib.ptr(plan),
                  _lib.stream_of(dev))
        _PLANS[k] = plan
    return _PLANS[k]


def bandpass_inplace(data, dt, flo, fhi):
    v = _DeviceView(data)
    t = v.t
    n_t = t.shape[-1]
    rows = t.reshape(-1, n_t)
    dev = t.device
    sos, padlen, sos_t, zi_t = _design(dt, flo, fhi, dev)
    if n_t <= padlen:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {padlen}.")
    nbytes = int(_lib.load().dvh_sosfiltfilt_workspace(rows.shape[0], n_t, len(sos), padlen))
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    plan = _plan((float(dt), float(flo), float(fhi), str(dev)), n_t, sos, padlen, sos_t, zi_t, dev)
    _lib.call("dvh_sosfiltfilt_planned", _lib.ptr(rows), v.dtype, rows.shape[0], rows.stride(0), n_t, _lib.ptr(sos_t),
              len(sos), padlen, _lib.ptr(zi_t), None if plan is None else _lib.ptr(plan), _lib.ptr(work),
              _lib.stream_of(dev))
    v.write_back()
    return data


def mute_traj_table(x_axis, t_axis, veh_state_x, veh_state_t, offset=200, alpha=0.3, delta_x=20):
    """[T, 3] = (start, end, taper_start) per time sample and the taper, as the reference places them."""
    f = interp1d_extrap(veh_state_t, veh_state_x)
    car = f(np.asarray(t_axis, dtype=np.float64))
    x_axis = np.asarray(x_axis, dtype=np.float64)
    dx = x_axis[1] - x_axis[0]
    nx = x_axis.size
    n_samp = int(offset / dx)
    center = car - offset / 2 + delta_x
    c = np.argmax(x_axis[None, :] > center[:, None], axis=1)
    s = np.maximum(0, c - n_samp // 2)
    e = np.minimum(nx, c + n_samp // 2)
    ts = s + n_samp // 2 - c
    return np.stack([s, e, ts], axis=1).astype(np.int32), tukey(n_samp, alpha)


def taper_on_device(taper, dev):
    """The taper as a float64 device tensor.  An offset below one channel spacing gives an empty taper (every sample
    is zeroed, as the reference does); the kernel then reads none of it but refuses a null pointer, which is what an
    empty tensor has, so one unused entry stands in."""
    taper = np.ascontiguousarray(taper, dtype=np.float64)
    return torch.from_numpy(taper if taper.size else np.zeros(1)).to(dev)


def mute_along_traj(window, offset=200, alpha=0.3, delta_x=20):
    tab, taper = mute_traj_table(window.x_axis, window.t_axis, window.veh_state_x, window.veh_state_t, offset, alpha,
                                 delta_x)
    v = _DeviceView(window.data)
    n_ch, n_t = v.t.shape[-2], v.t.shape[-1]
    dev = v.t.device
    tab_t = torch.from_numpy(np.ascontiguousarray(tab)).to(dev)
    taper_t = taper_on_device(taper, dev)
    _lib.call("dvh_mute_traj", _lib.ptr(v.t), v.dtype, 1, n_ch * n_t, n_ch, n_t, _lib.ptr(tab_t), _lib.ptr(taper_t),
              _lib.stream_of(dev))
    v.write_back()


def mute_along_time(window, alpha=0.3):
    v = _DeviceView(window.data)
    n_t = v.t.shape[-1]
    dev = v.t.device
    taper_t = torch.from_numpy(np.ascontiguousarray(tukey(n_t, alpha), dtype=np.float64)).to(dev)
    _lib.call("dvh_mute_time", _lib.ptr(v.t), v.dtype, v.t.numel() // n_t, n_t, _lib.ptr(taper_t),
              _lib.stream_of(dev))
    v.write_back()


def surface_wave_preprocessing(data, dt, method="surface_wave", flo=1.2, fhi=30, impute_noise_traces=True,
                               noise_threshold=5, impute_empty_traces=True, return_indices=False, _phases=None):
    """TimeLapseImaging._preprocessing_for_surface_waves (apis/timeLapseImaging.py:51-71) of a
    continuous record [n_ch, n_t] -> ``data_for_imaging`` (a new array; the input is left as is):
    bandpass_data(flo, fhi) (dvh_sosfiltfilt), then find_noise_idx / impute_noisy_trace for an empty
    trace and for a noisy trace, then for method 'surface_wave' the per-trace L2 norm
    (dvh_trace_cleanup).  Host arrays in -> host arrays out in the record's dtype, like the
    reference's data.copy(): a float32 record is filtered in float64 and stored in float32, then
    imputed and normalised in float32 (other dtypes are imaged as float64); device tensors stay on the
    device.  With return_indices, also the (empty, noisy) trace indices imputed."""
    if method not in ("surface_wave", "xcorr"):
        raise AssertionError("method must be 'surface_wave' or 'xcorr'")
    on_device = isinstance(data, torch.Tensor) and data.is_cuda
    if on_device:
        t = data.clone()
    else:
        host = np.asarray(data.detach().cpu() if isinstance(data, torch.Tensor) else data)
        dt_keep = np.float32 if host.dtype == np.float32 else np.float64
        t = torch.from_numpy(np.array(host, dtype=dt_keep, copy=True)).to(default_device())
    if t.dim() != 2:
        raise ValueError("data must be [n_ch, n_t]")
    ev = (lambda k: _phases.setdefault(k, torch.cuda.Event(enable_timing=True)).record()) if _phases is not None \
        else (lambda k: None)  # timing hook (bench.py --workload prep)
    ev("bandpass0")
    bandpass_inplace(t, dt, flo, fhi)
    ev("bandpass1")
    dev = t.device
    stats = torch.empty(2 * t.shape[0], dtype=torch.float64, device=dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    flags = (1 if impute_empty_traces else 0) | (2 if impute_noise_traces else 0) | (4 if method == "surface_wave" else 0)
    _lib.call("dvh_trace_cleanup", _lib.ptr(t), 0 if t.dtype == torch.float32 else 1, t.shape[0], t.stride(0),
              t.shape[1], flags, float(noise_threshold), _lib.ptr(stats), _lib.ptr(idx), _lib.stream_of(dev))
    ev("cleanup1")
    out = t if on_device else t.cpu().numpy()
    if return_indices:
        return out, tuple(int(i) for i in idx.cpu())
    return out


_RESAMPLERS = {}


def _resampler(up, down, dev):
    """(up, down, half_len, h on the device) of scipy.signal.resample_poly(x, up, down)'s default filter, cached per
    (up, down, device): the ratio reduced by its gcd, h = firwin(2 half_len + 1, 1 / max(up, down),
    window=('kaiser', 5.0)) * up with half_len = 10 max(up, down); a 1 / 1 ratio is the identity (h = [1])."""
    key = (int(up), int(down), str(dev))
    if key not in _RESAMPLERS:
        up, down = int(up), int(down)
        if up < 1 or down < 1:
            raise ValueError("up and down must be >= 1")
        g = int(np.gcd(up, down))
        up, down = up // g, down // g
        if up == down == 1:
            half_len, h = 0, np.ones(1)
        else:
            half_len = 10 * max(up, down)
            h = scipy.signal.firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        _RESAMPLERS[key] = (up, down, half_len, torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64)).to(dev))
    return _RESAMPLERS[key]


TRACKING_DX = 8.16  # channel spacing [m] of the record the tracking grid is resampled from (apis/timeLapseImaging.py:92)


def tracking_preprocessing(data, dt, x0_channel, *, flo=0.08, fhi=1, flo_space=0.006, fhi_space=0.04, subsamp_factor=5,
                           noise_level=10, channel0=400, up=204, down=25, return_info=False, _phases=None):
    """TimeLapseImaging._preprocess_for_tracking (apis/timeLapseImaging.py:74-102) of a continuous record
    [n_ch, n_t] with first channel number ``x0_channel`` -> (data_for_tracking [ceil(n_ch up / down),
    ceil(n_t / subsamp_factor)] float64, dist_along_fiber_tracking, subsamp_factor): the tracking time axis is
    ``t_axis[::subsamp_factor]``.  The input is left as is; a host array gives a host array, a device tensor a device
    tensor (the distance axis is a host array either way, computed with the reference's expression).  On the device,
    in the reference's order:
      copy to float64 (a float32 record is promoted here; the reference keeps float32 up to resample_poly, whose
        output is float64 -- the tracking grid is float64 throughout in this project)
      means = median(|x|) per trace, traces with means > noise_level *= 0            dvh_median_abs_gate
      find_noise_idx(30, empty_tr=True) / impute_noisy_trace                          dvh_trace_cleanup (flags 1)
      bandpass_data(dt, flo, fhi)                                                     dvh_sosfiltfilt_planned
      resample_poly(x[:, ::subsamp_factor], up, down), written transposed             dvh_resample_rows_t
      bandpass_data_space(dist, flo_space, fhi_space) on the transposed rows (skipped when both are -1)
      transpose back                                                                  dvh_transpose_f64
    With return_info, also a dict: ``median`` per trace, the ``gated`` trace indices, the ``imputed`` trace index."""
    on_device = isinstance(data, torch.Tensor) and data.is_cuda
    if on_device:
        t = data.to(torch.float64, copy=True).contiguous()
    else:
        host = np.asarray(data.detach().cpu() if isinstance(data, torch.Tensor) else data)
        t = torch.from_numpy(np.array(host, dtype=np.float64, copy=True)).to(default_device())
    if t.dim() != 2:
        raise ValueError("data must be [n_ch, n_t]")
    subsamp_factor = int(subsamp_factor)
    if subsamp_factor < 1:
        raise ValueError("subsamp_factor must be >= 1")
    dev = t.device
    n_ch, n_t = t.shape
    up_r, down_r, half_len, h_t = _resampler(up, down, dev)
    n_out = -(-n_ch * up_r // down_r)
    n_t_out = -(-n_t // subsamp_factor)
    space = not (flo_space == -1 and fhi_space == -1)
    dist = np.arange(n_out) + (x0_channel - channel0) * TRACKING_DX
    padlen = _design(dt, flo, fhi, dev)[1]  # 63 for every order-10 band-pass: the spatial filter's as well
    if n_t <= padlen or (space and n_out <= padlen):
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {padlen}.")
    ev = (lambda k: _phases.setdefault(k, torch.cuda.Event(enable_timing=True)).record()) if _phases is not None \
        else (lambda k: None)  # timing hook (tools/bench_tracking_prep.py)
    st = _lib.stream_of(dev)
    med = torch.empty(n_ch, dtype=torch.float64, device=dev)
    gated = torch.empty(n_ch, dtype=torch.int32, device=dev)
    stats = torch.empty(2 * n_ch, dtype=torch.float64, device=dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    ev("start")
    _lib.call("dvh_median_abs_gate", _lib.ptr(t), 1, n_ch, t.stride(0), n_t, float(noise_level), _lib.ptr(med),
              _lib.ptr(gated), st)
    ev("gate")
    _lib.call("dvh_trace_cleanup", _lib.ptr(t), 1, n_ch, t.stride(0), n_t, 1, 30.0, _lib.ptr(stats), _lib.ptr(idx), st)
    ev("cleanup")
    bandpass_inplace(t, dt, flo, fhi)
    ev("time_filter")
    rs = torch.empty((n_t_out, n_out), dtype=torch.float64, device=dev)
    _lib.call("dvh_resample_rows_t", _lib.ptr(t), 1, n_ch, t.stride(0), subsamp_factor, n_t_out, _lib.ptr(h_t),
              half_len, up_r, down_r, _lib.ptr(rs), rs.stride(0), n_out, st)
    ev("resample")
    if space:
        bandpass_inplace(rs, dist[1] - dist[0], flo_space, fhi_space)  # the axis' own step, as the reference takes it
    ev("space_filter")
    out = torch.empty((n_out, n_t_out), dtype=torch.float64, device=dev)
    _lib.call("dvh_transpose_f64", _lib.ptr(rs), n_t_out, n_out, rs.stride(0), _lib.ptr(out), out.stride(0), st)
    ev("transpose")
    res = (out if on_device else out.cpu().numpy(), dist, subsamp_factor)
    if return_info:
        return res + (dict(median=med.cpu().numpy(), gated=np.flatnonzero(gated.cpu().numpy()),
                           imputed=int(idx[0].cpu())),)
    return res


_SAVGOL_OPS = {}
_SAVGOL_DEV = {}


def savgol_interp_operator(window_length, polyorder):
    """scipy.signal.savgol_filter(x, window_length, polyorder) (mode='interp', along the last axis) as three linear
    maps (h, el, er), cached per design: ``h = savgol_coeffs(W, P)[::-1]`` for the interior
    (y[t] = sum_j h[j] x[t - half + j]) and the first / last ``half`` rows of the W x W matrix that savgol_filter
    itself makes of the identity, one column at a time: el maps the first W samples onto the first half outputs, er
    the last W onto the last half.  SciPy is the coefficient designer: at (21, 15) its taps are not the exact
    least-squares ones (its Vandermonde solve is ill-conditioned; they are not even symmetric), and the reference's
    output is defined by them."""
    W, P = int(window_length), int(polyorder)
    key = (W, P)
    if key not in _SAVGOL_OPS:
        if W % 2 == 0 or W < 3:
            raise ValueError("window_length must be odd and >= 3")
        if P >= W:
            raise ValueError("polyorder must be less than window_length.")
        half = W // 2
        h = np.ascontiguousarray(scipy.signal.savgol_coeffs(W, P)[::-1], dtype=np.float64)
        eye = np.eye(W)
        m = np.stack([scipy.signal.savgol_filter(eye[:, c], W, P) for c in range(W)], axis=1)
        _SAVGOL_OPS[key] = (h, np.ascontiguousarray(m[:half]), np.ascontiguousarray(m[W - half:]))
    return _SAVGOL_OPS[key]


def _savgol_device(window_length, polyorder, dev):
    key = (int(window_length), int(polyorder), str(dev))
    if key not in _SAVGOL_DEV:
        _SAVGOL_DEV[key] = tuple(torch.from_numpy(a).to(dev) for a in savgol_interp_operator(window_length, polyorder))
    return _SAVGOL_DEV[key]


def savgol_smooth(data, window_length=21, polyorder=15, divisor=1.0):
    """savgol_filter(data, window_length, polyorder) along time followed by ``/= divisor``: what
    ImagingIO.__getitem__ (modules/imaging_IO.py:44-46) does to a record, in one pass of dvh_savgol_rows.  A host
    array gives a host array, a device tensor a new device tensor (the input is left as is).  float32 and float64
    are kept (float32: float64 sums rounded once, then divided in float32, as SciPy and numpy do); any other dtype
    is converted to float64 on the host first, as SciPy does."""
    on_device = isinstance(data, torch.Tensor) and data.is_cuda
    if on_device:
        if data.dtype not in (torch.float32, torch.float64):
            raise TypeError("a device record must be float32 or float64")
        shape = tuple(data.shape)
    else:
        host = np.asarray(data.detach().cpu() if isinstance(data, torch.Tensor) else data)
        if host.dtype not in (np.float32, np.float64):
            host = host.astype(np.float64)
        shape = host.shape
    if len(shape) < 1 or shape[-1] < int(window_length):
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    t = data if on_device else torch.from_numpy(np.ascontiguousarray(host)).to(default_device())
    n_t = shape[-1]
    rows = t.reshape(-1, n_t)
    if rows.stride(-1) != 1 or (rows.shape[0] > 1 and rows.stride(0) < n_t):  # e.g. an expanded row dimension
        rows = rows.contiguous()
    dev = rows.device
    h_t, el_t, er_t = _savgol_device(window_length, polyorder, dev)
    out = torch.empty((rows.shape[0], n_t), dtype=rows.dtype, device=dev)
    if rows.shape[0]:
        _lib.call("dvh_savgol_rows", _lib.ptr(rows), 0 if rows.dtype == torch.float32 else 1, rows.shape[0],
                  rows.stride(0) if rows.shape[0] > 1 else n_t, n_t, _lib.ptr(h_t), int(window_length), _lib.ptr(el_t), _lib.ptr(er_t),
                  float(divisor), _lib.ptr(out), out.stride(0), _lib.stream_of(dev))
    out = out.reshape(shape)
    return out if on_device else out.cpu().numpy()
