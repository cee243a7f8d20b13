"""Hot-path functions of modules/utils.py of the reference, served by the HIP kernels.

  fk            modules/utils.py:236-248  -> full |FK| grid from the dispersion GEMMs
  map_fv        modules/utils.py:457-475  -> dvh_disp_tdft / dvh_disp_fk / dvh_disp_fv
  map_fv_FD_slant_stack modules/utils.py:429-454 -> dvh_disp_row_l1 / dvh_disp_tdft / dvh_disp_slant
  Dispersion    modules/utils.py:383-426  (same constructor, attributes, npz format, arithmetic; transform="slant"
                stores the phase-shift image instead of map_fv's)
  bandpass_data modules/utils.py:179-189  -> dvh_sosfiltfilt (zero-phase order-10 Butterworth)
  extract_ridge_ref_idx modules/utils.py:621-678 -> dvh_ridge (one wave per ridge)
  win_avg_psd   modules/utils.py:715-728  -> dvh_welch_rows (one launch per window shape, das_diff_veh_amd.spectra)
  disp_curve_stats  the statistics of plot_disp_curves (:680-713), without the figure
  _cut_taper, _read_das_npz modules/utils.py:87-113 (host: the record file, its channel and taper cut; ImagingIO of
                modules/imaging_IO.py smooths and scales the result on the device)
Host arrays in, host arrays out, like the reference; device tensors are accepted too.
"""
from __future__ import annotations

import copy
import os

import numpy as np
import torch

from ..device import default_device


def _as_device_batch(data, device=None):
    device = device or default_device()
    if isinstance(data, torch.Tensor):
        t = data.to(device=device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(data, dtype=np.float32))).to(device)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    return t.contiguous() if t.stride(-1) != 1 else t


def _first_at_or_above(axis, value):
    """Index of the first axis entry >= value (0 when there is none, as np.argmax of an all-False mask)."""
    return int(np.argmax(np.asarray(axis) >= value))


def _cut_taper(data, t_axis):
    """Trim the acquisition taper (modules/utils.py:87-92 of the reference): the sample whose time is nearest 0 sits
    ``m`` samples into the record, and ``m`` samples leave at both ends of the data and of the time axis."""
    m = int(np.argmin(np.abs(t_axis)))
    keep = slice(m, data.shape[-1] - m)
    return data[:, keep], t_axis[keep]


def _read_das_npz(fname, **kwargs):
    """One record file (keys data [n_ch, n_t], x_axis, t_axis) -> (data, x_axis, t_axis) cut as the reference's
    reader cuts it (modules/utils.py:94-113).  Host work only: file reading and index arithmetic.
      ch1, ch2    channel numbers; rows from the first x_axis >= ch1 up to, not including, the first x_axis >= ch2
                  (defaults: the axis' first and last entry, so the last channel is dropped)
      cut_taper   (default True) apply _cut_taper
    A file that cannot be opened raises Exception("fname: <path>")."""
    try:
        npz = np.load(fname)
    except Exception:
        raise Exception(f"fname: {fname}")
    x_axis, t_axis = npz["x_axis"], npz["t_axis"]
    rows = slice(_first_at_or_above(x_axis, kwargs.get("ch1", x_axis[0])),
                 _first_at_or_above(x_axis, kwargs.get("ch2", x_axis[-1])))
    data = npz["data"][rows]
    if kwargs.get("cut_taper", True):
        data, t_axis = _cut_taper(data, t_axis)
    return data, x_axis[rows], t_axis


_PLANS = {}


def disp_plan(nch, nt, dx, dt, freqs, vels, full_grid=False):
    from ..disp import DispPlan
    freqs = np.asarray(freqs, dtype=np.float64)
    vels = np.asarray(vels, dtype=np.float64)
    key = (nch, nt, float(dx), float(dt), freqs.tobytes(), vels.tobytes(), full_grid)
    if key not in _PLANS:
        if len(_PLANS) > 64:
            _PLANS.clear()
        _PLANS[key] = DispPlan(nch, nt, dx, dt, freqs, vels, full_grid=full_grid)
    return _PLANS[key]


def fk(data, dx, dt):
    """|fftshift(fft2(data, s=[nk, nf]))|, fft_f, fft_k (float32 magnitudes from the MFMA GEMMs)."""
    from ..disp import fk_grid
    t = _as_device_batch(data)
    nch, nt = t.shape[1], t.shape[2]
    plan = disp_plan(nch, nt, dx, dt, [1.0] * 25, [1.0], full_grid=True)
    g = fk_grid(t, plan)[0].to("cpu").numpy()
    return g, plan.fft_f, plan.fft_k


def map_fv(data, dx, dt, freqs, vels, norm=False):
    """f-v image [Nvel, Nfreq] (float32, rows in sorted-query order like interp2d)."""
    from ..disp import fv_maps
    t = _as_device_batch(data)
    plan = disp_plan(t.shape[1], t.shape[2], dx, dt, freqs, vels)
    return fv_maps(t, plan, norm=norm)[0].to("cpu").numpy()


def slant_plan(nch, nt, dx, dt, freqs, vels, rows=(6, 25)):
    from ..disp import SlantPlan
    freqs = np.asarray(freqs, dtype=np.float64)
    vels = np.asarray(vels, dtype=np.float64)
    key = ("slant", nch, nt, float(dx), float(dt), freqs.tobytes(), vels.tobytes(), tuple(rows))
    if key not in _PLANS:
        if len(_PLANS) > 64:
            _PLANS.clear()
        _PLANS[key] = SlantPlan(nch, nt, dx, dt, freqs, vels, rows=rows)
    return _PLANS[key]


def map_fv_FD_slant_stack(data, dx, dt, freqs, vels, norm=True):
    """Phase-shift (frequency-domain slant-stack) image [Nvel, Nfreq] of rows [6:25] of the gather, rows in the
    caller's velocity order: float64 holding the float32 values the device stores (dvh_disp_slant).  A velocity of 0
    raises ValueError, as in the reference."""
    from ..disp import slant_maps
    t = _as_device_batch(data)
    plan = slant_plan(t.shape[1], t.shape[2], dx, dt, freqs, vels)
    return slant_maps(t, plan, norm=norm)[0].to("cpu").numpy().astype(np.float64)


class Dispersion:
    """``transform`` selects the image: "fk" (default) is map_fv; "slant" is the phase-shift transform of
    map_fv_FD_slant_stack over all rows of ``data``, stored with rows in descending velocity (map_fv's row
    convention), so the ridge walk and save_to_npz consume it as they consume an f-k image."""

    def __init__(self, data, dx, dt, freqs, vels, norm=False, compute_fv=True, transform="fk"):
        if transform not in ("fk", "slant"):
            raise ValueError(f"transform must be 'fk' or 'slant', not {transform!r}")
        self.data = data
        self.dx = dx
        self.dt = dt
        self.freqs = freqs
        self.vels = vels
        self.norm = norm
        self.transform = transform
        if compute_fv:
            self._map_fv()

    def save_to_npz(self, fname, fdir="./"):
        np.savez(os.path.join(fdir, fname), freqs=self.freqs, vels=self.vels, fv_map=self.fv_map)

    @classmethod
    def get_dispersion_obj(cls, fname, fdir="./"):
        f = np.load(os.path.join(fdir, fname), allow_pickle=False)
        obj = Dispersion(data=None, dx=None, dt=None, freqs=f["freqs"], vels=f["vels"], compute_fv=False)
        obj.fv_map = f["fv_map"]
        return obj

    def _map_fv(self):
        if self.transform == "slant":
            from ..disp import slant_maps
            t = _as_device_batch(self.data)
            plan = slant_plan(t.shape[1], t.shape[2], self.dx, self.dt, self.freqs,
                              np.sort(np.asarray(self.vels, dtype=np.float64))[::-1], rows=(0, t.shape[1]))
            self.fv_map = slant_maps(t, plan, norm=self.norm)[0].to("cpu").numpy()
            return
        self.fv_map = map_fv(self.data, self.dx, self.dt, freqs=self.freqs, vels=self.vels, norm=self.norm)

    def plot_image(self, *args, **kwargs):
        raise NotImplementedError("plotting is outside the accelerated path; use the reference's plot_fv_map on "
                                  "obj.fv_map / obj.freqs / obj.vels")

    def __add__(self, other):
        sum_ = Dispersion(self.data, self.dx, self.dt, self.freqs, self.vels, compute_fv=False)
        sum_.fv_map = self.fv_map + other.fv_map
        return sum_

    def __radd__(self, other):
        if other == 0:
            return self
        return self.__add__(other)

    def __truediv__(self, other):
        div_ = copy.deepcopy(self)
        div_.fv_map /= other
        return div_


def bandpass_data(data, dt, flo, fhi):
    """In-place zero-phase Butterworth bandpass (order 10, SOS) along time, on device."""
    from ..preprocess import bandpass_inplace
    bandpass_inplace(data, dt, flo, fhi)


def extract_ridge_ref_idx(freq, vel, fv_map, ref_freq_idx=None, sigma=25, vel_max=400, ref_vel=None):
    """modules/utils.py:621-678 (fv_map [Nvel, Nfreq] with rows in vel[::-1] order), walked on the
    device by dvh_ridge (das_diff_veh_amd.bootstrap.ridges)."""
    import torch

    from ..bootstrap import ridges
    fv = torch.as_tensor(np.ascontiguousarray(fv_map, dtype=np.float32), device=default_device())[None]
    freq = np.asarray(freq, dtype=np.float64)
    out = ridges(fv, freq, vel, freq[0], np.nextafter(freq[-1], np.inf), ref_freq_idx=ref_freq_idx, sigma=sigma,
                 vel_max=vel_max, ref_vel=ref_vel)[0]
    return out


def win_avg_psd(win_spectrum, fs, nperseg=2048):
    """modules/utils.py:715-728: (f, Pxx_avg, Pxxs) in float64, Pxxs[i] the mean over window i's own rows of
    scipy.signal.welch(row, fs, nperseg=nperseg) and Pxx_avg = Pxxs.mean(0).  Windows are batched by shape, one
    float32 device batch and one dvh_welch_rows launch per shape (the rows' own spectra are never stored); ``data``
    may be a host array or a device tensor.  As in the reference an empty list raises IndexError, windows whose
    spectra differ in length raise ValueError, and an nperseg above the window length is clipped with SciPy's warning."""
    from ..device import to_device_f32
    from ..spectra import welch_plan, welch_rows
    shapes = [tuple(w.data.shape) for w in win_spectrum]
    if not shapes:
        raise IndexError("list index out of range")
    if any(len(s) != 2 or s[0] < 1 for s in shapes):
        raise ValueError("every window's data must be [channels >= 1, samples]")
    plans = {n_t: welch_plan(n_t, fs, nperseg) for n_t in dict.fromkeys(s[1] for s in shapes)}
    bins = plans[shapes[0][1]].bins
    for s in shapes:
        if plans[s[1]].bins != bins:
            raise ValueError(f"could not broadcast input array from shape ({plans[s[1]].bins},) into shape ({bins},)")
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)
    Pxxs = np.zeros((len(shapes), bins))
    for s, idx in groups.items():
        batch = to_device_f32([win_spectrum[i].data for i in idx])
        _, out = welch_rows(batch, fs, plan=plans[s[1]])
        Pxxs[idx] = out.to("cpu").numpy()
    return plans[shapes[-1][1]].freqs, np.mean(Pxxs, axis=0), Pxxs


def disp_curve_stats(freqs, freq_lb, freq_up, ridge_vels):
    """The statistics of plot_disp_curves (modules/utils.py:680-713) without the figure:
    per mode the mean, range (max - min) and std over resamples of the ridge velocities."""
    means, ranges, stds = [], [], []
    for i in range(len(ridge_vels)):
        rv = np.array([d for d in ridge_vels[i]], dtype=np.float64)
        means.append(np.mean(rv, axis=0))
        stds.append(np.std(rv, axis=0))
        ranges.append(np.max(rv, axis=0) - np.min(rv, axis=0))
    return means, ranges, stds
