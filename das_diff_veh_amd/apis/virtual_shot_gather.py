"""VirtualShotGather — drop-in for apis/virtual_shot_gather.py:183-270 of the reference.

The constructor signature, keyword defaults (those of construct_shot_gather, :165-166), attributes
(``XCF_out`` float64 [R, w], ``x_axis``, ``t_axis``, ``disp``, ``window``) and the stacking
arithmetic (``__add__``, ``__radd__(0)``, ``__truediv__``) are the reference's; the correlation
itself runs in the HIP kernels of libdvh (das_diff_veh_amd/csrc/dvh_vsg.hip).  Errors the reference
raises for unusable inputs (the dt == 0.004 window-length mismatch, out-of-order gather geometry)
are raised as ValueError before any launch.
"""
from __future__ import annotations

import copy
import os

import numpy as np

from .. import engine
from ..plan import VsgParams

_POSITIONAL = ("start_x", "end_x", "pivot", "wlen", "norm", "norm_amp", "time_window_to_xcorr", "delta_t")


def vsg_params(include_other_side=False, *args, **kwargs):
    """construct_shot_gather(window, start_x=530, end_x=680, pivot=635, wlen=2, norm=True, norm_amp=True,
    time_window_to_xcorr=4, delta_t=1) keyword surface -> VsgParams."""
    if len(args) > len(_POSITIONAL):
        raise TypeError("too many positional arguments")
    kw = dict(zip(_POSITIONAL, args))
    for k, v in kwargs.items():
        if k in kw:
            raise TypeError(f"got multiple values for argument '{k}'")
        if k not in _POSITIONAL:
            raise TypeError(f"construct_shot_gather() got an unexpected keyword argument '{k}'")
        kw[k] = v
    return VsgParams(include_other_side=bool(include_other_side), **kw)


def _device_rows_f32(XCF_out):
    """A gather [R, w] as a float32 device tensor (the kernels' input type; XCF_out itself is float64)."""
    import torch

    from ..device import default_device
    if isinstance(XCF_out, torch.Tensor):
        return XCF_out.to(device=default_device(), dtype=torch.float32)
    return torch.from_numpy(np.ascontiguousarray(XCF_out, dtype=np.float32)).to(default_device())


def psd_vs_offset(XCF_out, x_axis, t_axis, fhi=20, pclip=98, log_scale=False, x_max=200, x_min=0, vmax=None,
                  vmin=None):
    """The data of plot_psd_vs_offset (apis/virtual_shot_gather.py:45-89 of the reference) without the figure:
    welch(XCF_out, fs, nperseg=256, nfft=1024) per gather row on the device (dvh_welch_rows), then the reference's
    host steps on the small result.  Returns (spec, freq[:fhi_idx], x_axis[min_idx:max_idx], vmax, vmin), ``spec``
    being the array the reference hands to imshow before ``.T``.
      fs         int(1 / (t_axis[1] - t_axis[0])) in float64: 250 on a w = 500 axis, 249 on a w = 499 one
      fhi_idx    first bin >= fhi; 0 when there is none, and the result is then empty (the reference's np.percentile
                 raises on it; here vmax / vmin are NaN unless given)
      vmax, vmin the pclip / 100 - pclip percentiles over all rows, after the optional 10 log10 and before the offset
                 crop; a given value of 0 counts as not given (``if not vmax``)
      rows       [min_idx, max_idx) of the nearest offsets to x_min / x_max; a descending x_axis is negated first"""
    from ..spectra import welch_rows
    x_axis, t_axis = np.asarray(x_axis), np.asarray(t_axis)
    if x_axis[0] > x_axis[-1]:
        x_axis = x_axis * -1
    dt = t_axis[1] - t_axis[0]
    fs = int(1 / dt)
    freq, pxx = welch_rows(_device_rows_f32(XCF_out), fs, nperseg=256, nfft=1024)
    fhi_idx = int(np.argmax(freq >= fhi))
    spec = pxx[:, :fhi_idx].to("cpu").numpy()
    if log_scale:
        spec = 10 * np.log10(spec)
    if not vmax:
        vmax = np.percentile(spec, pclip) if spec.size else np.nan
    if not vmin:
        vmin = np.percentile(spec, 100 - pclip) if spec.size else np.nan
    x_max_idx = np.abs(x_max - x_axis).argmin()
    x_min_idx = np.abs(x_min - x_axis).argmin()
    min_idx, max_idx = min(x_max_idx, x_min_idx), max(x_max_idx, x_min_idx)
    return spec[min_idx:max_idx], freq[:fhi_idx], x_axis[min_idx:max_idx], vmax, vmin


def spectrum_vs_offset(XCF_out, x_axis, t_axis, fhi=20):
    """The data of plot_spectrum_vs_offset (apis/virtual_shot_gather.py:92-109): (|fft(XCF_out)[:, :fhi_idx]|,
    freq[:fhi_idx]) with freq = fftfreq(w, dt).  Only the first fhi_idx bins are formed, by dvh_disp_tdft in float64
    from the w-point twiddles (w = 500 or the prime 499 alike); the magnitude is taken on the downloaded array."""
    import torch

    from .. import _lib
    t_axis = np.asarray(t_axis)
    data = _device_rows_f32(XCF_out).contiguous()
    R, nt = data.shape
    dt = t_axis[1] - t_axis[0]
    freq = np.fft.fftfreq(nt, d=dt)
    fhi_idx = int(np.argmax(freq >= fhi))
    if fhi_idx == 0:
        return np.zeros((R, 0)), freq[:0]
    ang = 2.0 * np.pi * ((np.outer(np.arange(nt), np.arange(fhi_idx)) % nt) / nt)
    wt = np.empty((nt, 2 * fhi_idx))
    wt[:, 0::2] = np.cos(ang)
    wt[:, 1::2] = -np.sin(ang)
    wt_t = torch.from_numpy(wt).to(data.device)
    D = torch.empty((R, 2 * fhi_idx), dtype=torch.float64, device=data.device)
    _lib.call("dvh_disp_tdft", _lib.ptr(data), R * nt, nt, 1, R, nt, _lib.ptr(wt_t), fhi_idx, None, _lib.ptr(D),
              _lib.stream_of(data.device))
    d = D.to("cpu").numpy()
    return np.hypot(d[:, 0::2], d[:, 1::2]), freq[:fhi_idx]


class VirtualShotGather:
    def __init__(self, window, compute_xcorr=True, disp=None, include_other_side=False, *args, **kwargs):
        self.window = window
        self.disp = disp
        if compute_xcorr:
            prm = vsg_params(include_other_side, *args, **kwargs)
            res, geoms = engine.gathers([window], prm)
            self.XCF_out, self.x_axis, self.t_axis = res[0], geoms[0].gather_x_axis, geoms[0].gather_t_axis

    @classmethod
    def _from_arrays(cls, window, xcf, x_axis, t_axis):
        obj = cls(window=window, compute_xcorr=False)
        obj.XCF_out, obj.x_axis, obj.t_axis = xcf, x_axis, t_axis
        return obj

    def __add__(self, other):
        sum_ = copy.deepcopy(self)
        length = min(self.XCF_out.shape[-1], other.XCF_out.shape[-1])
        sum_.XCF_out[:, :length] += other.XCF_out[:, :length]
        return sum_

    def __radd__(self, other):
        if other == 0:
            return self
        return self.__add__(other)

    def __truediv__(self, other):
        new_obj = copy.deepcopy(self)
        new_obj.XCF_out /= other
        return new_obj

    @classmethod
    def get_VirtualShotGather_obj(cls, fdir, fname):
        new_obj = cls(window=None, compute_xcorr=False)
        f = np.load(os.path.join(fdir, fname), allow_pickle=False)
        new_obj.XCF_out, new_obj.x_axis, new_obj.t_axis = f["XCF_out"], f["x_axis"], f["t_axis"]
        return new_obj

    def save_to_npz(self, fname, fdir, **kwargs):
        np.savez(os.path.join(fdir, fname), XCF_out=self.XCF_out, x_axis=self.x_axis, t_axis=self.t_axis, **kwargs)

    def compute_disp_image(self, freqs=np.arange(0.8, 25, 0.1), vels=np.arange(200, 1200), norm=False,
                           start_x=None, end_x=None, transform="fk"):
        """apis/virtual_shot_gather.py:247-258: nearest-offset channel slice -> Dispersion(dx=8.16).
        ``transform`` is Dispersion's: "fk" (map_fv) or "slant" (the phase-shift transform on the sliced rows)."""
        from ..modules.utils import Dispersion
        if start_x is None:
            start_x = self.x_axis[0]
        if end_x is None:
            end_x = self.x_axis[-1]
        s = np.abs(self.x_axis - start_x).argmin()
        e = np.abs(self.x_axis - end_x).argmin()
        self.disp = Dispersion(self.XCF_out[s:e + 1], 8.16, self.t_axis[1] - self.t_axis[0], freqs=freqs, vels=vels,
                               norm=norm, transform=transform)

    def save_disp_to_npz(self, *args, **kwargs):
        assert self.disp, "please run obj.compute_disp_image() first"
        self.disp.save_to_npz(*args, **kwargs)

    def norm(self):
        self.XCF_out /= np.linalg.norm(self.XCF_out, axis=-1, keepdims=True)

    def plot_image(self, *args, **kwargs):
        raise NotImplementedError("plotting is outside the accelerated path; use the reference's plot_xcorr on "
                                  "obj.XCF_out / obj.x_axis / obj.t_axis")

    plot_disp = plot_image

    def spec_vs_offset(self, psd=True, pclip=98, x_max=100, x_min=-100, log_scale=False, vmin=None, vmax=None):
        """The data of plot_spec_vs_offset (apis/virtual_shot_gather.py:219-229), dispatched as the reference does:
        psd=True -> psd_vs_offset with these keywords, psd=False -> spectrum_vs_offset with its defaults."""
        if not psd:
            return spectrum_vs_offset(self.XCF_out, self.x_axis, self.t_axis)
        return psd_vs_offset(self.XCF_out, self.x_axis, self.t_axis, pclip=pclip, x_max=x_max, x_min=x_min,
                             log_scale=log_scale, vmax=vmax, vmin=vmin)

    def plot_spec_vs_offset(self, *args, **kwargs):
        raise NotImplementedError("plotting is outside the accelerated path; obj.spec_vs_offset(...) returns the "
                                  "arrays the reference's plot_psd_vs_offset / plot_spectrum_vs_offset draw")
