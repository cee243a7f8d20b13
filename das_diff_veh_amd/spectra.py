"""Welch power spectra on the device (dvh_welch_rows, csrc/dvh_psd.hip): scipy.signal.welch with SciPy's defaults.

``welch_plan`` is the host side in float64 (the nperseg clip with SciPy's warning, the segment count, the window
table, the scale and the frequency axis); ``welch_rows`` runs the kernel on a float32 device tensor.  The callers are
``modules.utils.win_avg_psd`` and ``apis.virtual_shot_gather.psd_vs_offset``.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import scipy.signal
import torch

from . import _lib

FAST_NFFT = (256, 512, 1024, 2048, 4096)  # one wave per segment; any other length takes the direct float64 form


@dataclass
class WelchPlan:
    n_t: int
    fs: float
    nperseg: int
    nfft: int
    noverlap: int
    step: int
    nseg: int
    win: np.ndarray    # [nperseg] float64, scipy.signal.get_window('hann', nperseg)
    scale: float       # 1 / (fs sum win^2)
    freqs: np.ndarray  # [nfft // 2 + 1] float64

    @property
    def bins(self):
        return self.nfft // 2 + 1

    @property
    def fast(self):
        return self.nfft in FAST_NFFT


def welch_plan(n_t, fs, nperseg=256, nfft=None):
    """The quantities scipy.signal.welch(x, fs, nperseg=nperseg, nfft=nfft) derives from a row of n_t samples.  An
    nperseg above n_t becomes n_t with SciPy's UserWarning (and nfft then follows it unless it was given)."""
    n_t, nperseg = int(n_t), int(nperseg)
    if n_t < 1 or nperseg < 1:
        raise ValueError("nperseg must be a positive integer")
    if nperseg > n_t:
        warnings.warn(f"nperseg = {nperseg:d} is greater than input length  = {n_t:d}, using nperseg = {n_t:d}",
                      UserWarning, stacklevel=3)
        nperseg = n_t
    nfft = nperseg if nfft is None else int(nfft)
    if nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    noverlap = nperseg // 2
    step = nperseg - noverlap
    win = np.ascontiguousarray(scipy.signal.get_window("hann", nperseg), dtype=np.float64)
    return WelchPlan(n_t, float(fs), nperseg, nfft, noverlap, step, (n_t - noverlap) // step, win,
                     1.0 / (float(fs) * float((win * win).sum())), np.fft.rfftfreq(nfft, 1.0 / float(fs)))


_TABLES = {}


def _tables(plan: WelchPlan, device):
    """(win, tab) on the device; tab = (cos, -sin)(2 pi m / nfft) for the direct form, None for the fast one."""
    key = (plan.nperseg, plan.nfft, str(device))
    if key not in _TABLES:
        if len(_TABLES) > 16:
            _TABLES.clear()
        tab = None
        if not plan.fast:
            ang = 2.0 * np.pi * (np.arange(plan.nfft) / plan.nfft)
            tab = torch.from_numpy(np.stack([np.cos(ang), -np.sin(ang)], axis=1)).to(device)
        _TABLES[key] = (torch.from_numpy(plan.win).to(device), tab)
    return _TABLES[key]


def welch_rows(x, fs, nperseg=256, nfft=None, plan=None, out=None):
    """Power spectral densities of the rows of a float32 device tensor.

    x [R, n_t]: one spectrum per row, [R, bins] float64.  x [G, C, n_t]: per group the mean of its C rows' spectra,
    [G, bins] float64 (win_avg_psd's per-window spectrum).  Returns (freqs as a host array, the device tensor)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("x must be a float32 device tensor (no CPU fallback)")
    if x.dim() not in (2, 3):
        raise ValueError("x must be [rows, n_t] or [groups, rows, n_t]")
    if plan is None:
        plan = welch_plan(x.shape[-1], fs, nperseg, nfft)
    elif plan.n_t != x.shape[-1]:
        raise ValueError("the plan is for rows of another length")
    if x.dim() == 2:
        x = x.unsqueeze(1)
    G, C, n_t = x.shape
    if x.stride(2) != 1 or (C > 1 and x.stride(1) < n_t) or (G > 1 and x.stride(0) < (C - 1) * x.stride(1) + n_t):
        x = x.contiguous()
    dev = x.device
    win, tab = _tables(plan, dev)
    if out is None:
        out = torch.empty((G, plan.bins), dtype=torch.float64, device=dev)
    elif out.shape != (G, plan.bins) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float64 device tensor [groups, bins]")
    nbytes = _lib.load().dvh_welch_rows_workspace(G, C, plan.nfft)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    _lib.call("dvh_welch_rows", _lib.ptr(x), G, x.stride(0), C, x.stride(1), n_t, _lib.ptr(win), plan.nperseg,
              plan.nfft, plan.scale, _lib.ptr(tab), _lib.ptr(out), _lib.ptr(ws), _lib.stream_of(dev))
    return plan.freqs, out
