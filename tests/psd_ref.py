"""NumPy restatement, in float64, of the reference's spectral analysis: scipy.signal.welch with SciPy's defaults as
win_avg_psd (modules/utils.py:715-728) and plot_psd_vs_offset (apis/virtual_shot_gather.py:45-89) call it, and
plot_spectrum_vs_offset (:92-109).  SciPy only designs the window (get_window); everything else is plain NumPy.

  window    periodic Hann of length P; noverlap = P // 2, step = P - noverlap, nseg = (n_t - noverlap) // step, the tail
            past the last full segment ignored
  segment   minus its own mean, times the window, rFFT of length F (zero padded), re^2 + im^2
  row       mean over segments, times 1 / (fs sum win^2), every bin doubled except DC and, for even F, Nyquist
  clip      P > n_t: P = n_t with SciPy's UserWarning, and F = P unless nfft was given
  NaN, inf  a segment holding one is NaN in every bin (the mean is not finite), and so is the row
"""
from __future__ import annotations

import warnings

import numpy as np


def plan(n_t, nperseg=256, nfft=None):
    """(P, F, noverlap, step, nseg) of welch on rows of n_t samples."""
    n_t, P = int(n_t), int(nperseg)
    if P > n_t:
        warnings.warn(f"nperseg = {P:d} is greater than input length  = {n_t:d}, using nperseg = {n_t:d}", UserWarning,
                      stacklevel=3)
        P = n_t
    F = P if nfft is None else int(nfft)
    if F < P:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    noverlap = P // 2
    step = P - noverlap
    return P, F, noverlap, step, (n_t - noverlap) // step


def fold(F):
    """The one-sided factors of the F // 2 + 1 bins: 2 everywhere but DC and, for even F, the last bin."""
    m = np.full(F // 2 + 1, 2.0)
    m[0] = 1.0
    if F % 2 == 0:
        m[-1] = 1.0
    return m


def welch(x, fs, nperseg=256, nfft=None):
    """(f [F // 2 + 1], Pxx [..., F // 2 + 1]) of rows x [..., n_t] (any dtype, computed in float64)."""
    import scipy.signal
    x = np.asarray(x).astype(np.float64)
    n_t = x.shape[-1]
    P, F, noverlap, step, nseg = plan(n_t, nperseg, nfft)
    win = scipy.signal.get_window("hann", P).astype(np.float64)
    acc = np.zeros(x.shape[:-1] + (F // 2 + 1,))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(nseg):
            seg = x[..., s * step:s * step + P]
            mean = seg.mean(axis=-1, keepdims=True)
            X = np.fft.rfft((seg - mean) * win, n=F, axis=-1)
            p = X.real ** 2 + X.imag ** 2
            acc = acc + np.where(np.isfinite(mean), p, np.nan)
        pxx = acc / nseg * (1.0 / (fs * (win * win).sum())) * fold(F)
    return np.fft.rfftfreq(F, 1.0 / fs), pxx


def win_avg_psd(windows, fs, nperseg=2048):
    """(f, Pxx_avg, Pxxs) of win_avg_psd for a list of [channels, n_t] arrays (channel counts may differ)."""
    _, first = welch(np.asarray(windows[0])[0], fs, nperseg)
    pxxs = np.zeros((len(windows), first.shape[0]))
    f = None
    for i, w in enumerate(windows):
        f, p = welch(np.asarray(w), fs, nperseg)
        pxxs[i, :] = p.sum(axis=0) / p.shape[0]
    return f, pxxs.mean(axis=0), pxxs


def sample_rate(t_axis):
    """int(1 / dt) in float64: 250 for dt just below 0.004 (w = 500 axes), 249 just above (w = 499)."""
    return int(1 / (t_axis[1] - t_axis[0]))


def psd_vs_offset(xcf, x_axis, t_axis, fhi=20, pclip=98, log_scale=False, x_max=200, x_min=0, vmax=None, vmin=None):
    """(spec, freq[:fhi_idx], x_axis[min_idx:max_idx], vmax, vmin, fhi_idx): what plot_psd_vs_offset hands to imshow
    (before .T) and its colour limits."""
    x_axis = np.asarray(x_axis)
    if x_axis[0] > x_axis[-1]:
        x_axis = x_axis * -1
    fs = sample_rate(t_axis)
    freq, pxx = welch(xcf, fs, nperseg=256, nfft=1024)
    fhi_idx = int(np.argmax(freq >= fhi))
    spec = pxx[:, :fhi_idx]
    if log_scale:
        spec = 10 * np.log10(spec)
    if not vmax:
        vmax = np.percentile(spec, pclip) if spec.size else np.nan
    if not vmin:
        vmin = np.percentile(spec, 100 - pclip) if spec.size else np.nan
    a, b = np.abs(x_max - x_axis).argmin(), np.abs(x_min - x_axis).argmin()
    lo, hi = min(a, b), max(a, b)
    return spec[lo:hi], freq[:fhi_idx], x_axis[lo:hi], vmax, vmin, fhi_idx


def spectrum_vs_offset(xcf, t_axis, fhi=20):
    """(|fft(xcf)[:, :fhi_idx]|, freq[:fhi_idx], fhi_idx) with freq = fftfreq(w, dt)."""
    xcf = np.asarray(xcf, dtype=np.float64)
    freq = np.fft.fftfreq(xcf.shape[-1], d=t_axis[1] - t_axis[0])
    fhi_idx = int(np.argmax(freq >= fhi))
    return np.abs(np.fft.fft(xcf, axis=-1)[:, :fhi_idx]), freq[:fhi_idx], fhi_idx
