"""NumPy restatement of the record ingest (ImagingIO.__getitem__ after the file is read, modules/imaging_IO.py:44-46):
scipy.signal.savgol_filter(x, W, P) (mode='interp') as the three linear maps (h, el, er) evaluated in float64, and
the dtype and divide rules:

  float32 stays float32: the float64 sums are rounded once to float32, then divided by float32(divisor)
  float64 stays float64 and divides in float64
  any other dtype is converted to float64 first (SciPy's rule)

``operator`` takes the maps from SciPy the way the product does (SciPy is the coefficient designer); everything
else is plain NumPy, summed in tap order j = 0 .. W - 1.
"""
from __future__ import annotations

import numpy as np


def operator(window_length=21, polyorder=15):
    """(h [W], el [half, W], er [half, W]): h = savgol_coeffs[::-1]; el / er the first / last half rows of the matrix
    savgol_filter makes of the W x W identity, one column at a time."""
    import scipy.signal
    W, half = int(window_length), int(window_length) // 2
    h = np.ascontiguousarray(scipy.signal.savgol_coeffs(W, polyorder)[::-1], dtype=np.float64)
    m = np.zeros((W, W))
    for c in range(W):
        e = np.zeros(W)
        e[c] = 1.0
        m[:, c] = scipy.signal.savgol_filter(e, W, polyorder)
    return h, m[:half].copy(), m[W - half:].copy()


def smooth64(x, h, el, er):
    """The float64 result [..., n_t] of the three maps on rows x (any dtype), before any rounding or division."""
    x = np.asarray(x)
    x64 = x.astype(np.float64)
    W = len(h)
    half = W // 2
    n_t = x64.shape[-1]
    if n_t < W:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    out = np.zeros(x64.shape, dtype=np.float64)
    n_int = n_t - 2 * half
    acc = np.zeros(x64.shape[:-1] + (n_int,), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(W):
            acc = acc + h[j] * x64[..., j:j + n_int]
        out[..., half:n_t - half] = acc
        for t in range(half):
            sl = np.zeros(x64.shape[:-1])
            sr = np.zeros(x64.shape[:-1])
            for j in range(W):
                sl = sl + el[t, j] * x64[..., j]
                sr = sr + er[t, j] * x64[..., n_t - W + j]
            out[..., t] = sl
            out[..., n_t - half + t] = sr
    return out


def smooth(x, h, el, er, divisor=1.0):
    """savgol_filter(x, W, P) then ``/= divisor`` with the reference's dtypes."""
    x = np.asarray(x)
    y = smooth64(x, h, el, er)
    if x.dtype == np.float32:
        y = y.astype(np.float32)
        return y / np.float32(divisor) if divisor != 1 else y
    return y / np.float64(divisor) if divisor != 1 else y


def scale_only(x, divisor):
    """smoothing=False: the division alone (other dtypes as float64: the reference's in-place divide of an integer
    record raises)."""
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    return x / x.dtype.type(divisor) if divisor != 1 else x.copy()


def ulp32(v):
    """One float32 ulp at |v| (v float64 or float32)."""
    return np.spacing(np.abs(np.asarray(v)).astype(np.float32)).astype(np.float64)


def edge_mask(n_t, half):
    m = np.zeros(n_t, dtype=bool)
    m[:half] = True
    m[n_t - half:] = True
    return m
