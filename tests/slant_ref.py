"""Float64 NumPy restatement of the reference's map_fv_FD_slant_stack (modules/utils.py:429-454), vectorised: the
oracle of the device transform (tests/test_slant_gpu.py), itself pinned to the reference's recorded outputs
(tests/test_slant_host.py, tests/golden/slant.npz).

    rows = data[6:25], each divided by its L1 norm with ``norm``
    nf = 2 ** (1 + ceil(log2(nt))),  f_idx(f) = argmin |f - fftfreq(nf, dt)|  (the first minimum)
    pout[f, v] = | sum_ix fft(rows, n=nf)[ix, f_idx(f)] * exp(+i 2 pi f (dx ix) / v) |,  returned as pout.T

The time DFT is taken at the needed bins only; the steering is one exp(i theta) per (f, v), theta = 2 pi f dx / v, its
powers by recurrence, and the sum runs in row order, as the reference's loop does.
"""
import math

import numpy as np


QUANT = 2.0 ** -8      # the fixture's gathers are int16 multiples of this
CASES = "ABCDEFG"      # tests/golden/slant.npz (tests/golden/make_golden_slant.py)


def case(g, name):
    """(data float64, dx, dt, freqs, vels, norm) of a case of the loaded fixture g."""
    return (g[f"{name}_q"].astype(np.float64) * QUANT, float(g[f"{name}_dx"]), float(g[f"{name}_dt"]),
            g[f"{name}_freqs"], g[f"{name}_vels"], bool(g[f"{name}_norm"]))


def sizes(nt):
    return 2 ** (1 + math.ceil(math.log(nt, 2)))


def bins(nt, dt, freqs):
    """(nf, f_idx[nF]) with the reference's own expressions."""
    nf = sizes(nt)
    fft_freqs = np.fft.fftfreq(nf, d=dt)
    return nf, np.array([np.abs(f - fft_freqs).argmin() for f in np.asarray(freqs, dtype=np.float64)], dtype=np.int64)


def spectra(rows, nf, fidx):
    """fft(rows, n=nf)[:, fidx] by the DFT sum at the unique bins (float64, the angle reduced mod nf exactly)."""
    ub, inv = np.unique(fidx, return_inverse=True)
    t = np.arange(rows.shape[-1])
    ang = 2.0 * np.pi * ((np.outer(t, ub) % nf) / nf)
    return (rows @ (np.cos(ang) - 1j * np.sin(ang)))[:, inv]


def slant(data, dx, dt, freqs, vels, norm=True, rows=(6, 25)):
    data = np.asarray(data, dtype=np.float64)[slice(*rows)]
    freqs = np.asarray(freqs, dtype=np.float64)
    vels = np.asarray(vels, dtype=np.float64)
    if (vels == 0).any():
        raise ValueError("math domain error")
    if norm:
        with np.errstate(invalid="ignore", divide="ignore"):
            data = data / np.linalg.norm(data, axis=-1, keepdims=True, ord=1)
    nf, fidx = bins(data.shape[-1], dt, freqs)
    acc = np.zeros((freqs.size, vels.size), dtype=complex)
    if data.shape[0]:
        D = spectra(data, nf, fidx)
        w = np.exp(1j * (2 * math.pi * freqs[:, None] * dx / vels[None, :]))
        p = np.ones_like(w)
        for ix in range(data.shape[0]):
            acc += D[ix][:, None] * p
            p = p * w
    return np.abs(acc).T


def coherence_ratio(data, dt, freqs, image, norm=True, rows=(6, 25)):
    """Condition (a) of the fixture: max_f sum_ix |D[ix, f_idx(f)]| / max |image| -- how far the steering sum's terms
    exceed its largest magnitude, the factor by which a per-row relative error can show in the image."""
    data = np.asarray(data, dtype=np.float64)[slice(*rows)]
    if norm:
        data = data / np.linalg.norm(data, axis=-1, keepdims=True, ord=1)
    nf, fidx = bins(data.shape[-1], dt, freqs)
    return float(np.abs(spectra(data, nf, fidx)).sum(axis=0).max() / np.abs(image).max())


def near_tie_fraction(image, rel=2e-6):
    """Condition (b): the share of frequency columns whose runner-up lies within rel * max|image| of the maximum."""
    image = np.asarray(image)
    if image.shape[0] < 2:
        return 1.0
    top = np.sort(image, axis=0)[-2:]
    return float(np.mean(top[1] - top[0] <= rel * np.abs(image).max()))
