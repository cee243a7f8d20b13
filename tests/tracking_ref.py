"""SciPy / NumPy restatement of TimeLapseImaging._preprocess_for_tracking (apis/timeLapseImaging.py:74-102) and of
its helpers (find_noise_idx, impute_noisy_trace, bandpass_data, bandpass_data_space: modules/utils.py:179-189,
316-329, 584-594).  Test support only: the product never imports it.  tests/test_tracking_ref.py pins it to the
reference's own outputs (tests/golden/tracking_prep*.npz); the GPU tests and tools/bench_tracking_prep.py use it as
the CPU statement of the chain and of its stages."""
import numpy as np
import scipy.signal

DX = 8.16


def butter_sos(step, flo, fhi):
    fny = 0.5 / step
    return scipy.signal.butter(10, [flo / fny, fhi / fny], analog=False, btype="band", output="sos")


def resample_filter(up, down):
    """resample_poly's default design for the reduced ratio: (up, down, half_len, h)."""
    g = int(np.gcd(up, down))
    up, down = up // g, down // g
    if up == down == 1:
        return up, down, 0, np.ones(1)
    half_len = 10 * max(up, down)
    return up, down, half_len, scipy.signal.firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up


def resample_rows(x, up, down):
    """scipy.signal.resample_poly(x, up, down, axis=0) written out:
    y[m] = sum_k h[half_len + down m - up k] x[k], k over the rows whose coefficient index is in [0, 2 half_len]."""
    x = np.asarray(x, dtype=np.float64)
    up, down, half_len, h = resample_filter(up, down)
    n_in = x.shape[0]
    n_out = -(-n_in * up // down)
    y = np.zeros((n_out,) + x.shape[1:])
    for m in range(n_out):
        k0 = max(0, -((half_len - down * m) // up))          # ceil((down m - half_len) / up)
        k1 = min(n_in - 1, (down * m + half_len) // up)
        for k in range(k0, k1 + 1):
            y[m] += h[half_len + down * m - up * k] * x[k]
    return y


def gate(data, noise_level=10):
    """-> (gated copy, medians, gated indices)."""
    d = np.array(data, dtype=np.float64, copy=True)
    med = np.median(np.abs(d), axis=-1)
    d[med > noise_level] *= 0
    return d, med, np.flatnonzero(med > noise_level)


def impute_empty(d, threshold=30):
    """find_noise_idx(empty_tr=True) + impute_noisy_trace, in place; -> the imputed index."""
    i = int(np.argmax(np.linalg.norm(d, axis=1) < threshold))
    if i + 1 == d.shape[0]:
        d[i] = d[i - 1]
    elif i == 0:
        d[i] = d[i + 1]
    else:
        d[i] = d[i - 1] + d[i + 1]
    return i


def tracking_ref(data, dt, x0_channel, flo=0.08, fhi=1, flo_space=0.006, fhi_space=0.04, subsamp_factor=5,
                 noise_level=10, channel0=400, up=204, down=25, use_scipy_resample=False):
    """-> dict(out, dist, med, gated, imputed, bp (after the time band-pass), rs (resampled, before the space
    band-pass))."""
    d, med, gated = gate(data, noise_level)
    imputed = impute_empty(d)
    d[:] = scipy.signal.sosfiltfilt(butter_sos(dt, flo, fhi), d, axis=1)
    sub = d[:, ::subsamp_factor]
    rs = scipy.signal.resample_poly(sub, up, down) if use_scipy_resample else resample_rows(sub, up, down)
    dist = np.arange(rs.shape[0]) + (x0_channel - channel0) * DX
    out = rs.copy()
    if not (flo_space == -1 and fhi_space == -1):
        out[:] = scipy.signal.sosfiltfilt(butter_sos(dist[1] - dist[0], flo_space, fhi_space), out, axis=0)
    return dict(out=out, dist=dist, med=med, gated=gated, imputed=imputed, bp=d, rs=rs)
