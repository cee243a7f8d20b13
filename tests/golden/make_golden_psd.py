"""Generate the spectra fixture by running the REFERENCE's win_avg_psd (modules/utils.py:715-728), plot_psd_vs_offset
and plot_spectrum_vs_offset (apis/virtual_shot_gather.py:45-109) where the reference is installed (the same place
make_golden.py runs; never on the GPU box):

    python tests/golden/make_golden_psd.py

The two plot functions return nothing: they get a recorder as ``ax`` that keeps what they hand to imshow (the array,
``extent``, ``vmax``, ``vmin``), and an ``fname`` in a temporary directory so that they save an (empty) Agg figure
instead of showing one.  Only data leaves this script, tests/golden/psd.npz (under 1 MiB):
  a_q0 .. a_q4    class A: five windows of 5 500 samples at fs = 250, band-passed (order-10 Butterworth, 1.2-30 Hz,
                  zero phase) noise plus two tones, four of 6 rows and one (a_q2) of 4; int16, value = q * 2**-8
  b_q             class B: three 5 x 2 000 windows (nperseg = 2048 is clipped to 2 000, one segment, 1 001 bins)
  {a,b}_f, _avg, _pxxs    win_avg_psd(windows, 250) of the class
  band_ratio      per class, the largest max(row) / min(row over 2-25 Hz) over the rows of Pxxs and Pxx_avg: the factor
                  between an error bound relative to a row's maximum and one relative to a bin of the band.  The
                  noise seed of a class is the first of 0, 1, ... that keeps it under 80 (the tests require <= 100).
  g500_q, g499_q  a 49 x 500 and a 49 x 499 gather (int16, * 2**-8), g500_x ascending, g499_x descending offsets,
                  g500_t / g499_t time axes of dt = 0.003999999999997783 / 0.004000000000001336
  g*_psd<k>_{spec,extent,vmax,vmin,args}   plot_psd_vs_offset case k; args = (log_scale, x_min, x_max, pclip)
  g*_spec, g*_spec_extent                  plot_spectrum_vs_offset
"""
from __future__ import annotations

import os
import sys
import tempfile
import types
import warnings

sys.dont_write_bytecode = True

import numpy as np
import scipy
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import import_reference  # noqa: E402

QUANT = 2.0 ** -8
FS = 250
DT = {500: 0.003999999999997783, 499: 0.004000000000001336}
PSD_CASES = [(False, -100, 100, 98), (True, -100, 100, 98), (False, 0, 200, 98), (True, -60, 150, 90)]


def bandpassed(rng, rows, n_t):
    sos = scipy.signal.butter(10, [1.2 / (FS / 2), 30 / (FS / 2)], btype="band", output="sos")
    x = scipy.signal.sosfiltfilt(sos, rng.standard_normal((rows, n_t + 2000)), axis=-1)[:, 1000:1000 + n_t]
    return x / x.std()


def windows_of(seed, shapes):
    rng = np.random.default_rng(seed)
    out = []
    for rows, n_t in shapes:
        t = np.arange(n_t) / FS
        x = 8.0 * bandpassed(rng, rows, n_t)
        x += 0.4 * np.sin(2 * np.pi * 7.3 * t + rng.uniform(0, 6, (rows, 1)))
        x += 0.3 * np.sin(2 * np.pi * 14.1 * t + rng.uniform(0, 6, (rows, 1)))
        out.append(np.round(x / QUANT).astype(np.int16))
    return out


def band_ratio(f, avg, pxxs):
    band = (f >= 2) & (f <= 25)
    rows = np.vstack([pxxs, avg[None]])
    return float((rows.max(axis=1) / rows[:, band].min(axis=1)).max())


def run_class(ref, shapes):
    for seed in range(100):
        qs = windows_of(seed, shapes)
        wins = [types.SimpleNamespace(data=q.astype(np.float64) * QUANT) for q in qs]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            f, avg, pxxs = ref.ut.win_avg_psd(wins, FS)
        r = band_ratio(f, avg, pxxs)
        if r < 80:
            return qs, f, avg, pxxs, r, seed
    raise AssertionError("no seed keeps the band ratio under 80")


class AxRecorder:
    def imshow(self, arr, extent=None, vmax=None, vmin=None, **kw):
        self.arr, self.extent, self.vmax, self.vmin = np.array(arr), np.array(extent, dtype=np.float64), vmax, vmin

    def set_xlabel(self, *a, **k):
        pass

    set_ylabel = set_xlabel


def gather_of(seed, w):
    rng = np.random.default_rng(seed)
    t = np.arange(w) / FS
    x = 0.5 * bandpassed(rng, 49, w)
    for r in range(49):
        off = abs(r - 24) * 8.16
        x[r] += 20.0 * np.exp(-off / 150.0) * np.exp(-0.5 * ((t - 1.0 - off / 400.0) / 0.05) ** 2) * \
            np.cos(2 * np.pi * 9.0 * (t - 1.0 - off / 400.0))
    return np.round(x / QUANT).astype(np.int16)


def main():
    ref = import_reference()
    out = dict(meta=np.array(repr(dict(numpy=np.__version__, scipy=scipy.__version__))))
    ratios = []
    for name, shapes in (("a", [(6, 5500), (6, 5500), (4, 5500), (6, 5500), (6, 5500)]), ("b", [(5, 2000)] * 3)):
        qs, f, avg, pxxs, r, seed = run_class(ref, shapes)
        if name == "a":
            out.update({f"a_q{i}": q for i, q in enumerate(qs)})
        else:
            out["b_q"] = np.stack(qs)
        out.update({f"{name}_f": f, f"{name}_avg": avg, f"{name}_pxxs": pxxs, f"{name}_seed": np.array(seed)})
        ratios.append(r)
        print(f"class {name}: seed {seed}, {pxxs.shape[1]} bins, band ratio {r:.1f}")
    out["band_ratio"] = np.array(ratios)
    with tempfile.TemporaryDirectory() as tmp:
        for w, seed in ((500, 11), (499, 12)):
            q = gather_of(seed, w)
            xcf = q.astype(np.float64) * QUANT
            x_axis = (np.arange(49) - 24) * 8.16
            if w == 499:
                x_axis = x_axis[::-1].copy()
            t_axis = np.arange(w) * DT[w]
            g = f"g{w}"
            out.update({f"{g}_q": q, f"{g}_x": x_axis, f"{g}_t": t_axis})
            for k, (log_scale, x_min, x_max, pclip) in enumerate(PSD_CASES):
                ax = AxRecorder()
                ref.vsg.plot_psd_vs_offset(xcf, x_axis, t_axis, ax=ax, pclip=pclip, log_scale=log_scale, x_max=x_max,
                                           x_min=x_min, fname=f"{g}_{k}.png", fdir=tmp)
                out.update({f"{g}_psd{k}_spec": ax.arr.T, f"{g}_psd{k}_extent": ax.extent,
                            f"{g}_psd{k}_vmax": np.array(ax.vmax), f"{g}_psd{k}_vmin": np.array(ax.vmin),
                            f"{g}_psd{k}_args": np.array([log_scale, x_min, x_max, pclip], dtype=np.float64)})
            ax = AxRecorder()
            ref.vsg.plot_spectrum_vs_offset(xcf, x_axis, t_axis, ax=ax, fname=f"{g}_s.png", fdir=tmp)
            out.update({f"{g}_spec": ax.arr.T, f"{g}_spec_extent": ax.extent})
            print(f"gather {w}: psd {out[f'{g}_psd0_spec'].shape}, spectrum {ax.arr.T.shape}")
    path = os.path.join(HERE, "psd.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 2 ** 20:.2f} MiB")
    assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
