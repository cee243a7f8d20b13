"""Spectra, host side (no GPU): tests/psd_ref against scipy.signal.welch and against the reference's recorded outputs
(tests/golden/psd.npz), the float64 host arithmetic of das_diff_veh_amd.spectra.welch_plan, the error rules of
win_avg_psd and the argument checks of dvh_welch_rows, which return before any device work.

Tolerances: psd_ref and SciPy evaluate the same float64 formula with different FFT codes; both are within a few
float64 roundings of log2(F) butterflies, so they agree within 1e-13 of a row's maximum (measured: 2e-16).
"""
import ctypes
import os
import types
import warnings

import numpy as np
import pytest
import scipy.signal

from tests import golden_io as gio
from tests import psd_ref

# (nperseg, nfft) of the fast form and the row lengths at which the segment count changes
PF = [(256, 1024), (512, 512), (2048, 2048), (2048, 4096)]
QUANT = 2.0 ** -8
DT500, DT499 = 0.003999999999997783, 0.004000000000001336


def lengths(P):
    step = P - P // 2
    return [P, P + step - 1, P + step, 2 * P + 1, 5500]


def golden_windows(g, name):
    qs = [g[f"a_q{i}"] for i in range(5)] if name == "a" else list(g["b_q"])
    return [q.astype(np.float64) * QUANT for q in qs]


@pytest.mark.parametrize("P,F", PF)
def test_psd_ref_matches_scipy(P, F):
    rng = np.random.default_rng(P + F)
    for n_t in lengths(P):
        x = rng.standard_normal((3, n_t)) + 0.3
        f, p = psd_ref.welch(x, 250, P, F)
        fs, ps = scipy.signal.welch(x, 250, nperseg=P, nfft=F)
        assert np.array_equal(f, fs) and p.shape == ps.shape == (3, F // 2 + 1)
        err = (np.abs(p - ps).max(axis=1) / ps.max(axis=1)).max()
        print(P, F, n_t, err)
        assert err <= 1e-13


@pytest.mark.parametrize("n_t", [2000, 1999, 301])
def test_psd_ref_clipped_matches_scipy(n_t):
    """nperseg above the row length: clipped with SciPy's warning; 1 999 and 301 give an odd nfft, whose last bin is
    doubled like the others."""
    x = np.random.default_rng(n_t).standard_normal((2, n_t))
    with pytest.warns(UserWarning, match=f"using nperseg = {n_t}"):
        f, p = psd_ref.welch(x, 250, 2048)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fs, ps = scipy.signal.welch(x, 250, nperseg=2048)
    assert p.shape == (2, n_t // 2 + 1) and np.array_equal(f, fs)
    assert (np.abs(p - ps).max(axis=1) / ps.max(axis=1)).max() <= 1e-13


def test_fold():
    assert psd_ref.fold(4).tolist() == [1, 2, 1] and psd_ref.fold(5).tolist() == [1, 2, 2]
    # Parseval on an odd length: the folded one-sided sum is the whole two-sided power
    x = np.random.default_rng(0).standard_normal(7)
    X = np.fft.fft(x)
    one = (np.abs(np.fft.rfft(x)) ** 2 * psd_ref.fold(7)).sum()
    assert abs(one - (np.abs(X) ** 2).sum()) <= 1e-12 * one


def test_non_finite_rows_are_nan_as_scipys():
    x = np.random.default_rng(1).standard_normal((4, 700))
    x[1, 5] = np.nan
    x[2, 300] = np.inf
    x[3, 699] = np.nan      # in the ignored tail: nseg = (700 - 128) // 128 = 4 segments end at sample 639
    _, p = psd_ref.welch(x, 250, 256, 1024)
    with np.errstate(all="ignore"):
        _, ps = scipy.signal.welch(x, 250, nperseg=256, nfft=1024)
    assert np.isnan(p[1]).all() and np.isnan(p[2]).all() and np.isnan(ps[1]).all() and np.isnan(ps[2]).all()
    assert np.isfinite(p[0]).all() and np.isfinite(p[3]).all() and np.isfinite(ps[3]).all()


@pytest.mark.parametrize("name", ["a", "b"])
def test_psd_ref_reproduces_reference_classes(name):
    g = gio.load("psd")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        f, avg, pxxs = psd_ref.win_avg_psd(golden_windows(g, name), 250)
    assert np.array_equal(f, g[f"{name}_f"]) and pxxs.shape == g[f"{name}_pxxs"].shape
    assert pxxs.shape[1] == (1025 if name == "a" else 1001)
    assert np.abs(avg - g[f"{name}_avg"]).max() <= 1e-12 * g[f"{name}_avg"].max()
    assert (np.abs(pxxs - g[f"{name}_pxxs"]).max(axis=1) <= 1e-12 * g[f"{name}_pxxs"].max(axis=1)).all()


def test_fixture_band_ratio():
    """The fixture condition behind the per-bin bound of the GPU test: over 2-25 Hz no bin of a class spectrum lies more
    than a factor 100 under its row's maximum (recomputed here from the reference's recorded output)."""
    g = gio.load("psd")
    for k, name in enumerate("ab"):
        f = g[f"{name}_f"]
        band = (f >= 2) & (f <= 25)
        rows = np.vstack([g[f"{name}_pxxs"], g[f"{name}_avg"][None]])
        ratio = (rows.max(axis=1) / rows[:, band].min(axis=1)).max()
        print(name, ratio)
        assert abs(ratio - g["band_ratio"][k]) <= 1e-9 * ratio and ratio <= 100


def gather(g, w):
    return g[f"g{w}_q"].astype(np.float64) * QUANT, g[f"g{w}_x"], g[f"g{w}_t"]


def psd_cases(g, w):
    k = 0
    while f"g{w}_psd{k}_args" in g.files:
        log_scale, x_min, x_max, pclip = g[f"g{w}_psd{k}_args"]
        yield k, dict(log_scale=bool(log_scale), x_min=x_min, x_max=x_max, pclip=pclip)
        k += 1


@pytest.mark.parametrize("w,fs,fhi_idx", [(500, 250, 82), (499, 249, 83)])
def test_psd_ref_reproduces_reference_gathers(w, fs, fhi_idx):
    g = gio.load("psd")
    xcf, x_axis, t_axis = gather(g, w)
    assert t_axis[1] - t_axis[0] == (DT500 if w == 500 else DT499)
    assert psd_ref.sample_rate(t_axis) == fs
    n = 0
    for k, kw in psd_cases(g, w):
        spec, freq, x, vmax, vmin, idx = psd_ref.psd_vs_offset(xcf, x_axis, t_axis, **kw)
        want = g[f"g{w}_psd{k}_spec"]
        assert idx == fhi_idx and spec.shape == want.shape and freq.shape == (fhi_idx,) and x.shape == (len(want),)
        assert np.abs(spec - want).max() <= 1e-12 * np.abs(want).max()
        assert abs(vmax - g[f"g{w}_psd{k}_vmax"]) <= 1e-12 * abs(vmax)
        assert abs(vmin - g[f"g{w}_psd{k}_vmin"]) <= 1e-12 * abs(vmin)
        ext = g[f"g{w}_psd{k}_extent"]
        assert x[0] == ext[0] and freq[0] == ext[3] == 0 and np.fft.rfftfreq(1024, 1.0 / fs)[fhi_idx] == ext[2]
        n += 1
    assert n == 4
    spec, freq, idx = psd_ref.spectrum_vs_offset(xcf, t_axis)
    want = g[f"g{w}_spec"]
    assert spec.shape == want.shape == (49, idx) and np.abs(spec - want).max() <= 1e-12 * want.max()
    # no bin at or above fhi: argmax of an all-False mask is 0 and the result is empty
    assert psd_ref.psd_vs_offset(xcf, x_axis, t_axis, fhi=200)[0].shape[1] == 0
    assert psd_ref.spectrum_vs_offset(xcf, t_axis, fhi=200)[0].shape == (49, 0)


def test_welch_plan_is_scipys_host_arithmetic():
    from das_diff_veh_amd.spectra import welch_plan
    for P, F in PF:
        for n_t in lengths(P):
            p = welch_plan(n_t, 250, P, F)
            assert (p.nperseg, p.nfft, p.noverlap, p.step, p.nseg) == psd_ref.plan(n_t, P, F)
            assert np.array_equal(p.win, scipy.signal.get_window("hann", P)) and p.fast
            assert np.array_equal(p.freqs, scipy.signal.welch(np.zeros(n_t), 250, nperseg=P, nfft=F)[0])
            assert p.scale == 1.0 / (250 * (p.win * p.win).sum())
    with pytest.warns(UserWarning, match="nperseg = 2048 is greater than input length  = 2000, using nperseg = 2000"):
        p = welch_plan(2000, 250, 2048)
    assert (p.nperseg, p.nfft, p.nseg, p.bins, p.fast) == (2000, 2000, 1, 1001, False)
    with pytest.warns(UserWarning):
        assert welch_plan(1999, 249, 2048).bins == 1000
    with pytest.warns(UserWarning):   # a given nfft stays
        assert welch_plan(200, 250, 256, 1024).nfft == 1024
    with pytest.raises(ValueError, match="nfft must be greater than or equal to nperseg"):
        welch_plan(5500, 250, 2048, 1024)


def test_win_avg_psd_error_rules():
    """The reference's failures, raised on the host before any device work: an empty list (IndexError from
    win_spectrum[0]) and windows whose spectra differ in length (ValueError from the row assignment)."""
    from das_diff_veh_amd.modules.utils import extract_ridge_ref_idx, win_avg_psd  # the notebooks' import line
    assert callable(extract_ridge_ref_idx)
    with pytest.raises(IndexError):
        win_avg_psd([], 250)
    with pytest.raises(IndexError):
        psd_ref.win_avg_psd([], 250)
    wins = [types.SimpleNamespace(data=np.zeros((3, 5500))), types.SimpleNamespace(data=np.zeros((3, 2000)))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        with pytest.raises(ValueError, match="could not broadcast"):
            win_avg_psd(wins, 250)
        with pytest.raises(ValueError, match="could not broadcast"):
            psd_ref.win_avg_psd([w.data for w in wins], 250)


def test_welch_rows_argument_checks_need_no_gpu():
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    lib = _lib.load()
    P = ctypes.c_void_p
    x, win, out, ws = P(0x10000), P(0x20000), P(0x40000000), P(0x50000000)

    def call(n_t=5500, nperseg=2048, nfft=2048, rows=6, groups=3, tab=None, out=out, ws=None, rs=None, gs=None, x=x):
        rs = n_t if rs is None else rs
        gs = rows * rs if gs is None else gs
        return lib.dvh_welch_rows(x, groups, gs, rows, rs, n_t, win, nperseg, nfft, 1.0, tab, out, ws, None)
    for kw, rc, msg in ((dict(nperseg=5501, nfft=8192), -4, b"nperseg"), (dict(nfft=1024), -4, b"nfft"),
                        (dict(nperseg=300, nfft=300), -4, b"twiddle table"),
                        (dict(n_t=30000, nperseg=20000, nfft=20000, tab=P(0x30000)), -4, b"unsupported nfft"),
                        (dict(x=None), -2, b"null"), (dict(rs=5499), -2, b"row stride"),
                        (dict(gs=6 * 5500 - 1), -2, b"group stride"), (dict(rows=0), -2, b"invalid"),
                        (dict(out=P(0x10000 + 4 * 5500)), -2, b"overlap"), (dict(rows=65), -2, b"workspace"),
                        (dict(rows=65, ws=P(0x40000000 + 8)), -2, b"workspace overlaps")):
        assert call(**kw) == rc, kw
        assert msg in lib.dvh_last_error(), (kw, lib.dvh_last_error())
    assert lib.dvh_welch_rows_workspace(5, 64, 2048) == 0
    assert lib.dvh_welch_rows_workspace(5, 65, 2048) == 8 * 5 * 2 * 1025
    assert lib.dvh_welch_rows_workspace(5, 200, 2000) == 0      # the direct form sums a group in one block
    assert lib.dvh_abi_version() == 2
