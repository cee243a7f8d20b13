"""Welch power spectra on the device: dvh_welch_rows against tests/psd_ref on the same float32 values, win_avg_psd
against the reference's recorded class spectra, and the gather spectra (psd_vs_offset, spectrum_vs_offset,
VirtualShotGather.spec_vs_offset) against the reference's recorded imshow arrays (tests/golden/psd.npz).

Error bound of the fast form: |got - want| <= 1e-5 max(want over the row or group).  A float32 FFT's norm-wise error is
about eps log2(F) = 6e-8 * 11 on amplitudes, twice that on power, and ||x|| <= max|X| by Parseval: about 1.3e-6 of the
maximum; 1e-5 leaves 8 x.  On the golden classes a bin of the 2-25 Hz band lies at most band_ratio <= 100 under its
row's maximum (tests/test_psd_host.py), so its relative error is at most 1e-5 band_ratio <= 1e-3.  The direct form and
spectrum_vs_offset are float64 on float32-exact inputs: 1e-10 of the maximum.  Measured values: DESIGN.md, Spectra.
"""
import ctypes
import warnings

import numpy as np
import pytest

from tests import golden_io as gio
from tests import psd_ref
from tests.test_psd_host import PF, gather, golden_windows, lengths, psd_cases

pytestmark = pytest.mark.gpu

FAST_TOL, F64_TOL = 1e-5, 1e-10
CANARY = -7.0
_TAB = {}


def _place(x, layout, device):
    """A device view [G, C, n_t] holding x: 'contig', 'stride5' (row stride n_t + 5: rows at every alignment), 'odd'
    (base one element into the buffer)."""
    import torch
    G, C, n_t = x.shape
    stride = n_t + 5 if layout == "stride5" else n_t
    off = 1 if layout == "odd" else 0
    buf = torch.zeros(G * C * stride + off, dtype=torch.float32, device=device)
    view = buf[off:].view(G, C, stride)[:, :, :n_t]
    view.copy_(torch.from_numpy(x))
    return view


def _tables(P, F, fs, device):
    """(win, tab, scale) as the caller of dvh_welch_rows makes them (include/dvh.h), independent of spectra.py."""
    import scipy.signal
    import torch
    key = (P, F, fs)
    if key not in _TAB:
        win = scipy.signal.get_window("hann", P).astype(np.float64)
        ang = 2.0 * np.pi * np.arange(F) / F
        tab = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
        _TAB[key] = (torch.from_numpy(win).to(device), torch.from_numpy(tab).to(device),
                     1.0 / (fs * float((win * win).sum())))
    return _TAB[key]


def _welch(xv, P, F, fs=250.0, ws="auto", tab="auto", out=None):
    """dvh_welch_rows on a view [G, C, n_t] into the middle of a canary-filled buffer; returns (result, buffer)."""
    import torch

    from das_diff_veh_amd import _lib
    G, C, n_t = xv.shape
    bins = F // 2 + 1
    buf = torch.full((G * bins + 64,), CANARY, dtype=torch.float64, device=xv.device)
    o = buf[32:32 + G * bins].view(G, bins) if out is None else out
    win, t, scale = _tables(P, F, fs, xv.device)
    if ws == "auto":
        nbytes = _lib.load().dvh_welch_rows_workspace(G, C, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=xv.device) if nbytes else None
    _lib.call("dvh_welch_rows", _lib.ptr(xv), G, xv.stride(0), C, xv.stride(1), n_t, _lib.ptr(win), P, F, scale,
              _lib.ptr(t if tab == "auto" else tab), _lib.ptr(o), _lib.ptr(ws), _lib.stream_of(xv.device))
    return o, buf


def _untouched(buf, G, bins):
    b = buf.cpu().numpy()
    return bool((b[:32] == CANARY).all() and (b[32 + G * bins:] == CANARY).all())


def _group_ref(x, P, F, fs=250.0):
    """psd_ref's group spectra [G, bins] of x [G, C, n_t]."""
    return psd_ref.welch(x, fs, P, F)[1].mean(axis=1)


def _rel_err(got, want):
    return float((np.abs(got - want).max(axis=-1) / want.max(axis=-1)).max())


@pytest.mark.parametrize("P,F", PF)
def test_welch_rows_matches_psd_ref(device, P, F):
    rng = np.random.default_rng(P * 3 + F)
    worst = 0.0
    for n_t in lengths(P):
        for C in (1, 3, 61):
            x = rng.standard_normal((5, C, n_t)).astype(np.float32)
            want5 = _group_ref(x, P, F)                      # groups are independent: the first is want5[:1]
            for G in (1, 5):
                want = want5[:G]
                outs = []
                for layout in ("contig", "stride5", "odd"):
                    o, buf = _welch(_place(x[:G], layout, device), P, F)
                    outs.append(o.cpu().numpy())
                    assert _untouched(buf, G, F // 2 + 1), (n_t, C, G, layout)
                err = _rel_err(outs[0], want)
                worst = max(worst, err)
                assert err <= FAST_TOL, (n_t, C, G, err)
                assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (n_t, C, G)
    print(f"P {P} F {F}: worst error {worst:.3g} of the maximum")


@pytest.mark.parametrize("P,F", [(256, 1024), (2048, 2048)])
def test_groups_of_more_rows_than_one_block_sums(device, P, F):
    """130 rows per group: chunks of 64, 64 and 2 rows, their partials added in chunk order from the workspace; a group
    is the same whichever call it is part of."""
    from das_diff_veh_amd import _lib
    x = np.random.default_rng(F).standard_normal((2, 130, P + P // 2 + 3)).astype(np.float32)
    want = _group_ref(x, P, F)
    outs = []
    for layout in ("contig", "stride5", "odd"):
        o, buf = _welch(_place(x, layout, device), P, F)
        outs.append(o.cpu().numpy())
        assert _untouched(buf, 2, F // 2 + 1)
    err = _rel_err(outs[0], want)
    print(f"130 rows, F {F}: {err:.3g}")
    assert err <= FAST_TOL
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    alone = _welch(_place(x[1:], "contig", device), P, F)[0].cpu().numpy()
    assert np.array_equal(alone[0], outs[0][1])
    with pytest.raises(_lib.DvhError, match="workspace"):
        _welch(_place(x, "contig", device), P, F, ws=None)


def test_detrending_is_float64(device):
    """A DC offset of 2**10 on unit noise: a float32 mean would leave 1e-4 of DC per sample in every segment."""
    x = (np.random.default_rng(2).standard_normal((1, 3, 5500)) + 2.0 ** 10).astype(np.float32)
    for P, F in ((2048, 2048), (256, 1024)):
        got = _welch(_place(x, "contig", device), P, F)[0].cpu().numpy()
        err = _rel_err(got, _group_ref(x, P, F))
        print(f"DC offset, F {F}: {err:.3g}")
        assert err <= FAST_TOL


@pytest.mark.parametrize("P,F,n_t", [(256, 1024, 700), (2048, 2048, 5500), (2000, 2000, 2000)])
def test_non_finite_rows(device, P, F, n_t):
    """One NaN and one inf row in the first 3-row group of a 2-group call: that group is NaN in every bin, the other is
    within the bound; a NaN in the tail past the last full segment is never read."""
    x = np.random.default_rng(4).standard_normal((2, 3, n_t)).astype(np.float32)
    x[0, 1, n_t // 3] = np.nan
    x[0, 2, P - 1] = np.inf
    step = P - P // 2
    used = (n_t - P // 2) // step * step + P // 2
    if used < n_t:
        x[1, 0, used:] = np.nan
    got = _welch(_place(x, "stride5", device), P, F)[0].cpu().numpy()
    assert np.isnan(got[0]).all()
    want = psd_ref.welch(x[1], 250.0, P, F)[1].mean(axis=0)
    assert np.isfinite(want).all()
    assert _rel_err(got[1], want) <= (FAST_TOL if F != 2000 else F64_TOL)


@pytest.mark.parametrize("n_t", [2000, 1999])
def test_direct_form_for_clipped_segments(device, n_t):
    """nperseg = 2048 on 2 000 / 1 999 samples: P = F = n_t, one segment, float64 sums; 1 999 is an odd F."""
    from das_diff_veh_amd.spectra import welch_rows
    import torch
    x = np.random.default_rng(n_t).standard_normal((2, 3, n_t)).astype(np.float32)
    want = _group_ref(x, n_t, n_t)
    outs = []
    for layout in ("contig", "stride5", "odd"):
        o, buf = _welch(_place(x, layout, device), n_t, n_t)
        outs.append(o.cpu().numpy())
        assert _untouched(buf, 2, n_t // 2 + 1)
    err = _rel_err(outs[0], want)
    print(f"direct form, F {n_t}: {err:.3g}")
    assert outs[0].shape == (2, n_t // 2 + 1) and err <= F64_TOL
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    with pytest.warns(UserWarning, match=f"using nperseg = {n_t}"):
        f, rows = welch_rows(torch.from_numpy(x[0]).to(device), 250, nperseg=2048)
    fr, pr = psd_ref.welch(x[0], 250, n_t, n_t)
    assert np.array_equal(f, fr) and _rel_err(rows.cpu().numpy(), pr) <= F64_TOL


def test_refusals_leave_the_output_untouched(device):
    import torch

    from das_diff_veh_amd import _lib
    x = _place(np.ones((2, 3, 3000), np.float32), "contig", device)
    many = _place(np.ones((2, 65, 3000), np.float32), "contig", device)
    bufs = []
    for xv, P, F, kw, msg in ((x, 3001, 4096, {}, "nperseg"), (x, 2048, 1024, {}, "nfft"),
                              (x, 300, 300, dict(tab=None), "twiddle table"),
                              (x, 3000, 9000, {}, "unsupported nfft"), (many, 2048, 2048, dict(ws=None), "workspace")):
        bufs.append(torch.full((2 * (F // 2 + 1),), CANARY, dtype=torch.float64, device=device))
        with pytest.raises((ValueError, _lib.DvhError), match=msg):
            _welch(xv, P, F, out=bufs[-1].view(2, -1), **kw)
    alias = x.reshape(-1).view(torch.float64)[:2 * 1025].view(2, 1025)
    with pytest.raises(_lib.DvhError, match="overlap"):
        _welch(x, 2048, 2048, out=alias)
    torch.cuda.synchronize()
    assert all(bool((b == CANARY).all()) for b in bufs) and bool((x == 1.0).all())
    assert ctypes.CDLL(_lib.LIB_PATH).dvh_abi_version() == 2


class _Win:
    def __init__(self, data):
        self.data = data


@pytest.mark.parametrize("name", ["a", "b"])
def test_win_avg_psd_matches_reference(device, name):
    """Class a: 5 500 samples, nperseg 2048 (fast form), windows of 6, 6, 4, 6, 6 rows (two launches, rows restored to
    the input order).  Class b: 2 000 samples, nperseg clipped (direct form)."""
    import torch

    from das_diff_veh_amd.modules.utils import win_avg_psd
    g = gio.load("psd")
    data = golden_windows(g, name)
    band = (g[f"{name}_f"] >= 2) & (g[f"{name}_f"] <= 25)
    ratio = float(g["band_ratio"]["ab".index(name)])
    tol = FAST_TOL if name == "a" else F64_TOL
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        f, avg, pxxs = win_avg_psd([_Win(d) for d in data], 250)
    assert len([r for r in rec if "nperseg" in str(r.message)]) == (0 if name == "a" else 1)
    assert f.dtype == avg.dtype == pxxs.dtype == np.float64
    assert np.array_equal(f, g[f"{name}_f"]) and pxxs.shape == g[f"{name}_pxxs"].shape
    for got, want in ((pxxs, g[f"{name}_pxxs"]), (avg[None], g[f"{name}_avg"][None])):
        err = _rel_err(got, want)
        rel = float((np.abs(got - want) / want)[:, band].max())
        print(f"class {name}: {err:.3g} of the maximum, {rel:.3g} per bin in 2-25 Hz (band ratio {ratio:.1f})")
        assert err <= tol and rel <= tol * ratio <= 1e-3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        f2, avg2, pxxs2 = win_avg_psd([_Win(torch.from_numpy(d).to(device)) for d in data], 250)
    assert np.array_equal(pxxs, pxxs2) and np.array_equal(avg, avg2) and np.array_equal(f, f2)


def _log_tol(lin, eps):
    """Bound on |10 log10(v + e) - 10 log10 v| for |e| <= eps at v >= lin > eps."""
    return 10.0 / np.log(10.0) * eps / (lin - eps)


@pytest.mark.parametrize("w", [500, 499])
def test_gather_spectra_match_reference(device, w):
    from das_diff_veh_amd.apis.virtual_shot_gather import VirtualShotGather, psd_vs_offset, spectrum_vs_offset
    g = gio.load("psd")
    xcf, x_axis, t_axis = gather(g, w)
    full = psd_ref.welch(xcf, psd_ref.sample_rate(t_axis), 256, 1024)[1]
    eps = FAST_TOL * full.max()               # every entry of the linear spectrum is within eps
    for k, kw in psd_cases(g, w):
        spec, freq, x, vmax, vmin = psd_vs_offset(xcf, x_axis, t_axis, **kw)
        want = g[f"g{w}_psd{k}_spec"]
        ref = psd_ref.psd_vs_offset(xcf, x_axis, t_axis, **kw)
        assert spec.shape == want.shape and np.array_equal(freq, ref[1]) and np.array_equal(x, ref[2])
        lin = (lambda a: 10.0 ** (a / 10.0)) if kw["log_scale"] else (lambda a: a)
        err = float((np.abs(lin(spec) - lin(want)).max(axis=1) / lin(want).max(axis=1)).max())
        print(f"gather {w} case {k}: {err:.3g} of the row maximum")
        assert err <= FAST_TOL
        for got, name, q in ((vmax, "vmax", kw["pclip"]), (vmin, "vmin", 100 - kw["pclip"])):
            wv = float(g[f"g{w}_psd{k}_{name}"])
            # an order statistic moves by at most the largest entry error; the log of one by _log_tol at its value
            low = np.percentile(full[:, :len(freq)], q, method="lower")
            assert abs(got - wv) <= (_log_tol(low, eps) if kw["log_scale"] else eps), (name, got, wv)
        given = psd_vs_offset(xcf, x_axis, t_axis, vmax=3.5, vmin=0, **kw)
        assert given[3] == 3.5 and given[4] == vmin       # 0 counts as not given
    mag, freq = spectrum_vs_offset(xcf, x_axis, t_axis)
    want = g[f"g{w}_spec"]
    assert mag.shape == want.shape and np.array_equal(freq, psd_ref.spectrum_vs_offset(xcf, t_axis)[1])
    err = float(np.abs(mag - want).max() / want.max())
    print(f"gather {w} spectrum: {err:.3g}")
    assert err <= F64_TOL
    obj = VirtualShotGather._from_arrays(None, xcf, x_axis, t_axis)
    a = obj.spec_vs_offset()
    b = psd_vs_offset(xcf, x_axis, t_axis, x_max=100, x_min=-100)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert np.array_equal(a[0], psd_vs_offset(xcf, x_axis, t_axis, **dict(psd_cases(g, w))[0])[0])
    assert np.array_equal(obj.spec_vs_offset(psd=False)[0], mag)
    with pytest.raises(NotImplementedError, match="spec_vs_offset"):
        obj.plot_spec_vs_offset()
    # no bin at or above fhi (above Nyquist): empty results
    spec, freq, x, vmax, vmin = psd_vs_offset(xcf, x_axis, t_axis, fhi=200)
    assert spec.shape == (len(x), 0) and freq.shape == (0,) and np.isnan(vmax) and np.isnan(vmin)
    mag, freq = spectrum_vs_offset(xcf, x_axis, t_axis, fhi=200)
    assert mag.shape == (49, 0) and freq.shape == (0,)
