"""Vehicle classes on the device: dvh_qs_curves and dvh_class_curve_stats against tests/classes_ref.py and NumPy, the
Python layer of das_diff_veh_amd.classes, and the notebooks' split end to end on tests/golden/classes.npz.

Tolerance: classes_ref.bound, the worst-case forward bound derived there from the coefficient magnitudes of the chain
(7.8e-12 max|x| at n_t = 1500); float32 input is compared against the chain on the upcast values with the same bound
(every device sum is float64 on the exact values).  The inputs are multiples of 2**-8, exact in float32, so one
reference serves both dtypes."""
import numpy as np
import pytest

from tests import classes_ref as cr
from tests import golden_io as gio

pytestmark = pytest.mark.gpu

T = 512  # DVH_QS_TILE (das_diff_veh_amd.classes.QS_TILE): interior outputs per block of the Savitzky-Golay stage
LENGTHS = (101, 102, 150, 151, 201, 202, 1500, 1501, T - 1, T, T + 1, T + 50, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 7)
CHANNELS = (1, 2, 3, 37, 63, 64, 65, 140)
OP = cr.operator(101, 3)
_TABS = {}


def _tabs(device, wlen=101, order=3):
    import torch
    if (wlen, order) not in _TABS:
        _TABS[(wlen, order)] = tuple(torch.from_numpy(a).to(device) for a in cr.operator(wlen, order))
    return _TABS[(wlen, order)]


def _states(seed, n_pass, n_ch, n_t):
    """Troughs of varied depth plus noise and a drift, as multiples of 2**-8 (float64 holding float32 values)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_t)
    depth = rng.uniform(0.5, 6.0, (n_pass, 1, 1))
    x = -depth * np.exp(-((t - n_t / 2) / (0.1 * n_t)) ** 2) + rng.uniform(-1, 1, (n_pass, n_ch, 1)) * t / n_t \
        + 0.3 * rng.standard_normal((n_pass, n_ch, n_t))
    return np.round(x * 2 ** 8) / 2 ** 8


def _qs(x, off, n_pass, n_ch, n_t, device, wlen=101, order=3, want_curves=True, stride=None, fill=-7.0):
    """dvh_qs_curves on the device tensor x with the row table off (host int64) -> (curves buffer [n_pass, stride] or
    None, peaks, status) as host arrays."""
    import torch

    from das_diff_veh_amd import _lib
    h, el, er = _tabs(device, wlen, order)
    stride = n_t if stride is None else stride
    curves = torch.full((max(n_pass, 1), stride), fill, dtype=torch.float64, device=device) if want_curves else None
    peaks = torch.full((max(n_pass, 1),), fill, dtype=torch.float64, device=device)
    status = torch.zeros(max(n_pass, 1), dtype=torch.int32, device=device)
    ws = torch.empty(max(_lib.load().dvh_qs_curves_workspace(n_pass, n_t) // 8, 1), dtype=torch.float64, device=device)
    off_d = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(device)
    _lib.call("dvh_qs_curves", _lib.ptr(x), 0 if x.dtype == torch.float32 else 1, _lib.ptr(off_d), n_pass, n_ch, n_t,
              _lib.ptr(h), wlen, _lib.ptr(el), _lib.ptr(er), _lib.ptr(curves), stride, _lib.ptr(peaks),
              _lib.ptr(status), _lib.ptr(ws), _lib.stream_of(device))
    torch.cuda.synchronize()
    return (None if curves is None else curves.cpu().numpy()), peaks.cpu().numpy(), status.cpu().numpy()


def _batch(x, device, dtype, **kw):
    import torch
    n_pass, n_ch, n_t = x.shape
    xd = torch.from_numpy(x.astype(dtype)).to(device)
    return _qs(xd, np.arange(n_pass * n_ch) * n_t, n_pass, n_ch, n_t, device, **kw)


@pytest.mark.parametrize("n_t", LENGTHS)
def test_kernel_matches_classes_ref(device, n_t):
    """Every time length at which the kernel takes another path (no interior at 101, first disjoint edge windows at
    202, the tile and the float32 chunk (2 T) boundaries) x every channel count, both dtypes, against the float64
    restatement within the derived bound; the peak is the curve's."""
    worst = 0.0
    for n_ch in CHANNELS:
        x = _states(n_t * 1000 + n_ch, 2, n_ch, n_t)
        want_c, want_p = cr.curves(x, *OP)
        tol = cr.bound(n_t, *OP, float(np.abs(x).max()))
        got = {}
        for dtype in (np.float64, np.float32):
            c, p, st = _batch(x, device, dtype)
            err = float(np.abs(c - want_c).max())
            worst = max(worst, err / tol)
            assert err <= tol, (n_ch, dtype, err, tol)
            assert np.array_equal(p, np.abs(c).max(-1)) and np.abs(p - want_p).max() <= tol
            assert not st.any() and np.all(c[:, 0] == 0.0)
            got[dtype] = c
        assert np.array_equal(got[np.float32], got[np.float64])  # the same values in either dtype: the same bits
    print(f"n_t {n_t}: worst error / bound {worst:.2e}")


@pytest.mark.parametrize("n_pass", [1, 2, 257])
def test_pass_counts(device, n_pass):
    x = _states(n_pass, n_pass, 5, 300)
    want_c, want_p = cr.curves(x, *OP)
    c, p, st = _batch(x, device, np.float64)
    tol = cr.bound(300, *OP, float(np.abs(x).max()))
    assert np.abs(c - want_c).max() <= tol and np.abs(p - want_p).max() <= tol and not st.any()


def test_no_pass_launches_nothing(device):
    import torch

    from das_diff_veh_amd import classes
    x = torch.zeros(8, dtype=torch.float64, device=device)
    c, p, st = _qs(x, np.zeros(0), 0, 5, 300, device)
    assert np.all(c == -7.0) and np.all(p == -7.0)
    c, p = classes.quasi_static_curves(torch.zeros((0, 5, 300), device=device))
    assert c.is_cuda and c.shape[0] == 0 and p.shape == (0,) and p.dtype == torch.float64


def test_other_windows_match_scipy(device):
    """(5, 2) and the longest window the kernel takes against SciPy itself (benign designs: SciPy's edge fit is clean)."""
    import scipy.signal

    from das_diff_veh_amd import classes
    rng = np.random.default_rng(12)
    for wlen, order, n_t in ((5, 2, 64), (classes.QS_MAX_WLEN, 3, 700)):
        x = rng.standard_normal((3, 4, n_t))
        c, p = classes.quasi_static_curves(x, wlen, order)
        want = np.stack([scipy.signal.detrend(scipy.signal.savgol_filter(d.mean(0), wlen, order)) for d in x])
        want = want - want[:, :1]
        op = cr.operator(wlen, order)
        assert np.abs(c - want).max() <= cr.bound(n_t, *op, float(np.abs(x).max()))


def _record(dtype, n_rows=9, rec_n_t=1400, seed=3):
    rng = np.random.default_rng(seed)
    rec = np.round((rng.standard_normal((n_rows, rec_n_t)) + np.linspace(0, 2, rec_n_t)) * 2 ** 8) / 2 ** 8
    return rec.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_record_mode(device, dtype):
    """Rows read from a record through the table: consecutive rows start one sample apart (every alignment mod 4
    elements), passes overlap (3 samples apart), and the last pass's last row ends on the record's last sample.  The
    curves equal those of the gathered batch bit for bit."""
    import torch
    n_rows, rec_n_t, n_ch, n_t, row_stride = 9, 1400, 7, 600, 1403
    rec = _record(dtype, n_rows, rec_n_t)
    buf = torch.zeros((n_rows - 1) * row_stride + rec_n_t, dtype=torch.from_numpy(rec).dtype, device=device)
    torch.as_strided(buf, (n_rows, rec_n_t), (row_stride, 1)).copy_(torch.from_numpy(rec))  # ends on the last sample
    n_pass = 6
    ch0 = n_rows - n_ch
    t_start = np.array([[3 * p + c for c in range(n_ch)] for p in range(n_pass)])
    t_start[-1] += rec_n_t - n_t - t_start[-1, -1]          # the last row of the last pass ends on the last sample
    off = (ch0 + np.arange(n_ch))[None, :] * row_stride + t_start
    assert t_start[-1, -1] + n_t == rec_n_t and {int(v) % 4 for v in off.ravel()} == {0, 1, 2, 3}
    c, p, st = _qs(buf, off, n_pass, n_ch, n_t, device)
    x = np.stack([np.stack([rec[ch0 + k, t_start[q, k]:t_start[q, k] + n_t] for k in range(n_ch)])
                  for q in range(n_pass)]).astype(np.float64)
    want_c, want_p = cr.curves(x, *OP)
    tol = cr.bound(n_t, *OP, float(np.abs(x).max()))
    assert np.abs(c - want_c).max() <= tol and np.abs(p - want_p).max() <= tol and not st.any()
    cb, pb, _ = _batch(x, device, dtype)
    assert np.array_equal(c, cb) and np.array_equal(p, pb)


def test_null_curves_and_wide_stride(device):
    x = _states(21, 3, 4, 700)
    c, p, st = _batch(x, device, np.float64)
    c0, p0, st0 = _batch(x, device, np.float64, want_curves=False)
    assert c0 is None and np.array_equal(p0, p) and np.array_equal(st0, st)
    cw, pw, _ = _batch(x, device, np.float64, stride=700 + 13)
    assert np.array_equal(cw[:, :700], c) and np.all(cw[:, 700:] == -7.0) and np.array_equal(pw, p)


def test_position_batch_size_and_source_do_not_change_a_pass(device):
    """One pass at position 0 of 1, at position 200 of 257, and read from a record: bit-identical curve and peak."""
    import torch
    n_ch, n_t = 6, 1100
    one = _states(77, 1, n_ch, n_t)
    c1, p1, _ = _batch(one, device, np.float64)
    many = _states(78, 257, n_ch, n_t)
    many[200] = one[0]
    cm, pm, _ = _batch(many, device, np.float64)
    assert np.array_equal(cm[200], c1[0]) and pm[200] == p1[0]
    rec = _record(np.float64, n_ch + 2, n_t + 40, seed=5)
    t_start = 5 + 3 * np.arange(n_ch)
    for k in range(n_ch):
        rec[1 + k, t_start[k]:t_start[k] + n_t] = one[0, k]
    off = (1 + np.arange(n_ch)) * rec.shape[1] + t_start
    cr_, pr_, _ = _qs(torch.from_numpy(rec).to(device), off[None, :], 1, n_ch, n_t, device)
    assert np.array_equal(cr_[0], c1[0]) and pr_[0] == p1[0]


def test_non_finite_passes_are_flagged_and_contained(device):
    from das_diff_veh_amd import classes
    x = _states(31, 6, 5, 400)
    clean_c, clean_p, _ = _batch(x, device, np.float64)
    bad = x.copy()
    bad[1, 2, 17] = np.nan
    bad[3, 0, 399] = np.inf
    bad[4, 4, 200] = -np.inf
    for dtype in (np.float64, np.float32):
        c, p, st = _batch(bad, device, dtype)
        assert st.tolist() == [0, 1, 0, 1, 1, 0]
        assert np.isnan(p).tolist() == [False, True, False, True, True, False]
        for k in (0, 2, 5):
            assert np.array_equal(c[k], clean_c[k]) and p[k] == clean_p[k]
    with pytest.raises(ValueError, match=r"array must not contain infs or NaNs \(pass 1\)"):
        classes.quasi_static_curves(bad)
    with pytest.raises(ValueError, match=r"array must not contain infs or NaNs \(pass 3\)"):
        classes.quasi_static_curves(bad[[0, 2, 5, 3, 1]])
    c, p, failed = classes.quasi_static_curves(bad, skip_failed=True)
    assert sorted(failed) == [1, 3, 4] and all("infs or NaNs" in r for r in failed.values())
    assert np.isnan(p).tolist() == [False, True, False, True, True, False] and np.array_equal(c[0], clean_c[0])
    want_c, want_p = cr.curves(bad, *OP)
    assert np.array_equal(np.isnan(want_p), np.isnan(p))


def test_refusals_launch_nothing(device):
    import torch

    from das_diff_veh_amd import _lib, classes
    x = torch.ones((2, 3, 300), dtype=torch.float64, device=device)
    off = np.arange(6) * 300
    for kw, n_ch, n_t in ((dict(wlen=100), 3, 300), (dict(wlen=classes.QS_MAX_WLEN + 2), 3, 300), (dict(), 3, 100),
                          (dict(), 0, 300)):
        wlen = kw.get("wlen", 101)
        tabs = torch.zeros(3 * 300 * 300, dtype=torch.float64, device=device)
        curves = torch.full((2, 300), -7.0, dtype=torch.float64, device=device)
        peaks = torch.full((2,), -7.0, dtype=torch.float64, device=device)
        status = torch.full((2,), 5, dtype=torch.int32, device=device)
        ws = torch.full((2 * 2 * 300,), -7.0, dtype=torch.float64, device=device)
        off_d = torch.from_numpy(off).to(device)
        with pytest.raises(ValueError):
            _lib.call("dvh_qs_curves", _lib.ptr(x), 1, _lib.ptr(off_d), 2, n_ch, n_t, _lib.ptr(tabs), wlen,
                      _lib.ptr(tabs), _lib.ptr(tabs), _lib.ptr(curves), 300, _lib.ptr(peaks), _lib.ptr(status),
                      _lib.ptr(ws), _lib.stream_of(device))
        torch.cuda.synchronize()
        assert bool((curves == -7.0).all()) and bool((peaks == -7.0).all()) and bool((status == 5).all())
        assert bool((ws == -7.0).all()) and bool((x == 1.0).all())


@pytest.mark.parametrize("n_t", [1, 63, 64, 65, 1500])
def test_class_curve_stats_match_numpy(device, n_t):
    """Classes of 1, 2 and 100 passes, an empty class and passes in no class.  Tolerances from the formats: the mean of
    n values summed in any order errs by at most (n - 1) u max|x| (NumPy adds rows in order for n_t > 1 and pairwise
    for n_t = 1), two evaluations by twice that; the std is a 2-norm of the deviations, so it moves by at most the
    deviations' error (the mean's, plus u |x|) plus the relative n u / 2 of its own sum: 2 (2 n + 4) u max|x| covers
    both sides."""
    import torch

    from das_diff_veh_amd import classes
    rng = np.random.default_rng(n_t)
    n_pass = 110
    curves = rng.standard_normal((n_pass, n_t)) * 3
    perm = rng.permutation(n_pass)
    split = classes.ClassSplit(("one", "two", "none", "hundred"),
                               (perm[:1], np.sort(perm[1:3]), np.zeros(0, dtype=np.int64), np.sort(perm[3:103])), {})
    for src in (curves, torch.from_numpy(curves).to(device)):
        mean, std, count = classes.class_curve_stats(src, split)
        if isinstance(mean, torch.Tensor):
            assert mean.is_cuda
            mean, std, count = mean.cpu().numpy(), std.cpu().numpy(), count.cpu().numpy()
        assert count.tolist() == [1, 2, 0, 100] and mean.shape == std.shape == (4, n_t)
        amax = float(np.abs(curves).max())
        for k, idx in enumerate(split.indices):
            if idx.size == 0:
                assert np.isnan(mean[k]).all() and np.isnan(std[k]).all()
                continue
            state = [curves[i] for i in idx]
            n = len(state)
            assert np.abs(mean[k] - np.mean(state, axis=0)).max() <= 2 * n * cr.U * amax
            assert np.abs(std[k] - np.std(state, axis=0)).max() <= 2 * (2 * n + 4) * cr.U * amax
        assert np.array_equal(mean[0], curves[perm[0]]) and np.all(std[0] == 0.0)


@pytest.fixture(scope="module")
def golden():
    g = gio.load("classes")
    return g, g["q"].astype(np.float32) / np.float32(2 ** 8)


def test_golden_split_end_to_end(device, golden):
    """Device peaks -> the notebooks' index arrays, for both notebooks' order of cells; the cell-11 curves."""
    import torch

    from das_diff_veh_amd import classes
    g, states = golden
    speed = g["veh_speed"]
    curves, peaks = classes.quasi_static_curves(torch.from_numpy(states).to(device))      # speed notebook: cell 5
    assert curves.is_cuda and peaks.is_cuda and curves.dtype == torch.float64
    tol = cr.bound(states.shape[-1], *OP, float(np.abs(states).max()))
    assert np.abs(curves.cpu().numpy() - g["s_mean"]).max() <= tol
    peaks = peaks.cpu().numpy()
    major = classes.peak_majority(peaks)                                                   # cell 6
    assert np.array_equal(major.indices[0], g["s_peak_idx"])
    sp = classes.speed_classes(speed[major.indices[0]])                                    # cell 8
    for name in sp.names:
        assert np.array_equal(sp[name], g[f"s_{name}_idx"])
    mean, std, count = classes.class_curve_stats(curves, sp)                               # cells 9, 11
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    for k, name in enumerate(sp.names):
        assert np.abs(mean[k] - g[f"s_mean_{name}"]).max() <= 2 * tol
    assert np.abs(std[2] - g["s_std_slow"]).max() <= 4 * tol
    kept = classes.speed_majority(speed).indices[0]                                        # weight notebook: cell 5
    assert np.array_equal(kept, g["w_speed_idx"])
    host_curves, host_peaks = classes.quasi_static_curves([states[i] for i in kept])       # cell 7, the list form
    assert isinstance(host_curves, np.ndarray) and np.abs(host_curves - g["w_mean"]).max() <= tol
    assert np.array_equal(host_peaks, peaks[kept])                                         # a pass is a pass
    w = classes.weight_classes(host_peaks)                                                 # cell 8
    for k, name in enumerate(w.names):
        assert np.array_equal(w[name], g[f"w_{name}_idx"])
    mean, std, _ = classes.class_curve_stats(host_curves, w)
    for k, name in enumerate(w.names):
        assert np.abs(mean[k] - g[f"w_mean_{name}"]).max() <= 2 * tol
        assert np.abs(std[k] - g[f"w_std_{name}"]).max() <= 4 * tol


def test_mixed_shapes_come_back_in_the_callers_order(device):
    from das_diff_veh_amd import classes
    a, b, c = _states(1, 2, 3, 200), _states(2, 2, 4, 260), _states(3, 1, 3, 200)
    states = [a[0], b[0], a[1].astype(np.float32), b[1], c[0], (a[0] * 256).astype(np.int16)]
    curves, peaks = classes.quasi_static_curves(states)
    assert isinstance(curves, list) and [len(x) for x in curves] == [200, 260, 200, 260, 200, 200]
    for x, got, pk in zip(states, curves, peaks):
        want_c, want_p = cr.curves(x.astype(np.float64), *OP)
        tol = cr.bound(x.shape[-1], *OP, float(np.abs(x).max()))
        assert np.abs(got - want_c).max() <= tol and abs(pk - want_p) <= tol
    assert np.array_equal(curves[5], 256.0 * curves[0])  # int16 goes through float64; a power of two scales exactly


def test_stacked_on_the_subset_equals_the_goldens_slots(device, golden):
    """engine.stacked on split.subset() of the device peaks' classes against stacked with slots built from the golden
    index arrays: the same windows in the same classes.  A class of more than one chunk of 8 passes is summed over
    its chunks by float32 atomics, whose order varies from run to run, so two runs agree up to that order: at most
    (chunks - 1) 2^-24 sum |chunk sums| per sample, 14 chunks for the 105 passes here; 64 x 2^-24 of the largest
    sample leaves a factor 4 for cancellation between chunks."""
    import torch

    from das_diff_veh_amd import classes, engine
    from das_diff_veh_amd.apis.data_classes import SurfaceWaveWindow
    from das_diff_veh_amd.plan import VsgParams
    g, states = golden
    _, peaks = classes.quasi_static_curves(states)
    major = classes.peak_majority(peaks).indices[0]
    sel, slots, n_slot = classes.speed_classes(g["veh_speed"][major]).subset()
    want_slots = np.full(major.size, -1)
    for k, name in enumerate(("fast", "mid", "slow")):
        want_slots[g[f"s_{name}_idx"]] = k
    assert n_slot == 3 and np.array_equal(sel, np.arange(major.size)) and np.array_equal(slots, want_slots)
    v = gio.load("vsg_w500")
    base = [SurfaceWaveWindow(**gio.pass_arrays(v, i)) for i in range(min(gio.n_pass(v), 3))]
    windows = [base[i % len(base)] for i in range(major.size)]
    prm = VsgParams(include_other_side=True, norm=False, pivot=700, start_x=500, end_x=900, wlen=2)
    got, _ = engine.stacked([windows[i] for i in sel], prm, slots, n_slot, device=device)
    want, _ = engine.stacked(windows, prm, want_slots, 3, device=device)
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    assert float((got - want).abs().max()) <= 64 * 2.0 ** -24 * float(want.abs().max())


def test_from_a_record_equals_the_numpy_gather(device):
    """A synthetic record: noise plus vehicles on linear trajectories with planted trough depths.  The curves equal
    the NumPy gather + chain, the peaks rank the passes by depth, and a vehicle that passes after the record's end is
    reported invalid, not raised."""
    import torch

    from das_diff_veh_amd import classes
    rng = np.random.default_rng(41)
    n_ch, n_T, dt, pivot, v = 40, 9000, 0.004, 560.0, 22.0
    x_axis = 400.0 + 8.16 * np.arange(n_ch)
    t_axis = 3.0 + dt * np.arange(n_T)
    depths = [2.0, 0.7, 3.5, 1.3]
    tcs = [11.0, 17.0, 23.0, 29.0]
    rec = 0.05 * rng.standard_normal((n_ch, n_T))
    for d, tc in zip(depths, tcs):
        xc = pivot + v * (t_axis - tc)
        rec -= d * np.exp(-((x_axis[:, None] - xc[None, :]) / 15.0) ** 2)
    rec = (np.round(rec * 2 ** 10) / 2 ** 10).astype(np.float32)
    xs = np.arange(380.0, 760.0)
    tracks = [(xs, tc + (xs - pivot) / v) for tc in tcs] + [(xs, 60.0 + (xs - pivot) / v)]
    start_x, end_x, n_t = 480.0, 640.0, 1500
    rec_d = torch.from_numpy(rec).to(device)
    curves, peaks, valid = classes.quasi_static_curves_from_record(rec_d, x_axis, t_axis, tracks, start_x, end_x, n_t)
    assert valid.tolist() == [True, True, True, True, False] and curves.is_cuda and tuple(curves.shape) == (4, n_t)
    states = []
    for trk in tracks[:4]:
        ch0, nc, ts, ok = cr.states_table(x_axis, t_axis, trk, start_x, end_x, n_t)
        assert ok
        states.append(cr.gather_states(rec, ch0, nc, ts, n_t))
    x = np.stack(states).astype(np.float64)
    want_c, want_p = cr.curves(x, *OP)
    tol = cr.bound(n_t, *OP, float(np.abs(x).max()))
    assert np.abs(curves.cpu().numpy() - want_c).max() <= tol and np.abs(peaks.cpu().numpy() - want_p).max() <= tol
    assert np.argsort(peaks.cpu().numpy()).tolist() == np.argsort(depths).tolist()
    batch_c, batch_p = classes.quasi_static_curves(torch.from_numpy(x.astype(np.float32)).to(device))
    assert torch.equal(batch_c, curves) and torch.equal(batch_p, peaks)
    host = classes.quasi_static_curves_from_record(rec, x_axis, t_axis, tracks, start_x, end_x, n_t, return_curves=False)
    assert host[0] is None and isinstance(host[1], np.ndarray) and np.array_equal(host[1], peaks.cpu().numpy())
