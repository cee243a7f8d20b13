"""GPU parity of the tracking-grid preprocessing (TimeLapseImaging._preprocess_for_tracking,
apis/timeLapseImaging.py:74-102): the three kernels of dvh_track.hip through the C ABI against NumPy / SciPy, the two
band-passes in isolation and the whole chain against the reference's outputs (tests/golden/tracking_prep*.npz), and
the TimeLapseImaging methods built on it.

Bounds: the median, the gate and the transpose are exact; the resampler is a <= 31-tap float64 dot product, held to
1e-13 max|ref| (gamma_31 sum|h||x| is two orders below); each band-pass is held to the project's 1e-10 max|ref|; the
chain to the two filter contracts added, 1e-10 (max|after the time band-pass| + max|final|), the unit-passband linear
stages after the first filter not amplifying its error."""
import numpy as np
import pytest
import scipy.signal

from tests import golden_io as gio
from tests import tracking_ref as tr

pytestmark = pytest.mark.gpu
CASES = ["plain", "loud", "dead_first_loud", "two_loud_last"]
LEVEL = 10.0


@pytest.fixture(scope="module")
def head():
    return gio.load("tracking_prep")


@pytest.fixture(scope="module")
def loud_stages():
    return gio.load("tracking_prep_loud_stages")


def _golden(case):
    return gio.load("tracking_prep_" + case)["data_for_tracking"]


_BOUNDS = {}


def _chain_bound(case, head):
    """1e-10 (max|bp| + max|final|) from the reference: bp restated by the helper (pinned to the golden at 1e-13)."""
    if case not in _BOUNDS:
        d, _, _ = tr.gate(head[case + "_in"])
        tr.impute_empty(d)
        bp = scipy.signal.sosfiltfilt(tr.butter_sos(float(head["dt"]), 0.08, 1), d, axis=1)
        _BOUNDS[case] = 1e-10 * (np.abs(bp).max() + np.abs(_golden(case)).max())
    return _BOUNDS[case]


# ------------------------------------------------------------------------------------------ the gate alone

def _gate_row(kind, n_t, dtype, rng):
    """One trace of the kind: 0 heavy ties, 1 all equal, 2 median exactly LEVEL, 3 median one step above LEVEL,
    4 holds a NaN, 5 loud, 6 quiet with -0.0."""
    sign = rng.choice([-1.0, 1.0], n_t)
    if kind == 0:
        return (rng.choice([0.5, 1.0, 1.5, 2.0], n_t) * sign).astype(dtype)
    if kind == 1:
        return np.full(n_t, -3.25, dtype)
    if kind in (2, 3):
        v = dtype(LEVEL) if kind == 2 else np.nextafter(dtype(LEVEL), dtype(np.inf))
        n_lo = (n_t - 1) // 2
        n_mid = 1 if n_t % 2 else 2
        lo = rng.uniform(0, 9, n_lo).astype(dtype)
        if n_lo > 3:
            lo[0], lo[1], lo[2] = -0.0, lo[3], 0.0  # -0.0 and a tie below the median
        hi = rng.uniform(11, 30, n_t - n_lo - n_mid).astype(dtype)
        row = np.concatenate([lo, np.full(n_mid, v, dtype), hi]) * sign.astype(dtype)
        return row[rng.permutation(n_t)]
    if kind == 4:
        row = (rng.standard_normal(n_t) * 20).astype(dtype)
        row[n_t // 3] = np.nan
        return row
    if kind == 5:
        return (rng.standard_normal(n_t) * 20).astype(dtype)
    row = rng.standard_normal(n_t).astype(dtype)
    row[0] = -0.0
    return row


GATE_SHAPES = {(5, 1): [1, 2, 3, 4, 6], (5, 2): [1, 2, 3, 4, 6], (7, 255): range(7), (7, 256): range(7),
               (3, 1501): [2, 3, 4], (4, 15000): [0, 2, 3, 5]}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", list(GATE_SHAPES))
def test_median_abs_gate(device, shape, dtype):
    import torch

    from das_diff_veh_amd import _lib
    n_rows, n_t = shape
    rng = np.random.default_rng(n_t)
    pad = 3
    buf = np.full((n_rows, n_t + pad), 4.5, dtype)
    for r, kind in enumerate(GATE_SHAPES[shape]):
        buf[r, :n_t] = _gate_row(kind, n_t, dtype, rng)
    x = buf[:, :n_t]
    with np.errstate(invalid="ignore"):
        med = np.median(np.abs(x.astype(np.float64)), axis=-1)  # float64 input: np.median(np.abs(x), -1) itself
    gated = med > LEVEL
    want = buf.copy()
    want[:, :n_t][gated] *= 0
    for r, kind in enumerate(GATE_SHAPES[shape]):  # the rows are what their kind says
        assert gated[r] == (kind in (3, 5)), (kind, med[r])
        assert np.isnan(med[r]) == (kind == 4)
        if kind == 2:
            assert med[r] == LEVEL
    dev = torch.from_numpy(buf).to(device)
    med_t = torch.full((n_rows,), -1.0, dtype=torch.float64, device=device)
    gated_t = torch.full((n_rows,), -1, dtype=torch.int32, device=device)
    _lib.call("dvh_median_abs_gate", _lib.ptr(dev), 0 if dtype == np.float32 else 1, n_rows, dev.stride(0), n_t, LEVEL,
              _lib.ptr(med_t), _lib.ptr(gated_t), _lib.stream_of(device))
    got_med = med_t.cpu().numpy()
    assert np.array_equal(np.isnan(got_med), np.isnan(med))
    ok = ~np.isnan(med)
    assert np.array_equal(got_med[ok].view(np.uint64), med[ok].view(np.uint64))  # bit-equal
    assert np.array_equal(gated_t.cpu().numpy(), gated.astype(np.int32))
    bits = np.uint32 if dtype == np.float32 else np.uint64
    assert np.array_equal(dev.cpu().numpy().view(bits), want.view(bits))  # zeroed rows (-0.0 too), the rest and the pad

    # nullable outputs: the same rows without them
    dev2 = torch.from_numpy(buf).to(device)
    _lib.call("dvh_median_abs_gate", _lib.ptr(dev2), 0 if dtype == np.float32 else 1, n_rows, dev2.stride(0), n_t,
              LEVEL, None, None, _lib.stream_of(device))
    assert np.array_equal(dev2.cpu().numpy().view(bits), want.view(bits))


# ------------------------------------------------------------------------------------------ the resampler alone

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("up,down", [(204, 25), (3, 2), (2, 3)])
def test_resample_rows_t(device, up, down, dtype):
    import torch

    from das_diff_veh_amd import _lib
    from das_diff_veh_amd.preprocess import _resampler
    up_r, down_r, half_len, h_t = _resampler(up, down, device)
    assert (up_r, down_r) == (up, down) and h_t.numel() == 2 * half_len + 1
    rng = np.random.default_rng(up)
    pad = 5
    for n_in in (1, 2, 11, 24, 65):
        n_out = -(-n_in * up // down)
        for t_step in (1, 5):
            for n_t_out in (1, 63, 300):
                n_t = (n_t_out - 1) * t_step + 1 + (t_step > 1)  # one sample past the last one read
                x = rng.standard_normal((n_in, n_t)).astype(dtype)
                ref = scipy.signal.resample_poly(x[:, ::t_step][:, :n_t_out].astype(np.float64), up, down, axis=0).T
                assert ref.shape == (n_t_out, n_out)
                xd = torch.from_numpy(x).to(device)
                out = torch.full((n_t_out, n_out + pad), 7.25, dtype=torch.float64, device=device)
                _lib.call("dvh_resample_rows_t", _lib.ptr(xd), 0 if dtype == np.float32 else 1, n_in, xd.stride(0),
                          t_step, n_t_out, _lib.ptr(h_t), half_len, up, down, _lib.ptr(out), out.stride(0), n_out,
                          _lib.stream_of(device))
                got = out.cpu().numpy()
                err = np.abs(got[:, :n_out] - ref).max()
                assert err <= 1e-13 * np.abs(ref).max(), (n_in, t_step, n_t_out, err)
                assert np.all(got[:, n_out:] == 7.25)  # the padding of out_stride is left alone


def test_resample_rows_t_rejects_a_wrong_n_out(device):
    import torch

    from das_diff_veh_amd import _lib
    from das_diff_veh_amd.preprocess import _resampler
    up, down, half_len, h_t = _resampler(204, 25, device)
    x = torch.ones((24, 10), dtype=torch.float64, device=device)
    out = torch.full((10, 200), 7.25, dtype=torch.float64, device=device)
    lib = _lib.load()
    for n_out in (195, 197):
        rc = lib.dvh_resample_rows_t(_lib.ptr(x), 1, 24, x.stride(0), 1, 10, _lib.ptr(h_t), half_len, up, down,
                                     _lib.ptr(out), out.stride(0), n_out, _lib.stream_of(device))
        assert rc == -2 and b"n_out" in lib.dvh_last_error()
    with pytest.raises(_lib.DvhError):
        _lib.call("dvh_resample_rows_t", _lib.ptr(x), 1, 24, x.stride(0), 1, 10, _lib.ptr(h_t), half_len, up, down,
                  _lib.ptr(out), out.stride(0), 195, _lib.stream_of(device))
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())  # nothing was launched


# ------------------------------------------------------------------------------------------ the transpose

@pytest.mark.parametrize("n_rows,n_cols", [(1, 1), (63, 65), (300, 196)])
def test_transpose_f64(device, n_rows, n_cols):
    import torch

    from das_diff_veh_amd import _lib
    rng = np.random.default_rng(n_rows)
    src = rng.standard_normal((n_rows, n_cols + 3))
    sd = torch.from_numpy(src).to(device)
    dst = torch.full((n_cols, n_rows + 2), 7.25, dtype=torch.float64, device=device)
    _lib.call("dvh_transpose_f64", _lib.ptr(sd), n_rows, n_cols, sd.stride(0), _lib.ptr(dst), dst.stride(0),
              _lib.stream_of(device))
    got = dst.cpu().numpy()
    assert np.array_equal(got[:, :n_rows], src[:, :n_cols].T)
    assert np.all(got[:, n_rows:] == 7.25)


# ------------------------------------------------------------------------------------------ the filters in isolation

def test_time_bandpass_of_the_loud_case(device, head, loud_stages):
    import torch

    from das_diff_veh_amd.preprocess import bandpass_inplace
    d, _, gated = tr.gate(head["loud_in"])
    imputed = tr.impute_empty(d)
    assert gated.tolist() == [9] and imputed == 9
    t = torch.from_numpy(d).to(device)
    bandpass_inplace(t, float(head["dt"]), 0.08, 1)
    ref = loud_stages["bp"]
    err = np.abs(t.cpu().numpy() - ref).max()
    print(f"time band-pass: {err:.3e} of max {np.abs(ref).max():.3e}")
    assert err <= 1e-10 * np.abs(ref).max()


def test_space_bandpass_of_the_loud_case(device, head, loud_stages):
    import torch

    from das_diff_veh_amd.preprocess import bandpass_inplace
    dist = head["loud_dist"]
    t = torch.from_numpy(np.ascontiguousarray(loud_stages["rs"].T)).to(device)
    bandpass_inplace(t, dist[1] - dist[0], 0.006, 0.04)
    ref = _golden("loud")
    err = np.abs(t.cpu().numpy().T - ref).max()
    print(f"space band-pass: {err:.3e} of max {np.abs(ref).max():.3e}")
    assert err <= 1e-10 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------ the chain

@pytest.mark.parametrize("case", CASES)
def test_tracking_preprocessing(device, head, case):
    from das_diff_veh_amd.preprocess import tracking_preprocessing
    x = head[case + "_in"].astype(np.float64)
    keep = x.copy()
    got, dist, step, info = tracking_preprocessing(x, float(head["dt"]), head["x_axis"][0], return_info=True)
    ref = _golden(case)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == ref.shape
    err, bound = np.abs(got - ref).max(), _chain_bound(case, head)
    print(f"{case}: |got - ref|max = {err:.3e}, bound {bound:.3e}, max|final| {np.abs(ref).max():.3e}")
    assert err <= bound
    assert np.array_equal(dist, head[case + "_dist"])
    assert np.array_equal(head["t_axis"][::step], head[case + "_t_axis_tracking"])
    assert info["gated"].tolist() == head[case + "_gated"].tolist() and info["imputed"] == int(head[case + "_imputed"])
    assert np.array_equal(x, keep)


def test_tracking_preprocessing_device_tensor(device, head):
    import torch

    from das_diff_veh_amd.preprocess import tracking_preprocessing
    t = torch.as_tensor(head["loud_in"].astype(np.float64), device=device)
    keep = t.clone()
    got, dist, step = tracking_preprocessing(t, float(head["dt"]), head["x_axis"][0])
    assert got.is_cuda and got.dtype == torch.float64 and step == 5
    assert np.abs(got.cpu().numpy() - _golden("loud")).max() <= _chain_bound("loud", head)
    assert np.array_equal(dist, head["loud_dist"])
    assert torch.equal(t, keep)


@pytest.mark.parametrize("case", CASES)
def test_tracking_preprocessing_float32_record(device, head, case):
    """A float32 record is promoted at entry: the same values as the golden's float64 run, the same bound."""
    from das_diff_veh_amd.preprocess import tracking_preprocessing
    x = head[case + "_in"]
    assert x.dtype == np.float32
    got, _, _ = tracking_preprocessing(x, float(head["dt"]), head["x_axis"][0])
    assert got.dtype == np.float64
    assert np.abs(got - _golden(case)).max() <= _chain_bound(case, head)
    assert np.array_equal(x, head[case + "_in"])


def test_tracking_preprocessing_without_the_space_filter(device, head, loud_stages):
    from das_diff_veh_amd.preprocess import tracking_preprocessing
    got, _, _ = tracking_preprocessing(head["loud_in"], float(head["dt"]), head["x_axis"][0], flo_space=-1,
                                       fhi_space=-1)
    ref = loud_stages["rs"]
    assert np.abs(got - ref).max() <= 1e-10 * (np.abs(loud_stages["bp"]).max() + np.abs(ref).max())


def test_padlen_errors(device, head):
    from das_diff_veh_amd.preprocess import tracking_preprocessing
    x = head["plain_in"]
    for bad in (x[:7], x[:, :60]):
        with pytest.raises(ValueError, match="must be greater than padlen, which is 63"):
            tracking_preprocessing(bad, float(head["dt"]), 449)
    got, _, _ = tracking_preprocessing(x[:8, :64], float(head["dt"]), 449)  # the smallest record that passes
    assert got.shape == (66, 13)


# ------------------------------------------------------------------------------------------ TimeLapseImaging

def test_time_lapse_imaging_tracking_flow(device):
    from das_diff_veh_amd.apis.timeLapseImaging import TimeLapseImaging
    from das_diff_veh_amd.preprocess import tracking_preprocessing
    c = gio.select_cases()["short"]
    x_axis = gio.load("tli")["x_axis"]
    obj = TimeLapseImaging(c["rec"].copy(), x_axis, c["t_axis"])
    assert not hasattr(obj, "data_for_tracking")  # the constructor still skips the tracking preprocessing
    # the case's tracks (time indices on its 0.012 s tracking axis) on the 50 Hz grid preprocess_for_tracking leaves
    vs = np.round(c["veh_states"] * 0.012 / 0.02)
    with pytest.raises(AttributeError):
        obj.set_veh_states(vs, c["start_x_tracking"])
    obj.preprocess_for_tracking()
    want, dist, step = tracking_preprocessing(c["rec"], obj.dt, x_axis[0])
    assert np.array_equal(obj.data_for_tracking, want) and want.shape == (392, 1200)
    assert np.array_equal(obj.dist_along_fiber_tracking, dist)
    assert np.array_equal(dist, np.arange(392) + (x_axis[0] - 400) * 8.16)
    assert np.array_equal(obj.t_axis_tracking, c["t_axis"][::5]) and step == 5
    obj.set_veh_states(vs, c["start_x_tracking"])
    assert obj.start_x == c["start_x_tracking"] and obj.end_x is None
    obj.select_surface_wave_windows(c["x0"], **c["kw"])
    assert len(obj.sw_selector) > 0 and len(obj.sw_selector) == len(obj.qs_selector)
    assert obj.sw_selector.windows[0].t_axis_tracking is obj.t_axis_tracking


def test_preprocess_for_tracking_reads_the_band_edges(device, head):
    from das_diff_veh_amd.apis.timeLapseImaging import TimeLapseImaging
    from das_diff_veh_amd.preprocess import tracking_preprocessing
    kw = dict(flo=0.1, fhi=2, flo_space=-1, fhi_space=-1)
    obj = TimeLapseImaging(head["plain_in"].astype(np.float64), head["x_axis"], head["t_axis"],
                           tracking_preprecessing_dict=kw)
    obj.preprocess_for_tracking(subsamp_factor=4, noise_level=5, channel0=440)
    want, dist, _ = tracking_preprocessing(head["plain_in"], float(head["dt"]), 449, subsamp_factor=4, noise_level=5,
                                           channel0=440, **kw)
    assert np.array_equal(obj.data_for_tracking, want) and want.shape == (196, 375)
    assert np.array_equal(obj.dist_along_fiber_tracking, dist) and dist[0] == 9 * 8.16
    assert np.array_equal(obj.t_axis_tracking, head["t_axis"][::4])
