"""GPU parity of the vehicle tracker (KF_tracking, apis/tracking.py): the three kernels of dvh_tracker.hip through the
C ABI against SciPy and tests/tracker_ref.py, the KF_tracking drop-in against the reference's outputs
(tests/golden/tracker_*.npz), and TimeLapseImaging.track_vehicles / DeviceTracker built on it.

Bounds: peak indices, counts, matches and NaN patterns are exact.  The random rows are distinct multiples of 2**-8, so
no two peaks tie (the order of equal heights under the distance rule is not pinned) and the prominence subtraction is
exact.  The detection curve is a sum of at most a few hundred positive terms, each good to a few ulp: the true bound is
near 1e-13 max|ref| and 1e-12 leaves a decade for the device exp.  The final tracks are integers and np.interp of
integers; they are held to 1e-9.  The fixture's grids are free of equal-height peaks that the distance rule would
have to order (tests/golden/make_golden_tracker.py asserts it), so SciPy's result on them is unique."""
import numpy as np
import pytest
import scipy.signal
import scipy.stats

from tests import golden_io as gio
from tests import tracker_ref as kr

pytestmark = pytest.mark.gpu
GUARD = 16
FILL = -7


# ------------------------------------------------------------------------------------------ helpers

def _find_peaks(x, n_t=None, row0=0, row_step=1, n_sel=None, sign=1, distance=0.0, prominence=None, wlen=0.0,
                cap=None, want_prom=False):
    """dvh_find_peaks_rows on the rows of the 2-D host array x -> (peak lists, counts, status, prominences or None,
    the raw [n_sel, cap] peaks buffer); every buffer ends in a guard region that must come back untouched."""
    import torch

    from das_diff_veh_amd import _lib
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n_t = x.shape[1] if n_t is None else n_t
    n_sel = len(range(row0, x.shape[0], row_step)) if n_sel is None else n_sel
    cap = max((n_t - 1) // 2, 1) if cap is None else cap
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    peaks = torch.full((n_sel * cap + GUARD,), FILL, dtype=torch.int32, device="cuda")
    count = torch.full((n_sel + GUARD,), FILL, dtype=torch.int32, device="cuda")
    status = torch.full((n_sel + GUARD,), FILL, dtype=torch.int32, device="cuda")
    prom = torch.full((n_sel * cap + GUARD,), -1.0, dtype=torch.float64, device="cuda") if want_prom else None
    _lib.call("dvh_find_peaks_rows", _lib.ptr(t), x.shape[1], n_t, row0, row_step, n_sel, sign, float(distance),
              0 if prominence is None else 1, 0.0 if prominence is None else float(prominence), float(wlen),
              _lib.ptr(peaks), cap, _lib.ptr(count), _lib.ptr(prom), _lib.ptr(status), _lib.stream_of(t.device))
    torch.cuda.synchronize()
    pk, ct, st = peaks.cpu().numpy(), count.cpu().numpy(), status.cpu().numpy()
    assert (pk[n_sel * cap:] == FILL).all() and (ct[n_sel:] == FILL).all() and (st[n_sel:] == FILL).all()
    body = pk[:n_sel * cap].reshape(n_sel, cap)
    lists = [body[k, :ct[k]] for k in range(n_sel)]
    pr = None
    if want_prom:
        pr = prom.cpu().numpy()
        assert (pr[n_sel * cap:] == -1.0).all()
        pr = [pr[:n_sel * cap].reshape(n_sel, cap)[k, :ct[k]] for k in range(n_sel)]
    return lists, ct[:n_sel], st[:n_sel], pr, body


def _scipy(row, distance=0.0, prominence=None, wlen=0.0):
    kw = {}
    if distance > 0:
        kw["distance"] = distance
    if prominence is not None:
        kw["prominence"] = prominence
        if wlen > 1:
            kw["wlen"] = wlen
    return scipy.signal.find_peaks(row, **kw)


def _distinct_rows(n_rows, n_t, seed):
    """Rows of distinct multiples of 2**-8 in [-8, 8): a random walk would repeat, a permutation does not."""
    rng = np.random.default_rng(seed)
    return np.stack([(rng.permutation(4096)[:n_t] if n_t <= 4096 else rng.permutation(8 * n_t)[:n_t]) / 256.0 - 8.0
                     for _ in range(n_rows)])


def _check_rows(x, **kw):
    lists, counts, status, prom, _ = _find_peaks(x, want_prom=True, **kw)
    x = np.atleast_2d(x)
    for k, row in enumerate(x):
        ref, props = _scipy(row, **kw)
        assert counts[k] == len(ref) and np.array_equal(lists[k], ref), (k, kw, lists[k], ref)
        assert status[k] == 0
        if "prominences" in props and kw.get("prominence") is not None:
            assert np.array_equal(prom[k], props["prominences"]), (k, kw)
    return lists


# ------------------------------------------------------------------------------------------ dvh_find_peaks_rows

@pytest.mark.parametrize("n_t", [1, 2, 3, 5, 63, 64, 65, 257, 700, 3000, 6000, 6001, 16384])
def test_find_peaks_random_rows(device, n_t):
    """Every rule together on distinct-valued rows, at the sizes around the wave, the tile and the LDS staging limit
    (6 000) and at the longest row the entry point takes."""
    x = _distinct_rows(3 if n_t > 3000 else 5, n_t, 900 + n_t)
    _check_rows(x)                                                   # local maxima alone
    _check_rows(x, distance=7)                                       # distance only, prominence off
    _check_rows(x, prominence=3.0)                                   # prominence over the whole row
    _check_rows(x, distance=4.5, prominence=2.0, wlen=41)            # all three; ceil(4.5) = 5, odd window
    _check_rows(x, distance=50, prominence=0.2, wlen=600)            # the tracker's defaults


def test_find_peaks_above_the_limit_is_refused(device):
    with pytest.raises(ValueError, match="DVH_FIND_PEAKS_MAX_NT"):
        _find_peaks(np.zeros((1, 16385)))


def test_find_peaks_plateaus_and_edges(device):
    rows = {
        "odd flat top": ([0, 1, 3, 3, 3, 1, 0], [3]),
        "even flat top": ([0, 1, 3, 3, 3, 3, 1, 0], [3]),                # (2 + 5) // 2
        "two-sample top": ([0, 2, 2, 0, 1, 0], [1, 4]),
        "plateau at the start": ([3, 3, 1, 2, 1], [3]),
        "plateau at the end": ([1, 2, 1, 4, 4], [1]),
        "rise to the end": ([0, 1, 2, 3], []),
        "fall from the start": ([3, 2, 1, 0], []),
        "all equal": ([2, 2, 2, 2, 2, 2], []),
        "plateau then higher": ([0, 2, 2, 3, 0], [3]),
        "peak before the last sample": ([0, 0, 1, 0], [2]),
        "plateau before the last sample": ([0, 1, 1, 0], [1]),
    }
    for name, (row, want) in rows.items():
        row = np.array(row, dtype=np.float64)
        lists = _check_rows(row)
        assert lists[0].tolist() == want, name


def test_find_peaks_nan(device):
    x = _distinct_rows(4, 300, 5)
    x[0, 100] = np.nan
    x[1, 0] = np.nan
    x[2, -1] = np.nan
    x[3, 150:153] = np.nan
    _check_rows(x)
    _check_rows(x, distance=6, prominence=1.5, wlen=80)
    row = np.array([0, 1, np.nan, 1, 0, 2, 0], dtype=np.float64)   # neither neighbour of the NaN is a peak
    assert _check_rows(row)[0].tolist() == [5]


def test_find_peaks_distance_rule(device):
    d = 6
    for gap, want in ((d - 1, [10]), (d, [10, 10 + d]), (d + 1, [10, 10 + d + 1])):
        row = np.zeros(40)
        row[10], row[10 + gap] = 3.0, 2.0
        assert _check_rows(row, distance=d)[0].tolist() == want, gap
        row[10], row[10 + gap] = 2.0, 3.0                           # the later one is the higher
        assert _check_rows(row, distance=d)[0].tolist() == ([10 + gap] if gap < d else want), gap
    chain = np.zeros(40)                                             # 10 removes 13; 13, removed, leaves 16 alone
    chain[10], chain[13], chain[16] = 3.0, 2.0, 1.0
    assert _check_rows(chain, distance=4)[0].tolist() == [10, 16]
    ramp = np.zeros(64)                                              # ascending heights 2 apart: one round each
    ramp[1:63:2] = np.arange(1, 32)
    assert _check_rows(ramp, distance=3)[0].tolist() == list(range(61, 0, -4))[::-1]
    assert _find_peaks(ramp, distance=0.5)[0][0].tolist() == list(range(1, 63, 2))   # ceil -> 1: nothing is closer


def test_find_peaks_prominence_rule(device):
    q = 2.0 ** -8
    row = np.zeros(60)
    row[10], row[30], row[50] = 2.0, 2.0 - q, 2.0 + q
    assert _check_rows(row, prominence=2.0)[0].tolist() == [10, 50]        # exactly min_prominence is kept
    # the window: the bases of peak 30 lie at 20 (-1) and 40 (-0.5), the next higher sample at 45
    row = np.zeros(80)
    row[20], row[30], row[40], row[45] = -1.0, 1.0, -0.5, 5.0
    row[46:] = 4.0
    for wlen in (0, -3, 1):                                                 # the whole row: bases -1 and -0.5
        lists, _, _, prom, _ = _find_peaks(row, prominence=0.5, wlen=wlen, want_prom=True)
        ref, props = scipy.signal.find_peaks(row, prominence=0.5)
        assert np.array_equal(lists[0], ref) and np.array_equal(prom[0], props["prominences"])
        assert ref.tolist() == [30, 45] and prom[0].tolist() == [1.5, 1.0]
    for wlen in (1.5, 2, 3, 4, 5, 19, 20, 21, 22, 23, 29, 30, 31, 200):                # odd and even, short of and past the base
        _check_rows(row, prominence=0.5, wlen=wlen)
    _, _, _, prom, _ = _find_peaks(row, prominence=0.5, wlen=19, want_prom=True)   # 21 .. 39: both bases outside
    assert prom[0][0] == 1.0
    _, _, _, prom, _ = _find_peaks(row, prominence=0.5, wlen=20, want_prom=True)   # 20 .. 40: both inside
    assert prom[0][0] == 1.5
    row2 = np.zeros(30)                                                     # windows clipped at both ends
    row2[2], row2[27] = 1.0, 1.5
    row2[0], row2[29] = -2.0, -1.0
    for wlen in (3, 4, 5, 6, 10, 59, 60):
        _check_rows(row2, prominence=0.25, wlen=wlen)
    x = _distinct_rows(3, 500, 77)
    for wlen in (2, 3, 10, 11, 999, 1000, 1001):
        _check_rows(x, prominence=1.0, wlen=wlen)


def test_find_peaks_sign(device):
    x = _distinct_rows(4, 257, 31)
    kw = dict(distance=5, prominence=2.0, wlen=60)
    lists, counts, _, _, _ = _find_peaks(x, sign=-1, **kw)
    for k, row in enumerate(x):
        ref = scipy.signal.find_peaks(-row, **kw)[0]
        assert np.array_equal(lists[k], ref)
    plateau = np.array([0, -1, -3, -3, -3, -3, -1, 0], dtype=np.float64)
    assert _find_peaks(plateau, sign=-1)[0][0].tolist() == [3]


def test_find_peaks_strided_selection(device):
    """row0 / row_step = 3 over a matrix whose row stride is longer than n_t: the tracker's [start::3] without a
    gather; the samples past n_t are never read (they would add peaks)."""
    n_t, stride = 200, 211
    x = _distinct_rows(11, stride, 41)
    x[:, n_t:] += 100.0
    kw = dict(distance=9, prominence=1.0, wlen=50)
    lists, counts, _, _, _ = _find_peaks(x, n_t=n_t, row0=2, row_step=3, n_sel=3, **kw)
    for k, r in enumerate((2, 5, 8)):
        assert np.array_equal(lists[k], scipy.signal.find_peaks(x[r, :n_t], **kw)[0])
    with pytest.raises(Exception, match="invalid shape"):
        _find_peaks(x, n_t=stride + 1)


def test_find_peaks_cap_overflow(device):
    """A row with more peaks than cap: status 1, count = cap, the first cap peaks, and nothing past the row's cap
    slots: the next row's slots hold only its own peaks and the guard region after the buffer is intact (checked in
    the helper)."""
    x = np.zeros((3, 64))
    x[0, 1:63:2] = np.arange(1, 32)           # 31 peaks
    x[1, 5], x[1, 9] = 1.0, 2.0                # 2 peaks
    x[2, 3:60:4] = np.arange(1, 16)           # 15 peaks
    lists, counts, status, _, body = _find_peaks(x, cap=4)
    assert counts.tolist() == [4, 2, 4] and status.tolist() == [1, 0, 1]
    assert lists[0].tolist() == [1, 3, 5, 7] and lists[1].tolist() == [5, 9] and lists[2].tolist() == [3, 7, 11, 15]
    assert body[1, 2:].tolist() == [FILL, FILL]
    lists, counts, status, _, _ = _find_peaks(x, cap=31)
    assert counts.tolist() == [31, 2, 15] and status.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------ dvh_peak_likelihood

def _likelihood(peaks, counts, t_axis, sigma, n_rows=None):
    import torch

    from das_diff_veh_amd import _lib
    pk = torch.from_numpy(np.ascontiguousarray(peaks, dtype=np.int32)).cuda()
    ct = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(t_axis, dtype=np.float64)).cuda()
    out = torch.full((len(t_axis) + GUARD,), -1.0, dtype=torch.float64, device="cuda")
    _lib.call("dvh_peak_likelihood", _lib.ptr(pk), peaks.shape[1], _lib.ptr(ct),
              len(counts) if n_rows is None else n_rows, _lib.ptr(t), len(t_axis), float(sigma), _lib.ptr(out),
              _lib.stream_of(t.device))
    got = out.cpu().numpy()
    assert (got[len(t_axis):] == -1.0).all()
    return got[:len(t_axis)]


@pytest.mark.parametrize("case", ["a", "b"])
def test_peak_likelihood(device, case):
    g = gio.load("tracker_" + case)
    t_axis, sigma = g["t_axis"], float(g["sigma"])
    ref = np.zeros(len(t_axis))
    for k in range(len(g["det_counts"])):
        row = np.zeros(len(t_axis))
        for p in g["det_peaks"][k, :g["det_counts"][k]]:
            row = row + scipy.stats.norm.pdf(t_axis, loc=t_axis[p], scale=sigma)
        ref += row
    got = _likelihood(g["det_peaks"], g["det_counts"], t_axis, sigma)
    err = np.abs(got - ref).max()
    print(f"{case}: |device - norm.pdf sum|max = {err:.3e} of max {ref.max():.3e}")
    assert err <= 1e-12 * np.abs(ref).max()
    assert np.abs(got - g["peak_erode"]).max() <= 1e-12 * g["peak_erode"].max()


def test_peak_likelihood_empty(device):
    g = gio.load("tracker_a")
    zero = np.zeros_like(g["det_counts"])
    assert not _likelihood(g["det_peaks"], zero, g["t_axis"], 0.08).any()             # no peak on any row
    assert not _likelihood(g["det_peaks"], g["det_counts"], g["t_axis"], 0.08, n_rows=0).any()   # no row


# ------------------------------------------------------------------------------------------ dvh_kf_track

def _kf(g, veh_base):
    import torch

    from das_diff_veh_amd import _lib
    i0 = int(np.argmin(np.abs(g["start_x"] - g["x_axis"])))
    i1 = int(np.argmin(np.abs(g["end_x"] - g["x_axis"])))
    x_sel = np.ascontiguousarray(g["x_axis"][i0:i1 + 1:3], dtype=np.float64)
    n_steps, n_veh = len(x_sel), len(veh_base)
    assert n_steps == len(g["row_counts"])
    pk = torch.from_numpy(np.ascontiguousarray(g["row_peaks"], dtype=np.int32)).cuda()
    ct = torch.from_numpy(np.ascontiguousarray(g["row_counts"], dtype=np.int32)).cuda()
    xs = torch.from_numpy(x_sel).cuda()
    vb = torch.from_numpy(np.ascontiguousarray(veh_base, dtype=np.int32)).cuda()
    out = torch.full((n_veh * n_steps + GUARD,), -1.0, dtype=torch.float64, device="cuda")
    _lib.call("dvh_kf_track", _lib.ptr(pk), g["row_peaks"].shape[1], _lib.ptr(ct), n_steps, _lib.ptr(xs), _lib.ptr(vb),
              n_veh, float(g["sigma_a"]), _lib.ptr(out), _lib.stream_of(xs.device))
    got = out.cpu().numpy()
    assert (got[n_veh * n_steps:] == -1.0).all()
    lists = [g["row_peaks"][k, :g["row_counts"][k]] for k in range(n_steps)]
    return got[:n_veh * n_steps].reshape(n_veh, n_steps), kr.kf_track(lists, x_sel, veh_base, float(g["sigma_a"]))


@pytest.mark.parametrize("case", ["a", "b"])
def test_kf_track(device, case):
    g = gio.load("tracker_" + case)
    got, ref = _kf(g, g["veh_base"])
    assert np.array_equal(ref, g["veh_states_raw"], equal_nan=True)
    assert np.array_equal(got, ref, equal_nan=True)
    one, ref1 = _kf(g, g["veh_base"][1:2])                                    # n_veh = 1
    assert np.array_equal(one, ref1, equal_nan=True) and np.array_equal(one[0], got[1], equal_nan=True)
    many = np.resize(g["veh_base"], 65)                                       # more vehicles than one wave
    many[60:] += np.array([3, -4, 11, 40, -40])                               # bases off the arrivals as well
    got65, ref65 = _kf(g, many)
    assert np.array_equal(got65, ref65, equal_nan=True)
    assert np.array_equal(got65[:60], np.resize(got, (60, got.shape[1])), equal_nan=True)


# ------------------------------------------------------------------------------------------ the drop-in and the wiring

def _args(g):
    return {"detect": dict(minprominence=float(g["minprominence"]), minseparation=int(g["minseparation"]),
                           prominenceWindow=int(g["prominenceWindow"]))}


def _check_tracks(got, ref):
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.nanmax(np.abs(got - ref)) <= 1e-9


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("where", ["device_negated", "host"])
def test_kf_tracking_drop_in(device, case, where):
    import torch

    from das_diff_veh_amd.apis.tracking import KF_tracking
    g = gio.load("tracker_" + case)
    grid = g["grid"].astype(np.float64)
    if where == "host":
        trk = KF_tracking(grid, g["t_axis"], g["x_axis"], _args(g))
    else:
        t = torch.from_numpy(-grid).cuda()
        trk = KF_tracking(t, g["t_axis"], g["x_axis"], _args(g), sign=-1)
        assert trk.data is t                                                  # not copied
    base = trk.detect_in_one_section(float(g["start_x"]), nx=int(g["nx"]), sigma=float(g["sigma"]))
    assert np.array_equal(base, g["veh_base"]) and base.dtype.kind == "i"
    assert np.abs(trk.peak_erode.cpu().numpy() - g["peak_erode"]).max() <= 1e-12 * g["peak_erode"].max()
    tracks = trk.tracking_with_veh_base(float(g["start_x"]), float(g["end_x"]), base, sigma_a=float(g["sigma_a"]))
    counts = trk.row_counts.cpu().numpy()
    assert np.array_equal(counts, g["row_counts"])
    peaks = trk.row_peaks.cpu().numpy()
    for k, c in enumerate(counts):
        assert np.array_equal(peaks[k, :c], g["row_peaks"][k, :c])
    assert np.array_equal(trk.veh_states_raw, g["veh_states_raw"], equal_nan=True)
    _check_tracks(tracks, g["tracks"])
    for plot in (trk.plot_data, trk.show_detection_example, trk.tracking_visulization_one_section):
        with pytest.raises(NotImplementedError):
            plot(0)


OFFSET = 592   # case a then tracks from 595 m, the selection fixture's start_x_tracking


def _tli_with_grid(g):
    """A TimeLapseImaging of the selection fixture's record, given the tracker fixture's grid as the tracking grid
    (negated: reverse_amp), on a whole-metre axis so that x0 - start_x indexes a track column.  The tracker sees the
    axis through differences only (3 m a step on either axis)."""
    import torch

    from das_diff_veh_amd.apis.timeLapseImaging import TimeLapseImaging
    c = gio.select_cases()["short"]
    obj = TimeLapseImaging(c["rec"].copy(), gio.load("tli")["x_axis"], c["t_axis"])
    obj.data_for_tracking = torch.from_numpy(-g["grid"].astype(np.float64)).cuda()
    obj.dist_along_fiber_tracking = np.arange(g["grid"].shape[0]) + OFFSET
    obj.t_axis_tracking = g["t_axis"]
    i0 = int(np.argmin(np.abs(g["start_x"] - g["x_axis"])))
    i1 = int(np.argmin(np.abs(g["end_x"] - g["x_axis"])))
    return obj, OFFSET + i0, OFFSET + i1, c


def test_track_vehicles_and_selection(device):
    from das_diff_veh_amd.select import pass_table
    g = gio.load("tracker_a")
    obj, start_x, end_x, c = _tli_with_grid(g)
    ret = obj.track_vehicles(start_x, end_x)
    assert ret is obj.veh_states and obj.start_x == start_x and obj.end_x == end_x
    assert obj.tracking_args == {"detect": {"minprominence": 0.2, "minseparation": 50, "prominenceWindow": 600}}
    assert obj.tracking.data is obj.data_for_tracking
    _check_tracks(obj.veh_states, g["tracks"])
    x0 = c["x0"]
    assert x0 - start_x == 25
    kw = dict(wlen_sw=2, length_sw=120, spatial_ratio=0.5)
    obj.select_surface_wave_windows(x0, **kw)
    ks = pass_table(obj.t_axis, obj.distances_along_fiber, x0, start_x, g["tracks"], g["t_axis"], obj.dt, **kw)[0]
    assert len(ks) > 0 and np.array_equal(obj.sw_selector.pass_indices, ks)
    assert len(obj.sw_selector) == len(obj.qs_selector) == len(ks)
    obj.data_for_tracking = -obj.data_for_tracking                     # the grid itself: tracked without the sign
    _check_tracks(obj.track_vehicles(start_x, end_x, reverse_amp=False), g["tracks"])


def test_device_tracker(device):
    from das_diff_veh_amd.apis.imaging_workflow import DeviceTracker
    g = gio.load("tracker_b")
    obj, start_x, end_x, _ = _tli_with_grid(g)
    veh_states, dist, t_trk = DeviceTracker(start_x, end_x, tracking_args=_args(g))(0, obj)
    _check_tracks(veh_states, g["tracks"])
    assert dist is obj.dist_along_fiber_tracking and t_trk is obj.t_axis_tracking
    assert obj.start_x == start_x and obj.tracking_args == _args(g)


def _traffic_record():
    """48 channels x 36 s as the workflow fixture's records, two vehicles crossing x0 = 620 m at 8 s and 24 s (a
    quasi-static trough of -4, 0.6 s wide: inside the 0.08-1 Hz tracking band, so that the band-pass leaves no ringing
    above the 0.2 prominence) over 0.3 * standard_normal; multiples of 2**-8."""
    from das_diff_veh_amd.synth import DT_W500
    rng = np.random.default_rng(720)
    n_ch, n_t, dt = 48, 9000, 0.004
    x_axis = 449.0 + np.arange(n_ch)
    t_axis = DT_W500 + np.arange(n_t) * dt
    pos = (x_axis - 400) * 8.16
    rec = 0.3 * rng.standard_normal((n_ch, n_t))
    for tc, v in ((8.0, 15.0), (24.0, 18.0)):
        rec += -4.0 * np.exp(-0.5 * ((t_axis[None, :] - t_axis[0] - tc - (pos[:, None] - 620.0) / v) / 0.6) ** 2)
    return np.round(rec * 2 ** 8) / 2 ** 8, x_axis, t_axis


def test_workflow_from_raw_records(device):
    """ImagingWorkflowOneDirectory(records, tracks=DeviceTracker(...)): raw record -> tracking grid -> tracks ->
    windows -> class mean with nothing supplied from outside.  The tracks equal the CPU chain's on the same grid, and
    the day's image equals the one the workflow forms when it is handed those tracks."""
    from das_diff_veh_amd.apis.imaging_workflow import DeviceTracker, ImagingWorkflowOneDirectory
    rec, x_axis, t_axis = _traffic_record()
    start_x, end_x, x0 = 595, 780, 620
    kw = dict(verbal=False, imaging_kwargs=dict(pivot=620, start_x=500, end_x=680, wlen=2, include_other_side=True),
              wlen_sw=12, length_sw=300, spatial_ratio=0.75)
    tracker, seen = DeviceTracker(start_x, end_x), []

    def tracks(k, obj):
        seen.append((obj, tracker(k, obj)))
        return seen[-1][1]

    wf = ImagingWorkflowOneDirectory([(rec.copy(), x_axis, t_axis)], tracks=tracks, method="xcorr")
    wf.imaging(start_x, end_x, x0, **kw)
    obj, (veh_states, dist, t_trk) = seen[0]
    assert dist[0] == (449 - 400) * 8.16 and len(dist) == 392 and np.array_equal(t_trk, t_axis[::5])
    grid = -np.asarray(obj.data_for_tracking)
    ref_base, ref_tracks = kr.chain(grid, t_trk, dist, start_x, end_x, sigma=0.08)
    assert ref_tracks.shape == (2, 186)                                      # 186 rows -> 62 steps
    _check_tracks(veh_states, ref_tracks)
    assert np.abs(t_trk[np.trunc(veh_states[:, x0 - start_x]).astype(int)] - t_axis[0] - [8.0, 24.0]).max() < 0.1
    assert wf.num_veh == 2
    wf2 = ImagingWorkflowOneDirectory([(rec.copy(), x_axis, t_axis)], [(ref_tracks, dist, t_trk)], method="xcorr")
    wf2.imaging(start_x, end_x, x0, **kw)
    assert wf2.num_veh == 2 and np.array_equal(wf.avg_image.XCF_out, wf2.avg_image.XCF_out)


def test_track_cars_still_raises(device):
    from das_diff_veh_amd.apis.timeLapseImaging import TimeLapseImaging
    obj = TimeLapseImaging.__new__(TimeLapseImaging)
    with pytest.raises(NotImplementedError, match="track_vehicles"):
        obj.track_cars(0, 1, {})
