"""Vehicle classes without a GPU: the NumPy restatement of the quasi-static chain (tests/classes_ref.py) against the
notebooks' cells (tests/golden/classes.npz) and against SciPy, the four split functions against the cells' index
arrays, the error messages, and the record functions against their plain-loop definition."""
import ctypes
import os

import numpy as np
import pytest
import scipy.signal

from tests import classes_ref as cr
from tests import golden_io as gio

SHAPES = [(1, 101), (2, 102), (37, 1500), (64, 1500), (49, 151)]


@pytest.fixture(scope="module")
def golden():
    g = gio.load("classes")
    states = g["q"].astype(np.float32) / np.float32(2 ** 8)  # exact: the fixture's float32 states
    return g, states


def test_ref_matches_the_notebook_cells(golden):
    g, states = golden
    op = cr.operator(101, 3)
    c, p = cr.curves(states, *op)
    tol = cr.bound(states.shape[-1], *op, float(np.abs(states).max()))
    assert np.abs(c - g["s_mean"]).max() <= tol
    assert np.abs(p - g["s_peaks"]).max() <= tol
    kept = g["w_speed_idx"]
    assert np.abs(c[kept] - g["w_mean"]).max() <= tol and np.abs(p[kept] - g["w_peaks"]).max() <= tol


@pytest.mark.parametrize("n_ch,n_t", SHAPES)
def test_ref_matches_scipy_within_the_derived_bound(n_ch, n_t):
    """|restatement - detrend(savgol_filter(d.mean(0), 101, 3))| <= classes_ref.bound (derived there from the
    coefficient magnitudes: 7.8e-12 max|x| at n_t = 1500, 4.0e-12 at 101), and the float64 restatement against its
    longdouble form within the same bound.  Measured: at most 2.8e-15 max|x| and 5.5e-16 max|x|."""
    rng = np.random.default_rng(n_ch * 10000 + n_t)
    d = rng.standard_normal((n_ch, n_t)) + np.linspace(-2, 3, n_t) - 4 * np.exp(-((np.arange(n_t) - n_t / 2) / 20) ** 2)
    op = cr.operator(101, 3)
    c, p = cr.curves(d, *op)
    want = cr.scipy_chain(d)
    amax = float(np.abs(d).max())
    tol = cr.bound(n_t, *op, amax)
    err = float(np.abs(c - want).max())
    cl, pl = cr.curves(d, *op, longdouble=True)
    err_l = float(np.abs(c - cl.astype(np.float64)).max())
    print(f"({n_ch}, {n_t}): vs scipy {err / amax:.2e} max|x|, vs longdouble {err_l / amax:.2e} max|x|, "
          f"bound {tol / amax:.2e} max|x|")
    assert err <= tol and err_l <= tol
    assert abs(p - np.abs(want).max()) <= tol and c[0] == 0.0
    assert 1e-13 * amax < tol < 1e-11 * amax  # the bound itself stays where its derivation puts it


def test_mean_is_numpys_bit_for_bit():
    rng = np.random.default_rng(4)
    for n_ch in (3, 37, 140, 1024):
        d = rng.standard_normal((n_ch, 200))
        assert np.array_equal(cr.channel_mean(d), d.mean(0))


def test_detrend_closed_form_is_scipys():
    rng = np.random.default_rng(6)
    for n_t in (3, 101, 1500):
        y = rng.standard_normal(n_t) + np.linspace(0, 5, n_t)
        assert np.abs(cr.detrend(y) - scipy.signal.detrend(y)).max() <= 2.5 * 2 * (n_t + 8) * cr.U * np.abs(y).max()


def test_splits_match_the_notebook_cells_exactly(golden):
    from das_diff_veh_amd import classes
    g, _ = golden
    s = classes.peak_majority(g["s_peaks"])
    assert s.names == ("majority",) and np.array_equal(s.indices[0], g["s_peak_idx"])
    assert s.indices[0].dtype == g["s_peak_idx"].dtype
    for k in ("mode_peak", "sigma"):
        assert s.thresholds[k] == g[f"s_{k}"]
    assert s.thresholds["lower_limit"] == g["s_lower"] and s.thresholds["upper_limit"] == g["s_upper"]
    speeds = g["veh_speed"][s.indices[0]]                      # cell 6 keeps the majority's speeds
    v = classes.speed_classes(speeds)
    assert v.names == ("fast", "mid", "slow")
    for name in v.names:
        assert np.array_equal(v[name], g[f"s_{name}_idx"]), name
    assert v.thresholds["threshold_1"] == g["s_threshold_1"] and v.thresholds["threshold_2"] == g["s_threshold_2"]
    m = classes.speed_majority(g["veh_speed"])
    assert np.array_equal(m.indices[0], g["w_speed_idx"])
    assert m.thresholds["lower_limit"] == g["w_lower"] and m.thresholds["upper_limit"] == g["w_upper"]
    w = classes.weight_classes(g["w_peaks"])
    assert w.names == ("heavy", "mid", "light") and w.thresholds["threshold_1"] == 1.2
    assert w.thresholds["threshold_2"] == g["w_mode_peak"]
    for name in w.names:
        assert np.array_equal(w[name], g[f"w_{name}_idx"]), name
    assert classes.peak_majority(g["s_peaks"], width=1e9).indices[0].size == g["s_peaks"].size


def test_subset_is_the_ascending_union_with_aligned_slots(golden):
    from das_diff_veh_amd import classes
    g, _ = golden
    w = classes.weight_classes(g["w_peaks"])
    sel, slots, n_slot = w.subset()
    assert n_slot == 3 and np.array_equal(sel, np.arange(g["w_peaks"].size))  # the three classes cover every pass
    for k, name in enumerate(w.names):
        assert np.array_equal(sel[slots == k], g[f"w_{name}_idx"])
    two = classes.ClassSplit(("a", "b"), (np.array([7, 2]), np.array([5])), {})
    sel, slots, n_slot = two.subset()
    assert sel.tolist() == [2, 5, 7] and slots.tolist() == [0, 1, 0] and n_slot == 2
    assert classes.peak_majority(g["s_peaks"]).subset()[2] == 1


def test_errors_are_the_reference_chains():
    from das_diff_veh_amd import classes
    short = "If mode is 'interp', window_length must be less than or equal to the size of x."
    with pytest.raises(ValueError, match=short):
        classes.quasi_static_curves(np.zeros((2, 3, 100)))
    with pytest.raises(ValueError, match=short):
        classes.quasi_static_curves([np.zeros((3, 200)), np.zeros((3, 100))])
    with pytest.raises(ValueError, match=short) as e:
        scipy.signal.savgol_filter(np.zeros(100), 101, 3)
    assert str(e.value) == short
    with pytest.raises(ValueError, match="polyorder must be less than window_length"):
        classes.quasi_static_curves(np.zeros((2, 3, 100)), 3, 3)
    with pytest.raises(ValueError):
        classes.quasi_static_curves(np.zeros((2, 3, 100)), 20, 3)
    with pytest.raises(ValueError, match="n_pass, n_ch, n_t"):
        classes.quasi_static_curves(np.zeros((3, 200)))
    with pytest.raises(ValueError, match="array must not contain infs or NaNs"):  # what the kernel's status stands for
        scipy.signal.detrend(np.array([0.0, np.nan, 1.0]))
    c, p = classes.quasi_static_curves(np.zeros((0, 3, 200)))  # no pass: no launch, no device needed
    assert c.shape[0] == 0 and p.shape == (0,) and p.dtype == np.float64
    assert classes.quasi_static_curves([], skip_failed=True)[2] == {}


def test_c_entry_refuses_before_it_touches_anything():
    """-4 for wlen even, < 3 or over the limit, n_t < wlen, n_ch < 1, n_pass < 0 (checked before any pointer is read),
    0 for n_pass == 0; the tile and limit constants are the header's."""
    from das_diff_veh_amd import _lib, classes
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(gio.GOLDEN), os.pardir, "include", "dvh.h")).read()
    assert f"#define DVH_QS_TILE {classes.QS_TILE}\n" in hdr and f"#define DVH_QS_MAX_WLEN {classes.QS_MAX_WLEN}\n" in hdr

    def rc(n_pass=1, n_ch=1, n_t=200, wlen=101):
        return lib.dvh_qs_curves(None, 1, None, n_pass, n_ch, n_t, None, wlen, None, None, None, n_t, None, None, None,
                                 None)
    assert rc(wlen=100) == -4 and rc(wlen=1) == -4 and rc(wlen=classes.QS_MAX_WLEN + 2) == -4
    assert rc(n_t=100) == -4 and rc(n_ch=0) == -4 and rc(n_pass=-1) == -4
    assert rc(n_pass=0) == 0
    assert rc() == -2 and b"null" in lib.dvh_last_error()
    assert lib.dvh_qs_curves_workspace(3, 200) == 2 * 3 * 200 * 8 and lib.dvh_qs_curves_workspace(0, 200) == 0
    assert lib.dvh_class_curve_stats(None, 10, None, 0, 10, 0, None, None, None, None) == 0
    assert isinstance(lib.dvh_qs_curves_workspace.restype(), ctypes.c_int64)


X_AXIS = 400.0 + 8.16 * np.arange(40)
T_AXIS = 5.0 + 0.004 * np.arange(3000)


def _track(t_at_x0, speed, x0=500.0):
    xs = np.arange(380.0, 760.0, 1.0)
    return xs, t_at_x0 + (xs - x0) / speed


@pytest.mark.parametrize("start_x,end_x", [(400.0, 500.0), (X_AXIS[0] - 5, X_AXIS[3]), (X_AXIS[30], X_AXIS[-1]),
                                           (455.5, 610.1)])
@pytest.mark.parametrize("t_at,speed,n_t,valid", [
    (11.0, 100.0, 1500, True),
    (5.0 + 0.004 * 750 + 100 / 25.0, 25.0, 1500, None),   # around the record's start: decided by the definition
    (5.0 + 0.004 * 2999, -40.0, 400, None),               # around the record's end, a vehicle going the other way
    (30.0, 25.0, 1500, False),                            # passes after the record ends
    (-3.0, 25.0, 1500, False)])                           # passed before it began
def test_aligned_states_table_is_its_definition(start_x, end_x, t_at, speed, n_t, valid):
    from das_diff_veh_amd import classes
    trk = _track(t_at, speed)
    ch0, n_ch, t_start = classes.aligned_states_table(X_AXIS, T_AXIS, trk, start_x, end_x, n_t)
    r0, rn, rt, rvalid = cr.states_table(X_AXIS, T_AXIS, trk, start_x, end_x, n_t)
    assert (ch0, n_ch) == (r0, rn) and t_start.dtype == np.int64 and np.array_equal(t_start, rt)
    assert classes.states_table_valid(t_start, n_t, T_AXIS.size) == rvalid
    if valid is not None:
        assert rvalid == valid


def test_aligned_states_table_touches_both_ends_of_the_record():
    """A pass whose first row starts on the record's first sample and one whose last row ends on its last."""
    from das_diff_veh_amd import classes
    n_t = 400
    first = (np.array([X_AXIS[0], X_AXIS[5]]), np.array([T_AXIS[200], T_AXIS[230]]) - 0.002)  # between two samples
    ch0, n_ch, ts = classes.aligned_states_table(X_AXIS, T_AXIS, first, X_AXIS[0], X_AXIS[5], n_t)
    assert (ch0, n_ch) == (0, 5) and ts[0] == 0 and classes.states_table_valid(ts, n_t, T_AXIS.size)
    last = (np.array([X_AXIS[34], X_AXIS[39]]), np.array([T_AXIS[2770], T_AXIS[2800]]) - 0.002)
    ch0, n_ch, ts = classes.aligned_states_table(X_AXIS, T_AXIS, last, X_AXIS[34], X_AXIS[39], n_t)
    assert (ch0, n_ch) == (34, 5) and classes.states_table_valid(ts, n_t, T_AXIS.size)
    late = (last[0], last[1] + 0.004 * 6)
    ch0, n_ch, ts = classes.aligned_states_table(X_AXIS, T_AXIS, late, X_AXIS[34], X_AXIS[39], n_t)
    assert ts.max() + n_t == T_AXIS.size and classes.states_table_valid(ts, n_t, T_AXIS.size)
    later = (last[0], last[1] + 0.004 * 7)
    ts = classes.aligned_states_table(X_AXIS, T_AXIS, later, X_AXIS[34], X_AXIS[39], n_t)[2]
    assert not classes.states_table_valid(ts, n_t, T_AXIS.size)
    with pytest.raises(ValueError, match="no channel"):
        classes.aligned_states_table(X_AXIS, T_AXIS, last, X_AXIS[34], X_AXIS[-1] + 50, n_t)


def test_aligned_states_table_takes_a_window():
    from das_diff_veh_amd import classes
    from das_diff_veh_amd.apis.data_classes import SurfaceWaveWindow
    from das_diff_veh_amd.synth import synth_pass
    p = synth_pass(5, n_t=3000)
    w = SurfaceWaveWindow(p["data"], p["x_axis"], p["t_axis"], p["veh_state"], p["start_x_tracking"],
                          p["distance_along_fiber_tracking"], p["t_axis_tracking"])
    a = classes.aligned_states_table(p["x_axis"], p["t_axis"], w, 600, 800, 1500)
    b = classes.aligned_states_table(p["x_axis"], p["t_axis"], (w.veh_state_x, w.veh_state_t), 600, 800, 1500)
    r = cr.states_table(p["x_axis"], p["t_axis"], (w.veh_state_x, w.veh_state_t), 600, 800, 1500)
    assert a[:2] == b[:2] == r[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[2], r[2])


def test_track_speeds_is_its_definition():
    from das_diff_veh_amd import classes
    dist = np.arange(300.0, 900.0)
    t_trk = 2.0 + 0.02 * np.arange(4000)
    rng = np.random.default_rng(2)
    n_x = 400
    vs = np.full((6, n_x), np.nan)
    speeds = [12.0, 25.0, -30.0, 20.0, 18.0, 22.0]
    for k, v in enumerate(speeds):
        t = 30.0 + (np.arange(n_x)) / v + 0.01 * rng.standard_normal(n_x)
        vs[k] = np.round((t - t_trk[0]) / 0.02)
    vs[1, ::3] = np.nan
    vs[3, :] = np.nan
    vs[3, 200] = 1500.0             # one sample: NaN
    vs[4, :] = 1500.0               # zero slope: NaN
    vs[5, 120:] = np.nan            # tracked only before start_x: NaN
    got = classes.track_speeds(vs, dist, t_trk, 350.0, 480.0, 700.0)
    want = np.array([cr.track_speed(v, dist, t_trk, 350.0, 480.0, 700.0) for v in vs])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).tolist() == [False, False, False, True, True,
                                                                                       True]
    ok = ~np.isnan(want)
    assert np.abs(got[ok] / want[ok] - 1).max() < 1e-9
    assert np.abs(got[:3] / np.array(speeds[:3]) - 1).max() < 0.02
