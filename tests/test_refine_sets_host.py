"""Observation sets without a GPU: dvh_lm_normal_sets_host (csrc/refine.h on the CPU) bit for bit against
dvh_lm_normal_host called per set and on the reduced tables that define an absent sample, its flags and refusals, and
the host halves of the Python layer: observation_sets, sets_from_ridges and EnsembleResult's profiles."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import refine_ref as ref
from tests import refine_sets_ref as sets_ref
from tests.test_refine_host import POISON, case_arrays, normal_host


@pytest.fixture(scope="module")
def lib():
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    return _lib.load()


def sets_host(lib, c, dcdp, chain, tab, set_obs, set_sigma, model_set, n_period=ref.N_PERIOD, n_mode=ref.N_MODE,
              rho_floor=ref.RHO_FLOOR):
    """One dvh_lm_normal_sets_host call into poisoned buffers of a model more than asked -> (f, g, H, status)."""
    M, (K, D) = c.shape[0], chain.shape[1:]
    n_set, S = set_obs.shape
    model_set = np.ascontiguousarray(model_set, np.int32)
    assert set_sigma.shape == (n_set, S) and model_set.shape == (M,) and tab["sample_curve"].size == S
    arrays = [np.ascontiguousarray(a) for a in (c, dcdp, chain, tab["sample_period"], tab["sample_mode"], set_obs,
                                                set_sigma, model_set, tab["sample_curve"], tab["curve_weight"])]
    f, g, H = (np.full(s, POISON) for s in ((M + 1,), (M + 1, D), (M + 1, D, D)))
    status = np.full(M + 1, -7, np.int32)
    p = [a.ctypes.data for a in arrays]
    rc = lib.dvh_lm_normal_sets_host(p[0], p[1], p[2], M, n_period, n_mode, K // 4, D, *p[3:8], n_set, p[8], S, p[9],
                                     tab["curve_weight"].size, rho_floor, f.ctypes.data, g.ctypes.data, H.ctypes.data,
                                     status.ctypes.data)
    assert rc == 0, lib.dvh_last_error()
    assert f[M] == POISON and (g[M] == POISON).all() and (H[M] == POISON).all() and status[M] == -7
    assert not (g[:M] == POISON).any() and not (H[:M] == POISON).any() and not (status[:M] == -7).any()
    return f[:M], g[:M], H[:M], status[:M]


def same_bits(got, want, m, at=None):
    """Model m of ``got`` equals model ``at`` (default m) of ``want`` in f, g, H and status, NaN included."""
    at = m if at is None else at
    return all(np.array_equal(a[m], b[at], equal_nan=a.dtype.kind == "f") for a, b in zip(got, want))


def is_flagged(got, m):
    f, g, H, status = got
    return status[m] == 1 and f[m] == np.inf and (g[m] == 0).all() and (H[m] == 0).all()


def check_present_sets(sets_launch, normal_launch, n_layer, D, S):
    """Every model against dvh_lm_normal with its set's observations and uncertainties, bit for bit."""
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    set_obs, set_sigma = sets_ref.present_sets(n_layer, D, S)
    per_set = [normal_launch(c, dcdp, chain, sets_ref.table_of_set(tab, set_obs, set_sigma, k))
               for k in range(sets_ref.N_SET)]
    assert not np.array_equal(per_set[0][0], per_set[1][0]) and not np.array_equal(per_set[1][1], per_set[2][1])
    used = set()
    for model_set in sets_ref.MODEL_SETS:
        got = sets_launch(c, dcdp, chain, tab, set_obs, set_sigma, model_set)
        assert (got[3] == 0).all()
        for m, k in enumerate(model_set):
            assert same_bits(got, per_set[k], m), (model_set, m)
        used |= set(model_set)
    assert used == set(range(sets_ref.N_SET))


def check_absent_samples(sets_launch, normal_launch):
    """Absent samples of set 1 against dvh_lm_normal on the reduced table, bit for bit, for the models that name set
    1; the model on set 0 keeps the bits of the full table.  A set of all NaN is flagged."""
    n_layer, D, S = sets_ref.ABSENT_SHAPE
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    set_obs, set_sigma = sets_ref.present_sets(n_layer, D, S)
    model_set = (1, 0, 1)
    full = normal_launch(c, dcdp, chain, sets_ref.table_of_set(tab, set_obs, set_sigma, 0))
    for name, absent in sets_ref.absent_cases():
        got = sets_launch(c, dcdp, chain, tab, sets_ref.with_absent(set_obs, 1, absent), set_sigma, model_set)
        reduced = sets_ref.reduced_table(sets_ref.table_of_set(tab, set_obs, set_sigma, 1), absent)
        assert reduced["sample_obs"].size == S - absent.size
        assert reduced["curve_weight"].size == (2 if name != "one sample of a curve" else 3)
        want = normal_launch(c, dcdp, chain, reduced)
        assert (got[3] == 0).all() and (want[3] == 0).all(), name
        assert same_bits(got, want, 0) and same_bits(got, want, 2) and same_bits(got, full, 1), name
        assert not same_bits(got, full, 0), name
    got = sets_launch(c, dcdp, chain, tab, sets_ref.with_absent(set_obs, 1, np.arange(S)), set_sigma, model_set)
    assert is_flagged(got, 0) and is_flagged(got, 2) and same_bits(got, full, 1)


def check_set_flags(sets_launch):
    """Each spoiled input flags exactly model 1 and leaves the others' bits unchanged."""
    n_layer, D, S = sets_ref.ABSENT_SHAPE
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    set_obs, set_sigma = sets_ref.present_sets(n_layer, D, S)
    clean = sets_launch(c, dcdp, chain, tab, set_obs, set_sigma, (0, 1, 2))
    assert (clean[3] == 0).all()

    def only_model_1(got, name):
        assert is_flagged(got, 1) and same_bits(got, clean, 0) and same_bits(got, clean, 2), name

    for bad in (0.0, -0.5, np.nan, np.inf):
        sigma = set_sigma.copy()
        sigma[1, 4] = bad
        only_model_1(sets_launch(c, dcdp, chain, tab, set_obs, sigma, (0, 1, 2)), f"sigma {bad}")
    for bad in (-1, sets_ref.N_SET):
        only_model_1(sets_launch(c, dcdp, chain, tab, set_obs, set_sigma, (0, bad, 2)), f"model_set {bad}")
    # an absent sample's sigma is not looked at
    obs = sets_ref.with_absent(set_obs, 1, np.array([4]))
    want = sets_launch(c, dcdp, chain, tab, obs, set_sigma, (0, 1, 2))
    sigma = set_sigma.copy()
    sigma[1, 4] = np.nan
    got = sets_launch(c, dcdp, chain, tab, obs, sigma, (0, 1, 2))
    assert (got[3] == 0).all() and all(same_bits(got, want, m) for m in range(3))
    assert not same_bits(got, clean, 1)
    # what dvh_lm_normal flags on, at a present sample: a root that is not finite
    bad_c = c.copy()
    bad_c[1, tab["sample_period"][3], tab["sample_mode"][3]] = np.nan
    only_model_1(sets_launch(bad_c, dcdp, chain, tab, set_obs, set_sigma, (0, 1, 2)), "nan root")
    # ... and not at an absent one, nor on its dcdp row, where no other sample shares the slot
    slot = list(zip(tab["sample_period"], tab["sample_mode"]))
    alone = next(s for s in range(S) if slot.count(slot[s]) == 1)
    obs = sets_ref.with_absent(set_obs, 1, np.array([alone]))
    want = sets_launch(c, dcdp, chain, tab, obs, set_sigma, (1, 1, 1))
    bad_c, bad_d = c.copy(), dcdp.copy()
    bad_c[1, slot[alone][0], slot[alone][1]] = np.nan
    bad_d[2, slot[alone][0], slot[alone][1]] = np.inf
    got = sets_launch(bad_c, bad_d, chain, tab, obs, set_sigma, (1, 1, 1))
    assert (got[3] == 0).all() and all(same_bits(got, want, m) for m in range(3))


@pytest.mark.parametrize("S", sorted(ref.CURVE_SIZES))
@pytest.mark.parametrize("n_layer,D", ref.SHAPES)
def test_present_sets_are_lm_normal_per_set(lib, n_layer, D, S):
    check_present_sets(lambda *a: sets_host(lib, *a), lambda *a: normal_host(lib, *a), n_layer, D, S)


def test_absent_samples_are_the_reduced_table(lib):
    check_absent_samples(lambda *a: sets_host(lib, *a), lambda *a: normal_host(lib, *a))


def test_flags_touch_only_their_own_model(lib):
    check_set_flags(lambda *a: sets_host(lib, *a))


def test_refusals_come_before_any_launch(lib):
    """-2 and -4 of both entries with nothing written (the pointers are never dereferenced); the device entry returns
    them, and 0 for n_model = 0, before a device is touched."""
    p = ctypes.c_void_p(64)
    ok = (p, p, p, 2, 5, 4, 3, 8, p, p, p, p, p, 3, p, 7, p, 2, 1e-12, p, p, p, p)
    for name, tail in (("dvh_lm_normal_sets", (None,)), ("dvh_lm_normal_sets_host", ())):
        f = lambda *a: getattr(lib, name)(*a, *tail)
        for at in (0, 1, 2, 8, 9, 10, 11, 12, 14, 16, 19, 20, 21, 22):  # NULL tables, model_set and outputs
            assert f(*ok[:at], None, *ok[at + 1:]) == -2, (name, at)
        for at, bad in ((13, 0), (13, -1), (3, -1), (4, 0), (5, 0), (6, 0), (7, 0), (15, 0), (17, 0), (18, 0.0),
                        (18, float("nan"))):
            assert f(*ok[:at], bad, *ok[at + 1:]) == -2, (name, at, bad)
        for at, bad, word in ((7, 97, b"96 parameters"), (6, 33, b"32 layers"), (5, 17, b"16 modes"),
                              (17, 65, b"64 curves")):
            assert f(*ok[:at], bad, *ok[at + 1:]) == -4 and word in lib.dvh_last_error(), (name, at)
        assert f(None, None, None, 0, 5, 4, 3, 8, None, None, None, None, None, 3, None, 7, None, 2, 1e-12, None, None,
                 None, None) == 0


# ------------------------------------------------------------------------------------------------- the Python layer

def templates():
    from das_diff_veh_amd.inversion import Curve
    return [Curve([0.2, 0.1, 0.4], [0.3, 0.3, 0.3], 0, "rayleigh", "phase", weight=2.0, uncertainties=[0.01, 0.02, 0.04]),
            Curve([0.1, 0.05], [0.5, 0.5], 2, "rayleigh", "phase")]


def test_observation_sets_are_in_table_order():
    """obs and sigma [K, S] follow sample_table's order: curve by curve, each in the order of its own periods."""
    from das_diff_veh_amd.inversion import observation_sets
    curves = templates()
    data = [np.array([[1.0, 2.0, 3.0], [4.0, np.nan, 6.0]]), np.array([[7.0, 8.0], [np.nan, np.nan]])]
    sets = observation_sets(curves, data, device=torch.device("cpu"))
    assert sets.n_set == 2 and sets.obs.dtype == sets.sigma.dtype == torch.float64
    assert np.array_equal(sets.obs.numpy(), [[1, 2, 3, 7, 8], [4, np.nan, 6, np.nan, np.nan]], equal_nan=True)
    assert np.array_equal(sets.sigma.numpy(), [[0.01, 0.02, 0.04, 1, 1]] * 2)  # the curves' own, or 1
    tab = sets.table
    assert tab.periods.tolist() == [0.05, 0.1, 0.2, 0.4] and tab.need.tolist() == [3, 3, 1, 1] and tab.n_mode == 3
    assert tab.sample_period.tolist() == [2, 1, 3, 1, 0] and tab.sample_mode.tolist() == [0, 0, 0, 2, 2]
    assert tab.sample_curve.tolist() == [0, 0, 0, 1, 1] and tab.curve_weight.tolist() == [2.0, 1.0]
    unc = [np.array([[0.1, 0.2, 0.3], [0.4, np.nan, 0.6]]), np.array([[0.7, 0.8], [-1.0, 0.0]])]  # absent: anything
    sets = observation_sets(curves, data, unc, device=torch.device("cpu"))
    assert np.array_equal(sets.sigma.numpy(), [[0.1, 0.2, 0.3, 0.7, 0.8], [0.4, np.nan, 0.6, -1.0, 0.0]],
                          equal_nan=True)


def test_observation_sets_and_refine_sets_refuse_bad_input():
    """Every ValueError before any device work: there is no device here."""
    from das_diff_veh_amd.inversion import observation_sets
    from tests.test_refine_host import chain_model
    curves = templates()
    good = [np.full((2, 3), 0.3), np.full((2, 2), 0.5)]
    bad_inputs = {
        "one array short": dict(data_sets=good[:1]),
        "a wrong length": dict(data_sets=[good[0], np.full((2, 3), 0.5)]),
        "two values of K": dict(data_sets=[good[0], np.full((3, 2), 0.5)]),
        "not two-dimensional": dict(data_sets=[good[0][0], good[1][0]]),
        "K = 0": dict(data_sets=[np.empty((0, 3)), np.empty((0, 2))]),
        "+inf data": dict(data_sets=[np.where(np.eye(2, 3) > 0, np.inf, 0.3), good[1]]),
        "-inf data": dict(data_sets=[good[0], np.where(np.eye(2) > 0, -np.inf, 0.5)]),
        "uncertainty shapes": dict(uncertainty_sets=[np.ones((2, 3)), np.ones((2, 3))]),
        "uncertainty 0": dict(uncertainty_sets=[np.where(np.eye(2, 3) > 0, 0.0, 1.0), np.ones((2, 2))]),
        "uncertainty < 0": dict(uncertainty_sets=[np.ones((2, 3)), -np.ones((2, 2))]),
        "uncertainty NaN": dict(uncertainty_sets=[np.where(np.eye(2, 3) > 0, np.nan, 1.0), np.ones((2, 2))]),
        "uncertainty inf": dict(uncertainty_sets=[np.ones((2, 3)), np.full((2, 2), np.inf)]),
    }
    for name, bad in bad_inputs.items():
        with pytest.raises(ValueError):
            observation_sets(**{**dict(curves=curves, data_sets=good), **bad})
            pytest.fail(name)
    model = chain_model(lambda vp: 1.56 + 0.186 * vp)
    lo, hi = model.bounds()
    x = np.tile(0.5 * (lo + hi), (2, 1))
    ok = dict(curves=curves, data_sets=good, xs=x)
    for name, bad in {**bad_inputs, "xs outside": dict(xs=x + 1.0), "xs width": dict(xs=x[:, :7]),
                      "M != K without model_set": dict(xs=x[:1]), "model_set length": dict(model_set=[0]),
                      "model_set below": dict(model_set=[0, -1]), "model_set above": dict(model_set=[0, 2]),
                      "model_set of floats": dict(model_set=[0.0, 1.0]), "maxiter": dict(maxiter=-1),
                      "lam0": dict(lam0=0.0), "no curves": dict(curves=[], data_sets=[])}.items():
        with pytest.raises(ValueError):
            model.refine_sets(**{**ok, **bad})
            pytest.fail(name)
    with pytest.raises(TypeError):
        model.refine_sets(["curve", "curve"], good, x)


def test_sets_from_ridges():
    """Periods ascend (the frequencies reversed), m/s become km/s, the templates carry the mean and the standard
    deviation over the resamples, and a frequency of zero deviation takes the band's smallest positive one."""
    from das_diff_veh_amd.inversion import sets_from_ridges
    freqs = np.array([2.0, 4.0, 5.0, 8.0, 10.0, 20.0])
    lb, ub = [2.0, 5.0], [8.0, 20.0]                                  # bands 2, 4, 5 Hz and 5, 8, 10 Hz
    # velocities whose km/s, means and deviations are exact in binary
    r0 = np.array([[250.0, 500.0, 500.0], [750.0, 500.0, 750.0]])     # std 250, 0, 125 m/s
    r1 = np.array([[500.0, np.nan, 250.0], [500.0, 750.0, 750.0]])    # std 0, 0 (one pick), 250 m/s
    curves, data = sets_from_ridges(freqs, lb, ub, [r0, r1], modes=[0, 3], weights=[2.0, 1.0])
    assert [c.mode for c in curves] == [0, 3] and [c.weight for c in curves] == [2.0, 1.0]
    assert curves[0].period.tolist() == [0.2, 0.25, 0.5] and curves[1].period.tolist() == [0.1, 0.125, 0.2]
    assert np.array_equal(data[0], [[0.5, 0.5, 0.25], [0.75, 0.5, 0.75]])
    assert np.array_equal(data[1], [[0.25, np.nan, 0.5], [0.75, 0.75, 0.5]], equal_nan=True)
    assert curves[0].data.tolist() == [0.625, 0.5, 0.5] and curves[1].data.tolist() == [0.5, 0.75, 0.5]
    assert np.std(data[0], axis=0).tolist() == [0.125, 0.0, 0.25]
    assert curves[0].uncertainties.tolist() == [0.125, 0.125, 0.25]  # the zero takes the smallest positive one
    assert curves[1].uncertainties.tolist() == [0.25, 0.25, 0.25]
    # no positive deviation in a band: no uncertainties; and none asked for
    curves, _ = sets_from_ridges(freqs, lb, ub, [r0[:1], r1[1:]], modes=[0, 3])
    assert curves[0].uncertainties is None and curves[1].uncertainties is None and curves[0].weight == 1.0
    curves, _ = sets_from_ridges(freqs, lb, ub, [r0, r1], modes=[0, 3], uncertainties=None)
    assert curves[0].uncertainties is None and curves[1].uncertainties is None
    # every second frequency, counted from the band's first
    curves, data = sets_from_ridges(freqs, lb, ub, [r0, r1], modes=[0, 3], stride=2)
    assert curves[0].period.tolist() == [0.2, 0.5] and np.array_equal(data[0], [[0.5, 0.25], [0.75, 0.75]])
    for bad in (dict(ridges=[r0]), dict(ridges=[r0[:, :2], r1]), dict(ridges=[r0, r1[:1]]), dict(stride=0),
                dict(uncertainties="range"), dict(ridges=[r0, np.where(np.isnan(r1), np.inf, r1)]),
                dict(ridges=[r0, np.where(np.arange(3) == 1, np.nan, r1)])):
        with pytest.raises(ValueError):
            sets_from_ridges(**{**dict(freqs=freqs, freq_lb=lb, freq_ub=ub, ridges=[r0, r1], modes=[0, 3]), **bad})


def ensemble():
    """Six rows of a three-layer model by hand: interfaces at 0.01 and 0.03 km in rows 0 - 4, at 0.02 and 0.02 (an
    empty second layer) in row 5; four sets, the last named by no row."""
    from das_diff_veh_amd.inversion import EnsembleResult
    M, n = 6, 3
    models = np.zeros((M, n, 4))
    models[:, :, 0] = [0.01, 0.02, 0.0]
    models[5, :, 0] = [0.02, 0.0, 0.0]
    models[:, :, 2] = np.arange(M)[:, None] + [0.1, 0.2, 0.3]
    models[:, :, 1] = 2.0 * models[:, :, 2]
    models[:, :, 3] = 1.5
    misfits = np.array([0.5, 0.25, 0.25, np.inf, np.inf, 0.75])
    z = np.zeros
    return EnsembleResult(z((M, 8)), models, misfits, misfits.copy(), z((1, M)), z((0, M), bool), z(M),
                          z(M, np.int32), z((M, 8)), z((M, 8, 8)), model_set=np.array([0, 0, 0, 1, 1, 2], np.int32),
                          n_set=4)


def test_best_per_set_takes_the_first_minimum_and_marks_empty_sets():
    res = ensemble()
    assert res.best_per_set().tolist() == [1, -1, 5, -1]  # a tie, all +inf, one row, no row


def test_profiles_at_between_and_below_the_interfaces():
    res = ensemble()
    depths = [0.0, 0.005, 0.01, 0.02, 0.03, 0.5]  # the surface, inside, on an interface, inside, on the last, below
    vs = res.profiles(depths)
    assert vs.shape == (6, 6)
    assert np.array_equal(vs[:5], np.arange(5)[:, None] + np.array([0.1, 0.1, 0.2, 0.2, 0.3, 0.3]))
    assert np.array_equal(vs[5], 5 + np.array([0.1, 0.1, 0.1, 0.3, 0.3, 0.3]))  # both interfaces at 0.02
    assert np.array_equal(res.profiles(depths, "velocity_p"), 2.0 * vs)
    assert (res.profiles(depths, "density") == 1.5).all()
    with pytest.raises(ValueError):
        res.profiles(depths, "poisson")


def test_profile_stats_over_the_best_rows():
    res = ensemble()
    depths = [0.005, 0.01, 0.5]
    stats = res.profile_stats(depths)  # rows 1 and 5
    rows = res.profiles(depths)[[1, 5]]
    assert stats.mean.shape == stats.std.shape == (3,) and stats.percentiles.shape == (5, 3)
    assert np.array_equal(stats.mean, rows.mean(axis=0)) and np.array_equal(stats.std, rows.std(axis=0))
    assert np.array_equal(stats.percentiles, np.percentile(rows, (0, 25, 50, 75, 100), axis=0))
    assert np.array_equal(stats.percentiles[0], rows.min(axis=0)) and np.array_equal(stats.percentiles[4], rows[1])
    some = res.profile_stats(depths, "velocity_p", percentiles=(50,), rows=[0, 2, 4])
    assert some.percentiles.shape == (1, 3) and np.array_equal(some.percentiles[0], 2.0 * res.profiles(depths)[2])
    res.misfits[:] = np.inf
    with pytest.raises(ValueError):
        res.profile_stats(depths)
