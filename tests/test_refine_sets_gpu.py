"""Observation sets on the device: dvh_lm_normal_sets bit for bit against dvh_lm_normal per set and on the reduced
tables of absent samples (the cases of tests/refine_sets_ref.py), and EarthModel.refine_sets row by row against
EarthModel.refine on that row's set alone; then the chain from bootstrap ridges to a Vs spread."""
import numpy as np
import pytest
import torch

from tests import refine_ref as ref
from tests import refine_sets_ref as sets_ref
from tests.test_inversion_replay_gpu import FREQS, TRUE_H, TRUE_NU, TRUE_VS, density, earth_model
from tests.test_refine_gpu import POISON, normal_dev
from tests.test_refine_sets_host import (check_absent_samples, check_present_sets, check_set_flags, same_bits,
                                         sets_host)
from tests.test_refine_sets_host import lib  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def sets_dev(device, c, dcdp, chain, tab, set_obs, set_sigma, model_set, rho_floor=ref.RHO_FLOOR):
    """One raw dvh_lm_normal_sets launch over poisoned outputs of a model more than asked -> NumPy (f, g, H, status)."""
    from das_diff_veh_amd import _lib
    M, (K, D) = c.shape[0], chain.shape[1:]
    n_set, S = set_obs.shape
    model_set = np.ascontiguousarray(model_set, np.int32)
    assert set_sigma.shape == (n_set, S) and model_set.shape == (M,) and tab["sample_curve"].size == S
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    t = [put(a) for a in (c, dcdp, chain, tab["sample_period"], tab["sample_mode"], set_obs, set_sigma, model_set,
                          tab["sample_curve"], tab["curve_weight"])]
    f, g, H = (torch.full(s, POISON, dtype=torch.float64, device=device) for s in ((M + 1,), (M + 1, D), (M + 1, D, D)))
    status = torch.full((M + 1,), -7, dtype=torch.int32, device=device)
    _lib.call("dvh_lm_normal_sets", *(_lib.ptr(a) for a in t[:3]), M, ref.N_PERIOD, ref.N_MODE, K // 4, D,
              *(_lib.ptr(a) for a in t[3:8]), n_set, _lib.ptr(t[8]), S, _lib.ptr(t[9]), tab["curve_weight"].size,
              rho_floor, _lib.ptr(f), _lib.ptr(g), _lib.ptr(H), _lib.ptr(status), _lib.stream_of(device))
    f, g, H, status = (a.cpu().numpy() for a in (f, g, H, status))
    assert f[M] == POISON and (g[M] == POISON).all() and (H[M] == POISON).all() and status[M] == -7
    assert not (g[:M] == POISON).any() and not (H[:M] == POISON).any() and not (status[:M] == -7).any()
    return f[:M], g[:M], H[:M], status[:M]


# ------------------------------------------------------------------------------------------------ the entry itself

@pytest.mark.parametrize("S", sorted(ref.CURVE_SIZES))
@pytest.mark.parametrize("n_layer,D", ref.SHAPES)
def test_present_sets_are_lm_normal_per_set(device, n_layer, D, S):
    check_present_sets(lambda *a: sets_dev(device, *a), lambda *a: normal_dev(device, *a), n_layer, D, S)


def test_absent_samples_are_the_reduced_table(device):
    check_absent_samples(lambda *a: sets_dev(device, *a), lambda *a: normal_dev(device, *a))


def test_flags_touch_only_their_own_model(device):
    check_set_flags(lambda *a: sets_dev(device, *a))


def assert_within_normal_bound(got, host, c, dcdp, chain, tab, n_layer, name):
    """Device against host twin: g and H within refine_ref.normal_bound of their absolute-value expressions (the bound
    of either against the exact value, which covers the device's FMA contraction), f within it relative."""
    S = tab["sample_obs"].size
    _, _, _, ga, Ha = ref.normal_reference(c, dcdp, chain, tab)
    bound = ref.normal_bound(n_layer, S)
    dg, dH = np.abs(got[1] - host[1]) / ga, np.abs(got[2] - host[2]) / Ha
    df = np.abs(got[0] - host[0]) / host[0]
    print(f"{name}: device against host g {float(dg.max()):.2e}, H {float(dH.max()):.2e}, f {df.max():.2e} "
          f"of bound {bound:.2e}")
    assert np.array_equal(got[3], host[3]) and (dg <= bound).all() and (dH <= bound).all() and (df <= bound).all()


@pytest.mark.parametrize("n_layer,D,S", [(1, 2, 1), (3, 8, 13), (32, 95, 257)])
def test_sets_against_the_host_twin(device, lib, n_layer, D, S):
    from tests.test_refine_host import case_arrays
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    set_obs, set_sigma = sets_ref.present_sets(n_layer, D, S)
    cases = [("present", set_obs, None)]
    if (n_layer, D, S) == sets_ref.ABSENT_SHAPE:
        cases += [(name, sets_ref.with_absent(set_obs, 1, absent), absent) for name, absent in sets_ref.absent_cases()]
    for name, obs, absent in cases:
        got = sets_dev(device, c, dcdp, chain, tab, obs, set_sigma, (1, 1, 1))
        host = sets_host(lib, c, dcdp, chain, tab, obs, set_sigma, (1, 1, 1))
        table = sets_ref.table_of_set(tab, set_obs, set_sigma, 1)
        if absent is not None:
            table = sets_ref.reduced_table(table, absent)
        assert_within_normal_bound(got, host, c, dcdp, chain, table, n_layer, name)


@pytest.mark.parametrize("n_layer,D,S", [(3, 8, 13), (32, 95, 257)])
def test_position_independence(device, n_layer, D, S):
    """A model's outputs are unchanged when the batch is reversed and when it is launched alone."""
    from tests.test_refine_host import case_arrays
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    set_obs, set_sigma = sets_ref.present_sets(n_layer, D, S)
    if (n_layer, D, S) == sets_ref.ABSENT_SHAPE:
        set_obs = sets_ref.with_absent(set_obs, 2, sets_ref.absent_cases()[2][1])
    model_set = np.array([2, 0, 2], np.int32)
    batch = sets_dev(device, c, dcdp, chain, tab, set_obs, set_sigma, model_set)
    assert (batch[3] == 0).all()
    back = sets_dev(device, c[::-1], dcdp[::-1], chain[::-1], tab, set_obs, set_sigma, model_set[::-1])
    assert all(np.array_equal(a[::-1], b) for a, b in zip(back, batch))
    for m in range(ref.N_MODEL):
        alone = sets_dev(device, c[m:m + 1], dcdp[m:m + 1], chain[m:m + 1], tab, set_obs, set_sigma,
                         model_set[m:m + 1])
        assert same_bits(alone, batch, 0, m), m


# ----------------------------------------------------------- refine_sets on the three-layer model of the swarm replay

K_SETS, MAXITER = 5, 6
MODEL_SET = np.array([0, 1, 1, 2, 3, 3, 4])  # seven starts, two sets with two starts each
FIELDS = ("xs", "misfits", "history", "accepted", "lam", "status", "gradient", "hessian")
TRUE_X = np.array(TRUE_H + TRUE_VS + TRUE_NU)


START_WIDTH, BOX_WIDTH = 0.1, 0.3  # in the unit cube: where the starts lie, and where mode 1 is asked to exist


def unit_of(x, lo, hi):
    return np.where(hi > lo, (x - lo) / np.where(hi > lo, hi - lo, 1.0), 0.0)


def corners(lo, hi, width):
    """The true model and every corner of the box of +-width around it in the free coordinates of the unit cube,
    cut to the cube."""
    free = np.flatnonzero(hi > lo)
    u0 = unit_of(TRUE_X, lo, hi)
    rows = [TRUE_X]
    for bits in range(1 << free.size):
        u = u0.copy()
        u[free] = np.clip(u0[free] + np.where((bits >> np.arange(free.size)) & 1, width, -width), 0.0, 1.0)
        rows.append(lo + u * (hi - lo))
    return np.stack(rows)


@pytest.fixture(scope="module")
def problem(device):
    """Modes 0 and 1 of the true model on the eight periods of the swarm replay; five sets of seeded noisy data of one
    percent, and seven starts within START_WIDTH of the true model in the unit cube.

    Mode 1 is cut off below a frequency that moves with the model.  Over the whole bounds it does not exist at any of
    the eight periods (at 25 Hz 4 of the 64 corners lack it, at 5 Hz 44 do), so its curve keeps the periods at which it
    exists at the true model and at every corner of the box of BOX_WIDTH around it, three times as wide as the starts
    lie (the four shortest, when this was written).  A trial step that leaves that region for a model without the mode
    gets f = +inf and is refused, by refine and refine_sets alike."""
    from das_diff_veh_amd.inversion import Curve, phase_velocity, rayleigh_modes
    model = earth_model()
    lo, hi = model.bounds()
    period = 1.0 / FREQS[::-1]
    models = model.models_of(torch.from_numpy(corners(lo, hi, BOX_WIDTH)).to(device)).contiguous()
    c = rayleigh_modes(models, torch.from_numpy(period).to(device), 2, dc=model.dc, c_min=0.8 * 0.15).cpu().numpy()
    assert np.isfinite(c[:, :, 0]).all()
    has = np.isfinite(c[:, :, 1]).all(axis=0)                       # per period, ascending: the last are the lowest f
    n1 = int(np.argmin(has)) if not has.all() else has.size  # the periods before the first at which it is missing
    print(f"mode 1 exists over the box at {n1} of {period.size} periods")
    assert n1 >= 3
    rng = np.random.default_rng(12)
    vs, nu = np.array(TRUE_VS), np.array(TRUE_NU)
    vp = vs * np.sqrt((2 - 2 * nu) / (1 - 2 * nu))
    templates, data_sets = [], []
    for mode, per in ((0, period), (1, period[:n1])):
        true = phase_velocity(per, np.array(TRUE_H + [0.0]), vp, vs, density(vp), mode=mode)
        assert np.isfinite(true).all()
        templates.append(Curve(per, true, mode, "rayleigh", "phase", weight=1.0 + mode, uncertainties=0.01 * true))
        data_sets.append(true + rng.normal(0.0, 0.01, (K_SETS, per.size)) * true)
    u = unit_of(TRUE_X, lo, hi)
    u = np.clip(u + rng.uniform(-START_WIDTH, START_WIDTH, (MODEL_SET.size, lo.size)) * (hi > lo), 0.0, 1.0)
    return dict(model=model, templates=templates, data_sets=data_sets, xs=lo + u * (hi - lo), lo=lo, hi=hi)


@pytest.fixture(scope="module")
def ensemble(problem):
    p = problem
    return p["model"].refine_sets(p["templates"], p["data_sets"], p["xs"], model_set=MODEL_SET, maxiter=MAXITER)


def curves_of_set(problem, data_sets, k):
    from das_diff_veh_amd.inversion import Curve
    return [Curve(t.period, d[k], t.mode, "rayleigh", "phase", weight=t.weight, uncertainties=t.uncertainties)
            for t, d in zip(problem["templates"], data_sets)]


def test_refine_sets_is_refine_per_set(problem, ensemble):
    """Every field of row m is what refine gives for start m alone against the curves of its set, bit for bit."""
    assert ensemble.xs.shape == (7, 8) and ensemble.history.shape == (MAXITER + 1, 7) and ensemble.n_set == K_SETS
    assert np.array_equal(ensemble.model_set, MODEL_SET) and (ensemble.status & 1 == 0).all()
    assert np.isfinite(ensemble.start_misfits).all() and ensemble.accepted.any(axis=0).all()
    for m, k in enumerate(MODEL_SET):
        one = problem["model"].refine(curves_of_set(problem, problem["data_sets"], k), problem["xs"][m:m + 1],
                                      maxiter=MAXITER)
        for name in FIELDS:
            a, b = getattr(ensemble, name), getattr(one, name)
            a, b = (a[:, m], b[:, 0]) if name in ("history", "accepted") else (a[m], b[0])
            assert np.array_equal(a, b), (m, k, name)
    # two starts of one set go their own ways, and two sets from nearby starts differ
    assert not np.array_equal(ensemble.history[:, 1], ensemble.history[:, 2])


@pytest.fixture(scope="module")
def with_gaps(problem):
    """The five sets and two more: set 5 is set 0 without its mode-1 curve, set 6 has no sample at all; start 0 again
    on each."""
    p = problem
    data = [np.concatenate([d, d[:1], np.full_like(d[:1], np.nan)]) for d in p["data_sets"]]
    data[1][5] = np.nan
    xs = np.concatenate([p["xs"], p["xs"][:1], p["xs"][:1]])
    model_set = np.concatenate([MODEL_SET, [5, 6]])
    run = lambda: p["model"].refine_sets(p["templates"], data, xs, model_set=model_set, maxiter=MAXITER)
    return dict(res=run(), again=run(), xs=xs, data=data)


def test_rows_do_not_depend_on_the_other_sets(ensemble, with_gaps):
    for name in FIELDS + ("models", "start_misfits"):
        a, b = getattr(ensemble, name), getattr(with_gaps["res"], name)
        assert np.array_equal(a, b[:, :7] if name in ("history", "accepted") else b[:7]), name


def test_a_set_that_lacks_a_curve_is_refine_on_the_other_curve(problem, with_gaps):
    """The tables differ (refine scans one mode, the sets two), so what the presence rule fixes is compared: the
    misfit after every iteration, what was accepted and the damping."""
    res = with_gaps["res"]
    one = problem["model"].refine(curves_of_set(problem, problem["data_sets"], 0)[:1], problem["xs"][:1],
                                  maxiter=MAXITER)
    assert res.status[7] & 1 == 0 and np.isfinite(res.history[:, 7]).all()
    assert np.array_equal(res.history[:, 7], one.history[:, 0])
    assert np.array_equal(res.accepted[:, 7], one.accepted[:, 0]) and res.lam[7] == one.lam[0]
    assert not np.array_equal(res.history[:, 7], res.history[:, 0])  # set 0 with both curves is another problem


def test_properties_of_the_ensemble(problem, with_gaps):
    res, again, lo, hi = with_gaps["res"], with_gaps["again"], problem["lo"], problem["hi"]
    # a set of all NaN: status bit 0, the start returned unchanged, never accepted
    assert res.status[8] & 1 and np.array_equal(res.xs[8], with_gaps["xs"][8]) and not res.accepted[:, 8].any()
    assert (res.history[:, 8] == np.inf).all() and res.misfits[8] == np.inf
    assert (res.status[:8] & 1 == 0).all()
    assert (res.history[1:] <= res.history[:-1]).all()
    fixed = lo == hi
    assert fixed.sum() == 2 and (res.xs[:, fixed] == lo[fixed]).all()
    assert (res.xs >= lo).all() and (res.xs <= hi).all()
    for name in FIELDS + ("models", "start_misfits", "model_set"):
        assert np.array_equal(getattr(res, name), getattr(again, name)), name
    assert res.best_per_set().tolist() == [0, int(np.argmin(res.misfits[1:3])) + 1, 3,
                                           int(np.argmin(res.misfits[4:6])) + 4, 6, 7, -1]


def test_from_ridges_to_a_vs_spread(problem):
    """sets_from_ridges on synthetic bootstrap ridges (the true curves plus seeded noise, B = 16) into refine_sets into
    profile_stats."""
    from das_diff_veh_amd.inversion import sets_from_ridges
    B = 16
    rng = np.random.default_rng(3)
    t0, t1 = problem["templates"]
    n1 = t1.period.size
    ridges = [1000.0 * t.data[::-1] * (1.0 + rng.normal(0.0, 0.01, (B, t.period.size))) for t in (t0, t1)]
    lb, ub = [FREQS[0], FREQS[-n1]], [FREQS[-1] + 1.0, FREQS[-1] + 1.0]
    curves, data_sets = sets_from_ridges(FREQS, lb, ub, ridges, modes=[0, 1])
    assert [c.period.size for c in curves] == [8, n1] and data_sets[0].shape == (B, 8)
    assert np.allclose(curves[0].period, t0.period, rtol=1e-15, atol=0)
    res = problem["model"].refine_sets(curves, data_sets, np.tile(problem["xs"][:1], (B, 1)), maxiter=MAXITER)
    assert res.best_per_set().tolist() == list(range(B))
    assert (res.misfits < res.start_misfits).all()
    depths = np.linspace(0.0, 0.03, 7)
    stats = res.profile_stats(depths, "velocity_s")
    assert stats.mean.shape == stats.std.shape == (7,) and stats.percentiles.shape == (5, 7)
    assert (stats.percentiles[0] <= stats.mean).all() and (stats.mean <= stats.percentiles[4]).all()
    assert (stats.std > 0).any() and (np.diff(stats.percentiles, axis=0) >= 0).all()
