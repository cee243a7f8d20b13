"""dvh_curve_misfit against its NumPy restatement (tests/rayleigh_ref.py:curve_misfit) at real grid sizes, one thread
per model in blocks of 256: one model, a block less one, a full block, a block and one, three blocks with a ragged
tail; sample tables that are not grouped by curve; the +inf cases of include/dvh.h; and inversion.sample_table."""
import numpy as np
import pytest
import torch

from tests import rayleigh_ref as ref

pytestmark = pytest.mark.gpu

POISON = -777.25
N_PERIOD, N_MODE = 4, 3
CURVE_SIZES = (5, 1, 7)


def table(seed=7):
    """Three curves of 5, 1 and 7 samples, grouped by curve, with random sigma and weights: a dict of NumPy arrays."""
    rng = np.random.default_rng(seed)
    n = sum(CURVE_SIZES)
    return dict(sample_period=rng.integers(0, N_PERIOD, n).astype(np.int32),
                sample_mode=rng.integers(0, N_MODE, n).astype(np.int32),
                sample_obs=rng.uniform(0.2, 0.9, n), sample_sigma=rng.uniform(0.01, 0.05, n),
                sample_curve=np.repeat(np.arange(3), CURVE_SIZES).astype(np.int32),
                curve_weight=rng.uniform(0.5, 2.0, 3))


def velocities(M, seed=1):
    return np.random.default_rng(seed).uniform(0.1, 1.0, (M, N_PERIOD, N_MODE))


def launch(device, c, tab):
    """One dvh_curve_misfit launch into a poisoned buffer of M + 1 doubles -> [M]; the last one must stay poisoned."""
    from das_diff_veh_amd import _lib
    M, P, n_mode = c.shape
    C = torch.from_numpy(np.ascontiguousarray(c)).to(device)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in tab.items()}
    out = torch.full((M + 1,), POISON, dtype=torch.float64, device=device)
    _lib.call("dvh_curve_misfit", _lib.ptr(C), M, P, n_mode, _lib.ptr(t["sample_period"]), _lib.ptr(t["sample_mode"]),
              _lib.ptr(t["sample_obs"]), _lib.ptr(t["sample_sigma"]), _lib.ptr(t["sample_curve"]),
              tab["sample_obs"].size, _lib.ptr(t["curve_weight"]), tab["curve_weight"].size, _lib.ptr(out),
              _lib.stream_of(device))
    out = out.cpu().numpy()
    assert out[M] == POISON and not (out[:M] == POISON).any()
    return out[:M]


def numpy_misfit(c, tab):
    return ref.curve_misfit(c, **tab)


def shuffled(tab, seed=2):
    order = np.random.default_rng(seed).permutation(tab["sample_obs"].size)
    out = {k: (v if k == "curve_weight" else v[order]) for k, v in tab.items()}
    assert (np.diff(out["sample_curve"]) < 0).any()  # interleaved: no longer grouped by curve
    return out


@pytest.mark.parametrize("M", [1, 255, 256, 257, 600])
def test_misfit_matches_numpy_at_every_grid_size(device, M):
    """Float64 sums of at most 7 terms in the same order: 1e-12 relative, for the grouped table and for the same
    samples shuffled (the sums follow table order); nothing is written past model M - 1."""
    c = velocities(M)
    for tab in (table(), shuffled(table())):
        got, want = launch(device, c, tab), numpy_misfit(c, tab)
        assert np.isfinite(want).all() and (want > 0).all()
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), np.abs(got / want - 1.0).max()
    if M > 1:
        assert np.unique(got).size == M  # every model has its own row of c


def test_samples_outside_c_give_inf(device):
    """A sample with sample_period = n_period or -1, or sample_mode = n_mode or -1, gives +inf for every model."""
    c = velocities(257)
    for key, bad in (("sample_period", N_PERIOD), ("sample_period", -1), ("sample_mode", N_MODE), ("sample_mode", -1)):
        for at in (0, 5, 12):  # a sample of each curve
            tab = table()
            tab[key][at] = bad
            assert np.isposinf(launch(device, c, tab)).all(), (key, bad, at)


def test_a_curve_without_samples_gives_inf(device):
    """Four weights over samples that name three curves: the last curve has no sample, then a middle one."""
    c = velocities(257)
    tab = table()
    tab["curve_weight"] = np.r_[tab["curve_weight"], 1.0]
    assert np.isposinf(launch(device, c, tab)).all()  # curve 3 is named by no sample
    tab["sample_curve"] = np.where(tab["sample_curve"] == 2, 3, tab["sample_curve"]).astype(np.int32)
    assert np.isposinf(launch(device, c, tab)).all()  # nor curve 2 now


@pytest.mark.parametrize("at", [255, 256])
def test_one_nan_spoils_one_model(device, at):
    """A NaN in one sampled slot of model 255 (the last thread of block 0) or 256 (the first of block 1): that model
    alone is +inf, every other one keeps its bits."""
    c, tab = velocities(600), table()
    clean = launch(device, c, tab)
    c[at, tab["sample_period"][3], tab["sample_mode"][3]] = np.nan
    got = launch(device, c, tab)
    assert got[at] == np.inf and np.isfinite(clean).all()
    assert np.array_equal(np.delete(got, at), np.delete(clean, at))


def test_sample_table(device):
    """Two curves that share periods, one of them given unsorted and one reversed: `periods` is the sorted union,
    `need` the highest sampled mode plus one at each, sample_period indexes the union, and the samples keep the
    curves' own order."""
    from das_diff_veh_amd import inversion as inv
    p0 = np.array([0.2, 0.05, 0.1, 0.4])        # unsorted
    p1 = np.array([0.4, 0.25, 0.1])             # reversed; shares 0.4 and 0.1
    d0, d1 = np.array([0.5, 0.2, 0.3, 0.6]), np.array([0.8, 0.7, 0.5])
    s1 = np.array([0.02, 0.03, 0.04])
    curves = [inv.Curve(p0, d0, 0, "rayleigh", "phase", weight=1.5),
              inv.Curve(p1, d1, 2, "rayleigh", "phase", weight=0.5, uncertainties=s1)]
    tab = inv.sample_table(curves, device)
    g = lambda t: t.cpu().numpy()
    union = np.array([0.05, 0.1, 0.2, 0.25, 0.4])
    assert np.array_equal(g(tab.periods), union) and tab.n_mode == 3
    assert g(tab.need).tolist() == [1, 3, 1, 3, 3] and tab.need.dtype == torch.int32
    assert g(tab.sample_period).tolist() == [2, 0, 1, 4, 4, 3, 1] and tab.sample_period.dtype == torch.int32
    assert np.array_equal(union[g(tab.sample_period)], np.r_[p0, p1])
    assert g(tab.sample_mode).tolist() == [0] * 4 + [2] * 3 and g(tab.sample_curve).tolist() == [0] * 4 + [1] * 3
    assert np.array_equal(g(tab.sample_obs), np.r_[d0, d1]) and np.array_equal(g(tab.sample_sigma), np.r_[np.ones(4), s1])
    assert np.array_equal(g(tab.curve_weight), [1.5, 0.5])
    # and the table scores as NumPy scores it
    c = np.random.default_rng(9).uniform(0.1, 1.0, (257, 5, 3))
    got = g(inv.curve_misfit(torch.from_numpy(c).to(device), tab))
    want = ref.curve_misfit(c, g(tab.sample_period), g(tab.sample_mode), g(tab.sample_obs), g(tab.sample_sigma),
                            g(tab.sample_curve), g(tab.curve_weight))
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
