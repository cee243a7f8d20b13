"""dvh_rayleigh_modes and dvh_curve_misfit on the device against the 80-digit oracle's recorded roots
(tests/golden/rayleigh.npz, tests/rayleigh_ref.py): every case, period and mode count, the boundary between two scan
rounds, batches, a scan point on a layer velocity, the misfit against its NumPy restatement, and the NumPy front."""
import numpy as np
import pytest
import torch

from tests import rayleigh_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-9        # the refinement's relative width, and (test_rayleigh_host.py) the bound on |c - c_ref| / c_ref
POISON = -777.25
PERIODS = np.array([1.0 / f for f in ref.FREQS])


@pytest.fixture(scope="module")
def recorded():
    return ref.load()


def launch(device, layers, periods, need, n_mode, c_min, dc=ref.DC, tol=TOL):
    """One dvh_rayleigh_modes launch over poisoned outputs -> (c [M, P, n_mode], count [M, P]) as NumPy."""
    from das_diff_veh_amd import _lib
    layers = np.ascontiguousarray(layers, np.float64)
    layers = layers[None] if layers.ndim == 2 else layers
    M, n_layer, _ = layers.shape
    periods = np.ascontiguousarray(periods, np.float64)
    L, T = torch.from_numpy(layers).to(device), torch.from_numpy(periods).to(device)
    nd = torch.from_numpy(np.ascontiguousarray(need, np.int32)).to(device)
    c = torch.full((M, periods.size, n_mode), POISON, dtype=torch.float64, device=device)
    count = torch.full((M, periods.size), -99, dtype=torch.int32, device=device)
    _lib.call("dvh_rayleigh_modes", _lib.ptr(L), M, n_layer, _lib.ptr(T), periods.size, _lib.ptr(nd), c_min, dc, tol,
              n_mode, _lib.ptr(c), _lib.ptr(count), _lib.stream_of(device))
    return c.cpu().numpy(), count.cpu().numpy()


def expect(roots, need, n_mode):
    want = np.full(n_mode, np.nan)
    n = min(need, roots.size)
    want[:n] = roots[:n]
    return want, n


def assert_modes(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / want[ok]
    assert (err <= TOL).all(), (err.max(), got, want)


def padded(layers, n):
    """The same medium as n rows: zero-thickness copies of the top layer above it (a layer with h = 0 is skipped)."""
    pad = np.repeat(layers[:1], n - len(layers), axis=0)
    pad[:, 0] = 0.0
    return np.concatenate([pad, layers])


@pytest.mark.parametrize("n_mode", [1, 5, 16])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_modes_match_the_oracle(device, recorded, name, n_mode):
    """One launch of mixed need per case and mode count: the roots to 1e-9 relative (the contract is 1e-6), NaN
    exactly where the oracle has no such mode or none is wanted, the counts, and no slot left unwritten."""
    layers = ref.CASES[name][0]
    need = np.array([n_mode, 0, n_mode, min(2, n_mode), n_mode - 1], np.int32)
    c, count = launch(device, layers, PERIODS, need, n_mode, ref.c_min_of(name))
    assert not (c == POISON).any() and not (count == -99).any()
    for i in range(len(ref.FREQS)):
        want, n = expect(recorded[name, i][1], int(need[i]), n_mode)
        assert count[0, i] == n, (name, i, count[0, i], n)
        assert_modes(c[0, i], want)


def test_sign_change_between_two_rounds(device, recorded):
    """c_min placed so that a root lies between point 63 and 64, or 127 and 128: the last lane of one round and the
    first of the next.  The roots below it stay above c_min, so every mode keeps its index."""
    for name, i, m in (("lvz", 0, 0), ("notebook", 0, 0), ("notebook", 0, 1)):
        roots = recorded[name, i][1]
        for k in (63.5, 127.5):
            c_min = float(roots[m] - k * ref.DC)
            assert 0.0 < c_min < roots[0] - ref.DC
            c, count = launch(device, ref.CASES[name][0], PERIODS[i:i + 1], [16], 16, c_min)
            want, n = expect(roots, 16, 16)
            assert count[0, 0] == n
            assert_modes(c[0, 0], want)


def test_batch_equals_single_launches(device):
    """7 models x 3 periods (21 waves, not a multiple of the block's 4): each (model, period) equals its own launch
    bit for bit, NaN pattern and count included."""
    rng = np.random.default_rng(5)
    names = ["halfspace3", "one_layer", "notebook", "lvz", "dyadic"]
    models = [padded(ref.CASES[n][0], 6) for n in names]
    for _ in range(2):
        m = ref.CASES["notebook"][0].copy()
        m[:-1, 0] *= rng.uniform(0.8, 1.25, 5)
        vs = m[:, 2] * rng.uniform(0.9, 1.1, 6)
        models.append(ref.make_layers(m[:-1, 0], vs))
    models = np.stack(models)
    periods, need = PERIODS[[0, 2, 4]], np.array([3, 16, 7], np.int32)
    c, count = launch(device, models, periods, need, 16, 0.12)
    assert not (c == POISON).any()
    assert (count > 0).all() and len({tuple(x) for x in count}) > 3  # the models do differ
    for a in range(len(models)):
        for b in range(len(periods)):
            c1, n1 = launch(device, models[a], periods[b:b + 1], need[b:b + 1], 16, 0.12)
            assert n1[0, 0] == count[a, b]
            assert np.array_equal(c1[0, 0], c[a, b], equal_nan=True), (a, b)


def test_scan_point_on_a_layer_velocity(device, recorded):
    """The dyadic case's point 32 is exactly beta_2: no NaN, and the same roots as a scan moved off it."""
    layers, c_min = ref.CASES["dyadic"]
    assert ref.scan_points(layers, c_min)[32] == layers[1, 2]
    on, n_on = launch(device, layers, PERIODS, [16] * 5, 16, c_min)
    off, n_off = launch(device, layers, PERIODS, [16] * 5, 16, c_min - ref.DC / 3.0)
    assert np.array_equal(n_on, n_off)
    for i in range(len(ref.FREQS)):
        want, n = expect(recorded["dyadic", i][1], 16, 16)
        assert n_on[0, i] == n
        assert_modes(on[0, i], want)
        assert_modes(off[0, i], want)


def test_padding_layers_change_nothing(device):
    """Zero-thickness rows are skipped: the padded model's results equal the bare one's bit for bit."""
    layers = ref.CASES["lvz"][0]
    a = launch(device, layers, PERIODS, [16] * 5, 16, 0.144)
    b = launch(device, padded(layers, 9), PERIODS, [16] * 5, 16, 0.144)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------ misfit

def two_curves(uncertain):
    from das_diff_veh_amd.inversion import Curve
    rng = np.random.default_rng(11)
    p0, p1 = PERIODS[[4, 3, 2, 1]], PERIODS[[4, 3]]  # mode 1 exists at 16 and 25 Hz in the one-layer case
    return [Curve(p0, rng.uniform(0.2, 0.5, 4), 0, "rayleigh", "phase", weight=1.0,
                  uncertainties=rng.uniform(0.01, 0.05, 4) if uncertain else None),
            Curve(p1, rng.uniform(0.3, 0.5, 2), 1, "rayleigh", "phase", weight=2.0,
                  uncertainties=rng.uniform(0.01, 0.05, 2) if uncertain else None)]


def numpy_misfit(c, tab):
    g = lambda t: t.cpu().numpy()
    return ref.curve_misfit(g(c), g(tab.sample_period), g(tab.sample_mode), g(tab.sample_obs), g(tab.sample_sigma),
                            g(tab.sample_curve), g(tab.curve_weight))


@pytest.mark.parametrize("uncertain", [False, True])
def test_misfit_matches_numpy(device, uncertain):
    """Float64 sums of under 200 terms in the same order: 1e-12 relative."""
    from das_diff_veh_amd import inversion as inv
    tab = inv.sample_table(two_curves(uncertain), device)
    assert tab.periods.numel() == 4 and tab.n_mode == 2 and tab.need.tolist() == [2, 2, 1, 1]
    rng = np.random.default_rng(3)
    models = np.stack([ref.make_layers([0.01 * s], [0.2 * s, 0.5]) for s in rng.uniform(0.9, 1.1, 5)])
    c = inv.rayleigh_modes(torch.from_numpy(models).to(device), tab.periods, 2, dc=ref.DC, c_min=0.14, need=tab.need)
    got = inv.curve_misfit(c, tab).cpu().numpy()
    want = numpy_misfit(c, tab)
    assert np.isfinite(want).all() and (want > 0).all()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (got, want)
    # one missing sample -> +inf, the other models untouched
    c2 = c.clone()
    c2[3, 0, 1] = float("nan")
    got2 = inv.curve_misfit(c2, tab).cpu().numpy()
    assert got2[3] == np.inf and numpy_misfit(c2, tab)[3] == np.inf
    assert np.array_equal(np.delete(got2, 3), np.delete(got, 3))


def test_true_model_scores_zero(device):
    from das_diff_veh_amd import inversion as inv
    layers = ref.CASES["one_layer"][0]
    L = torch.from_numpy(layers[None]).to(device)
    T = torch.from_numpy(PERIODS[::-1].copy()).to(device)
    c = inv.rayleigh_modes(L, T, 2, dc=ref.DC, c_min=0.16).cpu().numpy()[0]
    curves = [inv.Curve(PERIODS[::-1][:4], c[:4, 0], 0, "rayleigh", "phase", uncertainties=0.01 * c[:4, 0]),
              inv.Curve(PERIODS[::-1][:2], c[:2, 1], 1, "rayleigh", "phase", weight=2.0)]
    tab = inv.sample_table(curves, device)
    got = inv.curve_misfit(inv.rayleigh_modes(L, tab.periods, tab.n_mode, dc=ref.DC, c_min=0.16, need=tab.need), tab)
    assert 0.0 <= float(got[0]) <= 1e-8


# ------------------------------------------------------------------------------------------------------ the NumPy front

def test_phase_velocity_is_rayleigh_modes(device, recorded):
    from das_diff_veh_amd import inversion as inv
    layers = ref.CASES["notebook"][0]
    c = inv.rayleigh_modes(torch.from_numpy(layers[None]).to(device), torch.from_numpy(PERIODS).to(device), 5)
    for mode in (0, 3, 4):
        pv = inv.phase_velocity(PERIODS, *layers.T, mode=mode)
        assert isinstance(pv, np.ndarray) and pv.shape == (5,)
        assert np.array_equal(pv, c[0, :, mode].cpu().numpy(), equal_nan=True)
        back = inv.phase_velocity(PERIODS[::-1], *layers.T, mode=mode)  # a reversed view, as the notebooks pass
        assert np.array_equal(back[::-1], pv, equal_nan=True)
        kept = pv[pv > 0.0]  # the notebooks' filter drops the missing modes
        assert kept.size == sum(recorded["notebook", i][1].size > mode for i in range(5))
    # dc = 0.005 (the default) and the default c_min = 0.8 min(vs) find the recorded roots too
    for i in range(5):
        roots = recorded["notebook", i][1][:5]
        assert_modes(c[0, i, :roots.size].cpu().numpy(), roots)


def test_value_errors_before_device_work():
    from das_diff_veh_amd import inversion as inv
    p, d = [0.1, 0.2], [0.3, 0.4]
    with pytest.raises(ValueError, match="rayleigh"):
        inv.Curve(p, d, 0, "love", "phase")
    with pytest.raises(ValueError, match="phase"):
        inv.Curve(p, d, 0, "rayleigh", "group")
    m = inv.EarthModel().add(inv.Layer([0.001, 0.01], [0.1, 0.5], [0.4375, 0.4375]))
    with pytest.raises(ValueError, match='"pso"'):
        m.configure(optimizer="cpso")
    with pytest.raises(ValueError, match="rmse"):
        m.configure(optimizer="pso", misfit="norm1")
    with pytest.raises(ValueError):
        m.invert([inv.Curve(p, d, 0, "rayleigh", "phase")])  # not configured
