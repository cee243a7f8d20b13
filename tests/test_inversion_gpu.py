"""EarthModel.invert on the device: what follows from the definitions of the swarm, the misfit and the result layout
(das_diff_veh_amd/inversion.py), and one comparison against a random search scored by the same forward entries.  No
convergence figure is fixed: the measured ones are in DESIGN.md."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NU = 0.4375
TRUE_H, TRUE_VS = [0.005, 0.015], [0.2, 0.35, 0.6]
FREQS = np.linspace(4.0, 25.0, 12)
ARGS = dict(popsize=48, maxiter=60, seed=0)
MAXRUN = 2


def density(vp):
    return 1.56 + 0.186 * vp


def earth_model(args=ARGS):
    from das_diff_veh_amd.inversion import EarthModel, Layer
    m = EarthModel()
    m.add(Layer([0.002, 0.01], [0.1, 0.3], [NU, NU]))
    m.add(Layer([0.005, 0.03], [0.2, 0.5], [NU, NU]))
    m.add(Layer([0.01, 0.01], [0.4, 0.8], [NU, NU]))
    return m.configure(optimizer="pso", misfit="rmse", density=density, optimizer_args=dict(args))


@pytest.fixture(scope="module")
def curves(device):
    """Mode 0 at 12 periods and mode 1 at the 6 shortest, from the forward call on the true model; sigma 1 %."""
    from das_diff_veh_amd.inversion import Curve, phase_velocity
    vs = np.array(TRUE_VS)
    vp = vs * np.sqrt((2 - 2 * NU) / (1 - 2 * NU))
    period = 1.0 / FREQS[::-1]
    out = []
    for mode, p in ((0, period), (1, period[:6])):
        c = phase_velocity(p, np.array(TRUE_H + [0.0]), vp, vs, density(vp), mode=mode)
        assert np.isfinite(c).all()
        out.append(Curve(p, c, mode, "rayleigh", "phase", uncertainties=0.01 * c))
    return out


@pytest.fixture(scope="module")
def result(device, curves):
    return earth_model().invert(curves, maxrun=MAXRUN)


def rescore(model, curves, models, device):
    """dvh_rayleigh_modes + dvh_curve_misfit on (h, vp, vs, rho) rows, with invert()'s scan."""
    from das_diff_veh_amd import inversion as inv
    tab = inv.sample_table(curves, device)
    c_min = 0.8 * min(l.velocity_s[0] for l in model.layers)
    c = inv.rayleigh_modes(torch.from_numpy(np.ascontiguousarray(models)).to(device), tab.periods, tab.n_mode,
                           dc=model.dc, c_min=c_min, need=tab.need)
    return inv.curve_misfit(c, tab).cpu().numpy()


def test_result_layout_and_bounds(result):
    n_eval = MAXRUN * ARGS["popsize"] * ARGS["maxiter"]
    assert result.xs.shape == (n_eval, 8) and result.models.shape == (n_eval, 3, 4)
    assert result.misfits.shape == (n_eval,) and result.global_misfits.shape == (MAXRUN, ARGS["maxiter"])
    lo, hi = earth_model().bounds()
    assert (result.xs >= lo).all() and (result.xs <= hi).all()
    fixed = lo == hi
    assert fixed.sum() == 3 and (result.xs[:, fixed] == lo[fixed]).all()  # nu; the half-space's h is not a parameter
    free = result.xs[:, ~fixed]
    assert (free.std(axis=0) > 0).all()
    h, vp, vs, rho = (result.models[:, :, k] for k in range(4))
    assert np.array_equal(h[:, :2], result.xs[:, :2]) and (h[:, 2] == 0).all()
    assert np.array_equal(vs, result.xs[:, 2:5])
    assert np.allclose(vp, vs * np.sqrt((2 - 2 * NU) / (1 - 2 * NU)), rtol=1e-15, atol=0)
    assert np.allclose(rho, density(vp), rtol=1e-15, atol=0)


def test_misfits_are_the_misfit_entry_on_the_models(device, curves, result):
    again = rescore(earth_model(), curves, result.models, device)
    assert np.array_equal(again, result.misfits)
    assert np.isfinite(result.misfits).any()
    assert result.misfit == result.misfits.min()
    assert np.array_equal(result.model, result.models[np.argmin(result.misfits)])


def test_best_so_far_never_rises(result):
    f = result.misfits.reshape(MAXRUN, ARGS["maxiter"], ARGS["popsize"])
    best = np.minimum.accumulate(f.min(axis=2), axis=1)
    assert np.array_equal(best, result.global_misfits)
    assert (np.diff(result.global_misfits, axis=1) <= 0).all()
    assert not np.array_equal(f[0], f[1])  # the runs are independent swarms


def test_same_seed_same_result(curves, result):
    again = earth_model().invert(curves, maxrun=MAXRUN)
    assert np.array_equal(again.xs, result.xs) and np.array_equal(again.misfits, result.misfits)
    other = earth_model(dict(ARGS, seed=1, maxiter=2)).invert(curves, maxrun=MAXRUN)
    assert not np.array_equal(other.xs[:ARGS["popsize"]], result.xs[:ARGS["popsize"]])


def test_a_mode_that_never_exists(device):
    from das_diff_veh_amd.inversion import Curve
    never = [Curve([0.4, 0.3], [0.3, 0.3], 10, "rayleigh", "phase")]
    res = earth_model(dict(popsize=8, maxiter=3, seed=0)).invert(never, maxrun=2)
    assert res.misfits.shape == (48,) and np.isposinf(res.misfits).all() and np.isposinf(res.misfit)
    assert np.isposinf(res.global_misfits).all() and res.model.shape == (3, 4)


def test_beats_a_random_search(device, curves, result):
    """The same number of evaluations drawn uniformly over the same bounds and scored by the same entries."""
    model = earth_model()
    lo, hi = model.bounds()
    rng = np.random.default_rng(0)
    xs = lo + rng.uniform(size=(result.misfits.size, lo.size)) * (hi - lo)
    models = model.models_of(torch.from_numpy(xs).to(device)).cpu().numpy()
    baseline = rescore(model, curves, models, device).min()
    print(f"best misfit: swarm {result.misfit:.4g}, random search {baseline:.4g}, runs {result.global_misfits[:, -1]}")
    assert result.misfit < baseline
