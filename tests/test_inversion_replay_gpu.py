"""EarthModel.invert's swarm recurrence replayed in NumPy float64: the same draws from a torch.Generator of the same
seed, `result.misfits` as the objective, and per iteration the personal-best update on strict `<`, each run's argmin,
the velocity in the expression's own order, the `free` mask and the clamp.  A wrong gather index, swapped c1 / c2
draws or a personal best taken from the wrong tensor move the positions in the first iterations."""
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TRUE_H, TRUE_VS, TRUE_NU = [0.006, 0.012], [0.2, 0.35, 0.6], [0.3, 0.33, 0.25]
FREQS = np.linspace(5.0, 25.0, 8)
POPSIZE, MAXITER, MAXRUN, SEED = 12, 15, 3, 4
D = 8


def density(vp):
    return 1.56 + 0.186 * vp


def earth_model():
    """h0 free, h1 fixed; vs free in all three; Poisson's ratio free in two layers and fixed in the half-space."""
    from das_diff_veh_amd.inversion import EarthModel, Layer
    m = EarthModel()
    m.add(Layer([0.003, 0.01], [0.15, 0.25], [0.2, 0.4]))
    m.add(Layer([0.012, 0.012], [0.3, 0.45], [0.25, 0.4]))
    m.add(Layer([0.01, 0.01], [0.5, 0.8], [0.25, 0.25]))
    return m.configure(optimizer="pso", misfit="rmse", density=density,
                       optimizer_args=dict(popsize=POPSIZE, maxiter=MAXITER, seed=SEED))


@pytest.fixture(scope="module")
def result(device):
    from das_diff_veh_amd.inversion import Curve, phase_velocity
    vs, nu = np.array(TRUE_VS), np.array(TRUE_NU)
    vp = vs * np.sqrt((2 - 2 * nu) / (1 - 2 * nu))
    period = 1.0 / FREQS[::-1]
    c = phase_velocity(period, np.array(TRUE_H + [0.0]), vp, vs, density(vp), mode=0)
    assert np.isfinite(c).all()
    return earth_model().invert([Curve(period, c, 0, "rayleigh", "phase", uncertainties=0.01 * c)], maxrun=MAXRUN)


@pytest.fixture(scope="module")
def replay(device, result):
    """dict(x [R, T, N, D] with separate multiply and add, x_fma with them fused, best [R, T], unique: every run's
    smallest personal best is held by one particle at every iteration)."""
    from das_diff_veh_amd.inversion import PSO_C1, PSO_C2, PSO_W
    R, N, T = MAXRUN, POPSIZE, MAXITER
    gen = torch.Generator(device=device)
    gen.manual_seed(SEED)
    draws = [torch.rand((R, N, D), dtype=torch.float64, device=device, generator=gen).cpu().numpy()
             for _ in range(1 + 2 * T)]
    lo, hi = earth_model().bounds()
    span = hi - lo
    free = (span > 0).astype(np.float64)
    f_all = result.misfits.reshape(R, T, N)
    u = draws[0] * free
    v = np.zeros_like(u)
    pbest_u, pbest_f = u.copy(), np.full((R, N), np.inf)
    x, x_fma, best, unique = np.empty((R, T, N, D)), np.empty((R, T, N, D)), np.empty((R, T)), True
    lo_q, span_q = [Fraction(a) for a in lo], [Fraction(a) for a in span]
    for it in range(T):
        x[:, it] = lo + u * span
        x_fma[:, it] = [[[float(lo_q[d] + Fraction(u[r, n, d]) * span_q[d]) for d in range(D)] for n in range(N)]
                        for r in range(R)]
        f = f_all[:, it]
        better = f < pbest_f
        pbest_f = np.where(better, f, pbest_f)
        pbest_u = np.where(better[..., None], u, pbest_u)
        g_at = pbest_f.argmin(axis=1)
        best[:, it] = pbest_f.min(axis=1)
        unique = unique and all((pbest_f[r] == best[r, it]).sum() == 1 for r in range(R))
        g_u = pbest_u[np.arange(R), g_at][:, None, :]
        c1, c2 = draws[1 + 2 * it], draws[2 + 2 * it]
        v = (PSO_W * v + PSO_C1 * c1 * (pbest_u - u) + PSO_C2 * c2 * (g_u - u)) * free
        u = np.clip(u + v, 0.0, 1.0)
    return dict(x=x, x_fma=x_fma, best=best, unique=unique)


def test_every_misfit_is_finite_and_every_argmin_unique(result, replay):
    """What the replay rests on: the objective is finite everywhere (mode 0 exists all over the bounds) and a tie never
    leaves the device's argmin unspecified."""
    assert result.misfits.shape == (MAXRUN * MAXITER * POPSIZE,) and np.isfinite(result.misfits).all()
    assert replay["unique"]
    assert (np.diff(replay["best"], axis=1) < 0).any(axis=1).all()  # every run does improve: personal bests move


def test_positions_are_the_replayed_recurrence(result, replay):
    """Within 2 float64 spacings of every value; the recurrence on the unit cube is separate IEEE operations in a
    fixed order and only addcmul may fuse its multiply-add, so the positions equal one of the two replays bit for
    bit."""
    xs = result.xs.reshape(MAXRUN, MAXITER, POPSIZE, D)
    err = np.abs(xs - replay["x"]) / np.spacing(np.abs(replay["x"]))
    print(f"largest difference from the replay: {err.max():.1f} spacings; equal to the separate replay: "
          f"{np.array_equal(xs, replay['x'])}, to the fused one: {np.array_equal(xs, replay['x_fma'])}")
    assert err.max() <= 2.0, np.unravel_index(err.argmax(), err.shape)
    assert np.array_equal(xs, replay["x"]) or np.array_equal(xs, replay["x_fma"])
    assert (xs != xs[0, 0, 0]).any(axis=(0, 1, 2)).sum() == 6  # the swarm moves in every free parameter


def test_best_so_far_is_the_replays(result, replay):
    assert result.global_misfits.shape == (MAXRUN, MAXITER)
    assert np.array_equal(result.global_misfits, replay["best"])


def test_fixed_parameters_sit_at_their_bound(result):
    lo, hi = earth_model().bounds()
    fixed = lo == hi
    assert fixed.tolist() == [False, True, False, False, False, False, False, True]
    assert (result.xs[:, fixed] == lo[fixed]).all()
    assert (result.xs >= lo).all() and (result.xs <= hi).all()


def test_models_are_models_of_the_replayed_positions(device, result, replay):
    xs = result.xs.reshape(MAXRUN, MAXITER, POPSIZE, D)
    x = replay["x_fma"] if np.array_equal(xs, replay["x_fma"]) else replay["x"]
    models = earth_model().models_of(torch.from_numpy(x.reshape(-1, D)).to(device)).cpu().numpy()
    assert models.shape == result.models.shape == (MAXRUN * MAXITER * POPSIZE, 3, 4)
    assert np.array_equal(models, result.models)
    # and they are the layer rows of the parameters: h with the half-space's 0, vp from vs and nu, rho from vp
    h, vs, nu = x.reshape(-1, D)[:, :2], x.reshape(-1, D)[:, 2:5], x.reshape(-1, D)[:, 5:]
    vp = vs * np.sqrt((2.0 - 2.0 * nu) / (1.0 - 2.0 * nu))
    assert np.array_equal(models[:, :2, 0], h) and (models[:, 2, 0] == 0).all() and np.array_equal(models[:, :, 2], vs)
    assert np.allclose(models[:, :, 1], vp, rtol=1e-15, atol=0)
    assert np.allclose(models[:, :, 3], density(vp), rtol=1e-15, atol=0)
