"""The Gauss-Newton refinement on the device: dvh_lm_normal and dvh_lm_solve against the np.longdouble references and
their host twins (tests/refine_ref.py), EarthModel.refine's gradient against central differences of the misfit, the
loop against its definition, recovery of a known model, and refinement of a swarm's result."""
import numpy as np
import pytest
import torch

from tests import refine_ref as ref
from tests.test_refine_host import case_arrays, check_flagged, check_position_independence, normal_host, solve_host
from tests.test_refine_host import lib  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

POISON = -777.25


def normal_dev(device, c, dcdp, chain, tab, rho_floor=ref.RHO_FLOOR):
    """One raw dvh_lm_normal launch over poisoned outputs of a model more than asked -> NumPy (f, g, H, status)."""
    from das_diff_veh_amd import _lib
    M, (K, D) = c.shape[0], chain.shape[1:]
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    t = [put(a) for a in (c, dcdp, chain, *(tab[k] for k in ref.TABLE_KEYS), tab["curve_weight"])]
    f, g, H = (torch.full(s, POISON, dtype=torch.float64, device=device) for s in ((M + 1,), (M + 1, D), (M + 1, D, D)))
    status = torch.full((M + 1,), -7, dtype=torch.int32, device=device)
    _lib.call("dvh_lm_normal", *(_lib.ptr(a) for a in t[:3]), M, ref.N_PERIOD, ref.N_MODE, K // 4, D,
              *(_lib.ptr(a) for a in t[3:8]), tab["sample_obs"].size, _lib.ptr(t[8]), tab["curve_weight"].size,
              rho_floor, _lib.ptr(f), _lib.ptr(g), _lib.ptr(H), _lib.ptr(status), _lib.stream_of(device))
    f, g, H, status = (a.cpu().numpy() for a in (f, g, H, status))
    assert f[M] == POISON and (g[M] == POISON).all() and (H[M] == POISON).all() and status[M] == -7
    assert not (g[:M] == POISON).any() and not (H[:M] == POISON).any() and not (status[:M] == -7).any()
    return f[:M], g[:M], H[:M], status[:M]


def solve_dev(device, H, g, lam, free):
    from das_diff_veh_amd import _lib
    M, D = g.shape
    t = [torch.from_numpy(np.array(a)).to(device) for a in (H, g, lam, free)]
    delta = torch.full((M + 1, D), POISON, dtype=torch.float64, device=device)
    status = torch.full((M + 1,), -7, dtype=torch.int32, device=device)
    _lib.call("dvh_lm_solve", *(_lib.ptr(a) for a in t), M, D, _lib.ptr(delta), _lib.ptr(status),
              _lib.stream_of(device))
    delta, status = delta.cpu().numpy(), status.cpu().numpy()
    assert (delta[M] == POISON).all() and status[M] == -7 and not (delta[:M] == POISON).any()
    return delta[:M], status[:M]


# ------------------------------------------------------------------------------------------------ host/device parity

@pytest.mark.parametrize("S", sorted(ref.CURVE_SIZES))
@pytest.mark.parametrize("n_layer,D", ref.SHAPES)
def test_normal_against_longdouble_and_the_host_twin(device, lib, n_layer, D, S):
    """The host test's reference and bound, and the host entry itself to 1e-13 of the absolute-value expression (the
    device compile contracts a * b + c into one FMA, the host compile does not)."""
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    got = normal_dev(device, c, dcdp, chain, tab)
    ref.assert_normal(got, n_layer, D, S)
    host = normal_host(lib, c, dcdp, chain, tab)
    _, _, _, ga, Ha = ref.normal_expected(n_layer, D, S)
    dg, dH = np.abs(got[1] - host[1]) / ga, np.abs(got[2] - host[2]) / Ha
    print(f"device against host: g {float(dg.max()):.2e}, H {float(dH.max()):.2e}, "
          f"f {np.abs(got[0] / host[0] - 1).max():.2e}")
    assert (dg <= 1e-13).all() and (dH <= 1e-13).all() and (np.abs(got[0] - host[0]) <= 1e-13 * host[0]).all()


def test_normal_flags_one_model(device):
    check_flagged(lambda *a: normal_dev(device, *a), 3, 8, 13)


@pytest.mark.parametrize("n_layer,D,S", [(3, 8, 13), (32, 95, 257)])
def test_normal_position_independence(device, n_layer, D, S):
    check_position_independence(lambda *a: normal_dev(device, *a), n_layer, D, S)


@pytest.mark.parametrize("D", ref.SOLVE_SIZES)
def test_solve_backward_error(device, lib, D):
    """The host test's bound.  The step itself may differ from the host twin's by the matrix's condition times the
    rounding (FMA contraction), so there is no absolute-value expression to hold it to: the model of condition 1e2 is
    held to the host twin within 1e2 x 1e-13, the others through the backward-error bound, their difference printed."""
    case = ref.solve_case(D)
    delta, status = solve_dev(device, case["H"], case["g"], case["lam"], case["free"])
    ref.assert_solve(delta, status, D)
    host, host_status = solve_host(lib, case["H"], case["g"], case["lam"], case["free"])
    assert np.array_equal(status, host_status)
    print("device against host, relative:",
          np.abs(delta - host).max(axis=1) / np.maximum(np.abs(host).max(axis=1), 1e-300))
    # the well-conditioned model (condition 1e2) against the host twin: the condition times 1e-13
    assert np.abs(delta[0] - host[0]).max() <= 1e2 * 1e-13 * np.abs(host[0]).max()
    for m in range(4):  # the refusing model leaves the others alone: each equals itself solved alone
        one, st = solve_dev(device, case["H"][m:m + 1], case["g"][m:m + 1], case["lam"][m:m + 1], case["free"])
        assert np.array_equal(one[0], delta[m]) and st[0] == status[m]


def test_solve_special_matrices(device):
    D = 5
    eye, g = np.eye(D), np.arange(1.0, D + 1)
    nan = eye.copy()
    nan[2, 1] = np.nan
    H = np.stack([np.zeros((D, D)), nan, eye, eye])
    delta, status = solve_dev(device, H, np.tile(g, (4, 1)), np.array([1e-3, 1e-3, np.inf, 0.0]), np.ones(D, np.int32))
    assert status.tolist() == [2, 2, 2, 0] and (delta[:3] == 0).all() and np.array_equal(delta[3], -g)
    delta, status = solve_dev(device, H[3:], g[None], np.array([0.0]), np.zeros(D, np.int32))
    assert status[0] == 2 and (delta == 0).all()


# ------------------------------------------------------------- the three-layer problem of tests/test_inversion_gpu.py

NU = 0.4375
TRUE_H, TRUE_VS = [0.005, 0.015], [0.2, 0.35, 0.6]
FREQS = np.linspace(4.0, 25.0, 12)
ARGS = dict(popsize=48, maxiter=60, seed=0)


def density(vp):
    return 1.56 + 0.186 * vp


def earth_model(args=ARGS):
    from das_diff_veh_amd.inversion import EarthModel, Layer
    m = EarthModel()
    m.add(Layer([0.002, 0.01], [0.1, 0.3], [NU, NU]))
    m.add(Layer([0.005, 0.03], [0.2, 0.5], [NU, NU]))
    m.add(Layer([0.01, 0.01], [0.4, 0.8], [NU, NU]))
    return m.configure(optimizer="pso", misfit="rmse", density=density, optimizer_args=dict(args))


TRUE_X = np.array(TRUE_H + TRUE_VS + [NU] * 3)


def around_truth(seed, count, width):
    """``count`` points at the true model plus a uniform perturbation of +-width in every free u_k."""
    lo, hi = earth_model().bounds()
    free = hi > lo
    u = np.where(free, (TRUE_X - lo) / np.where(free, hi - lo, 1.0), 0.0)
    u = u + np.random.default_rng(seed).uniform(-width, width, (count, lo.size)) * free
    assert (u >= 0).all() and (u <= 1).all()
    return lo + u * (hi - lo)


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


def misfit_at(model, curves, xs, device, tol=1e-13):
    """dvh_rayleigh_modes (roots to ``tol``) + dvh_curve_misfit at parameters xs [M, D], with invert()'s scan."""
    from das_diff_veh_amd import inversion as inv
    tab = inv.sample_table(curves, device)
    c_min = 0.8 * min(l.velocity_s[0] for l in model.layers)
    models = model.models_of(torch.from_numpy(np.ascontiguousarray(xs)).to(device)).contiguous()
    c = inv.rayleigh_modes(models, tab.periods, tab.n_mode, dc=model.dc, c_min=c_min, tol=tol, need=tab.need)
    return inv.curve_misfit(c, tab).cpu().numpy()


GRADIENT_STEP = 2e-4  # relative, in u_k
GRADIENT_SEEDS = (11, 12, 13, 14)


def test_gradient_against_central_differences(device, curves):
    """refine's gradient at four points (truth +- 0.2 in u) against central differences of curve_misfit with roots at
    tol = 1e-13, at the relative steps h and h / 2 in every free u_k: within 10 |fd(h) - fd(h / 2)| + 1e-9 |g|_max.
    With h = 2e-4 the truncation of the differences (about h^2 u^2 f''' / 6) and their rounding (the roots' 1e-13 over
    sigma = 1 %, over the step) are both near 1e-7 of the gradient.  A parameter whose two differences disagree by more
    than 1e-3 |g|_max has a renumbered mode inside its stencil (the misfit jumps) and is excluded: at most one in
    all."""
    model = earth_model()
    lo, hi = model.bounds()
    span = hi - lo
    free = np.flatnonzero(span > 0)
    xs = np.concatenate([around_truth(seed, 1, 0.2) for seed in GRADIENT_SEEDS])
    res = model.refine(curves, xs, maxiter=0)
    assert np.array_equal(res.xs, xs) and np.isfinite(res.misfits).all() and (res.status == 0).all()
    assert (res.gradient[:, span == 0] == 0).all()
    excluded, worst = 0, 0.0
    for at, x in enumerate(xs):
        u = (x - lo)[free] / span[free]
        fd = []
        for h in (GRADIENT_STEP, GRADIENT_STEP / 2):
            pts = np.repeat(x[None], 2 * free.size, axis=0)
            for j, k in enumerate(free):
                pts[2 * j, k] = lo[k] + (u[j] * (1 + h)) * span[k]
                pts[2 * j + 1, k] = lo[k] + (u[j] * (1 - h)) * span[k]
            f = misfit_at(model, curves, pts, device)
            du = (pts[0::2, free] - pts[1::2, free])[np.arange(free.size), np.arange(free.size)] / span[free]
            fd.append((f[0::2] - f[1::2]) / du)
        g = res.gradient[at, free]
        gmax = np.abs(g).max()
        own = np.abs(fd[0] - fd[1])
        jump = ~(own <= 1e-3 * gmax)  # also a difference that is not finite
        excluded += int(jump.sum())
        allowed = 10.0 * own + 1e-9 * gmax
        err = np.abs(g - fd[1])
        print(f"point {at}: f {res.misfits[at]:.4g}, |g|max {gmax:.4g}, excluded {np.flatnonzero(jump)}, "
              f"err / allowed {(err / allowed)[~jump]}, err / |g|max {(err / gmax)[~jump]}")
        worst = max(worst, float((err / allowed)[~jump].max()))
        assert (err[~jump] <= allowed[~jump]).all()
    print(f"worst ratio of the gradient's deviation to its allowance: {worst:.3g}; excluded {excluded}")
    assert excluded <= 1


# ------------------------------------------------------------------------------------------- the loop is its definition

WALK_ITER = 12


@pytest.fixture(scope="module")
def walk(device, curves):
    """Starts at truth +- 0.2 in u, far enough for rejected steps, and the same call again."""
    xs = around_truth(21, 6, 0.2)
    model = earth_model()
    return xs, model.refine(curves, xs, maxiter=WALK_ITER), model.refine(curves, xs, maxiter=WALK_ITER)


def test_history_accepted_and_lambda_follow_the_rule(walk):
    xs, res, _ = walk
    M = xs.shape[0]
    assert res.history.shape == (WALK_ITER + 1, M) and res.accepted.shape == (WALK_ITER, M)
    assert res.accepted.dtype == bool and res.lam.shape == (M,) and res.status.dtype == np.int32
    assert np.array_equal(res.history[0], res.start_misfits) and np.array_equal(res.history[-1], res.misfits)
    fell = res.history[1:] < res.history[:-1]
    assert np.array_equal(fell, res.accepted)
    assert np.array_equal(res.history[1:][~fell], res.history[:-1][~fell])
    lam = np.full(M, 1e-3)
    for take in res.accepted:
        lam = np.where(take, np.maximum(lam / 10.0, 1e-12), np.minimum(lam * 10.0, 1e12))
    assert np.array_equal(lam, res.lam)
    print(f"accepted {res.accepted.sum(axis=0)} of {WALK_ITER}; misfit {res.start_misfits} -> {res.misfits}")
    assert res.accepted.any() and not res.accepted.all()  # the case has both branches
    assert (res.misfits < res.start_misfits).any()


def test_refined_models_stay_in_bounds_and_keep_fixed_parameters(walk):
    xs, res, _ = walk
    lo, hi = earth_model().bounds()
    assert (res.xs >= lo).all() and (res.xs <= hi).all()
    fixed = lo == hi
    assert fixed.sum() == 3 and np.array_equal(res.xs[:, fixed], xs[:, fixed])
    assert (res.gradient[:, fixed] == 0).all() and (res.hessian[:, fixed] == 0).all()
    assert (res.hessian[:, :, fixed] == 0).all()
    never = ~res.accepted.any(axis=0)
    assert np.array_equal(res.xs[never], xs[never])


def test_misfits_are_the_normal_entry_on_the_models(device, curves, walk):
    """dvh_rayleigh_modes, dvh_rayleigh_sens and dvh_lm_normal by raw calls on ``models`` give ``misfits``,
    ``gradient`` and ``hessian`` bit for bit."""
    from das_diff_veh_amd import inversion as inv
    _, res, _ = walk
    model = earth_model()
    tab = inv.sample_table(curves, device)
    c_min = 0.8 * min(l.velocity_s[0] for l in model.layers)
    models = torch.from_numpy(res.models).to(device)
    dcdp, c = inv.rayleigh_sensitivity(models, tab.periods, tab.n_mode, dc=model.dc, c_min=c_min, need=tab.need,
                                       return_modes=True)
    f, g, H, status = inv.lm_normal(c, dcdp, model.chain(torch.from_numpy(res.xs).to(device)), tab)
    assert (status == 0).all()
    assert np.array_equal(f.cpu().numpy(), res.misfits)
    assert np.array_equal(g.cpu().numpy(), res.gradient) and np.array_equal(H.cpu().numpy(), res.hessian)


def test_same_call_same_bits(walk):
    _, a, b = walk
    for name in ("xs", "models", "misfits", "start_misfits", "history", "accepted", "lam", "status", "gradient",
                 "hessian"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


# ------------------------------------------------------------------------------------------------------------- recovery

RECOVERY_WIDTH = 0.01


def test_recovers_the_true_model(device, curves):
    """Eight starts at the true model +- 0.01 in every free u_k, noise-free curves, 20 iterations: every misfit ends at
    or below 1e-6.  (The data and the roots are each within 1e-9 relative of the truth and sigma is 1 %, so the minimum
    is at most about 2e-7; the factor 5 is for stopping on accepted steps only.)"""
    xs = around_truth(31, 8, RECOVERY_WIDTH)
    res = earth_model().refine(curves, xs, maxiter=20)
    lo, hi = earth_model().bounds()
    free = hi > lo
    off = np.abs((res.xs - TRUE_X)[:, free] / (hi - lo)[free]).max(axis=1)
    print(f"misfit {res.start_misfits} -> {res.misfits}; accepted {res.accepted.sum(axis=0)}; |u - u_true| {off}")
    assert (res.status == 0).all() and (res.misfits <= 1e-6).all()


# ---------------------------------------------------------------------------------------------- on the swarm's result

def test_refines_the_swarms_run_bests(device, curves):
    model = earth_model()
    inv_res = model.invert(curves, maxrun=2)
    best = inv_res.run_best()
    assert best.shape == (2, 8)
    per_run = inv_res.misfits.reshape(2, -1)
    assert np.array_equal(per_run.min(axis=1), inv_res.global_misfits[:, -1])
    for r in range(2):
        assert np.array_equal(best[r], inv_res.xs.reshape(2, -1, 8)[r, per_run[r].argmin()])
    res = model.refine(curves, best)
    print(f"swarm {inv_res.global_misfits[:, -1]}, refine start {res.start_misfits} -> {res.misfits}")
    assert (res.misfits <= res.start_misfits).all() and (res.misfits < res.start_misfits).any()


def test_a_start_without_its_mode_stays(device):
    from das_diff_veh_amd.inversion import Curve
    never = [Curve([0.4, 0.3], [0.3, 0.3], 10, "rayleigh", "phase")]
    xs = around_truth(41, 3, 0.2)
    res = earth_model().refine(never, xs, maxiter=3)
    assert np.array_equal(res.xs, xs) and ((res.status & 1) == 1).all()
    assert np.isposinf(res.misfits).all() and np.isposinf(res.history).all() and not res.accepted.any()
    assert (res.gradient == 0).all() and (res.hessian == 0).all()
    assert np.array_equal(res.lam, np.full(3, 1e-3 * 10.0 * 10.0 * 10.0))


# --------------------------------------------------------------------------- bounds whose lo + (hi - lo) rounds above hi

def rounding_model(args):
    """The three-layer problem with vs of the top layer in 0.03 .. 0.3, for which lo + 1.0 * (hi - lo) is one ulp above
    hi.  The true model lies inside."""
    from das_diff_veh_amd.inversion import EarthModel, Layer
    m = EarthModel()
    m.add(Layer([0.002, 0.01], [0.03, 0.3], [NU, NU]))
    m.add(Layer([0.005, 0.03], [0.2, 0.5], [NU, NU]))
    m.add(Layer([0.01, 0.01], [0.4, 0.8], [NU, NU]))
    return m.configure(optimizer="pso", misfit="rmse", density=density, optimizer_args=dict(args))


def test_models_on_a_rounded_bound_are_taken_and_stay_inside(device, curves):
    """Starts at u = 1 in the parameter whose upper bound rounds up (as invert forms it, one ulp above hi), a
    swarm's own models, and the refined models given back: all are taken, and every returned xs is inside the bounds."""
    model = rounding_model(dict(popsize=16, maxiter=12, seed=0))
    lo, hi = model.bounds()
    top = lo + 1.0 * (hi - lo)
    assert top[2] == np.nextafter(hi[2], np.inf)
    starts = np.repeat(TRUE_X[None], 3, axis=0)
    starts[0, 2] = top[2]
    starts[1, [0, 2]] = hi[0], top[2]
    first = model.refine(curves, starts, maxiter=0)
    assert (first.xs >= lo).all() and (first.xs <= hi).all() and np.array_equal(first.xs, np.minimum(starts, hi))
    res = model.refine(curves, starts, maxiter=8)
    print(f"from the rounded bound: {res.start_misfits} -> {res.misfits}, accepted {res.accepted.sum(axis=0)}")
    assert (res.xs >= lo).all() and (res.xs <= hi).all() and (res.misfits <= res.start_misfits).all()
    assert res.accepted[:, :2].any(axis=0).all()  # both left the bound they started on
    swarm = model.invert(curves, maxrun=2)
    over = (swarm.xs > hi).any(axis=1)
    print(f"{over.sum()} of {over.size} swarm models are an ulp above a bound")
    assert over.any()  # the case is real: the swarm returns such models
    rows = np.concatenate([swarm.run_best(), swarm.xs[over][:6]])
    again = model.refine(curves, rows, maxiter=4)
    assert (again.xs >= lo).all() and (again.xs <= hi).all()
    once_more = model.refine(curves, torch.from_numpy(again.xs).to(device), maxiter=1)
    assert (once_more.xs >= lo).all() and (once_more.xs <= hi).all()
