"""Laterally constrained refinement on the device: dvh_lm_solve_chain against the dense system in np.longdouble, its
host twin and dvh_lm_solve (the cases and checks of tests/test_refine_section_host.py), and EarthModel.refine_section on
the three-layer problem of tests/test_refine_sets_gpu.py: chains of one position against refine_sets bit for bit, the
descent of the chain objective, smoothing of noisy sets, and a gap carried by its neighbours."""
import math

import numpy as np
import pytest
import torch

from tests import section_ref as sec
from tests.test_refine_gpu import POISON, solve_dev
from tests.test_refine_section_host import (case_call, chain_host, check_bit_contract, check_containment, check_gap,
                                            check_identical_positions, check_residuals)
from tests.test_refine_section_host import lib  # noqa: F401  (the fixture)
from tests.test_refine_sets_gpu import FIELDS, MAXITER, MODEL_SET, START_WIDTH, TRUE_X, unit_of
from tests.test_refine_sets_gpu import problem  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def chain_dev(device, H, g, u, lam, free, mu, link, L):
    """One dvh_lm_solve_chain launch over poisoned outputs of a chain more than asked, through a workspace of exactly
    the size asked for (and a poisoned word behind it) -> NumPy (delta [M, D], status [C])."""
    from das_diff_veh_amd import _lib
    M, D = g.shape
    C = M // L
    link = np.ascontiguousarray(link, np.float64).reshape(C, L - 1)
    arrays = [np.array(a) for a in (H, g, u, lam, free, mu)] + [np.array(link) if link.size else np.zeros(1)]
    t = [torch.from_numpy(a).to(device) for a in arrays]
    words = _lib.load().dvh_lm_solve_chain_workspace(M, D) // 8
    work = torch.full((words + 1,), POISON, dtype=torch.float64, device=device)
    delta = torch.full((M + L, D), POISON, dtype=torch.float64, device=device)
    status = torch.full((C + 1,), -7, dtype=torch.int32, device=device)
    _lib.call("dvh_lm_solve_chain", *(_lib.ptr(a) for a in t), C, L, D, _lib.ptr(work), _lib.ptr(delta),
              _lib.ptr(status), _lib.stream_of(device))
    delta, status, last = delta.cpu().numpy(), status.cpu().numpy(), float(work[-1])
    assert (delta[M:] == POISON).all() and status[C] == -7 and last == POISON and not (delta[:M] == POISON).any()
    return delta[:M], status[:C]


# ------------------------------------------------------------------------------------------------------ the kernel

@pytest.mark.parametrize("L", sec.LENGTHS)
@pytest.mark.parametrize("D", sec.SIZES)
def test_chain_backward_error_and_the_host_twin(device, lib, D, L):
    """The host test's bound; and the chain of condition-1e2 blocks against the host twin within 1e2 x 1e-13, as
    tests/test_refine_gpu.py holds the dense solve (the device compile contracts a * b + c into one FMA)."""
    _, delta = check_residuals(lambda *a: chain_dev(device, *a), D, L)
    host, host_status = case_call(lambda *a: chain_host(lib, *a), sec.chain_case(D, L))
    assert (host_status == 0).all()
    apart = [np.abs(delta[c * L:(c + 1) * L] - host[c * L:(c + 1) * L]).max() / np.abs(host[c * L:(c + 1) * L]).max()
             for c in range(sec.N_CHAIN)]
    print("device against host, relative:", apart)
    assert apart[0] <= 1e2 * 1e-13


@pytest.mark.parametrize("D", sec.SIZES)
def test_chain_bit_contract_with_lm_solve(device, D):
    check_bit_contract(lambda *a: chain_dev(device, *a), lambda *a: solve_dev(device, *a), D)


@pytest.mark.parametrize("D,L", [(1, 3), (17, 7), (95, 3)])
def test_chain_identical_positions(device, D, L):
    check_identical_positions(lambda *a: chain_dev(device, *a), lambda *a: solve_dev(device, *a), D, L)


@pytest.mark.parametrize("D", [1, 17, 95])
def test_chain_gap(device, D):
    check_gap(lambda *a: chain_dev(device, *a), D)


@pytest.mark.parametrize("D,L", [(2, 2), (17, 7), (95, 3)])
def test_chain_failures_are_contained(device, D, L):
    check_containment(lambda *a: chain_dev(device, *a), D, L)


def test_lm_solve_chain_front(device):
    """The checked front: the raw launch's bits, and ValueError for shapes that are not chains."""
    from das_diff_veh_amd.inversion import lm_solve_chain
    case = sec.chain_case(17, 3)
    want, want_status = case_call(lambda *a: chain_dev(device, *a), case)
    put = lambda a: torch.from_numpy(np.array(a)).to(device)
    t = {k: put(case[k]) for k in ("H", "g", "u", "lam", "free", "mu", "link")}
    delta, status = lm_solve_chain(t["H"], t["g"], t["u"], t["lam"], t["free"], t["mu"], t["link"], 3)
    assert np.array_equal(delta.cpu().numpy(), want) and np.array_equal(status.cpu().numpy(), want_status)
    for bad in (dict(chain_len=2), dict(chain_len=0), dict(lam=t["lam"][:2]), dict(link=t["link"][:, :1]),
                dict(mu=t["mu"][:5]), dict(u=t["u"].cpu())):
        a = {**t, "chain_len": 3, **bad}
        with pytest.raises(ValueError):
            lm_solve_chain(a["H"], a["g"], a["u"], a["lam"], a["free"], a["mu"], a["link"], a["chain_len"])


# ------------------------------------------------------ refine_section on the three-layer model of the swarm replay

MORE_FIELDS = FIELDS + ("models", "start_misfits")
SECTION_FIELDS = MORE_FIELDS + ("objective", "penalty", "objective_history", "chain_status", "gap", "model_set")
VS_TOP = 2  # the column of the top layer's vs in xs (h0, h1, vs0, ..)


def same_fields(a, b, names):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), name


def test_chains_of_one_are_refine_sets(problem):
    """chain_len = 1: no coupling term exists, whatever ``coupling`` says, and every field is refine_sets' own."""
    p = problem
    want = p["model"].refine_sets(p["templates"], p["data_sets"], p["xs"], model_set=MODEL_SET, maxiter=MAXITER)
    got = p["model"].refine_section(p["templates"], p["data_sets"], p["xs"], chain_len=1, coupling=3.0,
                                    model_set=MODEL_SET, maxiter=MAXITER)
    assert want.accepted.any() and not want.accepted.all()
    same_fields(got, want, MORE_FIELDS)
    assert got.n_chain == 7 and got.chain_len == 1 and not got.gap.any() and (got.chain_status == 0).all()
    assert np.array_equal(got.objective, got.misfits) and (got.penalty == 0).all()
    assert np.array_equal(got.objective_history, got.history) and got.link_weights.shape == (7, 0)


def test_one_chain_without_coupling_descends(problem):
    """chain_len = 7, coupling = 0: the objective is the sum of the misfits (to the rounding of a sum of 7 terms in any
    order), it never rises, and falls strictly where the trial was taken."""
    p = problem
    res = p["model"].refine_section(p["templates"], p["data_sets"], p["xs"], coupling=0.0, model_set=MODEL_SET,
                                    maxiter=MAXITER)
    assert res.n_chain == 1 and res.chain_len == 7 and res.objective_history.shape == (MAXITER + 1, 1)
    h, taken = res.objective_history[:, 0], res.accepted[:, 0]
    print(f"objective {h}; accepted {taken}")
    assert (res.accepted == taken[:, None]).all() and (res.lam == res.lam[0]).all()
    assert (h[1:] <= h[:-1]).all() and (h[1:][taken] < h[:-1][taken]).all()
    assert np.array_equal(h[1:][~taken], h[:-1][~taken])
    assert taken.any() and res.objective[0] == h[-1]
    assert (res.penalty == 0).all() and not np.signbit(res.penalty).any()
    total = math.fsum(res.misfits)
    assert abs(res.objective[0] - total) <= 7 * 2.0 ** -53 * total
    for row in range(MAXITER + 1):
        total = math.fsum(res.history[row])
        assert abs(h[row] - total) <= 7 * 2.0 ** -53 * total


N_NOISY, SMOOTH_COUPLING = 8, 1000.0


@pytest.fixture(scope="module")
def noisy(problem):
    """Eight positions over one true model: seeded noisy sets of one percent (the templates carry the true curves) and
    seeded starts within START_WIDTH of the true model, refined apart and as one chain."""
    p = problem
    rng = np.random.default_rng(2024)
    data = [t.data + rng.normal(0.0, 0.01, (N_NOISY, t.period.size)) * t.data for t in p["templates"]]
    lo, hi = p["lo"], p["hi"]
    u = unit_of(TRUE_X, lo, hi)
    u = np.clip(u + rng.uniform(-START_WIDTH, START_WIDTH, (N_NOISY, lo.size)) * (hi > lo), 0.0, 1.0)
    xs = lo + u * (hi - lo)
    apart = p["model"].refine_sets(p["templates"], data, xs, maxiter=MAXITER)
    tied = p["model"].refine_section(p["templates"], data, xs, coupling=SMOOTH_COUPLING, maxiter=MAXITER)
    return dict(apart=apart, tied=tied, data=data, xs=xs)


def test_coupling_smooths_noisy_sets(noisy):
    """The spread over the positions of the refined top-layer vs is less than half of what refine_sets leaves on the
    same sets and starts; the objective never rises and the penalty is not negative."""
    apart, tied = noisy["apart"], noisy["tied"]
    spread = lambda res: float(np.std(res.xs[:, VS_TOP]))
    ratio = spread(tied) / spread(apart)
    print(f"spread of the top-layer vs: {spread(apart):.3e} apart, {spread(tied):.3e} tied, ratio {ratio:.3f}; "
          f"objective {tied.objective_history[:, 0]}, penalty {tied.penalty}; accepted {tied.accepted[:, 0]}")
    assert (apart.status == 0).all() and (tied.status == 0).all() and tied.accepted.any()
    assert ratio < 0.5
    h = tied.objective_history[:, 0]
    assert (h[1:] <= h[:-1]).all() and (tied.penalty >= 0).all() and np.isfinite(h).all()
    assert abs(tied.objective[0] - (math.fsum(tied.misfits) + tied.penalty[0])) <= 9 * 2.0 ** -53 * tied.objective[0]


GAP_COUPLING = 10.0


@pytest.fixture(scope="module")
def sloped(problem):
    """Five positions whose true top-layer vs rises linearly along the chain, noise-free curves of each, the middle set
    all NaN; every start at the true model of the middle but the gap's own, which starts elsewhere.  A second chain
    of five sets of NaN only.  Each call made twice."""
    from das_diff_veh_amd.inversion import phase_velocity
    from tests.test_inversion_replay_gpu import TRUE_H, TRUE_NU, TRUE_VS, density
    p = problem
    lo, hi = p["lo"], p["hi"]
    tops = TRUE_VS[0] + np.linspace(-0.01, 0.01, 5)
    nu = np.array(TRUE_NU)
    data = [np.empty((10, t.period.size)) for t in p["templates"]]
    for k, top in enumerate(tops):
        vs = np.array([top] + TRUE_VS[1:])
        vp = vs * np.sqrt((2 - 2 * nu) / (1 - 2 * nu))
        for t, d in zip(p["templates"], data):
            d[k] = phase_velocity(t.period, np.array(TRUE_H + [0.0]), vp, vs, density(vp), mode=t.mode)
            assert np.isfinite(d[k]).all()
    for d in data:
        d[2] = np.nan
        d[5:] = np.nan
    u = np.tile(unit_of(TRUE_X, lo, hi), (10, 1))
    u[2] = np.clip(u[2] + 0.07 * (hi > lo), 0.0, 1.0)
    xs = lo + u * (hi - lo)
    run = lambda **kw: p["model"].refine_section(p["templates"], data, xs, chain_len=5, coupling=GAP_COUPLING, **kw)
    return dict(res=run(maxiter=MAXITER), again=run(maxiter=MAXITER), run=run, data=data, xs=xs, tops=tops)


def test_a_gap_is_carried_by_its_neighbours(problem, sloped):
    p, res = problem, sloped["res"]
    lo, hi = p["lo"], p["hi"]
    assert res.n_chain == 2 and res.gap.tolist() == [False, False, True, False, False] + [True] * 5
    assert res.chain_status[0] == 0 and (res.status[[0, 1, 3, 4]] == 0).all()  # the chain is alive
    assert res.status[2] == 4 and np.isnan(res.misfits[2]) and np.isnan(res.history[:, 2]).all()
    assert np.isfinite(res.misfits[[0, 1, 3, 4]]).all() and (res.gradient[2] == 0).all() and (res.hessian[2] == 0).all()
    taken = res.accepted[:, 0]
    print(f"objective {res.objective_history[:, 0]}, accepted {taken}, vs top {res.xs[:5, VS_TOP]} of {sloped['tops']}")
    assert taken.any() and (res.accepted[:, :5] == taken[:, None]).all()
    # after the first accepted iteration the gap's u is the mean of its neighbours' (the links are 1), where no
    # coordinate of the three was clamped
    first = sloped["run"](maxiter=int(np.argmax(taken)) + 1)
    assert first.accepted[-1, 0] and first.accepted[:, 0].sum() == 1
    u = unit_of(first.xs[:5], lo, hi)
    free = hi > lo
    inside = ((u[1:4] > 0) & (u[1:4] < 1)).all(axis=0) & free
    off = np.abs(u[2] - 0.5 * (u[1] + u[3]))
    print(f"first accepted iteration: {inside.sum()} of {free.sum()} free coordinates unclamped, off the mean {off}")
    assert inside[VS_TOP] and (off[inside] <= 1e-12).all()
    u0 = unit_of(sloped["xs"][:5], lo, hi)
    assert (np.abs(u0[2] - 0.5 * (u0[1] + u0[3]))[inside] > 0.05).all()  # it did not start there
    # at the end its vs lies between its neighbours'
    top = res.xs[:5, VS_TOP]
    assert min(top[1], top[3]) <= top[2] <= max(top[1], top[3]) and top[1] != top[3]
    # refine_sets on the same input leaves the start where it is: the gap this closes
    apart = p["model"].refine_sets(p["templates"], sloped["data"], sloped["xs"], maxiter=MAXITER)
    assert apart.status[2] & 1 and np.array_equal(apart.xs[2], sloped["xs"][2]) and apart.misfits[2] == np.inf


def test_a_chain_without_data_stays_and_repeats_are_bit_equal(sloped, noisy, problem):
    res = sloped["res"]
    assert res.chain_status[1] & 1 and (res.status[5:] & 1 == 1).all() and (res.status[5:] & 4 == 0).all()
    assert np.array_equal(res.xs[5:], sloped["xs"][5:]) and not res.accepted[:, 5:].any()
    assert (res.misfits[5:] == np.inf).all() and (res.history[:, 5:] == np.inf).all()
    assert res.objective_history[0, 1] == res.objective[1]
    same_fields(res, sloped["again"], SECTION_FIELDS)
    p = problem
    again = p["model"].refine_section(p["templates"], noisy["data"], noisy["xs"], coupling=SMOOTH_COUPLING,
                                      maxiter=MAXITER)
    same_fields(noisy["tied"], again, SECTION_FIELDS)


def test_section_is_profiles_reshaped(noisy, sloped):
    depths = np.linspace(0.0, 0.03, 7)
    for res, shape in ((noisy["tied"], (1, 8, 7)), (sloped["res"], (2, 5, 7))):
        got = res.section(depths)
        assert got.shape == shape and np.array_equal(got.reshape(-1, 7), res.profiles(depths))
        assert np.array_equal(res.section(depths, "thickness").reshape(-1, 7), res.profiles(depths, "thickness"))
