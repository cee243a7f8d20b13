"""The chain solve without a GPU: dvh_lm_solve_chain_host (csrc/refine.h, the header the device kernel compiles, run on
the CPU) against the dense block-tridiagonal system in np.longdouble within the derived bound of tests/section_ref.py,
its bit contract with dvh_lm_solve_host, gaps, contained failures and refusals; then the host half of
EarthModel.refine_section: the coupling terms and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from tests import section_ref as sec
from tests.test_refine_host import POISON, solve_host
from tests.test_refine_host import lib  # noqa: F401  (the fixture)


def chain_host(lib, H, g, u, lam, free, mu, link, L):
    """One dvh_lm_solve_chain_host call into poisoned buffers of a chain more than asked -> (delta [M, D],
    status [C])."""
    M, D = g.shape
    C = M // L
    link = np.ascontiguousarray(link, np.float64).reshape(C, L - 1)
    arrays = [np.ascontiguousarray(a) for a in (H, g, u, lam, free, mu)] + [link if link.size else np.zeros(1)]
    assert arrays[0].shape == (M, D, D) and arrays[2].shape == (M, D) and arrays[3].shape == (C,)
    nbytes = lib.dvh_lm_solve_chain_workspace(M, D)
    assert nbytes == M * D * (D + 1) * 8
    work = np.full(nbytes // 8 + 1, POISON)
    delta, status = np.full((M + L, D), POISON), np.full(C + 1, -7, np.int32)
    rc = lib.dvh_lm_solve_chain_host(*(a.ctypes.data for a in arrays), C, L, D, work.ctypes.data, delta.ctypes.data,
                                     status.ctypes.data)
    assert rc == 0, lib.dvh_last_error()
    assert (delta[M:] == POISON).all() and status[C] == -7 and work[-1] == POISON and not (delta[:M] == POISON).any()
    return delta[:M], status[:C]


def case_call(solve, case, **changed):
    a = {**case, **changed}
    return solve(a["H"], a["g"], a["u"], a["lam"], a["free"], a["mu"], a["link"], case["L"])


# ------------------------------------------------------------------ checks shared with tests/test_refine_section_gpu.py

def check_residuals(solve, D, L):
    case = sec.chain_case(D, L)
    delta, status = case_call(solve, case)
    return sec.assert_chains(delta, status, case), delta


def check_bit_contract(solve, solve_one, D):
    """chain_len = 1 with the case's mu, and chain_len = 7 with mu = 0 and with every link 0: dvh_lm_solve's step with
    the chain's lambda at each row, bit for bit."""
    one = sec.chain_case(D, 1)
    delta, status = case_call(solve, one)
    want, want_status = solve_one(one["H"], one["g"], one["lam"], one["free"])
    assert np.array_equal(delta, want) and np.array_equal(status, want_status) and (status == 0).all()
    seven = sec.chain_case(D, 7)
    want, want_status = solve_one(seven["H"], seven["g"], np.repeat(seven["lam"], 7), seven["free"])
    assert (want_status == 0).all()
    for name, changed in (("mu = 0", dict(mu=np.zeros(D))), ("link = 0", dict(link=np.zeros((3, 6))))):
        delta, status = case_call(solve, seven, **changed)
        assert np.array_equal(delta, want) and (status == 0).all(), name
    coupled, _ = case_call(solve, seven)
    assert not np.array_equal(coupled, want)  # the case's own mu and links do couple


def check_identical_positions(solve, solve_one, D, L):
    """The same H, g, u at every position: the coupling cancels, every position's step is dvh_lm_solve's.  Both solve
    the chain's system within its bound, so they differ by at most 2 cond(A) bound ||delta||."""
    case = sec.chain_case(D, L)
    first = lambda a: np.ascontiguousarray(np.broadcast_to(a[:1], a.shape))
    same = dict(H=first(case["H"]), g=first(case["g"]), u=first(case["u"]), lam=np.full(3, case["lam"][0]))
    delta, status = case_call(solve, case, **same)
    assert (status == 0).all()
    alone, _ = solve_one(same["H"][:1], same["g"][:1], same["lam"][:1], case["free"])
    for c in range(sec.N_CHAIN):
        system = sec.dense_system(*sec.chain_of(case, c, **same))
        rows = delta[c * L:(c + 1) * L]
        res, bound = sec.residual_of(rows, system)
        res_alone, _ = sec.residual_of(np.tile(alone, (L, 1)), system)
        cond = np.linalg.cond(system[0].astype(np.float64))
        off = np.linalg.norm(rows - alone) / np.linalg.norm(rows)
        print(f"D {D} L {L} chain {c}: residuals {res:.2e}, {res_alone:.2e} of {bound:.2e}; apart {off:.2e}, "
              f"cond {cond:.2e}")
        assert res <= bound and res_alone <= bound and off <= 2.0 * cond * bound


def gap_case(D, L=5):
    """The well-conditioned chain with its middle position emptied (H = 0, g = 0) and every free parameter coupled."""
    case = sec.chain_case(D, L)
    H, g = case["H"][:L].copy(), case["g"][:L].copy()
    H[L // 2], g[L // 2] = 0.0, 0.0
    return dict(H=H, g=g, u=case["u"][:L], lam=case["lam"][:1], free=case["free"], mu=np.linspace(0.1, 0.5, D),
                link=case["link"][:1], L=L, D=D)


def check_gap(solve, D):
    """The gap's rows of the system say that its u + delta is the w-weighted mean of its neighbours': held to 1e-12
    per free parameter.  A chain of gaps only has nothing to solve: status 2, zeros."""
    case = gap_case(D)
    delta, status = case_call(solve, case)
    assert status[0] == 0
    at, k = np.flatnonzero(case["free"]), case["L"] // 2
    new = (case["u"] + delta)[:, at]
    w = case["link"][0]
    mean = (w[k - 1] * new[k - 1] + w[k] * new[k + 1]) / (w[k - 1] + w[k])
    print(f"D {D}: the gap is off its neighbours' mean by {np.abs(new[k] - mean).max():.2e}")
    assert (np.abs(new[k] - mean) <= 1e-12).all()
    res, bound = sec.residual_of(delta, sec.dense_system(case["H"], case["g"], case["u"], case["lam"][0], case["free"],
                                                          case["mu"], w))
    assert res <= bound
    delta, status = case_call(solve, case, H=np.zeros_like(case["H"]), g=np.zeros_like(case["g"]))
    assert status[0] == 2 and (delta == 0).all()


def check_containment(solve, D, L):
    """An indefinite block, or a NaN in H, at one position of the middle chain: status 2 and zeros for that chain, the
    others bit-unchanged; and every chain alone equals itself in the batch, at either end of it."""
    case = sec.chain_case(D, L)
    clean, clean_status = case_call(solve, case)
    assert (clean_status == 0).all()
    k0 = int(np.flatnonzero(case["free"])[0])
    for name, value in (("indefinite", -10.0), ("nan", np.nan)):
        for k in sorted({0, L // 2, L - 1}):
            H = case["H"].copy()
            H[L + k, k0, k0] = value
            delta, status = case_call(solve, case, H=H)
            assert status.tolist() == [0, 2, 0], (name, k, status)
            assert (delta[L:2 * L] == 0).all() and not np.signbit(delta[L:2 * L]).any()
            assert np.array_equal(delta[:L], clean[:L]) and np.array_equal(delta[2 * L:], clean[2 * L:]), (name, k)
    for c in range(sec.N_CHAIN):
        rows = slice(c * L, (c + 1) * L)
        alone, st = solve(case["H"][rows], case["g"][rows], case["u"][rows], case["lam"][c:c + 1], case["free"],
                          case["mu"], case["link"][c:c + 1], L)
        assert np.array_equal(alone, clean[rows]) and st[0] == 0, c
    order = [2, 1, 0]
    pick = np.concatenate([np.arange(c * L, (c + 1) * L) for c in order])
    back, _ = solve(case["H"][pick], case["g"][pick], case["u"][pick], case["lam"][order], case["free"], case["mu"],
                    case["link"][order], L)
    assert np.array_equal(back, clean[pick])


# ------------------------------------------------------------------------------------------------------- the host entry

@pytest.mark.parametrize("L", sec.LENGTHS)
@pytest.mark.parametrize("D", sec.SIZES)
def test_chain_host_backward_error(lib, D, L):
    check_residuals(lambda *a: chain_host(lib, *a), D, L)


@pytest.mark.parametrize("D", sec.SIZES)
def test_chain_host_bit_contract(lib, D):
    check_bit_contract(lambda *a: chain_host(lib, *a), lambda *a: solve_host(lib, *a), D)


@pytest.mark.parametrize("D,L", [(1, 3), (17, 7), (95, 3)])
def test_chain_host_identical_positions(lib, D, L):
    check_identical_positions(lambda *a: chain_host(lib, *a), lambda *a: solve_host(lib, *a), D, L)


@pytest.mark.parametrize("D", [1, 17, 95])
def test_chain_host_gap(lib, D):
    check_gap(lambda *a: chain_host(lib, *a), D)


@pytest.mark.parametrize("D,L", [(2, 2), (17, 7), (95, 3)])
def test_chain_host_failures_are_contained(lib, D, L):
    check_containment(lambda *a: chain_host(lib, *a), D, L)


def test_chain_host_without_a_free_parameter(lib):
    case = sec.chain_case(2, 3)
    delta, status = case_call(lambda *a: chain_host(lib, *a), case, free=np.zeros(2, np.int32))
    assert (status == 2).all() and (delta == 0).all()


def test_chain_refusals_come_before_any_launch(lib):
    """-2 and -4 of both entries; the device entry returns them (and 0 for n_chain = 0) before a device is touched."""
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused or empty
    ok = (p, p, p, p, p, p, p, 2, 3, 8, p, p, p)
    for name, tail in (("dvh_lm_solve_chain", (None,)), ("dvh_lm_solve_chain_host", ())):
        f = lambda *a: getattr(lib, name)(*a, *tail)
        for at in (0, 1, 2, 3, 4, 5, 6, 10, 11, 12):
            assert f(*ok[:at], None, *ok[at + 1:]) == -2, (name, at)
        for at, bad in ((7, -1), (8, 0), (8, -3), (9, 0), (9, -1)):
            assert f(*ok[:at], bad, *ok[at + 1:]) == -2, (name, at, bad)
        assert f(*ok[:9], 97, *ok[10:]) == -4 and b"96 parameters" in lib.dvh_last_error()
        assert f(None, None, None, None, None, None, None, 0, 3, 8, None, None, None) == 0
    assert lib.dvh_lm_solve_chain_workspace(7, 96) == 7 * 2 * 4656 * 8
    assert lib.dvh_lm_solve_chain_workspace(-1, 8) == 0 and lib.dvh_lm_solve_chain_workspace(1, 97) == 0


# ------------------------------------------------------------------------------------------------ Python on the host

@pytest.mark.parametrize("C,L,D", [(1, 1, 3), (2, 2, 1), (3, 7, 17)])
def test_coupling_terms_against_longdouble(C, L, D):
    """P and q of the loop's torch ops within (L + 4) 2^-52 of the same expressions on absolute values (three products
    and the sum over the links and parameters for P; a product chain and two terms for q)."""
    from das_diff_veh_amd.inversion import coupling_terms
    rng = np.random.default_rng(100 * C + 10 * L + D)
    u, mu, link = rng.uniform(0.0, 1.0, (C, L, D)), rng.uniform(0.0, 3.0, D), rng.uniform(0.0, 4.0, (C, L - 1))
    mu[0] = 0.0
    P, q = coupling_terms(torch.from_numpy(u), torch.from_numpy(mu), torch.from_numpy(link))
    want_P, want_q = sec.coupling_terms(u, mu, link)
    assert P.shape == (C,) and q.shape == (C, L, D) and P.dtype == q.dtype == torch.float64
    du = np.abs(np.diff(u, axis=1))
    q_abs = np.zeros_like(u)
    q_abs[:, 1:] += mu * link[:, :, None] * du
    q_abs[:, :-1] += mu * link[:, :, None] * du
    assert (np.abs(P.numpy() - want_P) <= (L * D + 4) * 2.0 ** -52 * want_P).all()
    assert (np.abs(q.numpy() - want_q) <= 6 * 2.0 ** -52 * q_abs).all()
    if L == 1:
        assert (P == 0).all() and (q == 0).all()
    assert (q.numpy()[:, :, 0] == 0).all() and np.abs(want_q.sum(axis=1)).max() <= 1e-15 * max(q_abs.max(), 1.0)


def section_model():
    from tests.test_refine_host import chain_model
    return chain_model(lambda vp: 1.56 + 0.186 * vp)


def test_refine_section_refuses_bad_input():
    """Every ValueError comes before any device work: there is no device here."""
    from das_diff_veh_amd.inversion import Curve
    model = section_model()
    curve = Curve([0.1, 0.2], [0.3, 0.3], 0, "rayleigh", "phase")
    lo, hi = model.bounds()
    xs = np.tile(0.5 * (lo + hi), (6, 1))
    good = dict(curves=[curve], data_sets=[np.full((6, 2), 0.3)], xs=xs, chain_len=3)
    for bad in (dict(chain_len=4), dict(chain_len=0), dict(chain_len=-3), dict(coupling=-1.0),
                dict(coupling=float("nan")), dict(coupling=float("inf")), dict(coupling=np.ones(7)),
                dict(coupling=np.ones((2, 8))), dict(coupling=np.r_[np.ones(7), -1e-300]),
                dict(link_weights=np.ones(3)), dict(link_weights=np.ones((3, 2))), dict(link_weights=np.ones((2, 3))),
                dict(link_weights=[1.0, -1.0]), dict(link_weights=[1.0, np.nan]), dict(link_weights=[np.inf, 1.0]),
                dict(xs=xs[:5], chain_len=None, data_sets=[np.full((6, 2), 0.3)]), dict(model_set=np.arange(6) + 1),
                dict(maxiter=-1), dict(lam0=0.0), dict(data_sets=[np.full((6, 3), 0.3)]), dict(xs=xs + 1.0)):
        with pytest.raises(ValueError):
            model.refine_section(**{**good, **bad})
    with pytest.raises(TypeError):
        model.refine_section(**{**good, "curves": ["curve"]})


def test_checked_chains_broadcasts():
    from das_diff_veh_amd.inversion import _checked_chains
    C, L, mu, w = _checked_chains(12, 8, 4, 2.0, [1.0, 0.0, 4.0])
    assert (C, L) == (3, 4) and np.array_equal(mu, np.full(8, 2.0))
    assert np.array_equal(w, np.tile([1.0, 0.0, 4.0], (3, 1)))
    C, L, mu, w = _checked_chains(12, 8, None, np.arange(8.0), None)
    assert (C, L) == (1, 12) and np.array_equal(mu, np.arange(8.0)) and np.array_equal(w, np.ones((1, 11)))
    C, L, mu, w = _checked_chains(5, 8, 1, 0.0, None)
    assert (C, L) == (5, 1) and w.shape == (5, 0)


def test_section_is_profiles_reshaped():
    from das_diff_veh_amd.inversion import SectionResult
    rng = np.random.default_rng(4)
    models = rng.uniform(0.1, 1.0, (6, 3, 4))
    empty = np.zeros(0)
    res = SectionResult(empty, models, *([empty] * 8), n_chain=2, chain_len=3)
    depths = np.linspace(0.0, 3.0, 11)
    for name in ("velocity_s", "thickness"):
        got = res.section(depths, name)
        assert got.shape == (2, 3, 11) and np.array_equal(got.reshape(6, 11), res.profiles(depths, name))
