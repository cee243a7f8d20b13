"""The Gauss-Newton refinement without a GPU: dvh_lm_normal_host and dvh_lm_solve_host (csrc/refine.h, the header the
device kernels compile, run on the CPU) against np.longdouble references within derived rounding bounds
(tests/refine_ref.py), their flagged models and refusals, and EarthModel.chain on CPU tensors against its closed
forms."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import refine_ref as ref

POISON = -777.25


@pytest.fixture(scope="module")
def lib():
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    return _lib.load()


def normal_host(lib, c, dcdp, chain, tab, n_period=ref.N_PERIOD, n_mode=ref.N_MODE, rho_floor=ref.RHO_FLOOR):
    """One dvh_lm_normal_host call into poisoned buffers of a model more than asked -> (f, g, H, status)."""
    M, (K, D) = c.shape[0], chain.shape[1:]
    arrays = [np.ascontiguousarray(a) for a in (c, dcdp, chain, *(tab[k] for k in ref.TABLE_KEYS), tab["curve_weight"])]
    f, g, H = (np.full(s, POISON) for s in ((M + 1,), (M + 1, D), (M + 1, D, D)))
    status = np.full(M + 1, -7, np.int32)
    p = [a.ctypes.data for a in arrays]
    rc = lib.dvh_lm_normal_host(p[0], p[1], p[2], M, n_period, n_mode, K // 4, D, *p[3:8], tab["sample_obs"].size, p[8],
                                tab["curve_weight"].size, rho_floor, f.ctypes.data, g.ctypes.data, H.ctypes.data,
                                status.ctypes.data)
    assert rc == 0, lib.dvh_last_error()
    assert f[M] == POISON and (g[M] == POISON).all() and (H[M] == POISON).all() and status[M] == -7
    assert not (g[:M] == POISON).any() and not (H[:M] == POISON).any() and not (status[:M] == -7).any()
    return f[:M], g[:M], H[:M], status[:M]


def solve_host(lib, H, g, lam, free):
    M, D = g.shape
    arrays = [np.ascontiguousarray(a) for a in (H, g, lam, free)]
    delta, status = np.full((M + 1, D), POISON), np.full(M + 1, -7, np.int32)
    rc = lib.dvh_lm_solve_host(*(a.ctypes.data for a in arrays), M, D, delta.ctypes.data, status.ctypes.data)
    assert rc == 0, lib.dvh_last_error()
    assert (delta[M] == POISON).all() and status[M] == -7 and not (delta[:M] == POISON).any()
    return delta[:M], status[:M]


def case_arrays(n_layer, D, S):
    """A writable copy of the shared case."""
    case = ref.normal_case(n_layer, D, S)
    return case["c"].copy(), case["dcdp"].copy(), case["chain"].copy(), {k: v.copy() for k, v in case["tab"].items()}


@pytest.mark.parametrize("S", sorted(ref.CURVE_SIZES))
@pytest.mark.parametrize("n_layer,D", ref.SHAPES)
def test_normal_host_against_longdouble(lib, n_layer, D, S):
    """g and H within 4 (K + S + 4) 2^-52 of their absolute-value expressions, f within 1e-13 relative of
    dvh_curve_misfit's formula, with NaN in every slot that no sample names."""
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    ref.assert_normal(normal_host(lib, c, dcdp, chain, tab), n_layer, D, S)


def flag_cases(n_layer, D, S):
    """(name, c, dcdp, chain, tab, n_curve_model): the shared case with model 1 spoiled, or the table spoiled for every
    model (then the flag is every model's)."""
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    p, m = tab["sample_period"][3], tab["sample_mode"][3]
    bad_c = c.copy()
    bad_c[1, p, m] = np.nan
    yield "nan root", bad_c, dcdp, chain, tab, [1]
    bad_d = dcdp.copy()
    bad_d[1, p, m, n_layer - 1, 2] = np.inf
    yield "inf dcdp", c, bad_d, chain, tab, [1]
    for key, bad in (("sample_period", ref.N_PERIOD), ("sample_period", -1), ("sample_mode", ref.N_MODE),
                     ("sample_mode", -1), ("sample_curve", 3), ("sample_curve", -1)):
        t = {k: v.copy() for k, v in tab.items()}
        t[key][5] = bad
        yield f"{key} {bad}", c, dcdp, chain, t, [0, 1, 2]
    t = {k: v.copy() for k, v in tab.items()}
    t["curve_weight"] = np.r_[t["curve_weight"], 1.0]
    yield "a curve without a sample", c, dcdp, chain, t, [0, 1, 2]


def check_flagged(launch, n_layer, D, S):
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    clean = launch(c, dcdp, chain, tab)
    assert (clean[3] == 0).all()
    for name, c2, d2, ch2, t2, flagged in flag_cases(n_layer, D, S):
        f, g, H, status = launch(c2, d2, ch2, t2)
        for m in range(ref.N_MODEL):
            if m in flagged:
                assert status[m] == 1 and f[m] == np.inf and (g[m] == 0).all() and (H[m] == 0).all(), (name, m)
            else:  # the neighbours keep their bits
                assert status[m] == 0 and all(np.array_equal(a[m], b[m]) for a, b in zip((f, g, H), clean)), (name, m)


def check_position_independence(launch, n_layer, D, S):
    c, dcdp, chain, tab = case_arrays(n_layer, D, S)
    batch = launch(c, dcdp, chain, tab)
    for m in range(ref.N_MODEL):
        alone = launch(c[m:m + 1], dcdp[m:m + 1], chain[m:m + 1], tab)
        assert all(np.array_equal(a[0], b[m]) for a, b in zip(alone, batch)), m
    back = launch(c[::-1], dcdp[::-1], chain[::-1], tab)
    assert all(np.array_equal(a[::-1], b) for a, b in zip(back, batch))


def test_normal_host_flags_one_model(lib):
    check_flagged(lambda *a: normal_host(lib, *a), 3, 8, 13)


@pytest.mark.parametrize("n_layer,D,S", [(3, 8, 13), (32, 95, 257)])
def test_normal_host_position_independence(lib, n_layer, D, S):
    check_position_independence(lambda *a: normal_host(lib, *a), n_layer, D, S)


def test_rho_floor_bounds_the_factor_at_a_perfect_fit(lib):
    """Residuals of exactly 0: f = 0, g = 0 and H = sum_i w_i / (W n_i rho_floor) sum_s j_s j_s^T, finite."""
    c, dcdp, chain, tab = case_arrays(3, 8, 13)
    tab["sample_obs"] = c[0, tab["sample_period"], tab["sample_mode"]].copy()
    f, g, H, status = normal_host(lib, c[:1], dcdp[:1], chain[:1], tab, rho_floor=0.5)
    assert status[0] == 0 and f[0] == 0 and (g == 0).all() and np.isfinite(H).all() and (np.diagonal(H[0]) > 0).all()
    f2, g2, H2, _ = normal_host(lib, c[:1], dcdp[:1], chain[:1], tab, rho_floor=0.25)
    assert np.array_equal(H2, 2.0 * H)


@pytest.mark.parametrize("D", ref.SOLVE_SIZES)
def test_solve_host_backward_error(lib, D):
    case = ref.solve_case(D)
    delta, status = solve_host(lib, case["H"], case["g"], case["lam"], case["free"])
    ref.assert_solve(delta, status, D)
    for m in range(4):  # the refusing model leaves the others alone: each equals itself solved alone
        one, st = solve_host(lib, case["H"][m:m + 1], case["g"][m:m + 1], case["lam"][m:m + 1], case["free"])
        assert np.array_equal(one[0], delta[m]) and st[0] == status[m]


def test_solve_host_special_matrices(lib):
    """All H_kk = 0, no free parameter, a NaN in H and an infinite lambda each give status 2 and a zero step; the
    identity with lambda = 0 returns -g exactly."""
    D = 5
    eye, g = np.eye(D), np.arange(1.0, D + 1)
    free = np.ones(D, np.int32)
    nan = eye.copy()
    nan[2, 1] = np.nan
    H = np.stack([np.zeros((D, D)), nan, eye, eye])
    delta, status = solve_host(lib, H, np.tile(g, (4, 1)), np.array([1e-3, 1e-3, np.inf, 0.0]), free)
    assert status.tolist() == [2, 2, 2, 0] and (delta[:3] == 0).all() and np.array_equal(delta[3], -g)
    delta, status = solve_host(lib, H[3:], g[None], np.array([0.0]), np.zeros(D, np.int32))
    assert status[0] == 2 and (delta == 0).all()


def test_refusals_come_before_any_launch(lib):
    """-2 and -4 of the four entries; the device entries return them (and 0 for n_model = 0) before a device is
    touched."""
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused or empty
    ok = (p, p, p, 2, 5, 4, 3, 8, p, p, p, p, p, 7, p, 2, 1e-12, p, p, p, p)
    for name, tail in (("dvh_lm_normal", (None,)), ("dvh_lm_normal_host", ())):
        f = lambda *a: getattr(lib, name)(*a, *tail)
        for at in (0, 1, 2, 8, 9, 10, 11, 12, 14, 17, 18, 19, 20):
            assert f(*ok[:at], None, *ok[at + 1:]) == -2, (name, at)
        for at, bad in ((3, -1), (4, 0), (5, 0), (6, 0), (7, 0), (13, 0), (15, 0), (16, 0.0), (16, float("nan"))):
            assert f(*ok[:at], bad, *ok[at + 1:]) == -2, (name, at, bad)
        for at, bad, word in ((7, 97, b"96 parameters"), (6, 33, b"32 layers"), (5, 17, b"16 modes"),
                              (15, 65, b"64 curves")):
            assert f(*ok[:at], bad, *ok[at + 1:]) == -4 and word in lib.dvh_last_error(), (name, at)
        assert f(None, None, None, 0, 5, 4, 3, 8, None, None, None, None, None, 7, None, 2, 1e-12, None, None, None,
                 None) == 0
    ok = (p, p, p, p, 2, 8, p, p)
    for name, tail in (("dvh_lm_solve", (None,)), ("dvh_lm_solve_host", ())):
        f = lambda *a: getattr(lib, name)(*a, *tail)
        for at in (0, 1, 2, 3, 6, 7):
            assert f(*ok[:at], None, *ok[at + 1:]) == -2, (name, at)
        assert f(*ok[:4], -1, *ok[5:]) == -2 and f(*ok[:5], 0, *ok[6:]) == -2
        assert f(*ok[:5], 97, *ok[6:]) == -4 and b"96 parameters" in lib.dvh_last_error()
        assert f(None, None, None, None, 0, 8, None, None) == 0


# ------------------------------------------------------------------------------------------------- EarthModel.chain

NU_BOUNDS = [(0.2, 0.4), (0.4375, 0.4375), (0.3, 0.45)]


def chain_model(density):
    from das_diff_veh_amd.inversion import EarthModel, Layer
    m = EarthModel()
    m.add(Layer([0.002, 0.01], [0.1, 0.3], NU_BOUNDS[0]))
    m.add(Layer([0.005, 0.03], [0.2, 0.2], NU_BOUNDS[1]))  # vs and nu fixed
    m.add(Layer([0.01, 0.01], [0.4, 0.8], NU_BOUNDS[2]))
    return m.configure(density=density)


@pytest.mark.parametrize("name,density,slope", [
    ("linear", lambda vp: 1.56 + 0.186 * vp, lambda vp: 0.186 + 0.0 * vp),
    ("quadratic", lambda vp: 1.2 + 0.3 * vp - 0.02 * vp * vp, lambda vp: 0.3 - 0.04 * vp),
    ("constant tensor", lambda vp: 0.0 * vp + 2.0, lambda vp: 0.0 * vp),
    ("constant float", lambda vp: 2.0, lambda vp: 0.0 * vp)])
def test_chain_closed_forms(name, density, slope):
    """Every entry of chain() to 1e-14 relative of the closed form evaluated in np.longdouble; zero columns for the
    fixed parameters, a zero row for the half-space's h, zero rho rows for a constant density."""
    model = chain_model(density)
    lo, hi = model.bounds()
    n, D, LD = 3, 8, np.longdouble
    rng = np.random.default_rng(5)
    x = lo + rng.uniform(size=(4, D)) * (hi - lo)
    got = model.chain(torch.from_numpy(x)).numpy()
    assert got.shape == (4, 4 * n, D) and got.dtype == np.float64
    span = (hi - lo).astype(LD)
    want = np.zeros((4, n, 4, D), LD)
    vs, nu = x[:, n - 1:2 * n - 1].astype(LD), x[:, 2 * n - 1:].astype(LD)
    g = np.sqrt((2 - 2 * nu) / (1 - 2 * nu))
    dvp = {n - 1: g * span[n - 1:2 * n - 1], 2 * n - 1: vs / (g * (1 - 2 * nu) ** 2) * span[2 * n - 1:]}
    for l in range(n):
        if l < n - 1:
            want[:, l, 0, l] = span[l]
        want[:, l, 2, n - 1 + l] = span[n - 1 + l]
        for first, d in dvp.items():
            want[:, l, 1, first + l] = d[:, l]
            want[:, l, 3, first + l] = slope(vs * g)[:, l] * d[:, l]
    want = want.reshape(4, 4 * n, D)
    assert (np.abs(got - want) <= 1e-14 * np.abs(want)).all(), np.abs(got / want - 1)[want != 0].max()
    assert ((want != 0).sum(axis=(0, 1)) > 0).tolist() == (hi > lo).tolist()  # the case has every kind of column
    fixed = hi == lo
    assert fixed.sum() == 2 and (got[:, :, fixed] == 0).all()
    assert (got[:, 4 * (n - 1)] == 0).all()
    if name.startswith("constant"):
        assert (got[:, 3::4] == 0).all()
    else:
        assert (got[:, 3::4, n - 1] != 0).any()


def test_chain_is_the_derivative_of_models_of():
    """Against autograd through models_of itself, for the quadratic density."""
    model = chain_model(lambda vp: 1.2 + 0.3 * vp - 0.02 * vp * vp)
    lo, hi = (torch.from_numpy(b) for b in model.bounds())
    u = torch.from_numpy(np.random.default_rng(6).uniform(size=(1, 8)))
    J = torch.autograd.functional.jacobian(lambda u: model.models_of(lo + u * (hi - lo)).reshape(-1), u)[:, 0]
    got = model.chain(lo + u * (hi - lo))[0]
    assert (got - J).abs().max() <= 1e-14 * J.abs().max()


def test_chain_and_refine_refuse_bad_input():
    from das_diff_veh_amd.inversion import Curve, EarthModel, Layer
    model = chain_model(lambda vp: 1.56 + 0.186 * vp)
    with pytest.raises(ValueError):
        model.chain(torch.zeros((2, 7), dtype=torch.float64))
    with pytest.raises(ValueError):
        model.chain(torch.zeros((2, 8), dtype=torch.float32))
    curve = Curve([0.1, 0.2], [0.3, 0.3], 0, "rayleigh", "phase")
    lo, hi = model.bounds()
    x = 0.5 * (lo + hi)[None]
    for bad in (dict(xs=x[:, :7]), dict(xs=x + 1.0), dict(maxiter=-1), dict(lam0=0.0), dict(tol=float("nan")),
                dict(curves=[])):
        with pytest.raises(ValueError):  # before any device work: there is no device here
            model.refine(**{**dict(curves=[curve], xs=x), **bad})
    with pytest.raises(TypeError):
        model.refine(["curve"], x)
    with pytest.raises(ValueError):
        model.refine([Curve([0.1], [0.3], 0, "rayleigh", "group")], x)
    with pytest.raises(ValueError):
        EarthModel().add(Layer([0.1, 0.2], [0.1, 0.3])).refine([curve], x)  # not configured


ROUNDING_BOUNDS = [(0.03, 0.3), (0.015, 0.15), (0.03, 0.45)]  # lo + (hi - lo) is one ulp above hi for each


def test_starts_an_ulp_outside_the_cube_are_taken():
    """invert forms lo + u (hi - lo); at u = 1 these bounds give a value one ulp above hi, which refine's input check
    must take (NumPy and tensor alike).  Two ulps outside, on either side, is refused, before any device work."""
    from das_diff_veh_amd.inversion import Curve, EarthModel, Layer, starts_in_bounds
    model = EarthModel()
    model.add(Layer(ROUNDING_BOUNDS[1], ROUNDING_BOUNDS[0], [0.25, 0.25]))
    model.add(Layer(ROUNDING_BOUNDS[2], [0.4, 0.8], [0.25, 0.25]))
    model.configure(density=lambda vp: 1.56 + 0.186 * vp)
    lo, hi = model.bounds()
    top = lo + 1.0 * (hi - lo)  # as invert does at u = 1
    assert (top[:2] > hi[:2]).all() and np.array_equal(top[:2], np.nextafter(hi[:2], np.inf))
    for xs in (top[None], lo[None], hi[None], np.stack([top, lo])):
        assert starts_in_bounds(xs, lo, hi) and starts_in_bounds(torch.from_numpy(xs), lo, hi)
    curve = Curve([0.1, 0.2], [0.3, 0.3], 0, "rayleigh", "phase")
    for k in (0, 1):
        for bad in (np.nextafter(top[k], np.inf), np.nextafter(np.nextafter(lo[k], -np.inf), -np.inf)):
            xs = hi[None].copy()
            xs[0, k] = bad
            assert not starts_in_bounds(xs, lo, hi) and not starts_in_bounds(torch.from_numpy(xs), lo, hi)
            for given in (xs, torch.from_numpy(xs)):
                with pytest.raises(ValueError, match="inside the bounds"):
                    model.refine([curve], given)


def test_run_best_picks_each_runs_first_minimum():
    from das_diff_veh_amd.inversion import InversionResult
    f = np.array([3.0, 1.0, 2.0, 1.0, np.inf, np.inf, np.inf, np.inf, 5.0, 4.0, 4.0, 6.0])  # 3 runs of 2 x 2
    xs = np.arange(24.0).reshape(12, 2)
    res = InversionResult(xs, np.zeros((12, 1, 4)), f, np.zeros((3, 2)), 3, 2, 2)
    best = res.run_best()
    assert np.array_equal(best, xs[[1, 4, 9]]) and best.base is None
