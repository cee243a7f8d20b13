"""References of the Gauss-Newton refinement entries (dvh_lm_normal, dvh_lm_solve) in np.longdouble, the random cases
they are held to and the derived bounds, shared by tests/test_refine_host.py and tests/test_refine_gpu.py.  Every case
and its reference is built once (lru_cache) and never modified: the tests copy what they change."""
import functools

import numpy as np

LD = np.longdouble
N_PERIOD, N_MODE, N_MODEL = 37, 3, 3
RHO_FLOOR = 1e-12
SHAPES = [(1, 2), (3, 8), (32, 95)]                      # (n_layer, D)
CURVE_SIZES = {1: (1,), 13: (5, 1, 7), 257: (100, 1, 156)}  # S -> samples per curve
SOLVE_SIZES = [1, 2, 16, 17, 64, 65, 95]
TABLE_KEYS = ("sample_period", "sample_mode", "sample_obs", "sample_sigma", "sample_curve")


@functools.lru_cache(maxsize=None)
def normal_case(n_layer, D, S):
    """A random problem of N_MODEL models: interleaved samples of the curves of CURVE_SIZES[S] with random sigma and
    weights (as tests/test_misfit_gpu.py draws them), dense random dcdp rows and chain, and NaN in every slot of c and
    dcdp that no sample names."""
    rng = np.random.default_rng(1000 * n_layer + 10 * S + D)
    sizes = CURVE_SIZES[S]
    K = 4 * n_layer
    curve = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    if len(sizes) > 1:
        assert (np.diff(curve) < 0).any()  # not grouped by curve
    tab = dict(sample_period=rng.integers(0, N_PERIOD, S).astype(np.int32),
               sample_mode=rng.integers(0, N_MODE, S).astype(np.int32),
               sample_obs=rng.uniform(0.2, 0.9, S), sample_sigma=rng.uniform(0.01, 0.05, S), sample_curve=curve,
               curve_weight=rng.uniform(0.5, 2.0, len(sizes)))
    c = rng.uniform(0.1, 1.0, (N_MODEL, N_PERIOD, N_MODE))
    dcdp = rng.uniform(-1.0, 1.0, (N_MODEL, N_PERIOD, N_MODE, n_layer, 4))
    chain = rng.uniform(-1.0, 1.0, (N_MODEL, K, D))
    sampled = np.zeros((N_PERIOD, N_MODE), bool)
    sampled[tab["sample_period"], tab["sample_mode"]] = True
    assert S >= N_PERIOD * N_MODE or not sampled.all()
    c[:, ~sampled] = np.nan
    dcdp[:, ~sampled] = np.nan
    for a in (c, dcdp, chain, *tab.values()):
        a.setflags(write=False)
    return dict(c=c, dcdp=dcdp, chain=chain, tab=tab, n_layer=n_layer, D=D, S=S)


def normal_reference(c, dcdp, chain, tab, rho_floor=RHO_FLOOR):
    """f [M], g [M, D], H [M, D, D] of the definitions in np.longdouble, and the same expressions of g and H evaluated
    on absolute values (|r_s|, |dcdp| |chain|), which the rounding bound scales with."""
    M = c.shape[0]
    K, D = chain.shape[1:]
    sp, sm, sc = tab["sample_period"], tab["sample_mode"], tab["sample_curve"]
    sigma, w = tab["sample_sigma"].astype(LD), tab["curve_weight"].astype(LD)
    W = w.sum()
    f, g, H, ga, Ha = (np.zeros(s, LD) for s in ((M,), (M, D), (M, D, D), (M, D), (M, D, D)))
    for m in range(M):
        r = (c[m, sp, sm].astype(LD) - tab["sample_obs"].astype(LD)) / sigma
        rows = dcdp[m, sp, sm].reshape(sp.size, K).astype(LD)
        J = (rows @ chain[m].astype(LD)) / sigma[:, None]
        Ja = (np.abs(rows) @ np.abs(chain[m]).astype(LD)) / sigma[:, None]
        a = np.zeros(sp.size, LD)
        for i in range(w.size):
            of = sc == i
            rho = np.sqrt((r[of] ** 2).mean())
            f[m] += w[i] * rho / W
            a[of] = w[i] / (W * of.sum() * max(rho, LD(rho_floor)))
        g[m], ga[m] = (a * r) @ J, (a * np.abs(r)) @ Ja
        H[m], Ha[m] = (J * a[:, None]).T @ J, (Ja * a[:, None]).T @ Ja
    return f, g, H, ga, Ha


@functools.lru_cache(maxsize=None)
def normal_expected(n_layer, D, S):
    case = normal_case(n_layer, D, S)
    return normal_reference(case["c"], case["dcdp"], case["chain"], case["tab"])


def normal_bound(n_layer, S):
    """The recursive-summation bound of an entry of g or H relative to its absolute-value expression: K + 1 operations
    in j, S in the sum over the samples and in rho, and a factor 4 for the products, the square root and the division
    in a_i."""
    return 4.0 * (4 * n_layer + S + 4) * 2.0 ** -52


def assert_normal(got, n_layer, D, S):
    """(f, g, H, status) of a launch on normal_case(n_layer, D, S) against the reference."""
    f, g, H, status = got
    rf, rg, rH, ga, Ha = normal_expected(n_layer, D, S)
    assert (status == 0).all()
    bound = normal_bound(n_layer, S)
    eg, eH = np.abs(g.astype(LD) - rg) / ga, np.abs(H.astype(LD) - rH) / Ha
    print(f"n_layer {n_layer} D {D} S {S}: g {float(eg.max()):.2e}, H {float(eH.max()):.2e} of bound {bound:.2e}; "
          f"f {float(np.abs(f / rf - 1).max()):.2e}")
    assert (eg <= bound).all() and (eH <= bound).all()
    assert (np.abs(f.astype(LD) - rf) <= 1e-13 * rf).all()
    assert np.array_equal(H, H.transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------- solve

@functools.lru_cache(maxsize=None)
def solve_case(D):
    """Four models of D parameters under one mixed free mask: SPD of condition 1e2 and 1e8, a singular PSD matrix
    (rank D - 1; the zero matrix at D = 1) and the first matrix with the first free diagonal entry negated, which is
    indefinite in the free block; a lambda of its own each."""
    rng = np.random.default_rng(77 + D)
    free = (rng.uniform(size=D) < 0.7).astype(np.int32)
    free[rng.integers(0, D)] = 1
    if D > 1 and free.all():
        free[rng.integers(0, D)] = 0
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    H = np.empty((4, D, D))
    for m, cond in enumerate((1e2, 1e8)):
        H[m] = (Q * np.logspace(0.0, -np.log10(cond), D)) @ Q.T
    B = rng.standard_normal((D, D - 1))
    H[2] = B @ B.T
    H[3] = H[0]
    k0 = int(np.flatnonzero(free)[0])
    H[3, k0, k0] = -H[3, k0, k0]
    H = 0.5 * (H + H.transpose(0, 2, 1))
    g = rng.standard_normal((4, D))
    lam = np.array([1e-3, 1e-6, 1e-2, 1e-3])
    for a in (H, g, lam, free):
        a.setflags(write=False)
    return dict(H=H, g=g, lam=lam, free=free, D=D)


def damped(H, lam, free):
    """A = H + lambda diag(d) over the free parameters, in np.longdouble."""
    at = np.flatnonzero(free)
    A = H[np.ix_(at, at)].astype(LD)
    diag = np.diag(A).copy()
    A[np.diag_indices(at.size)] += LD(lam) * np.maximum(diag, LD(1e-12) * diag.max())
    return A, at


def assert_solve(delta, status, D):
    """(delta [4, D], status [4]) of a launch on solve_case(D): Higham's backward error of a Cholesky solve of n
    unknowns, ||A delta + g|| <= 2 n (3 n + 1) 2^-53 ||A|| ||delta|| with || |R^T| |R| || <= n ||A|| and a factor 2 for
    forming A; the indefinite model refuses; fixed parameters get exactly 0."""
    case = solve_case(D)
    fixed = case["free"] == 0
    assert (delta[:, fixed] == 0).all() and not np.signbit(delta[:, fixed]).any()
    rescued = [0, 1, 2] if D > 1 else [0, 1]  # the zero matrix has d = 0: lambda cannot rescue it
    for m in range(4):
        if m not in rescued:
            assert status[m] == 2 and (delta[m] == 0).all(), (m, status[m])
            continue
        assert status[m] == 0, (m, status[m])
        A, at = damped(case["H"][m], case["lam"][m], case["free"])
        n = at.size
        x = delta[m, at].astype(LD)
        res = float(np.linalg.norm(A @ x + case["g"][m, at].astype(LD)))
        scale = float(np.linalg.norm(A.astype(np.float64), 2) * np.linalg.norm(x))
        bound = 2.0 * n * (3 * n + 1) * 2.0 ** -53
        print(f"D {D} model {m}: residual {res / scale:.2e} of bound {bound:.2e}")
        assert np.isfinite(x.astype(np.float64)).all() and res <= bound * scale
