"""References of the chain solve (dvh_lm_solve_chain) and of the coupling terms of EarthModel.refine_section in
np.longdouble, the seeded chains they are held to and the derived bound, shared by tests/test_refine_section_host.py and
tests/test_refine_section_gpu.py.  Every case is built once (lru_cache) and never modified: the tests copy what they
change.

The bound.  With first-difference coupling the damped matrix A of a chain is block tridiagonal with diagonal blocks
beside the diagonal: over the n free parameters of each position it is a band matrix of half-bandwidth n, and the
kernel's block factorisation (S_k = A_k - X_{k-1} X_{k-1}^T, L_k = chol(S_k), X_k = B_k L_k^-T) computes, entry by
entry, exactly the Cholesky factor R^T R = A of that band matrix: the rows of R are [L_k^T  X_k^T].  refine_ref's dense
bound is Higham's backward error of a Cholesky solve, ||A x - b|| <= 2 n (3 n + 1) 2^-53 ||A|| ||x||, where n enters
twice: as the length of the longest inner product (3 n + 1 roundings over the factorisation and the two substitutions)
and through || |R^T| |R| || <= n ||A||.  For the band factor the longest inner product has the n - i products of
X_{k-1} X_{k-1}^T and the j of the reduction against L_k's finished columns (refine.h: schur_reduce, chol_reduce), at
most 2 n = m terms, and likewise in the substitutions (carry_forward with the column sweep; carry_back with it); and a
row or column of R holds at most n + 1 <= m entries, so || |R| ||_2^2 <= ||R||_1 ||R||_inf <= m ||R||_2^2 = m ||A||.
Hence

    ||A delta - r|| <= 2 m (3 m + 1) 2^-53 ||A|| ||delta||,   m = 2 n_free,

for a chain of any length, the factor 2 again for forming A and r: an entry of A takes at most 4 roundings, and an
entry of q at most 5 relative to mu (w_{k-1} + w_k) max|u - u'|, which with the cases' mu w <= 1, u in the unit cube
and g of unit variance (so ||A|| ||delta|| >= ||r|| is about sqrt(L n)) is a few 2^-53 ||r||.
"""
import functools

import numpy as np

from tests import refine_ref as ref

LD = np.longdouble
SIZES = [1, 2, 17, 64, 65, 95]
LENGTHS = [1, 2, 3, 7]
N_CHAIN = 3
CONDITIONS = (1e2, 1e8, 1e8)  # chain 2 has a singular block at its middle position as well


@functools.lru_cache(maxsize=None)
def chain_case(D, L):
    """Three chains of L positions under refine_ref.solve_case(D)'s free mask: blocks of condition 1e2 (chain 0) and 1e8
    (chains 1 and 2, the latter with a singular PSD block of rank D - 1 in the middle, which the neighbours or lambda
    rescue), built as solve_case builds them; g of unit variance, u in the unit cube, a lambda per chain, mu in
    0.05 .. 0.5 with zeros in it (D > 1), links in 0.5 .. 2."""
    rng = np.random.default_rng(9000 + 10 * D + L)
    free = ref.solve_case(D)["free"]
    H = np.empty((N_CHAIN, L, D, D))
    for c, cond in enumerate(CONDITIONS):
        for k in range(L):
            Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
            H[c, k] = (Q * np.logspace(0.0, -np.log10(cond), D)) @ Q.T
    if D > 1:
        B = rng.standard_normal((D, D - 1))
        H[2, L // 2] = B @ B.T
    H = 0.5 * (H + H.transpose(0, 1, 3, 2))
    mu = rng.uniform(0.05, 0.5, D)
    if D > 1:
        mu[rng.uniform(size=D) < 0.3] = 0.0
        mu[int(np.flatnonzero(free)[-1])] = 0.0   # a free parameter that is not coupled (where there are two)
        mu[int(np.flatnonzero(free)[0])] = 0.25   # and one that is
    case = dict(H=H.reshape(N_CHAIN * L, D, D), g=rng.standard_normal((N_CHAIN * L, D)),
                u=rng.uniform(0.0, 1.0, (N_CHAIN * L, D)), lam=np.array([1e-3, 1e-6, 1e-2]), free=free, mu=mu,
                link=rng.uniform(0.5, 2.0, (N_CHAIN, L - 1)))
    for a in case.values():
        a.setflags(write=False)
    return dict(case, D=D, L=L)


def coupling_terms(u, mu, link):
    """P [C] and q [C, L, D] of the definitions in np.longdouble: u [C, L, D], mu [D], link [C, L - 1]."""
    u, mu, w = u.astype(LD), mu.astype(LD), link.astype(LD)
    du = u[:, 1:] - u[:, :-1]                                    # [C, L - 1, D]
    P = 0.5 * (w[:, :, None] * mu * du * du).sum(axis=(1, 2))
    q = np.zeros_like(u)
    q[:, 1:] += mu * w[:, :, None] * du
    q[:, :-1] -= mu * w[:, :, None] * du
    return P, q


def dense_system(H, g, u, lam, free, mu, link):
    """A [L n, L n] and r [L n] of one chain over its free parameters in np.longdouble: H [L, D, D], g and u [L, D],
    link [L - 1]."""
    L = H.shape[0]
    at = np.flatnonzero(free)
    n = at.size
    A = np.zeros((L * n, L * n), LD)
    _, q = coupling_terms(u[None], mu, link[None])
    for k in range(L):
        block, _ = ref.damped(H[k], lam, free)
        w = (link[k - 1] if k > 0 else 0.0) + (link[k] if k + 1 < L else 0.0)
        block[np.diag_indices(n)] += LD(w) * mu[at].astype(LD)
        A[k * n:(k + 1) * n, k * n:(k + 1) * n] = block
        if k + 1 < L:
            off = np.diag(-LD(link[k]) * mu[at].astype(LD))
            A[k * n:(k + 1) * n, (k + 1) * n:(k + 2) * n] = off
            A[(k + 1) * n:(k + 2) * n, k * n:(k + 1) * n] = off
    r = -(g[:, at].astype(LD) + q[0][:, at]).reshape(-1)
    return A, r, at


def bound_of(n_free):
    m = 2 * n_free
    return 2.0 * m * (3 * m + 1) * 2.0 ** -53


def chain_of(case, c, **changed):
    """The arrays of chain c of a case (or of the case with some arrays replaced) as dense_system takes them."""
    a = {**case, **changed}
    L = case["L"]
    rows = slice(c * L, (c + 1) * L)
    return a["H"][rows], a["g"][rows], a["u"][rows], a["lam"][c], a["free"], a["mu"], a["link"][c]


def residual_of(delta, system):
    """||A delta - r|| / (||A|| ||delta||) of one chain's step [L, D] in np.longdouble, and the system's bound."""
    A, r, at = system
    x = delta[:, at].astype(LD).reshape(-1)
    res = float(np.linalg.norm(A @ x - r))
    scale = float(np.linalg.norm(A.astype(np.float64), 2) * np.linalg.norm(x))
    return res / scale, bound_of(at.size)


def assert_chains(delta, status, case, name=""):
    """(delta [3 L, D], status [3]) of a call on a case: every chain solves, within the bound; fixed parameters get
    exactly 0.  -> the worst ratio of a residual to its bound."""
    D, L = case["D"], case["L"]
    fixed = case["free"] == 0
    assert delta.shape == (N_CHAIN * L, D) and (delta[:, fixed] == 0).all() and not np.signbit(delta[:, fixed]).any()
    worst = 0.0
    for c in range(N_CHAIN):
        assert status[c] == 0, (name, c, status[c])
        rows = delta[c * L:(c + 1) * L]
        assert np.isfinite(rows).all()
        res, bound = residual_of(rows, dense_system(*chain_of(case, c)))
        print(f"{name} D {D} L {L} chain {c}: residual {res:.2e} of bound {bound:.2e}")
        assert res <= bound
        worst = max(worst, res / bound)
    return worst
