"""dvh_rayleigh_modes and dvh_rayleigh_sens on the device over the wide case table (tests/rayleigh_wide_ref.py,
tests/golden/rayleigh_wide.npz): Poisson's ratios 0.05 .. 0.49 and mixed, 32 rows, a stiff cap, a half-space ten times
faster than the top, more brackets than the 16 slots, neighbouring brackets, twelve scan rounds and a clamped sublayer
count, against the oracle's recorded roots; the six-row cases as one batch; and Euler's identities of the
sensitivities, held to ten times the host path's residual (tests/test_rayleigh_wide_host.py)."""
import numpy as np
import pytest

from tests import rayleigh_ref as ref
from tests import rayleigh_wide_ref as wide
from tests.test_rayleigh_gpu import POISON, TOL, launch
from tests.test_rayleigh_sens_gpu import omega_c_omega, sens
from tests.test_rayleigh_wide_host import DISPERSIVE, FLAT_MODE_0, SENS_MODES, euler_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return wide.load()


def periods_of(name):
    return np.array([1.0 / f for f in wide.CASES[name][1]])


@pytest.mark.parametrize("n_mode", [1, 16])
@pytest.mark.parametrize("name", list(wide.CASES))
def test_modes_match_the_oracle(device, recorded, name, n_mode):
    """One launch per case and mode count, every mode wanted: the roots to 1e-9 relative, NaN exactly where the oracle
    has fewer brackets, count = min(need, brackets) (16 with every slot filled where the oracle has more), and no slot
    left unwritten.  Of `clamped` four roots are recorded: the other slots are finite and increasing."""
    layers, freqs, c_min, _ = wide.CASES[name]
    c, count = launch(device, layers, periods_of(name), [n_mode] * len(freqs), n_mode, c_min, dc=wide.DC)
    assert not (c == POISON).any() and not (count == -99).any()
    worst = 0.0
    for i in range(len(freqs)):
        signs, roots = recorded[name, i]
        n = min(n_mode, wide.brackets(signs).size)
        got = c[0, i]
        assert count[0, i] == n, (name, i, count[0, i], n)
        assert np.isfinite(got[:n]).all() and np.isnan(got[n:]).all(), (name, i, got)
        assert (np.diff(got[:n]) > 0).all(), (name, i, got)
        m = min(n, roots.size)
        assert m == n or name == "clamped"
        err = np.abs(got[:m] - roots[:m]) / roots[:m]
        worst = max(worst, err.max())
        assert (err <= TOL).all(), (name, i, err.max(), got, roots)
    print(f"{name}, n_mode {n_mode}: largest relative root error on the device {worst:.2e}")


def test_six_row_batch_equals_single_launches(device, recorded):
    """The five six-row cases x two periods as one launch (10 waves, not a multiple of the block's 4): each (model,
    period) equals its own launch bit for bit, and the recorded roots where the file has the pair."""
    models = np.stack([wide.CASES[name][0] for name in wide.SIX_ROW])
    freqs = (5.0, 25.0)
    periods, need = np.array([1.0 / f for f in freqs]), np.array([16, 16], np.int32)
    c, count = launch(device, models, periods, need, 16, 0.12, dc=wide.DC)
    assert not (c == POISON).any() and not (count == -99).any()
    for a, name in enumerate(wide.SIX_ROW):
        for b in range(2):
            c1, n1 = launch(device, models[a], periods[b:b + 1], need[b:b + 1], 16, 0.12, dc=wide.DC)
            assert n1[0, 0] == count[a, b]
            assert np.array_equal(c1[0, 0], c[a, b], equal_nan=True), (name, b)
            if freqs[b] in wide.CASES[name][1]:
                signs, roots = recorded[name, wide.CASES[name][1].index(freqs[b])]
                assert count[a, b] == roots.size == min(16, wide.brackets(signs).size)
                assert (np.abs(c[a, b, :roots.size] - roots) <= TOL * roots).all(), (name, b)
    assert len({tuple(x) for x in c[:, 1]}) == len(wide.SIX_ROW)  # the models do differ


@pytest.mark.parametrize("name", list(wide.CASES))
def test_sens_satisfies_eulers_identities(device, name):
    """No oracle: sum h c_h = omega c_omega, sum (alpha c_alpha + beta c_beta) + omega c_omega = c, sum rho c_rho = 0
    at the first three modes, within ten times the residual of the host path on these models (`thick` and `clamped`
    have figures of their own); NaN exactly where the root is NaN.  No case here is a half-space, so U = c nowhere but at mode 0 of
    `thick` and `clamped`, the top layer's own Rayleigh wave (k h of 196 and 2 957 hide everything below it): there
    U = c within the bound and c is the cubic's root."""
    layers, freqs, c_min, _ = wide.CASES[name]
    bound = euler_bound(name)
    r = sens(device, layers, periods_of(name), SENS_MODES, c_min)
    ok = np.isfinite(r["c_in"])
    assert ok[0, :, 0].all()
    for k in ("c", "u"):
        assert np.array_equal(np.isfinite(r[k]), ok), (name, k)
    assert np.isfinite(r["p"][ok]).all() and np.isnan(r["p"][~ok]).all()
    c, u = r["c"], r["u"]
    w = layers[None, None, None] * r["p"]
    wcw = omega_c_omega(c, u)
    worst = 0.0
    for e in (w[..., 0].sum(-1) - wcw, w[..., 1].sum(-1) + w[..., 2].sum(-1) + wcw - c, w[..., 3].sum(-1)):
        worst = max(worst, (np.abs(e[ok]) / c[ok]).max())
    print(f"{name}: largest Euler residual over c on the device {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound, (name, worst)
    flat = np.zeros_like(ok)
    if name in FLAT_MODE_0:
        flat[0, :, 0] = True
        want = layers[0, 2] * ref.rayleigh_cubic(0.3)
        assert (np.abs(c[flat] - want) <= TOL * want).all()
        assert (np.abs(u[flat] - c[flat]) <= bound * c[flat]).all(), (u[flat], c[flat])
    rest = ok & ~flat
    print(f"{name}: smallest |U / c - 1| of a dispersive mode {np.abs(u[rest] / c[rest] - 1.0).min():.2e}")
    assert (np.abs(u[rest] - c[rest]) > DISPERSIVE * bound * c[rest]).all()
