"""The wide case table (tests/rayleigh_wide_ref.py, tests/golden/rayleigh_wide.npz) without a GPU: the recorded file
against its table and against the oracle again, dvh_rayleigh_secular_host against the oracle's signs at every scan
point and on both sides of every recorded root, the float64 bisection's error per case, and Euler's identities
through dvh_rayleigh_tangent_host, whose worst residual sets the bound of the device test
(tests/test_rayleigh_wide_gpu.py)."""
import os

import mpmath as mp
import numpy as np
import pytest

from tests import rayleigh_ref as ref
from tests import rayleigh_wide_ref as wide
from tests.test_rayleigh_host import host_secular
from tests.test_rayleigh_sens_host import host_tangent

TOL = 1e-9
SENS_MODES = 3

# The largest residual over c of Euler's three identities through dvh_rayleigh_tangent_host, after one Newton step
# from the recorded root, over the first SENS_MODES modes (test_host_euler_residuals prints every case's and holds them
# to these figures, rounded up in the last digit).  The two single-layer cases of k h = 196 and 2 957 are a hundred
# times worse than the other eight, whose worst is `cap`'s, so each of the two has its own figure and the others are
# not widened by them.  The device test asserts ten times the figure, the convention of
# tests/test_rayleigh_sens_host.py.
WORST_HOST_EULER = 5.31e-14
WORST_HOST_EULER_DEEP = {"thick": 6.46e-12, "clamped": 4.48e-12}


def euler_bound(name):
    return 10.0 * WORST_HOST_EULER_DEEP.get(name, WORST_HOST_EULER)


# Mode 0 of these two is the top layer's own Rayleigh wave (k h of 196 and 2 957 hide what lies below): U = c within
# the bound.  Every other mode of the table is dispersive: |U / c - 1| is more than DISPERSIVE times the bound.
FLAT_MODE_0 = ("thick", "clamped")
BISECTED_AGAIN = {"thick": [1], "contrast": [0], "cap": [-1]}  # thick's is the root of a bracket that holds three
DISPERSIVE = 1e3


@pytest.fixture(scope="module")
def lib():
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    return wide.load()


def case_of(name, i):
    layers, freqs, c_min, digits = wide.CASES[name]
    return layers, wide.omega_of(freqs[i]), ref.scan_points(layers, c_min, wide.DC), digits


def test_case_table_matches_the_recorded_file(recorded):
    """Point counts, bracket counts = sign changes, the roots inside their brackets, the digits rule, and what the
    table is there to reach: more than 16 brackets, neighbouring brackets, twelve scan rounds, a clamped sublayer
    count."""
    assert set(recorded) == set(wide.keys())
    n_bracket, closest = {}, (np.inf, None)
    for (name, i), (signs, roots) in recorded.items():
        layers, omega, c, digits = case_of(name, i)
        assert digits >= wide.digits_needed(name), name
        assert signs.dtype == np.int8 and set(np.unique(signs)) <= {-1, 1}
        assert signs.size == c.size == wide.SCAN_POINTS[name], (name, i)
        at = wide.brackets(signs)
        n_bracket[name, i] = at.size
        assert roots.size == min(at.size, wide.n_recorded(name)), (name, i)
        assert (c[at[:roots.size]] < roots).all() and (roots < c[at[:roots.size] + 1]).all(), (name, i)
        if at.size > 1 and np.diff(at).min() < closest[0]:
            closest = (np.diff(at).min(), (name, i))
        if roots.size > 1:
            print(f"{name}@{wide.CASES[name][1][i]}: {at.size} brackets, closest recorded pair "
                  f"{np.diff(roots).min() / wide.DC:.2f} dc")
    print(f"closest brackets: {closest[0]} scan step(s) apart in {closest[1]}")
    assert n_bracket["nu005", 1] > 16 and n_bracket["nu02", 1] > 16 and n_bracket["gradient32", 0] > 16
    assert n_bracket["mixed_nu", 0] >= 16 and n_bracket["thick", 0] > 16
    assert np.diff(wide.brackets(recorded["thick", 0][0])).min() == 1  # neighbouring brackets
    assert wide.SCAN_POINTS["contrast"] > 11 * 64 and n_bracket["contrast", 0] >= 1
    layers, freqs, c_min, _ = wide.CASES["clamped"]
    kh = wide.omega_of(freqs[0]) / recorded["clamped", 0][1][0] * layers[0, 0]
    assert kh > 2048.0 and kh / 256.0 > 8.0  # kMaxSub clamps: k h_sub exceeds kSubKh
    assert len(wide.CASES["gradient32"][0]) == 32
    for name in wide.SIX_ROW:
        assert len(wide.CASES[name][0]) == 6


@pytest.mark.parametrize("name", list(wide.CASES))
def test_recorded_file_regenerates(recorded, name):
    """A subset of the file from the oracle again: signs at a stride of the scan points and, per (case, frequency), the
    first and the last recorded root.  A root is 140 evaluations of 0.02 to 0.6 s at these digits, so only the roots
    of BISECTED_AGAIN are made again and compared bit for bit; the others are held by the oracle's signs two float64
    spacings to either side of the recorded value, which are the signs of the bracket's ends."""
    layers, freqs, _, digits = wide.CASES[name]
    for i in range(len(freqs)):
        signs, roots = recorded[name, i]
        for k in range(i, signs.size, 29 if digits > 200 else 23):
            assert wide.sign_at(name, i, k) == signs[k], (name, i, k)
        at = wide.brackets(signs)
        again = [range(roots.size)[j] for j in BISECTED_AGAIN.get(name, ())]
        for m in sorted({0, roots.size - 1, *again}):
            if m not in again:
                for s, k in ((-1.0, at[m]), (1.0, at[m] + 1)):
                    x = float(roots[m] + s * 2.0 * np.spacing(roots[m]))
                    assert int(mp.sign(ref.secular(layers, x, wide.omega_of(freqs[i]), digits))) == signs[k], (name, m)
            else:
                assert wide.root_at(name, i, int(at[m])) == roots[m], (name, i, m)


def test_host_secular_signs_match_the_oracle(lib, recorded):
    """Finite, |D| <= 1, of the oracle's sign at every scan point farther than 1e-9 c from a recorded root, and of
    opposite signs at c_ref (1 -+ 1e-9) of every recorded root."""
    for (name, i), (signs, roots) in recorded.items():
        layers, omega, c, _ = case_of(name, i)
        v = host_secular(lib, layers, c, omega)
        assert np.isfinite(v).all() and np.abs(v).max() <= 1.0 + 1e-12, (name, i)
        far = np.array([roots.size == 0 or np.abs(roots - x).min() > 1e-9 * x for x in c])
        assert np.array_equal(np.where(v < 0, -1, 1)[far], signs[far]), (name, i, np.nonzero(~far)[0])
        below, above = (host_secular(lib, layers, roots * (1.0 + s * 1e-9), omega) for s in (-1.0, 1.0))
        assert np.all(below * above < 0), (name, i, below, above)
        at = wide.brackets(signs)[:roots.size]
        assert np.array_equal(np.where(below < 0, -1, 1), signs[at]), (name, i)


def test_brackets_of_three_roots_and_more(lib, recorded):
    """What `thick` and `clamped` reach: scan brackets that hold an odd number of roots above one.  The refinement's
    first step is then part of the definition (the first change of sign over its 64 points), and the recorded root is
    that one: it lies in the first part of the bracket's 65 over which the host path changes sign."""
    most = {}
    for (name, i), (signs, roots) in recorded.items():
        layers, omega, c, _ = case_of(name, i)
        for r, k in zip(roots, wide.brackets(signs)):
            x = np.r_[c[k], c[k] + np.arange(1, 65) * ((c[k + 1] - c[k]) / 65.0), c[k + 1]]
            neg = host_secular(lib, layers, x, omega) < 0
            at = np.nonzero(neg[1:] != neg[:-1])[0]
            assert at.size % 2 == 1 and x[at[0]] < r < x[at[0] + 1], (name, i, k, at)
            most[name] = max(most.get(name, 0), at.size)
    print("most changes of sign inside one recorded bracket: " + ", ".join(f"{k} {v}" for k, v in most.items()))
    assert most["thick"] == 3 and most["clamped"] >= 13
    assert all(v == 1 for k, v in most.items() if k not in ("thick", "clamped"))


def test_host_bisection_error(lib, recorded):
    """The roots a float64 bisection of the host entry converges to, from the bracket the first sectioning step
    leaves, against the oracle's: per case, for DESIGN.md."""
    for name in wide.CASES:
        worst = 0.0
        for i in range(len(wide.CASES[name][1])):
            signs, roots = recorded[name, i]
            layers, omega, c, _ = case_of(name, i)
            for r, k in zip(roots, wide.brackets(signs)):
                lo, hi = wide.section(c[k], c[k + 1], lambda pts: host_secular(lib, layers, pts, omega) < 0)
                neg = host_secular(lib, layers, lo, omega)[0] < 0
                for _ in range(60):
                    mid = 0.5 * (lo + hi)
                    if (host_secular(lib, layers, mid, omega)[0] < 0) == neg:
                        lo = mid
                    else:
                        hi = mid
                worst = max(worst, abs(0.5 * (lo + hi) - r) / r)
        print(f"{name}: largest relative root error of the host path {worst:.2e}")
        assert worst <= TOL, name


def euler_residuals(layers, omega, c, dD):
    """The three identities' residuals over c, from D's derivatives at c [n]: dD [n][2 + 4 n_layer]."""
    wcw = -omega * dD[:, 1] / dD[:, 0]
    w = layers[None] * (-dD[:, 2:] / dD[:, :1]).reshape(c.size, len(layers), 4)
    return np.abs(np.stack([w[..., 0].sum(-1) - wcw, w[..., 1].sum(-1) + w[..., 2].sum(-1) + wcw - c,
                            w[..., 3].sum(-1)]) / c)


def test_host_euler_residuals(lib, recorded):
    """sum h c_h = omega c_omega, sum (alpha c_alpha + beta c_beta) + omega c_omega = c and sum rho c_rho = 0 at the
    first three recorded roots of every wide case, after the Newton step the kernel takes."""
    worst, flat0, dispersive = {}, {}, {}
    for (name, i), (_, roots) in recorded.items():
        layers, omega, _, _ = case_of(name, i)
        c0 = roots[:SENS_MODES]
        D0, dD0 = host_tangent(lib, layers, c0, omega, [0])
        c1 = c0 - D0 / dD0[:, 0]
        assert (np.abs(c1 - c0) <= 4e-9 * c0).all(), (name, i)
        _, dD = host_tangent(lib, layers, c1, omega)
        assert np.isfinite(dD).all() and (dD[:, 0] != 0.0).all(), (name, i)
        worst[name] = max(worst.get(name, 0.0), euler_residuals(layers, omega, c1, dD).max())
        # U / c - 1 = (omega / c) c_omega / (1 - (omega / c) c_omega): what the device test takes as dispersive
        x = -omega * dD[:, 1] / dD[:, 0] / c1
        flat = np.abs(x / (1.0 - x))
        if name in FLAT_MODE_0:
            flat0[name], flat = flat[0], flat[1:]
        dispersive[name] = min(dispersive.get(name, np.inf), flat.min())
    for name, e in worst.items():
        print(f"{name}: largest Euler residual over c on the host {e:.2e}, smallest |U / c - 1| of a dispersive mode "
              f"{dispersive[name]:.2e}" + (f", of mode 0 {flat0[name]:.2e}" if name in flat0 else ""))
    measured = dict(WORST_HOST_EULER_DEEP, rest=WORST_HOST_EULER)
    got = {name: worst[name] for name in WORST_HOST_EULER_DEEP}
    got["rest"] = max(e for name, e in worst.items() if name not in WORST_HOST_EULER_DEEP)
    print(", ".join(f"{name} {e:.2e}" for name, e in got.items()))
    for name, e in got.items():
        assert 0.5 * measured[name] <= e <= measured[name], (name, e)  # the figures above are these
    for name in worst:
        assert dispersive[name] > DISPERSIVE * euler_bound(name), name
        assert name not in flat0 or flat0[name] <= euler_bound(name), name
