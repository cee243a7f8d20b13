"""The tangent of the Rayleigh secular function without a GPU: dvh_rayleigh_tangent_host (csrc/rayleigh_tangent.h, the
header the sensitivity kernel compiles, run on the CPU) against the 80-digit oracle's derivatives at every recorded root
(tests/golden/rayleigh_sens.npz, tests/rayleigh_sens_ref.py), the oracle against Euler's identities, the value part
against dvh_rayleigh_secular_host bit for bit, and the argument checks of both new entries.

The error measure is dimensionless: |p_l (got - want)| / c per (layer, column) entry and |omega (got - want)| / c for
dc/domega.  Raw kernel entries span 1e-29 .. 1, so a per-entry relative error would mean nothing."""
import ctypes
import os

import numpy as np
import pytest

from tests import rayleigh_ref as ref
from tests import rayleigh_sens_ref as sref

# The largest dimensionless error of the host path over every recorded root (test_tangent_matches_the_oracle prints
# it: 7.09e-14 at the roots rounded to float64, 1.43e-13 after a Newton step from c_ref (1 -+ 1e-9)).  The bound the
# host and the GPU tests assert is ten times that: the margin covers FMA contraction differing between the host and
# the device compile and the device's own root position inside its bracket.  It is far inside the forward model's
# 1e-6 contract.
WORST_HOST_ERROR = 1.43e-13
BOUND = 10.0 * WORST_HOST_ERROR


@pytest.fixture(scope="module")
def lib():
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return sref.load_sens()


def golden_points(golden):
    """(label, layers, omega, c [n], dcdw [n], dcdp [n][n_layer][4]) of every recorded (case, frequency) with roots."""
    for name, (layers, _) in ref.CASES.items():
        for i, f in enumerate(ref.FREQS):
            c, dcdw, dcdp = golden[name, i]
            if c.size:
                yield f"{name}@{f}", layers, sref.omega_of(f), c, dcdw, dcdp
    g = golden["grazing"]
    yield "grazing", ref.CASES[sref.GRAZING_LAYERS][0], sref.omega_of(g["freq"]), g["c"], g["dcdw"], g["dcdp"]


def host_tangent(lib, layers, c, omega, dirs=None):
    """dvh_rayleigh_tangent_host -> (D [n_c], dD [n_c][n_dir]); dirs None takes every direction of the model."""
    layers = np.ascontiguousarray(layers, np.float64)
    c = np.ascontiguousarray(np.atleast_1d(c), np.float64)
    dirs = np.arange(2 + 4 * len(layers), dtype=np.int32) if dirs is None else np.ascontiguousarray(dirs, np.int32)
    D, dD = np.full(c.size, 7.0), np.full((c.size, dirs.size), 7.0)
    assert lib.dvh_rayleigh_tangent_host(layers.ctypes.data, len(layers), c.ctypes.data, c.size, omega,
                                         dirs.ctypes.data, dirs.size, D.ctypes.data, dD.ctypes.data) == 0
    return D, dD


def errors(layers, omega, c, dD, dcdw, dcdp):
    """The dimensionless errors of -dD_omega / dD_c and -dD_p / dD_c at the points c [n] -> (omega's, the layers')."""
    got_w = -dD[:, 1] / dD[:, 0]
    got_p = (-dD[:, 2:] / dD[:, :1]).reshape(dcdp.shape)
    return (np.abs(omega * (got_w - dcdw)) / c).max(), (np.abs(layers[None] * (got_p - dcdp)) / c[:, None, None]).max()


def test_golden_file_covers_the_case_table(golden):
    n = 0
    recorded = ref.load()
    for name, (layers, _) in ref.CASES.items():
        for i in range(len(ref.FREQS)):
            c, dcdw, dcdp = golden[name, i]
            roots = recorded[name, i][1]
            assert c.size == min(roots.size, sref.MAX_MODES) and np.array_equal(c, roots[:c.size])
            assert dcdw.shape == (c.size,) and dcdp.shape == (c.size, len(layers), 4)
            assert np.isfinite(dcdw).all() and np.isfinite(dcdp).all()
            n += c.size
    g = golden["grazing"]
    beta = ref.CASES[sref.GRAZING_LAYERS][0][g["layer"], 2]
    assert g["c"].size == sref.GRAZING_MODES and 0.0 < g["c"][1] / beta - 1.0 <= 1e-5
    assert n == 74


def test_oracle_satisfies_eulers_identities(golden):
    """c is homogeneous of degree 0 in (h, 1 / omega) and in rho, and of degree 1 in (alpha, beta, omega): the recorded
    derivatives obey the three identities to float64 rounding of their sums."""
    for label, layers, omega, c, dcdw, dcdp in golden_points(golden):
        w = layers[None] * dcdp
        assert np.abs(w[:, :, 0].sum(1) - omega * dcdw).max() <= 1e-14 * c.max(), label
        assert np.abs(w[:, :, 1].sum(1) + w[:, :, 2].sum(1) + omega * dcdw - c).max() <= 1e-14 * c.max(), label
        assert np.abs(w[:, :, 3].sum(1)).max() <= 1e-14 * c.max(), label


def test_oracle_derivatives_regenerate(golden):
    """Two recorded roots from the oracle again (a half-space and the one-layer case's first overtone at 10 Hz)."""
    for name, i, m in (("halfspace1", 2, 0), ("one_layer", 2, 1)):
        c, dcdw, dcdp = golden[name, i]
        got = sref.derivatives(ref.CASES[name][0], sref.omega_of(ref.FREQS[i]), float(c[m]))
        assert got[0] == c[m] and got[1] == dcdw[m] and np.array_equal(got[2], dcdp[m])


def test_tangent_matches_the_oracle(lib, golden):
    """-dD_p / dD_c and -dD_omega / dD_c at every recorded root rounded to float64, and at c_ref (1 -+ 1e-9) followed
    by one Newton step on the host: the worst dimensionless error is printed (it is WORST_HOST_ERROR) and held to
    BOUND."""
    worst = {"at the root": 0.0, "after a Newton step": 0.0}
    for label, layers, omega, c, dcdw, dcdp in golden_points(golden):
        _, dD = host_tangent(lib, layers, c, omega)
        assert np.isfinite(dD).all() and (dD[:, 0] != 0.0).all(), label
        e = max(errors(layers, omega, c, dD, dcdw, dcdp))
        worst["at the root"] = max(worst["at the root"], e)
        assert e <= BOUND, (label, e)
        for s in (-1.0, 1.0):
            c0 = c * (1.0 + s * 1e-9)
            D0, dD0 = host_tangent(lib, layers, c0, omega, [0])
            c1 = c0 - D0 / dD0[:, 0]
            assert (np.abs(c1 - c0) <= 4e-9 * c0).all(), label  # the step the kernel accepts
            assert (np.abs(c1 - c) <= 1e-13 * c).all(), (label, np.abs(c1 / c - 1.0).max())
            _, dD1 = host_tangent(lib, layers, c1, omega)
            e = max(errors(layers, omega, c, dD1, dcdw, dcdp))
            worst["after a Newton step"] = max(worst["after a Newton step"], e)
            assert e <= BOUND, (label, s, e)
    print("largest dimensionless error of the host tangent: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_a_root_off_by_the_refinement_width_is_not_enough(lib, golden):
    """Why the Newton step is not optional: without it, at c_ref (1 + 1e-9), the notebook case at 25 Hz misses BOUND."""
    c, dcdw, dcdp = golden["notebook", 4]
    layers, omega = ref.CASES["notebook"][0], sref.omega_of(ref.FREQS[4])
    _, dD = host_tangent(lib, layers, c * (1.0 + 1e-9), omega)
    assert max(errors(layers, omega, c, dD, dcdw, dcdp)) > BOUND


def test_value_part_is_the_secular_function(lib, golden):
    """The tangent's value output equals dvh_rayleigh_secular_host bit for bit, at scan points and at roots."""
    for name, (layers, _) in ref.CASES.items():
        layers = np.ascontiguousarray(layers)
        for i, f in enumerate(ref.FREQS):
            c = np.concatenate([ref.scan_points(layers, ref.c_min_of(name))[::5], golden[name, i][0]])
            want = np.full(c.size, 7.0)
            assert lib.dvh_rayleigh_secular_host(layers.ctypes.data, len(layers), c.ctypes.data, c.size,
                                                 sref.omega_of(f), want.ctypes.data) == 0
            for dirs in ([0], [1, 2 + 4 * (len(layers) - 1) + 2], None):
                D, _ = host_tangent(lib, layers, c, sref.omega_of(f), dirs)
                assert np.array_equal(D, want), (name, f, dirs)


def test_skipped_rows_have_zero_derivatives(lib):
    """A row with h = 0 and the half-space's h: derivative exactly 0, and the other rows' derivatives unchanged."""
    layers = ref.CASES["lvz"][0]
    padded = np.concatenate([layers[:1] * [0.0, 1.0, 1.0, 1.0], layers])
    c, omega = np.array([0.25, 0.4]), sref.omega_of(10.0)
    D, dD = host_tangent(lib, layers, c, omega)
    Dp, dDp = host_tangent(lib, padded, c, omega)
    assert np.array_equal(D, Dp) and np.array_equal(dDp[:, 2:6], np.zeros((2, 4)))
    assert np.array_equal(dDp[:, :2], dD[:, :2]) and np.array_equal(dDp[:, 6:], dD[:, 2:])
    assert np.array_equal(dD[:, 2 + 4 * 3], np.zeros(2))  # the half-space's h


def test_tangent_host_refusals(lib):
    layers = np.ascontiguousarray(ref.CASES["one_layer"][0])
    c, dirs = np.array([0.3, -1.0, 0.0]), np.array([0, 1, 9], np.int32)
    D, dD = np.zeros(3), np.zeros((3, 3))
    L, C, R, O, Q = layers.ctypes.data, c.ctypes.data, dirs.ctypes.data, D.ctypes.data, dD.ctypes.data
    f = lib.dvh_rayleigh_tangent_host
    assert f(L, 2, C, 3, 10.0, R, 3, O, Q) == 0
    assert np.isfinite(D[0]) and np.isfinite(dD[0]).all() and np.isnan(D[1:]).all() and np.isnan(dD[1:]).all()
    for at in (0, 2, 5, 7, 8):
        a = [L, 2, C, 3, 10.0, R, 3, O, Q]
        a[at] = None
        assert f(*a) == -2, at
    assert f(L, 0, C, 3, 10.0, R, 3, O, Q) == -2 and f(L, 2, C, -1, 10.0, R, 3, O, Q) == -2
    assert f(L, 2, C, 3, 10.0, R, 0, O, Q) == -2
    assert f(L, 2, C, 3, 0.0, R, 3, O, Q) == -2 and f(L, 2, C, 3, float("inf"), R, 3, O, Q) == -2
    assert f(L, 33, C, 3, 10.0, R, 3, O, Q) == -4
    assert f(None, 2, None, 0, 10.0, None, 3, None, None) == 0
    for bad in (-1, 10):
        d2 = np.array([0, bad], np.int32)
        assert f(L, 2, C, 3, 10.0, d2.ctypes.data, 2, O, Q) == -2 and b"direction" in lib.dvh_last_error()
    worse = layers.copy()
    worse[1, 3] = 0.0  # rho = 0
    assert f(worse.ctypes.data, 2, C, 3, 10.0, R, 3, O, Q) == -2 and b"alpha > beta" in lib.dvh_last_error()


def test_sens_refuses_before_any_launch(lib):
    """The argument checks of dvh_rayleigh_sens return before a device is touched."""
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused or empty
    sens = lambda *a: lib.dvh_rayleigh_sens(*a, None)
    ok = (p, 2, 3, p, 5, p, 4, 15, 1e-9, p, p, p)
    for at in (0, 3, 5):
        assert sens(*ok[:at], None, *ok[at + 1:]) == -2, at
    assert sens(*ok[:9], None, None, None) == -2 and b"output" in lib.dvh_last_error()
    for at, bad in ((1, -1), (2, 0), (4, -1), (6, 0), (7, -1), (7, 16), (8, 0.0), (8, float("nan")),
                    (8, float("inf"))):
        assert sens(*ok[:at], bad, *ok[at + 1:]) == -2, (at, bad)
    assert sens(*ok[:2], 33, *ok[3:]) == -4 and b"32 layers" in lib.dvh_last_error()
    assert sens(*ok[:6], 17, *ok[7:]) == -4 and b"16 modes" in lib.dvh_last_error()
    assert sens(None, 0, 3, None, 5, None, 4, 15, 1e-9, None, None, None) == 0
    assert sens(None, 2, 3, None, 0, None, 4, 15, 1e-9, None, None, None) == 0
