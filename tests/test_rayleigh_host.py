"""The Rayleigh secular function without a GPU: the 80-digit oracle (tests/rayleigh_ref.py) against closed forms and
against tests/golden/rayleigh.npz, the root spacing the scan definition rests on, and dvh_rayleigh_secular_host (the
header the device kernels compile, run on the CPU) against the oracle's signs at every scan point and on both sides of
every recorded root."""
import ctypes
import os

import numpy as np
import pytest

from tests import rayleigh_ref as ref


@pytest.fixture(scope="module")
def lib():
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    return ref.load()


def omega_of(i):
    return 2.0 * np.pi / (1.0 / ref.FREQS[i])


def host_secular(lib, layers, c, omega):
    layers = np.ascontiguousarray(layers, np.float64)
    c = np.ascontiguousarray(np.atleast_1d(c), np.float64)
    out = np.full(c.size, 7.0)
    assert lib.dvh_rayleigh_secular_host(layers.ctypes.data, len(layers), c.ctypes.data, c.size, omega,
                                         out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("nu", [0.25, 0.4375])
def test_oracle_half_space_is_the_rayleigh_cubic(nu):
    layers = ref.make_layers([], [0.3], nu)
    want = 0.3 * ref.rayleigh_cubic(nu)
    for f in (2.5, 25.0):
        got = ref.roots_of(layers, 2.0 * np.pi * f, 0.24)
        assert got.size == 1 and abs(got[0] - want) <= 1e-14 * want, (got, want)
    if nu == 0.4375:
        assert abs(want - 0.28419) < 5e-6


def test_oracle_layer_splitting():
    """One layer is the same layer cut in three: equal to 60 of the 80 digits, at the stack's largest k h."""
    import mpmath as mp
    one = ref.make_layers([2.0 ** -5], [0.2, 0.5])  # dyadic thicknesses: the three add up exactly
    cut = ref.make_layers([2.0 ** -7, 2.0 ** -6, 2.0 ** -7], [0.2, 0.2, 0.2, 0.5])
    for f, c in ((2.5, 0.45), (25.0, 0.17), (25.0, 0.3)):
        a, b = ref.secular(one, c, 2.0 * np.pi * f), ref.secular(cut, c, 2.0 * np.pi * f)
        assert abs(a - b) <= mp.mpf("1e-60") * abs(a), (f, c, a, b)


def test_case_table_matches_the_recorded_file(recorded):
    for name, (layers, _) in ref.CASES.items():
        for i in range(len(ref.FREQS)):
            signs, roots = recorded[name, i]
            assert signs.size == ref.SCAN_POINTS[name] == ref.scan_points(layers, ref.c_min_of(name)).size
            assert roots.size == np.count_nonzero(signs[1:] != signs[:-1])
        assert recorded[name, 4][1].size == ref.ROOTS_25HZ[name]
    assert ref.scan_points(*ref.CASES["dyadic"])[32] == 0.25 == ref.CASES["dyadic"][0][1, 2]


@pytest.mark.parametrize("name,i,which", [("halfspace3", 4, [0]), ("one_layer", 3, [0, 2]), ("notebook", 3, [9]),
                                          ("lvz", 2, [1]), ("dyadic", 4, [2])])
def test_recorded_roots_regenerate(recorded, name, i, which):
    """A subset of the file from the oracle again: signs at a stride of the scan points, and some roots."""
    layers = ref.CASES[name][0]
    signs, roots = recorded[name, i]
    c = ref.scan_points(layers, ref.c_min_of(name))
    import mpmath as mp
    for k in range(0, c.size, 23):
        assert int(mp.sign(ref.secular(layers, float(c[k]), omega_of(i)))) == signs[k]
    got = ref.roots_of(layers, omega_of(i), ref.c_min_of(name), signs=signs, which=which)
    assert np.array_equal(got, roots[which])


def test_recorded_roots_are_two_scan_steps_apart(recorded):
    """What the scan definition rests on: no two roots share a scan interval or sit in neighbouring ones."""
    closest = np.inf
    for (name, i), (_, roots) in recorded.items():
        if roots.size > 1:
            closest = min(closest, np.diff(roots).min())
            assert np.diff(roots).min() >= 2.0 * ref.DC, (name, i, roots)
    print(f"closest pair of recorded roots: {closest / ref.DC:.2f} dc")


def test_host_secular_signs_match_the_oracle(lib, recorded):
    """Finite and of the oracle's sign at every scan point farther than 1e-9 c from a root, and of opposite signs at
    c_ref (1 -+ 1e-9) of every root: with that, a bracket refined to 1e-9 relative holds the oracle's root."""
    for (name, i), (signs, roots) in recorded.items():
        layers = ref.CASES[name][0]
        c = ref.scan_points(layers, ref.c_min_of(name))
        v = host_secular(lib, layers, c, omega_of(i))
        assert np.isfinite(v).all() and np.abs(v).max() <= 1.0 + 1e-12, (name, i)
        far = np.array([roots.size == 0 or np.abs(roots - x).min() > 1e-9 * x for x in c])
        assert far.all()  # no recorded root lies that close to a scan point
        assert np.array_equal(np.where(v < 0, -1, 1)[far], signs[far]), (name, i)
        below, above = (host_secular(lib, layers, roots * (1.0 + s * 1e-9), omega_of(i)) for s in (-1.0, 1.0))
        assert np.all(below * above < 0), (name, i, below, above)
        # the sign below a root is the sign of the scan point before it
        at = np.nonzero(signs[1:] != signs[:-1])[0]
        assert np.array_equal(np.where(below < 0, -1, 1), signs[at])


def test_host_bisection_error(lib, recorded):
    """The roots a float64 bisection of the host entry converges to, against the oracle's: printed for DESIGN.md."""
    worst = 0.0
    for (name, i), (signs, roots) in recorded.items():
        layers = ref.CASES[name][0]
        c = ref.scan_points(layers, ref.c_min_of(name))
        for r, k in zip(roots, np.nonzero(signs[1:] != signs[:-1])[0]):
            lo, hi = c[k], c[k + 1]
            neg = host_secular(lib, layers, lo, omega_of(i))[0] < 0
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                if (host_secular(lib, layers, mid, omega_of(i))[0] < 0) == neg:
                    lo = mid
                else:
                    hi = mid
            worst = max(worst, abs(0.5 * (lo + hi) - r) / r)
    print(f"largest relative root error of the host path: {worst:.2e}")
    assert worst <= 1e-9


def test_host_secular_refusals(lib):
    layers = np.ascontiguousarray(ref.CASES["one_layer"][0])
    c = np.array([0.3, -1.0, 0.0])
    out = np.zeros(3)
    L, C, O = layers.ctypes.data, c.ctypes.data, out.ctypes.data
    f = lib.dvh_rayleigh_secular_host
    assert f(L, 2, C, 3, 10.0, O) == 0 and np.isfinite(out[0]) and np.isnan(out[1:]).all()
    assert f(None, 2, C, 3, 10.0, O) == -2 and f(L, 2, None, 3, 10.0, O) == -2 and f(L, 2, C, 3, 10.0, None) == -2
    assert f(L, 0, C, 3, 10.0, O) == -2 and f(L, 2, C, -1, 10.0, O) == -2
    assert f(L, 2, C, 3, 0.0, O) == -2 and f(L, 2, C, 3, float("nan"), O) == -2
    assert f(L, 33, C, 3, 10.0, O) == -4
    assert f(None, 2, None, 0, 10.0, None) == 0
    bad = layers.copy()
    bad[0, 2] = bad[0, 1]  # beta = alpha
    assert f(bad.ctypes.data, 2, C, 3, 10.0, O) == -2
    assert b"alpha > beta" in lib.dvh_last_error()
    big = np.ascontiguousarray(np.tile(layers[:1], (32, 1)))
    out32 = np.zeros(1)
    assert f(big.ctypes.data, 32, C, 1, 10.0, out32.ctypes.data) == 0 and np.isfinite(out32[0])


def test_device_entries_refuse_before_any_launch(lib):
    """The argument checks of dvh_rayleigh_modes and dvh_curve_misfit return before a device is touched."""
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused or empty
    modes = lambda *a: lib.dvh_rayleigh_modes(*a, None)
    ok = (p, 2, 3, p, 5, p, 0.1, 0.005, 1e-9, 4, p, p)
    for at in (0, 3, 5, 10, 11):
        assert modes(*ok[:at], None, *ok[at + 1:]) == -2, at
    for at, bad in ((1, -1), (2, 0), (4, -1), (9, 0), (6, 0.0), (6, float("nan")), (7, 0.0), (7, -1.0), (8, 0.0),
                    (8, float("inf"))):
        assert modes(*ok[:at], bad, *ok[at + 1:]) == -2, (at, bad)
    assert modes(*ok[:2], 33, *ok[3:]) == -4 and b"32 layers" in lib.dvh_last_error()
    assert modes(*ok[:9], 17, *ok[10:]) == -4 and b"16 modes" in lib.dvh_last_error()
    assert modes(None, 0, 3, None, 5, None, 0.1, 0.005, 1e-9, 4, None, None) == 0
    assert modes(None, 2, 3, None, 0, None, 0.1, 0.005, 1e-9, 4, None, None) == 0
    misfit = lambda *a: lib.dvh_curve_misfit(*a, None)
    ok = (p, 2, 5, 4, p, p, p, p, p, 7, p, 2, p)
    for at in (0, 4, 5, 6, 7, 8, 10, 12):
        assert misfit(*ok[:at], None, *ok[at + 1:]) == -2, at
    for at, bad in ((1, -1), (2, 0), (3, 0), (9, 0), (11, 0)):
        assert misfit(*ok[:at], bad, *ok[at + 1:]) == -2, (at, bad)
    assert misfit(None, 0, 5, 4, None, None, None, None, None, 7, None, 2, None) == 0
