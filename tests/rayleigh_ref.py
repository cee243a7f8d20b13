"""Oracle of the Rayleigh forward model: Thomson-Haskell at 80 digits with mpmath, the case table of the Rayleigh
tests, a NumPy restatement of dvh_curve_misfit, and the generator of tests/golden/rayleigh.npz.

The secular function is the one das_diff_veh_amd/csrc/rayleigh.h defines: the two solutions of Aki & Richards'
eq. 7.28 system dr/dz = A r, r = (r1, r2, r3, r4), that decay in the half-space, started as the potentials' vectors
(k, nu_a, -2 mu k nu_a, -mu t) and (nu_b, k, -mu t, -2 mu k nu_b), t = 2 k^2 - omega^2 / beta^2, carried to the free
surface by expm(-A h) of every layer (no stabilisation: 80 digits outlast k h = 125), and there the minor of the two
traction rows.  Nothing here shares code with the library.

    python -m tests.rayleigh_ref        regenerates tests/golden/rayleigh.npz (minutes)
"""
import os

import mpmath as mp
import numpy as np

DIGITS = 80
NU = 0.4375
DC = 2.0 ** -8
FREQS = (2.5, 5.0, 10.0, 16.0, 25.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rayleigh.npz")


def vp_of(vs, nu=NU):
    vs = np.asarray(vs, np.float64)
    return vs * np.sqrt((2.0 - 2.0 * nu) / (1.0 - 2.0 * nu))


def density_of(vp):
    return 1.56 + 0.186 * vp


def make_layers(h, vs, nu=NU):
    """[n][4] float64 rows (h, vp, vs, rho); h has one entry fewer than vs (the half-space gets 0)."""
    vs = np.asarray(vs, np.float64)
    vp = vp_of(vs, nu)
    return np.stack([np.r_[np.asarray(h, np.float64), 0.0], vp, vs, density_of(vp)], axis=1)


# name -> (layers, c_min); c_min is the forward call's default 0.8 min(beta) unless the case names one
CASES = {
    "halfspace1": (make_layers([], [0.3]), None),
    "halfspace3": (make_layers([0.01, 0.02], [0.3, 0.3, 0.3]), None),
    "one_layer": (make_layers([0.01], [0.2, 0.5]), None),
    "notebook": (make_layers([0.008, 0.008, 0.015, 0.015, 0.05], [0.15, 0.22, 0.3, 0.42, 0.6, 0.9]), None),
    "lvz": (make_layers([0.006, 0.01, 0.03], [0.3, 0.18, 0.45, 0.8]), None),
    "dyadic": (make_layers([2.0 ** -7, 2.0 ** -6], [0.15625, 0.25, 0.5]), 0.125),
}
SCAN_POINTS = {"halfspace1": 16, "halfspace3": 16, "one_layer": 88, "notebook": 200, "lvz": 168, "dyadic": 96}
ROOTS_25HZ = {"halfspace1": 1, "halfspace3": 1, "one_layer": 3, "notebook": 14, "lvz": 8, "dyadic": 6}


def c_min_of(name):
    layers, c_min = CASES[name]
    return float(0.8 * layers[:, 2].min()) if c_min is None else c_min


def scan_points(layers, c_min, dc=DC):
    """c_k = fma(k, dc, c_min) below the half-space beta (k dc is exact for the dyadic dc of the tests)."""
    n = int(np.ceil((layers[-1, 2] - c_min) / dc)) + 2
    c = c_min + np.arange(n) * dc
    return c[c < layers[-1, 2]]


def _system(k, w, al, be, rho):
    mu = rho * be * be
    lam = rho * al * al - 2 * mu
    l2m = lam + 2 * mu
    zeta = 4 * mu * (lam + mu) / l2m
    return mp.matrix([[0, k, 1 / mu, 0],
                      [-k * lam / l2m, 0, 0, 1 / l2m],
                      [k * k * zeta - w * w * rho, 0, 0, k * lam / l2m],
                      [0, -w * w * rho, -k, 0]])


def secular(layers, c, omega, digits=DIGITS):
    """The secular function at `digits` digits (an mpf); layers float64 [n][4], c a float or mpf."""
    with mp.workdps(digits):
        c, w = mp.mpf(c), mp.mpf(omega)
        k = w / c
        L = [[mp.mpf(float(x)) for x in row] for row in layers]
        _, al, be, rho = L[-1]
        mu = rho * be * be
        na, nb = mp.sqrt(k * k - (w / al) ** 2), mp.sqrt(k * k - (w / be) ** 2)
        t = 2 * k * k - (w / be) ** 2
        Y = mp.matrix([[k, nb], [na, k], [-2 * mu * k * na, -mu * t], [-mu * t, -2 * mu * k * nb]])
        for h, al, be, rho in reversed(L[:-1]):
            Y = mp.expm(-_system(k, w, al, be, rho) * h) * Y
        return Y[2, 0] * Y[3, 1] - Y[3, 0] * Y[2, 1]


def bisect(layers, omega, lo, hi, width=mp.mpf("1e-25"), digits=DIGITS):
    """The root in (lo, hi), which must bracket a sign change, to `width`."""
    with mp.workdps(digits):
        lo, hi = mp.mpf(lo), mp.mpf(hi)
        slo = mp.sign(secular(layers, lo, omega, digits))
        assert slo * mp.sign(secular(layers, hi, omega, digits)) < 0
        while hi - lo > width:
            mid = (lo + hi) / 2
            if mp.sign(secular(layers, mid, omega, digits)) == slo:
                lo = mid
            else:
                hi = mid
        return (lo + hi) / 2


def scan_signs(layers, omega, c_min, dc=DC, digits=DIGITS):
    """The oracle's sign (+1 / -1) at every scan point."""
    return np.array([int(mp.sign(secular(layers, float(c), omega, digits))) for c in scan_points(layers, c_min, dc)],
                    np.int8)


def roots_of(layers, omega, c_min, dc=DC, signs=None, which=None):
    """Every root the scan at dc brackets (or those of the bracket numbers in `which`), as float64 of the 80-digit
    value."""
    c = scan_points(layers, c_min, dc)
    s = scan_signs(layers, omega, c_min, dc) if signs is None else signs
    at = np.nonzero(s[1:] != s[:-1])[0]
    if which is not None:
        at = at[list(which)]
    return np.array([float(bisect(layers, omega, float(c[i]), float(c[i + 1]))) for i in at])


def rayleigh_cubic(nu):
    """c_R / beta of a homogeneous half-space: the root in (0, 1) of x^3 - 8 x^2 + 8 (3 - 2 g) x - 16 (1 - g) = 0,
    x = (c / beta)^2, g = (beta / alpha)^2."""
    with mp.workdps(50):
        nu = mp.mpf(nu)
        g = (1 - 2 * nu) / (2 - 2 * nu)
        r = [x.real for x in mp.polyroots([1, -8, 8 * (3 - 2 * g), -16 * (1 - g)], maxsteps=200, extraprec=200)
             if abs(x.imag) < mp.mpf("1e-30") and 0 < x.real < 1]
        assert len(r) == 1
        return float(mp.sqrt(r[0]))


def curve_misfit(c, sample_period, sample_mode, sample_obs, sample_sigma, sample_curve, curve_weight):
    """dvh_curve_misfit restated: c [M][P][n_mode] -> [M]; the sums run over the samples in table order."""
    c = np.asarray(c, np.float64)
    out = np.empty(c.shape[0])
    for m in range(c.shape[0]):
        num = den = 0.0
        for i, w in enumerate(curve_weight):
            acc, n = 0.0, 0
            for j in range(len(sample_obs)):
                if sample_curve[j] == i:
                    r = (sample_obs[j] - c[m, sample_period[j], sample_mode[j]]) / sample_sigma[j]
                    acc += r * r
                    n += 1
            num += w * np.sqrt(acc / n)
            den += w
        out[m] = num / den
    out[np.isnan(out)] = np.inf
    return out


def load():
    """{(case, freq index): (signs int8 [n_scan], roots float64 [n_root])} of the recorded file."""
    z = np.load(GOLDEN)
    return {(name, i): (z[f"{name}_signs_{i}"], z[f"{name}_roots_{i}"]) for name in CASES for i in range(len(FREQS))}


def generate():
    out = {}
    for name, (layers, _) in CASES.items():
        for i, f in enumerate(FREQS):
            w = 2.0 * np.pi / (1.0 / f)  # omega as the library forms it from the period
            s = scan_signs(layers, w, c_min_of(name))
            out[f"{name}_signs_{i}"] = s
            out[f"{name}_roots_{i}"] = roots_of(layers, w, c_min_of(name), signs=s)
            print(name, f, s.size, out[f"{name}_roots_{i}"], flush=True)
    return out


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **generate())
