"""Oracle of the Rayleigh sensitivity kernels and group velocity: derivatives of the 80-digit Thomson-Haskell secular
function of tests/rayleigh_ref.py at its recorded roots, and the generator of tests/golden/rayleigh_sens.npz.

At a root c of D(c, omega, layers):  dc/dp = -D_p / D_c for a layer value p (h, alpha, beta, rho) and
dc/domega = -D_omega / D_c.  Every recorded root is bisected again to 1e-60 and D_c, D_omega and every D_p are
central differences of the 80-digit function at a relative step of 1e-25 (truncation 1e-50, rounding 1e-55
relative).  The secular function is written again here over mpf layer values (rayleigh_ref.secular rounds the layers
to float64, which a step of 1e-25 cannot move); nothing here shares code with the library.

Recorded: every case of rayleigh_ref.CASES at its five frequencies for the first min(n_roots, 5) modes, and a
"grazing" case, the lvz layers at the frequency where mode 1's root sits 5e-6 relative above a layer's beta (found by
bisection in omega), modes 0 and 1: there nu_b^2 h^2 of that layer is about 1e-5 at a root, on the power-series branch
of cosh_sinhc and of its derivative.

    python -m tests.rayleigh_sens_ref        regenerates tests/golden/rayleigh_sens.npz (minutes)
"""
import multiprocessing
import os

import mpmath as mp
import numpy as np

from tests.rayleigh_ref import CASES, DC, DIGITS, FREQS, _system, bisect, c_min_of, load, roots_of, scan_signs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rayleigh_sens.npz")
MAX_MODES = 5
STEP = mp.mpf("1e-25")
GRAZING_LAYERS = "lvz"
GRAZING_OFFSET = 5e-6   # mode 1's root over the layer's beta, minus one
GRAZING_MODES = 2


def omega_of(freq):
    return 2.0 * np.pi / (1.0 / freq)  # omega as the library forms it from the period


def secular(L, c, w):
    """The secular function over mpf values; L rows of (h, alpha, beta, rho).  Call under mp.workdps(DIGITS)."""
    k = w / c
    _, al, be, rho = L[-1]
    mu = rho * be * be
    na, nb = mp.sqrt(k * k - (w / al) ** 2), mp.sqrt(k * k - (w / be) ** 2)
    t = 2 * k * k - (w / be) ** 2
    Y = mp.matrix([[k, nb], [na, k], [-2 * mu * k * na, -mu * t], [-mu * t, -2 * mu * k * nb]])
    for h, al, be, rho in reversed(L[:-1]):
        Y = mp.expm(-_system(k, w, al, be, rho) * h) * Y
    return Y[2, 0] * Y[3, 1] - Y[3, 0] * Y[2, 1]


def derivatives(layers, omega, root):
    """(c, dc/domega, dc/dp [n_layer][4]) as float64 of the 80-digit values at the root near `root` (a float64)."""
    with mp.workdps(DIGITS):
        c = bisect(layers, omega, root * (1.0 - 1e-13), root * (1.0 + 1e-13), width=mp.mpf("1e-60"))
        w = mp.mpf(omega)
        L = [[mp.mpf(float(x)) for x in row] for row in layers]

        def central(f, x):
            return (f(x * (1 + STEP)) - f(x * (1 - STEP))) / (2 * x * STEP)

        d_c = central(lambda x: secular(L, x, w), c)
        d_w = central(lambda x: secular(L, c, x), w)
        dcdp = np.zeros((len(L), 4))
        for l in range(len(L)):
            for q in range(4):
                if L[l][q] == 0:  # the half-space's h (never read), or a row with h = 0
                    continue

                def moved(x, l=l, q=q):
                    M = [list(row) for row in L]
                    M[l][q] = x
                    return secular(M, c, w)

                dcdp[l, q] = float(-central(moved, L[l][q]) / d_c)
        return float(c), float(-d_w / d_c), dcdp


def _job(job):
    layers, omega, root = job
    return derivatives(layers, omega, root)


def grazing_frequency(recorded):
    """(freq, layer) such that mode 1 of the GRAZING_LAYERS case has its root at beta_layer (1 + GRAZING_OFFSET):
    the first layer and pair of recorded frequencies whose mode-1 roots straddle that velocity, then a bisection in
    omega of the secular function's sign at it."""
    layers = CASES[GRAZING_LAYERS][0]
    for l in range(len(layers) - 1):
        target = float(layers[l, 2]) * (1.0 + GRAZING_OFFSET)
        for i in range(len(FREQS) - 1):
            a, b = recorded[GRAZING_LAYERS, i][1], recorded[GRAZING_LAYERS, i + 1][1]
            if a.size > 1 and b.size > 1 and (a[1] - target) * (b[1] - target) < 0:
                with mp.workdps(DIGITS):
                    L = [[mp.mpf(float(x)) for x in row] for row in layers]
                    lo, hi = mp.mpf(omega_of(FREQS[i])), mp.mpf(omega_of(FREQS[i + 1]))
                    slo = mp.sign(secular(L, mp.mpf(target), lo))
                    assert slo * mp.sign(secular(L, mp.mpf(target), hi)) < 0
                    while hi - lo > mp.mpf("1e-12") * lo:
                        mid = (lo + hi) / 2
                        if mp.sign(secular(L, mp.mpf(target), mid)) == slo:
                            lo = mid
                        else:
                            hi = mid
                    return float((lo + hi) / 2) / (2.0 * np.pi), l
    raise AssertionError("no layer velocity is crossed by mode 1 between two recorded frequencies")


def load_sens():
    """{(case, freq index): (c [n], dcdw [n], dcdp [n][n_layer][4])} for the cases of CASES, and under the key
    "grazing" a dict(freq, layer, c_min, c, dcdw, dcdp) on the GRAZING_LAYERS layers."""
    z = np.load(GOLDEN)
    out = {(name, i): (z[f"{name}_c_{i}"], z[f"{name}_dcdw_{i}"], z[f"{name}_dcdp_{i}"])
           for name in CASES for i in range(len(FREQS))}
    out["grazing"] = dict(freq=float(z["grazing_freq"]), layer=int(z["grazing_layer"]), c_min=c_min_of(GRAZING_LAYERS),
                          c=z["grazing_c"], dcdw=z["grazing_dcdw"], dcdp=z["grazing_dcdp"])
    return out


def generate():
    recorded = load()
    jobs, keys = [], []
    for name, (layers, _) in CASES.items():
        for i, f in enumerate(FREQS):
            for r in recorded[name, i][1][:MAX_MODES]:
                jobs.append((layers, omega_of(f), float(r)))
                keys.append((name, i))
    freq, layer = grazing_frequency(recorded)
    layers = CASES[GRAZING_LAYERS][0]
    s = scan_signs(layers, omega_of(freq), c_min_of(GRAZING_LAYERS))
    roots = roots_of(layers, omega_of(freq), c_min_of(GRAZING_LAYERS), signs=s, which=range(GRAZING_MODES))
    assert abs(roots[1] / layers[layer, 2] - 1.0) <= 1e-5, (freq, layer, roots)
    assert np.diff(roots).min() >= 2.0 * DC
    print("grazing", freq, layer, roots, flush=True)
    for r in roots:
        jobs.append((layers, omega_of(freq), float(r)))
        keys.append("grazing")
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_job, jobs, chunksize=1)
    out = {"grazing_freq": np.float64(freq), "grazing_layer": np.int32(layer)}
    for key in dict.fromkeys(keys):
        mine = [r for k, r in zip(keys, res) if k == key]
        stem = "grazing_{}" if key == "grazing" else f"{key[0]}_{{}}_{key[1]}"
        n_layer = len(layers if key == "grazing" else CASES[key[0]][0])
        out[stem.format("c")] = np.array([m[0] for m in mine])
        out[stem.format("dcdw")] = np.array([m[1] for m in mine])
        out[stem.format("dcdp")] = np.array([m[2] for m in mine]).reshape(len(mine), n_layer, 4)
        print(key, out[stem.format("c")], flush=True)
    for name in CASES:  # a (case, frequency) without roots still has its (empty) entries
        for i in range(len(FREQS)):
            n_layer = len(CASES[name][0])
            out.setdefault(f"{name}_c_{i}", np.zeros(0))
            out.setdefault(f"{name}_dcdw_{i}", np.zeros(0))
            out.setdefault(f"{name}_dcdp_{i}", np.zeros((0, n_layer, 4)))
    return out


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **generate())
