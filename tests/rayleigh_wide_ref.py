"""The wide case table of the Rayleigh tests and the generator of tests/golden/rayleigh_wide.npz: the swarm's search
space beyond tests/rayleigh_ref.py's table (Poisson's ratio 0.05 .. 0.49 and mixed, 32 rows, a stiff cap, a half-space
ten times faster than the top, k h up to 196 in one layer and a layer whose sublayer count is clamped), scanned at
dc = 2^-8 by the same oracle at as many digits as the unstabilised expm needs.

    python -m tests.rayleigh_wide_ref        regenerates tests/golden/rayleigh_wide.npz (minutes, at most 16 processes)
"""
import multiprocessing
import os

import mpmath as mp
import numpy as np

from tests import rayleigh_ref as ref

DC = ref.DC
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rayleigh_wide.npz")
MAX_ROOTS = 16                # the brackets the kernel can return
CLAMPED_ROOTS = 4             # of `clamped`, whose oracle costs half a second an evaluation
CLAMPED_WIDTH = 1e-18         # and its bisection width, relative

NB_H = [0.008, 0.008, 0.015, 0.015, 0.05]
NB_VS = [0.15, 0.22, 0.3, 0.42, 0.6, 0.9]
MIXED_NU = np.array([0.2, 0.4, 0.25, 0.35, 0.3, 0.22])

# name -> (layers, frequencies Hz, c_min, oracle digits)
CASES = {
    "nu005": (ref.make_layers(NB_H, NB_VS, 0.05), (5.0, 25.0), 0.12, 200),
    "nu02": (ref.make_layers(NB_H, NB_VS, 0.2), (5.0, 25.0), 0.12, 200),
    "nu03": (ref.make_layers(NB_H, NB_VS, 0.3), (5.0, 25.0), 0.12, 200),
    "nu049": (ref.make_layers(NB_H, NB_VS, 0.49), (5.0, 25.0), 0.12, 200),
    "mixed_nu": (ref.make_layers(NB_H, NB_VS, MIXED_NU), (25.0,), 0.12, 200),
    "thick": (ref.make_layers([0.1], [0.2, 0.5], 0.3), (50.0,), 0.16, 320),
    "gradient32": (ref.make_layers([0.004] * 31, np.linspace(0.15, 0.9, 32), 0.3), (25.0,), 0.12, 260),
    "contrast": (ref.make_layers([0.01, 0.02], [0.1, 0.3, 3.0], 0.25), (10.0,), 0.08, 110),
    "cap": (ref.make_layers([0.005, 0.02], [0.8, 0.2, 0.9], 0.25), (25.0,), 0.16, 110),
    "clamped": (ref.make_layers([1.0], [0.2, 0.5], 0.3), (80.0,), 0.16, 2900),
}
SIX_ROW = ("nu005", "nu02", "nu03", "nu049", "mixed_nu")  # the cases that share NB_H / NB_VS: one batch
SCAN_POINTS = {"nu005": 200, "nu02": 200, "nu03": 200, "nu049": 200, "mixed_nu": 200, "thick": 88, "gradient32": 200,
               "contrast": 748, "cap": 190, "clamped": 88}


def omega_of(f):
    return 2.0 * np.pi / (1.0 / f)  # omega as the library forms it from the period


def keys():
    return [(name, i) for name, case in CASES.items() for i in range(len(case[1]))]


def digits_needed(name):
    """80 digits and the 0.87 k sum(h) that expm(-A h) without stabilisation loses, at the case's largest k."""
    layers, freqs, c_min, _ = CASES[name]
    return 80.0 + 0.87 * omega_of(max(freqs)) / c_min * layers[:-1, 0].sum()


def n_recorded(name):
    return CLAMPED_ROOTS if name == "clamped" else MAX_ROOTS


def sign_at(name, i, k):
    layers, freqs, c_min, digits = CASES[name]
    c = ref.scan_points(layers, c_min, DC)[k]
    return int(mp.sign(ref.secular(layers, float(c), omega_of(freqs[i]), digits)))


def section(lo, hi, neg_at):
    """One step of dvh_rayleigh_modes' refinement, which is part of the definition where a bracket holds three roots
    or more (`thick` has one such bracket, `clamped` many, of up to 19 roots): the 64 points that cut (lo, hi) into 65
    equal parts are taken, and the first of them whose sign differs from lo's closes the new bracket.  neg_at(points)
    gives `D < 0` as a bool array.  -> (lo, hi) of the new bracket."""
    w = (hi - lo) / 65.0
    pts = lo + np.arange(1, 65) * w
    diff = np.asarray(neg_at(pts)) != np.asarray(neg_at(np.array([lo])))[0]
    if not diff.any():
        return float(pts[63]), hi
    j = int(np.argmax(diff))
    return (lo if j == 0 else float(pts[j - 1])), float(pts[j])


def root_at(name, i, k):
    """The root between scan points k and k + 1 that the definition returns (the lowest the first sectioning step
    separates), as the float64 of the oracle's value."""
    layers, freqs, c_min, digits = CASES[name]
    c = ref.scan_points(layers, c_min, DC)
    omega = omega_of(freqs[i])
    lo, hi = section(float(c[k]), float(c[k + 1]),
                     lambda pts: [mp.sign(ref.secular(layers, float(x), omega, digits)) < 0 for x in pts])
    width = mp.mpf(CLAMPED_WIDTH) * mp.mpf(lo) if name == "clamped" else mp.mpf("1e-25")
    return float(ref.bisect(layers, omega, lo, hi, width, digits))


def brackets(signs):
    return np.nonzero(signs[1:] != signs[:-1])[0]


def _sign_job(job):
    return sign_at(*job)


def _root_job(job):
    return root_at(*job)


def load():
    """{(case, freq index): (signs int8 [n_scan], roots float64 [min(brackets, 16); 4 for clamped])}"""
    z = np.load(GOLDEN)
    return {(name, i): (z[f"{name}_signs_{i}"], z[f"{name}_roots_{i}"]) for name, i in keys()}


def generate():
    # the dearest jobs first: the pool stays busy to the end
    order = sorted(keys(), key=lambda key: -CASES[key[0]][3] * len(CASES[key[0]][0]))
    out = {}
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        jobs = [(name, i, k) for name, i in order for k in range(SCAN_POINTS[name])]
        res = pool.map(_sign_job, jobs, chunksize=1)
        for name, i in order:
            out[f"{name}_signs_{i}"] = np.array([s for j, s in zip(jobs, res) if j[:2] == (name, i)], np.int8)
        jobs = [(name, i, int(k)) for name, i in order for k in brackets(out[f"{name}_signs_{i}"])[:n_recorded(name)]]
        res = pool.map(_root_job, jobs, chunksize=1)
        for name, i in order:
            out[f"{name}_roots_{i}"] = np.array([r for j, r in zip(jobs, res) if j[:2] == (name, i)], np.float64)
            print(name, CASES[name][1][i], brackets(out[f"{name}_signs_{i}"]).size, out[f"{name}_roots_{i}"],
                  flush=True)
    return {f"{name}_{what}_{i}": out[f"{name}_{what}_{i}"] for name, i in keys() for what in ("signs", "roots")}


if __name__ == "__main__":
    for name_ in CASES:
        assert CASES[name_][3] >= digits_needed(name_), name_
        assert ref.scan_points(CASES[name_][0], CASES[name_][2], DC).size == SCAN_POINTS[name_], name_
    np.savez_compressed(GOLDEN, **generate())
