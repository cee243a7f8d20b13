"""Generate the phase-shift dispersion fixture by running the REFERENCE's map_fv_FD_slant_stack (modules/utils.py:429-454)
where the reference is installed (the same place make_golden.py runs; never on the GPU box):

    python tests/golden/make_golden_slant.py

Only data leaves this script, tests/golden/slant.npz (under 1 MiB).  Per case X of CASES:
  X_q         the gather, int16, value = q * 2**-8 (exact in float32): plane waves of a few frequencies and velocities
              under a moving envelope plus noise
  X_dx, X_dt, X_freqs, X_vels, X_norm    the call's arguments
  X_out       what the reference returned: float64 [nV, nF]  (case F: X_out for norm=True, X_out_plain for norm=False)
  X_nf, X_fidx, X_bins, X_rows           nf, argmin |f - fftfreq(nf, dt)| per frequency (the reference's expression,
              evaluated here), its sorted unique values, and (row0, n_row) of data[6:25]
  X_ratio     condition (a): max_f sum_ix |D[ix, f]| / max |image|
  X_ties      condition (b): the share of frequency columns with a runner-up within 2e-6 max|image| of the maximum
  X_seed      the first noise seed at which (a) <= 8 and (b) <= 0.1 hold (multi-row cases with a finite image; a
              one-row gather ties in every column and is exempt from (b))
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import slant_ref  # noqa: E402
from tests.golden.make_golden import import_reference  # noqa: E402

QUANT = 2.0 ** -8
DX = 8.16
DT500, DT499 = 0.003999999999997783, 0.004000000000001336

CASES = {
    # 19 rows, the notebook geometry
    "A": dict(nch=25, nt=500, dt=DT500, norm=True, freqs=np.arange(0.8, 25, 0.8), vels=np.arange(200, 1200, 37.)),
    # odd length, descending velocities: the caller's row order is kept
    "B": dict(nch=25, nt=499, dt=DT499, norm=False, freqs=np.linspace(1.0, 30.0, 33), vels=np.linspace(1100., 250., 17)),
    # one row: the image is constant over v
    "C": dict(nch=7, nt=64, dt=0.004, norm=True, freqs=np.array([3.0, 11.0]), vels=np.array([300., -450., 800.])),
    # 14 rows; negative, above-Nyquist and exact halfway frequencies (nf = 1 024, bins 0.244140625 Hz apart)
    "D": dict(nch=20, nt=257, dt=0.004, norm=True, freqs=np.append(np.linspace(-5.0, 140.0, 21), 1.5869140625),
              vels=np.arange(150., 900., 50.)),
    # rows past 25 ignored; 65 x 130 pairs: tiles straddle 64 and 128 lanes, partial last tiles
    "E": dict(nch=40, nt=500, dt=0.004, norm=True, freqs=np.linspace(0.8, 24.8, 65), vels=np.linspace(200., 1199., 130)),
    # empty slice: all zeros, with and without norm
    "F": dict(nch=5, nt=100, dt=0.004, norm=True, freqs=np.linspace(2.0, 20.0, 5), vels=np.array([250., 400., 600., 900.])),
    # a zero row under norm: all NaN
    "G": dict(nch=25, nt=64, dt=0.004, norm=True, freqs=np.array([5.0, 12.0]), vels=np.array([300., 600.]),
              zero_row=10),
}


def gather_of(seed, nch, nt, dt):
    rng = np.random.default_rng(seed)
    t = np.arange(nt) * dt
    x = 0.6 * rng.standard_normal((nch, nt))
    for f, c in ((4.0, 310.0), (9.0, 420.0), (15.0, 560.0), (21.0, 700.0)):
        for r in range(nch):
            delay = r * DX / c
            x[r] += 4.0 * np.exp(-0.5 * ((t - 0.3 * nt * dt - delay) / (0.12 * nt * dt)) ** 2) * \
                np.cos(2 * np.pi * f * (t - delay) + 0.7 * f)
    return np.round(x / QUANT).astype(np.int16)


def main():
    ref = import_reference()
    out = dict(meta=np.array(repr(dict(numpy=np.__version__, scipy=scipy.__version__))))
    for name, c in CASES.items():
        multi = min(c["nch"], 25) - 6 > 1 and "zero_row" not in c
        for seed in range(100):
            q = gather_of(1000 + 17 * seed + ord(name), c["nch"], c["nt"], c["dt"])
            if "zero_row" in c:
                q[c["zero_row"]] = 0
            data = q.astype(np.float64) * QUANT
            with np.errstate(all="ignore"):
                img = ref.ut.map_fv_FD_slant_stack(data, DX, c["dt"], c["freqs"], c["vels"], norm=c["norm"])
            if not multi:
                break
            ratio = slant_ref.coherence_ratio(data, c["dt"], c["freqs"], img, norm=c["norm"])
            ties = slant_ref.near_tie_fraction(img)
            if ratio <= 8 and ties <= 0.1:
                break
        else:
            raise AssertionError(f"case {name}: no seed meets conditions (a) and (b)")
        assert img.dtype == np.float64 and img.shape == (c["vels"].size, c["freqs"].size)
        nf, fidx = slant_ref.bins(c["nt"], c["dt"], c["freqs"])
        row0, stop, _ = slice(6, 25).indices(c["nch"])
        finite = bool(np.isfinite(img).all()) and img.max() > 0
        ratio = slant_ref.coherence_ratio(data, c["dt"], c["freqs"], img, norm=c["norm"]) if finite else np.nan
        ties = slant_ref.near_tie_fraction(img) if finite else np.nan
        out.update({f"{name}_q": q, f"{name}_dx": np.array(DX), f"{name}_dt": np.array(c["dt"]),
                    f"{name}_freqs": c["freqs"], f"{name}_vels": c["vels"], f"{name}_norm": np.array(c["norm"]),
                    f"{name}_out": img, f"{name}_nf": np.array(nf), f"{name}_fidx": fidx, f"{name}_bins": np.unique(fidx),
                    f"{name}_rows": np.array([row0, max(0, stop - row0)]), f"{name}_ratio": np.array(ratio),
                    f"{name}_ties": np.array(ties), f"{name}_seed": np.array(seed)})
        if name == "F":
            out["F_out_plain"] = ref.ut.map_fv_FD_slant_stack(data, DX, c["dt"], c["freqs"], c["vels"], norm=False)
        print(f"case {name}: seed {seed}, image {img.shape}, nf {nf}, rows {out[f'{name}_rows']}, "
              f"ratio {ratio:.2f}, near-tie columns {ties:.3f}")
    path = os.path.join(HERE, "slant.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 2 ** 20:.2f} MiB")
    assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
