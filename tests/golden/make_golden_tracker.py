"""Generate the vehicle-tracker fixture by running the REFERENCE's KF_tracking (apis/tracking.py) where the reference
is installed (the same place make_golden.py runs; never on the GPU box):

    python tests/golden/make_golden_tracker.py

detect_in_one_section runs unmodified.  tracking_with_veh_base does not run on current NumPy: the statement on line
105 of apis/tracking.py assigns a ragged list (a one-element array and a number) to a column, which NumPy >= 1.24
rejects.  Its meaning is "the single non-NaN state, then 0".  The method's source is taken at generation time, that one
line (checked to be the assignment to ``Tkk[:, v]``) is replaced by this script's own statement of that meaning, and
the result is compiled in the reference module's namespace.  Nothing is written into the reference tree and only data
leaves this script.

One file per case, tests/golden/tracker_<case>.npz, each under 1 MiB:
  grid            the input grid, float32 multiples of 2**-20 (peaks are positive: this is what KF_tracking gets)
  x_axis, t_axis, start_x, end_x, nx, sigma, sigma_a, minprominence, minseparation, prominenceWindow
  veh_base        detect_in_one_section's return
  peak_erode      the detection curve (the array of detect_in_one_section's last find_peaks call)
  det_peaks, det_counts    find_peaks of the nx detection rows, padded with -1
  row_peaks, row_counts    find_peaks of the tracked rows start_idx, start_idx + 3, ..., padded with -1
  veh_states_raw  [n_veh, n_steps] the matches handed to remove_unrealistic_tracking (every third column of the
                  reference's array, the others are never written)
  tracks          the return of tracking_with_veh_base
  rejected        per vehicle, bit flags of the rejection tests that fired, as this script restates them:
                  1 too few matches, 2 moving backwards, 4 too little net motion, 8 >= 20 adjacent misses
  jumps           per vehicle, the number of matches removed as > 20-sample jumps
Every case is checked to be unchanged under grid * (1 +- 1e-9) and sigma_a * (1 +- 1e-6), and to be free of the order
in which find_peaks' distance rule visits equal heights: SciPy takes that order from an unstable np.argsort, so a row
in which it mattered would pin the sort of the NumPy build that wrote the fixture.  On a 2**-8 grid a quarter of these
rows have such ties (several equal samples on a vehicle's rounded top); 2**-20, still exact in float32, leaves none.
"""
from __future__ import annotations

import inspect
import os
import sys
import textwrap
import warnings

sys.dont_write_bytecode = True

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import import_reference  # noqa: E402
from tests.tracker_ref import distance_order_free  # noqa: E402

REPAIRED_LINE = 105
DETECT = dict(minprominence=0.2, minseparation=50, prominenceWindow=600)
FACTOR = 3
QUANT = 2.0 ** -20

# name -> (rows, samples, start row, end row, cars); a car is (t0, slowness [samples / row], amplitude, width,
# last row it is seen on or None, (row, shift) of a step in its arrival or None)
CASES = {
    "a": (96, 700, 3, 94, [(60, 3.3, 1.0, 8, None, None), (200, 2.5, 0.8, 8, None, None),
                           (330, 4.0, 1.2, 10, None, None), (420, -1.0, 0.9, 8, None, None),
                           (215, 2.5, 0.7, 8, None, None)]),
    "b": (150, 1000, 4, 147, [(60, 2.0, 1.0, 8, None, None), (250, 2.0, 0.9, 8, 70, None),
                              (450, 2.0, 1.1, 8, None, (80, 24)), (650, 2.0, 0.8, 8, 35, None)]),
}


def grid_of(n_x, n_t, cars):
    rng = np.random.default_rng(1)
    d = rng.standard_normal((n_x, n_t)) * 0.02
    t = np.arange(n_t, dtype=np.float64)
    for t0, slow, amp, wid, last, step in cars:
        for r in range(n_x):
            if last is not None and r > last:
                continue
            c = t0 + slow * r + (step[1] if step is not None and r >= step[0] else 0)
            d[r] += amp * np.exp(-0.5 * ((t - c) / wid) ** 2)
    return (np.round(d / QUANT) * QUANT).astype(np.float32)


def repaired_tracking(trk):
    """tracking_with_veh_base with line 105 replaced, compiled in the reference module's namespace."""
    fn = trk.KF_tracking.tracking_with_veh_base
    lines, first = inspect.getsourcelines(fn)
    k = REPAIRED_LINE - first
    old = lines[k]
    assert old.strip().startswith("Tkk[:, v] =") and "isnan" in old, old
    indent = old[:len(old) - len(old.lstrip())]
    lines[k] = indent + "Tkk[:, v] = (np.nanmax(veh_states[v]), 0.0)\n"
    ns = {}
    exec(compile(textwrap.dedent("".join(lines)), "<repaired tracking_with_veh_base>", "exec"), trk.__dict__, ns)
    return ns["tracking_with_veh_base"]


ORIGINAL = {}


class Recorder:
    """Stands in for a function of the reference module: calls it and keeps (first argument, result)."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *a, **k):
        first = np.array(a[1] if self.fn.__name__ == "remove_unrealistic_tracking" else a[0], copy=True)
        out = self.fn(*a, **k)
        self.calls.append((first, out))
        return out


def pad(lists):
    cap = max([len(p) for p in lists] + [1])
    out = np.full((len(lists), cap), -1, np.int32)
    for k, p in enumerate(lists):
        out[k, :len(p)] = p
    return out, np.array([len(p) for p in lists], np.int32)


def run(trk, track_fn, grid, x_axis, t_axis, start_x, end_x, sigma, sigma_a, nx=15):
    fp, rm = Recorder(ORIGINAL["find_peaks"]), Recorder(ORIGINAL["remove_unrealistic_tracking"])
    trk.find_peaks, trk.remove_unrealistic_tracking = fp, rm
    obj = trk.KF_tracking(grid, t_axis, x_axis, {"detect": dict(DETECT)})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        veh_base = obj.detect_in_one_section(start_x=start_x, nx=nx, sigma=sigma)
        n_det = len(fp.calls)
        assert n_det == nx + 1
        tracks = track_fn(obj, start_x=start_x, end_x=end_x, veh_base=veh_base, sigma_a=sigma_a)
    det = [c[1][0] for c in fp.calls[:nx]]
    rows = [c[1][0] for c in fp.calls[n_det:]]
    assert len(rm.calls) == 1
    raw = rm.calls[0][0][:, ::FACTOR]
    assert np.isnan(np.delete(rm.calls[0][0], np.s_[::FACTOR], axis=1)).all()
    return dict(veh_base=np.asarray(veh_base, np.int64), peak_erode=fp.calls[nx][0], det=det, rows=rows,
                veh_states_raw=raw, tracks=tracks)


def judge(raw):
    """The rejection tests and the jump count per vehicle, restated (flags as in the module docstring)."""
    n = raw.shape[1]
    flags, jumps = [], []
    for s in raw:
        m = s[~np.isnan(s)]
        d = np.diff(m)
        f = 1 if len(m) < 0.3 * n else 0
        if len(d) and (np.convolve(d, np.ones(20), "valid") <= -15).any():
            f |= 2
        if abs(d.sum()) < 30 * (len(m) / n):
            f |= 4
        if np.sum(np.diff(np.flatnonzero(np.isnan(s))) == 1) >= 20:
            f |= 8
        flags.append(f)
        jumps.append(int((np.abs(d) > 20).sum()))
    return np.array(flags, np.int32), np.array(jumps, np.int32)


def assert_order_free(row, distance):
    assert distance_order_free(row, distance), "equal heights decide this row"


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)
               for k in ("veh_base", "veh_states_raw", "tracks")) and \
        all(np.array_equal(p, q) for p, q in zip(a["rows"] + a["det"], b["rows"] + b["det"]))


def main():
    import_reference()
    import apis.tracking as trk
    track_fn = repaired_tracking(trk)
    ORIGINAL.update(find_peaks=trk.find_peaks, remove_unrealistic_tracking=trk.remove_unrealistic_tracking)
    meta = np.array(repr(dict(numpy=np.__version__, scipy=scipy.__version__)))
    seen = dict(lost=False, jump=False, short=False, ragged=False)
    for name, (n_x, n_t, i0, i1, cars) in CASES.items():
        q = grid_of(n_x, n_t, cars)
        grid = q.astype(np.float64)
        assert np.array_equal(grid / QUANT, np.round(grid / QUANT))
        x_axis = np.arange(n_x) + 16.32
        t_axis = np.arange(n_t) * 0.02
        kw = dict(x_axis=x_axis, t_axis=t_axis, start_x=x_axis[i0], end_x=x_axis[i1], sigma=0.08)
        res = run(trk, track_fn, grid, sigma_a=0.01, **kw)
        for scale in (1 + 1e-9, 1 - 1e-9):
            assert same(res, run(trk, track_fn, grid * scale, sigma_a=0.01, **kw)), (name, "grid", scale)
        for scale in (1 + 1e-6, 1 - 1e-6):
            assert same(res, run(trk, track_fn, grid, sigma_a=0.01 * scale, **kw)), (name, "sigma_a", scale)
        for r in list(range(i0, i0 + 15)) + list(range(i0, i1 + 1, FACTOR)):
            assert_order_free(grid[r], DETECT["minseparation"])
        assert_order_free(res["peak_erode"], DETECT["minseparation"])
        flags, jumps = judge(res["veh_states_raw"])
        n_steps = res["veh_states_raw"].shape[1]
        assert n_steps == -(-(i1 - i0 + 1) // FACTOR) and len(res["rows"]) == n_steps
        assert res["tracks"].shape == (int((flags == 0).sum()), n_steps * FACTOR), (flags, res["tracks"].shape)
        seen["lost"] |= bool((flags & 8).any())
        seen["short"] |= bool((flags & 1).any())
        seen["jump"] |= bool(((flags == 0) & (jumps > 0)).any())
        seen["ragged"] |= (i1 - i0 + 1) % FACTOR != 0
        det_peaks, det_counts = pad(res["det"])
        row_peaks, row_counts = pad(res["rows"])
        out = dict(grid=q, x_axis=x_axis, t_axis=t_axis, start_x=np.array(x_axis[i0]), end_x=np.array(x_axis[i1]),
                   nx=np.array(15), sigma=np.array(0.08), sigma_a=np.array(0.01),
                   minprominence=np.array(DETECT["minprominence"]), minseparation=np.array(DETECT["minseparation"]),
                   prominenceWindow=np.array(DETECT["prominenceWindow"]), veh_base=res["veh_base"],
                   peak_erode=res["peak_erode"], det_peaks=det_peaks, det_counts=det_counts, row_peaks=row_peaks,
                   row_counts=row_counts, veh_states_raw=res["veh_states_raw"], tracks=res["tracks"],
                   rejected=flags, jumps=jumps, meta=meta)
        path = os.path.join(HERE, f"tracker_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}: {os.path.getsize(path) / 2 ** 20:.2f} MiB; veh_base {res['veh_base']}, rejected {flags}, "
              f"jumps {jumps}, tracks {res['tracks'].shape}, NaN left {int(np.isnan(res['tracks']).sum())}")
        assert os.path.getsize(path) < 2 ** 20
    assert all(seen.values()), seen


if __name__ == "__main__":
    main()
