"""Generate tests/golden/classes.npz by running the REFERENCE's own notebook cells where the reference is installed
(the same place make_golden.py runs; never on the GPU box):

    python tests/golden/make_golden_classes.py [--reference DIR]

The class split lives only in notebook cells (imaging_diff_speed.ipynb cells 5, 6, 8, 9, 11 and
imaging_diff_weight.ipynb cells 5, 7, 8, 9, 11).  The cells' sources are read from the notebooks' JSON at generation
time and executed as they are, in a namespace holding seeded synthetic ``das_veh_states`` / ``veh_speed`` /
``windows_all``, with matplotlib on the Agg backend, ``savefig`` / ``plot`` / ``fill_between`` stubbed (cell 11 draws against a fixed
1 500-sample axis) and a temporary working directory.  Nothing
of the cell text is kept: only the arrays the cells leave behind.

Inputs: N_PASS passes x 5 channels x 160 samples, multiples of 2**-8 stored as int16 (``q``; exact in float32, which is
how the tests load them; the cells get them as float64).  Each pass is a trough of log-normal depth under the vehicle
plus white noise and a linear drift; ``veh_speed`` is normal around 25 m/s.

Keys: q, veh_speed; from the speed notebook s_mean (das_veh_states_mean), s_peaks, s_mode_peak, s_sigma, s_lower,
s_upper, s_peak_idx, s_threshold_1, s_threshold_2, s_fast_idx, s_mid_idx, s_slow_idx, s_mean_{slow,mid,fast},
s_std_slow; from the weight notebook w_lower, w_upper, w_speed_idx, w_mean, w_peaks, w_mode_peak, w_heavy_idx, w_mid_idx,
w_light_idx, w_mean_{light,mid,heavy}, w_std_{light,mid,heavy}.

The generator asserts what lets the tests demand identical index arrays from peaks that differ in the last bits:
every class is non-empty, each histogram's fullest bin leads the next by at least 2 counts, and no peak or speed lies
within 1e-9 max of a threshold or a bin edge (apart from the minimum and maximum, which are bin edges by construction).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.make_golden import REF  # noqa: E402  (where the reference is installed)

N_PASS, N_CH, N_T, SEED = 300, 5, 160, 20234
SPEED_CELLS = (5, 6, 8, 9, 11)
WEIGHT_CELLS = (5, 7, 8, 9, 11)


def synthetic(seed=SEED):
    rng = np.random.default_rng(seed)
    t = np.arange(N_T)
    depth = rng.lognormal(mean=0.75, sigma=0.55, size=N_PASS)
    centre = N_T / 2 + rng.uniform(-6, 6, N_PASS)
    width = rng.uniform(9, 14, N_PASS)
    trough = -depth[:, None] * np.exp(-((t[None, :] - centre[:, None]) / width[:, None]) ** 2)
    drift = rng.uniform(-0.3, 0.3, (N_PASS, N_CH, 1)) * (t / N_T) + rng.uniform(-0.2, 0.2, (N_PASS, N_CH, 1))
    x = trough[:, None, :] * rng.uniform(0.9, 1.1, (N_PASS, N_CH, 1)) + drift + 0.05 * rng.standard_normal(
        (N_PASS, N_CH, N_T))
    q = np.round(x * 2 ** 8).astype(np.int16)
    return q, rng.normal(25.0, 4.0, N_PASS)


def run_cells(notebook, cells, ns):
    """Execute the code cells ``cells`` of ``notebook`` in ``ns``, in order."""
    with open(notebook) as fh:
        nb = json.load(fh)
    for k in cells:
        cell = nb["cells"][k]
        assert cell["cell_type"] == "code", (notebook, k)
        exec(compile("".join(cell["source"]), f"{os.path.basename(notebook)}#cell{k}", "exec"), ns)
    return ns


def namespace(q, veh_speed):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from scipy import signal
    # drawing only: cell 11 plots against the notebooks' 1 500-sample time axis, which these 160-sample curves do not fit
    plt.savefig = plt.plot = plt.fill_between = lambda *a, **k: None
    states = [q[i].astype(np.float32).astype(np.float64) / 2 ** 8 for i in range(q.shape[0])]
    return dict(np=np, plt=plt, signal=signal, das_veh_states=states, veh_speed=np.array(veh_speed),
                windows_all=list(range(q.shape[0])), _x0=700)


def clear_of(values, marks, what, skip_extremes=False):
    """No value within 1e-9 max|values| of a mark (the minimum and maximum excepted for bin edges)."""
    values = np.asarray(values, dtype=np.float64)
    marks = np.atleast_1d(np.asarray(marks, dtype=np.float64))
    v = np.sort(values)[1:-1] if skip_extremes else values
    gap = np.abs(v[:, None] - marks[None, :]).min()
    assert gap > 1e-9 * np.abs(values).max(), (what, gap)


def lead(peaks):
    hist = np.sort(np.histogram(peaks, bins=100)[0])
    return int(hist[-1] - hist[-2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REF)
    ap.add_argument("--out", default=os.path.join(HERE, "classes.npz"))
    args = ap.parse_args()
    q, veh_speed = synthetic()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            s = run_cells(os.path.join(args.reference, "imaging_diff_speed.ipynb"), SPEED_CELLS, namespace(q, veh_speed))
            w = run_cells(os.path.join(args.reference, "imaging_diff_weight.ipynb"), WEIGHT_CELLS,
                          namespace(q, veh_speed))
        finally:
            os.chdir(cwd)
    out = dict(q=q, veh_speed=veh_speed,
               s_mean=np.array(s["das_veh_states_mean"]), s_peaks=s["peaks"], s_mode_peak=s["mode_peak"],
               s_sigma=s["sigma"], s_lower=s["lower_limit"], s_upper=s["upper_limit"], s_peak_idx=s["peak_idx"],
               s_threshold_1=s["threshold_1"], s_threshold_2=s["threshold_2"], s_fast_idx=s["fast_idx"],
               s_mid_idx=s["mid_idx"], s_slow_idx=s["slow_idx"], s_mean_slow=s["mean_slow"], s_mean_mid=s["mean_mid"],
               s_mean_fast=s["mean_fast"], s_std_slow=s["std_slow"],
               w_lower=w["lower_limit"], w_upper=w["upper_limit"], w_speed_idx=w["speed_idx"],
               w_mean=np.array(w["das_veh_states_mean"]), w_peaks=w["peaks"], w_mode_peak=w["mode_peak"],
               w_threshold_1=w["threshold_1"], w_heavy_idx=w["heavy_idx"], w_mid_idx=w["mid_idx"],
               w_light_idx=w["light_idx"], w_mean_light=w["mean_light"], w_mean_mid=w["mean_mid"],
               w_mean_heavy=w["mean_heavy"], w_std_light=w["std_light"], w_std_mid=w["std_mid"],
               w_std_heavy=w["std_heavy"])
    out = {k: np.asarray(v) for k, v in out.items()}

    for k in ("s_peak_idx", "s_fast_idx", "s_mid_idx", "s_slow_idx", "w_speed_idx", "w_heavy_idx", "w_mid_idx",
              "w_light_idx"):
        assert out[k].size > 0, f"{k} is empty"
    assert lead(out["s_peaks"]) >= 2 and lead(out["w_peaks"]) >= 2, (lead(out["s_peaks"]), lead(out["w_peaks"]))
    clear_of(out["s_peaks"], [out["s_lower"], out["s_upper"]], "speed notebook peak limits")
    clear_of(out["s_peaks"], np.histogram(out["s_peaks"], bins=100)[1], "speed notebook bin edges", skip_extremes=True)
    clear_of(out["w_peaks"], [out["w_threshold_1"]], "weight notebook threshold_1")
    clear_of(out["w_peaks"], np.histogram(out["w_peaks"], bins=100)[1], "weight notebook bin edges", skip_extremes=True)
    s_speed = np.asarray(s["veh_speed"])  # the speeds the majority filter kept
    clear_of(s_speed, [out["s_threshold_1"], out["s_threshold_2"]], "speed classes")
    clear_of(veh_speed, [out["w_lower"], out["w_upper"]], "speed majority")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes; classes",
          {k: int(out[k].size) for k in out if k.endswith("_idx")}, "leads", lead(out["s_peaks"]), lead(out["w_peaks"]))


if __name__ == "__main__":
    sys.exit(main())
