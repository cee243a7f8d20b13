#!/usr/bin/env python
"""Swarm inversion on one MI355X at the speed notebook's configuration (inversion_diff_speed.ipynb cells 5-9):

  model     the notebook's six layers: thickness and vs bounds as in its cell 7, Poisson's ratio fixed at 0.4375,
            rho = 1.56 + 0.186 vp
  curves    its period grids (0.1 Hz steps: mode 0 on 2.5 .. 14.0 Hz with weight 2, mode 3 on 14.1 .. 19.0 Hz, mode 4
            on 16.1 .. 20.0 Hz), the data computed by the forward call from a synthetic true model inside the bounds,
            uncertainties 2 % (the notebook's own curves are pickled picks)
  swarm     popsize 50, maxiter 1000, maxrun 5 (the five runs advance together as one batch of 250 particles)

One JSON line: the wall time of invert() by device events (whole, and per run = whole / maxrun), model evaluations per
second, the per-iteration split between the dvh_rayleigh_modes launch and the rest of the iteration (misfit, swarm
update) from a second, event-instrumented call, and the best misfit.  The notebook prints 3:20 - 4:39 per run for
evodcinv's CPSO on its CPU; the machine, the optimizer and the forward code all differ, so the two are printed side by
side and no ratio is formed.

    python tools/bench_inversion.py [--popsize 50] [--maxiter 1000] [--maxrun 5] [--out profiles/inversion.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from das_diff_veh_amd.inversion import Curve, EarthModel, Layer, phase_velocity  # noqa: E402

NU = 0.4375
BOUNDS = [([0.001, 0.015], [0.1, 0.5]), ([0.001, 0.015], [0.1, 0.5]), ([0.005, 0.025], [0.2, 0.6]),
          ([0.005, 0.025], [0.2, 0.6]), ([0.02, 0.08], [0.4, 1.0]), ([0.02, 0.08], [0.4, 1.0])]
TRUE_H = [0.008, 0.008, 0.015, 0.015, 0.05]
TRUE_VS = [0.15, 0.22, 0.3, 0.42, 0.6, 0.9]
FREQS = 2.5 + 0.1 * np.arange(176)  # one grid, so that the curves share their common periods exactly
GRIDS = [(0, 0, 116, 2.0), (3, 116, 166, 1.0), (4, 136, 176, 1.0)]  # mode, first and end index into FREQS, weight


def density(vp):
    return 1.56 + 0.186 * vp


def earth_model(popsize, maxiter, seed=0):
    m = EarthModel()
    for h, vs in BOUNDS:
        m.add(Layer(h, vs, [NU, NU]))
    return m.configure(optimizer="pso", misfit="rmse", density=density,
                       optimizer_args=dict(popsize=popsize, maxiter=maxiter, seed=seed))


def curves():
    vs = np.array(TRUE_VS)
    vp = vs * np.sqrt((2 - 2 * NU) / (1 - 2 * NU))
    out = []
    for mode, first, end, weight in GRIDS:
        period = (1.0 / FREQS[first:end])[::-1]
        c = phase_velocity(period, np.array(TRUE_H + [0.0]), vp, vs, density(vp), mode=mode)
        if not np.isfinite(c).all():
            raise SystemExit(f"the true model has no mode {mode} on part of its grid")
        out.append(Curve(period, c, mode, "rayleigh", "phase", weight=weight, uncertainties=0.02 * c))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--popsize", type=int, default=50)
    ap.add_argument("--maxiter", type=int, default=1000)
    ap.add_argument("--maxrun", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inversion needs the MI355X: there is no CPU path to time")
    torch.cuda.set_device(0)
    cs = curves()
    earth_model(args.popsize, 5).invert(cs, maxrun=args.maxrun)  # warm-up: library load, allocator, first launches
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = earth_model(args.popsize, args.maxiter).invert(cs, maxrun=args.maxrun)
    b.record()
    b.synchronize()
    wall_s = a.elapsed_time(b) / 1e3
    prof = earth_model(args.popsize, args.maxiter).invert(cs, maxrun=args.maxrun, profile=True)
    assert np.array_equal(prof.misfits, res.misfits)
    modes_ms, rest_ms = prof.timings["modes_ms"], prof.timings["rest_ms"]
    n_eval = res.misfits.size
    n_period = int(np.unique(np.concatenate([c.period for c in cs])).size)
    line = json.dumps({
        "metric": "EarthModel.invert wall time per run (dvh_rayleigh_modes + dvh_curve_misfit + swarm update)",
        "value": wall_s / args.maxrun, "unit": "s/run", "n_gpus": 1,
        "config": {"workload": "inversion", "layers": len(BOUNDS), "poisson": NU, "modes": [g[0] for g in GRIDS],
                   "periods": n_period, "samples": int(sum(c.period.size for c in cs)), "popsize": args.popsize,
                   "maxiter": args.maxiter, "maxrun": args.maxrun, "dc": 0.005, "tol": 1e-9},
        "invert": {"wall_s": wall_s, "s_per_run": wall_s / args.maxrun, "evaluations": n_eval,
                   "evaluations_per_s": n_eval / wall_s},
        "per_iteration": {"modes_ms_mean": float(modes_ms.mean()), "modes_ms_first": float(modes_ms[0]),
                          "modes_ms_last": float(modes_ms[-1]), "rest_ms_mean": float(rest_ms.mean()),
                          "modes_share": float(modes_ms.sum() / (modes_ms.sum() + rest_ms.sum()))},
        "misfit": {"best": float(res.misfit), "runs": [float(x) for x in res.global_misfits[:, -1]],
                   "finite_share": float(np.isfinite(res.misfits).mean())},
        "notebook": {"what": "evodcinv CPSO + disba on the notebook's CPU, as its cell 9 prints",
                     "s_per_run": [200, 279], "comparable": False},
    })
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
