#!/usr/bin/env python
"""Gauss-Newton refinement on one MI355X at the notebook configuration of tools/bench_inversion.py (six layers, 176
periods, three curves of 206 samples in all; popsize 50, maxiter 1000, maxrun 5).

  per iteration   EarthModel.refine(profile=True) for M = 5 (the run-bests) and M = 250 (the swarms' last positions):
                  device events around dvh_lm_solve with the trial point and its chain (torch ops), dvh_rayleigh_modes,
                  dvh_rayleigh_sens, dvh_lm_normal and the torch.where selection; the median over the iterations
  against swarm   invert + refine(run_best(), maxiter=20) against invert alone with as many further swarm iterations as
                  the refinement's device time buys (same seed, so the same first iterations); the five runs' misfits
                  before and after both, where the refined models stand (parameters on a bound, remaining gradient), and
                  for information the same refinement with five times the iterations.  No ratio is fixed in advance:
                  whichever way it comes out is what is written.

One JSON line.

    python tools/bench_refine.py [--maxiter 1000] [--refine-iter 20] [--out profiles/refine.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_inversion as cfg  # noqa: E402  (puts the repository root on sys.path)

NAMES = ("solve_ms", "modes_ms", "sens_ms", "normal_ms", "select_ms")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def split(model, curves, xs, iters):
    model.refine(curves, xs, maxiter=2)  # warm-up at this batch size
    res = model.refine(curves, xs, maxiter=iters, profile=True)
    per = {k: float(np.median(res.timings[k])) for k in NAMES}
    per["iteration_ms"] = float(np.median(sum(res.timings[k] for k in NAMES)))
    return {"models": int(xs.shape[0]), "iterations": iters, "per_iteration": per,
            "finite_starts": int(np.isfinite(res.start_misfits).sum()),
            "improved": int((res.misfits < res.start_misfits).sum()),
            "median_start": float(np.median(res.start_misfits)), "median_end": float(np.median(res.misfits))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--popsize", type=int, default=50)
    ap.add_argument("--maxiter", type=int, default=1000)
    ap.add_argument("--maxrun", type=int, default=5)
    ap.add_argument("--refine-iter", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine needs the MI355X: there is no CPU path to time")
    torch.cuda.set_device(0)
    cs = cfg.curves()
    R, N, T = args.maxrun, args.popsize, args.maxiter
    cfg.earth_model(N, 5).invert(cs, maxrun=R)  # warm-up: library load, allocator, first launches
    model = cfg.earth_model(N, T)
    res, invert_ms = timed(lambda: model.invert(cs, maxrun=R))
    best = res.run_best()
    model.refine(cs, best, maxiter=2)
    ref, refine_ms = timed(lambda: model.refine(cs, best, maxiter=args.refine_iter))
    long_ref, long_ms = timed(lambda: model.refine(cs, best, maxiter=5 * args.refine_iter))  # for information
    swarm_iter_ms = invert_ms / T
    extra = int(math.ceil(refine_ms / swarm_iter_ms))
    longer, longer_ms = timed(lambda: cfg.earth_model(N, T + extra).invert(cs, maxrun=R))
    assert np.array_equal(longer.global_misfits[:, :T], res.global_misfits)
    last = res.xs.reshape(R, T, N, -1)[:, -1].reshape(R * N, -1)
    # where the refined run-bests stand: parameters on a bound, and the gradient that the cube does not block
    lo, hi = model.bounds()
    free = hi > lo
    u = (ref.xs - lo)[:, free] / (hi - lo)[free]
    g = ref.gradient[:, free]
    blocked = ((u <= 0.0) & (g > 0.0)) | ((u >= 1.0) & (g < 0.0))
    out = {
        "metric": "EarthModel.refine device time per iteration (dvh_lm_solve + dvh_rayleigh_modes + "
                  "dvh_rayleigh_sens + dvh_lm_normal + selection), M = 5",
        "config": {"workload": "refine", "layers": len(cfg.BOUNDS), "parameters": 3 * len(cfg.BOUNDS) - 1,
                   "periods": int(np.unique(np.concatenate([c.period for c in cs])).size),
                   "samples": int(sum(c.period.size for c in cs)), "curves": len(cs), "popsize": N, "maxiter": T,
                   "maxrun": R, "refine_iter": args.refine_iter, "lam0": 1e-3, "dc": 0.005, "tol": 1e-9},
        "run_bests": split(model, cs, best, args.refine_iter),
        "final_swarm": split(model, cs, last, args.refine_iter),
        "against_swarm": {
            "invert_ms": invert_ms, "swarm_iteration_ms": swarm_iter_ms, "refine_ms": refine_ms,
            "extra_swarm_iterations": extra, "longer_invert_ms": longer_ms,
            "swarm_runs": [float(x) for x in res.global_misfits[:, -1]],
            "refine_start": [float(x) for x in ref.start_misfits],
            "refined_runs": [float(x) for x in ref.misfits],
            "accepted": [int(x) for x in ref.accepted.sum(axis=0)],
            "status": [int(x) for x in ref.status],
            "lam": [float(x) for x in ref.lam],
            "on_a_bound": [int(x) for x in ((u <= 0.0) | (u >= 1.0)).sum(axis=1)],
            "gradient_max": [float(x) for x in np.abs(g).max(axis=1)],
            "unblocked_gradient_max": [float(x) for x in np.where(blocked, 0.0, np.abs(g)).max(axis=1)],
            "longer_swarm_runs": [float(x) for x in longer.global_misfits[:, -1]],
            "five_times_the_iterations": {"refine_iter": 5 * args.refine_iter, "refine_ms": long_ms,
                                          "refined_runs": [float(x) for x in long_ref.misfits],
                                          "accepted": [int(x) for x in long_ref.accepted.sum(axis=0)]},
            "best": {"swarm": float(res.misfit), "refined": float(ref.misfits.min()),
                     "longer_swarm": float(longer.misfit)}},
    }
    out.update(value=out["run_bests"]["per_iteration"]["iteration_ms"], unit="ms/iteration", n_gpus=1)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
