#!/usr/bin/env python
"""EarthModel.refine_sets on one MI355X at the notebook configuration of tools/bench_inversion.py (six layers, modes
0 / 3 / 4 on 176 periods, 206 samples): an ensemble of K observation sets refined in one batch, against a loop of
EarthModel.refine over sets one at a time.

  sets      the true model's curves plus seeded noise of the curves' sigma (2 %), K = 1800 (what the bootstrap
            produces); every set starts from the true model
  batched   refine_sets(profile=True): device events around dvh_lm_solve with the trial point and its chain, the scan,
            dvh_rayleigh_sens, dvh_lm_normal_sets and the selection, the median over the iterations; and the whole
            call's wall time
  looped    on the same run, refine over the first 64 of the sets, one call each: wall time per (set, iteration)
  scaled    the batched iteration against tools/bench_refine.py's 250-model iteration (profiles/refine.json) scaled
            by K / 250

No time is fixed in advance; the only condition is that the batched time per (set, iteration) is below the looped one.
One JSON line.

    python tools/bench_refine_sets.py [--sets 1800] [--loop-sets 64] [--refine-iter 20] [--out profiles/refine_sets.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_inversion as cfg  # noqa: E402  (puts the repository root on sys.path)

from das_diff_veh_amd.inversion import Curve  # noqa: E402

NAMES = ("solve_ms", "modes_ms", "sens_ms", "normal_ms", "select_ms")
REFINE_250_MS = 6.00  # profiles/refine.json, final_swarm.per_iteration.iteration_ms (250 models on one table)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=1800)
    ap.add_argument("--loop-sets", type=int, default=64)
    ap.add_argument("--refine-iter", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine_sets needs the MI355X: there is no CPU path to time")
    torch.cuda.set_device(0)
    K, L, T = args.sets, min(args.loop_sets, args.sets), args.refine_iter
    cs = cfg.curves()
    model = cfg.earth_model(50, 5)
    rng = np.random.default_rng(0)
    data_sets = [c.data + rng.standard_normal((K, c.period.size)) * c.uncertainties for c in cs]
    true_x = np.array(cfg.TRUE_H + cfg.TRUE_VS + [cfg.NU] * len(cfg.BOUNDS))
    xs = np.tile(true_x, (K, 1))

    model.refine_sets(cs, data_sets, xs, maxiter=2)  # warm-up at this batch size: library load, allocator
    res, batched_ms = wall(lambda: model.refine_sets(cs, data_sets, xs, maxiter=T))
    prof = model.refine_sets(cs, data_sets, xs, maxiter=T, profile=True)
    assert np.array_equal(prof.misfits, res.misfits)
    per = {k: float(np.median(prof.timings[k])) for k in NAMES}
    per["iteration_ms"] = float(np.median(sum(prof.timings[k] for k in NAMES)))

    def one(k):
        curves = [Curve(c.period, d[k], c.mode, "rayleigh", "phase", weight=c.weight, uncertainties=c.uncertainties)
                  for c, d in zip(cs, data_sets)]
        return model.refine(curves, xs[k:k + 1], maxiter=T)

    one(0)  # warm-up at batch size 1
    loop, looped_ms = wall(lambda: [one(k) for k in range(L)])
    same = all(np.array_equal(r.history[:, 0], res.history[:, k]) and np.array_equal(r.xs[0], res.xs[k])
               for k, r in enumerate(loop))
    batched_each = batched_ms / (K * T)
    looped_each = looped_ms / (L * T)
    scaled = REFINE_250_MS * K / 250.0
    out = {
        "metric": "EarthModel.refine_sets device time per iteration (dvh_lm_solve + dvh_rayleigh_modes + "
                  f"dvh_rayleigh_sens + dvh_lm_normal_sets + selection), K = {K} sets",
        "config": {"workload": "refine_sets", "layers": len(cfg.BOUNDS), "parameters": 3 * len(cfg.BOUNDS) - 1,
                   "periods": int(np.unique(np.concatenate([c.period for c in cs])).size),
                   "samples": int(sum(c.period.size for c in cs)), "curves": len(cs), "sets": K, "loop_sets": L,
                   "refine_iter": T, "noise": "the curves' sigma (2 %)", "lam0": 1e-3, "dc": 0.005, "tol": 1e-9},
        "batched": {"per_iteration": per, "wall_ms": batched_ms, "ms_per_set_iteration": batched_each,
                    "flagged": int((res.status & 1).sum()), "improved": int((res.misfits < res.start_misfits).sum()),
                    "median_start": float(np.median(res.start_misfits)), "median_end": float(np.median(res.misfits))},
        "looped": {"wall_ms": looped_ms, "ms_per_set_iteration": looped_each,
                   "rows_equal_the_batch": bool(same)},
        "looped_over_batched": looped_each / batched_each,
        "scaled_refine": {"iteration_ms_250": REFINE_250_MS, "scaled_to_sets_ms": scaled,
                          "batched_iteration_over_scaled": per["iteration_ms"] / scaled},
        "vs_spread": {"depths_km": [0.005, 0.02, 0.04, 0.08],
                      "std_km_s": [float(x) for x in res.profile_stats([0.005, 0.02, 0.04, 0.08]).std]},
    }
    out.update(value=per["iteration_ms"], unit="ms/iteration", n_gpus=1)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    if not batched_each < looped_each:
        raise SystemExit("the batched time per (set, iteration) is not below the looped one")


if __name__ == "__main__":
    main()
