#!/usr/bin/env python
"""One convergence test on the phase-shift transform on one MI355X: the ridge walk on stored images against the
fused walk that computes the values it compares.

The shape is the notebooks' (imaging_diff_speed.ipynb#cell25, #cell30): 60 sizes x 30 resamples = 1 800 stacks of the
(-150, 0) rows x 500 lags, 1 000 velocities x 242 frequencies, four modes with the notebook's sigma, bands, reference
indices and reference curves; the windows are the synthetic ones of ``bench.py --workload bootstrap``.  The gathers
and the draws are made once, outside the timed part.  Two paths, timed alternately:

  image   resample_stacks_sizes, slant_maps with an all-rows plan (1.7 GB of float32 images), dvh_ridge per mode.
          Only functions the library had before the fused walk: the same tool times the baseline on an older tree
          (``--paths image``).
  fused   resample_stacks_sizes, then slant_ridges_launch: dvh_disp_tdft once, dvh_slant_ridge per mode on side
          streams, no image.

Each sample is a host clock around one path that ends with the ridges on the host (so it ends in a synchronise);
``--warmup`` rounds run untimed, then the median, minimum and maximum over ``--steps`` rounds.  The paths' ridges are
compared (they must be equal).  ``decision`` is the default the measurement gives walk=None: "fused" when the fused
median beats the image median by more than the two spreads (max - min) together, else "image".

    python tools/bench_boot_slant.py [--steps 15] [--warmup 3] [--paths image,fused] [--n 1442] [--out FILE]

Kernel times come from a run of its own under ``rocprofv3 --kernel-trace --stats`` (few steps): the events above
include launch gaps and the read-back.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import scipy.interpolate
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from das_diff_veh_amd import bootstrap as bt  # noqa: E402
from das_diff_veh_amd.disp import SlantPlan, slant_maps  # noqa: E402
from das_diff_veh_amd.plan import pack_trajectories  # noqa: E402
from das_diff_veh_amd.synth import synth_batch_device  # noqa: E402

SIGMA, REF_IDX, LB, UB = [25, 50, 50, 50], [80, 130, 170, 170], [2.5, 10, 14, 16], [14, 15, 19, 20]
CURVES = [None,
          scipy.interpolate.interp1d([10, 12, 13, 14, 15, 16], [530, 470, 450, 430, 410, 391]),
          scipy.interpolate.interp1d([14, 15, 16, 17, 18, 19], [630, 583, 550, 520, 500, 490]),
          scipy.interpolate.interp1d([16, 17, 18, 19, 20, 21], [745, 690, 657, 626, 600, 580])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--paths", default="image,fused")
    ap.add_argument("--n", type=int, default=1442, help="windows of the class")
    ap.add_argument("--max-size", type=int, default=60)
    ap.add_argument("--bt-times", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_boot_slant needs the MI355X: there is no CPU path to time")
    paths = args.paths.split(",")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    wins, x_axis, t_axis, trk, _ = synth_batch_device(args.n, pivot=700.0, seed=3, device=dev)
    tx, tt, tl = pack_trajectories(trk, dev)
    cache = bt.GatherCache.from_device(wins, x_axis, t_axis, tx, tt, tl, 700.0, 500.0, 900.0)
    del wins
    sels = bt.draw_sizes(cache.n, range(1, args.max_size + 1), args.bt_times, random.Random(100))
    first = np.concatenate([x[:, 0] for x in sels])
    refs = [r - int(np.sum(bt.FREQS < lb)) for r, lb in zip(REF_IDX, LB)]
    s, e, _ = cache.disp_plan()
    gt = cache.gt
    plan = SlantPlan(e + 1 - s, cache.W, 8.16, float(gt[1] - gt[0]), bt.FREQS, np.sort(bt.VELS)[::-1].astype(np.float64),
                     rows=(0, e + 1 - s))
    B = args.max_size * args.bt_times

    def image():
        stacks = cache.resample_stacks_sizes(sels)
        fv = slant_maps(stacks, plan, norm=False)
        pend = [bt.ridges_launch(fv, bt.FREQS, bt.VELS, LB[m], UB[m], ref_freq_idx=refs[m], sigma=SIGMA[m],
                                 vel_max=800, ref_vel=CURVES[m]) for m in range(4)]
        return [bt.ridges_finish(p) for p in pend]

    def fused():
        stacks = cache.resample_stacks_sizes(sels)
        return bt.slant_ridges_finish(bt.slant_ridges_launch(cache, stacks, first, LB, UB, refs, SIGMA, 800, CURVES,
                                                             side_streams=True))

    fns = {"image": image, "fused": fused}
    times = {p: [] for p in paths}
    last = {}
    for rnd in range(args.warmup + args.steps):
        for p in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[p] = fns[p]()
            dt = time.perf_counter() - t0
            if rnd >= args.warmup:
                times[p].append(dt * 1e3)
    res = {"metric": f"convergence test on the phase-shift transform: {B} resamples of {plan.n_row} x {plan.nt}, "
                     f"{plan.nV} x {plan.nF}, 4 modes; ms per test, gathers and draws outside",
           "unit": "ms", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "config": {"passes": cache.n, "resamples": B, "n_row": plan.n_row, "nt": plan.nt, "nV": plan.nV,
                      "nF": plan.nF, "n_fb": plan.n_fb, "bands": [int(np.sum((bt.FREQS >= a) & (bt.FREQS < b)))
                                                                   for a, b in zip(LB, UB)],
                      "image_bytes": 4 * B * plan.nV * plan.nF}}
    for p in paths:
        t = times[p]
        res[p] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "spread_ms": max(t) - min(t),
                  "resamples_per_s": B / (statistics.median(t) / 1e3)}
    if "image" in res and "fused" in res:
        equal = all(np.array_equal(a, b) for a, b in zip(last["image"], last["fused"]))
        if not equal:
            raise SystemExit("the fused walk's ridges differ from the image walk's")
        gain = res["image"]["ms_median"] - res["fused"]["ms_median"]
        res["ridges_equal"] = True
        res["image_over_fused"] = res["image"]["ms_median"] / res["fused"]["ms_median"]
        res["decision"] = "fused" if gain > res["image"]["spread_ms"] + res["fused"]["spread_ms"] else "image"
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
