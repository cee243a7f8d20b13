#!/usr/bin/env python
"""EarthModel.refine_section on one MI355X at the notebook configuration of tools/bench_inversion.py (six layers, modes
0 / 3 / 4 on 176 periods, 206 samples): 512 observation sets refined as chains, against EarthModel.refine_sets over the
same 512 sets on the same run, which is what existed before.

  sets      the true model's curves plus seeded noise of the curves' sigma (2 %); every set starts from the true model
  shapes    one chain of L = 512 (the sliding workload's pivot count) and C = 8 chains of L = 64
  section   refine_section(profile=True): device events around dvh_lm_solve_chain with the trial point and its chain
            rule, the scan, dvh_rayleigh_sens, dvh_lm_normal_sets and the selection, the median over the iterations
  apart     refine_sets(profile=True) over the same sets: the same events around dvh_lm_solve
  solve     device events around the raw dvh_lm_solve_chain launch alone on the refined g, H, u of each shape, around
            dvh_lm_solve on the same rows, and around both on 512 random SPD systems of 96 parameters (the largest the
            entries take)

No time is a pass/fail condition.  One JSON line.

    python tools/bench_refine_section.py [--refine-iter 20] [--coupling 100] [--out profiles/refine_section.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_inversion as cfg  # noqa: E402  (puts the repository root on sys.path)

from das_diff_veh_amd import inversion as inv  # noqa: E402

NAMES = ("solve_ms", "modes_ms", "sens_ms", "normal_ms", "select_ms")
SHAPES = ((1, 512), (8, 64))  # (chains, positions)


def per_iteration(res):
    per = {k: float(np.median(res.timings[k])) for k in NAMES}
    per["iteration_ms"] = float(np.median(sum(res.timings[k] for k in NAMES)))
    return per


def device_ms(fn, repeats=10):
    """The median device time of fn() by events, after one warm-up call."""
    fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def solve_times(H, g, u, free, mu, C, L):
    """dvh_lm_solve_chain on C chains of L and dvh_lm_solve on the same rows, ms each."""
    dev = H.device
    lam_c = torch.full((C,), 1e-3, dtype=torch.float64, device=dev)
    lam_m = torch.full((C * L,), 1e-3, dtype=torch.float64, device=dev)
    link = torch.ones((C, L - 1), dtype=torch.float64, device=dev)
    chain = device_ms(lambda: inv.lm_solve_chain(H, g, u, lam_c, free, mu, link, L))
    _, status = inv.lm_solve_chain(H, g, u, lam_c, free, mu, link, L)
    return {"lm_solve_chain_ms": chain, "lm_solve_ms": device_ms(lambda: inv.lm_solve(H, g, lam_m, free)),
            "chains_refused": int((status != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refine-iter", type=int, default=20)
    ap.add_argument("--coupling", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine_section needs the MI355X: there is no CPU path to time")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    M, T = SHAPES[0][0] * SHAPES[0][1], args.refine_iter
    cs = cfg.curves()
    model = cfg.earth_model(50, 5)
    rng = np.random.default_rng(0)
    data_sets = [c.data + rng.standard_normal((M, c.period.size)) * c.uncertainties for c in cs]
    true_x = np.array(cfg.TRUE_H + cfg.TRUE_VS + [cfg.NU] * len(cfg.BOUNDS))
    xs = np.tile(true_x, (M, 1))
    lo, hi = model.bounds()
    free = torch.from_numpy((hi > lo).astype(np.int32)).to(dev)

    model.refine_sets(cs, data_sets, xs, maxiter=2)  # warm-up at this batch size: library load, allocator
    apart = model.refine_sets(cs, data_sets, xs, maxiter=T, profile=True)
    depths = [0.005, 0.02, 0.04, 0.08]
    spread = lambda p: [float(x) for x in p.std(axis=0)]
    out = {
        "metric": "EarthModel.refine_section device time per iteration (dvh_lm_solve_chain + dvh_rayleigh_modes + "
                  "dvh_rayleigh_sens + dvh_lm_normal_sets + selection), 512 sets as one chain",
        "config": {"workload": "refine_section", "layers": len(cfg.BOUNDS), "parameters": 3 * len(cfg.BOUNDS) - 1,
                   "free_parameters": int((hi > lo).sum()),
                   "periods": int(np.unique(np.concatenate([c.period for c in cs])).size),
                   "samples": int(sum(c.period.size for c in cs)), "curves": len(cs), "sets": M, "refine_iter": T,
                   "coupling": args.coupling, "noise": "the curves' sigma (2 %)", "lam0": 1e-3, "dc": 0.005,
                   "tol": 1e-9},
        "refine_sets": {"per_iteration": per_iteration(apart), "accepted": int(apart.accepted.sum()),
                        "median_start": float(np.median(apart.start_misfits)),
                        "median_end": float(np.median(apart.misfits)), "depths_km": depths,
                        "vs_std_km_s": spread(apart.profiles(depths))},
        "shapes": {},
    }
    for C, L in SHAPES:
        model.refine_section(cs, data_sets, xs, chain_len=L, coupling=args.coupling, maxiter=2)
        res = model.refine_section(cs, data_sets, xs, chain_len=L, coupling=args.coupling, maxiter=T, profile=True)
        u = np.where(hi > lo, (res.xs - lo) / np.where(hi > lo, hi - lo, 1.0), 0.0)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        out["shapes"][f"{C}x{L}"] = {
            "per_iteration": per_iteration(res), "accepted_per_chain": res.accepted[:, ::L].sum(axis=0).tolist(),
            "chain_status": res.chain_status.tolist(), "objective_start": res.objective_history[0].tolist(),
            "objective_end": res.objective.tolist(), "penalty_end": res.penalty.tolist(),
            "median_end": float(np.median(res.misfits)), "vs_std_km_s": spread(res.profiles(depths)),
            "solve_alone": solve_times(put(res.hessian), put(res.gradient), put(u), free, put(res.coupling), C, L)}
    D = inv.LM_MAX_PARAMS
    gen = torch.Generator(device=dev).manual_seed(0)
    B = torch.randn((M, D, D), dtype=torch.float64, device=dev, generator=gen)
    H = (B @ B.transpose(1, 2)) / D + torch.eye(D, dtype=torch.float64, device=dev)
    g = torch.randn((M, D), dtype=torch.float64, device=dev, generator=gen)
    u = torch.rand((M, D), dtype=torch.float64, device=dev, generator=gen)
    all_free = torch.ones(D, dtype=torch.int32, device=dev)
    mu = torch.ones(D, dtype=torch.float64, device=dev)
    out["largest"] = {f"{C}x{L}": solve_times(H, g, u, all_free, mu, C, L) for C, L in SHAPES}
    out["largest"]["parameters"] = D
    one = out["shapes"]["1x512"]["per_iteration"]
    out.update(value=one["iteration_ms"], unit="ms/iteration", n_gpus=1,
               section_over_refine_sets=one["iteration_ms"] / out["refine_sets"]["per_iteration"]["iteration_ms"])
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
