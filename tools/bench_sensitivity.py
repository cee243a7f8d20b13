#!/usr/bin/env python
"""Rayleigh sensitivity kernels and group velocity on one MI355X, against what differencing the forward model costs:

  (a) kernel figure   the "Sensitivity kernel" section of inversion_diff_weight.ipynb: a six-layer model cut into 30
                      layers of 10 m over its half-space, 2 / 3 / 4 / 5 / 10 / 15 / 20 / 25 Hz, mode 0, velocity_s only
  (b) Jacobian        one swarm iteration of tools/bench_inversion.py: 250 six-layer models inside its bounds x its 176
                      periods, the modes its curves need at each, all four columns and the group velocity

For each: the time of rayleigh_modes + dvh_rayleigh_sens (and of the dvh_rayleigh_sens launch alone) by device events,
and the time of the same numbers by central differences of rayleigh_modes at tol = 1e-13, which is what the library
offered before the kernel: two launches per direction (every selected layer column, and omega for the group velocity),
and the same 2 n_dir perturbed batches as one launch.  The worst disagreement of the differences with the kernel is
reported in the tests' dimensionless measure, |p (a - b)| / c.  One JSON line; no ratio is claimed in advance.

    python tools/bench_sensitivity.py [--reps 20] [--out profiles/sensitivity.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_inversion as bi  # noqa: E402
from das_diff_veh_amd import inversion as inv  # noqa: E402

STEP = 3e-5       # relative step of the central differences: truncation 1e-9, rounding 1e-13 / 3e-5 = 3e-9
FD_TOL = 1e-13    # the width the differenced roots are refined to
KERNEL_HZ = (2.0, 3.0, 4.0, 5.0, 10.0, 15.0, 20.0, 25.0)


def layers_of(h, vs):
    vs = np.asarray(vs, np.float64)
    vp = vs * np.sqrt((2 - 2 * bi.NU) / (1 - 2 * bi.NU))
    return np.stack([np.r_[np.asarray(h, np.float64), 0.0], vp, vs, bi.density(vp)], 1)


def kernel_figure_model():
    """bench_inversion's true model as 30 layers of 10 m (each takes the velocity at its middle) over the half-space."""
    tops = np.r_[0.0, np.cumsum(bi.TRUE_H)]
    mid = 0.005 + 0.01 * np.arange(30)
    vs = np.array(bi.TRUE_VS)[np.minimum(np.searchsorted(tops, mid, side="right") - 1, 5)]
    return layers_of(np.full(30, 0.01), np.r_[vs, bi.TRUE_VS[-1]])[None]


def swarm_models(n=250, seed=0):
    rng = np.random.default_rng(seed)
    lo = np.array([(b[0][0], b[1][0]) for b in bi.BOUNDS])
    hi = np.array([(b[0][1], b[1][1]) for b in bi.BOUNDS])
    x = rng.uniform(lo, hi, (n, 6, 2))
    return np.stack([layers_of(m[:-1, 0], m[:, 1]) for m in x])


def swarm_need():
    need = np.zeros(bi.FREQS.size, np.int32)
    for mode, first, end, _ in bi.GRIDS:
        need[first:end] = np.maximum(need[first:end], mode + 1)
    return need


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, out


def measure(models, periods, n_mode, need, parameters, c_min, reps):
    dev = torch.device("cuda:0")
    L = torch.from_numpy(np.ascontiguousarray(models)).to(dev)
    T = torch.from_numpy(np.ascontiguousarray(periods)).to(dev)
    nd = None if need is None else torch.from_numpy(need).to(dev)
    cols = [inv.PARAMETERS.index(p) for p in parameters]
    M, n_layer, _ = models.shape
    kw = dict(dc=0.005, c_min=c_min, need=nd)

    def kernel():
        return inv._sens(L, T, n_mode, cols, True, tol=1e-9, **kw)

    kernel_ms, (c, u, dcdp) = timed(kernel, reps)
    c_in = inv.rayleigh_modes(L, T, n_mode, tol=1e-9, **kw)
    out = [torch.empty_like(c), torch.empty_like(c), torch.empty_like(dcdp)]

    def sens_only():
        inv._lib.call("dvh_rayleigh_sens", inv._lib.ptr(L), M, n_layer, inv._lib.ptr(T), T.numel(), inv._lib.ptr(c_in),
                      n_mode, sum(1 << q for q in cols), 1e-9, *(inv._lib.ptr(o) for o in out),
                      inv._lib.stream_of(dev))

    sens_ms, _ = timed(sens_only, reps)
    modes_ms, _ = timed(lambda: inv.rayleigh_modes(L, T, n_mode, tol=1e-9, **kw), reps)

    # central differences of rayleigh_modes: the perturbed batches, direction by direction (omega first)
    dirs = [(l, q) for l in range(n_layer) for q in cols if models[0, l, q] != 0.0]
    batches, periods_of = [], []
    for s in (1.0 + STEP, 1.0 - STEP):
        batches.append(L)
        periods_of.append(T / s)  # omega (1 +- STEP)
    for l, q in dirs:
        for s in (1.0 + STEP, 1.0 - STEP):
            m = L.clone()
            m[:, l, q] *= s
            batches.append(m)
            periods_of.append(T)

    def differences():
        return [inv.rayleigh_modes(m, t, n_mode, tol=FD_TOL, **kw) for m, t in zip(batches, periods_of)]

    fd_ms, cs = timed(differences, max(1, reps // 5))
    stacked = torch.cat(batches[2:])

    def differences_one_launch():
        inv.rayleigh_modes(batches[0], periods_of[0], n_mode, tol=FD_TOL, **kw)
        inv.rayleigh_modes(batches[1], periods_of[1], n_mode, tol=FD_TOL, **kw)
        return inv.rayleigh_modes(stacked, T, n_mode, tol=FD_TOL, **kw)

    fd1_ms, _ = timed(differences_one_launch, max(1, reps // 5))

    ok = torch.isfinite(c)
    w_cw = (cs[0] - cs[1]) / (2.0 * STEP)  # omega dc/domega
    u_fd = c / (1.0 - w_cw / c)
    e_u = (torch.abs(u_fd - u) / u)[ok & torch.isfinite(u_fd)]
    e_p = []
    for j, (l, q) in enumerate(dirs):
        p_cp = (cs[2 + 2 * j] - cs[3 + 2 * j]) / (2.0 * STEP)  # p dc/dp
        e = torch.abs(p_cp - L[:, l, q][:, None, None] * dcdp[..., l, q]) / c
        e_p.append(e[ok & torch.isfinite(p_cp)])
    e_p = torch.cat(e_p)
    # a perturbed model whose scan loses or gains a pair of roots renumbers its modes: the differences of such a root
    # are not derivatives, so the bulk is reported beside the worst
    q999 = lambda e: float(torch.quantile(e[torch.randperm(e.numel(), device=e.device)[:1000000]], 0.999))
    return {"models": int(M), "layers": int(n_layer), "periods": int(T.numel()), "n_mode": int(n_mode),
            "parameters": list(parameters), "roots": int(ok.sum()), "directions_differenced": len(dirs) + 1,
            "modes_plus_sens_ms": kernel_ms, "sens_launch_ms": sens_ms, "modes_launch_ms": modes_ms,
            "differences_two_launches_per_direction_ms": fd_ms, "differences_one_batched_launch_ms": fd1_ms,
            "disagreement_dcdp": {"worst": float(e_p.max()), "q999": q999(e_p), "entries": int(e_p.numel())},
            "disagreement_group": {"worst": float(e_u.max()), "q999": q999(e_u), "entries": int(e_u.numel())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sensitivity needs the MI355X: there is no CPU path to time")
    torch.cuda.set_device(0)
    fig = kernel_figure_model()
    a = measure(fig, 1.0 / np.array(KERNEL_HZ), 1, None, ("velocity_s",), 0.8 * fig[0, :, 2].min(), args.reps * 10)
    b = measure(swarm_models(), (1.0 / bi.FREQS)[::-1].copy(), 5, swarm_need()[::-1].copy(), inv.PARAMETERS,
                0.8 * min(x[1][0] for x in bi.BOUNDS), args.reps)
    line = json.dumps({
        "metric": "rayleigh_modes + dvh_rayleigh_sens, one swarm iteration's Jacobian and group velocities",
        "value": b["modes_plus_sens_ms"], "unit": "ms", "n_gpus": 1,
        "config": {"workload": "sensitivity", "dc": 0.005, "tol": 1e-9, "difference_step": STEP,
                   "difference_tol": FD_TOL},
        "kernel_figure": a, "swarm_jacobian": b})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
