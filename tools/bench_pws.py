#!/usr/bin/env python
"""The phase-weighted stack beside the linear one on one MI355X, on the bootstrap workload's geometry.

The shape is the notebooks' convergence test (imaging_diff_speed.ipynb#cell25, #cell30): 60 sizes x 30 resamples = 1 800
stacks of the (-150, 0) rows x 500 lags, four ridge modes; the windows are the synthetic ones of
``bench.py --workload bootstrap``.  The gathers and the draws are made once, outside the timed parts.  Timed:

  analytic     dvh_hilbert_rows over every cached row (n x 48 rows of 500 lags), once per cache in use; here repeated
               into a spare buffer.  Device events.
  select       dvh_select_pws (power 2) and dvh_select_mean_var on the same 1 800 draws, alternately in the same run.
               The selection tables are uploaded once, outside; device events bracket one C-ABI launch each (no host
               work between them), and the result of each launch is compared with resample_stacks_sizes'.
               ``select_pws_over_linear`` is the ratio of the medians.  The draws' reads are 2x the linear stack's
               bytes (g and h per read), so about 2 is what the bytes predict.
  convergence  convergence(..., stack="pws") and stack="linear" alternately (the analytic signal already cached): a host
               clock around each call, which ends with the ridges on the host.

``--warmup`` rounds run untimed, then the median, minimum and maximum over ``--steps`` rounds.  Both [n_modes, max_size]
convergence curves of the synthetic class (the same draws) are recorded: whether the phase-weighted stack needs fewer
passes is read off them and gated nowhere.

    python tools/bench_pws.py [--steps 15] [--warmup 3] [--n 1442] [--power 2] [--out profiles/pws.json]
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

from das_diff_veh_amd import _lib  # noqa: E402
from das_diff_veh_amd import bootstrap as bt  # noqa: E402
from das_diff_veh_amd.device import upload  # noqa: E402
from das_diff_veh_amd.plan import pack_trajectories  # noqa: E402
from das_diff_veh_amd.synth import synth_batch_device  # noqa: E402

SIGMA, REF_IDX, LB, UB = [25, 50, 50, 50], [80, 130, 170, 170], [2.5, 10, 14, 16], [14, 15, 19, 20]
CURVES = [None,
          scipy.interpolate.interp1d([10, 12, 13, 14, 15, 16], [530, 470, 450, 430, 410, 391]),
          scipy.interpolate.interp1d([14, 15, 16, 17, 18, 19], [630, 583, 550, 520, 500, 490]),
          scipy.interpolate.interp1d([16, 17, 18, 19, 20, 21], [745, 690, 657, 626, 600, 580])]


def _summary(t):
    return {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "spread_ms": max(t) - min(t)}


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=1442, help="windows of the class")
    ap.add_argument("--max-size", type=int, default=60)
    ap.add_argument("--bt-times", type=int, default=30)
    ap.add_argument("--power", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pws.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pws needs the MI355X: there is no CPU path to time")
    power = bt.check_stack("pws", args.power)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    wins, x_axis, t_axis, trk, _ = synth_batch_device(args.n, pivot=700.0, seed=3, device=dev)
    tx, tt, tl = pack_trajectories(trk, dev)
    cache = bt.GatherCache.from_device(wins, x_axis, t_axis, tx, tt, tl, 700.0, 500.0, 900.0)
    del wins
    sels = bt.draw_sizes(cache.n, range(1, args.max_size + 1), args.bt_times, random.Random(100))
    B = args.max_size * args.bt_times
    s, e, _ = cache.disp_plan()
    nch, W, R = e + 1 - s, cache.W, cache.plan.R
    H = cache.analytic()

    # analytic(): the same launch into a spare buffer
    spare = torch.empty_like(H)
    row_len = torch.full((cache.n * R,), W, dtype=torch.int32, device=dev)

    def analytic():
        _lib.call("dvh_hilbert_rows", _lib.ptr(cache.G), W, cache.n * R, W, _lib.ptr(row_len), _lib.ptr(spare),
                  _lib.stream_of(dev))
    t_an = [_event_ms(analytic)[0] for _ in range(args.warmup + args.steps)][args.warmup:]
    if not torch.equal(spare, H):
        raise SystemExit("dvh_hilbert_rows is not reproducible")
    del spare

    # the 1 800 draws through both select kernels
    # (the selection tables cross to the device once, outside the events: the events bracket one kernel launch each)
    out = torch.empty((B, nch, W), dtype=torch.float32, device=dev)
    cnt = np.concatenate([np.full(x.shape[0], x.shape[1], dtype=np.int32) for x in sels])
    off = np.concatenate([[0], np.cumsum(cnt[:-1], dtype=np.int64)]).astype(np.int32)
    sel_t, off_t, cnt_t = upload([np.concatenate([x.reshape(-1) for x in sels]).astype(np.int32), off, cnt], dev)
    Gs, Hs, rows = cache.G[:, s:e + 1, :], H[:, s:e + 1, :], nch * W
    tabs = (_lib.ptr(sel_t), _lib.ptr(off_t), _lib.ptr(cnt_t), B)
    tail = (_lib.ptr(out), rows, _lib.stream_of(dev))
    launch = {"pws": lambda: _lib.call("dvh_select_pws", _lib.ptr(Gs), _lib.ptr(Hs), R * W, rows, *tabs, power, *tail),
              "linear": lambda: _lib.call("dvh_select_mean_var", _lib.ptr(Gs), R * W, rows, *tabs, *tail)}
    t_sel = {"pws": [], "linear": []}
    for rnd in range(args.warmup + args.steps):
        for name in ("pws", "linear"):
            ms, _ = _event_ms(launch[name])
            if rnd >= args.warmup:
                t_sel[name].append(ms)
    for name in ("pws", "linear"):  # the launches above are the library's own: same bits as the public call
        launch[name]()
        if not torch.equal(out, cache.resample_stacks_sizes(sels, stack=name, power=power)):
            raise SystemExit(f"the timed {name} launch differs from resample_stacks_sizes")
    mean_cnt = float(np.mean([x.shape[1] for x in sels]))
    read_bytes = 4.0 * B * mean_cnt * nch * W  # per kernel operand: G for both, H for pws as well

    # convergence() end to end
    conv_args = (args.max_size, args.bt_times, SIGMA, REF_IDX, LB, UB, CURVES)
    t_conv = {"pws": [], "linear": []}
    curves = {}
    for rnd in range(args.warmup + args.steps):
        for name in ("pws", "linear"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            curves[name] = bt.convergence(cache, *conv_args, rand=random.Random(100), stack=name, power=power)
            dt = time.perf_counter() - t0
            if rnd >= args.warmup:
                t_conv[name].append(dt * 1e3)

    res = {"metric": f"phase-weighted stack (power {power:g}) beside the linear stack: {B} draws of {nch} x {W} from "
                     f"{cache.n} passes; ms",
           "unit": "ms", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "config": {"passes": cache.n, "rows": cache.n * R, "lags": W, "resamples": B, "nch": nch,
                      "mean_draw_size": mean_cnt, "power": power, "gather_abs_max": float(cache.G.abs().max())},
           "analytic": dict(_summary(t_an), rows_per_s=cache.n * R / (statistics.median(t_an) / 1e3),
                            f64_fma=float(cache.n) * R * W * W),
           "select_pws": dict(_summary(t_sel["pws"]), read_bytes=2 * read_bytes),
           "select_linear": dict(_summary(t_sel["linear"]), read_bytes=read_bytes),
           "convergence_pws": _summary(t_conv["pws"]),
           "convergence_linear": _summary(t_conv["linear"])}
    res["select_pws"]["read_GBps"] = 2 * read_bytes / (res["select_pws"]["ms_median"] * 1e6)
    res["select_linear"]["read_GBps"] = read_bytes / (res["select_linear"]["ms_median"] * 1e6)
    res["select_pws_over_linear"] = res["select_pws"]["ms_median"] / res["select_linear"]["ms_median"]
    res["convergence_pws_over_linear"] = res["convergence_pws"]["ms_median"] / res["convergence_linear"]["ms_median"]
    res["curves"] = {name: np.asarray(c).tolist() for name, c in curves.items()}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
