#!/usr/bin/env python
"""Phase-shift dispersion (map_fv_FD_slant_stack) on one MI355X: slant_maps and its dvh_disp_slant launch.

One JSON line per shape:
  class      B = 3 class stacks of 25 x 500 on the notebooks' grid, 1 000 velocities x 242 frequencies
  timelapse  B = 512 gathers of 25 x 500 on the time-lapse grid, 512 velocities x 1 000 frequencies
Timing: a round times the launch, the call, the spectra and the f-k chain one after the other, each as HIP events
around a sample of back-to-back calls (200 for the class shape, 5 for the timelapse shape); `--warmup` rounds run untimed,
then the median, minimum and maximum per call over `--steps` rounds.  Inputs and outputs rotate over `--sets` buffer
sets with every call, so that no call finds its own output in the caches.
Per line:
  call     slant_maps (row L1 norms, time DFT at the needed bins, steering sum) on resident gathers, into the set's
           output buffer
  launch   dvh_disp_slant alone on each set's resident spectra, into the same buffers, and its share of the float64
           vector floor: 4 * n_row * B * nF * nV FMAs at the 28-31 T FMA/s the float64 vector pipe gave
  spectra  the two launches before it alone; call_minus_parts = call - spectra - launch says how well the three agree
  numpy    tests/slant_ref.slant, the vectorised float64 restatement, in this process on this host: seconds per gather
           over `--numpy-gathers` gathers, and that scaled to the batch
  fk       fv_maps (the f-k chain, map_fv) on the same batch, for scale
  parity   the device images of the first `--numpy-gathers` gathers against slant_ref on the same float32 values: the
           worst error relative to the image maximum (above 1e-6: no line and a non-zero exit) and the picks (argmax over
           velocity per frequency) strictly identical to the float64 ones

    python tools/bench_slant.py [--steps 30] [--warmup 10] [--sets 3] [--numpy-gathers 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from das_diff_veh_amd.disp import DispPlan, SlantPlan, _slant_launch, _slant_spectra, fv_maps, slant_maps  # noqa: E402
from das_diff_veh_amd.synth import synth_gathers  # noqa: E402
from tests import slant_ref  # noqa: E402

FP64_VALU_TFMA = (28.0, 31.0)  # measured float64 FMA rate of the vector pipe, T FMA/s
DX, DT = 8.16, 0.003999999999997783
SHAPES = {
    "class": dict(B=3, inner=200, freqs=np.arange(0.8, 25, 0.1), vels=np.arange(200, 1200).astype(np.float64)),
    "timelapse": dict(B=512, inner=5, freqs=np.linspace(1.0, 25.0, 1000), vels=np.linspace(200.0, 1200.0, 512)),
}


def alternating_ms(fns, n_set, steps, warmup, inner):
    """{name: (median, min, max) ms per call} of the functions fns[name](k), k cycling over the buffer sets.  A round
    times every function once, one after the other, each as HIP events around `inner` back-to-back calls; `warmup`
    rounds run untimed first.  The functions alternate, so a drift of the clocks or of the box falls on all of them."""
    k = 0
    evs = {name: [] for name in fns}
    for rnd in range(warmup + steps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn(k % n_set)
                k += 1
            b.record()
            if rnd >= warmup:
                evs[name].append((a, b))
        torch.cuda.synchronize()
    out = {}
    for name, pairs in evs.items():
        ts = [a.elapsed_time(b) / inner for a, b in pairs]
        out[name] = (statistics.median(ts), min(ts), max(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--numpy-gathers", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_slant needs the MI355X: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []
    for name, sh in SHAPES.items():
        B, freqs, vels = sh["B"], sh["freqs"], sh["vels"]
        plan = SlantPlan(25, 500, DX, DT, freqs, vels)
        fk_plan = DispPlan(25, 500, DX, DT, freqs, vels)
        data = [synth_gathers(B, 25, 500, DX, DT, dev, seed=7 + k) for k in range(args.sets)]
        outs = [torch.empty((B, plan.nV, plan.nF), dtype=torch.float32, device=dev) for _ in range(args.sets)]
        specs = [_slant_spectra(d, plan, True) for d in data]

        def call(k):
            slant_maps(data[k], plan, norm=True, out=outs[k])

        def spectra(k):
            _slant_spectra(data[k], plan, True)

        def launch(k):
            _slant_launch(specs[k], plan, B, outs[k])

        def fk(k):
            fv_maps(data[k], fk_plan, norm=True)

        inner = sh["inner"]
        ms = alternating_ms(dict(launch=launch, call=call, spectra=spectra, fk=fk), args.sets, args.steps, args.warmup,
                            inner)
        launch_ms, call_ms, spec_ms, fk_ms = ms["launch"], ms["call"], ms["spectra"], ms["fk"]
        got = slant_maps(data[0], plan, norm=True)[:args.numpy_gathers].cpu().numpy()

        host = data[0][:args.numpy_gathers].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        want = np.stack([slant_ref.slant(h, DX, DT, freqs, vels, norm=True) for h in host])
        np_s = (time.perf_counter() - t0) / len(host)
        scale = want.reshape(len(host), -1).max(axis=1)
        err = float((np.abs(got - want).reshape(len(host), -1).max(axis=1) / scale).max())
        strict = int((got.argmax(axis=1) == want.argmax(axis=1)).sum())
        if not err <= 1e-6:
            raise SystemExit(f"{name}: the device images miss slant_ref by {err:.3e} of the image maximum")
        fmas = 4.0 * plan.n_row * B * plan.nF * plan.nV
        floor_ms = [fmas / (r * 1e12) * 1e3 for r in FP64_VALU_TFMA]
        res = {
            "metric": f"phase-shift dispersion, {name}: slant_maps of {B} gathers of 25 x 500 -> {plan.nV} x {plan.nF}",
            "value": call_ms[0], "unit": "ms/call", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "config": {"workload": f"slant_{name}", "B": B, "nch": 25, "nt": 500, "n_row": plan.n_row, "nF": plan.nF,
                       "nV": plan.nV, "n_fb": plan.n_fb, "nf": plan.nf, "buffer_sets": args.sets, "calls_per_sample": inner},
            "call": {"ms_median": call_ms[0], "ms_min": call_ms[1], "ms_max": call_ms[2]},
            "spectra": {"what": "dvh_disp_row_l1 + dvh_disp_tdft alone: call = spectra + launch",
                        "ms_median": spec_ms[0], "ms_min": spec_ms[1], "ms_max": spec_ms[2],
                        "call_minus_parts": call_ms[0] - spec_ms[0] - launch_ms[0]},
            "launch": {"ms_median": launch_ms[0], "ms_min": launch_ms[1], "ms_max": launch_ms[2], "fp64_fmas": fmas,
                       "achieved_tfma": fmas / (launch_ms[0] / 1e3) / 1e12, "floor_tfma": list(FP64_VALU_TFMA),
                       "floor_ms": floor_ms, "floor_share": [f / launch_ms[0] for f in floor_ms]},
            "numpy": {"what": "tests/slant_ref.slant (vectorised float64), one process on this host",
                      "version": np.__version__, "s_per_gather": np_s, "s_per_batch": np_s * B,
                      "speedup_call": np_s * B / (call_ms[0] / 1e3)},
            "fk": {"what": "fv_maps (time DFT + f-k contraction + sampling + savgol) on the same batch",
                   "ms_median": fk_ms[0], "ms_min": fk_ms[1], "ms_max": fk_ms[2], "slant_over_fk": call_ms[0] / fk_ms[0]},
            "parity": {"gathers": len(host), "max_err_of_image_max": err, "strict_picks": strict,
                       "picks": int(len(host) * plan.nF), "ok": True},
        }
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del data, outs, specs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
