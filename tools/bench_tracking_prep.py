#!/usr/bin/env python
"""Tracking-grid preprocessing of one continuous record on one MI355X (preprocess.tracking_preprocessing:
TimeLapseImaging._preprocess_for_tracking, apis/timeLapseImaging.py:74-102).

One step = one record of the prep workload's shape (1,024 channels x 15,000 samples, float64, resident on the device
before timing) -> data_for_tracking [8,356 x 3,000] float64 on the device:
  gate          dvh_median_abs_gate       radix select of median |x| per trace + the `*= 0` of loud traces
  cleanup       dvh_trace_cleanup         first empty trace imputed (flags 1, threshold 30)
  time_filter   dvh_sosfiltfilt_planned   0.08-1 Hz zero-phase band-pass, 1,024 rows x 15,000 (the block recursion)
  resample      dvh_resample_rows_t       204/25 polyphase along channels on every 5th sample, written transposed
  space_filter  dvh_sosfiltfilt_planned   0.006-0.04 1/m band-pass, 3,000 rows x 8,356 (the matrix form)
  transpose     dvh_transpose_f64         back to [8,356 x 3,000]
records/s is a host clock around `steps` whole calls (the float64 copy of the input included) ending in a device
synchronise; the stage times are HIP events on the launch stream, averaged over the same number of separately
synchronised calls.  The resampler is priced against HBM with its algorithmic bytes: one read of the 128-byte lines
its strided samples touch plus the write of the output.  The CPU figure is tests/tracking_ref.py (NumPy median, SciPy
sosfiltfilt and resample_poly: the reference's own calls) on the same record in this process, and the device result
is checked against it at the chain's bound, 1e-10 (max|after the time band-pass| + max|final|).

    python tools/bench_tracking_prep.py [--channels 1024] [--samples 15000] [--steps 50] [--warmup 3] [--no-cpu]
                                        [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from das_diff_veh_amd.preprocess import tracking_preprocessing  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip parameters
STAGES = ["gate", "cleanup", "time_filter", "resample", "space_filter", "transpose"]
LINE = 128


def record(n_ch, n_t, dt, seed=801):
    """Traffic-like record: 3 * standard_normal, Gaussian troughs of -60 moving at 8-20 m/s, a few loud traces
    (gated) and one dead trace (imputed), as multiples of 2**-8."""
    rng = np.random.default_rng(seed)
    x = 3.0 * rng.standard_normal((n_ch, n_t))
    t = np.arange(n_t) * dt
    pos = 8.16 * np.arange(n_ch)
    for _ in range(12):
        t0, v = rng.uniform(-400.0, t[-1]), rng.uniform(8.0, 20.0)
        x += -60.0 * np.exp(-0.5 * ((t[None, :] - t0 - pos[:, None] / v) / 0.25) ** 2)
    for r in rng.choice(n_ch, max(1, n_ch // 128), replace=False):
        x[r] = 40.0 * rng.standard_normal(n_t)
    x[n_ch // 3] = 0.0
    return np.round(x * 2 ** 8) / 2 ** 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=15000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU figure and the parity check")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tracking_prep needs the MI355X: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_ch, n_t, dt, x0, sub, up, down = args.channels, args.samples, 0.004, 449, 5, 204, 25
    host = record(n_ch, n_t, dt)
    data = torch.from_numpy(host).to(dev)

    for _ in range(args.warmup):
        out, dist, _ = tracking_preprocessing(data, dt, x0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out, dist, _ = tracking_preprocessing(data, dt, x0)
    torch.cuda.synchronize()
    step = (time.perf_counter() - t0) / args.steps

    ph, acc = {}, np.zeros(len(STAGES))
    for _ in range(args.steps):
        tracking_preprocessing(data, dt, x0, _phases=ph)
        torch.cuda.synchronize()
        names = ["start"] + STAGES
        acc += [ph[a].elapsed_time(ph[b]) for a, b in zip(names[:-1], names[1:])]
    stage_ms = acc / args.steps

    n_out, n_t_out = out.shape
    touched = n_ch * (n_t * 8 if sub * 8 <= LINE else n_t_out * LINE)
    rs_bytes = float(touched + n_out * n_t_out * 8)
    rs_s = stage_ms[STAGES.index("resample")] / 1e3
    res = {
        "metric": "tracking-grid preprocessing records/s (1,024 ch x 15,000 float64 -> 8,356 x 3,000 tracking grid)",
        "value": 1.0 / step, "unit": "records/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": step * 1e3, "dtype": "f64", "data": "synthetic traffic record, resident",
        "config": {"workload": "tracking_prep", "n_ch": n_ch, "n_t": n_t, "dt": dt, "subsamp_factor": sub, "up": up,
                   "down": down, "n_out": int(n_out), "n_t_out": int(n_t_out)},
        "stages_ms": {k: float(v) for k, v in zip(STAGES, stage_ms)},
        "stages_ms_sum": float(stage_ms.sum()),
        "resample_kernel": {"us": rs_s * 1e6, "bytes": rs_bytes, "achieved_gbs": rs_bytes / rs_s / 1e9,
                            "peak_gbs": HBM_PEAK_GBS, "frac": rs_bytes / rs_s / 1e9 / HBM_PEAK_GBS},
    }
    if not args.no_cpu:
        from tests import tracking_ref as tr
        t0 = time.perf_counter()
        ref = tr.tracking_ref(host, dt, x0, use_scipy_resample=True)
        cpu_s = time.perf_counter() - t0
        err = float(np.abs(out.cpu().numpy() - ref["out"]).max())
        bound = 1e-10 * float(np.abs(ref["bp"]).max() + np.abs(ref["out"]).max())
        res["cpu"] = {"what": "tests/tracking_ref.py (NumPy / SciPy, this process)", "s_per_record": cpu_s,
                      "records_per_s": 1.0 / cpu_s, "speedup": cpu_s / step}
        res["parity"] = {"max_abs_err": err, "bound": bound, "max_final": float(np.abs(ref["out"]).max()),
                         "ok": bool(err <= bound), "axes_equal": bool(np.array_equal(dist, ref["dist"])),
                         "gated": int(ref["gated"].size), "imputed": int(ref["imputed"])}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
