#!/usr/bin/env python
"""Welch power spectra on one MI355X: win_avg_psd's class spectrum and a gather's PSD vs offset (dvh_welch_rows).

Two JSON lines:
  class    one vehicle class of the 700_speeds size, 2 108 windows x 60 rows x 5 500 samples float32 (2.78 GB, eleven
           times the 256 MB Infinity Cache, so every launch streams its windows from HBM without rotating buffers), at
           nperseg = nfft = 2048: 4 segments per row.
             kernel   HIP events around `steps` back-to-back launches on resident windows after `warmup`; priced against
                      the 8 TB/s HBM peak with its algorithmic bytes: every sample of a row's segments read once (the
                      380-sample tail past the last full segment is never needed) plus the [windows, 1025] float64 output
             host     modules.utils.win_avg_psd on NumPy float32 windows, staging and H2D included, one call after a
                      small warm-up call
             scipy    the reference's double loop of scipy.signal.welch over `--scipy-windows` of the windows in this
                      process, and that time scaled to the class
             parity   the device spectra of those windows against tests/psd_ref within 1e-5 of the row maximum, else no
                      line and a non-zero exit
  gather   one 49 x 500 gather at nperseg 256 / nfft 1024 (cache-resident: 98 kB): the launch, and psd_vs_offset from
           the host gather to the cropped host arrays.

    python tools/bench_psd.py [--steps 10] [--warmup 2] [--windows 2108] [--scipy-windows 4] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import numpy as np
import scipy
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from das_diff_veh_amd.apis.virtual_shot_gather import psd_vs_offset  # noqa: E402
from das_diff_veh_amd.modules.utils import win_avg_psd  # noqa: E402
from das_diff_veh_amd.spectra import welch_plan, welch_rows  # noqa: E402
from tests import psd_ref  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip parameters
FS, ROWS, N_T, NPERSEG = 250, 60, 5500, 2048


def launch_ms(x, plan, steps, warmup):
    out = torch.empty((x.shape[0], plan.bins), dtype=torch.float64, device=x.device)
    for _ in range(warmup):
        welch_rows(x, FS, plan=plan, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        welch_rows(x, FS, plan=plan, out=out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps, out


def scipy_loop(windows):
    """The body of the reference's win_avg_psd (modules/utils.py:715-728) on host windows."""
    out = []
    for w in windows:
        acc = 0.0
        for j in range(w.shape[0]):
            acc = acc + scipy.signal.welch(w[j, :], FS, nperseg=NPERSEG)[1]
        out.append(acc / w.shape[0])
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=2108)
    ap.add_argument("--scipy-windows", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_psd needs the MI355X: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    # ---- class
    n_win = args.windows
    rng = np.random.default_rng(7)
    distinct = [rng.standard_normal((ROWS, N_T)).astype(np.float32) for _ in range(min(n_win, 128))]
    hosts = [distinct[i % len(distinct)] for i in range(n_win)]       # 169 MB of distinct host windows, cycled
    plan = welch_plan(N_T, FS, NPERSEG)
    x = torch.stack([torch.from_numpy(h) for h in distinct]).to(dev)
    x = x.repeat(-(-n_win // len(distinct)), 1, 1)[:n_win].contiguous()
    ms, out = launch_ms(x, plan, args.steps, args.warmup)
    k = args.scipy_windows
    want = psd_ref.welch(np.stack(hosts[:k]), FS, NPERSEG)[1].mean(axis=1)
    got = out[:k].cpu().numpy()
    err = float((np.abs(got - want).max(axis=1) / want.max(axis=1)).max())
    if not err <= 1e-5:
        raise SystemExit(f"class spectra miss psd_ref by {err:.3e} of the row maximum")
    used = plan.nseg * plan.step + plan.noverlap
    nbytes = 4.0 * n_win * ROWS * used + 8.0 * n_win * plan.bins
    gbs = nbytes / (ms / 1e3) / 1e9
    wins = [types.SimpleNamespace(data=h) for h in hosts]
    win_avg_psd(wins[:64], FS, NPERSEG)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f, avg, pxxs = win_avg_psd(wins, FS, NPERSEG)
    host_s = time.perf_counter() - t0
    if not np.array_equal(pxxs[:k], got):
        raise SystemExit("win_avg_psd and the resident launch disagree")
    t0 = time.perf_counter()
    sp = scipy_loop(hosts[:k])
    sp_s = (time.perf_counter() - t0) / k
    res = {
        "metric": "class source spectrum: win_avg_psd, nperseg 2048 (dvh_welch_rows)", "value": ms, "unit": "ms/class",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "config": {"workload": "psd_class", "windows": n_win, "rows": ROWS, "n_t": N_T, "nperseg": NPERSEG,
                   "nfft": plan.nfft, "nseg": plan.nseg, "samples_used_per_row": used, "input_bytes": 4.0 * x.numel()},
        "kernel": {"ms": ms, "bytes": nbytes, "achieved_gbs": gbs, "peak_gbs": HBM_PEAK_GBS, "frac": gbs / HBM_PEAK_GBS},
        "host": {"what": "win_avg_psd on NumPy float32 windows, staging and H2D included", "s": host_s},
        "scipy": {"what": f"scipy.signal.welch per row, {k} windows in this process, scaled to the class",
                  "version": scipy.__version__, "s_per_window": sp_s, "s_per_class": sp_s * n_win,
                  "speedup_kernel": sp_s * n_win / (ms / 1e3), "speedup_host": sp_s * n_win / host_s,
                  "float32_vs_device": float((np.abs(sp - got).max(axis=1) / got.max(axis=1)).max())},
        "parity": {"max_err_of_row_max": err, "ok": True},
    }
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    del x, out, wins, hosts

    # ---- gather
    g = rng.standard_normal((49, 500))
    g = np.round(g * 256) / 256
    t_axis = np.arange(500) * 0.003999999999997783
    x_axis = (np.arange(49) - 24) * 8.16
    gd = torch.from_numpy(g.astype(np.float32)).to(dev)
    gplan = welch_plan(500, 250, 256, 1024)
    gms, gout = launch_ms(gd, gplan, 200, 20)
    gerr = float((np.abs(gout.cpu().numpy() - psd_ref.welch(g, 250, 256, 1024)[1]).max(axis=1)
                  / psd_ref.welch(g, 250, 256, 1024)[1].max(axis=1)).max())
    if not gerr <= 1e-5:
        raise SystemExit(f"gather spectra miss psd_ref by {gerr:.3e}")
    psd_vs_offset(g, x_axis, t_axis)
    t0 = time.perf_counter()
    for _ in range(20):
        psd_vs_offset(g, x_axis, t_axis)
    e2e = (time.perf_counter() - t0) / 20
    t0 = time.perf_counter()
    for _ in range(20):
        scipy.signal.welch(g, 250, nperseg=256, nfft=1024)
    sp_g = (time.perf_counter() - t0) / 20
    gbytes = 4.0 * 49 * (gplan.nseg * gplan.step + gplan.noverlap) + 8.0 * 49 * gplan.bins
    res = {
        "metric": "gather PSD vs offset: welch(nperseg 256, nfft 1024) per row (dvh_welch_rows)", "value": gms * 1e3,
        "unit": "us/launch", "n_gpus": 1, "steps": 200, "warmup": 20,
        "config": {"workload": "psd_gather", "rows": 49, "n_t": 500, "nperseg": 256, "nfft": 1024, "nseg": gplan.nseg},
        "kernel": {"us": gms * 1e3, "bytes": gbytes, "achieved_gbs": gbytes / (gms / 1e3) / 1e9,
                   "peak_gbs": HBM_PEAK_GBS, "frac": gbytes / (gms / 1e3) / 1e9 / HBM_PEAK_GBS,
                   "note": "49 blocks of one active wave: launch-latency bound, cache-resident"},
        "host": {"what": "psd_vs_offset from the host gather to the cropped host arrays", "us": e2e * 1e6},
        "scipy": {"what": "scipy.signal.welch(gather, 250, nperseg=256, nfft=1024), batched, this process",
                  "us": sp_g * 1e6},
        "parity": {"max_err_of_row_max": gerr, "ok": True},
    }
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
