#!/usr/bin/env python
"""Vehicle classes on one MI355X: the quasi-static curves and peaks of every pass (classes.quasi_static_curves ->
dvh_qs_curves; imaging_diff_speed.ipynb#cell5, imaging_diff_weight.ipynb#cell7-8).

One JSON line per case:
  batch    2 108 passes x 49 channels x 1 500 samples resident on the device, float64 and float32 (the notebooks' data)
  record   the same number of passes read from a resident record through the row table (rows start at every element
           alignment and overlap between passes), float64 and float32
  class    60 passes, the bootstrap class size
Each line holds
  call      ms per dvh_qs_curves call (its three launches) by HIP events on the launch stream around `steps`
            back-to-back calls after `warmup`; the batch cases rotate through copies of the states totalling more than
            twice the 256 MB Infinity Cache where one copy does not exceed it already
  frac      the call's share of the 8 TB/s HBM peak on its algorithmic bytes: one read of the states and one write of
            the curves (a record's rows overlap, so its algorithmic bytes are the rows', as if gathered)
  notebook  the notebooks' per-pass loop (mean, savgol_filter, detrend, shift, then the peaks) in this process on the
            same arrays, or on the first `--cpu-passes` of them scaled to all
  parity    device curves against the NumPy restatement (tests/classes_ref.py) within its derived bound on the first
            passes; a case that misses it prints no line and the tool exits non-zero

    python tools/bench_classes.py [--steps 20] [--warmup 3] [--cpu-passes 200] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from das_diff_veh_amd import _lib  # noqa: E402
from das_diff_veh_amd.preprocess import _savgol_device  # noqa: E402
from tests import classes_ref  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip parameters
ROTATE_BYTES = 600 << 20
N_CH, N_T = 49, 1500
CASES = [("batch", 2108, np.float64), ("batch", 2108, np.float32), ("record", 2108, np.float64),
         ("record", 2108, np.float32), ("class", 60, np.float64), ("class", 60, np.float32)]


def states_on_device(n_pass, dtype, dev, seed=11):
    """[n_pass, N_CH, N_T] troughs plus noise and drift, generated on the device, multiples of 2**-8."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    t = torch.arange(N_T, device=dev, dtype=torch.float64)
    depth = 0.5 + 5.0 * torch.rand((n_pass, 1, 1), generator=g, device=dev, dtype=torch.float64)
    x = -depth * torch.exp(-((t - N_T / 2) / 150.0) ** 2) + 0.3 * torch.randn((n_pass, N_CH, N_T), generator=g,
                                                                             device=dev, dtype=torch.float64)
    x += torch.rand((n_pass, N_CH, 1), generator=g, device=dev, dtype=torch.float64) * t / N_T
    return (torch.round(x * 256) / 256).to(torch.float32 if dtype == np.float32 else torch.float64)


def record_case(n_pass, dtype, dev, seed=12):
    """A record [N_CH + 8, rec_n_t] and a row table: pass p starts 41 samples after pass p - 1 (the passes overlap)
    and row c another c samples later (every alignment)."""
    rec_n_t = 41 * n_pass + N_T + N_CH + 64
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rec = torch.round(torch.randn((N_CH + 8, rec_n_t), generator=g, device=dev, dtype=torch.float64) * 256) / 256
    rec = rec.to(torch.float32 if dtype == np.float32 else torch.float64)
    t_start = 41 * np.arange(n_pass)[:, None] + np.arange(N_CH)[None, :]
    off = (4 + np.arange(N_CH))[None, :] * rec_n_t + t_start
    assert off.max() + N_T <= rec.numel()
    return rec, off


def time_calls(xs, offs, n_pass, steps, warmup, dev):
    h, el, er = _savgol_device(101, 3, dev)
    curves = [torch.empty((n_pass, N_T), dtype=torch.float64, device=dev) for _ in xs]
    peaks = torch.empty(n_pass, dtype=torch.float64, device=dev)
    status = torch.zeros(n_pass, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().dvh_qs_curves_workspace(n_pass, N_T) // 8, dtype=torch.float64, device=dev)
    st = _lib.stream_of(dev)

    def launch(k):
        i = k % len(xs)
        _lib.call("dvh_qs_curves", _lib.ptr(xs[i]), 0 if xs[i].dtype == torch.float32 else 1, _lib.ptr(offs[i]), n_pass,
                  N_CH, N_T, _lib.ptr(h), 101, _lib.ptr(el), _lib.ptr(er), _lib.ptr(curves[i]), N_T, _lib.ptr(peaks),
                  _lib.ptr(status), _lib.ptr(ws), st)

    for k in range(max(warmup, len(xs))):
        launch(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(steps):
        launch(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps, curves[0], int(status.sum().cpu())


def notebook_loop(states):
    """The cells' own loop, timed."""
    t0 = time.perf_counter()
    means = []
    for das_veh in states:
        tmp = scipy.signal.detrend(scipy.signal.savgol_filter(das_veh.mean(0), 101, 3))
        means.append(tmp - tmp[0])
    np.max(np.abs(means), 1)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-passes", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classes needs the MI355X: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    op = classes_ref.operator(101, 3)
    lines = []
    for kind, n_pass, dtype in CASES:
        esz = np.dtype(dtype).itemsize
        state_bytes = n_pass * N_CH * N_T * esz
        if kind == "record":
            rec, off = record_case(n_pass, dtype, dev)
            xs, offs = [rec], [torch.from_numpy(off).to(dev)]
            n_chk = 4
            r = rec.cpu().numpy().reshape(-1)
            host = np.stack([np.stack([r[off[p, c]:off[p, c] + N_T] for c in range(N_CH)])
                             for p in range(max(n_chk, min(args.cpu_passes, n_pass)))])
            resident = rec.numel() * esz
        else:
            n_copies = 1 if kind == "class" else max(1, -(-ROTATE_BYTES // state_bytes))
            xs = [states_on_device(n_pass, dtype, dev, seed=11 + k) for k in range(n_copies)]
            o = torch.arange(n_pass * N_CH, dtype=torch.int64, device=dev) * N_T
            offs = [o] * n_copies
            n_chk = 4
            host = xs[0][:max(n_chk, min(args.cpu_passes, n_pass))].cpu().numpy()
            resident = state_bytes * n_copies
        ms, curves, n_bad = time_calls(xs, offs, n_pass, args.steps, args.warmup, dev)
        want, _ = classes_ref.curves(host[:n_chk].astype(np.float64), *op)
        err = float(np.abs(curves[:n_chk].cpu().numpy() - want).max())
        tol = classes_ref.bound(N_T, *op, float(np.abs(host[:n_chk]).max()))
        if not err <= tol or n_bad:
            raise SystemExit(f"{kind} {n_pass} {np.dtype(dtype).name}: device curves miss classes_ref by {err:.3e}")
        n_cpu = min(args.cpu_passes, n_pass, host.shape[0])
        cpu_s = notebook_loop([h.astype(np.float64) for h in host[:n_cpu]]) * n_pass / n_cpu
        nbytes = float(state_bytes + n_pass * N_T * 8)
        gbs = nbytes / (ms / 1e3) / 1e9
        res = {
            "metric": "quasi-static curves and peaks of every pass (dvh_qs_curves: mean, savgol(101, 3), detrend)",
            "value": ms * 1e3, "unit": "us/call", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "config": {"workload": "classes", "case": kind, "n_pass": n_pass, "n_ch": N_CH, "n_t": N_T,
                       "dtype": np.dtype(dtype).name},
            "call": {"us": ms * 1e3, "algorithmic_bytes": nbytes, "achieved_gbs": gbs, "peak_gbs": HBM_PEAK_GBS,
                     "frac": gbs / HBM_PEAK_GBS, "resident_bytes": resident, "buffers_rotated": len(xs)},
            "notebook": {"what": "per pass: detrend(savgol_filter(d.mean(0), 101, 3)) - first sample; then the peaks "
                                 "(this process, float64)", "scipy": scipy.__version__, "passes_timed": n_cpu,
                         "s_for_all_passes": cpu_s, "speedup": cpu_s / (ms / 1e3)},
            "parity": {"max_abs_err": err, "bound": tol, "passes_checked": n_chk, "ok": True},
        }
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del xs, offs, curves
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
