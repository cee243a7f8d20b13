#!/usr/bin/env python
"""Record ingest on one MI355X: ImagingIO's smoothing and scaling (preprocess.savgol_smooth -> dvh_savgol_rows,
modules/imaging_IO.py:44-46) and the records/s of ImagingIO itself from files.

Per shape (1,024 x 15,000 float64 and float32: the prep workload's record; 140 x 15,000 float32: the reference's
default ch1 = 400, ch2 = 540) one JSON line:
  kernel      dvh_savgol_rows(21, 15, divisor 6463.8...) on resident records into resident outputs, HIP events on
              the launch stream around `steps` back-to-back launches after `warmup`; the launches rotate through
              copies of the record and output buffers totalling more than 600 MB, over twice the 256 MB Infinity
              Cache, so that the figure is an HBM one; priced against the 8 TB/s HBM peak with its algorithmic
              bytes, one read and one write of the record
  scipy       scipy.signal.savgol_filter(x, 21, 15) followed by the divide, on the same record in this process
  parity      the device output against the NumPy restatement (tests/ingest_ref.smooth): 1e-13 max|x| (float64) or
              one float32 ulp; a shape that misses it prints no line and the tool exits non-zero
  files       records/s of ``for data, x, t in ImagingIO(...)`` over `n_files` copies of the record written to a
              temporary directory (np.savez, uncompressed), prefetch 0 and 1, ending in a device synchronise: file
              reading and the host copy dominate it

    python tools/bench_ingest.py [--steps 50] [--warmup 5] [--n-files 6] [--no-files] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from das_diff_veh_amd import _lib  # noqa: E402
from das_diff_veh_amd.modules.imaging_IO import SCALE, ImagingIO  # noqa: E402
from das_diff_veh_amd.preprocess import _savgol_device, savgol_smooth  # noqa: E402
from tests import ingest_ref  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip parameters
SHAPES = [(1024, 15000, np.float64), (1024, 15000, np.float32), (140, 15000, np.float32)]


def record(n_ch, n_t, dtype, seed=901):
    rng = np.random.default_rng(seed)
    x = 3.0 * rng.standard_normal((n_ch, n_t)) + np.cumsum(rng.standard_normal((n_ch, n_t)), axis=-1) * 0.1
    return (np.round(x * 2 ** 8) / 2 ** 8).astype(dtype)


ROTATE_BYTES = 600 << 20  # more than twice the 256 MB Infinity Cache: no launch finds its record or output cached


def kernel_ms(x, steps, warmup):
    """ms per launch over `steps` launches that rotate through enough (record, output) pairs to exceed ROTATE_BYTES,
    so that every launch reads its record from HBM and writes to lines no earlier launch left in a cache; and the
    output of the first pair."""
    dev = x.device
    h, el, er = _savgol_device(21, 15, dev)
    n_pairs = max(2, -(-ROTATE_BYTES // (2 * x.numel() * x.element_size())))
    xs = [x] + [x.clone() for _ in range(n_pairs - 1)]
    ys = [torch.empty_like(x) for _ in range(n_pairs)]
    dt = 0 if x.dtype == torch.float32 else 1

    def launch(k):
        xi, yi = xs[k % n_pairs], ys[k % n_pairs]
        _lib.call("dvh_savgol_rows", _lib.ptr(xi), dt, xi.shape[0], xi.stride(0), xi.shape[1], _lib.ptr(h), 21,
                  _lib.ptr(el), _lib.ptr(er), SCALE, _lib.ptr(yi), yi.stride(0), _lib.stream_of(dev))

    for k in range(max(warmup, n_pairs)):
        launch(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(steps):
        launch(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps, ys[0], n_pairs


def files_rate(host, n_files, prefetch, root):
    io = ImagingIO("20230301", root, ch1=0, ch2=host.shape[0], prefetch=prefetch)
    for _ in io:  # warm-up: page cache, pinned buffers, the operator's device copy
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for data, _, _ in io:
        n += 1
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-files", type=int, default=6)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest needs the MI355X: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    op = ingest_ref.operator(21, 15)
    lines = []
    for n_ch, n_t, dtype in SHAPES:
        host = record(n_ch, n_t, dtype)
        x = torch.from_numpy(host).to(dev)
        ms, y, n_pairs = kernel_ms(x, args.steps, args.warmup)
        got = y.cpu().numpy()
        want = ingest_ref.smooth(host, *op, SCALE)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        tol = ingest_ref.ulp32(want) if dtype == np.float32 else 1e-13 * float(np.abs(host).max()) / SCALE
        if not np.all(err <= tol) or not np.array_equal(savgol_smooth(host, divisor=SCALE), got):
            raise SystemExit(f"{n_ch} x {n_t} {np.dtype(dtype).name}: device output misses ingest_ref by {err.max():.3e}")
        t0 = time.perf_counter()
        sp = scipy.signal.savgol_filter(host, 21, 15)
        sp /= SCALE
        cpu_s = time.perf_counter() - t0
        nbytes = 2.0 * host.nbytes
        gbs = nbytes / (ms / 1e3) / 1e9
        res = {
            "metric": "record smoothing: savgol_filter(21, 15) + scale, one pass (dvh_savgol_rows)",
            "value": ms * 1e3, "unit": "us/record", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "config": {"workload": "ingest", "n_ch": n_ch, "n_t": n_t, "dtype": np.dtype(dtype).name},
            "kernel": {"us": ms * 1e3, "bytes": nbytes, "achieved_gbs": gbs, "peak_gbs": HBM_PEAK_GBS,
                       "frac": gbs / HBM_PEAK_GBS, "rotated_pairs": n_pairs, "rotated_bytes": n_pairs * nbytes},
            "scipy": {"what": "scipy.signal.savgol_filter(x, 21, 15); x /= scale (this process)", "version":
                      scipy.__version__, "s_per_record": cpu_s, "speedup": cpu_s / (ms / 1e3)},
            "parity": {"max_abs_err": float(err.max()), "edge_vs_scipy": float(np.abs(
                got[:, :10].astype(np.float64) - sp[:, :10]).max() * SCALE / np.abs(host).max()), "ok": True},
        }
        if not args.no_files:
            with tempfile.TemporaryDirectory() as root:
                os.makedirs(os.path.join(root, "20230301"))
                for k in range(args.n_files):
                    np.savez(os.path.join(root, "20230301", f"20230301_00{k:02d}00.npz"), data=host,
                             x_axis=np.arange(n_ch + 1.0), t_axis=np.arange(n_t) * 0.004)
                res["files"] = {"n_files": args.n_files, "records_per_s_prefetch0": files_rate(host, args.n_files, 0, root),
                                "records_per_s_prefetch1": files_rate(host, args.n_files, 1, root)}
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
