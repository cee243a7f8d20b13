#!/usr/bin/env python
"""Vehicle tracking of one continuous record on one MI355X (TimeLapseImaging.track_vehicles: KF_tracking,
apis/tracking.py, on the grid left by preprocess_for_tracking).

One step = the tracker on the 8,356 x 3,000 float64 tracking grid of a 1,024 channel x 60 s synthetic record with a
few dozen vehicles, start_x / end_x spanning the grid (2,786 tracked rows):
  detect_peaks  dvh_find_peaks_rows   15 rows from start_x
  likelihood    dvh_peak_likelihood   the detection curve
  bases         dvh_find_peaks_rows   the curve's peaks -> veh_base
  track_peaks   dvh_find_peaks_rows   every third row of the span, one launch
  kf            dvh_kf_track          association + Kalman loop, one thread per vehicle
  host_tail     remove_unrealistic_tracking + interp_nan_value on [n_veh, n_steps] (host clock)
The kernel times are HIP events on the launch stream, averaged over `steps` separately synchronised calls;
track_vehicles end to end is a host clock around `steps` calls (downloads and the host tail included), and
record_to_tracks adds preprocess_for_tracking to every call.  The peak kernel is stated beside the time of streaming
the rows it reads at the 6.4 TB/s HBM bound DESIGN.md uses; the Kalman kernel as latency per sequential step.  The CPU
figure is the tests/tracker_ref.py chain (scipy.signal.find_peaks per row, scipy.stats.norm.pdf, NumPy Kalman loop) on
the host copy of the same grid in this process, preceded by tests/tracking_ref.py for the raw-record ratio; the device
tracks are checked against it.

    python tools/bench_tracker.py [--channels 1024] [--samples 15000] [--steps 20] [--warmup 2] [--no-cpu] [--out FILE]
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

from das_diff_veh_amd.apis import tracking as dev_tracking  # noqa: E402
from das_diff_veh_amd.apis.timeLapseImaging import DEFAULT_TRACKING_PARAM, TimeLapseImaging  # noqa: E402

HBM_BOUND_GBS = 6400.0  # DESIGN.md's achievable-HBM bound
STAGES = [("detect_peaks", "detect_start", "detect_peaks"), ("likelihood", "detect_peaks", "likelihood"),
          ("bases", "likelihood", "bases"), ("track_peaks", "track_start", "track_peaks"), ("kf", "kf_start", "kf")]


def record(n_ch, n_t, dt, n_veh=40, seed=802):
    """Traffic-like record: 0.5 * standard_normal plus the quasi-static troughs (-6, 0.6 s wide: inside the tracking
    bands in time and in space) of 40 vehicles moving at 12-25 m/s along the 8.16 m channels, spread so that a few
    dozen are on the fibre during the record; multiples of 2**-8.  A vehicle covers at most 1.5 km of the 8.4 km
    fibre in the 60 s, so over the whole span every one is judged short-lived; tracks survive on a 600 m span."""
    rng = np.random.default_rng(seed)
    x = 0.5 * rng.standard_normal((n_ch, n_t))
    t = np.arange(n_t) * dt
    pos = 8.16 * np.arange(n_ch)
    for k in range(n_veh):
        v = rng.uniform(12.0, 25.0)
        t0 = -pos[-1] / v + (t[-1] + pos[-1] / v) * (k + rng.uniform(0.2, 0.8)) / n_veh
        x += -6.0 * np.exp(-0.5 * ((t[None, :] - t0 - pos[:, None] / v) / 0.6) ** 2)
    return np.round(x * 2 ** 8) / 2 ** 8


class _Obj(TimeLapseImaging):
    """TimeLapseImaging without the imaging preprocessing, which this benchmark does not time."""

    def _preprocessing_for_surface_waves(self, *a, **k):
        self.data_for_imaging = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=15000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU figure and the parity check")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tracker needs the MI355X: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_ch, n_t, dt = args.channels, args.samples, 0.004
    host = record(n_ch, n_t, dt)
    x_axis, t_axis = 449 + np.arange(n_ch), np.arange(n_t) * dt
    obj = _Obj(torch.from_numpy(host).to(dev), x_axis, t_axis)
    obj.preprocess_for_tracking()
    dist = obj.dist_along_fiber_tracking
    start_x, end_x = dist[0], dist[-1]
    n_x, n_tt = obj.data_for_tracking.shape

    def sync_time(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    def from_record():
        obj.preprocess_for_tracking()
        obj.track_vehicles(start_x, end_x)

    for _ in range(args.warmup):
        tracks = obj.track_vehicles(start_x, end_x)
    e2e = sync_time(lambda: obj.track_vehicles(start_x, end_x), args.steps)
    rec2trk = sync_time(from_record, args.steps)
    prep = sync_time(obj.preprocess_for_tracking, args.steps)

    trk = obj.tracking
    acc, tail = np.zeros(len(STAGES)), 0.0
    for _ in range(args.steps):
        ev = {}
        base = trk.detect_in_one_section(start_x, nx=15, sigma=0.08, _events=ev)
        trk.tracking_with_veh_base(start_x, end_x, base, _events=ev)
        torch.cuda.synchronize()
        acc += [ev[a].elapsed_time(ev[b]) for _, a, b in STAGES]
        t0 = time.perf_counter()
        kept = dev_tracking.remove_unrealistic_tracking(trk.veh_states_raw)
        full = np.full((kept.shape[0], kept.shape[1] * 3), np.nan)
        full[:, ::3] = kept
        dev_tracking.interp_nan_value(full)
        tail += time.perf_counter() - t0
    stage_ms = dict(zip([s[0] for s in STAGES], (acc / args.steps).tolist()))
    stage_ms["host_tail"] = tail / args.steps * 1e3

    n_steps = trk.veh_states_raw.shape[1]
    n_peaks = int(trk.row_counts.sum().cpu())
    row_bytes = float(n_steps * n_tt * 8)
    pk_s = stage_ms["track_peaks"] / 1e3
    res = {
        "metric": "vehicle tracking records/s (8,356 x 3,000 float64 tracking grid -> tracks, on the device)",
        "value": 1.0 / e2e, "unit": "records/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": e2e * 1e3, "dtype": "f64", "data": "synthetic traffic record, grid resident",
        "config": {"workload": "tracker", "n_ch": n_ch, "n_t": n_t, "dt": dt, "grid": [int(n_x), int(n_tt)],
                   "n_steps": int(n_steps), "detect": DEFAULT_TRACKING_PARAM["detect"], "nx": 15, "sigma": 0.08,
                   "sigma_a": 0.01},
        "found": {"veh_base": int(len(base)), "tracks": int(tracks.shape[0]), "row_peaks": n_peaks,
                  "row_peaks_max": int(trk.row_counts.max().cpu())},
        "stages_ms": stage_ms,
        "track_vehicles_ms": e2e * 1e3, "preprocess_for_tracking_ms": prep * 1e3,
        "record_to_tracks_ms": rec2trk * 1e3,
        "peak_kernel": {"us": pk_s * 1e6, "row_bytes": row_bytes, "stream_us_at_bound": row_bytes / HBM_BOUND_GBS / 1e3,
                        "bound_gbs": HBM_BOUND_GBS, "achieved_gbs": row_bytes / pk_s / 1e9,
                        "us_per_row": pk_s * 1e6 / n_steps},
        "kf_kernel": {"us": stage_ms["kf"] * 1e3, "n_steps": int(n_steps), "n_veh": int(len(base)),
                      "us_per_step": stage_ms["kf"] * 1e3 / n_steps},
    }
    if not args.no_cpu:
        from tests import tracker_ref as kr
        from tests import tracking_ref as tr
        grid = -obj.data_for_tracking.cpu().numpy()   # reverse_amp, as the reference forms it
        tt = np.asarray(obj.t_axis_tracking)
        detect = DEFAULT_TRACKING_PARAM["detect"]

        def compare(sx, ex):
            """Device against the CPU chain on the same grid and span.  Where two equally high peaks of the detection
            curve compete under the distance rule (two vehicles seen on one row each give the same norm.pdf maximum),
            SciPy's pick follows np.argsort's unstable order and the kernel's the larger index: `detection_tie` says
            so, and veh_base may then differ."""
            b = trk.detect_in_one_section(sx, nx=15, sigma=0.08)
            got = trk.tracking_with_veh_base(sx, ex, b)
            t0 = time.perf_counter()
            rb, erode, _ = kr.detect(grid, tt, dist, sx, detect, 15, 0.08)
            ref, raw, _ = kr.track(grid, tt, dist, sx, ex, rb, detect)
            cpu_s = time.perf_counter() - t0
            base_eq = bool(np.array_equal(b, rb))
            raw_eq = bool(base_eq and np.array_equal(trk.veh_states_raw, raw, equal_nan=True))
            same = got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
            err = float(np.abs(got - ref).max()) if same and got.size else (0.0 if same else float("nan"))
            tie = not kr.distance_order_free(erode, detect["minseparation"])
            return cpu_s, {"veh_base": int(len(rb)), "tracks": int(ref.shape[0]), "detection_tie": bool(tie),
                           "veh_base_equal": base_eq,
                           "veh_states_raw_equal": raw_eq, "tracks_same_shape_and_nan": bool(same),
                           "tracks_max_abs_err": err, "ok": bool(base_eq and raw_eq and same and err <= 1e-9)}

        cpu_trk, full = compare(start_x, end_x)
        _, part = compare(dist[3000], dist[3600])
        t0 = time.perf_counter()
        tr.tracking_ref(host, dt, x_axis[0], use_scipy_resample=True)
        cpu_prep = time.perf_counter() - t0
        res["cpu"] = {"what": "tests/tracker_ref.py after tests/tracking_ref.py (NumPy / SciPy, this process)",
                      "tracker_s": cpu_trk, "prep_s": cpu_prep, "tracker_speedup": cpu_trk / e2e,
                      "record_to_tracks_speedup": (cpu_trk + cpu_prep) / rec2trk}
        res["parity"] = {"whole_span": full, "span_3000_3600": part,
                         "ok": bool(part["ok"] and (full["ok"] or full["detection_tie"]))}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
