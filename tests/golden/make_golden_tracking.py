"""Generate the tracking-grid preprocessing fixture by running the REFERENCE's
TimeLapseImaging._preprocess_for_tracking (apis/timeLapseImaging.py:74-102) where the reference is installed
(the same place make_golden.py runs; never on the GPU box):

    python tests/golden/make_golden_tracking.py

Only data leaves this script.  The fixture is split so that every file stays under 1 MiB:
  tracking_prep.npz              dt, x_axis, t_axis and per case <case>_in (float32, multiples of 2**-8), <case>_dist,
                                 <case>_t_axis_tracking, <case>_gated, <case>_imputed
  tracking_prep_<case>.npz       data_for_tracking of the case (196 x 300 float64)
  tracking_prep_loud_stages.npz  case `loud`: bp (after the time band-pass, 24 x 1500) and rs (resampled, before the
                                 spatial band-pass, 196 x 300)
The reference runs on the float64 values of the stored float32 inputs.
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import scipy
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden import import_reference  # noqa: E402

CASES = ["plain", "loud", "dead_first_loud", "two_loud_last"]
N_CH, N_T, DT = 24, 1500, 0.004


def records():
    """24 ch x 1 500 samples: three moving Gaussian troughs of -60 (width 0.25 s; 12, 15 and 10 m/s along the 8.16 m
    channels) + 3 * standard_normal, rounded to multiples of 2**-8; the cases change whole traces."""
    rng = np.random.default_rng(800)
    t = np.arange(N_T) * DT
    x = 8.16 * np.arange(N_CH)
    base = 3.0 * rng.standard_normal((N_CH, N_T))
    for t0, v in ((0.5, 12.0), (-4.0, 15.0), (-7.0, 10.0)):
        base += -60.0 * np.exp(-0.5 * ((t[None, :] - t0 - x[:, None] / v) / 0.25) ** 2)

    def loud():
        return 40.0 * rng.standard_normal(N_T)

    out = {}
    for name in CASES:
        d = base.copy()
        if name == "loud":
            d[9] = loud()
        elif name == "dead_first_loud":
            d[0] *= 0
            d[17] = loud()
        elif name == "two_loud_last":
            d[5] = loud()
            d[23] = loud()
        out[name] = (np.round(d * 2 ** 8) / 2 ** 8).astype(np.float32)
    return out


def main():
    ref = import_reference()
    import apis.timeLapseImaging as tli
    meta = np.array(repr(dict(numpy=np.__version__, scipy=scipy.__version__)))
    x_axis = 449 + np.arange(N_CH)
    t_axis = np.arange(N_T) * DT
    head = dict(dt=np.array(DT), x_axis=x_axis, t_axis=t_axis, meta=meta)
    files = {}
    for name, q in records().items():
        data = q.astype(np.float64)
        assert np.array_equal(data.astype(np.float32), q)
        obj = types.SimpleNamespace(data=data.copy(), dt=DT, t_axis=t_axis, x_axis=x_axis,
                                    tracking_preprecessing_dict={})
        tli.TimeLapseImaging._preprocess_for_tracking(obj)
        assert obj.data_for_tracking.dtype == np.float64 and np.array_equal(obj.data, data)
        # the stages again, with the reference's helpers, for the fixture facts and the intermediates
        d = data.copy()
        means = np.median(np.abs(d), axis=-1)
        d[means > 10] *= 0
        idx = ref.ut.find_noise_idx(d, noise_threshold=30, empty_tr=True)
        ref.ut.impute_noisy_trace(d, idx)
        ref.ut.bandpass_data(d, DT, 0.08, 1)
        rs = scipy.signal.resample_poly(d[:, ::5], 204, 25)
        fin = rs.copy()
        ref.ut.bandpass_data_space(fin, obj.dist_along_fiber_tracking, 0.006, 0.04)
        assert np.array_equal(fin, obj.data_for_tracking)
        head[name + "_in"] = q
        head[name + "_dist"] = obj.dist_along_fiber_tracking
        head[name + "_t_axis_tracking"] = obj.t_axis_tracking
        head[name + "_gated"] = np.flatnonzero(means > 10).astype(np.int64)
        head[name + "_imputed"] = np.array(int(idx))
        files[f"tracking_prep_{name}"] = dict(data_for_tracking=obj.data_for_tracking, meta=meta)
        if name == "loud":
            files["tracking_prep_loud_stages"] = dict(bp=d, rs=rs, meta=meta)
    files["tracking_prep"] = head
    for fname, out in files.items():
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}: {os.path.getsize(path) / 2 ** 20:.2f} MiB")
        assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
