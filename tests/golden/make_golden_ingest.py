"""Generate the record-ingest fixtures by running the REFERENCE's ImagingIO (modules/imaging_IO.py) where the
reference is installed (the same place make_golden.py runs; never on the GPU box):

    python tests/golden/make_golden_ingest.py

Every case writes two small .npz records into a temporary ``root/<date>/<%Y%m%d_%H%M%S>.npz`` tree and reads them
back through the reference's ImagingIO(date, root, ch1, ch2, smoothing).  The records are multiples of 2**-8 (exact in
float32) or int16 counts; 15 channels 396 .. 410 of which ch1 = 398, ch2 = 410 keep 12; the time axis starts at
-TAPER * dt, so that _cut_taper drops TAPER samples from both ends.

One file per case, tests/golden/ingest_<case>.npz, each under 1 MiB:
  date, ch1, ch2, smoothing, names        the folder, ImagingIO's arguments and the two file names
  data_k, x_axis_k, t_axis_k              what file k holds
  out_k, out_x_k, out_t_k                 the reference's (data, x_axis, t_axis) of imagingIO[k]
  time_interval                           get_time_interval()
  h, el, er                               SciPy's (21, 15) maps as tests/ingest_ref.operator forms them here
  edge_noise                              max |reference - ingest_ref| over the edge samples (the first and last 10 of
                                          every row) / max |x|, measured here: SciPy fits the edges of all rows in one
                                          ill-conditioned lstsq, which no linear operator reproduces
A case whose interior samples differ from ingest_ref by more than 1e-13 max|x| (float64, int16) or one float32 ulp
(float32) is not written.
"""
from __future__ import annotations

import os
import sys
import tempfile

sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import ingest_ref  # noqa: E402
from tests.golden.make_golden import import_reference  # noqa: E402

TAPER = 5
DT = 0.004
CH = np.arange(396, 411)
CH1, CH2 = 398, 410
NAMES = ("{date}_000000.npz", "{date}_000100.npz")

# name -> (date folder, dtype, smoothing, lengths after the taper cut of the two files, seed)
CASES = {
    "f32_scaled": ("20230301", np.float32, True, (3000, 22), 1),
    "f64_plain": ("20221202", np.float64, True, (3001, 21), 2),
    "i16_scaled": ("20230301", np.int16, True, (21, 300), 3),
    "f32_raw_scaled": ("20230301", np.float32, False, (22, 64), 4),
    "f64_raw_plain": ("20221202", np.float64, False, (21, 40), 5),
}


def record(rng, dtype, n_cut):
    n_t = n_cut + 2 * TAPER
    t_axis = (np.arange(n_t) - TAPER) * DT
    walk = np.cumsum(rng.standard_normal((len(CH), n_t)), axis=-1) * 0.2 + 3.0 * rng.standard_normal((len(CH), n_t))
    if dtype == np.int16:
        data = np.round(walk * 200).astype(np.int16)
    else:
        data = (np.round(walk * 2 ** 8) / 2 ** 8).astype(dtype)
    return data, CH.astype(np.float64), t_axis


def gen(name, ref_io, out_dir):
    date, dtype, smoothing, lengths, seed = CASES[name]
    rng = np.random.default_rng(seed)
    h, el, er = ingest_ref.operator(21, 15)
    out = dict(date=date, ch1=CH1, ch2=CH2, smoothing=smoothing, h=h, el=el, er=er,
               names=np.array([n.format(date=date) for n in NAMES]))
    edge_noise = 0.0
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, date))
        for k, n_cut in enumerate(lengths):
            data, x_axis, t_axis = record(rng, dtype, n_cut)
            np.savez(os.path.join(root, date, NAMES[k].format(date=date)), data=data, x_axis=x_axis, t_axis=t_axis)
            out[f"data_{k}"], out[f"x_axis_{k}"], out[f"t_axis_{k}"] = data, x_axis, t_axis
        io = ref_io.ImagingIO(date, root, ch1=CH1, ch2=CH2, smoothing=smoothing)
        assert len(io) == 2
        out["time_interval"] = io.get_time_interval()
        for k, n_cut in enumerate(lengths):
            got, gx, gt = io[k]
            assert got.shape == (12, n_cut) and gx[0] == CH1 and gt[0] == 0.0, (got.shape, gx[0], gt[0])
            cut = out[f"data_{k}"][2:14, TAPER:TAPER + n_cut]
            scale = 6463.81735715902 if date > "20230219" else 1
            want = ingest_ref.smooth(cut, h, el, er, scale) if smoothing else ingest_ref.scale_only(cut, scale)
            assert got.dtype == want.dtype, (got.dtype, want.dtype)
            amax = np.abs(cut).max()
            diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
            edge = ingest_ref.edge_mask(n_cut, 10)
            if (~edge).any():
                interior = diff[:, ~edge]
                tol = ingest_ref.ulp32(want[:, ~edge]) if got.dtype == np.float32 else 1e-13 * amax
                if np.any(interior > tol):
                    raise SystemExit(f"{name}[{k}]: interior differs from ingest_ref by {interior.max():.3e}")
            edge_noise = max(edge_noise, float(diff[:, edge].max() / amax))
            out[f"out_{k}"], out[f"out_x_{k}"], out[f"out_t_{k}"] = got, gx, gt
    out["edge_noise"] = edge_noise
    path = os.path.join(out_dir, f"ingest_{name}.npz")
    np.savez(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"{name}: edge_noise {edge_noise:.3e}, {os.path.getsize(path)} bytes")


def main():
    import_reference()
    import modules.imaging_IO as ref_io
    for name in CASES:
        gen(name, ref_io, HERE)


if __name__ == "__main__":
    main()
