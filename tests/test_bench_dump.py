"""bench.py --dump-outputs / --full: the options parse, and dump_outputs writes float32 / float64 .npy files whose
sample of an oversized array is the same from run to run and stays under the size cap."""
import os

import numpy as np


def test_options_default_off():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    a = bench.parse_args(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 3 * 4000)
    big = torch.arange(50 * 100, dtype=torch.float32).reshape(50, 100)
    arrays = {"small": torch.arange(12, dtype=torch.float16).reshape(3, 4), "f64": np.linspace(0, 1, 7), "big": big}
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, arrays)
    bench.dump_outputs(d2, arrays)
    small, f64, s1 = (np.load(os.path.join(d1, n + ".npy")) for n in ("small", "f64", "big"))
    assert small.dtype == np.float32 and small.shape == (3, 4) and np.array_equal(small.ravel(), np.arange(12))
    assert f64.dtype == np.float64 and np.array_equal(f64, np.linspace(0, 1, 7))
    # the oversized array: a sample of its own elements within its share of the cap, identical in both runs
    assert s1.dtype == np.float32 and s1.ndim == 1 and 0 < s1.nbytes <= 4000
    assert np.all(np.diff(s1) > 0) and np.all(np.isin(s1, big.numpy().ravel()))
    assert np.array_equal(s1, np.load(os.path.join(d2, "big.npy")))
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) < 3 * 4000 + 3 * 256
