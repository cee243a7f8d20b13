"""CPU checks of the tracking-grid preprocessing fixture (tests/golden/tracking_prep*.npz, the reference's
TimeLapseImaging._preprocess_for_tracking, apis/timeLapseImaging.py:74-102) and of tests/tracking_ref.py, the
SciPy / NumPy restatement the GPU tests and the benchmark tool lean on: the helper is pinned to the reference's
outputs at 1e-13 of their maximum, stage by stage where the fixture holds the stage."""
import numpy as np
import pytest
import scipy.signal

from tests import golden_io as gio
from tests import tracking_ref as tr

CASES = {"plain": ([], 0), "loud": ([9], 9), "dead_first_loud": ([17], 0), "two_loud_last": ([5, 23], 5)}
BOUND = 1e-13


@pytest.fixture(scope="module")
def head():
    return gio.load("tracking_prep")


def _ref(head, case):
    return tr.tracking_ref(head[case + "_in"].astype(np.float64), float(head["dt"]), head["x_axis"][0])


@pytest.mark.parametrize("case", list(CASES))
def test_helper_reproduces_the_reference(head, case):
    r = _ref(head, case)
    ref = gio.load("tracking_prep_" + case)["data_for_tracking"]
    assert r["out"].shape == ref.shape == (196, 300) and ref.dtype == np.float64
    err = np.abs(r["out"] - ref).max()
    print(f"{case}: |helper - reference|max = {err:.3e} of max {np.abs(ref).max():.3e}")
    assert err <= BOUND * np.abs(ref).max()
    assert np.array_equal(r["dist"], head[case + "_dist"])
    assert np.array_equal(head["t_axis"][::5], head[case + "_t_axis_tracking"])


def test_helper_stages_reproduce_the_reference(head):
    r = _ref(head, "loud")
    st = gio.load("tracking_prep_loud_stages")
    for k in ("bp", "rs"):
        assert r[k].shape == st[k].shape
        assert np.abs(r[k] - st[k]).max() <= BOUND * np.abs(st[k]).max(), k


@pytest.mark.parametrize("case", list(CASES))
def test_fixture_facts(head, case):
    gated, imputed = CASES[case]
    assert head[case + "_in"].dtype == np.float32 and head[case + "_in"].shape == (24, 1500)
    assert head[case + "_gated"].tolist() == gated and int(head[case + "_imputed"]) == imputed
    r = _ref(head, case)
    assert r["gated"].tolist() == gated and r["imputed"] == imputed
    assert np.array_equal(head[case + "_dist"], np.arange(196) + (449 - 400) * 8.16)  # 399.84, 400.84, ...
    q =head[case + "_in"].astype(np.float64) * 2 ** 8
    assert np.array_equal(q, np.round(q))  # multiples of 2**-8: exact in float32


@pytest.mark.parametrize("up,down", [(204, 25), (3, 2), (2, 3), (4, 2)])
@pytest.mark.parametrize("n_in", [1, 2, 11, 24])
def test_resample_formula_is_resample_poly(up, down, n_in):
    """The sum the resampling kernel implements (include/dvh.h) against scipy.signal.resample_poly itself."""
    x = np.random.default_rng(n_in).standard_normal((n_in, 7))
    ref = scipy.signal.resample_poly(x, up, down, axis=0)
    got = tr.resample_rows(x, up, down)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= BOUND * np.abs(ref).max()
