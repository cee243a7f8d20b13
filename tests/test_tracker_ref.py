"""tests/tracker_ref.py (the NumPy / SciPy restatement of the reference's vehicle tracker) against the reference's
own outputs in tests/golden/tracker_*.npz.  No GPU.

Peak indices, matches and the NaN pattern are integers and must agree exactly; the interpolated samples of the final
tracks are np.interp of integers (one rounding each way, |value| < 2**10) and are held to 1e-12; the detection curve
is a sum of a few hundred positive float64 terms computed with the same scipy.stats.norm.pdf, held to 1e-13 max."""
import numpy as np
import pytest

from tests import golden_io as gio
from tests import tracker_ref as kr

CASES = ["a", "b"]


@pytest.fixture(scope="module", params=CASES)
def case(request):
    g = gio.load("tracker_" + request.param)
    return request.param, g


def _detect_args(g):
    return dict(minprominence=float(g["minprominence"]), minseparation=int(g["minseparation"]),
                prominenceWindow=int(g["prominenceWindow"]))


def _lists(peaks, counts):
    return [peaks[k, :counts[k]] for k in range(len(counts))]


def test_detection(case):
    _, g = case
    grid = g["grid"].astype(np.float64)
    base, erode, lists = kr.detect(grid, g["t_axis"], g["x_axis"], float(g["start_x"]), _detect_args(g),
                                   nx=int(g["nx"]), sigma=float(g["sigma"]))
    assert np.array_equal(base, g["veh_base"])
    for got, ref in zip(lists, _lists(g["det_peaks"], g["det_counts"])):
        assert np.array_equal(got, ref)
    assert np.abs(erode - g["peak_erode"]).max() <= 1e-13 * g["peak_erode"].max()


def test_tracking(case):
    _, g = case
    grid = g["grid"].astype(np.float64)
    tracks, raw, lists = kr.track(grid, g["t_axis"], g["x_axis"], float(g["start_x"]), float(g["end_x"]),
                                  g["veh_base"], _detect_args(g), sigma_a=float(g["sigma_a"]))
    assert len(lists) == len(g["row_counts"])
    for got, ref in zip(lists, _lists(g["row_peaks"], g["row_counts"])):
        assert np.array_equal(got, ref)
    assert np.array_equal(raw, g["veh_states_raw"], equal_nan=True)
    ref = g["tracks"]
    assert tracks.shape == ref.shape and np.array_equal(np.isnan(tracks), np.isnan(ref))
    assert np.nanmax(np.abs(tracks - ref)) <= 1e-12


def test_chain(case):
    _, g = case
    base, tracks = kr.chain(g["grid"].astype(np.float64), g["t_axis"], g["x_axis"], float(g["start_x"]),
                            float(g["end_x"]), _detect_args(g), sigma=float(g["sigma"]), sigma_a=float(g["sigma_a"]))
    assert np.array_equal(base, g["veh_base"])
    assert tracks.shape == g["tracks"].shape and np.nanmax(np.abs(tracks - g["tracks"])) <= 1e-12


def test_fixture_facts():
    a, b = gio.load("tracker_a"), gio.load("tracker_b")
    for g in (a, b):
        assert g["grid"].dtype == np.float32
        q = g["grid"].astype(np.float64) * 2 ** 20
        assert np.array_equal(q, np.round(q))
        # no row's peaks hang on the order of equal heights under the distance rule (a 2**-8 grid's would)
        assert all(kr.distance_order_free(r, int(g["minseparation"])) for r in g["grid"].astype(np.float64))
        assert kr.distance_order_free(g["peak_erode"], int(g["minseparation"]))
    assert not kr.distance_order_free(np.array([0, 1, 0, 1, 0, 0.5, 0.0]), 3)
    assert kr.distance_order_free(np.array([0, 1, 0, 2, 0, 1, 0.0]), 3)       # both 1s fall to the 2
    assert a["veh_base"].tolist() == [77, 222, 360, 414] and a["tracks"].shape == (3, 93)
    assert not np.isnan(a["tracks"]).any()
    n_rows_a = int(np.argmin(np.abs(a["end_x"] - a["x_axis"])) - np.argmin(np.abs(a["start_x"] - a["x_axis"]))) + 1
    assert n_rows_a % 3 != 0 and a["veh_states_raw"].shape[1] == -(-n_rows_a // 3)   # a span that is no multiple of 3
    assert b["tracks"].shape == (2, 144) and b["veh_states_raw"].shape == (4, 48)
    assert (b["rejected"] & 8).any()                              # lost for >= 20 adjacent steps
    assert ((b["rejected"] & 1) != 0).any()                       # too short-lived
    assert ((b["rejected"] == 0) & (b["jumps"] > 0)).any()        # a jump, cut and interpolated, in a kept vehicle
    v = int(np.flatnonzero((b["rejected"] == 0) & (b["jumps"] > 0))[0])
    raw = b["veh_states_raw"][v]
    k = int(np.flatnonzero(np.abs(np.diff(raw)) > 20)[0]) + 1
    row = b["tracks"][int(np.sum(b["rejected"][:v] == 0))]
    assert row[3 * k] != raw[k] and row[3 * k - 3] == raw[k - 1]   # the jumped match was replaced


def test_restated_pieces_keep_the_quirks():
    """The rejection is judged before the jump is cut; fewer than 20 differences still convolve (NumPy swaps the
    operands: every output is the whole sum); the width is n_steps * 3."""
    n = 12
    up = np.arange(n, dtype=np.float64) * 4          # +44 over the span: kept
    down = up[::-1].copy()                            # -44: the short convolution sees -44 <= -15, rejected
    jump = up.copy()
    jump[6:] += 30                                    # a 34-sample jump: cut, but the vehicle stays
    still = np.full(n, 7.0)                           # no net motion: rejected
    kept, idx = kr.remove_unrealistic(np.stack([up, down, jump, still]))
    assert idx.tolist() == [0, 2]
    assert np.isnan(kept[1, 6]) and np.isnan(kept[1]).sum() == 1
    full = kr.spread_and_interp(kept)
    assert full.shape == (2, n * 3) and not np.isnan(full).any()
    assert full[1, 18] == pytest.approx((jump[5] + jump[7]) / 2) and full[0, -1] == up[-1]
