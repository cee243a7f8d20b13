"""Host checks behind tests/test_tracker_edges_gpu.py: the exact-rational Kalman loop (tests/kf_exact.py) against the
NumPy restatement (tests/tracker_ref.kf_track) and the reference's own outputs (tests/golden/tracker_*.npz), and the
conditions under which the GPU test may demand equality on the committed cases (tests/kf_cases.py).  No GPU.

Bounds.  DELTA = 1e-6 (kf_exact.DELTA) is the distance from an integer below which a predicted arrival would count as
undecided; the committed cases contain no such step (asserted, not measured: the seeds were chosen for it with the
reference alone).  DELTA is justified by the float64 restatement's own error: max |float64 prediction - exact
prediction| over every step of every case is asserted to be at most DELTA / 1000 = 1e-9 and printed (9.3e-11; the
largest contributions come after a vehicle is lost for several rows and found again, where P = Q - K Q cancels
against a large Q).  A float64 loop that rounds the same expressions in another order is off by a few of these at
most, a thousand times less than what would move a truncation.  Matches, NaN patterns and counts are exact."""
import numpy as np
import pytest

from tests import golden_io as gio
from tests import kf_cases as kc
from tests import kf_exact
from tests import tracker_ref as kr


@pytest.mark.parametrize("case", ["a", "b"])
def test_exact_equals_the_fixture(case):
    g = gio.load("tracker_" + case)
    i0 = int(np.argmin(np.abs(g["start_x"] - g["x_axis"])))
    i1 = int(np.argmin(np.abs(g["end_x"] - g["x_axis"])))
    x_sel = g["x_axis"][i0:i1 + 1:3]
    lists = [g["row_peaks"][k, :g["row_counts"][k]] for k in range(len(x_sel))]
    ex = kf_exact.exact(lists, x_sel, g["veh_base"], float(g["sigma_a"]))
    trace = np.full(ex.states.shape, np.nan)
    ref = kr.kf_track(lists, x_sel, g["veh_base"], float(g["sigma_a"]), trace=trace)
    assert np.array_equal(ref, kr.kf_track(lists, x_sel, g["veh_base"], float(g["sigma_a"])), equal_nan=True)
    assert np.array_equal(ex.states, ref, equal_nan=True)
    assert np.array_equal(ex.states, g["veh_states_raw"], equal_nan=True)
    assert ex.decided().all()
    gap = kf_exact.prediction_gap(ex, trace)
    print(f"tracker_{case}: float64 - exact prediction {gap:.2e}, closest to an integer "
          f"{ex.closest_undetermined():.2e}")
    assert gap <= kf_exact.DELTA / 1000


@pytest.mark.parametrize("name", kc.names())
def test_case_is_decided_and_reaches_its_state(name):
    c = kc.by_name(name)
    ex, ref, trace = kc.solve(name)
    assert np.array_equal(ex.states, ref, equal_nan=True)
    assert np.array_equal(ref, kr.kf_track(c.lists(), c.x_sel, c.veh_base, c.sigma_a), equal_nan=True)  # no trace
    undecided = np.argwhere(~ex.decided())
    assert undecided.size == 0, (name, undecided[:5], ex.gap[tuple(undecided[0])])
    gap = kf_exact.prediction_gap(ex, trace)
    print(f"{name}: float64 - exact prediction {gap:.2e}, closest to an integer {ex.closest_undetermined():.2e}")
    assert gap <= kf_exact.DELTA / 1000
    if c.check is not None:
        c.check(ex)


def test_measured_margins():
    """The two numbers DESIGN.md quotes, over all committed cases."""
    gap = max(kf_exact.prediction_gap(kc.solve(n)[0], kc.solve(n)[2]) for n in kc.names())
    closest = min(kc.solve(n)[0].closest_undetermined() for n in kc.names())
    print(f"max |float64 - exact prediction| = {gap:.3e}; closest approach to an integer = {closest:.3e}")
    assert gap <= kf_exact.DELTA / 1000 and closest > kf_exact.DELTA


def test_cases_cover_the_launch_shapes():
    shapes = {(c.n_veh, c.n_steps) for c in kc.cases()}
    assert {n for n, _ in shapes} >= {1, 63, 64, 65, 130} and {s for _, s in shapes} >= {1, 2, 3, 128}
    assert any((c.count > c.cap).any() for c in kc.cases()) and any((c.count == 0).any() for c in kc.cases())
    assert any(c.cap == 1 for c in kc.cases())
    assert {c.sigma_a for c in kc.cases()} >= {0.0, 1e-4, 0.01, 0.3, 100.0}
    for c in kc.cases():
        if c.name.startswith("batch_"):
            assert 6 <= c.n_veh <= 65 and 60 <= c.n_steps <= 128
