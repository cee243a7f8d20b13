"""preprocess.mute_traj_table, the host half of the trajectory mute, against the oracle's
mute_along_traj (oracle/preprocess.py, the restatement of apis/data_classes.py:49-72).  No GPU: the table is applied
in NumPy exactly as dvh_mute_traj applies it (tests/mute_ref.apply_table), so what is compared is the taper
placement; the device side is tests/test_cut_mute_gpu.py.

Bounds: equality bit for bit (the table holds indices, the taper is SciPy's, the product is one float64
multiplication per sample), and an exception of the same type where the oracle raises.  The grid is 2 430 cases: 6
channel counts x 3 channel spacings x 9 offsets x 3 taper shapes x 5 vehicle trajectories.  The invariants asserted
on every table are the ones the kernel indexes by without a check of its own."""
import itertools

import numpy as np
import pytest

from oracle import preprocess as opre
from tests import mute_ref

NX = [2, 3, 5, 17, 49, 120]
DX = [0.5, 1.0, 8.16]
OFFSET = [0, 1, 8, 8.16, 20, 100, 300, 1000, 2000]
ALPHA = [0, 0.3, 1]


def _run(fn):
    try:
        return fn(), None
    except Exception as e:  # noqa: BLE001 -- the type is what is compared
        return None, type(e)


@pytest.mark.parametrize("nx", NX)
def test_table_equals_the_oracle(nx):
    with np.errstate(invalid="ignore"):                       # inf * 0 and NaN * 0 are part of the data
        _grid(nx)


def _grid(nx):
    from das_diff_veh_amd.preprocess import mute_traj_table
    rng = np.random.default_rng(nx)
    n_t = 23
    t_axis = 10.0 + 0.004 * np.arange(n_t)
    data = np.round(rng.standard_normal((nx, n_t)) * 256) / 256
    data[0, 0], data[-1, 5], data[0, 7], data[-1, 9] = np.nan, np.inf, -np.inf, -0.0
    n = raised = 0
    for dx, offset, alpha, kind in itertools.product(DX, OFFSET, ALPHA, mute_ref.VEHICLES):
        x_axis = 500.0 + dx * np.arange(nx)
        vx, vt = mute_ref.vehicle(kind, x_axis, t_axis)
        ref, ref_err = _run(lambda: opre.mute_along_traj(data, x_axis, t_axis, vx, vt, offset=offset, alpha=alpha))
        tab_taper, err = _run(lambda: mute_traj_table(x_axis, t_axis, vx, vt, offset=offset, alpha=alpha))
        n += 1
        if ref_err is not None or err is not None:
            assert ref_err is err, (dx, offset, alpha, kind, ref_err, err)
            raised += 1
            continue
        tab, taper = tab_taper
        assert tab.dtype == np.int32 and tab.shape == (n_t, 3) and taper.dtype == np.float64
        s, e, ts = tab[:, 0], tab[:, 1], tab[:, 2]
        assert (0 <= s).all() and (s <= e).all() and (e <= nx).all(), (dx, offset, alpha, kind)
        assert (ts >= 0).all() and (ts + e - s <= len(taper)).all(), (dx, offset, alpha, kind)
        got = mute_ref.apply_table(data, tab, taper)
        assert got.tobytes() == ref.tobytes(), (dx, offset, alpha, kind)
    assert n == len(DX) * len(OFFSET) * len(ALPHA) * len(mute_ref.VEHICLES) == 405
    print(f"nx {nx}: {n} cases, {raised} raise in both")


def test_both_raise():
    """Where the oracle cannot place a taper, the table raises the same exception: a window of one channel (no
    spacing to take) and channels that all sit at one position (the offset is divided by a spacing of 0)."""
    from das_diff_veh_amd.preprocess import mute_traj_table
    t_axis = 10.0 + 0.004 * np.arange(9)
    x_axis = 500.0 + 8.16 * np.arange(12)
    vx, vt = mute_ref.vehicle("inside", x_axis, t_axis)
    data = np.ones((12, 9))
    for what, xa, x, t in (("one channel", x_axis[:1], vx, vt), ("equal channels", np.full(12, 500.0), vx, vt)):
        with np.errstate(divide="ignore"):
            ref, ref_err = _run(lambda: opre.mute_along_traj(data[:len(xa)], xa, t_axis, x, t))
            got, err = _run(lambda: mute_traj_table(xa, t_axis, x, t))
        assert ref_err is not None and err is ref_err, (what, ref_err, err)
