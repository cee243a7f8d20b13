"""Shared by tests/test_mute_table_host.py and tests/test_cut_mute_gpu.py: the trajectory mute's table applied in
NumPy the way dvh_mute_traj applies it, and the vehicle trajectories the two files place against a window.  Test
support only."""
import numpy as np

VEHICLES = ["inside", "left", "right", "crossing", "two_points"]


def vehicle(kind, x_axis, t_axis):
    """(veh_state_x, veh_state_t) of a vehicle that stays inside the window's channels, stays 300-500 m to the left
    of them or to the right, crosses them from 200 m before to 200 m after, or is known at two instants in the middle
    of the window only (the rest is interp1d's extrapolation, far outside on either side)."""
    x0, x1 = float(x_axis[0]), float(x_axis[-1])
    t0, t1 = float(t_axis[0]), float(t_axis[-1])
    span = max(x1 - x0, 1.0)
    n = 7
    if kind == "inside":
        vx = np.linspace(x0 + 0.3 * span, x0 + 0.7 * span, n)
    elif kind == "left":
        vx = np.linspace(x0 - 500.0, x0 - 300.0, n)
    elif kind == "right":
        vx = np.linspace(x1 + 300.0, x1 + 500.0, n)
    elif kind == "crossing":
        vx = np.linspace(x0 - 200.0, x1 + 200.0, n)
    elif kind == "two_points":
        tm = 0.5 * (t0 + t1)
        return np.array([x0 + 0.4 * span, x0 + 0.6 * span + 1.0]), np.array([tm, tm + 0.05 * max(t1 - t0, 0.004)])
    else:
        raise ValueError(kind)
    return vx, np.linspace(t0 - 0.01, t1 + 0.01, n)


def apply_table(data, tab, taper):
    """data[..., n_ch, n_t] times the mask of tab [n_t, 3] = (start, end, taper_start): taper[taper_start + x -
    start] for start <= x < end, 0 elsewhere; the product is formed in float64 and rounded to data's type once, as
    NumPy's ``data[:, t] *= mask`` and the kernel both do."""
    n_ch, n_t = data.shape[-2:]
    mask = np.zeros((n_ch, n_t))
    for k, (s, e, ts) in enumerate(np.asarray(tab).tolist()):
        mask[s:e, k] = taper[ts:ts + e - s]
    return (data.astype(np.float64) * mask).astype(data.dtype)
