"""dvh_kf_track and dvh_peak_likelihood through the C ABI at the edges of their rules and launch shapes, against
references they cannot share a mistake with: the Kalman loop in exact rational arithmetic (tests/kf_exact.py) and the
detection curve's double sum in numpy.longdouble.

Kalman loop.  The cases are tests/kf_cases.py: the association gates at d = -16 .. 32 and their priorities, the
one-match and two-match states, predictions below zero (truncated, not floored), the +-1e9 guard, sigma_a = 0, 1e-4
and 100, uneven, repeated and descending positions, empty rows, count > cap, cap = 1, 1-130 vehicles, 1-128 steps,
and three lock-and-clutter batches.  tests/test_kf_exact_host.py asserts on the host that every predicted arrival of
every case is either an exact integer reached with slope 0 (where float64 has no rounding to make) or more than
1e-6 from every integer, while the float64 restatement's prediction is within 1e-9 of the exact one.  So any
float64 evaluation of the reference's expressions truncates to the same bases, and the bound here is equality:
matches and NaN pattern, with the canaries on either side of the output untouched.

Detection curve.  out[t] = sum over rows of (sum over the row's first min(count, cap) peaks inside [0, n_t) of
exp(-z^2 / 2) / sqrt(2 pi) / sigma), z = (t_axis[t] - t_axis[peak]) / sigma, as the kernel's header has it; the
reference evaluates the same expression and order in longdouble (64-bit mantissa: its own error is 2**-11 of the
bound below).  Pointwise bound, with u = 2**-53 and a = z^2 / 2: the subtraction, the division and the square put
at most 5 u relative on z^2, which moves exp(-a) by 5 a u relative; exp itself is good to 1 ulp = 2 u, and the two
divisions add u each: (5 a + 4) u per term, taken as (5 a + 8) u.  Adding a zero is exact, so the N non-zero terms of
a sample meet in at most N - 1 rounded additions, each u relative on a partial sum that never exceeds the total:
N u times the sum.  A term below the normal range loses its relative accuracy; it and its additions are then good
to a few denormal steps, covered by N 2**-1070 (16 steps a term).  That floor holds while 1 / (sqrt(2 pi) sigma),
which multiplies the rounding of a denormal exp, stays under about 14: it does for sigma = 0.08 (5) and 10, and not
for sigma = 1e-3 (399).  So the sigma = 1e-3 runs use an axis with steps of 10, 20 and 30 ms: a is then 0, 50, 200, 450
or at least 800, every exp is either normal or below 1e-347, where the kernel's 0 is inside the floor, and the
denormal window 708 < a < 745 is met by sigma = 0.08 on the freely drawn axis (samples 3 s from a peak).  The bound is
    u (sum_i term_i (5 a_i + 8) + N sum_i term_i) (1 + 2**-20) + N 2**-1070,
the last factor for the second-order terms.  The project's own bound, 1e-12 of the curve's maximum, is asserted as
well.  The largest error / bound ratio is printed (it is recorded in DESIGN.md)."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import kf_cases as kc

pytestmark = pytest.mark.gpu
GUARD = 16
FILL = -7
CANARY = -1.0


# ------------------------------------------------------------------------------------------ dvh_kf_track

def _buffers(c):
    import torch
    pk = np.concatenate([c.peaks.ravel(), np.full(GUARD, FILL, dtype=np.int32)])   # a guard after the last row
    n = c.n_veh * c.n_steps
    return (torch.from_numpy(pk).cuda(), torch.from_numpy(c.count).cuda(), torch.from_numpy(c.x_sel).cuda(),
            torch.from_numpy(c.veh_base).cuda(),
            torch.full((GUARD + n + GUARD,), CANARY, dtype=torch.float64, device="cuda"))


def _kf(c):
    """dvh_kf_track on a case -> [n_veh, n_steps]; the output sits between two canary regions."""
    import torch

    from das_diff_veh_amd import _lib
    pk, ct, xs, vb, buf = _buffers(c)
    n = c.n_veh * c.n_steps
    _lib.call("dvh_kf_track", _lib.ptr(pk), c.cap, _lib.ptr(ct), c.n_steps, _lib.ptr(xs), _lib.ptr(vb), c.n_veh,
              c.sigma_a, _lib.ptr(buf[GUARD:]), _lib.stream_of(xs.device))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[GUARD + n:] == CANARY).all()
    return got[GUARD:GUARD + n].reshape(c.n_veh, c.n_steps)


@pytest.mark.parametrize("name", kc.names())
def test_kf_case(device, name):
    c = kc.by_name(name)
    ex, ref, _ = kc.solve(name)
    got = _kf(c)
    assert np.array_equal(np.isnan(got), np.isnan(ex.states)), (name, np.argwhere(np.isnan(got) != np.isnan(ex.states))[:5])
    assert np.array_equal(got, ex.states, equal_nan=True), (name, np.argwhere(~np.isclose(got, ex.states, equal_nan=True))[:5])
    assert np.array_equal(got, ref, equal_nan=True)
    if c.check is not None:                            # the device's matches reach the state the case is named for
        dev = copy.copy(ex)
        dev.states = got
        c.check(dev)


def test_kf_refusals_and_empty_calls(device):
    """A NaN sigma_a, cap < 1 or a null pointer with work to do return -2; no vehicles or no steps return 0; nothing
    is written in any of them.  All of it is decided on the host before a launch."""
    import torch

    from das_diff_veh_amd import _lib
    c = kc.by_name("clip")
    fn = _lib.load().dvh_kf_track
    pk, ct, xs, vb, buf = _buffers(c)
    st = _lib.stream_of(xs.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = p(buf[GUARD:])
    good = [p(pk), c.cap, p(ct), c.n_steps, p(xs), p(vb), c.n_veh, c.sigma_a, out, st]
    calls = {"NaN sigma_a": (7, float("nan"), -2), "cap 0": (1, 0, -2), "cap -1": (1, -1, -2),
             "n_steps -1": (3, -1, -2), "n_veh -1": (6, -1, -2),
             "null peaks": (0, None, -2), "null count": (2, None, -2), "null x_sel": (4, None, -2),
             "null veh_base": (5, None, -2), "null veh_states": (8, None, -2),
             "no vehicles": (6, 0, 0), "no steps": (3, 0, 0)}
    for what, (i, val, want) in calls.items():
        args = list(good)
        args[i] = val
        assert fn(*args) == want, what
        if want:
            assert _lib.load().dvh_last_error()
    null = [None, c.cap, None, 0, None, None, 0, c.sigma_a, None, st]      # nothing to do: the pointers are not looked at
    assert fn(*null) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all()
    assert fn(*good) == 0                                                   # and the same buffers do work
    torch.cuda.synchronize()
    n = c.n_veh * c.n_steps
    assert np.array_equal(buf.cpu().numpy()[GUARD:GUARD + n].reshape(c.n_veh, -1), kc.solve("clip")[0].states,
                          equal_nan=True)


# ------------------------------------------------------------------------------------------ dvh_peak_likelihood

LD = np.longdouble
U = 2.0 ** -53


def _likelihood_ref(peaks, counts, t_axis, sigma):
    """(the curve, its pointwise bound) in longdouble, in the kernel's order."""
    n_rows, cap = peaks.shape
    n_t = len(t_axis)
    t = t_axis.astype(LD)
    s = LD(sigma)
    sqrt_2pi = LD(2.5066282746310002)          # np.sqrt(2 * np.pi) as a double, the constant the kernel divides by
    acc = np.zeros(n_t, dtype=LD)
    weighted = np.zeros(n_t, dtype=LD)         # sum of term (5 a + 8)
    n_terms = 0
    for r in range(n_rows):
        row = np.zeros(n_t, dtype=LD)
        for p in peaks[r, :min(int(counts[r]), cap)]:
            if p < 0 or p >= n_t:
                continue                       # not a sample of this axis
            z = (t - t[p]) / s
            a = z * z / 2
            term = np.exp(-a) / sqrt_2pi / s
            row = row + term
            weighted += term * (5 * a + 8)
            n_terms += 1
        acc += row
    bound = LD(U) * (weighted + n_terms * acc) * (1 + LD(2.0) ** -20) + n_terms * LD(2.0) ** -1070
    return acc, bound


def _likelihood(peaks, counts, t_axis, sigma):
    import torch

    from das_diff_veh_amd import _lib
    n_t = len(t_axis)
    pk = torch.from_numpy(np.concatenate([np.ascontiguousarray(peaks, dtype=np.int32).ravel(),
                                          np.full(GUARD, 0, dtype=np.int32)])).cuda()   # a peak at 0 past the table
    ct = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(t_axis, dtype=np.float64)).cuda()
    buf = torch.full((GUARD + n_t + GUARD,), CANARY, dtype=torch.float64, device="cuda")
    _lib.call("dvh_peak_likelihood", _lib.ptr(pk), peaks.shape[1], _lib.ptr(ct), len(counts), _lib.ptr(t), n_t,
              float(sigma), _lib.ptr(buf[GUARD:]), _lib.stream_of(t.device))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[GUARD + n_t:] == CANARY).all()
    return got[GUARD:GUARD + n_t]


def _peak_table(rng, n_rows, n_t, cap):
    """Peaks per row, among them -1 and n_t (skipped); some rows empty, some with count > cap."""
    peaks = np.full((n_rows, cap), n_t // 2, dtype=np.int32)
    counts = np.zeros(n_rows, dtype=np.int32)
    for r in range(n_rows):
        k = int(rng.integers(0, cap + 1))
        row = np.sort(rng.integers(-1, n_t + 1, k)).astype(np.int32)    # -1 and n_t are drawn as often as a sample
        peaks[r, :k] = row
        counts[r] = k
        if r % 7 == 3:
            counts[r] = cap + 1 + r % 3       # more than cap: the slots of the next row are not this row's
            peaks[r, k:] = np.sort(rng.integers(0, n_t, cap - k))
    if n_rows > 1:
        counts[1] = 0
    return peaks, counts


def _t_axis(rng, n_t):
    return 4.0 + np.cumsum(rng.uniform(0.005, 0.035, n_t))               # uneven, about 50 Hz


def _t_axis_steps(rng, n_t):
    """Uneven in steps of 10, 20 and 30 ms (see the docstring: the axis of the sigma = 1e-3 runs)."""
    return 4.0 + 0.01 * np.cumsum(rng.integers(1, 4, n_t))


RATIO = {}


def _check_likelihood(peaks, counts, t_axis, sigma, tag):
    ref, bound = _likelihood_ref(peaks, counts, t_axis, sigma)
    got = _likelihood(peaks, counts, t_axis, sigma)
    err = np.abs(got.astype(LD) - ref)
    some = bound > 0                                                     # no term at all: the curve is 0 exactly
    ratio = float((err[some] / bound[some]).max()) if some.any() else 0.0
    RATIO[tag] = ratio
    print(f"{tag}: max err {float(err.max()):.3e}, max ref {float(ref.max()):.3e}, err / bound {ratio:.3f}")
    assert (err <= bound).all(), (tag, int(np.argmax(err - bound)))
    assert float(err.max()) <= 1e-12 * float(ref.max())
    return got, ref


@pytest.mark.parametrize("n_t", [1, 255, 256, 257, 1000])
def test_peak_likelihood_edges(device, n_t):
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has fewer than 63 mantissa bits here: no reference to hold the kernel to")
    rng = np.random.default_rng(4100 + n_t)
    t_axis, t_steps = _t_axis(rng, n_t), _t_axis_steps(rng, n_t)
    for n_rows in (1, 15, 300):
        peaks, counts = _peak_table(rng, n_rows, n_t, cap=6)
        if n_rows == 1:
            counts[0] = 9                                                # the single row overflows its cap
            peaks[0] = np.sort(rng.integers(0, n_t, 6))
        for sigma in (1e-3, 0.08, 10.0):
            got, ref = _check_likelihood(peaks, counts, t_steps if sigma == 1e-3 else t_axis, sigma,
                                         f"n_t {n_t} rows {n_rows} sigma {sigma}")
            if sigma == 1e-3 and n_t > 1 and n_rows == 1:                # six peaks; a term 40 ms or more from its
                assert (got == 0).mean() > 0.5 and got.max() > 100       # peak is below 2**-1074
    peaks, counts = _peak_table(rng, 15, n_t, cap=1)
    counts[2], counts[5] = 1, 4
    peaks[2, 0], peaks[5, 0] = n_t - 1, 0
    _check_likelihood(peaks, counts, t_axis, 0.08, f"n_t {n_t} cap 1")
    skipped = np.array([[-1, n_t, n_t + 5]], dtype=np.int32)             # no peak of the row is a sample
    assert not _likelihood(skipped, np.array([3], dtype=np.int32), t_axis, 0.08).any()
    print(f"n_t {n_t}: largest err / bound {max(RATIO.values()):.3f}")
