"""The committed cases of the Kalman-loop edge tests, shared by tests/test_kf_exact_host.py (which asserts on the host
that every step of every case is decided, see tests/kf_exact.py, and that each case reaches the state it is named
for) and tests/test_tracker_edges_gpu.py (which runs dvh_kf_track on them and demands equality).

A case is a peak table [n_steps, cap] int32 (ascending per row, unused slots filled with PAD, which is out of every
vehicle's reach), the per-row counts (which may exceed cap: only the first cap peaks exist), the row positions
x_sel, the vehicles' bases and sigma_a.  solve() computes the exact result, the NumPy reference's and its float64
predictions once per case and keeps them."""
import functools

import numpy as np

from tests import kf_exact
from tests import tracker_ref as kr

PAD = 2 ** 30


class Case:
    def __init__(self, name, rows, x_sel, veh_base, sigma_a, cap=None, count=None, check=None, stale=None):
        self.name = name
        n_steps = len(rows)
        self.cap = int(cap if cap is not None else max([len(r) for r in rows] + [1]))
        self.peaks = np.full((n_steps, self.cap), PAD, dtype=np.int32)
        for k, r in enumerate(rows):
            r = np.sort(np.asarray(r, dtype=np.int64))
            assert (np.diff(r) > 0).all(), (name, k)
            self.peaks[k, :min(len(r), self.cap)] = r[:self.cap]
        for (k, j), val in (stale or {}).items():     # a value past the row's count: never to be read
            self.peaks[k, j] = val
        self.count = np.array([len(r) for r in rows] if count is None else count, dtype=np.int32)
        self.x_sel = np.ascontiguousarray(x_sel, dtype=np.float64)
        self.veh_base = np.ascontiguousarray(veh_base, dtype=np.int32)
        self.sigma_a = float(sigma_a)
        self.check = check
        assert len(self.x_sel) == n_steps and np.isfinite(self.x_sel).all()

    @property
    def n_steps(self):
        return len(self.count)

    @property
    def n_veh(self):
        return len(self.veh_base)

    def lists(self):
        """What the loop may use of each row: its first min(count, cap) peaks."""
        return [self.peaks[k, :min(int(c), self.cap)] for k, c in enumerate(self.count)]


def _axis(kind, n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "3m":
        return 595.0 + 3.0 * np.arange(n)
    if kind == "jitter":                                    # uneven steps of 1.5 .. 4.5 m
        return 595.0 + np.cumsum(rng.uniform(1.5, 4.5, n))
    if kind == "repeat":                                    # every fifth position repeated: dx = 0
        return 595.0 + 3.0 * (np.arange(n) - np.arange(n) // 5)
    if kind == "descending":
        return 980.0 - 3.0 * np.arange(n)
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------ the designed cases

GATE_D = [-16, -15, -14, -1, 0, 1, 29, 30, 31, 32]


def _gates():
    """One row; vehicle i < 10 has the single peak base + GATE_D[i]; then four vehicles with two peaks each."""
    base = 500 + 1000 * np.arange(14)
    row = [base[i] + d for i, d in enumerate(GATE_D)]
    pairs = [(-3, 20), (5, 12), (-10, -4), (0, 30)]         # ahead beats a nearer behind; nearer ahead; nearer
    want = [20, 5, -4, 30]                                  # behind; 0 counts as behind, so 30 wins
    for i, (a, b) in enumerate(pairs):
        row += [base[10 + i] + a, base[10 + i] + b]

    def check(ex):
        for i, d in enumerate(GATE_D):
            got = ex.states[i, 0]
            assert (got == base[i] + d) if -15 < d <= 30 else np.isnan(got), (i, d, got)
        for i, w in enumerate(want):
            assert ex.states[10 + i, 0] == base[10 + i] + w, (i, ex.states[10 + i, 0])

    return Case("gates", [sorted(row)], [595.0], base, 0.01, check=check)


B = 500   # the base of the one- and two-match vehicle
_ONE_TWO_ROWS = [
    [B + 25],            # 0: the first match
    [B + 45],            # 1: within 30 of the match, 45 from the base: not taken
    [B - 20, B + 45],    # 2: nor is anything else out of the base's reach
    [B + 10],            # 3: the second match, through the base (15 behind the first match: out of its reach)
    [B + 0],             # 4: in reach of the second match (-10) but not of the first (-25): the prediction is the
                         #    first match, so nothing matches
    [B + 53],            # 5: 28 ahead of the first match, 43 ahead of the second: the third match
    [B + 50, B + 95],    # 6: see _two_match
]


def _one_match():
    def check(ex):
        cnt = ex.match_counts()[0]
        assert cnt[:3].tolist() == [1, 1, 1] and ex.states[0, 0] == B + 25      # exactly one match after steps 0-2
        assert np.isnan(ex.states[0, 1:3]).all() and ex.states[0, 3] == B + 10 and cnt[3] == 2
        assert all(p is None for p in ex.pred[0])                               # the base was veh_base throughout

    return Case("one_match", _ONE_TWO_ROWS[:4], _axis("3m", 4), [B], 0.01, check=check)


def _two_match():
    """After the third match the filter is updated with dx = x[5] - x[0] = 15 m: the position of the last update is
    the first match's, and step 6 predicts B + 63.9, base B + 63.  Had the position moved to the second match
    (dx = 6 m) the gain would be smaller and the slope larger, and step 6 would predict B + 67.8.  The peak at B + 95
    is 32 ahead of the right base and 28 ahead of the wrong one, so the right loop falls back on the peak 13 behind,
    B + 50."""
    def check(ex):
        cnt = ex.match_counts()[0]
        assert cnt.tolist() == [1, 1, 1, 2, 2, 3, 4], cnt
        assert ex.pred[0][4] == B + 25 and ex.pred[0][5] == B + 25 and ex.slope0[0, 4] and ex.slope0[0, 5]
        assert np.isnan(ex.states[0, 4]) and ex.states[0, 5] == B + 53 and ex.states[0, 6] == B + 50
        assert 63 < ex.pred[0][6] - B < 64

    return Case("two_match", _ONE_TWO_ROWS, _axis("3m", 7), [B], 0.01, check=check)


def _trunc_case(name, z0, last_peak, lo, hi, want_base):
    """A track descending 7, 6, 8, 5, 7, ... samples per 3 m row from z0 until the next step would pass sample 0
    (uneven, so that the filter does not settle on integer predictions; at most 13 over the first two rows, which
    the two-match state's reach of 15 behind allows); the last row holds one peak, 30 ahead of the truncated
    prediction and 31 ahead of the floored one."""
    zs = [z0]
    while zs[-1] - (7, 6, 8, 5)[(len(zs) - 1) % 4] >= 0:
        zs.append(zs[-1] - (7, 6, 8, 5)[(len(zs) - 1) % 4])
    n = len(zs)
    rows = [[z] for z in zs] + [[last_peak]]

    def check(ex):
        p = ex.pred[0][n]
        assert lo < p < hi, float(p)
        assert int(p) == want_base and last_peak - want_base == 30
        assert not np.isnan(ex.states[0, :n]).any() and ex.states[0, n] == last_peak

    return Case(name, rows, _axis("3m", n + 1), [z0 - 4], 0.3, check=check)


def _guard(sign):
    """sigma_a = 1/4 and rows 1 m apart make the third match's update exact in float64: Q00 = 1, the gain is
    (1/2, 1/2), and an innovation of +-9 leaves the state at (z + 4.5, 4.5) samples and samples per metre.  The next
    row is 2**28 m on, and the rows after it 2 m apart: every prediction from there is an odd multiple of 1/2 beyond
    +-1.2e9, exactly representable, and nothing can match.  (Were there no guard, the conversion of such a
    prediction to an index would be out of int32's range.)"""
    z = 2000
    x = np.array([0.0, 1.0, 2.0, 2.0 + 2.0 ** 28, 4.0 + 2.0 ** 28, 6.0 + 2.0 ** 28])
    rows = [[z], [z + 4 * sign], [z + 9 * sign], [z, z + 9 * sign], [z + 5 * sign], [z - 3, z + 20]]

    def check(ex):
        assert ex.states[0, :3].tolist() == [z, z + 4 * sign, z + 9 * sign] and np.isnan(ex.states[0, 3:]).all()
        for k in (3, 4, 5):
            assert sign * ex.pred[0][k] > 10 ** 9 and ex.pred[0][k].denominator == 2

    return Case("guard_pos" if sign > 0 else "guard_neg", rows, x, [z], 0.25, check=check)


def _single_track(name, sigma_a, axis, seed, n=40, check=None):
    """One vehicle at about 1.4 samples per metre of the axis, whichever way it runs, with integer jitter, two
    dropouts and a clutter peak on every fourth row."""
    rng = np.random.default_rng(seed)
    x = _axis(axis, n, seed)
    arr = np.round(900 + 1.4 * (x - x[0]) * (1 if x[-1] > x[0] else -1) + rng.integers(-1, 2, n)).astype(int)
    rows = []
    for k in range(n):
        r = set() if k in (7, 19) else {int(arr[k])}
        if k % 4 == 1:
            r.add(int(arr[k]) + int(rng.choice([-22, -9, 33, 45])))
        rows.append(sorted(r))
    return Case(name, rows, x, [int(arr[0]) + 3], sigma_a, check=check)


def _frozen(ex):
    """sigma_a = 0: the gain is 0, the base stays the first match and the vehicle is lost once it has moved out of
    that base's reach."""
    first = ex.states[0, 0]
    got = ex.states[0][~np.isnan(ex.states[0])]
    assert all(p is None or p == first for p in ex.pred[0]) and (got <= first + 30).all()
    assert np.isnan(ex.states[0, 12:]).all() and len(got) >= 4


def _follows(ex):
    """sigma_a = 100: the gain is above 0.9995 at every update, the base moves with the measurements, and the vehicle
    is followed far beyond the first match's reach (where sigma_a = 0 loses it)."""
    got = ex.states[0][~np.isnan(ex.states[0])]
    assert len(got) >= 20 and got[-1] > got[0] + 60
    k = int(np.flatnonzero(~np.isnan(ex.states[0]))[-1])
    assert abs(ex.pred[0][k] - got[-2]) < 30


def _clip():
    """Rows with count 0, rows whose count exceeds cap (only the first cap peaks exist; what follows them in memory
    is the next row), and stale entries past a row's count."""
    base = [300, 1300]
    cap = 3
    rows = [
        [100, 310, 1290],                 # 0: both match (ahead 10; behind -10)
        [],                               # 1: count 0, and the stale slots below hold peaks in reach
        [90, 120, 280, 318, 1310],        # 2: count 5 > cap 3: 318 and 1310 do not exist; 280 is out of reach (-20)
        [322, 1295, 1500],                # 3: its first peak follows row 2's three in memory, 22 ahead of base 300
        [],                               # 4
        [305, 1305, 1400],                # 5
    ]

    def check(ex):
        assert ex.states[:, 0].tolist() == [310.0, 1290.0]
        assert np.isnan(ex.states[:, 1]).all() and np.isnan(ex.states[:, 2]).all() and np.isnan(ex.states[:, 4]).all()
        assert ex.states[:, 3].tolist() == [322.0, 1295.0] and ex.states[:, 5].tolist() == [305.0, 1305.0]

    return Case("clip", rows, _axis("3m", 6), base, 0.01, cap=cap, count=[3, 0, 5, 3, 0, 3], check=check,
                stale={(1, 0): 305, (1, 1): 1295, (4, 0): 320, (4, 1): 1300})


def _cap_one():
    rows = [[700 + 4 * k] for k in range(6)]
    rows[2] = []
    return Case("cap_one", rows, _axis("3m", 6), [702, 650], 0.01, cap=1)


# ------------------------------------------------------------------------------------------ lock and clutter

def _scene(name, seed, n_veh, n_steps, sigma_a, axis="3m", dropout=0.15, clutter=3, spread=40, min_kept=None,
           twins=0):
    """n_veh vehicles 700 samples apart at 0.3-1.4 samples per metre with +-1 sample of jitter; a row holds each
    vehicle's arrival with probability 1 - dropout and `clutter` further peaks within `spread` samples of some
    vehicle.
    With `twins`, the last `twins` bases repeat the first ones."""
    rng = np.random.default_rng(seed)
    x = _axis(axis, n_steps, seed)
    b = 400 + 700 * np.arange(n_veh) + rng.integers(-40, 41, n_veh)
    slope = rng.uniform(0.3, 1.4, n_veh)
    arr = np.round(b[:, None] + slope[:, None] * np.abs(x - x[0])[None, :] + rng.integers(-1, 2, (n_veh, n_steps)))
    arr = arr.astype(np.int64)
    rows = []
    for k in range(n_steps):
        r = {int(a) for a in arr[rng.random(n_veh) > dropout, k]}
        for _ in range(clutter):
            r.add(int(arr[rng.integers(n_veh), k] + rng.integers(-spread, spread + 1)))
        rows.append(sorted(r))
    base = b + rng.integers(-8, 9, n_veh)
    if twins:
        base[-twins:] = base[:twins]

    def check(ex):
        if twins:
            assert np.array_equal(ex.states[-twins:], ex.states[:twins], equal_nan=True)
        if min_kept is not None:          # the vehicles the host tail keeps have at least 20 filtered updates each
            _, keep = kr.remove_unrealistic(ex.states)
            assert len(keep) >= min_kept, (name, len(keep))
            assert (ex.match_counts()[keep, -1] - 2 >= 20).all(), name

    return Case(name, rows, x, base, sigma_a, check=check)


# (z0, the last row's peak, the open interval the last prediction lies in, its truncation)
TRUNC_A = (82, 30, -1, 0, 0)        # predicts -0.764: base 0, not -1
TRUNC_B = (78, 26, -5, -4, -4)      # predicts -4.764: base -4, not -5, and the peak at 26 is 30 ahead of it


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        _gates(), _one_match(), _two_match(),
        _trunc_case("trunc_above_minus_one", *TRUNC_A), _trunc_case("trunc_below_minus_one", *TRUNC_B),
        _guard(+1), _guard(-1),
        _single_track("sigma_a_0", 0.0, "3m", 11, check=_frozen),
        _single_track("sigma_a_100", 100.0, "3m", 12, check=_follows),
        _single_track("sigma_a_1e-4", 1e-4, "3m", 13),
        _single_track("x_jitter", 0.01, "jitter", 14),
        _single_track("x_repeat", 0.3, "repeat", 15),
        _single_track("x_descending", 0.01, "descending", 16),
        _clip(), _cap_one(),
        _scene("shape_1x1", 21, 1, 1, 0.01), _scene("shape_63x2", 22, 63, 2, 0.01),
        _scene("shape_64x3", 23, 64, 3, 0.01), _scene("shape_130x12", 24, 130, 12, 0.01, twins=30),
        _scene("batch_6x128", 37, 6, 128, 1e-4, spread=150, min_kept=4),
        _scene("batch_20x90", 32, 20, 90, 0.01, spread=80, min_kept=10),
        _scene("batch_65x60", 36, 65, 60, 0.3, min_kept=40),
    ]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def names():
    return [c.name for c in cases()]


def by_name(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def solve(name):
    """(the exact result, tracker_ref.kf_track's matches, its float64 predictions) of a case."""
    c = by_name(name)
    ex = kf_exact.exact(c.lists(), c.x_sel, c.veh_base, c.sigma_a)
    trace = np.full((c.n_veh, c.n_steps), np.nan)
    ref = kr.kf_track(c.lists(), c.x_sel, c.veh_base, c.sigma_a, trace=trace)
    return ex, ref, trace
