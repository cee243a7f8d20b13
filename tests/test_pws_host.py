"""The phase-weighted stack where there is no GPU: tests/pws_ref.py's closed-form transform against
scipy.signal.hilbert, the host twins dvh_hilbert_rows_host / dvh_select_pws_host (csrc/pws.h's arithmetic, the same the
kernels run) against that reference at the bounds pws_ref derives, the entries' refusals and bootstrap.check_stack."""
import ctypes

import numpy as np
import pytest

from tests import pws_ref as ref

CANARY = np.float32(-77.25)
PAD = 64


@pytest.fixture(scope="module")
def lib():
    import os

    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    return _lib.load()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _hilbert_host(lib, X, W, row_len=None, row_stride=None):
    """dvh_hilbert_rows_host on rows X [n_row, W] placed row_stride apart in a canary-framed buffer: (rc, H rows);
    everything the call may not write is asserted to hold its canary."""
    n_row = X.shape[0]
    row_stride = W if row_stride is None else row_stride
    xin = np.full(n_row * row_stride, np.nan, np.float32)
    xin.reshape(n_row, row_stride)[:, :W] = X
    out = np.full(PAD + n_row * row_stride + PAD, CANARY, np.float32)
    body = out[PAD:PAD + n_row * row_stride]
    rl = None if row_len is None else np.ascontiguousarray(row_len, dtype=np.int32)
    rc = lib.dvh_hilbert_rows_host(_p(xin), row_stride, n_row, W, _p(rl), _p(body))
    assert np.all(out[:PAD] == CANARY) and np.all(out[PAD + n_row * row_stride:] == CANARY)
    rows = body.reshape(n_row, row_stride)
    assert np.all(rows[:, W:] == CANARY)
    return rc, rows[:, :W].copy()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 8, 64, 65, 499, 500, 1023, 1024])
def test_reference_transform_equals_scipy(n):
    import scipy.signal
    x = np.random.default_rng(n).standard_normal((3, n))
    got = ref.hilbert_imag(x, n).astype(np.float64)
    want = scipy.signal.hilbert(x, axis=-1).imag
    err = float(np.abs(got - want).max())
    print(f"N = {n}: max |closed form - scipy| = {err:.3e}")
    assert err <= 1e-12 * float(np.abs(x).max())


@pytest.mark.parametrize("W", ref.WS)
def test_hilbert_rows_host(lib, W):
    """Every row of the shared passes, strided rows with canaries between and around them."""
    G, Href = ref.case(W)[:2]
    X, want = G.reshape(-1, W), Href.reshape(-1, W)
    bound = np.stack([ref.hilbert_bound(want[r], W, np.abs(X[r]).max()) for r in range(len(X))])
    for stride in (W, W + 3):
        rc, got = _hilbert_host(lib, X, W, row_stride=stride)
        assert rc == 0
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    if W == 1:
        assert np.all(got == 0)
    print(f"W = {W}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")


def test_hilbert_rows_host_mixed_lengths(lib):
    """Rows of 500, 499, 1 and 0 lags inside W = 500 in one call: each transformed over its own length, zeros beyond."""
    W = 500
    X = np.random.default_rng(11).standard_normal((5, W)).astype(np.float32)
    lens = [500, 499, 1, 0, 499]
    rc, got = _hilbert_host(lib, X, W, row_len=lens, row_stride=W + 4)
    assert rc == 0
    for r, n in enumerate(lens):
        assert np.all(got[r, n:] == 0) and not np.any(np.signbit(got[r, n:]))
        if n:
            want = ref.hilbert_imag(X[r], n).astype(np.float64)
            assert np.all(np.abs(got[r, :n] - want) <= ref.hilbert_bound(want, n, np.abs(X[r, :n]).max())), (r, n)
    assert got[2, 0] == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_hilbert_rows_host_non_finite(lib, bad):
    """A non-finite sample makes its row NaN at every lag below the row's length, at even and odd lengths (the even
    form's zero taps included), and leaves the other rows alone."""
    W = 500
    X = np.random.default_rng(12).standard_normal((4, W)).astype(np.float32)
    X[1, 7] = bad
    X[2, 498] = bad  # under an odd length of 499
    X[3, 499] = bad  # beyond row 3's length: not read
    rc, got = _hilbert_host(lib, X, W, row_len=[500, 500, 499, 499])
    assert rc == 0
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[3]))
    assert np.all(np.isnan(got[1])) and np.all(np.isnan(got[2, :499])) and got[2, 499] == 0


def _select_host(lib, G, H, flat, off, cnt, power, out_stride=None):
    B, K = len(cnt), G[0].size
    out_stride = K + 3 if out_stride is None else out_stride
    out = np.full(PAD + B * out_stride + PAD, CANARY, np.float32)
    body = out[PAD:PAD + B * out_stride]
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (flat, off, cnt)]
    Gc, Hc = np.ascontiguousarray(G, np.float32), np.ascontiguousarray(H, np.float32)
    rc = lib.dvh_select_pws_host(_p(Gc), _p(Hc), K, K, _p(a[0]), _p(a[1]), _p(a[2]), B, ctypes.c_float(power),
                                 _p(body), out_stride)
    assert np.all(out[:PAD] == CANARY) and np.all(out[PAD + B * out_stride:] == CANARY)
    rows = body.reshape(B, out_stride)
    assert np.all(rows[:, K:] == CANARY)
    return rc, rows[:, :K].copy()


def _host_H(lib, G):
    W = G.shape[-1]
    rc, H = _hilbert_host(lib, G.reshape(-1, W), W)
    assert rc == 0
    return H.reshape(G.shape)


@pytest.mark.parametrize("W", ref.WS)
def test_select_pws_host(lib, W):
    """The GPU test's draws (m on both sides of the load group, a repeated pass, offsets neither monotone nor
    disjoint, B = 1 and 6) at every power, every element inside pws_ref.pws_bound; power 0 is the float32 sum in draw
    order divided by m, bit for bit."""
    G, _, flat, tables, sels, stats = ref.case(W)
    H = _host_H(lib, G)
    worst = 0.0
    for (m, B), (off, cnt) in tables.items():
        for power in ref.POWERS:
            rc, got = _select_host(lib, G, H, flat, off, cnt, power)
            assert rc == 0
            for b, (lin, c, mabs) in enumerate(stats[(m, B)]):
                want = ref.weighted(lin, c, power).reshape(-1)
                err = np.abs(got[b].astype(np.float64) - want)
                bound = ref.pws_bound(m, power, mabs).reshape(-1)
                assert np.all(err <= bound), (m, B, power, b)
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
            if power == 0:
                for b, row in enumerate(sels[(m, B)]):
                    acc = np.zeros(G[0].size, np.float32)
                    for j in row:
                        acc += G[j].reshape(-1)
                    assert np.array_equal(got[b], acc / np.float32(m))
    print(f"W = {W}: worst error / bound {worst:.3f}")


def test_select_pws_host_exact_cases(lib):
    """(pass, its negation) is exactly zero; a dead row is zero; a NaN sample turns its row NaN in every draw that holds
    the pass and no other row."""
    W = 65
    G = ref.passes(W)
    G[5, 0, 9] = np.nan
    H = _host_H(lib, G)
    flat = np.array([ref.NEG[1], ref.NEG[0], ref.DEAD[0], ref.DEAD[0], 5, 0, 1], np.int32)
    off = np.array([0, 2, 4, 5, 3], np.int32)
    cnt = np.array([2, 2, 3, 2, 2], np.int32)  # (2, 7), (3, 3), (5, 0, 1), (0, 1), (3, 5)
    for power in (1.0, 2.0, 3.5):
        rc, got = _select_host(lib, G, H, flat, off, cnt, power)
        assert rc == 0
        got = got.reshape(5, ref.R, W)
        assert np.all(got[0] == 0)
        assert np.all(got[1, ref.DEAD[1]] == 0) and np.any(got[1, 0] != 0)
        for b in (2, 4):
            assert np.all(np.isnan(got[b, 0])) and np.all(np.isfinite(got[b, 1:]))
        assert np.all(np.isfinite(got[3]))


def test_entry_refusals(lib):
    """-2 for null pointers, a resample without passes and a power that is negative, non-finite or inside (0, 1); -4 for
    a row longer than 1 024 lags and for B > 65 535; B = 0 and K = 0 return 0; nothing is written in any of them."""
    G = ref.passes(8)
    H = _host_H(lib, G)
    flat, off, cnt = np.arange(4, dtype=np.int32), np.array([0, 1], np.int32), np.array([2, 2], np.int32)
    for power in (-1.0, 0.5, 0.999, float("nan"), float("inf"), -0.25):
        rc, got = _select_host(lib, G, H, flat, off, cnt, power)
        assert rc == -2 and np.all(got == CANARY), power
    for bad_cnt in ([2, 0], [-1, 2]):
        rc, got = _select_host(lib, G, H, flat, off, bad_cnt, 2.0)
        assert rc == -2 and np.all(got == CANARY)
    K = G[0].size
    out = np.full(2 * K, CANARY, np.float32)
    args = [_p(G), _p(H), K, K, _p(flat), _p(off), _p(cnt), 2, ctypes.c_float(2.0), _p(out), K]
    for i in (0, 1, 4, 5, 6, 9):
        a = list(args)
        a[i] = None
        assert lib.dvh_select_pws_host(*a) == -2
        assert lib.dvh_select_pws(*a, None) == -2  # refused on the host, before any device call
    a = list(args)
    a[7] = 65536
    assert lib.dvh_select_pws_host(*a) == -4 and lib.dvh_select_pws(*a, None) == -4
    for i, v in ((7, 0), (3, 0)):
        a = list(args)
        a[i] = v
        assert lib.dvh_select_pws_host(*a) == 0
    a = list(args)
    a[8] = ctypes.c_float(0.5)
    assert lib.dvh_select_pws(*a, None) == -2
    assert np.all(out == CANARY)
    # the transform
    X = np.zeros((2, 1025), np.float32)
    Hh = np.full((2, 1025), CANARY, np.float32)
    assert lib.dvh_hilbert_rows_host(_p(X), 1025, 2, 1025, None, _p(Hh)) == -4
    assert lib.dvh_hilbert_rows(_p(X), 1025, 2, 1025, None, _p(Hh), None) == -4
    assert lib.dvh_hilbert_rows_host(None, 8, 2, 8, None, _p(Hh)) == -2
    assert lib.dvh_hilbert_rows_host(_p(X), 8, 2, 8, None, None) == -2
    assert lib.dvh_hilbert_rows_host(_p(X), 7, 2, 8, None, _p(Hh)) == -2  # rows would overlap
    assert lib.dvh_hilbert_rows_host(_p(X), 8, 2, 8, _p(np.array([8, 9], np.int32)), _p(Hh[1:])) == -2
    assert lib.dvh_hilbert_rows_host(_p(X), 8, 0, 8, None, _p(Hh)) == 0
    assert np.all(Hh[0] == CANARY)
    rc, got = _hilbert_host(lib, np.ones((2, 1024), np.float32), 1024)
    assert rc == 0 and np.all(np.isfinite(got))


def test_check_stack():
    from das_diff_veh_amd import bootstrap as bt
    assert bt.check_stack("linear", 2.0) == 2.0 and bt.check_stack("pws", 0) == 0.0
    assert bt.check_stack("pws", 1) == 1.0 and bt.check_stack("pws", 3.5) == 3.5
    for stack, power in (("mean", 2.0), (None, 2.0), ("PWS", 2.0), ("pws", -1), ("pws", 0.5), ("pws", float("nan")),
                         ("pws", float("inf")), ("pws", "two"), ("pws", None), ("linear", 0.25)):
        with pytest.raises(ValueError):
            bt.check_stack(stack, power)


def test_python_entries_refuse_before_device_work():
    """A stack or power that does not exist raises from the API entries before any window is touched."""
    from das_diff_veh_amd.apis import imaging_classes as ic
    with pytest.raises(ValueError, match="stack"):
        ic.bootstrap_disp(None, 3, 2, None, 0, 0, 0, None, None, None, None, stack="median")
    with pytest.raises(ValueError, match="power"):
        ic.convergence_test(3, None, 2, None, 0, 0, 0, None, None, None, None, stack="pws", pws_power=0.5)
    with pytest.raises(ValueError, match="power"):
        ic.phase_weighted_gather(None, 0, 0, 0, power=-2)
