"""dvh_hilbert_rows / dvh_select_pws (csrc/dvh_pws.hip) through the C ABI, against tests/pws_ref.py (the closed-form
transform in longdouble, the stack's definition in float64) at the bounds derived there.

11 passes of 3 rows per lag count W (one case each), one row all zero, one pass the exact negation of another.  The
select kernel has two load paths, float4 and grid-stride scalar; each layout's path is asserted from a restatement of
the kernel's predicate on the pointers and strides the call receives.  Outputs sit between canaries (both ends of the
allocation and the gaps a stride leaves); the gaps between G's and H's passes hold NaN, which a read of them would
carry into the result.

Worst error / bound ratios measured on an MI355X are recorded in DESIGN.md ("Phase-weighted stack")."""
import ctypes

import numpy as np
import pytest

from tests import pws_ref as ref

pytestmark = pytest.mark.gpu
PAD = 64  # floats of canary on either side of an output (a multiple of 4: the padding does not change the alignment)
CANARY = np.float32(-77.25)


def _ceil4(K):
    return (K + 3) // 4 * 4


# name -> (floats G starts into its allocation, the same for H, pass_stride(K), floats out starts in, out_stride(K))
LAYOUTS = {
    "aligned": (0, 0, lambda K: _ceil4(K) + 4, 0, lambda K: _ceil4(K) + 4),
    "leads4": (4, 8, lambda K: _ceil4(K) + 4, 4, lambda K: _ceil4(K) + 8),
    "pass_stride+1": (0, 0, lambda K: K + 1, 0, lambda K: _ceil4(K) + 4),
    "g_lead1": (1, 0, lambda K: _ceil4(K) + 4, 0, lambda K: _ceil4(K) + 4),
    "h_lead2": (0, 2, lambda K: _ceil4(K) + 4, 0, lambda K: _ceil4(K) + 4),
    "out_lead3": (0, 0, lambda K: _ceil4(K) + 4, 3, lambda K: _ceil4(K) + 4),
    "out_stride+3": (0, 0, lambda K: _ceil4(K) + 4, 0, lambda K: K + 3),
}
VEC_LAYOUTS = ("aligned", "leads4")  # the float4 path when K % 4 == 0; the scalar one otherwise
ALL_POWERS = ("aligned", "pass_stride+1")  # every power on one layout of each path; power 2 on the others


def _pws_vec(g_ptr, h_ptr, pass_stride, K, out_ptr, out_stride):
    """pws_vec of csrc/dvh_pws.hip."""
    return K % 4 == 0 and pass_stride % 4 == 0 and out_stride % 4 == 0 and (g_ptr | h_ptr | out_ptr) % 16 == 0


def _hilbert(device, X, W, row_len=None, row_stride=None):
    """dvh_hilbert_rows of rows X [n_row, W] placed row_stride apart (NaN between them): the H rows, everything the call
    may not write asserted to hold its canary."""
    import torch

    from das_diff_veh_amd import _lib
    n_row = X.shape[0]
    row_stride = W if row_stride is None else row_stride
    xin = np.full(n_row * row_stride, np.nan, np.float32)
    xin.reshape(n_row, row_stride)[:, :W] = X
    x_t = torch.from_numpy(xin).to(device)
    alloc = torch.full((PAD + n_row * row_stride + PAD,), float(CANARY), dtype=torch.float32, device=device)
    rl = None if row_len is None else torch.from_numpy(np.ascontiguousarray(row_len, dtype=np.int32)).to(device)
    _lib.call("dvh_hilbert_rows", _lib.ptr(x_t), row_stride, n_row, W, _lib.ptr(rl), _lib.ptr(alloc[PAD:]),
              _lib.stream_of(device))
    a = alloc.cpu().numpy()
    assert np.all(a[:PAD] == CANARY) and np.all(a[PAD + n_row * row_stride:] == CANARY)
    rows = a[PAD:PAD + n_row * row_stride].reshape(n_row, row_stride)
    assert np.all(rows[:, W:] == CANARY)
    return rows[:, :W].copy()


def _host_hilbert(X, W, row_len=None):
    from das_diff_veh_amd import _lib
    Xc = np.ascontiguousarray(X, np.float32)
    H = np.empty_like(Xc)
    rl = None if row_len is None else np.ascontiguousarray(row_len, dtype=np.int32)
    rc = _lib.load().dvh_hilbert_rows_host(ctypes.c_void_p(Xc.ctypes.data), W, len(Xc), W,
                                           None if rl is None else ctypes.c_void_p(rl.ctypes.data),
                                           ctypes.c_void_p(H.ctypes.data))
    assert rc == 0
    return H


_DEVICE_H = {}


def _device_H(device, W):
    """dvh_hilbert_rows of the shared passes of one lag count, [11, 3, W] on the host (computed once)."""
    if W not in _DEVICE_H:
        G = ref.case(W)[0]
        _DEVICE_H[W] = _hilbert(device, G.reshape(-1, W), W).reshape(G.shape)
    return _DEVICE_H[W]


class _Case:
    """G's and H's passes on the device in one layout, and dvh_select_pws / dvh_select_mean_var calls into
    canary-framed outputs."""

    def __init__(self, device, G, H, layout):
        import torch
        self.device, self.K = device, G[0].size
        K, n = self.K, len(G)
        g_lead, h_lead, ps, self.out_lead, os_ = LAYOUTS[layout]
        self.pass_stride, self.out_stride = ps(K), os_(K)
        self.allocs = []
        for lead, A in ((g_lead, G), (h_lead, H)):
            buf = np.full(lead + n * self.pass_stride, np.nan, np.float32)
            buf[lead:].reshape(n, self.pass_stride)[:, :K] = A.reshape(n, K)
            t = torch.from_numpy(buf).to(device)
            assert t.data_ptr() % 16 == 0
            self.allocs.append(t)
        self.G, self.H = self.allocs[0][g_lead:], self.allocs[1][h_lead:]
        self.expect_vec = K % 4 == 0 and layout in VEC_LAYOUTS

    def _call(self, name, flat, off, cnt, *mid):
        import torch

        from das_diff_veh_amd import _lib
        B = len(cnt)
        n = self.out_lead + B * self.out_stride
        alloc = torch.full((PAD + n + PAD,), float(CANARY), dtype=torch.float32, device=self.device)
        assert alloc.data_ptr() % 16 == 0
        out = alloc[PAD + self.out_lead:]
        vec = _pws_vec(self.G.data_ptr(), self.H.data_ptr(), self.pass_stride, self.K, out.data_ptr(), self.out_stride)
        assert vec == self.expect_vec
        t = [torch.from_numpy(np.array(a, dtype=np.int32)).to(self.device) for a in (flat, off, cnt)]
        src = (_lib.ptr(self.G), _lib.ptr(self.H)) if name == "dvh_select_pws" else (_lib.ptr(self.G),)
        _lib.call(name, *src, self.pass_stride, self.K, _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), B, *mid,
                  _lib.ptr(out), self.out_stride, _lib.stream_of(self.device))
        a = alloc.cpu().numpy()
        lo = PAD + self.out_lead
        body = a[lo:lo + B * self.out_stride].reshape(B, self.out_stride)
        assert np.all(a[:lo] == CANARY) and np.all(a[lo + B * self.out_stride:] == CANARY)
        assert np.all(body[:, self.K:] == CANARY)
        return body[:, :self.K].copy()

    def pws(self, flat, off, cnt, power):
        return self._call("dvh_select_pws", flat, off, cnt, float(power))

    def mean_var(self, flat, off, cnt):
        return self._call("dvh_select_mean_var", flat, off, cnt)


def _host_pws(G, H, flat, off, cnt, power):
    from das_diff_veh_amd import _lib
    K, B = G[0].size, len(cnt)
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (flat, off, cnt)]
    Gc, Hc = np.ascontiguousarray(G, np.float32), np.ascontiguousarray(H, np.float32)
    out = np.empty((B, K), np.float32)
    p = [ctypes.c_void_p(x.ctypes.data) for x in (Gc, Hc, *a, out)]
    rc = _lib.load().dvh_select_pws_host(p[0], p[1], K, K, p[2], p[3], p[4], B, float(power), p[5], K)
    assert rc == 0
    return out


@pytest.mark.parametrize("W", ref.WS)
def test_hilbert_rows(device, W):
    """Every row of the shared passes at row strides W and W + 3, each element inside pws_ref.hilbert_bound."""
    G, Href = ref.case(W)[:2]
    X, want = G.reshape(-1, W), Href.reshape(-1, W)
    bound = np.stack([ref.hilbert_bound(want[r], W, np.abs(X[r]).max()) for r in range(len(X))])
    host = _host_hilbert(X, W)
    for stride in (W, W + 3):
        got = _hilbert(device, X, W, row_stride=stride)
        err = np.abs(got.astype(np.float64) - want)
        ratio = float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))
        print(f"dvh_hilbert_rows W = {W}, stride {stride}: worst error / bound {ratio:.3f}; "
              f"device == host bit for bit: {np.array_equal(got.view(np.int32), host.view(np.int32))}")
        assert np.all(err <= bound), ratio
    if W == 1:
        assert np.all(got == 0)


def test_hilbert_rows_mixed_lengths_and_non_finite(device):
    """Rows of 500, 499, 1 and 0 lags inside W = 500 in one call: each transformed over its own length, zeros beyond;
    a NaN row and an inf row come out NaN below their length (the inf under an even and an odd length) and nowhere
    else; a non-finite sample beyond a row's length is not read."""
    W = 500
    X = np.random.default_rng(11).standard_normal((9, W)).astype(np.float32)
    lens = [500, 499, 1, 0, 499, 500, 500, 499, 499]
    X[5, 7] = np.nan
    X[6, 123] = np.inf
    X[7, 498] = -np.inf
    X[8, 499] = np.nan
    got = _hilbert(device, X, W, row_len=lens, row_stride=W + 4)
    for r, n in enumerate(lens):
        assert np.all(got[r, n:] == 0), r
        if r in (5, 6, 7):
            assert np.all(np.isnan(got[r, :n])), r
        elif n:
            want = ref.hilbert_imag(X[r], n).astype(np.float64)
            assert np.all(np.abs(got[r, :n] - want) <= ref.hilbert_bound(want, n, np.abs(X[r, :n]).max())), (r, n)
    assert got[2, 0] == 0


@pytest.mark.parametrize("W", ref.WS)
def test_select_pws(device, W):
    """m on both sides of the 4-load group (with a repeated pass), B = 1 and 6, offsets neither monotone nor disjoint,
    every layout, every power: each element inside pws_ref.pws_bound; power 0 equals dvh_select_mean_var bit for
    bit; K % 4 == 0 runs on both load paths."""
    G, _, flat, tables, _, stats = ref.case(W)
    H = _device_H(device, W)
    worst, paths, same_as_host = 0.0, set(), {p: True for p in ref.POWERS}
    for layout in LAYOUTS:
        case = _Case(device, G, H, layout)
        paths.add(case.expect_vec)
        for (m, B), (off, cnt) in tables.items():
            for power in (ref.POWERS if layout in ALL_POWERS else (2.0,)):
                got = case.pws(flat, off, cnt, power)
                for b, (lin, c, mabs) in enumerate(stats[(m, B)]):
                    err = np.abs(got[b].astype(np.float64) - ref.weighted(lin, c, power).reshape(-1))
                    bound = ref.pws_bound(m, power, mabs).reshape(-1)
                    ratio = float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))
                    worst = max(worst, ratio)
                    assert np.all(err <= bound), (layout, m, B, power, b, ratio)
                if power == 0:
                    lin32 = case.mean_var(flat, off, cnt)
                    assert np.array_equal(got.view(np.int32), lin32.view(np.int32)), (layout, m, B)
                if layout == "aligned":
                    host = _host_pws(G, H, flat, off, cnt, power)
                    same_as_host[power] &= bool(np.array_equal(got.view(np.int32), host.view(np.int32)))
    assert paths == ({True, False} if (3 * W) % 4 == 0 else {False})
    print(f"dvh_select_pws W = {W}: worst error / bound {worst:.3f}; device == host bit for bit, by power: "
          f"{same_as_host}")


@pytest.mark.parametrize("W", [8, 65])
def test_select_pws_exact_cases(device, W):
    """On both load paths: power 0 is dvh_select_mean_var bit for bit with -0.0 samples (a draw of one pass returns
    it, signed zeros included); (pass, its negation) is exactly +-0 everywhere; a dead row gives 0; a NaN sample turns
    its whole row NaN in every draw that holds the pass, and no other row."""
    G = ref.passes(W, seed=1)
    G[0, 0, [0, W - 1]] = -0.0
    G[1, 2, W // 2] = -0.0
    G[5, 0, W // 3] = np.nan
    H = _hilbert(device, G.reshape(-1, W), W).reshape(G.shape)
    assert np.all(np.isnan(H[5, 0])) and np.all(np.isfinite(H[5, 1:])) and np.all(H[ref.DEAD] == 0)
    flat = np.array([ref.NEG[1], ref.NEG[0], ref.DEAD[0], ref.DEAD[0], 5, 0, 1], np.int32)
    off = np.array([0, 2, 4, 5, 3, 5, 6], np.int32)
    cnt = np.array([2, 2, 3, 2, 2, 1, 1], np.int32)  # (2, 7), (3, 3), (5, 0, 1), (0, 1), (3, 5), (0), (1)
    for layout in ("aligned", "pass_stride+1"):
        case = _Case(device, G, H, layout)
        assert case.expect_vec == (layout == "aligned" and W == 8)
        lin32 = case.mean_var(flat, off, cnt)
        got = case.pws(flat, off, cnt, 0.0)
        assert np.array_equal(got.view(np.int32), lin32.view(np.int32))
        assert np.array_equal(got[5].view(np.int32), G[0].reshape(-1).view(np.int32))
        assert np.array_equal(got[6].view(np.int32), G[1].reshape(-1).view(np.int32))
        for power in (1.0, 2.0, 3.5):
            got = case.pws(flat, off, cnt, power).reshape(len(cnt), ref.R, W)
            assert np.all(got[0] == 0)
            assert np.all(got[1, ref.DEAD[1]] == 0) and np.any(got[1, 0] != 0)
            for b in (2, 4):
                assert np.all(np.isnan(got[b, 0])) and np.all(np.isfinite(got[b, 1:])), (layout, power, b)
            assert np.all(np.isfinite(got[3]))
            # one pass: every phasor has modulus 1 up to its roundings, so the stack is the pass within the bound
            one = np.abs(got[6].astype(np.float64) - G[1])
            assert np.all(one <= ref.pws_bound(1, power, np.abs(G[1])))


def test_empty_calls_write_nothing(device):
    """B = 0 and K = 0 return 0 and write nothing; n_row = 0 and W = 0 likewise; a resample without passes reads no pass
    and comes out NaN (cnt lives on the device: only the host twin can refuse it)."""
    import torch

    from das_diff_veh_amd import _lib
    G = ref.passes(8)
    H = _hilbert(device, G.reshape(-1, 8), 8).reshape(G.shape)
    case = _Case(device, G, H, "aligned")
    K = case.K
    out = torch.full((2 * case.out_stride,), float(CANARY), dtype=torch.float32, device=device)
    tabs = [torch.zeros(4, dtype=torch.int32, device=device), torch.zeros(2, dtype=torch.int32, device=device),
            torch.ones(2, dtype=torch.int32, device=device)]
    st = _lib.stream_of(device)
    lib = _lib.load()
    for B, K_ in ((0, K), (2, 0)):
        rc = lib.dvh_select_pws(_lib.ptr(case.G), _lib.ptr(case.H), case.pass_stride, K_, _lib.ptr(tabs[0]),
                                _lib.ptr(tabs[1]), _lib.ptr(tabs[2]), B, 2.0, _lib.ptr(out), case.out_stride, st)
        assert rc == 0
    for n_row, W in ((0, 8), (3, 0)):
        assert lib.dvh_hilbert_rows(_lib.ptr(case.G), 8, n_row, W, None, _lib.ptr(out), st) == 0
    torch.cuda.synchronize(device)
    assert torch.all(out == float(CANARY))
    got = case.pws(np.zeros(4, np.int32), [0, 1], [1, 0], 2.0)
    assert np.all(np.isfinite(got[0])) and np.all(np.isnan(got[1]))
