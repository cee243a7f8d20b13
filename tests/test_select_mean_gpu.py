"""dvh_select_mean / dvh_select_mean_var (csrc/dvh_boot.hip) through the C ABI on both of select_mean_one's paths:
the float4 path (K, both strides and both base addresses multiples of 4 floats) and the grid-stride scalar path
(everything else -- a cache of w = 499 passes alone: K = 19 x 499, base offset 6 x 499 floats).

The reference is NumPy in float32: acc = zeros(K); acc += G[sel[j]] in selection order; acc / float32(m).  The
kernel adds in the same order and divides, so every comparison is np.array_equal(..., equal_nan=True), bit for bit,
and the two paths agree with each other as well.  Each layout's path is asserted from a restatement of
select_vec's predicate on the pointers and strides the call receives.  Every output row sits between canaries (both
ends of the allocation and the gaps a stride leaves); the gaps between G's passes hold NaN, which a read of them
would carry into the result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N_PASS = 11
PAD = 64  # floats of canary on either side of out (a multiple of 4: the padding does not change the alignment)
CANARY = np.float32(-77.25)
KS = [1, 2, 3, 4, 5, 1020, 1023, 1024, 1025, 1028, 2052, 9481, 9500]
MS = [1, 2, 7, 8, 9, 16, 17, 31]


def _ceil4(K):
    return (K + 3) // 4 * 4


# name -> (floats G starts into its allocation, pass_stride(K), floats out starts in, out_stride(K))
LAYOUTS = {
    "aligned": (0, lambda K: _ceil4(K) + 4, 0, lambda K: _ceil4(K) + 4),
    "pass_stride+1": (0, lambda K: K + 1, 0, lambda K: _ceil4(K) + 4),
    "g_lead1": (1, lambda K: _ceil4(K) + 4, 0, lambda K: _ceil4(K) + 4),
    "g_lead2": (2, lambda K: _ceil4(K) + 4, 0, lambda K: _ceil4(K) + 4),
    "g_lead3": (3, lambda K: _ceil4(K) + 4, 0, lambda K: _ceil4(K) + 4),
    "g_lead4": (4, lambda K: _ceil4(K) + 4, 0, lambda K: _ceil4(K) + 4),
    "out_lead1": (0, lambda K: _ceil4(K) + 4, 1, lambda K: _ceil4(K) + 4),
    "out_stride+3": (0, lambda K: _ceil4(K) + 4, 0, lambda K: K + 3),
    "out_stride+4": (0, lambda K: _ceil4(K) + 4, 0, lambda K: K + 4),
}
VEC_LAYOUTS = ("aligned", "g_lead4", "out_stride+4")  # the float4 path when K % 4 == 0; the scalar one otherwise


def _select_vec(g_ptr, pass_stride, K, out_ptr, out_stride):
    """select_vec of csrc/dvh_boot.hip."""
    return K % 4 == 0 and pass_stride % 4 == 0 and out_stride % 4 == 0 and (g_ptr | out_ptr) % 16 == 0


class _Case:
    """G's passes on the device in one layout, and dvh_select_mean[_var] calls into canary-framed outputs."""

    def __init__(self, device, Gv, layout):
        import torch
        self.device, self.K = device, Gv.shape[1]
        K = self.K
        g_lead, ps, self.out_lead, os_ = LAYOUTS[layout]
        self.pass_stride, self.out_stride = ps(K), os_(K)
        buf = np.full(g_lead + N_PASS * self.pass_stride, np.nan, np.float32)
        buf[g_lead:].reshape(N_PASS, self.pass_stride)[:, :K] = Gv
        self.g_alloc = torch.from_numpy(buf).to(device)
        assert self.g_alloc.data_ptr() % 16 == 0
        self.G = self.g_alloc[g_lead:]
        self.expect_vec = K % 4 == 0 and layout in VEC_LAYOUTS

    def _out(self, B):
        import torch
        n = self.out_lead + B * self.out_stride
        alloc = torch.full((PAD + n + PAD,), float(CANARY), dtype=torch.float32, device=self.device)
        assert alloc.data_ptr() % 16 == 0
        return alloc, alloc[PAD + self.out_lead:]

    def _rows(self, alloc, B):
        """The B result rows of an output allocation, every other element asserted to hold its canary."""
        a = alloc.cpu().numpy()
        lo = PAD + self.out_lead
        body = a[lo:lo + B * self.out_stride].reshape(B, self.out_stride)
        assert np.all(a[:lo] == CANARY) and np.all(a[lo + B * self.out_stride:] == CANARY)
        assert np.all(body[:, self.K:] == CANARY)
        return body[:, :self.K].copy()

    def path_is_vec(self, out):
        vec = _select_vec(self.G.data_ptr(), self.pass_stride, self.K, out.data_ptr(), self.out_stride)
        assert vec == self.expect_vec
        return vec

    def mean(self, sel):
        import torch

        from das_diff_veh_amd import _lib
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        B, m = sel.shape
        alloc, out = self._out(B)
        self.path_is_vec(out)
        sel_t = torch.from_numpy(sel).to(self.device)
        _lib.call("dvh_select_mean", _lib.ptr(self.G), self.pass_stride, self.K, _lib.ptr(sel_t), B, m, _lib.ptr(out),
                  self.out_stride, _lib.stream_of(self.device))
        return self._rows(alloc, B)

    def mean_var(self, flat, off, cnt):
        import torch

        from das_diff_veh_amd import _lib
        B = len(cnt)
        alloc, out = self._out(B)
        self.path_is_vec(out)
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device) for a in (flat, off, cnt)]
        _lib.call("dvh_select_mean_var", _lib.ptr(self.G), self.pass_stride, self.K, _lib.ptr(t[0]), _lib.ptr(t[1]),
                  _lib.ptr(t[2]), B, _lib.ptr(out), self.out_stride, _lib.stream_of(self.device))
        return self._rows(alloc, B)


def _reference(Gv, sel):
    out = np.empty((len(sel), Gv.shape[1]), np.float32)
    with np.errstate(invalid="ignore"):
        for b, row in enumerate(sel):
            acc = np.zeros(Gv.shape[1], np.float32)
            for j in row:
                acc += Gv[j]
            out[b] = acc / np.float32(len(row))
    return out


def _passes(K, seed=0):
    return np.random.default_rng(1000 + K + seed).standard_normal((N_PASS, K)).astype(np.float32)


def _selection(rng, B, m):
    sel = rng.integers(0, N_PASS, size=(B, m)).astype(np.int32)
    if m >= 2:
        sel[0, 1] = sel[0, 0]  # a repeated pass in every size that has room for one
    return sel


@pytest.mark.parametrize("K", KS)
def test_shapes_layouts_sizes(device, K):
    """Every K in every layout, m on both sides of the 8-load group (and two groups plus a tail), B = 1 and 3: bit
    equal to the reference on whichever path the layout takes; K % 4 == 0 runs on both, with equal results."""
    Gv = _passes(K)
    rng = np.random.default_rng(K)
    sels = {(m, B): _selection(rng, B, m) for m in MS for B in (1, 3)}
    refs = {k: _reference(Gv, s) for k, s in sels.items()}
    paths = set()
    for layout in LAYOUTS:
        case = _Case(device, Gv, layout)
        paths.add(case.expect_vec)
        for k, sel in sels.items():
            got = case.mean(sel)
            assert np.array_equal(got, refs[k], equal_nan=True), (layout, k, "vec" if case.expect_vec else "scalar")
    assert paths == ({True, False} if K % 4 == 0 else {False})


@pytest.mark.parametrize("K", [1025, 1028, 9481, 9500])
def test_special_values(device, K):
    """NaN, +inf and -inf in one pass (and a -inf under its +inf in another) propagate as NumPy's do, on both
    paths; a selection of one pass returns that pass bit for bit, -0.0 included (sum() of one image is the image:
    VirtualShotGather.__radd__, apis/virtual_shot_gather.py:201-205)."""
    Gv = _passes(K, seed=1)
    Gv[5, 3], Gv[5, 7], Gv[5, K - 1] = np.nan, np.inf, -np.inf
    Gv[6, 7] = -np.inf
    Gv[2, [0, 1, K // 2, K - 1]] = -0.0
    Gv[2, [2, K - 2]] = 0.0
    Gv[2, 5], Gv[2, 6] = np.inf, -np.inf
    sel3 = np.array([[5, 0, 1], [5, 6, 1], [0, 1, 2], [6, 6, 5]], np.int32)
    sel9 = np.array([[0, 1, 2, 3, 4, 7, 8, 9, 5], [5, 1, 2, 3, 4, 7, 8, 9, 6], [10, 1, 2, 3, 4, 7, 8, 9, 0]], np.int32)
    one = np.array([[2], [5], [6], [2]], np.int32)
    for layout in ("aligned", "pass_stride+1", "g_lead2"):
        case = _Case(device, Gv, layout)
        for sel in (sel3, sel9):
            got, ref = case.mean(sel), _reference(Gv, sel)
            assert np.isnan(ref[0, 3]) and ref[0, 7] == np.inf and ref[0, K - 1] == -np.inf and np.isnan(ref[1, 7])
            assert np.array_equal(got, ref, equal_nan=True), layout
        got = case.mean(one)
        assert np.array_equal(got, Gv[one[:, 0]], equal_nan=True)
        assert np.array_equal(got[[0, 3]].view(np.int32), Gv[[2, 2]].view(np.int32)), layout  # signed zeros kept


@pytest.mark.parametrize("K", [4, 1024, 1025, 9481, 9500])
def test_select_mean_var(device, K):
    """Resamples of sizes 1, 8, 9, 3, 17 and 1 at offsets that are neither monotone nor disjoint: each row equals
    dvh_select_mean of the same selection and the reference, on both paths."""
    Gv = _passes(K, seed=2)
    rng = np.random.default_rng(K + 7)
    flat = rng.integers(0, N_PASS, size=30).astype(np.int32)
    cnt = np.array([1, 8, 9, 3, 17, 1], np.int32)
    off = np.array([20, 0, 4, 27, 2, 11], np.int32)
    assert np.all(off + cnt <= flat.size) and np.any(np.diff(off) < 0)
    rows = [flat[o:o + c] for o, c in zip(off, cnt)]
    ref = np.concatenate([_reference(Gv, r[None]) for r in rows])
    paths = set()
    for layout in ("aligned", "pass_stride+1", "g_lead1", "out_stride+3"):
        case = _Case(device, Gv, layout)
        paths.add(case.expect_vec)
        got = case.mean_var(flat, off, cnt)
        assert np.array_equal(got, ref, equal_nan=True), layout
        for b, r in enumerate(rows):
            assert np.array_equal(case.mean(r[None])[0], got[b], equal_nan=True), (layout, b)
    assert paths == ({True, False} if K % 4 == 0 else {False})


def test_refusals_and_empty_calls(device):
    """m = 0 is -2 and B = 65 536 is -4, with out untouched; B = 0 and K = 0 return 0 and write nothing."""
    import torch

    from das_diff_veh_amd import _lib
    K = 8
    case = _Case(device, _passes(K), "aligned")
    sel = torch.zeros(4, dtype=torch.int32, device=device)
    st = _lib.stream_of(device)

    def call(B, m, K_=K):
        alloc, out = case._out(3)
        rc = _lib.load().dvh_select_mean(_lib.ptr(case.G), case.pass_stride, K_, _lib.ptr(sel), B, m, _lib.ptr(out),
                                         case.out_stride, st)
        torch.cuda.synchronize(device)
        assert torch.all(alloc == float(CANARY))
        return rc, out

    rc, out = call(1, 0)
    assert rc == -2
    with pytest.raises(_lib.DvhError, match=r"\(-2\)"):
        _lib.call("dvh_select_mean", _lib.ptr(case.G), case.pass_stride, K, _lib.ptr(sel), 1, 0, _lib.ptr(out),
                  case.out_stride, st)
    rc, out = call(65536, 1)
    assert rc == -4
    with pytest.raises(ValueError):
        _lib.call("dvh_select_mean", _lib.ptr(case.G), case.pass_stride, K, _lib.ptr(sel), 65536, 1, _lib.ptr(out),
                  case.out_stride, st)
    assert call(0, 1)[0] == 0 and call(1, 1, K_=0)[0] == 0
    # the same entry checks of dvh_select_mean_var
    off = torch.zeros(3, dtype=torch.int32, device=device)
    cnt = torch.ones(3, dtype=torch.int32, device=device)
    for B, K_, want in ((65536, K, -4), (0, K, 0), (1, 0, 0)):
        alloc, out = case._out(3)
        rc = _lib.load().dvh_select_mean_var(_lib.ptr(case.G), case.pass_stride, K_, _lib.ptr(sel), _lib.ptr(off),
                                             _lib.ptr(cnt), B, _lib.ptr(out), case.out_stride, st)
        torch.cuda.synchronize(device)
        assert rc == want and torch.all(alloc == float(CANARY))


def test_largest_batch(device):
    """B = 65 535 (the grid's y limit) with K = 4, m = 1: every row is its pass."""
    Gv = _passes(4)
    case = _Case(device, Gv, "aligned")
    sel = (np.arange(65535, dtype=np.int32) * 7 % N_PASS)[:, None]
    got = case.mean(sel)
    assert np.array_equal(got, Gv[sel[:, 0]])
