"""dvh_ridge (csrc/dvh_boot.hip: ridge_kernel) through the C ABI against oracle.ridge.extract_ridge_ref_idx, on
inputs built to decide every rule of the walk rather than on smooth f-v maps:

  * the velocity axis 200 + 10 arange(nV) (reversed), so that a window bound v +- sigma sits between grid velocities
    (sigma = 25), exactly on one (sigma = 30: the strict < / > decides) or outside the axis (sigma = 1e6);
  * tie-rich images (8 levels: nearly every window holds equal maxima, across lanes and within one lane's rows) and
    the same with NaN, +inf and -inf sprinkled in and an all-NaN, an all -inf and a constant column in the band
    (np.argmax: the first NaN wins, then the first maximum);
  * nV at every rows-per-lane count of the register-held axis (1, 2, 3, 16 rows, ragged and full last lanes) and past
    it (the global-memory search); bands of 3 to 1 024 columns with savgol windows 3, 5 and 25;
  * the band at column c0 = 0 and 3 of a wider image whose other columns hold NaN and 1e30, images b_stride =
    nV nF + 7 apart with 1e30 between them, three different images per call.

The raw picks are asserted EQUAL to the oracle's; the smoothed ridge is held to 1e-9 absolute (an sgl-term float64
dot product; the bound of tests/test_boot_gpu.py); vel_max mode is asserted equal.  out, picks and status sit
between canaries."""
import numpy as np
import pytest

from oracle import ridge as orid

pytestmark = pytest.mark.gpu
B = 3
PAD = 16
CANARY = -77.25
ST_CANARY = -7
LEAD = 5  # floats the first image starts into its allocation
NVS = [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1500]
BANDS = [(3, 3), (5, 5), (25, 25), (26, 25), (64, 25), (65, 5), (130, 25), (1024, 25)]
INT32_MIN = -2 ** 31
_worst = {"smooth": 0.0}


def _vels(nV):
    return 200.0 + 10.0 * np.arange(nV)


def _images(nV, nb, c0, kind, seed=0):
    """[B, nV, nF] float32, nF = c0 + nb + 2."""
    nF = c0 + nb + 2
    rng = np.random.default_rng(100003 * nV + 101 * nb + 7 * c0 + seed + (50 if kind == "special" else 0))
    img = (rng.integers(0, 8, size=(B, nV, nF)) / 4.0).astype(np.float32)
    if kind == "special":
        u = rng.random((B, nV, nF))
        img[u < 0.03] = np.nan
        img[(u >= 0.03) & (u < 0.06)] = np.inf
        img[(u >= 0.06) & (u < 0.09)] = -np.inf
        img[:, :, c0 + nb // 2] = np.nan
        img[:, :, c0] = -np.inf
        img[:, :, c0 + nb - 1] = 0.75
    for c in list(range(c0)) + [c0 + nb, c0 + nb + 1]:  # a read outside the band would win every argmax
        img[:, :, c] = np.nan if c % 2 == 0 else 1e30
    return img


def _curve(nV, nb, seed):
    """Reference velocities inside the axis: even columns on grid velocities, odd ones halfway between two."""
    rng = np.random.default_rng(seed)
    k = 2 * rng.integers(0, nV, size=nb)
    if nV > 1:
        odd = np.arange(nb) % 2 == 1
        k[odd] = 2 * rng.integers(0, nV - 1, size=int(odd.sum())) + 1
    return 200.0 + 5.0 * k


class _Dev:
    """One image batch, its velocity axis and savgol operator on the device; calls into canary-framed outputs."""

    def __init__(self, device, img, c0, nb, sgl):
        import torch

        from das_diff_veh_amd.disp import savgol_operator
        self.device, self.img, self.c0, self.nb, self.sgl = device, img, c0, nb, sgl
        _, self.nV, self.nF = img.shape
        self.b_stride = self.nV * self.nF + 7
        buf = np.full(LEAD + B * self.b_stride, 1e30, np.float32)
        buf[LEAD:].reshape(B, self.b_stride)[:, :self.nV * self.nF] = img.reshape(B, -1)
        self.fv = torch.from_numpy(buf).to(device)[LEAD:]
        self.vels = _vels(self.nV)
        self.vel_t = torch.from_numpy(self.vels[::-1].copy()).to(device)
        h, el, er = savgol_operator(sgl, 2)  # as bootstrap._sg_ridge builds it
        self.sg = torch.from_numpy(np.concatenate([h, el.ravel(), er.ravel()])).to(device)

    def buffers(self):
        import torch
        n = PAD + B * self.nb + PAD
        return (torch.full((n,), CANARY, dtype=torch.float64, device=self.device),
                torch.full((2 * PAD + B,), ST_CANARY, dtype=torch.int32, device=self.device),
                torch.full((n,), CANARY, dtype=torch.float64, device=self.device))

    def launch(self, bufs, ref, sigma, vel_max=0.0, vref=None, images=(0, B), picks=True, raw=False, **over):
        """dvh_ridge on images [a, b) of the batch into rows [a, b) of the buffers.  raw=True returns the status
        code instead of raising; ``over`` replaces named arguments (the refusal cases)."""
        import torch

        from das_diff_veh_amd import _lib
        out, status, pk = bufs
        a, b = images
        vref_t = None if vref is None else torch.from_numpy(np.ascontiguousarray(vref, np.float64)).to(self.device)
        args = dict(fv=_lib.ptr(self.fv[a * self.b_stride:]), b_stride=self.b_stride, B=b - a, nV=self.nV, nF=self.nF,
                    c0=self.c0, nb=self.nb, vel=_lib.ptr(self.vel_t), ref=ref, sigma=float(sigma),
                    vel_max=float(vel_max), vref=_lib.ptr(vref_t), sg=_lib.ptr(self.sg), sgl=self.sgl,
                    out=_lib.ptr(out[PAD + a * self.nb:]), status=_lib.ptr(status[PAD + a:]),
                    picks=_lib.ptr(pk[PAD + a * self.nb:]) if picks else None, stream=_lib.stream_of(self.device))
        args.update(over)
        if raw:
            rc = _lib.load().dvh_ridge(*args.values())
        else:
            rc = _lib.call("dvh_ridge", *args.values())
        torch.cuda.synchronize(self.device)
        return rc

    def read(self, bufs):
        """(out [B, nb], status [B], picks [B, nb]) with the canaries on both sides asserted."""
        out, status, pk = (t.cpu().numpy() for t in bufs)
        for a in (out, pk):
            assert np.all(a[:PAD] == CANARY) and np.all(a[-PAD:] == CANARY)
        assert np.all(status[:PAD] == ST_CANARY) and np.all(status[-PAD:] == ST_CANARY)
        return out[PAD:-PAD].reshape(B, self.nb), status[PAD:-PAD], pk[PAD:-PAD].reshape(B, self.nb)

    def untouched(self, bufs):
        out, status, pk = (t.cpu().numpy() for t in bufs)
        return np.all(out == CANARY) and np.all(pk == CANARY) and np.all(status == ST_CANARY)

    def run(self, ref, sigma, vel_max=0.0, vref=None):
        bufs = self.buffers()
        self.launch(bufs, ref, sigma, vel_max, vref)
        return self.read(bufs)

    def oracle(self, b, ref, sigma, vel_max=0.0, vref=None):
        """(smoothed, picks) of image b, or None where the reference raises (an empty window)."""
        band = self.img[b][:, self.c0:self.c0 + self.nb].astype(np.float64)
        try:
            r = orid.extract_ridge_ref_idx(np.arange(self.nb, dtype=np.float64), self.vels, band,
                                           ref_freq_idx=None if ref == INT32_MIN else ref, sigma=sigma,
                                           vel_max=vel_max, ref_vel=None if vref is None else (lambda f: vref),
                                           return_picks=True, window_length=self.sgl)
        except ValueError:
            return None
        return (r, r) if ref == INT32_MIN else r

    def check(self, ref, sigma, vel_max=0.0, vref=None, what=""):
        out, status, pk = self.run(ref, sigma, vel_max, vref)
        assert np.array_equal(status, np.zeros(B, np.int32)), (what, status)
        for b in range(B):
            o = self.oracle(b, ref, sigma, vel_max, vref)
            assert o is not None, (what, b, "the reference raises: the case is not the one intended")
            np.testing.assert_array_equal(pk[b], o[1], err_msg=f"{what} image {b}: raw picks")
            if ref == INT32_MIN:
                np.testing.assert_array_equal(out[b], o[0], err_msg=f"{what} image {b}: vel_max")
            else:
                err = float(np.abs(out[b] - o[0]).max())
                _worst["smooth"] = max(_worst["smooth"], err)
                assert err <= 1e-9, (what, b, err)


def _refs(nb):
    return sorted({0, nb // 2, nb - 1, -1, max(-3, -nb), -nb})


def _vel_max_positions(nV):
    v = _vels(nV)
    mid = v[nV // 2]
    return [mid, mid + 5.0 if nV > 1 else mid, 100.0, v[-1] + 1000.0]  # on the grid, halfway, below, above the axis


def _all_modes(device, nV, nb, sgl):
    # long bands (the oracle's walk of them takes seconds): each image at one band position instead of both
    combos = [("tie", 0), ("special", 3)] if nb >= 130 else [(k, c) for k in ("tie", "special") for c in (0, 3)]
    for kind, c0 in combos:
        d = _Dev(device, _images(nV, nb, c0, kind), c0, nb, sgl)
        for ref in _refs(nb):
            for sigma in (25, 30, 1e6):
                d.check(ref, sigma, what=f"walk {kind} nV={nV} nb={nb} c0={c0} ref={ref} sigma={sigma}")
        vref = _curve(nV, nb, seed=nV + nb + c0)
        for sigma in (25, 30, 50):
            d.check(0, sigma, vref=vref, what=f"curve {kind} nV={nV} nb={nb} c0={c0} sigma={sigma}")
        for vm in _vel_max_positions(nV):
            d.check(INT32_MIN, 25, vel_max=vm, what=f"vel_max {kind} nV={nV} nb={nb} c0={c0} vel_max={vm}")
    print(f"dvh_ridge nV={nV} nb={nb} sgl={sgl}: worst |smoothed - oracle| so far {_worst['smooth']:.3e}")


@pytest.mark.parametrize("nV", NVS)
def test_every_velocity_axis_size(device, nV):
    """Band (26, 25), every reference index, sigma and mode, both images, c0 = 0 and 3."""
    _all_modes(device, nV, 26, 25)


@pytest.mark.parametrize("nb,sgl", BANDS)
@pytest.mark.parametrize("nV", [65, 1025])
def test_every_band_shape(device, nV, nb, sgl):
    """Bands of 3 (= sgl) to 1 024 (kMaxBand) columns on the register-held and the global-memory axis."""
    _all_modes(device, nV, nb, sgl)


def test_vel_max_halfway_takes_the_higher_velocity(device):
    """vel_max halfway between two grid velocities: equal distances, np.argmin takes the first row (the higher
    velocity), so the picks come from the rows at and below it -- the row above must never be picked although it
    holds the column maximum."""
    nV, nb = 65, 26
    img = _images(nV, nb, 0, "tie")
    k = 20  # rows k and k + 1 (descending) are equally far from vel_max
    img[:, :k, :] = 0.0
    img[:, k, :nb] = 5.0
    img[:, k - 1, :nb] = 9.0  # outside the search: rows [k, nV)
    d = _Dev(device, img, 0, nb, 25)
    v_desc = d.vels[::-1]
    vm = (v_desc[k] + v_desc[k + 1]) / 2
    d.check(INT32_MIN, 25, vel_max=vm, what="vel_max halfway")
    out, _, pk = d.run(INT32_MIN, 25, vel_max=vm)
    assert np.all(out == v_desc[k]) and np.all(pk == v_desc[k])


def test_vel_max_picks_at_ridges_level(device):
    """ridges(ref_freq_idx=None, return_picks=True): the raw picks are the result (the kernel writes both)."""
    import torch

    from das_diff_veh_amd.bootstrap import ridges
    nV, nb = 129, 26
    img = _images(nV, nb, 0, "special")
    freqs = np.arange(img.shape[2], dtype=np.float64)
    d = _Dev(device, img, 0, nb, 25)
    fv = torch.from_numpy(img).to(device)
    for vm in _vel_max_positions(nV):
        out, pk = ridges(fv, freqs, d.vels, 0, nb, ref_freq_idx=None, vel_max=vm, return_picks=True)
        want = np.stack([d.oracle(b, INT32_MIN, 25, vel_max=vm)[0] for b in range(B)])
        np.testing.assert_array_equal(out, want)
        np.testing.assert_array_equal(pk, want)
        np.testing.assert_array_equal(ridges(fv, freqs, d.vels, 0, nb, ref_freq_idx=None, vel_max=vm), want)


def test_empty_windows_set_status(device):
    """A window that holds no velocity: the reference raises, status[b] = 1.  vref = 505 (off the grid) with sigma = 4
    is empty, with sigma = 5.5 it is not.  vref and sigma are arguments of the call, shared by its images, so the one
    image with the off-grid curve is a call of its own: three calls of one image each into rows 0, 1, 2 of the same
    out / picks / status buffers (each writes its own row only: status == [0, 1, 0]), then whole batches."""
    nV, nb = 65, 26
    d = _Dev(device, _images(nV, nb, 3, "tie"), 3, nb, 25)
    on_grid = 200.0 + 10.0 * np.random.default_rng(3).integers(0, nV, size=nb)
    off_grid = np.full(nb, 505.0)
    assert d.oracle(1, 0, 4, vref=off_grid) is None and d.oracle(1, 0, 5.5, vref=off_grid) is not None
    bufs = d.buffers()
    for b, vref in enumerate((on_grid, off_grid, on_grid)):
        d.launch(bufs, 0, 4, vref=vref, images=(b, b + 1))
    out, status, pk = d.read(bufs)
    assert status.tolist() == [0, 1, 0]
    for b in (0, 2):
        sm, picks = d.oracle(b, 0, 4, vref=on_grid)
        np.testing.assert_array_equal(pk[b], picks)
        assert np.abs(out[b] - sm).max() <= 1e-9
    assert d.run(0, 4, vref=off_grid)[1].tolist() == [1, 1, 1]
    assert d.run(0, 5.5, vref=off_grid)[1].tolist() == [0, 0, 0]
    d.check(0, 4, vref=on_grid, what="grid-valued curve, sigma = 4")
    # the walk with sigma = 0: (v, v) holds nothing
    assert all(d.oracle(b, 5, 0) is None for b in range(B))
    assert d.run(5, 0)[1].tolist() == [1, 1, 1]
    assert d.run(-3, 0)[1].tolist() == [1, 1, 1]


def test_refusals(device):
    """The entry point's argument checks: each returns its code (-2 invalid argument -> DvhError, -4 unsupported
    size -> ValueError) and launches nothing: out, picks and status keep their canaries."""
    from das_diff_veh_amd import _lib
    nV, nb = 4, 26
    img = _images(nV, 1100, 0, "tie")  # wide enough that every refused band still lies inside the allocation
    d = _Dev(device, img, 0, nb, 25)
    import torch
    big = tuple(torch.full((2 * PAD + B * 1100,), CANARY if k != 1 else ST_CANARY, dtype=t, device=device)
                for k, t in enumerate((torch.float64, torch.int32, torch.float64)))
    cases = [
        ("even sgl", dict(sgl=24), -4), ("sgl > nb", dict(sgl=27), -4), ("ref = nb", dict(ref=nb), -2),
        ("ref = -nb - 1", dict(ref=-nb - 1), -2), ("nb = 1025", dict(nb=1025, ref=0), -4),
        ("c0 + nb > nF", dict(c0=d.nF - nb + 1), -2), ("nb = 0", dict(nb=0), -2), ("NULL fv", dict(fv=None), -2),
        ("NULL vel", dict(vel=None), -2), ("NULL out", dict(out=None), -2), ("NULL status", dict(status=None), -2),
    ]
    for name, over, want in cases:
        for vref in (None, np.full(nb, 300.0)):
            if name == "nb = 1025" and vref is not None:
                vref = np.full(1025, 300.0)
            ref, rest = over.get("ref", 3), {k: v for k, v in over.items() if k != "ref"}
            assert d.launch(big, ref, 25, vref=vref, raw=True, **rest) == want, name
            assert d.untouched(big), name
            with pytest.raises(ValueError if want == -4 else _lib.DvhError, match=None if want == -4 else r"\(-2\)"):
                d.launch(big, ref, 25, vref=vref, **rest)
            assert d.untouched(big), name
    # vel_max mode smooths nothing and takes any sgl; B = 0 launches nothing
    assert d.launch(big, INT32_MIN, 25, vel_max=300.0, raw=True, B=0) == 0 and d.untouched(big)
    bufs = d.buffers()
    assert d.launch(bufs, INT32_MIN, 25, vel_max=300.0, raw=True, sgl=24, sg=None) == 0
    assert np.array_equal(d.read(bufs)[1], np.zeros(B, np.int32))
