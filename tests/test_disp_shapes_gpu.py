"""The f-k half of the dispersion chain (dvh_disp_row_l1 -> dvh_disp_tdft -> dvh_disp_fk -> dvh_disp_fv*) against
float64 references at the gather shapes where its kernels change path: MFMA tile edges, the float4 / scalar loads,
both forms of tdft_rows_kernel and the atomic fallback, the padded contraction tables, the tiled contraction above
160 KB of LDS, slot accumulation, and |FK| grids on each side of the sampling kernels' staging limits.
tests/disp_shapes.py lists the geometries, tests/test_disp_shapes_host.py pins their plan arithmetic.

Bounds.  (a, b) a float64 dot product of nt terms with |w| <= 1 is off by at most nt 2^-53 sum_t |x_t|; the same
for the NumPy reference, hence 2 nt 2^-53 sum_t |x_t| per row, times the row's scale.  (c, d) |FK| within 1e-11
of the grid's peak against float64 fft2 and 1e-12 between the two forms, the bounds of tests/test_fk_gpu.py.
(e) 8 float64 additions in any order cost under 2e-15: 1e-13 of the peak.  (f, g) rel-err < 1e-4 and the
SURVEY 8(d) pick rule on every column, as tests/test_fv_batch_gpu.py.  Measured values: DESIGN.md.
"""
import warnings

import numpy as np
import pytest

from tests import disp_shapes as ds

pytestmark = pytest.mark.gpu

CANARY = -7.0
PAD = 32
TOL = 1e-4
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------ helpers
def _twiddles(nt, n_fb, j_lo=3):
    """wt[nt][2 * n_fb] = cos | -sin of n_fb consecutive bins of the nf-point transform, as DispPlan builds it."""
    nf = 2 ** (1 + int(np.ceil(np.log2(nt))))
    nu = (np.arange(j_lo, j_lo + n_fb) - nf // 2) % nf
    ang = 2.0 * np.pi * ((np.outer(np.arange(nt), nu) % nf) / nf)
    wt = np.empty((nt, 2 * n_fb))
    wt[:, 0::2] = np.cos(ang)
    wt[:, 1::2] = -np.sin(ang)
    return wt


LAYOUTS = ["contig", "stride5", "odd", "chslice", "tslice"]


def _place(x, layout, device):
    """A device view [B, nch, nt] holding x: 'contig'; 'stride5' (channel stride nt + 5: rows at every alignment);
    'odd' (base one element into the buffer); 'chslice' (channels 2 .. 2 + nch of a wider gather); 'tslice' (the
    first nt samples of a longer record)."""
    import torch
    B, nch, nt = x.shape
    if layout == "chslice":
        view = torch.zeros((B, nch + 5, nt), dtype=torch.float32, device=device)[:, 2:2 + nch, :]
    elif layout == "tslice":
        view = torch.zeros((B, nch, nt + 12), dtype=torch.float32, device=device)[:, :, :nt]
    else:
        stride = nt + 5 if layout == "stride5" else nt
        off = 1 if layout == "odd" else 0
        buf = torch.zeros(B * nch * stride + off, dtype=torch.float32, device=device)
        view = buf[off:].view(B, nch, stride)[:, :, :nt]
    view.copy_(torch.from_numpy(x))
    return view


def _tdft(xv, wt_dev, n_fb, scale):
    """dvh_disp_tdft into the middle of a canary-filled buffer: (D as numpy, canaries intact)."""
    import torch

    from das_diff_veh_amd import _lib
    B, nch, nt = xv.shape
    n = B * nch * 2 * n_fb
    buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float64, device=xv.device)
    _lib.call("dvh_disp_tdft", _lib.ptr(xv), xv.stride(0), xv.stride(1), B, nch, nt, _lib.ptr(wt_dev), n_fb,
              _lib.ptr(scale), _lib.ptr(buf[PAD:PAD + n]), _lib.stream_of(xv.device))
    b = buf.cpu().numpy()
    return b[PAD:PAD + n].reshape(B * nch, 2 * n_fb), bool((b[:PAD] == CANARY).all() and (b[PAD + n:] == CANARY).all())


def _tdft_case(B, nch, nt, n_fb, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, nch, nt)).astype(np.float32)
    scale = rng.uniform(0.25, 4.0, B * nch).astype(np.float32)
    wt = _twiddles(nt, n_fb)
    x64 = x.reshape(B * nch, nt).astype(np.float64)
    return x, scale, wt, x64 @ wt, 2.0 * nt * U * np.abs(x64).sum(axis=1)


def _rows_blocks(M, n_fb):
    """dvh_disp_tdft's block count of the plain form: 64-row x 112-column tiles."""
    return -(-M // 64) * -(-2 * n_fb // 112)


def _plain_form(M, n_fb, device):
    """The launcher's choice: the K-split form while blocks * 4 < CU count."""
    import torch
    return _rows_blocks(M, n_fb) * 4 >= torch.cuda.get_device_properties(device).multi_processor_count


def _fft2_ref(x64, plan):
    full = np.abs(np.fft.fftshift(np.fft.fft2(x64, s=[plan.nk, plan.nf])))
    return full[plan.m_lo:plan.m_lo + plan.n_kb, plan.j_lo:plan.j_lo + plan.n_fb]


def _plan(nch, nt, nF=47, nV=33, dx=ds.DX, _cache={}):
    from das_diff_veh_amd.disp import DispPlan
    key = (nch, nt, nF, nV, dx)
    if key not in _cache:
        _cache[key] = DispPlan(nch, nt, dx, ds.DT, *ds.axes(nF, nV))
    return _cache[key]


# ------------------------------------------------------------------------------------------ (a) the time-DFT GEMM
# (B, nch, nt, n_fb, plain form): every n_fb of {1, 8, 16, 17, 56, 57, 112, 113}, nt of {8, 31, 32, 33, 257, 500},
# nch of {1, 2, 17, 25} and M = B nch of {1, 15, 16, 17, 63, 65}; the plain rows need >= 64 blocks
TDFT_CASES = [
    (1, 1, 8, 1, False), (15, 1, 31, 8, False), (8, 2, 32, 16, False), (1, 17, 33, 17, False),
    (63, 1, 257, 57, False), (65, 1, 500, 113, False), (1, 25, 500, 112, False), (2, 25, 257, 56, False),
    (162, 25, 8, 56, True), (129, 17, 31, 57, True), (1000, 2, 33, 112, True), (56, 25, 257, 113, True),
    (4100, 1, 32, 17, True), (241, 17, 500, 1, True),
]


@pytest.mark.parametrize("B,nch,nt,n_fb,plain", TDFT_CASES)
def test_tdft_is_the_float64_gemm(device, B, nch, nt, n_fb, plain):
    """D = x @ wt per row within the dot-product bound, bitwise the same from every input layout (only the loads
    differ: float4 when the strides and the base are 4-element aligned, scalar otherwise), with and without
    row_scale, nothing written outside D."""
    import torch
    M = B * nch
    assert (_rows_blocks(M, n_fb) >= 64) == plain and _plain_form(M, n_fb, device) == plain
    x, scale, wt, ref, bound = _tdft_case(B, nch, nt, n_fb, seed=1000 * n_fb + nt)
    wt_dev = torch.from_numpy(wt).to(device)
    assert wt_dev.data_ptr() % 16 == 0
    scale_dev = torch.from_numpy(scale).to(device)
    worst = 0.0
    for sc_dev, sc in ((None, np.ones(M)), (scale_dev, scale.astype(np.float64))):
        first = None
        for layout in LAYOUTS:
            xv = _place(x, layout, device)
            vec4 = xv.data_ptr() % 16 == 0 and xv.stride(0) % 4 == 0 and xv.stride(1) % 4 == 0
            # which loads the kernel takes: 'odd' is always scalar, 'stride5' float4 only for nt = 3 (mod 4)
            assert vec4 == (layout != "odd" and xv.stride(1) % 4 == 0), layout
            assert layout != "contig" or vec4 == (nt % 4 == 0)
            got, intact = _tdft(xv, wt_dev, n_fb, sc_dev)
            assert intact, layout
            if first is None:
                first = got
                err = np.abs(got - ref * sc[:, None]).max(axis=1)
                lim = bound * sc
                worst = max(worst, float((err / lim).max()))
                assert np.all(err <= lim), (layout, float((err / lim).max()))
            else:
                assert np.array_equal(got, first), layout
    print(f"tdft rows B={B} nch={nch} nt={nt} n_fb={n_fb}: worst err / bound = {worst:.3g}")


# ------------------------------------------------------------------------------------------ (b) the atomic fallback
def _gemm_slices(M, N, nt):
    """dvh_disp_tdft's split-K choice for tdft_gemm_kernel: (kslice, slices)."""
    tiles = -(-M // 32) * -(-N // 32)
    splits = -(-1024 // tiles)
    kslice = -(-nt // splits)
    kslice = 64 if kslice < 64 else -(-kslice // 4) * 4
    return kslice, -(-nt // kslice)


@pytest.mark.parametrize("B,nch,nt,n_fb,slices", [(82, 25, 500, 57, (128, 4)), (1, 25, 500, 112, (64, 8)),
                                                   (3, 17, 33, 17, (64, 1)), (1, 1, 8, 1, (64, 1)),
                                                   (65, 1, 257, 113, (64, 5))])
def test_tdft_atomic_fallback(device, B, nch, nt, n_fb, slices):
    """A twiddle table 8 bytes off a 16-byte boundary cannot feed the LDS-DMA of tdft_rows_kernel: the launcher takes
    tdft_gemm_kernel (split K, float64 atomics into a zeroed D).  Same bound; (82, 25, 500, 57) has nt > 64 * slices
    (4 slices of 128 samples add into each tile), the others 64-sample slices, two shapes have nt < 64."""
    import torch
    M = B * nch
    assert _gemm_slices(M, 2 * n_fb, nt) == slices
    x, scale, wt, ref, bound = _tdft_case(B, nch, nt, n_fb, seed=7000 + nt + n_fb)
    wbuf = torch.zeros(wt.size + 1, dtype=torch.float64, device=device)
    wt_dev = wbuf[1:].view(nt, 2 * n_fb)
    wt_dev.copy_(torch.from_numpy(wt))
    assert wt_dev.data_ptr() % 16 == 8
    scale_dev = torch.from_numpy(scale).to(device)
    worst = 0.0
    for layout in ("contig", "stride5"):
        xv = _place(x, layout, device)
        for sc_dev, sc in ((None, np.ones(M)), (scale_dev, scale.astype(np.float64))):
            got, intact = _tdft(xv, wt_dev, n_fb, sc_dev)
            assert intact
            err, lim = np.abs(got - ref * sc[:, None]).max(axis=1), bound * sc
            worst = max(worst, float((err / lim).max()))
            assert np.all(err <= lim), (layout, float((err / lim).max()))
    print(f"tdft atomic B={B} nch={nch} nt={nt} n_fb={n_fb}: worst err / bound = {worst:.3g}")


# ------------------------------------------------------------------------------------------ (c) both forms of tdft_rows
@pytest.mark.parametrize("nch,nt,B", [(17, 257, 117), (33, 499, 61)])
def test_fk_grid_split_and_plain_forms_agree(device, nch, nt, B):
    """Two gathers alone (K-split form) and as the first two of a batch of >= 64 blocks (plain form): |FK| agrees to
    1e-12 of the peak, and both match float64 fft2 to 1e-11."""
    import torch

    from das_diff_veh_amd.disp import fk_grid
    plan = _plan(nch, nt)
    assert not _plain_form(2 * nch, plan.n_fb, device) and _rows_blocks(2 * nch, plan.n_fb) < 64
    assert _plain_form(B * nch, plan.n_fb, device) and _rows_blocks(B * nch, plan.n_fb) >= 64
    big = np.random.default_rng(nch * nt).standard_normal((B, nch, nt)).astype(np.float32)
    fk_small = fk_grid(torch.as_tensor(big[:2], device=device), plan).cpu().numpy()
    fk_big = fk_grid(torch.as_tensor(big, device=device), plan)[:2].cpu().numpy()
    peak = np.abs(fk_big).max()
    d_forms = np.abs(fk_small - fk_big).max() / peak
    worst = 0.0
    for b in range(2):
        ref = _fft2_ref(big[b].astype(np.float64), plan)
        for got in (fk_small[b], fk_big[b]):
            worst = max(worst, np.abs(got - ref).max() / np.abs(ref).max())
    print(f"fk forms {nch} x {nt}: split vs plain {d_forms:.3g}, vs fft2 {worst:.3g} of the peak")
    assert d_forms <= 1e-12
    assert worst <= 1e-11


# ------------------------------------------------------------------------------------------ (d) |FK| at every geometry
FK_GEOMS = [(nch, nt, ds.DX) for nch, nt in sorted(ds.GEOMETRIES)] + [(ds.RAGGED["nch"], ds.RAGGED["nt"], ds.RAGGED["dx"])]


@pytest.mark.parametrize("nch,nt,dx", FK_GEOMS)
def test_fk_grid_every_geometry(device, nch, nt, dx):
    """|FK| of 3 noise gathers against the float64 fft2 slice, 1e-11 of the peak; with norm=True against the
    transform of the rows times float32(1 / ||row||_1) (dvh_disp_row_l1 stores the scale as float32) to 1e-11, and
    against data / ||row||_1 in float64 within that rounding: a scale off by 2^-24 of itself moves bin (m, q) by
    at most 2^-24 sum_x |D_x[q]|, D_x the time DFT of the normalised row x."""
    import torch

    from das_diff_veh_amd.disp import fk_grid
    plan = _plan(nch, nt, dx=dx)
    x = np.random.default_rng(nch + nt).standard_normal((3, nch, nt)).astype(np.float32)
    x64 = x.astype(np.float64)
    xd = torch.as_tensor(x, device=device)
    got = fk_grid(xd, plan).cpu().numpy()
    gotn = fk_grid(xd, plan, norm=True).cpu().numpy()
    assert got.shape == gotn.shape == (3, plan.n_kb, plan.n_fb)
    l1 = np.abs(x64).sum(axis=-1, keepdims=True)
    inv32 = (1.0 / l1).astype(np.float32).astype(np.float64)
    worst = worst_n = worst_e = 0.0
    for b in range(3):
        ref = _fft2_ref(x64[b], plan)
        worst = max(worst, np.abs(got[b] - ref).max() / ref.max())
        refn32 = _fft2_ref(x64[b] * inv32[b], plan)
        worst_n = max(worst_n, np.abs(gotn[b] - refn32).max() / refn32.max())
        xn = x64[b] / l1[b]
        refn = _fft2_ref(xn, plan)
        rows = np.abs(np.fft.fftshift(np.fft.fft(xn, n=plan.nf, axis=1), axes=1))[:, plan.j_lo:plan.j_lo + plan.n_fb]
        lim = 2.0 ** -24 * rows.sum(axis=0)[None, :] + 1e-11 * refn.max()
        worst_e = max(worst_e, float((np.abs(gotn[b] - refn) / lim).max()))
    print(f"fk_grid {nch} x {nt}: {worst:.3g} of the peak, norm {worst_n:.3g}, norm vs exact scale {worst_e:.3g} of its bound")
    assert worst <= 1e-11
    assert worst_n <= 1e-11
    assert worst_e <= 1.0


def test_row_l1_is_the_float32_inverse_norm(device):
    """dvh_disp_row_l1 on strided rows: float32(1 / sum_t |x_t|) of a float64 sum, within one float32 rounding."""
    import torch

    from das_diff_veh_amd import _lib
    worst = 0.0
    for B, nch, nt in [(1, 1, 1), (3, 17, 257), (2, 25, 2000), (5, 2, 255)]:
        x = np.random.default_rng(nt).standard_normal((B, nch, nt)).astype(np.float32)
        want = 1.0 / np.abs(x.astype(np.float64)).sum(axis=-1).ravel()
        for layout in ("contig", "stride5", "odd"):
            xv = _place(x, layout, device)
            buf = torch.full((B * nch + 2 * PAD,), CANARY, dtype=torch.float32, device=device)
            _lib.call("dvh_disp_row_l1", _lib.ptr(xv), xv.stride(0), xv.stride(1), B, nch, nt,
                      _lib.ptr(buf[PAD:PAD + B * nch]), _lib.stream_of(device))
            b = buf.cpu().numpy()
            assert (b[:PAD] == CANARY).all() and (b[PAD + B * nch:] == CANARY).all()
            err = np.abs(b[PAD:PAD + B * nch].astype(np.float64) - want) / want
            worst = max(worst, float(err.max()))
    print(f"row_l1: worst relative error {worst:.3g}")
    assert worst <= 2.0 ** -24 * (1 + 1e-6)


@pytest.mark.parametrize("nch", sorted(ds.FULL_GRID))
def test_public_fk_full_grid(device, nch):
    """fk() forms the whole nk x nf grid: 64 channels fit one block's LDS, 65 and 130 take the tiled contraction."""
    from das_diff_veh_amd.modules.utils import fk
    from oracle import disp as odisp
    x = np.random.default_rng(nch).standard_normal((nch, 16)).astype(np.float32)
    res, ff, kk = fk(x, ds.DX, ds.DT)
    ref, rf, rk = odisp.fk(x.astype(np.float64), ds.DX, ds.DT)
    assert res.shape == ref.shape == (ds.FULL_GRID[nch]["nk"], 32)
    err = np.abs(res - ref).max() / ref.max()
    print(f"fk() {nch} x 16: {err:.3g} of the peak")
    assert err <= 1e-11
    assert np.array_equal(ff, rf) and np.array_equal(kk, rk)


@pytest.mark.parametrize("nch,nt", [(17, 257), (25, 31), (33, 499), (128, 500)])
def test_tiled_contraction_equals_one_block_kernel(device, nch, nt):
    """contraction="tiled" sends a table that fits one block through fk_contract_tiled_kernel: each bin is summed over
    the channels in the same order, so |FK| is bitwise the one-block kernel's (plain and slot-accumulated, one gather
    per slot)."""
    import torch

    from das_diff_veh_amd.disp import fk_grid
    plan = _plan(nch, nt)
    xd = torch.as_tensor(np.random.default_rng(nt).standard_normal((3, nch, nt)).astype(np.float32), device=device)
    kw = dict(slots=[2, 0, 1], weights=[1.0, 0.5, 2.0], n_slot=3)
    assert ds.fk_lds_bytes(plan) <= ds.FK_LDS_LIMIT  # by size these tables take the one-block kernel
    one = fk_grid(xd, plan, contraction="one_block").cpu().numpy()
    one_s = fk_grid(xd, plan, contraction="one_block", **kw).cpu().numpy()
    til = fk_grid(xd, plan, contraction="tiled").cpu().numpy()
    til_s = fk_grid(xd, plan, contraction="tiled", **kw).cpu().numpy()
    assert np.array_equal(one, til)
    assert np.array_equal(one_s, til_s)


def test_fk_refusal_leaves_output_untouched(device):
    """A contraction table whose MT is no multiple of 16 is refused with a message and FK is not written."""
    import torch

    from das_diff_veh_amd import _lib
    nch, n_fb, MT, K2, n_kb = 5, 8, 24, 12, 20
    D = torch.zeros((nch, 2 * n_fb), dtype=torch.float64, device=device)
    atab = torch.zeros((2 * MT, K2), dtype=torch.float64, device=device)
    FK = torch.full((n_kb * n_fb + 2 * PAD,), CANARY, dtype=torch.float64, device=device)
    with pytest.raises(_lib.DvhError, match="invalid contraction table shape"):
        _lib.call("dvh_disp_fk", _lib.ptr(D), 1, nch, n_fb, _lib.ptr(atab), MT, K2, n_kb, _lib.ptr(FK[PAD:]), None,
                  None, 0, _lib.stream_of(device))
    torch.cuda.synchronize(device)
    assert bool((FK == CANARY).all())


# ------------------------------------------------------------------------------------------ (e) slot accumulation
def _oracle_fv_of_fk(res, fft_f, fft_k, freqs, vels):
    """oracle.disp.map_fv from its |FK| on: bilinear samples -> float32 -> savgol -> transpose."""
    import scipy.signal

    from oracle import disp as odisp
    fv = np.zeros((len(freqs), len(vels)), dtype=np.float32)
    ones = np.ones(len(vels))
    for i, fr in enumerate(freqs):
        fv[i, :] = odisp.bilinear(res, fft_f, fft_k, np.divide(ones * fr, vels), fr)
    return scipy.signal.savgol_filter(fv, 25, 4, axis=0).T


@pytest.mark.parametrize("nch,nt", [(25, 500), (129, 64)])
def test_slot_accumulation(device, nch, nt):
    """7 gathers into 4 slots (slot 1 empty, one weight 0) against the same call's per-gather |FK| combined on the
    host in float64, 1e-13 of the peak; the empty slot stays exactly 0; a slot outside [0, n_slot) is refused.
    129 channels take the tiled contraction."""
    from das_diff_veh_amd.disp import fk_grid
    from das_diff_veh_amd.synth import synth_gathers
    plan = _plan(nch, nt)
    data = synth_gathers(7, nch, nt, ds.DX, ds.DT, device, seed=5)
    slots = np.array([0, 2, 0, 3, 2, 0, 3])
    weights = np.array([0.5, 1.0, 0.25, 0.0, 2.0, 1.0, 0.75])  # exact in float32
    per = fk_grid(data, plan).cpu().numpy()
    got = fk_grid(data, plan, slots=slots, weights=weights, n_slot=4).cpu().numpy()
    want = np.zeros_like(got)
    for b in range(7):
        want[slots[b]] += weights[b] * per[b]
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"slot sums {nch} x {nt}: {err:.3g} of the peak")
    assert err <= 1e-13
    assert np.all(got[1] == 0.0)
    for bad in (4, -1):
        with pytest.raises(ValueError, match="one class slot"):
            fk_grid(data, plan, slots=[0, 2, 0, bad, 2, 0, 3], weights=weights, n_slot=4)


def test_fv_class_means_vs_oracle(device):
    """fv_class_means averages |FK| per class and samples once: against the oracle's sampling of the float64 mean
    |FK| of each class (the mean of the per-gather maps before the float32 cast).  An empty class gives zeros."""
    from das_diff_veh_amd.disp import fv_class_means
    from das_diff_veh_amd.synth import synth_gathers
    from oracle import disp as odisp
    nch, nt = 25, 500
    plan = _plan(nch, nt)
    freqs, vels = ds.axes()
    data = synth_gathers(7, nch, nt, ds.DX, ds.DT, device, seed=9)
    slots = np.array([0, 2, 0, 3, 2, 0, 3])
    got = fv_class_means(data, plan, slots, 4).double().cpu().numpy()
    host = data.double().cpu().numpy()
    fks = [odisp.fk(host[b], ds.DX, ds.DT) for b in range(7)]
    worst = 0.0
    for c in (0, 2, 3):
        mean = np.mean([fks[b][0] for b in range(7) if slots[b] == c], axis=0)
        ref = _oracle_fv_of_fk(mean, fks[0][1], fks[0][2], freqs, vels)
        err = np.abs(got[c] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err < TOL, c
        assert np.all(odisp.pick_ok(ref, got[c].argmax(axis=0))), c
    print(f"fv_class_means: worst rel-err {worst:.3g}")
    assert np.all(got[1] == 0.0)


# ------------------------------------------------------------------------------------------ (f) f-v maps by grid size
# forced kernels whose structural conditions fail at a geometry, and the kernel the choice ends at instead
FV_FALLS = {
    # 6 400 bins: above the 4 096 the batched kernel's threads prefetch
    (33, 499): {"batched": "per_image"},
    # 12 700 and 12 640 bins: 99 KB of |FK| against the tiled kernel's 64 KB of LDS, above the batched kernel's 4 096
    # bins and the MFMA kernel's 8 192; the cell-staged kernel holds only the cells a block reads and still runs
    (65, 500): {"tiled": "per_image", "batched": "per_image", "mfma": "per_image"},
    (25, 2000): {"tiled": "per_image", "batched": "per_image", "mfma": "per_image"},
}
_FV_REF = {}


def _fv_case(nch, nt, B, nV, nF, device, norm=False, zero_row=None):
    """(data, plan, oracle maps) of one geometry and (B, nV, nF): made once, shared by every mode, never changed."""
    from das_diff_veh_amd.synth import synth_gathers
    from oracle import disp as odisp
    key = (nch, nt, B, nV, nF, norm, zero_row)
    if key not in _FV_REF:
        freqs, vels = ds.axes(nF, nV)
        data = synth_gathers(B, nch, nt, ds.DX, ds.DT, device, seed=nch + B)
        if zero_row is not None:
            data[zero_row[0], zero_row[1]] = 0.0
        host = data.double().cpu().numpy()
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            refs = [odisp.map_fv(host[b], ds.DX, ds.DT, freqs, vels, norm=norm) for b in range(B)]
        _FV_REF[key] = (data, _plan(nch, nt, nF, nV), refs)
    return _FV_REF[key]


def _check_maps(got, refs):
    from oracle import disp as odisp
    worst = 0.0
    for b, ref in enumerate(refs):
        err = np.abs(got[b] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err < TOL, b
        assert np.all(odisp.pick_ok(ref, got[b].argmax(axis=0))), b
    return worst


@pytest.mark.parametrize("mode", ds.FV_MODES)
@pytest.mark.parametrize("B,nV,nF", [(3, 33, 47), (5, 70, 260)])
@pytest.mark.parametrize("nch,nt", [(1, 500), (17, 257), (33, 499), (65, 500), (25, 2000)])
def test_fv_maps_each_side_of_the_staging_limits(device, nch, nt, B, nV, nF, mode):
    """fv_maps against oracle.map_fv with |FK| grids of 200, 3 200, 6 400 (above the batched kernel's 4 096), 12 700
    and 12 640 bins (above every staged kernel's limit: the per-image kernel) under every kernel selection of
    tests/test_fv_batch_gpu.py; fv_choice names the forced kernel, or where it does not apply (FV_FALLS) the one it
    falls back to, which still matches."""
    from das_diff_veh_amd.disp import fv_maps
    data, plan, refs = _fv_case(nch, nt, B, nV, nF, device)
    name = ds.check_fv_choice(plan, B, mode, falls=FV_FALLS.get((nch, nt), ()))
    worst = _check_maps(fv_maps(data, plan, **ds.fv_mode_kwargs(mode)).double().cpu().numpy(), refs)
    print(f"fv_maps {nch} x {nt} ({B}, {nV}, {nF}) {mode} -> {name}: rel-err {worst:.3g}")


@pytest.mark.parametrize("nch,nt", ds.TILED)
def test_fv_maps_above_the_one_block_contraction(device, nch, nt):
    """129 and 300 channels: the tiled contraction, then the per-image sampling kernel (25 300 / 50 600 bins)."""
    from das_diff_veh_amd.disp import fv_maps
    data, plan, refs = _fv_case(nch, nt, 2, 33, 47, device)
    worst = _check_maps(fv_maps(data, plan).double().cpu().numpy(), refs)
    print(f"fv_maps {nch} x {nt}: rel-err {worst:.3g}")


@pytest.mark.parametrize("nch,nt", ds.TILED)
def test_public_map_fv_many_channels(device, nch, nt):
    """The public map_fv (one gather, norm=True as SurfaceWaveDispersion calls it) at 129 and 300 channels."""
    from das_diff_veh_amd.modules.utils import map_fv
    data, plan, refs = _fv_case(nch, nt, 1, 33, 47, device, norm=True)
    freqs, vels = ds.axes()
    got = map_fv(data[0].cpu().numpy(), ds.DX, ds.DT, freqs, vels, norm=True).astype(np.float64)
    worst = _check_maps(got[None], refs)
    print(f"map_fv norm {nch} x {nt}: rel-err {worst:.3g}")


# ------------------------------------------------------------------------------------------ (g) a zero row under norm
def test_zero_row_under_norm_is_nan_like_the_reference(device):
    """One all-zero channel in the middle gather of three, norm=True: 0 / 0 makes the reference's whole map NaN, and
    ours; the neighbouring gathers of the batch are not affected."""
    from das_diff_veh_amd.disp import fv_maps
    data, plan, refs = _fv_case(17, 257, 3, 33, 47, device, norm=True, zero_row=(1, 8))
    assert np.isnan(refs[1]).all()
    got = fv_maps(data, plan, norm=True).double().cpu().numpy()
    assert np.array_equal(np.isnan(got[1]), np.isnan(refs[1]))
    worst = _check_maps(got[[0, 2]], [refs[0], refs[2]])
    print(f"zero row: neighbours rel-err {worst:.3g}")
