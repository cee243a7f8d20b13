"""Bootstrap and convergence on the phase-shift transform (transform="slant"): the resample images against
Dispersion(transform="slant"), tests/slant_ref and the float64 oracle chain; the fused walk (dvh_slant_ridge, which
computes the values it compares) against the walk on the stored image (dvh_ridge), which it must equal exactly; the
notebooks' bootstrap_disp / convergence_test with the keyword; mixed lag lengths; the C ABI's refusals."""
import functools
import random

import numpy as np
import pytest
import scipy.interpolate

from tests import boot_slant_ref as bsr
from tests import golden_io as gio
from tests import slant_ref

pytestmark = pytest.mark.gpu
KW = dict(pivot=700, start_x=500, end_x=900)
ARGS = [25, 50], 700, 500, 900, [80, 130], [2.5, 10], [14, 15]
SELS = np.array([[1, 3, 4], [2, 2, 1], [4, 1, 2]], dtype=np.int32)
INT32_MIN = -2 ** 31


def _mode1():
    g = gio.load("ridge")
    return scipy.interpolate.interp1d(g["refvel_f"], g["refvel_v"])


@functools.lru_cache(maxsize=None)
def _windows():
    from das_diff_veh_amd.apis.data_classes import SurfaceWaveWindow
    g = gio.load("vsg_w500")
    return [SurfaceWaveWindow(**gio.pass_arrays(g, i)) for i in range(gio.n_pass(g))], g


@functools.lru_cache(maxsize=None)
def _cache():
    from das_diff_veh_amd import bootstrap as bt
    return bt.GatherCache(_windows()[0], **KW)


def _end_to_end(sels):
    """The device's slant images of the draws against the float64 oracle chain: (device images, oracle images,
    largest discrepancy), each resample asserted under the derived bound (tests/boot_slant_ref.end_to_end_bound)."""
    from das_diff_veh_amd import bootstrap as bt
    cache, g = _cache(), _windows()[1]
    s, e, plan = cache.slant_plan()
    dt = float(cache.gt[1] - cache.gt[0])
    fv = cache.resample_images(sels, transform="slant").cpu().numpy()
    refs, worst = [], 0.0
    for b, sel in enumerate(sels):
        stack, ref = bsr.oracle_image([g["xcf"][i] for i in sel], s, e, dt, bt.FREQS, bt.VELS)
        assert stack.shape == (plan.n_row, 500)
        err, bound = float(np.abs(fv[b] - ref).max()), bsr.end_to_end_bound(stack)
        print(f"resample {b}: |device - float64 chain| = {err:.3e} (bound {bound:.3e}, image maximum {ref.max():.3e})")
        assert err <= bound
        refs.append(ref)
        worst = max(worst, err)
    return fv, refs, worst


def test_resample_images(device):
    """resample_images(transform="slant") of the draws: bit for bit the image Dispersion(transform="slant") gives for
    each resample's float32 stack alone (batch independence), within 1e-6 of the image maximum of slant_ref on that
    stack (the bound of INTEGRATION.md 2i), and end to end within the derived bound of the float64 oracle chain."""
    from das_diff_veh_amd import bootstrap as bt
    from das_diff_veh_amd.modules.utils import Dispersion
    cache = _cache()
    s, e, plan = cache.slant_plan()
    assert e + 1 - s == 19 and (plan.row0, plan.n_row) == (0, 19) and plan.dx == 8.16
    assert np.array_equal(plan.vels, np.sort(bt.VELS)[::-1]) and plan.n_fb < plan.nF
    assert cache.slant_plan()[2] is plan and bt.GatherCache(_windows()[0], **KW).slant_plan()[2] is plan  # cached
    dt = cache.gt[1] - cache.gt[0]
    stacks = cache.resample_stacks(SELS).cpu().numpy()
    fv, _, _ = _end_to_end(SELS)
    assert fv.dtype == np.float32 and fv.shape == (3, 1000, 242)
    for b in range(3):
        alone = Dispersion(stacks[b], 8.16, dt, bt.FREQS, bt.VELS, norm=False, transform="slant").fv_map
        assert np.array_equal(fv[b], alone), b
        ref = slant_ref.slant(stacks[b], 8.16, dt, bt.FREQS, np.sort(bt.VELS)[::-1], norm=False, rows=(0, 19))
        err = np.abs(fv[b] - ref).max() / ref.max()
        print(f"resample {b}: {err:.3e} of the image maximum against slant_ref on the same float32 stack")
        assert err <= 1e-6
    with pytest.raises(ValueError):
        cache.resample_images(SELS, transform="bogus")
    assert np.array_equal(cache.resample_images(SELS, transform="fk").cpu().numpy(),
                          cache.resample_images(SELS).cpu().numpy())


def _band(i0, n):
    """(lb, ub) selecting columns [i0, i0 + n) of FREQS."""
    from das_diff_veh_amd.bootstrap import FREQS
    lb, ub = FREQS[i0] - 0.05, FREQS[i0 + n] - 0.05
    assert int(np.sum((FREQS >= lb) & (FREQS < ub))) == n
    return lb, ub


def _modes(vels):
    """(lb, ub, ref, sigma, ref_vel) of every walk of the comparison: bands of 116, 26 and 25 (the smoothing length)
    columns; references 0, inside and nb - 1; the negative references of tests/test_boot_gpu.py; a reference curve
    inside the axis; ref_freq_idx=None; sigma 25, 50 and 0.5 (one velocity per window on a 1 m/s axis)."""
    lo, hi = float(vels[0]), float(vels[-1])
    curve = lambda f: lo + (hi - lo) * (0.5 + 0.4 * np.sin(f))  # noqa: E731
    wide, mid, short = _band(17, 116), _band(17, 26), _band(92, 25)
    return [(*wide, 63, 25, None), (*wide, 0, 50, None), (*wide, 115, 25, None), (*wide, -7, 25, None),
            (*wide, -1, 50, None), (*wide, -116, 25, None), (*wide, -3, 25, None), (*mid, 13, 50, None),
            (*mid, -3, 25, None), (*mid, 25, 25, None), (*short, 12, 25, None), (*short, 0, 50, None),
            (*short, 24, 25, None), (*short, -25, 25, None), (*_band(92, 50), 38, 50, curve), (*mid, 0, 25, curve),
            (*wide, None, 25, None), (*wide, 63, 0.5, None), (*short, 12, 0.5, None)]


@pytest.mark.parametrize("nV", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("n_row", [1, 19, 24, 25])
def test_fused_walk_equals_image_walk(device, n_row, nV):
    """plan_ridges (dvh_slant_ridge on the spectra) against ridges (dvh_ridge) on slant_maps of the same random
    stacks: outputs, raw picks and status are equal, not close.  n_row on both sides of dvh_slant.hip's register /
    running-power cut-over (24 | 25); nV around the 64-lane rounds and the notebooks' 1 000."""
    import torch

    from das_diff_veh_amd import bootstrap as bt
    from das_diff_veh_amd.disp import SlantPlan, slant_maps
    vels = np.arange(200.0, 200.0 + nV)
    plan = SlantPlan(n_row, 500, 8.16, 0.004, bt.FREQS, vels[::-1], rows=(0, n_row))
    assert plan.n_fb < plan.nF  # neighbouring frequencies share DFT bins: shared fb entries are covered
    rng = np.random.default_rng(1000 * n_row + nV)
    stacks = torch.from_numpy(rng.standard_normal((3, n_row, 500)).astype(np.float32)).to(device)
    fv = slant_maps(stacks, plan, norm=False)
    modes = _modes(vels)
    lb, ub, ref, sg, rv = (list(x) for x in zip(*modes))
    fused = bt.plan_ridges_launch(stacks, plan, lb, ub, ref, sg, 800, rv, return_picks=True)
    assert len(fused) == len(modes)
    for m, (got, md) in enumerate(zip(fused, modes)):
        want = bt.ridges_launch(fv, bt.FREQS, vels, md[0], md[1], ref_freq_idx=md[2], sigma=md[3], vel_max=800,
                                ref_vel=md[4], return_picks=True)
        for name, a, b in zip(("out", "status", "picks"), got, want):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), (m, md[:4], name)
        assert not got[1].any()
    if n_row == 19 and nV == 1000:  # the host-returning forms, and without the picks
        a = bt.plan_ridges(stacks, plan, lb[:2], ub[:2], ref[:2], sg[:2], 800, rv[:2])
        for m in range(2):
            assert np.array_equal(a[m], fused[m][0].cpu().numpy())


def test_reference_curve_outside_the_axis_raises(device):
    """A ref_vel curve above every velocity: each window is empty, the status is set in both kernels and both paths
    raise the reference's ValueError."""
    import torch

    from das_diff_veh_amd import bootstrap as bt
    from das_diff_veh_amd.disp import SlantPlan, slant_maps
    vels = np.arange(200.0, 1200.0)
    plan = SlantPlan(19, 500, 8.16, 0.004, bt.FREQS, vels[::-1], rows=(0, 19))
    stacks = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 19, 500)).astype(np.float32)).to(device)
    lb, ub = _band(17, 26)
    away = lambda f: np.full(np.shape(f), 5000.0)  # noqa: E731
    st = bt.plan_ridges_launch(stacks, plan, [lb], [ub], [0], [25], 800, [away])[0][1]
    assert st.cpu().tolist() == [1, 1, 1]
    with pytest.raises(ValueError) as fused:
        bt.plan_ridges(stacks, plan, [lb], [ub], [0], [25], 800, [away])
    with pytest.raises(ValueError) as image:
        bt.ridges(slant_maps(stacks, plan, norm=False), bt.FREQS, vels, lb, ub, ref_freq_idx=0, sigma=25, vel_max=800,
                  ref_vel=away)
    assert str(fused.value) == str(image.value)


def test_bootstrap_disp_slant(device):
    """bootstrap_disp(..., transform="slant") on the reference's draws: fused and image walks equal; the ridges are
    the oracle's extract_ridge_ref_idx on the device's own images (1e-9); every walk step is audited against the
    float64 oracle chain's image: the pick is inside the device's own window and the reference image there is within
    twice the measured image discrepancy of the reference maximum over that window.  Equal picks are not asserted:
    the float64 image itself has a runner-up within 2e-6 of the maximum at 92 of these 664 steps."""
    from das_diff_veh_amd import bootstrap as bt
    from das_diff_veh_amd.apis.imaging_classes import bootstrap_disp
    from oracle import ridge as orid
    wins, _ = _windows()
    g = gio.load("ridge")
    mode1 = _mode1()
    res = {}
    for walk in ("fused", "image", None):
        random.seed(11)
        res[walk], fq = bootstrap_disp(wins, 3, 4, *ARGS, [None, mode1], transform="slant", walk=walk)
        np.testing.assert_array_equal(fq, g["boot_freqs"])
    random.seed(11)
    sels = bt.draw(len(wins), 3, 4)
    np.testing.assert_array_equal(sels, g["boot_sel"])
    for m in range(2):
        assert np.array_equal(np.stack(res["fused"][m]), np.stack(res["image"][m])), m
        assert np.array_equal(np.stack(res[None][m]), np.stack(res["image"][m])), m
    rv = res["fused"]
    fv, ref_fv, fv_err = _end_to_end(sels)
    cache = _cache()
    stacks = cache.resample_stacks(sels)
    steps = other = 0
    worst = 0.0
    modes = ((2.5, 14, 80, 25, None), (10, 15, 130, 50, mode1))
    refs = [ri - int(np.sum(fq < lb)) for lb, _, ri, _, _ in modes]
    picks = bt.slant_ridges(cache, stacks, sels[:, 0], [md[0] for md in modes], [md[1] for md in modes], refs,
                            [md[3] for md in modes], 800, [md[4] for md in modes], return_picks=True)
    for m, (lb, ub, _, sg, vr) in enumerate(modes):
        band = (fq >= lb) & (fq < ub)
        assert np.array_equal(picks[m][0], np.stack(rv[m]))
        for b in range(4):
            o = orid.extract_ridge_ref_idx(fq[band], bt.VELS, fv[b][:, band].astype(np.float64),
                                           ref_freq_idx=refs[m], sigma=sg, vel_max=800, ref_vel=vr)
            np.testing.assert_allclose(rv[m][b], o, rtol=0, atol=1e-9)
            n, k, w = bsr.audit_walk(picks[m][1][b], ref_fv[b][:, band], bt.VELS, sg, 2 * fv_err,
                                     ref_idx=None if vr is not None else refs[m],
                                     vref=vr(fq[band]) if vr is not None else None)
            steps, other, worst = steps + n, other + k, max(worst, w)
    print(f"bootstrap_disp slant: {steps} walk steps audited, {other} picks off the float64 argmax, largest shortfall "
          f"{worst:.3e} against 2 x {fv_err:.3e}")
    assert steps == 4 * (116 + 50)


def test_convergence_test_slant(device):
    """convergence_test(3, wins, 4, ..., transform="slant"): [n_modes, 3]; each entry the summed standard deviation
    of the ridges of the same draws from bootstrap_ridges(transform="slant") (1e-9); fused and image walks equal."""
    from das_diff_veh_amd import bootstrap as bt
    from das_diff_veh_amd.apis.imaging_classes import convergence_test
    wins, _ = _windows()
    mode1 = _mode1()
    got = {}
    for walk in ("fused", "image"):
        random.seed(5)
        got[walk] = convergence_test(3, wins, 4, *ARGS, [None, mode1], transform="slant", walk=walk)
        assert got[walk].shape == (2, 3) and np.all(np.isfinite(got[walk]))
    assert np.array_equal(got["fused"], got["image"])
    random.seed(5)
    for k in range(1, 4):
        sels = bt.draw(len(wins), k, 4)
        for walk in ("fused", "image"):
            r = bt.bootstrap_ridges(_cache(), sels, ARGS[0], *ARGS[4:], [None, mode1], transform="slant", walk=walk)
            for m in range(2):
                assert abs(np.sum(np.std(r[m], axis=0)) - got[walk][m, k - 1]) <= 1e-9, (walk, m, k)


def _mixed_windows():
    """Passes of the w = 500 and w = 499 fixtures interleaved, as real records mix both lag lengths."""
    from das_diff_veh_amd.apis.data_classes import SurfaceWaveWindow
    g5, g9 = gio.load("vsg_w500"), gio.load("vsg_w499")
    srcs = [(g5, 0), (g9, 0), (g5, 1), (g5, 2), (g9, 1), (g5, 3), (g5, 4)]
    return [SurfaceWaveWindow(**gio.pass_arrays(g, i)) for g, i in srcs]


def test_mixed_lag_lengths(device):
    """A cache over windows of w = 500 and 499: a draw's image is Dispersion(transform="slant") of its stack cut to
    its first pass's lag length, with that pass's time step, bit for bit, for draws led by either length; the fused
    walk equals the walk on those images."""
    from das_diff_veh_amd import bootstrap as bt
    from das_diff_veh_amd.modules.utils import Dispersion
    cache = bt.GatherCache(_mixed_windows(), **KW)
    sels = np.array([[1, 2, 3], [2, 1, 4], [4, 6, 1], [3, 5, 2], [6, 1, 1]], dtype=np.int32)
    lead = cache.w_of[sels[:, 0]]
    assert set(lead.tolist()) == {499, 500} and cache.W == 500
    stacks = cache.resample_stacks(sels).cpu().numpy()
    fv = cache.resample_images(sels, transform="slant").cpu().numpy()
    for b, w in enumerate(lead):
        gt = cache._gt_of[int(w)]
        alone = Dispersion(stacks[b][:, :w], 8.16, gt[1] - gt[0], bt.FREQS, bt.VELS, norm=False, transform="slant")
        assert np.array_equal(fv[b], alone.fv_map), (b, w)
    mode1 = _mode1()
    r = {walk: bt.bootstrap_ridges(cache, sels, ARGS[0], *ARGS[4:], [None, mode1], transform="slant", walk=walk)
         for walk in ("fused", "image")}
    for m in range(2):
        assert r["fused"][m].shape == (5, (116, 50)[m])
        assert np.array_equal(r["fused"][m], r["image"][m]), m


def test_slant_ridge_c_abi(device):
    """dvh_slant_ridge through ctypes: -2 for null pointers, negative counts, a band past nF and a ref outside the
    band; -4 for an even sgl and for a band of more than 1 024 columns; 0 for B == 0; nothing is written by a refused
    call."""
    import torch

    from das_diff_veh_amd import _lib
    from das_diff_veh_amd.bootstrap import _sg_ridge
    lib = _lib.load()
    n_row, n_fb, nF, nV, B = 3, 4, 1100, 8, 2
    D = torch.zeros((B * n_row, 2 * n_fb), dtype=torch.float64, device=device)
    fb = torch.zeros(nF, dtype=torch.int32, device=device)
    freqs = torch.linspace(1, 20, nF, dtype=torch.float64, device=device)
    vel = torch.arange(300, 300 - nV, -1, dtype=torch.float64, device=device)
    sg = torch.from_numpy(np.asarray(_sg_ridge(), dtype=np.float64)).to(device)
    vref = torch.full((1025,), 298.0, dtype=torch.float64, device=device)
    out = torch.full((B, 1025), -77.25, dtype=torch.float64, device=device)
    picks = out.clone()
    status = torch.full((B,), -7, dtype=torch.int32, device=device)
    a = dict(D=_lib.ptr(D), B=B, n_row=n_row, n_fb=n_fb, fb=_lib.ptr(fb), freqs=_lib.ptr(freqs), nF=nF, dx=8.16, c0=3,
             nb=26, vel=_lib.ptr(vel), nV=nV, ref=5, sigma=25.0, vel_max=800.0, vref=None, sg=_lib.ptr(sg), sgl=25,
             out=_lib.ptr(out), status=_lib.ptr(status), picks=_lib.ptr(picks), stream=_lib.stream_of(device))
    cases = [(dict(D=None), -2), (dict(fb=None), -2), (dict(freqs=None), -2), (dict(vel=None), -2),
             (dict(out=None), -2), (dict(status=None), -2), (dict(B=-1), -2), (dict(n_row=-1), -2), (dict(nF=-1), -2),
             (dict(nV=-1), -2), (dict(nb=-1), -2), (dict(c0=nF - 25), -2), (dict(ref=26), -2), (dict(ref=-27), -2),
             (dict(sgl=24), -4), (dict(sgl=27), -4), (dict(nb=1025, c0=0), -4)]
    for over, want in cases:
        for curve in (None, _lib.ptr(vref)):
            assert lib.dvh_slant_ridge(*{**a, "vref": curve, **over}.values()) == want, (over, curve is not None)
            assert lib.dvh_last_error()
    assert lib.dvh_slant_ridge(*{**a, "B": 0}.values()) == 0
    torch.cuda.synchronize(device)
    assert bool((out == -77.25).all()) and bool((picks == -77.25).all()) and bool((status == -7).all())
    # and the accepted call writes exactly its rows: zero spectra give a zero image, the first row wins every window
    assert lib.dvh_slant_ridge(*a.values()) == 0
    torch.cuda.synchronize(device)
    assert status.cpu().tolist() == [0, 0]
    assert bool((picks.reshape(-1)[:B * 26] == 300.0).all()) and bool((picks.reshape(-1)[B * 26:] == -77.25).all())
    assert bool(((out.reshape(-1)[:B * 26] - 300.0).abs() <= 1e-9).all())
    assert bool((out.reshape(-1)[B * 26:] == -77.25).all())
