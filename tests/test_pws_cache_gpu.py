"""The phase-weighted stack through GatherCache and the notebooks' entries: caches built as tests/test_boot_cache_gpu.py
builds them, from 8 synthetic passes of one lag length (w = 500: the float4 path of dvh_select_pws; w = 499: the scalar
one), and one more from four w = 500 and four w = 499 passes (W = 500, every 499-lag pass transformed over its own 499
lags).  The reference is tests/pws_ref.py (longdouble transform, float64 stack) on the cache's own float32 gathers, at
the bounds derived there."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from tests import pws_ref as ref

pytestmark = pytest.mark.gpu
N_PASS = 8
GEOM = (700.0, 500.0, 900.0)  # pivot, start_x, end_x
MODES = dict(sigma=[25, 50, 50, 50], ref_idx=[80, 130, 170, 170], lb=[2.5, 10, 14, 16], ub=[14, 15, 19, 20])
EXTRA_ROWS = (0, 47)  # gather rows outside the disp slice 6..24 that the analytic() test reads as well
SIZES = (1, 2, 4, 3, 8, 9, 17)


def _curves():
    import scipy.interpolate
    return [None,
            scipy.interpolate.interp1d([10, 12, 13, 14, 15, 16], [530, 470, 450, 430, 410, 391]),
            scipy.interpolate.interp1d([14, 15, 16, 17, 18, 19], [630, 583, 550, 520, 500, 490]),
            scipy.interpolate.interp1d([16, 17, 18, 19, 20, 21], [745, 690, 657, 626, 600, 580])]


def _args():
    m = MODES
    return m["sigma"], m["ref_idx"], m["lb"], m["ub"], _curves()


_CASES = {}


def _windows(device, t0, n, seed):
    from das_diff_veh_amd import synth
    wins, x_axis, t_axis, trk, _ = synth.synth_batch_device(n, seed=seed, device=device, t0=t0)
    return [SimpleNamespace(data=wins[i], x_axis=x_axis, t_axis=t_axis, veh_state_x=trk[i][0], veh_state_t=trk[i][1])
            for i in range(n)]


def _case(device, name):
    """(windows, cache, the cache's gathers on the host, reference H over rows 6..24 and EXTRA_ROWS as {row: [n, W]})
    of one cache, built once."""
    if name not in _CASES:
        from das_diff_veh_amd import bootstrap as bt
        from das_diff_veh_amd import synth
        if name == "mixed":
            a, b = _windows(device, synth.DT_W500, 4, 3), _windows(device, synth.DT_W499, 4, 4)
            wins = [a[0], b[0], a[1], a[2], b[1], b[2], a[3], b[3]]
        else:
            wins = _windows(device, {"w500": synth.DT_W500, "w499": synth.DT_W499}[name], N_PASS, 3)
        cache = bt.GatherCache(wins, *GEOM, device=device)
        G = cache.G.cpu().numpy()
        s, e, _ = cache.disp_plan()
        assert (s, e, cache.plan.R) == (6, 24, 48)
        rows = sorted(set(range(s, e + 1)) | set(EXTRA_ROWS))
        Href = ref.analytic(G[:, rows], cache.w_of)
        Href.setflags(write=False)
        _CASES[name] = (wins, cache, G, dict(zip(rows, Href.transpose(1, 0, 2))))
    return _CASES[name]


@pytest.mark.parametrize("name", ["w500", "w499", "mixed"])
def test_analytic(device, name):
    """analytic() is computed once; every pass is transformed over its own w_of lags and is 0 beyond; the rows the
    reference covers are inside pws_ref.hilbert_bound."""
    _, cache, G, Href = _case(device, name)
    H_t = cache.analytic()
    assert cache.analytic() is H_t and tuple(H_t.shape) == tuple(cache.G.shape)
    H = H_t.cpu().numpy()
    if name == "mixed":
        assert cache.W == 500 and sorted(set(cache.w_of.tolist())) == [499, 500]
    worst = 0.0
    for j, w in enumerate(cache.w_of):
        assert np.all(H[j, :, w:] == 0)
        for r, want in Href.items():
            bound = ref.hilbert_bound(want[j, :w], int(w), np.abs(G[j, r, :w]).max())
            err = np.abs(H[j, r, :w] - want[j, :w])
            assert np.all(err <= bound), (j, r)
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    assert np.all(np.isfinite(H)) and float(np.abs(H).max()) > 0
    print(f"analytic ({name}): worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", ["w500", "w499", "mixed"])
def test_resample_stacks_pws(device, name):
    """resample_stacks(stack="pws") and resample_stacks_sizes agree bit for bit and stay inside pws_ref.pws_bound, at
    powers 2 and 1 and at sizes on both sides of the load group; power 0 is the linear call bit for bit."""
    import torch
    _, cache, G, Href = _case(device, name)
    s, e, _ = cache.disp_plan()
    rng = np.random.default_rng(5)
    sels = [rng.integers(0, N_PASS, size=(3, k)).astype(np.int32) for k in SIZES]
    Gd = G[:, s:e + 1]
    Hd = np.stack([Href[r] for r in range(s, e + 1)], axis=1)
    stats = [ref.parts(Gd, Hd, row) for x in sels for row in x]
    worst = 0.0
    for power in (2.0, 1.0):
        got_t = cache.resample_stacks_sizes(sels, stack="pws", power=power)
        per_size = torch.cat([cache.resample_stacks(x, stack="pws", power=power) for x in sels])
        assert torch.equal(got_t, per_size)
        got = got_t.cpu().numpy()
        for b, (lin, c, mabs) in enumerate(stats):
            m = SIZES[b // 3]
            err = np.abs(got[b] - ref.weighted(lin, c, power))
            bound = ref.pws_bound(m, power, mabs)
            ok = bound > 0
            worst = max(worst, float((err[ok] / bound[ok]).max(initial=0.0)))
            assert np.all(err <= bound), (power, b, m)
    assert torch.equal(cache.resample_stacks_sizes(sels, stack="pws", power=0), cache.resample_stacks_sizes(sels))
    assert torch.equal(cache.resample_stacks(sels[4], stack="pws", power=0), cache.resample_stacks(sels[4]))
    print(f"resample_stacks pws ({name}): worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", ["w500", "mixed"])
def test_bootstrap_ridges_pws(device, name):
    """power 0 gives the linear call's ridges bit for bit, for both transforms and both slant walks; with power 2 the
    ridges are finite and the fused slant walk equals the walk on the slant images, as for the linear stack."""
    from das_diff_veh_amd import bootstrap as bt
    _, cache, _, _ = _case(device, name)
    sels = np.array([[1, 3, 4], [2, 2, 1], [4, 1, 2], [7, 6, 5]], dtype=np.int32)
    walks = (("fk", None), ("slant", "image"), ("slant", "fused"))
    pws2 = {}
    for transform, walk in walks:
        lin = bt.bootstrap_ridges(cache, sels, *_args(), transform=transform, walk=walk)
        p0 = bt.bootstrap_ridges(cache, sels, *_args(), transform=transform, walk=walk, stack="pws", power=0)
        pws2[walk] = bt.bootstrap_ridges(cache, sels, *_args(), transform=transform, walk=walk, stack="pws", power=2)
        for m in range(4):
            assert np.array_equal(np.asarray(lin[m]), np.asarray(p0[m])), (transform, walk, m)
            assert np.asarray(pws2[walk][m]).shape == np.asarray(lin[m]).shape
            assert np.all(np.isfinite(pws2[walk][m])), (transform, walk, m)
    for m in range(4):
        assert np.array_equal(np.asarray(pws2["fused"][m]), np.asarray(pws2["image"][m])), m


def test_convergence_pws(device):
    """convergence(stack="pws") with sizes 1..3 x 4 draws: each entry the summed std of bootstrap_ridges on the same
    draws with the same stack (1e-9); power 0 equals the linear curves."""
    from das_diff_veh_amd import bootstrap as bt
    _, cache, _, _ = _case(device, "w500")
    got = bt.convergence(cache, 3, 4, *_args(), rand=random.Random(7), stack="pws", power=2)
    assert got.shape == (4, 3) and np.all(np.isfinite(got))
    sels = bt.draw_sizes(cache.n, range(1, 4), 4, random.Random(7))
    for k, sel in enumerate(sels):
        rv = bt.bootstrap_ridges(cache, sel, *_args(), stack="pws", power=2)
        for mode in range(4):
            assert abs(float(np.std(np.asarray(rv[mode]), axis=0).sum()) - got[mode, k]) <= 1e-9, (mode, k)
    lin = bt.convergence(cache, 3, 4, *_args(), rand=random.Random(7))
    assert np.array_equal(bt.convergence(cache, 3, 4, *_args(), rand=random.Random(7), stack="pws", power=0), lin)


@pytest.mark.parametrize("name", ["w500", "mixed"])
def test_phase_weighted_gather(device, name):
    """phase_weighted_gather is the stack of all windows in order over all gather rows, on the first window's axes;
    compute_disp_image runs on it with either transform."""
    from das_diff_veh_amd.apis.imaging_classes import phase_weighted_gather
    wins, cache, _, _ = _case(device, name)
    vsg = phase_weighted_gather(wins, *GEOM, power=2.0)
    want = cache.resample_stacks([list(range(cache.n))], cache.gx[0], cache.gx[-1], stack="pws", power=2.0)
    w = int(cache.w_of[0])
    assert tuple(want.shape) == (1, cache.plan.R, cache.W)
    assert vsg.XCF_out.dtype == np.float64 and vsg.XCF_out.shape == (cache.plan.R, w)
    assert np.array_equal(vsg.XCF_out, want[0, :, :w].cpu().numpy().astype(np.float64))
    assert np.array_equal(vsg.x_axis, cache.gx) and np.array_equal(vsg.t_axis, cache.gt) and vsg.window is wins[0]
    assert np.all(np.isfinite(vsg.XCF_out)) and float(np.abs(vsg.XCF_out).max()) > 0
    for transform in ("fk", "slant"):
        vsg.compute_disp_image(end_x=0, start_x=-150, transform=transform)
        fv = np.asarray(vsg.disp.fv_map)
        assert fv.ndim == 2 and fv.size > 0 and np.all(np.isfinite(fv)) and float(fv.max()) > 0
