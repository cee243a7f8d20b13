"""The device-built gather cache (GatherCache.from_device: a DevicePlan from packed trajectories, gx / gt recomputed
from the shared axes -- the constructor bench.py times) against the host-planned one (GatherCache: pass_geometry per
window), and a bootstrap over passes of ONE lag length, at both: t0 = synth.DT_W500 gives w = 500 (K = 19 x 500: the
float4 path of dvh_select_mean) and t0 = synth.DT_W499 gives w = 499 (K = 9 481, base offset 6 x 499 floats: the
scalar path, which a cache padded to W = 500 never takes).

The index tables of the two plans are bit-equal (tests/test_plan_gpu.py) and dvh_vsg_scales / dvh_vsg_gathers receive
nothing of a plan but its tables and (R, w, hop, flags) (vsg.vsg_gathers), so the gathers are asserted torch.equal.
Resample stacks equal the NumPy float32 sum in draw order divided by the size, bit for bit; resample images are held
to the oracle (float64 VSG of the host copies of the windows, stack, compute_disp_image) at the bounds of
tests/test_boot_gpu.py; convergence() is equal between the caches and equals the summed std of bootstrap_ridges on
the same draws to 1e-9."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N_PASS = 8
GEOM = (700.0, 500.0, 900.0)  # pivot, start_x, end_x
MODES = dict(sigma=[25, 50, 50, 50], ref_idx=[80, 130, 170, 170], lb=[2.5, 10, 14, 16], ub=[14, 15, 19, 20])


def _curves():
    import scipy.interpolate
    return [None,
            scipy.interpolate.interp1d([10, 12, 13, 14, 15, 16], [530, 470, 450, 430, 410, 391]),
            scipy.interpolate.interp1d([14, 15, 16, 17, 18, 19], [630, 583, 550, 520, 500, 490]),
            scipy.interpolate.interp1d([16, 17, 18, 19, 20, 21], [745, 690, 657, 626, 600, 580])]


_CASES = {}


def _case(device, clock):
    """(source, host-planned cache, device-planned cache) of one clock, built once."""
    if clock not in _CASES:
        from das_diff_veh_amd import bootstrap as bt
        from das_diff_veh_amd import synth
        from das_diff_veh_amd.plan import pack_trajectories
        t0 = {"w500": synth.DT_W500, "w499": synth.DT_W499}[clock]
        wins, x_axis, t_axis, trk, _ = synth.synth_batch_device(N_PASS, seed=3, device=device, t0=t0)
        host = bt.GatherCache([SimpleNamespace(data=wins[i], x_axis=x_axis, t_axis=t_axis, veh_state_x=trk[i][0],
                                               veh_state_t=trk[i][1]) for i in range(N_PASS)], *GEOM, device=device)
        dev = bt.GatherCache.from_device(wins, x_axis, t_axis, *pack_trajectories(trk, device), *GEOM)
        _CASES[clock] = (SimpleNamespace(wins=wins, x_axis=x_axis, t_axis=t_axis, trk=trk), host, dev)
    return _CASES[clock]


def _select_vec(g_ptr, pass_stride, K, out_ptr, out_stride):
    """select_vec of csrc/dvh_boot.hip."""
    return K % 4 == 0 and pass_stride % 4 == 0 and out_stride % 4 == 0 and (g_ptr | out_ptr) % 16 == 0


def _stack_reference(G, sel):
    acc = np.zeros(G.shape[1:], np.float32)
    for j in sel:
        acc += G[j]
    return acc / np.float32(len(sel))


@pytest.mark.parametrize("clock", ["w500", "w499"])
def test_device_planned_cache_equals_host_planned(device, clock):
    import torch
    _, host, dev = _case(device, clock)
    w = 500 if clock == "w500" else 499
    assert (host.n, host.W, host.plan.R, host.plan.w) == (dev.n, dev.W, dev.plan.R, dev.plan.w) == (N_PASS, w, 48, w)
    assert np.array_equal(host.w_of, dev.w_of) and host.w_of.dtype == dev.w_of.dtype
    for a, b in ((host.gx, dev.gx), (host.gt, dev.gt)):
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    (hs, he, hp), (ds, de, dp) = host.disp_plan(), dev.disp_plan()
    assert (hs, he) == (ds, de) == (6, 24)
    assert (hp.nch, hp.nt, hp.dx, hp.dt) == (dp.nch, dp.nt, dp.dx, dp.dt)
    assert torch.equal(host.G, dev.G)
    assert torch.isfinite(dev.G).all() and float(dev.G.abs().max()) > 0


@pytest.mark.parametrize("clock", ["w500", "w499"])
def test_resample_stacks_on_each_select_path(device, clock):
    """w = 499 alone runs the scalar path, w = 500 the float4 path (the predicate restated on the pointers the call
    receives); sizes on both sides of the 8-load group; bit equal to the NumPy float32 reference, on both caches."""
    import torch
    _, host, dev = _case(device, clock)
    rng = np.random.default_rng(5)
    sels = [rng.integers(0, N_PASS, size=(3, k)).astype(np.int32) for k in (1, 2, 4, 3, 8, 9, 17)]
    for cache in (host, dev):
        s, e, _ = cache.disp_plan()
        w, R = cache.W, cache.plan.R
        K = (e + 1 - s) * w
        out = torch.empty((sum(len(x) for x in sels), e + 1 - s, w), dtype=torch.float32, device=device)
        assert cache.G.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        vec = _select_vec(cache.G[:, s:e + 1, :].data_ptr(), R * w, K, out.data_ptr(), K)
        if clock == "w499":
            assert K == 9481 and (cache.G[:, s:e + 1, :].data_ptr() - cache.G.data_ptr()) // 4 % 4 == 2 and not vec
        else:
            assert K == 9500 and vec
        G = cache.G[:, s:e + 1, :].cpu().numpy()
        ref = np.stack([_stack_reference(G, row) for x in sels for row in x])
        got = cache.resample_stacks_sizes(sels, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(got.cpu().numpy(), ref)
        per_size = torch.cat([cache.resample_stacks(x) for x in sels])
        assert np.array_equal(per_size.cpu().numpy(), ref)


@pytest.mark.parametrize("clock", ["w500", "w499"])
def test_resample_images_against_the_oracle(device, clock):
    """Draws of sizes 1, 3 and 3 from the device-planned cache: f-v images within 1e-4 of the oracle image's maximum,
    every column's pick on the oracle's maximum."""
    from oracle import disp as odisp
    from oracle import vsg as ovsg
    src, _, dev = _case(device, clock)
    draws = [np.array([[1]], np.int32), np.array([[2, 3, 1], [3, 1, 1]], np.int32)]
    data = src.wins.cpu().numpy().astype(np.float64)
    og = {i: ovsg.virtual_shot_gather(dict(data=data[i], x_axis=src.x_axis, t_axis=src.t_axis,
                                           veh_state_x=src.trk[i][0], veh_state_t=src.trk[i][1]),
                                      include_other_side=True, norm=False, pivot=GEOM[0], start_x=GEOM[1],
                                      end_x=GEOM[2], wlen=2) for i in (1, 2, 3)}
    assert og[1][0].shape == (dev.plan.R, dev.plan.w)
    worst = 0.0
    for sels in draws:
        fv = dev.resample_images(sels).cpu().numpy()
        for b, sel in enumerate(sels):
            rfv = odisp.compute_disp_image(ovsg.stack([og[i][0] for i in sel]), og[sel[0]][1], og[sel[0]][2],
                                           start_x=-150, end_x=0)
            err = float(np.abs(fv[b] - rfv).max() / np.abs(rfv).max())
            worst = max(worst, err)
            assert err <= 1e-4, (sel, err)
            ok = odisp.pick_ok(rfv, fv[b].argmax(axis=0))
            assert np.all(ok), f"{(~ok).sum()} of {ok.size} image picks miss the reference maximum"
    print(f"from_device resample images ({clock}): worst rel-err {worst:.3e} of the oracle image's maximum")


@pytest.mark.parametrize("clock", ["w500", "w499"])
def test_convergence_equal_on_both_caches(device, clock):
    """convergence() with the bench's four ridge modes, sizes 1..3 x 4 draws: equal between the caches, and each entry
    the summed std of bootstrap_ridges on the same draws."""
    from das_diff_veh_amd import bootstrap as bt
    _, host, dev = _case(device, clock)
    m, curves = MODES, _curves()
    args = (m["sigma"], m["ref_idx"], m["lb"], m["ub"], curves)
    got = [bt.convergence(c, 3, 4, *args, rand=random.Random(7)) for c in (host, dev)]
    assert got[0].shape == (4, 3) and np.all(np.isfinite(got[0]))
    assert np.array_equal(got[0], got[1])
    sels = bt.draw_sizes(dev.n, range(1, 4), 4, random.Random(7))
    worst = 0.0
    for k, sel in enumerate(sels):
        rv = bt.bootstrap_ridges(dev, sel, *args)
        for mode in range(4):
            d = abs(float(np.std(np.asarray(rv[mode]), axis=0).sum()) - got[1][mode, k])
            worst = max(worst, d)
            assert d <= 1e-9, (mode, k, d)
    print(f"convergence ({clock}): worst |entry - summed std of bootstrap_ridges| {worst:.3e}")
