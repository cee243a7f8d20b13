"""GPU parity of the w = 500 engine's 10 x 10 x 5 transform: the sample layout of its register-fed first stage
(lane i < 50 holds samples i + 50 t, t < 10; lanes 50-63 repeat lane 49), the cross-pass receiver packing, the
per-pass path with the inverse transform, and the validated launch.  Reference: the float64 oracle, tolerance the
project's gather parity bound.  Synth default pass shape (60 channels x 5 500 samples, pivot 700, 500-900 m,
wlen = 2 s at the dt that gives w = 500)."""
import numpy as np
import pytest

from tests import golden_io as gio

pytestmark = pytest.mark.gpu
TOL = 1e-4
KW = dict(pivot=700, start_x=500, end_x=900, wlen=2)
N_PASS = 24
# first and last lanes (0, 49) and first and last t (0..49, 450..499) of stage 1, and the t boundaries between
POSITIONS = [0, 49, 50, 249, 250, 449, 450, 499]

_cache = {}


def _batch(device):
    """The shared synthetic passes (generated once, never modified: tests clone what they change)."""
    if "batch" not in _cache:
        from das_diff_veh_amd.synth import DT_W500, synth_batch_device
        wins, x, t, trk, _ = synth_batch_device(N_PASS, pivot=700.0, seed=11, device=device, t0=DT_W500)
        _cache["batch"] = (wins, x, t, trk, wins.double().cpu().numpy())
    return _cache["batch"]


def _plan(device, kw, idx):
    from das_diff_veh_amd.plan import VsgParams, VsgPlan, pass_geometry
    wins, x, t, trk, _ = _batch(device)
    prm = VsgParams(**{**KW, **kw})
    geoms = [pass_geometry(x, t, *trk[i], prm) for i in idx]
    assert geoms[0].w == 500 and geoms[0].hop == 250 and geoms[0].nsamp == 1000
    return geoms, VsgPlan(geoms, prm, wins.shape[1], wins.shape[2])


def _oracle(device, kw, i, data=None):
    """Oracle gather of pass i (cached for the unmodified pass)."""
    from oracle import vsg as ovsg
    _, x, t, trk, host = _batch(device)
    key = (i, tuple(sorted(kw.items())))
    if data is None and key in _cache:
        return _cache[key]
    o = dict(data=host[i] if data is None else data, x_axis=x, t_axis=t, veh_state_x=trk[i][0], veh_state_t=trk[i][1])
    with np.errstate(all="ignore"):
        ref = ovsg.virtual_shot_gather(o, **kw, **KW)[0]
    if data is None:
        _cache[key] = ref
    return ref


@pytest.mark.parametrize("kw", [dict(include_other_side=True, norm=False), dict(include_other_side=False, norm=False)])
def test_single_sample_receiver_slices(device, kw):
    """One gather row below the pivot (table-served receivers, packed two per transform; across passes when
    one-sided) and one above it (z = P + i R) per position: the row's receiver samples inside one forward
    sub-window are zero except the sample at the in-slice position.  The sub-window is live in the reference; an
    engine that missed the sample would skip it, which the size of the sample makes visible (checked against the
    oracle of the same data with the sample zeroed too)."""
    from das_diff_veh_amd import vsg
    from oracle import vsg as ovsg
    wins = _batch(device)[0]
    idx = [0, 1, 2, 3]
    geoms, plan = _plan(device, kw, idx)
    geo = geoms[1]
    prow = geo.pivot_idx - geo.start_idx
    data = wins[idx].clone()
    for n, pos in enumerate(POSITIONS):
        for row in (prow - 2 - n, prow + 2 + n):
            a, L = geo.seg[row, 0]
            assert L == geo.nsamp
            s = a + (n % 3) * geo.hop
            data[1, geo.start_idx + row, s:s + geo.w] = 0.0
            data[1, geo.start_idx + row, s + pos] = 40.0
    host1 = data[1].double().cpu().numpy()
    sched = vsg.StackSchedule(np.zeros(len(idx), np.int64), 1, chunk=4)
    got = vsg.vsg_stack(data, plan, sched).double().cpu().numpy()[0]
    refs = [_oracle(device, kw, i, host1 if i == 1 else None) for i in idx]
    err = gio.gather_rel_err(got, ovsg.stack(refs))
    # sensitivity: without the lone samples the class mean moves by far more than the tolerance
    blind = host1.copy()
    blind[host1 == 40.0] = 0.0
    moved = gio.gather_rel_err(ovsg.stack([refs[0], _oracle(device, kw, 1, blind), refs[2], refs[3]]), ovsg.stack(refs))
    print(f"single-sample slices {kw}: err {err:.3e}, lone samples move the mean by {moved:.3e}")
    assert moved > 10 * TOL
    assert err < TOL, (kw, err)


@pytest.mark.parametrize("kw", [dict(include_other_side=True, norm=False), dict(include_other_side=False, norm=False)])
def test_zero_receiver_row_is_exactly_zero(device, kw):
    """norm=False: a gather row whose receiver channel is all zero in every pass of the class is bit-exact 0.0."""
    from das_diff_veh_amd import vsg
    from oracle import vsg as ovsg
    wins = _batch(device)[0]
    idx = [4, 5, 6]
    geoms, plan = _plan(device, kw, idx)
    prow = geoms[0].pivot_idx - geoms[0].start_idx
    rows = [prow - 5, prow + 7]
    data = wins[idx].clone()
    for r in rows:
        data[:, geoms[0].start_idx + r] = 0.0
    host = data.double().cpu().numpy()
    got = vsg.vsg_stack(data, plan, vsg.StackSchedule(np.zeros(3, np.int64), 1, chunk=4)).cpu().numpy()[0]
    for r in rows:
        assert np.array_equal(got[r], np.zeros(plan.w, np.float32)), (kw, r)
    ref = ovsg.stack([_oracle(device, kw, i, host[n]) for n, i in enumerate(idx)])
    assert gio.gather_rel_err(got.astype(np.float64), ref) < TOL


def test_cross_pass_packing_lone_half(device):
    """One-sided rows, classes of 1, 2, 3 and 8 passes in chunks of 8: n = 1 takes the per-pass fallback, n = 3
    with three sub-windows has an odd number of halves (the last transform has no second receiver)."""
    from das_diff_veh_amd import vsg
    from oracle import vsg as ovsg
    wins = _batch(device)[0]
    kw = dict(include_other_side=False, norm=False)
    sizes = [1, 2, 3, 8]
    idx = list(range(8, 8 + sum(sizes)))
    slots = np.repeat(np.arange(len(sizes)), sizes)
    geoms, plan = _plan(device, kw, idx)
    sched = vsg.StackSchedule(slots, len(sizes), chunk=8)
    assert [e - b for b, e, _ in sched.chunk_tab] == sizes
    got = vsg.vsg_stack(wins[idx], plan, sched).double().cpu().numpy()
    for s, n in enumerate(sizes):
        ref = ovsg.stack([_oracle(device, kw, i) for i, sl in zip(idx, slots) if sl == s])
        err = gio.gather_rel_err(got[s], ref)
        print(f"class of {n} passes: err {err:.3e}")
        assert err < TOL, (n, err)


@pytest.mark.parametrize("kw", [dict(include_other_side=True, norm=False), dict(include_other_side=True),
                                dict(include_other_side=False, norm=False)])
def test_per_pass_gathers(device, kw):
    """vsg_gathers at w = 500: one transform per sub-window (z = P + i R) and one inverse per row."""
    from das_diff_veh_amd import vsg
    wins = _batch(device)[0]
    idx = [0, 1, 2, 3]
    geoms, plan = _plan(device, kw, idx)
    got = vsg.vsg_gathers(wins[idx], plan).double().cpu().numpy()
    errs = [gio.gather_rel_err(got[n], _oracle(device, kw, i)) for n, i in enumerate(idx)]
    print(f"per-pass gathers {kw}: max err {max(errs):.3e}")
    assert max(errs) < TOL, (kw, errs)


@pytest.mark.parametrize("kind", ["nan450", "nan499", "inf"])
def test_validated_launch(device, kind):
    """vsg_stack_validated: a NaN at in-slice positions 450 / 499 of a receiver sub-window whose pivot slice is all
    zero (never transformed: found where the samples are loaded), and an inf inside a transformed sub-window, make
    the pass's class NaN; the other classes equal the oracle."""
    from das_diff_veh_amd import vsg
    from oracle import vsg as ovsg
    wins = _batch(device)[0]
    two = kind == "inf"
    kw = dict(include_other_side=two, norm=False)
    idx = [0, 1, 2, 3, 4, 5]
    slots = np.arange(len(idx)) % 3
    geoms, plan = _plan(device, kw, idx)
    geo = geoms[1]
    prow = geo.pivot_idx - geo.start_idx
    data = wins[idx].clone()
    if two:
        a, L = geo.seg[prow + 3, 0]
        data[1, geo.start_idx + prow + 3, a + 400] = float("inf")
    else:
        a, L = geo.seg[prow - 3, 0]
        ap, Lp = geo.seg[prow, 0]
        assert (a, L) == (ap, Lp) and L == geo.nsamp  # the shared forward window
        data[1, geo.pivot_idx, ap:ap + Lp] = 0.0
        # the last sub-window's sample: in no other sub-window of the row
        data[1, geo.start_idx + prow - 3, a + 2 * geo.hop + int(kind[3:])] = float("nan")
    got = vsg.vsg_stack_validated(data, plan, vsg.StackSchedule(slots, 3, chunk=2)).double().cpu().numpy()
    assert np.isnan(got[1]).all()
    for s in (0, 2):
        ref = ovsg.stack([_oracle(device, kw, i) for i, sl in zip(idx, slots) if sl == s])
        assert gio.gather_rel_err(got[s], ref) < TOL, (kind, s)
