"""The production correlation engines (w = 500: EngF500, exact 10 x 10 x 5; w = 499: EngP1024, padded) held to the
per-lag float32 error budget of tests/vsg_budget.py, beside the gather-maximum tolerance: per-pass gathers, the class
stack with and without the pivot-slice table, and the validated stack, at wlen = 2 on the two clocks.

Batches: "six", the lengths test's geometry (6 passes of 24 x 6 500, R = 19; the validated launch scans 32.8 KB per
(pass, row): 5 + 3 waves at w = 500); "mixed", the 24 passes at two fiber offsets of test_vsg_stack_more_gpu (60 x 5 500,
R = 49, pivot rows 24 and 25; 26.9 KB: 7 + 1 waves); "far", six passes of 256 x 4 096 whose far rows take the clamped
trajectory window [0, nsamp) (the pivot-slice table's far-row entries).  The budgets come from each pass's own axes and
trajectory; C is read from golden/vsg_budget_calibration.json (host-calibrated, never measured on the kernels)."""
import numpy as np
import pytest

from tests import test_vsg_lengths_gpu as L
from tests import vsg_budget as vb

pytestmark = pytest.mark.gpu
CASES = {c[2]: c for c in vb.EXTRA_CASES}  # w -> (wlen, clock, w, transform length)
FLAGS = dict(zip(L.FLAG_IDS, L.FLAGS))
W71, W53 = 16 * 7 + 1, 16 * 5 + 3
WAVES = {"six": W53, "mixed": W71}
_cache = {}


def _batch(device, name, w):
    """(device windows [n, C, T], oracle windows, geometry keywords, class slots, chunk) of a batch on w's clock."""
    key = ("batch", name, w)
    if key in _cache:
        return _cache[key]
    from das_diff_veh_amd import synth
    clock = CASES[w][1]
    t0 = getattr(synth, "DT_" + clock)
    if name == "six":
        wins = L._windows(device, clock)
        windows = [vb.lengths_window(clock, i) for i in range(L.N_PASS)]
        geo, slots, chunk = dict(L.GEO), L.SLOTS, 2
    else:
        if name == "mixed":
            from tests.test_vsg_stack_more_gpu import KW, _mixed_batch
            wins, xs, ts, trk = _mixed_batch(device, t0=t0)
            geo = {k: KW[k] for k in ("pivot", "start_x", "end_x")}
            slots, chunk = np.arange(len(trk)) % 3, 4
        else:
            wins, x, t, trk, _ = synth.synth_batch_device(6, n_ch=256, n_t=4096, pivot=1044.0, seed=31, device=device,
                                                          x_first=0.0, track_half=300, chunk=2, t0=t0)
            xs, ts = [x] * 6, [t] * 6
            geo, slots, chunk = dict(pivot=1044.0, start_x=0.0, end_x=2100.0), np.arange(6) % 2, 4
        host = wins.double().cpu().numpy()
        windows = [dict(data=host[i], x_axis=xs[i], t_axis=ts[i], veh_state_x=trk[i][0], veh_state_t=trk[i][1])
                   for i in range(len(trk))]
    _cache[key] = wins, windows, geo, np.asarray(slots), chunk
    return _cache[key]


def _plan(device, name, w, flags):
    from das_diff_veh_amd import _lib
    from das_diff_veh_amd.plan import VsgParams, VsgPlan, pass_geometry
    wins, windows, geo, _, _ = _batch(device, name, w)
    prm = VsgParams(wlen=2, **flags, **geo)
    geoms = [pass_geometry(o["x_axis"], o["t_axis"], o["veh_state_x"], o["veh_state_t"], prm) for o in windows]
    plan = VsgPlan(geoms, prm, wins.shape[1], wins.shape[2])
    assert plan.w == w and _lib.load().dvh_vsg_fft_length(w) == CASES[w][3]
    return plan


def _budgets(device, name, w, flag_id):
    """[(oracle gather, budget)] per pass, computed once per (batch, w, flag set) and left unchanged."""
    key = ("budget", name, w, flag_id)
    if key not in _cache:
        _, windows, geo, _, _ = _batch(device, name, w)
        _cache[key] = [vb.budget_gather(o, wlen=2, **FLAGS[flag_id], **geo) for o in windows]
    return _cache[key]


def _check_classes(device, tag, got, name, w, flag_id):
    _, _, _, slots, _ = _batch(device, name, w)
    per = _budgets(device, name, w, flag_id)
    got = got.double().cpu().numpy()
    assert got.shape[0] == slots.max() + 1
    for s in range(got.shape[0]):
        ref, beta, extra = L._stack_budget([per[i] for i in np.flatnonzero(slots == s)])
        L._check(f"{tag} {name} w={w} {flag_id} class {s}", got[s], ref, FLAGS[flag_id], CASES[w], beta, extra)


def _sched(device, name, w):
    from das_diff_veh_amd import vsg
    _, _, _, slots, chunk = _batch(device, name, w)
    return vsg.StackSchedule(slots, int(slots.max()) + 1, chunk=chunk)


@pytest.mark.parametrize("flag_id", L.FLAG_IDS)
@pytest.mark.parametrize("w", [500, 499])
@pytest.mark.parametrize("name", ["six", "mixed"])
def test_per_pass_gathers(device, name, w, flag_id):
    from das_diff_veh_amd import vsg
    plan = _plan(device, name, w, FLAGS[flag_id])
    got = vsg.vsg_gathers(_batch(device, name, w)[0], plan).double().cpu().numpy()
    for i, (ref, beta) in enumerate(_budgets(device, name, w, flag_id)):
        L._check(f"gathers {name} w={w} {flag_id} pass {i}", got[i], ref, FLAGS[flag_id], CASES[w], beta)


@pytest.mark.parametrize("table", [True, False], ids=["table", "no_table"])
@pytest.mark.parametrize("flag_id", L.FLAG_IDS)
@pytest.mark.parametrize("w", [500, 499])
@pytest.mark.parametrize("name", ["six", "mixed"])
def test_class_stack(device, name, w, flag_id, table):
    """vsg_stack with the pivot-slice spectra table (receivers two per transform) and with one transform per
    sub-window."""
    from das_diff_veh_amd import vsg
    plan = _plan(device, name, w, FLAGS[flag_id])
    got = vsg.vsg_stack(_batch(device, name, w)[0], plan, _sched(device, name, w), table=table)
    _check_classes(device, f"stack table={table}", got, name, w, flag_id)


@pytest.mark.parametrize("flag_id", ["two_sided", "norm", "one_sided"])
@pytest.mark.parametrize("w", [500, 499])
@pytest.mark.parametrize("name", ["six", "mixed"])
def test_validated_stack(device, name, w, flag_id):
    """The fused validated launch; at w = 500 one batch per block shape (5 + 3 and 7 + 1 correlation + scan waves)."""
    from das_diff_veh_amd import _lib, vsg
    plan = _plan(device, name, w, FLAGS[flag_id])
    wins = _batch(device, name, w)[0]
    waves = _lib.load().dvh_vsg_stack_validated_waves(w, plan.n_pass, wins.shape[1], wins.shape[2], plan.n_pass, plan.R)
    assert waves == (WAVES[name] if w == 500 else W71), (name, w, waves)
    got = vsg.vsg_stack_validated(wins, plan, _sched(device, name, w))
    _check_classes(device, "validated", got, name, w, flag_id)


@pytest.mark.parametrize("flag_id", ["two_sided", "one_sided"])
@pytest.mark.parametrize("w", [500, 499])
def test_far_rows_with_clamped_windows(device, w, flag_id):
    """Rows the vehicle reaches after the record's end correlate the clamped window [0, nsamp): with the table and
    without it every such row stays within its own budget (unnormalised: the pivot row's peak would hide them)."""
    from das_diff_veh_amd import vsg
    plan = _plan(device, "far", w, FLAGS[flag_id])
    clamped = 0
    for g in plan.geoms:
        above = np.arange(g.pivot_idx - g.start_idx + 1, plan.R)
        clamped += int(((g.seg[above, 0, 0] == 0) & (g.seg[above, 0, 1] == g.nsamp)).sum())
    assert clamped >= plan.n_pass, "no clamped far rows"
    for table in (True, False):
        got = vsg.vsg_stack(_batch(device, "far", w)[0], plan, _sched(device, "far", w), table=table)
        _check_classes(device, f"stack table={table}", got, "far", w, flag_id)
