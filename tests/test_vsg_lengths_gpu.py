"""GPU parity of the VSG kernels at every correlation window length w the dispatch serves, against the float64
oracle: the six engines of the engine table (engine_for, dvh_vsg.hip) at their first, last and odd w, through the
per-pass gathers, the plain and validated class stacks, other sub-window counts, single samples at the edges of the
load masks, and the error beyond w = 1024.  Besides the gather-maximum tolerance every comparison holds the
kernels to the per-lag float32 error budget of tests/vsg_budget.py (row by row and lag by lag, C calibrated on the
host against a float32 restatement of the oracle).

Passes: synth_pass, 24 channels x 6 500 samples (610 m first channel), pivot 700, gather rows 620-780 m (19 rows: 10
below the pivot row, 8 above), delta_t = 1.  6 500 samples, not the 5 500 of the other VSG tests: at w ~ 1000 the two
8 s correlation windows of a far row then fit the record on both sides for most rows (_check_geometry).  w is set
through wlen on the two clocks DT_W500 / DT_W499 (dt just below / above 0.004).  Tolerance: the project's gather parity
bound (fp32 kernels against float64), plus the same bound per row where rows are normalised."""
import numpy as np
import pytest

from tests import golden_io as gio

pytestmark = pytest.mark.gpu
TOL = 1e-4
GEO = dict(pivot=700, start_x=620, end_x=780)
N_CH, N_T, N_PASS, R = 24, 6500, 6, 19

# (wlen, clock, w, transform length)
TABLE = [
    (0.01, "W500", 2, 512),      # smallest legal w, hop = 1
    (0.26, "W499", 64, 512),     # lane-group boundary of the lane + 64 j loads
    (0.26, "W500", 65, 512),
    (0.5, "W500", 125, 512),     # odd w, hop 62
    (1, "W499", 249, 512),       # the other clock of wlen = 1
    (1.026, "W500", 256, 512),   # 2w - 1 = 511: last w of the 512 engine
    (1, "W500", 250, 250),       # exact 2 x 5 x 5 x 5
    (1.03, "W500", 257, 1024),   # first w of EngP1024
    (1.5, "W500", 375, 1024),    # EngP1024 mid-range, odd
    (2.05, "W500", 512, 1024),   # 2w - 1 = 1023: every sample register live
    (2.054, "W500", 513, 2048),  # first w of the 2048 engine
    (3, "W500", 750, 2048),
    (4, "W499", 999, 2048),      # the other clock of a 500 Hz-style window
    (4.098, "W500", 1024, 2048),  # 2w - 1 = 2047: last supported w
    (4, "W500", 1000, 1000),     # exact 4 x 2 x 5 x 5 x 5
]
CASE_IDS = [f"w{c[2]}" for c in TABLE]
BY_W = {c[2]: c for c in TABLE}
# one exact engine, one 512-padded, EngP1024, the 2048 engine
SUBWIN_CASES = [BY_W[250], BY_W[125], BY_W[375], BY_W[750]]
SUBWIN_IDS = [f"w{c[2]}" for c in SUBWIN_CASES]

F_TWO = dict(include_other_side=True, norm=False)
F_NORM = dict(include_other_side=True)
F_ONE = dict(include_other_side=False, norm=False)
F_RAW = dict(include_other_side=True, norm=False, norm_amp=False)  # scales from window_sumsq
FLAGS = [F_TWO, F_NORM, F_ONE, F_RAW]
FLAG_IDS = ["two_sided", "norm", "one_sided", "raw"]

# two classes of 1 and 5 passes; chunks of 2: a one-pass class and a class spanning three chunks
SLOTS = np.array([1, 0, 1, 1, 1, 1])

_cache = {}


def _passes(clock):
    """The six host passes of a clock (generated once, never modified: tests copy what they change)."""
    key = ("passes", clock)
    if key not in _cache:
        from das_diff_veh_amd import synth
        from oracle import vsg as ovsg
        out = []
        for i in range(N_PASS):
            p = synth.synth_pass(300 + i, n_ch=N_CH, n_t=N_T, x_first=610.0, t0=getattr(synth, "DT_" + clock))
            vx, vt = ovsg.veh_state_xt(p["veh_state"], p["start_x_tracking"], p["distance_along_fiber_tracking"],
                                       p["t_axis_tracking"])
            out.append(dict(data=p["data"], host=p["data"].astype(np.float64), x_axis=p["x_axis"], t_axis=p["t_axis"],
                            veh_state_x=vx, veh_state_t=vt))
        _cache[key] = out
    return _cache[key]


def _windows(device, clock):
    import torch
    key = ("dev", clock)
    if key not in _cache:
        _cache[key] = torch.as_tensor(np.stack([p["data"] for p in _passes(clock)]), device=device)
    return _cache[key]


def _kw(case, flags, mult):
    """Keyword arguments of the oracle / VsgParams: the default time_window_to_xcorr is 2 wlen."""
    return dict(wlen=case[0], time_window_to_xcorr=mult * case[0], **flags, **GEO)


def _plan(case, flags, mult=2, idx=range(N_PASS)):
    """Geometries and launch plan of passes idx; the case must reach the engine it is named for."""
    from das_diff_veh_amd import _lib
    from das_diff_veh_amd.plan import VsgParams, VsgPlan, pass_geometry
    wlen, clock, w, nfft = case
    prm = VsgParams(**_kw(case, flags, mult))
    ps = _passes(clock)
    geoms = [pass_geometry(ps[i]["x_axis"], ps[i]["t_axis"], ps[i]["veh_state_x"], ps[i]["veh_state_t"], prm)
             for i in idx]
    plan = VsgPlan(geoms, prm, N_CH, N_T)
    assert plan.w == w and plan.R == R, (plan.w, plan.R)
    assert plan.hop == w // 2
    assert _lib.load().dvh_vsg_fft_length(plan.w) == nfft
    return geoms, plan


def _budget(case, flags, mult, i, data=None):
    """(oracle gather, per-lag budget) of pass i (cached per (case, flags, sub-window count, pass) for the unmodified
    pass)."""
    from tests import vsg_budget
    key = ("ref", case, tuple(sorted(flags.items())), mult, i)
    if data is None and key in _cache:
        return _cache[key]
    p = _passes(case[1])[i]
    o = dict(data=p["host"] if data is None else data, x_axis=p["x_axis"], t_axis=p["t_axis"],
             veh_state_x=p["veh_state_x"], veh_state_t=p["veh_state_t"])
    ref = vsg_budget.budget_gather(o, **_kw(case, flags, mult))
    if data is None:
        _cache[key] = ref
    return ref


def _oracle(case, flags, mult, i, data=None):
    return _budget(case, flags, mult, i, data)[0]


def _stack_budget(per):
    """(oracle.vsg.stack of the gathers, budget, float32 accumulation term) of [(gather, budget)]."""
    from oracle import vsg as ovsg
    from tests import vsg_budget
    _, beta, extra = vsg_budget.stack_budget([r for r, _ in per], [b for _, b in per])
    with np.errstate(all="ignore"):
        return ovsg.stack([r for r, _ in per]), beta, extra


def _class_refs(case, flags, mult):
    """Oracle class means of SLOTS with their budgets: [(ref, beta, extra)] per class."""
    per = [_budget(case, flags, mult, i) for i in range(N_PASS)]
    return [_stack_budget([per[i] for i in range(N_PASS) if SLOTS[i] == s]) for s in range(2)]


def row_rel_err(got, ref):
    """max over rows of max |got_row - ref_row| / max |ref_row| (finite reference entries; rows without a finite
    non-zero entry are left to gather_rel_err's pattern checks)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    worst = 0.0
    for g, r in zip(got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])):
        m = np.isfinite(r)
        if m.any() and np.abs(r[m]).max() > 0:
            worst = max(worst, float(np.abs(g[m] - r[m]).max() / np.abs(r[m]).max()))
    return worst


def _check(tag, got, ref, flags, case=None, beta=None, extra=0.0):
    """Gather parity, and per-row parity where every row is normalised (a wrong far row cannot hide under a strong
    near one); prints both figures.  Then the per-lag budget (tests/vsg_budget.py), which holds every row to its own
    scale with or without normalisation; every caller in this module passes it (case, beta; extra for a stack)."""
    from tests import vsg_budget
    err, rerr = gio.gather_rel_err(got, ref), row_rel_err(got, ref)
    print(f"{tag}: err {err:.3e}, per-row {rerr:.3e}")
    assert err < TOL, (tag, err)
    if flags.get("norm", True):
        assert rerr < TOL, (tag, rerr)
    if beta is not None:
        vsg_budget.assert_within_budget(tag, got, ref, beta, case[3], flags, extra, w=case[2])
    return err


def _sched(chunk=2):
    from das_diff_veh_amd import vsg
    sched = vsg.StackSchedule(SLOTS, 2, chunk=chunk)
    if chunk == 2:
        assert sorted(e - b for b, e, _ in sched.chunk_tab) == [1, 1, 2, 2]
    return sched


def _run_gathers(device, case, flags, mult=2):
    from das_diff_veh_amd import vsg
    _, plan = _plan(case, flags, mult)
    got = vsg.vsg_gathers(_windows(device, case[1]), plan).double().cpu().numpy()
    assert got.shape == (N_PASS, R, case[2])
    for i in range(N_PASS):
        ref, beta = _budget(case, flags, mult, i)
        _check(f"gathers w={case[2]} x{mult} {flags} pass {i}", got[i], ref, flags, case, beta)


def _run_stack(device, case, flags, mult=2):
    from das_diff_veh_amd import vsg
    _, plan = _plan(case, flags, mult)
    got = vsg.vsg_stack(_windows(device, case[1]), plan, _sched()).double().cpu().numpy()
    assert got.shape == (2, R, case[2])
    for s, (ref, beta, extra) in enumerate(_class_refs(case, flags, mult)):
        _check(f"stack w={case[2]} x{mult} {flags} class {s}", got[s], ref, flags, case, beta, extra)


@pytest.mark.parametrize("case", TABLE, ids=CASE_IDS)
def test_geometry_is_not_hollow(device, case):
    """Host arithmetic only (the device fixture is taken so that, as in every GPU test, torch is imported before the
    library is loaded): in every pass of every table case the pivot row and at least half of the rows have the full
    sub-window count on both sides, so that no case tests mostly clipped (empty) row sides."""
    from das_diff_veh_amd.plan import seg_nwin
    for mult in (2, 1):
        geoms, plan = _plan(case, F_TWO, mult)
        for g in geoms:
            full = (g.nsamp - g.w) // g.hop + 1
            assert full == (1 if mult == 1 else (4 if g.w == 2 else 3))
            ok = (seg_nwin(g.seg, g.w, g.hop) == full).all(axis=1)
            assert ok[g.pivot_idx - g.start_idx] and ok.sum() >= (R + 1) // 2, (case, mult, ok)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("case", TABLE, ids=CASE_IDS)
def test_per_pass_gathers(device, case, flags):
    """vsg_scales_kernel + vsg_gather_kernel of the case's engine: one transform per sub-window, one inverse per row."""
    _run_gathers(device, case, flags)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("case", TABLE, ids=CASE_IDS)
def test_class_stack(device, case, flags):
    """vsg_stackf_kernel (exact engines: phase-ramp class sums) / vsg_stackp_kernel (padded: summed side spectra,
    folded once per task) over a one-pass class and a five-pass class in chunks of 2."""
    _run_stack(device, case, flags)


@pytest.mark.parametrize("flags", [F_TWO, F_NORM, F_ONE], ids=["two_sided", "norm", "one_sided"])
@pytest.mark.parametrize("case", TABLE, ids=CASE_IDS)
def test_validated_stack(device, case, flags):
    """vsg_stack_validated (transform lengths 250, 1000, 2048: the scan as its own launch, then the plain stack
    launch; 512: the generic fused launch): the clean batch equals the oracle's class means; a NaN in a channel no
    gather row reads, or an all-zero window, makes that pass's class NaN and leaves the other class equal to the
    oracle."""
    from das_diff_veh_amd import vsg
    _, plan = _plan(case, flags)
    wins = _windows(device, case[1])
    refs = _class_refs(case, flags, 2)
    got = vsg.vsg_stack_validated(wins, plan, _sched()).double().cpu().numpy()
    for s in range(2):
        _check(f"validated w={case[2]} {flags} clean class {s}", got[s], refs[s][0], flags, case, *refs[s][1:])
    # pass 3 (the five-pass class 1): channel 23 lies beyond end_x; pass 1 (the one-pass class 0): all zero
    assert plan.geoms[3].end_idx <= N_CH - 1
    for p, kind in ((3, "nan"), (1, "zero")):
        data = wins.clone()
        if kind == "nan":
            data[p, N_CH - 1, 1234] = float("nan")
        else:
            data[p] = 0.0
        got = vsg.vsg_stack_validated(data, plan, _sched()).double().cpu().numpy()
        bad, good = int(SLOTS[p]), 1 - int(SLOTS[p])
        assert np.isnan(got[bad]).all(), (case, kind)
        _check(f"validated w={case[2]} {flags} {kind} in pass {p}, class {good}", got[good], refs[good][0], flags, case,
               *refs[good][1:])


@pytest.mark.parametrize("mult", [1, 3])
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("case", SUBWIN_CASES, ids=SUBWIN_IDS)
def test_subwindow_counts(device, case, flags, mult):
    """time_window_to_xcorr = wlen (one sub-window per row side) and 3 wlen (five: more than the pivot-slice table
    holds, so EngP1024's passes are marked unusable and their rows take the plain path), gathers and class stacks."""
    geoms, _ = _plan(case, flags, mult)
    g = geoms[0]
    assert (g.nsamp - g.w) // g.hop + 1 == (1 if mult == 1 else 5)
    assert g.seg[g.pivot_idx - g.start_idx, 0, 1] == g.nsamp  # the pivot row's forward side is not clipped
    _run_gathers(device, case, flags, mult)
    _run_stack(device, case, flags, mult)


def _edge_rows(geo):
    """Row pairs (one below the pivot, one above it) for the load-mask tests, nearest first."""
    prow = geo.pivot_idx - geo.start_idx
    return [(prow - 2 - n, prow + 1 + n) for n in range(7)]


@pytest.mark.parametrize("flags", [F_TWO, F_ONE], ids=["two_sided", "one_sided"])
@pytest.mark.parametrize("case", TABLE, ids=CASE_IDS)
def test_single_sample_receiver_slices(device, case, flags):
    """One sub-window [a, a + w) per row side.  Per in-slice position, one row below the pivot and one above it have
    their receiver's forward slice zeroed except a lone sample of 40.0 at the position: the first and last samples,
    both sides of the lane-group boundary (63, 64) and of the half-window.  An engine whose load mask or fold dropped
    the sample would leave the row zero; the oracle of the same data without the lone samples differs in every such
    row by far more than the tolerance.  Checked through the per-pass gathers and through a four-pass class stack."""
    from das_diff_veh_amd import vsg
    from oracle import vsg as ovsg
    w = case[2]
    positions = sorted({p for p in (0, 63, 64, w // 2 - 1, w // 2, w - 2, w - 1) if 0 <= p < w})
    idx = [0, 1, 2, 3]
    geoms, plan = _plan(case, flags, 1, idx)
    geo = geoms[1]
    wins = _windows(device, case[1])
    data = wins[idx].clone()
    rows = []
    for (lo, hi), pos in zip(_edge_rows(geo), positions):
        for row in (lo, hi):
            a, L = geo.seg[row, 0]
            assert L == geo.nsamp == w and 0 <= row < R
            data[1, geo.start_idx + row, a:a + w] = 0.0
            data[1, geo.start_idx + row, a + pos] = 40.0
            rows.append(row)
    host1 = data[1].double().cpu().numpy()
    ref1, beta1 = _budget(case, flags, 1, 1, host1)
    blind = host1.copy()
    blind[host1 == 40.0] = 0.0
    assert (host1 == 40.0).sum() == len(rows)
    refb = _oracle(case, flags, 1, 1, blind)
    scale = np.abs(ref1).max()
    moved = min(np.abs(ref1[r] - refb[r]).max() / scale for r in rows)
    print(f"w={w} {flags}: positions {positions}, the lone samples move every row by >= {moved:.3e}")
    assert moved > 10 * TOL
    got = vsg.vsg_gathers(data, plan).double().cpu().numpy()
    _check(f"single samples w={w} {flags} gathers", got[1], ref1, flags, case, beta1)
    sched = vsg.StackSchedule(np.zeros(len(idx), np.int64), 1, chunk=4)
    got = vsg.vsg_stack(data, plan, sched).double().cpu().numpy()[0]
    per = [(ref1, beta1) if i == 1 else _budget(case, flags, 1, i) for i in idx]
    refs = [r for r, _ in per]
    ref, beta, extra = _stack_budget(per)
    _check(f"single samples w={w} {flags} stack", got, ref, flags, case, beta, extra)
    moved = gio.gather_rel_err(ovsg.stack([refb if i == 1 else r for i, r in zip(idx, refs)]), ovsg.stack(refs))
    assert moved > 10 * TOL


@pytest.mark.parametrize("flags", [F_TWO, F_ONE], ids=["two_sided", "one_sided"])
@pytest.mark.parametrize("case", TABLE, ids=CASE_IDS)
def test_samples_next_to_the_slices_are_not_read(device, case, flags):
    """One sub-window [a, a + w) per row side, the data intact but for spikes of 1e4 on every row's channel at a - 1
    and a + w of each side (where inside the record and in no slice of that row).  No sub-window of the row covers
    them, so the row equals the oracle's, which never reads them; an n <= w load mask or a fold one lag off would add
    a term 1e4 times a pivot sample.  The pivot channel (every row's other operand) stays clean."""
    from das_diff_veh_amd import vsg
    from oracle import vsg as ovsg
    w = case[2]
    idx = [0, 1]
    geoms, plan = _plan(case, flags, 1, idx)
    geo = geoms[1]
    prow = geo.pivot_idx - geo.start_idx
    sides = 2 if flags["include_other_side"] else 1
    data = _windows(device, case[1])[idx].clone()
    n_spike = 0
    for row in range(R):
        if row == prow:
            continue
        own = [(int(geo.seg[row, s, 0]), int(geo.seg[row, s, 1])) for s in range(sides)]
        for a, L in own:
            assert L == w
            for t in (a - 1, a + w):
                if 0 <= t < N_T and not any(b <= t < b + Lb for b, Lb in own):
                    data[1, geo.start_idx + row, t] = 1e4
                    n_spike += 1
    assert n_spike >= 2 * sides * (R - 1) - 4
    host1 = data[1].double().cpu().numpy()
    ref1, beta1 = _budget(case, flags, 1, 1, host1)
    got = vsg.vsg_gathers(data, plan).double().cpu().numpy()
    _check(f"spikes beside the slices w={w} {flags} gathers", got[1], ref1, flags, case, beta1)
    got = vsg.vsg_stack(data, plan, vsg.StackSchedule(np.zeros(2, np.int64), 1, chunk=2)).double().cpu().numpy()[0]
    ref, beta, extra = _stack_budget([_budget(case, flags, 1, 0), (ref1, beta1)])
    _check(f"spikes beside the slices w={w} {flags} stack", got, ref, flags, case, beta, extra)


def test_unsupported_length_raises(device):
    """w = 1025 (2w - 1 > 2048: no engine): every entry point raises and writes nothing."""
    import torch

    from das_diff_veh_amd import engine, vsg
    from das_diff_veh_amd.apis.data_classes import SurfaceWaveWindow
    from das_diff_veh_amd.plan import VsgParams, VsgPlan, pass_geometry
    from das_diff_veh_amd.synth import DT_W500, synth_pass
    prm = VsgParams(wlen=4.102, **F_TWO, **GEO)
    ps = _passes("W500")
    geoms = [pass_geometry(p["x_axis"], p["t_axis"], p["veh_state_x"], p["veh_state_t"], prm) for p in ps]
    plan = VsgPlan(geoms, prm, N_CH, N_T)
    assert plan.w == 1025
    wins = _windows(device, "W500")
    msg = "unsupported correlation window length"
    out = torch.full((N_PASS, R, plan.w), 7.0, dtype=torch.float32, device=device)
    with pytest.raises(ValueError, match=msg):
        vsg.vsg_gathers(wins, plan, out=out)
    with pytest.raises(ValueError, match=msg):
        vsg.vsg_gathers(wins, plan, scales=torch.ones((N_PASS, 2), dtype=torch.float32, device=device), out=out)
    sout = torch.full((2, R, plan.w), 7.0, dtype=torch.float32, device=device)
    with pytest.raises(ValueError, match=msg):
        vsg.vsg_stack(wins, plan, _sched(), out=sout)
    with pytest.raises(ValueError, match=msg):
        vsg.vsg_stack_validated(wins, plan, _sched(), out=sout)
    with pytest.raises(ValueError, match=msg):
        vsg.vsg_scales(wins, plan)
    torch.cuda.synchronize(device)
    assert bool((out == 7.0).all()) and bool((sout == 7.0).all())
    raw = [synth_pass(300 + i, n_ch=N_CH, n_t=N_T, x_first=610.0, t0=DT_W500) for i in range(2)]
    windows = [SurfaceWaveWindow(p["data"], p["x_axis"], p["t_axis"], p["veh_state"], p["start_x_tracking"],
                                 p["distance_along_fiber_tracking"], p["t_axis_tracking"]) for p in raw]
    for flags in (F_TWO, F_RAW):  # the validated and the plain stack launch
        with pytest.raises(ValueError, match=msg):
            engine.stacked(windows, VsgParams(wlen=4.102, **flags, **GEO), device=device)
