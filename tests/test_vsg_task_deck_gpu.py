"""The stack kernels' task deck (FusedOps::deal / hand, vsg_engines.h) at its chunk boundaries, against the float64
oracle: a (chunk, row) task of the fused engines (w = 500: EngF500, w = 499: EngP1024) loads its passes' table words
lane-parallel once and hands them out by readlane: to direct_task whole, to the pass loop (EngF500) in hands of 8
passes.

Shapes as tests/test_vsg_lengths_gpu.py: the six synth passes of 24 channels x 6 500 samples, 19 gather rows.  A batch
is a list of pass specs (source pass, pivot, time_window_to_xcorr / wlen, data modification, late trajectory); its
windows are copies of the six source windows, so every oracle gather is computed once per distinct spec and shared.
Every fourth pass is late: its last rows above the pivot are far rows (clamped window).  Classes of 1, 2 and 67
passes: a chunk size c cuts the large class into tasks of c passes and a short last one (67 is no multiple of
2, 7, 8, 9, 16, 17 or 65); 65 is above the deck's limit of 64 passes (tables read pass by pass), 9, 16 and 17 deal
more than one hand.  Tolerance: the project's gather parity bound, 1e-4 of the gather maximum, per row where rows are
normalised (test_vsg_lengths_gpu._check)."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import test_vsg_lengths_gpu as L

pytestmark = pytest.mark.gpu
N_CH, N_T, R = L.N_CH, L.N_T, L.R
CASES = {500: (2, "W500", 500, 500), 499: (2, "W499", 499, 1024)}
CHUNKS = [1, 2, 7, 8, 9, 16, 17, 65]
FLAGS = dict(zip(L.FLAG_IDS, L.FLAGS))
VALIDATED = ["two_sided", "norm", "one_sided"]  # the validated launch needs norm or norm_amp
SIZES = (1, 2, 67)
GOLDEN_SIZES = (1, 2, 7, 9, 20, 31)  # one chunk (of up to 64 passes) per class: a single add per stack element
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vsg_task_deck_parent.json")

_cache = {}


def _slots(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def _specs(n, unusable=(), mods=None):
    """Pass j: source pass j % 6; every fifth pass has the pivot at 690 m (two rows below the others': passes with
    different pivots, and so different pivot rows, share every chunk of more than four passes); the passes listed in
    `unusable` correlate 3 wlen (five sub-windows per side: more than a table entry holds); mods: {pass: tag}."""
    mods = mods or {}
    return [(j % L.N_PASS, 690 if j % 5 == 3 else 700, 3 if j in unusable else 2, mods.get(j), j % 4 == 1)
            for j in range(n)]


def _trajectory(case, spec):
    """The pass's trajectory; a late one (spec[4]) is delayed so that the three rows above the pivot which the
    vehicle reaches last lie past the record's end on the forward side: their slices are the clamped window [0, nsamp)
    (far rows), the rows before them keep their own, clipped windows (near rows)."""
    p = L._passes(case[1])[spec[0]]
    vx, vt = p["veh_state_x"], p["veh_state_t"]
    if spec[4]:
        from das_diff_veh_amd.plan import interp1d_extrap
        x = np.asarray(p["x_axis"], np.float64)
        piv = int(np.argmax(x >= spec[1]))
        end = int(np.abs(x - L.GEO["end_x"]).argmin())
        ta = np.sort(interp1d_extrap(vx, vt)(x[piv + 1:end]))
        vt = vt + (p["t_axis"][-1] - 1.0 - 0.5 * (ta[-3] + ta[-4]))  # delta_t = 1
    return p, vx, vt


def _kw(case, flags, spec):
    return dict(wlen=case[0], time_window_to_xcorr=spec[2] * case[0], pivot=spec[1], start_x=L.GEO["start_x"],
                end_x=L.GEO["end_x"], **flags)


def _geom(case, flags, spec):
    from das_diff_veh_amd.plan import VsgParams, pass_geometry
    key = ("geom", case, tuple(sorted(flags.items())), spec[:3], spec[4])
    if key not in _cache:
        p, vx, vt = _trajectory(case, spec)
        _cache[key] = pass_geometry(p["x_axis"], p["t_axis"], vx, vt, VsgParams(**_kw(case, flags, spec)))
    return _cache[key]


def _sub(g, row, side, q):
    """Samples [a, a + w) of sub-window q (-1: the last) of a row side."""
    a, n = int(g.seg[row, side, 0]), int(g.seg[row, side, 1])
    nw = (n - g.w) // g.hop + 1
    assert nw >= 1
    a += (q % nw) * g.hop
    return a, a + g.w


def _modify(data, g, tag):
    """The data modifications of a spec, in place on a [N_CH, N_T] array (numpy or torch).  Rows: prow + 3 is a
    receiver above the pivot (its forward slices are its own or the clamped window), prow - 3 one below."""
    prow = g.pivot_idx - g.start_idx
    q = 0 if tag[-1] == "0" else -1
    if tag[:2] == "zp":    # a zero pivot slice: forward sub-window q of the pivot row
        a, b = _sub(g, prow, 0, q)
        data[g.pivot_idx, a:b] = 0.0
    elif tag[:2] == "zr":  # zero receiver slices: sub-window q, forward, of a row on each side of the pivot
        for row in (prow + 3, prow - 3):
            a, b = _sub(g, row, 0, q)
            data[g.start_idx + row, a:b] = 0.0
    elif tag in ("nan_in", "inf_in"):    # inside the first forward slice of a receiver above the pivot
        a, b = _sub(g, prow + 3, 0, 0)
        data[g.start_idx + prow + 3, a + 17] = float("nan") if tag == "nan_in" else float("inf")
    elif tag == "nan_out":  # just outside every slice of that receiver (or the record's last sample)
        ends = [int(g.seg[prow + 3, s, 0] + g.seg[prow + 3, s, 1]) for s in range(2)]
        data[g.start_idx + prow + 3, min(max(ends), N_T - 1)] = float("nan")
    else:
        raise ValueError(tag)


def _oracle(case, flags, spec):
    from oracle import vsg as ovsg
    key = ("ref", case, tuple(sorted(flags.items())), spec)
    if key not in _cache:
        p, vx, vt = _trajectory(case, spec)
        data = p["host"]
        if spec[3] is not None:
            data = data.copy()
            _modify(data, _geom(case, flags, spec), spec[3])
        o = dict(data=data, x_axis=p["x_axis"], t_axis=p["t_axis"], veh_state_x=vx, veh_state_t=vt)
        with np.errstate(all="ignore"):
            _cache[key] = ovsg.virtual_shot_gather(o, **_kw(case, flags, spec))[0]
    return _cache[key]


def _batch(device, case, flags, specs, guard=False):
    """Windows [n, N_CH, N_T] on the device and the launch plan of the specs.  guard: the batch is a view inside a
    larger buffer whose first and last pass-sized blocks are NaN."""
    import torch

    from das_diff_veh_amd.plan import VsgParams, VsgPlan
    base = L._windows(device, case[1])
    n = len(specs)
    buf = torch.full((n + 2, N_CH, N_T), float("nan"), dtype=torch.float32, device=device) if guard else None
    wins = buf[1:n + 1] if guard else torch.empty((n, N_CH, N_T), dtype=torch.float32, device=device)
    wins.copy_(base[torch.as_tensor([s[0] for s in specs], device=device)])
    geoms = [_geom(case, flags, s) for s in specs]
    for j, s in enumerate(specs):
        if s[3] is not None:
            _modify(wins[j], geoms[j], s[3])
    plan = VsgPlan(geoms, VsgParams(**_kw(case, flags, specs[0])), N_CH, N_T)
    assert plan.w == case[2] and plan.R == R
    return wins, plan


def _refs(case, flags, specs, slots):
    from oracle import vsg as ovsg
    per = [_oracle(case, flags, s) for s in specs]
    with np.errstate(all="ignore"):
        return [ovsg.stack([per[j] for j in np.flatnonzero(slots == c)]) for c in range(int(slots.max()) + 1)]


def _stack(kind, wins, plan, sched):
    from das_diff_veh_amd import vsg
    fn = vsg.vsg_stack if kind == "plain" else vsg.vsg_stack_validated
    return fn(wins, plan, sched).cpu().numpy()


def _run(device, tag, case, flags, specs, sizes, chunk, kinds, guard=False, nan_class=()):
    """Stack the batch in chunks of `chunk`; every class equals the oracle's mean, but those of nan_class are NaN."""
    from das_diff_veh_amd import vsg
    slots = _slots(sizes)
    assert len(specs) == slots.size
    wins, plan = _batch(device, case, flags, specs, guard)
    sched = vsg.StackSchedule(slots, len(sizes), chunk=chunk)
    if chunk < max(sizes):
        assert (sched.chunk_tab[:, 1] - sched.chunk_tab[:, 0]).max() == chunk
    refs = _refs(case, flags, specs, slots)
    for kind in kinds:
        got = _stack(kind, wins, plan, sched).astype(np.float64)
        for c, ref in enumerate(refs):
            if c in nan_class:
                assert np.isnan(got[c]).all(), (tag, kind, c)
            else:
                L._check(f"{tag} {kind} chunk {chunk} class {c}", got[c], ref, flags)


def _kinds(flag_id):
    return ["plain", "validated"] if flag_id in VALIDATED else ["plain"]


def test_batch_geometry_covers_the_row_kinds(device):
    """Host arithmetic (the device fixture as in every GPU test): in the chunks of the batch the same gather row is a
    far row (its trajectory slice equals the last row's clamped one) for some passes and a near row (own window) for
    others, passes with both pivots share a chunk, and the pivot row and rows on both sides are gather rows."""
    for w, case in CASES.items():
        specs = _specs(sum(SIZES))
        geoms = [_geom(case, FLAGS["two_sided"], s) for s in specs[3:11]]  # first chunk of 8 of the large class
        prows = {g.pivot_idx - g.start_idx for g in geoms}
        assert len(prows) == 2 and min(prows) >= 4 and max(prows) <= R - 5
        far = np.array([[tuple(g.seg[r, 0]) == (0, g.nsamp) for r in range(max(prows) + 1, R)] for g in geoms])
        assert (far.any(axis=0) & ~far.all(axis=0)).any(), far
        assert all(g.seg[g.pivot_idx - g.start_idx, 0, 1] >= g.w for g in geoms)  # the pivot row correlates


@pytest.mark.parametrize("flag_id", L.FLAG_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("w", sorted(CASES))
def test_chunk_sizes(device, w, chunk, flag_id):
    """Every chunk size, classes of 1, 2 and 67 passes, every flag set; plain and validated stack."""
    _run(device, f"w{w} {flag_id}", CASES[w], FLAGS[flag_id], _specs(sum(SIZES)), SIZES, chunk, _kinds(flag_id))


@pytest.mark.parametrize("flag_id", ["two_sided", "one_sided"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("w", sorted(CASES))
def test_unusable_table_in_a_chunk(device, w, where, flag_id):
    """A pass with five sub-windows per side (its table entries unusable: the plain path) as the first, a middle or
    the last pass of a chunk of 8, between table-served passes."""
    first = 3 + 8  # the large class starts at pass 3: its second chunk of 8 is passes 11 .. 18
    j = {"first": first, "middle": first + 4, "last": first + 7}[where]
    _run(device, f"w{w} {flag_id} unusable {where}", CASES[w], FLAGS[flag_id], _specs(sum(SIZES), unusable=(j,)), SIZES,
         8, _kinds(flag_id))


@pytest.mark.parametrize("flag_id", ["two_sided", "norm", "one_sided"])
@pytest.mark.parametrize("mod", ["zp0", "zpL", "zr0", "zrL"])
@pytest.mark.parametrize("w", sorted(CASES))
def test_zero_slices(device, w, mod, flag_id):
    """A zero pivot slice / zero receiver slices in the first / last sub-window, in the first and the last pass of a
    chunk of 8 (the deck's flag mask; a transform skipped at either end of a hand), and in a chunk of 17 (a
    pass right after a new hand is dealt)."""
    first = 3 + 8
    specs = _specs(sum(SIZES), mods={first: mod, first + 7: mod, 3 + 17 + 8: mod})
    for chunk in (8, 17):
        _run(device, f"w{w} {flag_id} {mod}", CASES[w], FLAGS[flag_id], specs, SIZES, chunk, _kinds(flag_id))


@pytest.mark.parametrize("mod", ["nan_in", "inf_in", "nan_out"])
@pytest.mark.parametrize("where", ["before", "after"])
@pytest.mark.parametrize("w", sorted(CASES))
def test_validated_non_finite(device, w, where, mod):
    """Validated stack: a NaN / inf inside a correlated slice, or a NaN just outside it, in the pass before a chunk
    boundary (the last pass of the two-pass class, whose chunk ends there) or after one (the first pass of the large
    class's second chunk).  The class holding the pass is NaN; the others equal the oracle."""
    j, bad = (2, 1) if where == "before" else (3 + 8, 2)
    for flag_id in ("two_sided", "one_sided"):
        _run(device, f"w{w} {flag_id} {mod} {where}", CASES[w], FLAGS[flag_id], _specs(sum(SIZES), mods={j: mod}),
             SIZES, 8, ["validated"], nan_class=(bad,))


@pytest.mark.parametrize("flag_id", L.FLAG_IDS)
@pytest.mark.parametrize("w", sorted(CASES))
def test_guarded_buffer(device, w, flag_id):
    """The batch is a view inside a larger buffer whose surroundings are NaN: the first and the last pass touch the
    guard, so a load that strays past the batch shows up in the result."""
    for chunk in (8, 9):
        _run(device, f"w{w} {flag_id} guarded", CASES[w], FLAGS[flag_id], _specs(sum(SIZES)), SIZES, chunk,
             _kinds(flag_id), guard=True)


def _golden_runs(device):
    """(name, stack) of the equal-arithmetic cases: one chunk per class (1 .. 31 passes), every flag set, with an
    unusable pass and zero slices among them."""
    from das_diff_veh_amd import vsg
    n = sum(GOLDEN_SIZES)
    specs = _specs(n, unusable=(5, 30), mods={12: "zp0", 26: "zrL", 46: "zpL"})
    slots = _slots(GOLDEN_SIZES)
    for w, case in sorted(CASES.items()):
        for flag_id in L.FLAG_IDS:
            wins, plan = _batch(device, case, FLAGS[flag_id], specs)
            sched = vsg.StackSchedule(slots, len(GOLDEN_SIZES), chunk=64)
            assert sched.chunk_tab.shape[0] == len(GOLDEN_SIZES)
            for kind in _kinds(flag_id):
                yield f"w{w}_{flag_id}_{kind}", _stack(kind, wins, plan, sched)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def record_golden(device):
    """Writes the fixture (run once on the parent build: python -c 'from tests import test_vsg_task_deck_gpu as t;
    t.record_golden("cuda:0")')."""
    import torch
    out = {name: _digest(got) for name, got in _golden_runs(torch.device(device))}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    return out


def test_equal_arithmetic(device):
    """With one chunk per class every stack element is written by a single add of one wave, in the order of the
    passes: the stack is bit-identical to the parent build's (sha256 of the float32 stack of each case, recorded on
    the GPU from the build before the task deck).  With several chunks per class the float atomics of the chunks
    reorder, and only the oracle bound (the other tests) applies."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {name: _digest(a) for name, a in _golden_runs(device)}
    assert sorted(got) == sorted(want)
    diff = [k for k in sorted(got) if got[k] != want[k]]
    print(f"{len(got) - len(diff)} of {len(got)} stacks bit-identical to the parent build's; differing: {diff}")
    assert not diff
