"""The per-lag error budget of the correlation engines (tests/vsg_budget.py) on the host: the float32 restatement
stays within the ratios recorded in golden/vsg_budget_calibration.json, every finite entry has a budget, the budget of
a stack is the weighted sum of its passes', and four defects that the gather-maximum rule (gather_rel_err < 1e-4)
lets through are caught by the budget rule.  No GPU: the constant C is calibrated against the restatement alone."""
import numpy as np
import pytest

from oracle import vsg as ovsg
from tests import golden_io as gio
from tests import test_vsg_lengths_gpu as lengths
from tests import vsg_budget as vb

OLD_TOL = 1e-4
CASES = vb.lengths_cases()


@pytest.mark.parametrize("case", CASES, ids=[f"w{c[2]}" for c in CASES])
def test_restatement_within_recorded_ratio(case):
    """Every case of the calibration sweep: the restatement's ratio is at most 1.05 x the recorded worst of its
    (transform length, flag set) (drift of the helper, NumPy or SciPy), and no finite entry is without a budget."""
    rec = vb.calibration()["ratio"][str(case[3])]
    for flags, fid in zip(lengths.FLAGS, lengths.FLAG_IDS):
        assert vb.flag_name(flags) == fid
        worst = 0.0
        for mult in vb.MULTS:
            for i in range(lengths.N_PASS):
                ratio, unbudgeted = vb.restatement_ratio(case, flags, mult, i)
                assert unbudgeted == 0, (case, fid, mult, i, unbudgeted)
                worst = max(worst, ratio)
        print(f"w={case[2]} nfft={case[3]} {fid}: restatement ratio {worst:.4f}, recorded {rec[fid]:.4f}")
        assert worst <= 1.05 * rec[fid], (case, fid, worst, rec[fid])


def test_calibration_file_covers_the_sweep():
    cal = vb.calibration()
    assert sorted(cal["ratio"], key=int) == sorted({str(c[3]) for c in CASES}, key=int)
    for nfft, per in cal["ratio"].items():
        assert sorted(per) == sorted(lengths.FLAG_IDS)
        assert all(0.01 < r < 1.0 for r in per.values()), (nfft, per)  # the restatement sits well inside C = 1
    assert [tuple(c) for c in cal["cases"]["lengths"]] == [tuple(c) for c in CASES]


def test_substitution_is_restored():
    saved = ovsg.circ_xcorr
    with pytest.raises(RuntimeError):
        with vb.substituted(vb.norm_product):
            assert ovsg.circ_xcorr is vb.norm_product
            raise RuntimeError
    assert ovsg.circ_xcorr is saved


def test_budget_bounds_every_lag_of_the_oracle():
    """|c| <= beta at every lag of an unnormalised gather (Cauchy-Schwarz carried through the oracle), and a zero
    receiver channel has a zero budget, a NaN reference only where its row's norm vanished."""
    case, flags = lengths.BY_W[125], lengths.F_RAW
    win = dict(vb.lengths_window(case[1], 0))
    win["data"] = win["data"].copy()
    x = win["x_axis"]
    row = 3
    win["data"][int(np.argmax(x >= lengths.GEO["start_x"])) + row] = 0.0
    kw = lengths._kw(case, flags, 2)
    ref, beta = vb.budget_gather(win, **kw)
    assert (np.abs(ref) <= beta * (1 + 1e-12)).all()
    assert (beta[row] == 0).all() and (ref[row] == 0).all() and (np.delete(beta, row, 0) > 0).all()
    refn, betan = vb.budget_gather(win, **lengths._kw(case, lengths.F_NORM, 2))
    assert np.isnan(refn[row]).all() and np.isfinite(np.delete(refn, row, 0)).all()
    got = vb.restated_f32_gather(win, case[3], **lengths._kw(case, lengths.F_NORM, 2))
    assert vb.budget_ratio(got, refn, betan, case[3], lengths.F_NORM)[1] == 0


# --- mutants of the restatement: each passes the gather-maximum rule and fails the budget rule ---

MUT_CASE = lengths.BY_W[250]  # an exact engine; the far rows are rows 0 and R - 1 of the 19-row gather
MUT_PASS, MUT_MULT, FAR_ROW = 0, 2, lengths.R - 1
WEAK = 2.0 ** -10


def _mut_setup(flags, weak=True):
    """Pass 0 of the lengths geometry.  weak: the far row's channel scaled by 2^-10 (exact), a receiver whose row is
    a few 1e-5 of the gather's maximum, as far rows of attenuated records are: whatever happens to it is invisible at
    1e-4 of the pivot row's peak, while its budget shrinks with it."""
    win, kw = dict(vb.lengths_window(MUT_CASE[1], MUT_PASS)), lengths._kw(MUT_CASE, flags, MUT_MULT)
    if weak:
        win["data"] = win["data"].copy()
        win["data"][int(np.argmax(win["x_axis"] >= kw["start_x"])) + FAR_ROW] *= WEAK
    ref, beta = vb.budget_gather(win, **kw)
    clean = vb.restated_f32_gather(win, MUT_CASE[3], **kw)
    assert vb.budget_ratio(clean, ref, beta, MUT_CASE[3], flags)[0] <= vb.constant(MUT_CASE[3], flags)
    return win, kw, ref, beta


def _passes_old_fails_new(tag, mutant, ref, beta, flags):
    old = gio.gather_rel_err(mutant, ref)
    ratio, unbudgeted = vb.budget_ratio(mutant, ref, beta, MUT_CASE[3], flags)
    c = vb.constant(MUT_CASE[3], flags)
    print(f"{tag}: gather error {old:.3e} (rule < {OLD_TOL}), budget ratio {ratio:.2f} (rule <= {c:.2f})")
    assert unbudgeted == 0
    assert old < OLD_TOL, (tag, old)
    assert ratio > c, (tag, ratio, c)
    with pytest.raises(AssertionError):
        vb.assert_within_budget(tag, mutant, ref, beta, MUT_CASE[3], flags)


class _FarRowCalls:
    """Wraps oracle.vsg.xcorr_two (one call per trajectory row of a side): the call of the forward side's far row
    gets the mutant."""

    def __init__(self, mutant, target):
        self.mutant, self.target, self.n, self.saved = mutant, target, 0, ovsg.xcorr_two

    def __call__(self, tr1, tr2, w, hop):
        self.n += 1
        return (self.mutant if self.n == self.target else self.saved)(tr1, tr2, w, hop)

    def __enter__(self):
        ovsg.xcorr_two = self
        return self

    def __exit__(self, *exc):
        ovsg.xcorr_two = self.saved


def _n_traj_rows(win, kw):
    """Trajectory rows of the forward side (those above the pivot): its last xcorr_two call is the far row's."""
    x = win["x_axis"]
    return int(np.abs(x - kw["end_x"]).argmin()) - int(np.argmax(x >= kw["pivot"])) - 1


@pytest.mark.parametrize("flags", [lengths.F_ONE, lengths.F_RAW], ids=["one_sided", "raw"])
def test_mutant_receiver_slice_one_sample_off(flags):
    """The far row's receiver slice of its second sub-window starts one sample late."""
    win, kw, ref, beta = _mut_setup(flags)

    def mutant(tr1, tr2, w, hop):
        out = np.zeros(w)
        nwin = (tr1.size - w) // hop + 1
        assert nwin == 3
        for i in range(nwin):
            off = 1 if i == 1 else 0
            out += ovsg.circ_xcorr(tr1[i * hop + off:i * hop + off + w], tr2[i * hop:i * hop + w])
        return np.roll(out, w // 2) / nwin

    with _FarRowCalls(mutant, _n_traj_rows(win, kw)) as calls:
        got = vb.restated_f32_gather(win, MUT_CASE[3], **kw)
    assert calls.n >= calls.target and not np.array_equal(got[FAR_ROW], vb.restated_f32_gather(
        win, MUT_CASE[3], **kw)[FAR_ROW])
    _passes_old_fails_new("slice one sample off", got, ref, beta, flags)


@pytest.mark.parametrize("flags", [lengths.F_ONE, lengths.F_RAW], ids=["one_sided", "raw"])
def test_mutant_far_row_divided_by_nwin_plus_one(flags):
    win, kw, ref, beta = _mut_setup(flags)
    saved = ovsg.xcorr_two

    def mutant(tr1, tr2, w, hop):
        nwin = (tr1.size - w) // hop + 1
        return saved(tr1, tr2, w, hop) * nwin / (nwin + 1)

    with _FarRowCalls(mutant, _n_traj_rows(win, kw)):
        got = vb.restated_f32_gather(win, MUT_CASE[3], **kw)
    _passes_old_fails_new("1 / (nwin + 1)", got, ref, beta, flags)


@pytest.mark.parametrize("flags", [lengths.F_ONE, dict(include_other_side=False)], ids=["one_sided", "norm_one_sided"])
def test_mutant_twiddle_like_bin(flags):
    """One frequency bin of one receiver spectrum (the row next to the pivot's, every sub-window) times 1 + 3e-5."""
    win, kw, ref, beta = _mut_setup(flags, weak=False)
    x = win["x_axis"]
    prow = int(np.argmax(x >= kw["pivot"])) - int(np.argmax(x >= kw["start_x"]))
    hit = []

    def mutate(fa, fb):
        if fb.ndim == 2 and fb.shape[0] == prow + 1:  # the forward side's xcorr_vshot: shared rows, the pivot's last
            k = int(np.argmax(np.abs(fb[prow - 1])))
            fb = fb.copy()
            fb[prow - 1, k] *= np.complex64(1 + 3e-5)
            hit.append(k)
        return fa, fb

    got = vb.restated_f32_gather(win, MUT_CASE[3], mutate=mutate, **kw)
    assert hit
    _passes_old_fails_new("one bin x (1 + 3e-5)", got, ref, beta, flags)


@pytest.mark.parametrize("flags", [lengths.F_ONE, lengths.F_TWO, lengths.F_RAW], ids=["one_sided", "two_sided", "raw"])
def test_mutant_far_row_scaled(flags):
    win, kw, ref, beta = _mut_setup(flags)
    got = vb.restated_f32_gather(win, MUT_CASE[3], **kw)
    got[FAR_ROW] *= 1 + 2e-3
    _passes_old_fails_new("far row x (1 + 2e-3)", got, ref, beta, flags)


def test_stack_budget_is_the_weighted_sum():
    """Class means of SLOTS (1 and 5 passes): the reference is oracle.vsg.stack's, the budget the mean of the passes'
    budgets, the accumulation term u x the mean of |ref_p|; uneven weights likewise."""
    case, flags = lengths.BY_W[125], lengths.F_TWO
    kw = lengths._kw(case, flags, 2)
    wins = [vb.lengths_window(case[1], i) for i in range(lengths.N_PASS)]
    per = [vb.budget_gather(w, **kw) for w in wins]
    classes = vb.budget_stack(wins, lengths.SLOTS, 2, **kw)
    for s, (ref, beta, extra) in enumerate(classes):
        idx = np.flatnonzero(lengths.SLOTS == s)
        assert np.allclose(ref, ovsg.stack([per[i][0] for i in idx]), rtol=1e-13, atol=1e-15)
        assert np.allclose(beta, np.sum([per[i][1] for i in idx], axis=0) / len(idx), rtol=1e-14, atol=0)
        assert np.allclose(extra, vb.U * np.sum([np.abs(per[i][0]) for i in idx], axis=0) / len(idx), rtol=1e-14)
        got = ovsg.stack([vb.restated_f32_gather(wins[i], case[3], **kw) for i in idx])
        ratio, unbudgeted = vb.budget_ratio(got, ref, beta, case[3], flags, extra)
        assert unbudgeted == 0 and ratio <= vb.calibration()["ratio"][str(case[3])]["two_sided"]
    wts = [0.5, 0.25, 0.25]
    ref, beta, _ = vb.stack_budget([p[0] for p in per[:3]], [p[1] for p in per[:3]], wts)
    assert np.allclose(beta, 0.5 * per[0][1] + 0.25 * per[1][1] + 0.25 * per[2][1], rtol=1e-14, atol=0)
