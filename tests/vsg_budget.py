"""Per-lag float32 error budget of a virtual shot gather (TEST INFRASTRUCTURE ONLY, no GPU).

Every output of the oracle (oracle/vsg.py) is a non-negative linear combination of circ_xcorr(a, b) calls, followed by
normalisations.  Each lag of circ_xcorr(a, b) is at most ||a||_2 ||b||_2 (Cauchy-Schwarz), and a float32 FFT
correlation of transform length nfft errs per lag on the scale u log2(nfft) ||a||_2 ||b||_2, u = 2^-24.  The budget
beta of a gather is therefore the oracle run with circ_xcorr replaced by the constant ||a||_2 ||b||_2 at every lag,
carried through the same sums over sub-windows, division by nwin, roll and concatenation.  Then, per side of a gather,
with c the unnormalised float64 row and b its budget:

  norm      y = c / ||c||_2.  dy = dc / ||c|| - c (c . dc) / ||c||^3 and |c . dc| <= b ||c||_1, so to first order
            |dy_k| <= (b / ||c||_2) (1 + |y_k| ||c||_1 / ||c||_2).
  norm_amp  z = y / m, m = y[pivot row][k*] that row's maximum.  dz = dy / m - z dm / m, so
            |dz_k| <= b_y[k] / |m| + |z_k| b_y[pivot row][k*] / |m|.
  two sides rows whose other side has a non-zero norm are the mean of the two sides, and so is their budget; the other
            rows keep the forward side's.
  stack     the weighted sum of the passes' budgets with the stack's weights; the float32 accumulation adds
            u sum_p weight_p |ref_p|, returned apart because it does not scale with the transform.
  raw       (neither norm nor norm_amp: the kernels scale by 1 / ||window||_F^2 in float32) the oracle's own division
            by ||data||_F is already in beta; the float32 scale adds 2u |ref|.

The assertion (assert_within_budget), for every finite reference entry:

  |got - ref| <= C u log2(nfft) beta + u |ref| (+ the stack / raw terms above)

Entries whose reference is not finite keep the pattern equality of golden_io.gather_rel_err; entries whose budget is
exactly 0 (a zero pivot or receiver slice, a row side without a sub-window) must be exactly 0; no finite entry is left
without a budget, which is asserted by counting.  C for a (transform length, flag set) is 16 times the worst ratio
|err| / (u log2(nfft) beta) of the float32 restatement below, recorded in golden/vsg_budget_calibration.json by
tools/measure_vsg_budget.py.  It is measured against the restatement, never against the kernels: the 16 covers the
kernels' twiddle powers formed as products of two table values (up to three roundings where pocketfft has one), the
longer dependent chains of the radix-10 and radix-16 butterflies and the float32 scale after the transform.

The restatement (restated_f32_gather) is the oracle with circ_xcorr replaced by a float32 correlation of float32
inputs through scipy.fft (which keeps single precision; the spectrum dtype is asserted): rfft / irfft of length w where
the engine's transform is exact (nfft == w), else zero-padded fft / ifft of length nfft whose linear correlation is
wrapped to the circular one, out[k] = lin[k] + (lin[k - w] if k > 0 else 0), as a padded engine does.
"""
import contextlib
import json
import os

import numpy as np

from oracle import vsg as ovsg
from tests import golden_io as gio

U = 2.0 ** -24
SAFETY = 16.0
CALIBRATION = os.path.join(gio.GOLDEN, "vsg_budget_calibration.json")
_GEO = ("pivot", "start_x", "end_x", "wlen", "time_window_to_xcorr", "delta_t")


def flag_name(flags):
    """Flag set of the calibration file: 'norm' (with or without norm_amp), 'raw' (neither), else norm_amp alone,
    'two_sided' or 'one_sided'."""
    if flags.get("norm", True):
        return "norm"
    if not flags.get("norm_amp", True):
        return "raw"
    return "two_sided" if flags.get("include_other_side", False) else "one_sided"


@contextlib.contextmanager
def substituted(fn):
    """oracle.vsg.circ_xcorr replaced by fn inside the block."""
    saved = ovsg.circ_xcorr
    ovsg.circ_xcorr = fn
    try:
        yield
    finally:
        ovsg.circ_xcorr = saved


def norm_product(a, b):
    """||a||_2 ||b||_2 at every lag, broadcast as circ_xcorr broadcasts."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p = np.linalg.norm(a, axis=-1, keepdims=True) * np.linalg.norm(b, axis=-1, keepdims=True)
    return np.broadcast_to(p, np.broadcast_shapes(a.shape, b.shape)).copy()


def circ_xcorr_f32(nfft, mutate=None):
    """float32 circ_xcorr at transform length nfft.  mutate(fa, fb) -> (fa, fb), if given, edits the two spectra
    (the host tests' mutants)."""
    import scipy.fft as sfft

    def f(a, b):
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        w = a.shape[-1]
        exact = nfft == w
        assert exact or nfft >= 2 * w - 1, (nfft, w)
        fa, fb = (sfft.rfft(a), sfft.rfft(b)) if exact else (sfft.fft(a, n=nfft), sfft.fft(b, n=nfft))
        assert fa.dtype == np.complex64 and fb.dtype == np.complex64, (fa.dtype, fb.dtype)
        if mutate is not None:
            fa, fb = mutate(fa, fb)
        prod = fa * np.conj(fb)
        assert prod.dtype == np.complex64
        if exact:
            out = sfft.irfft(prod, n=w)
        else:
            lin = sfft.ifft(prod).real
            out = lin[..., :w].copy()
            out[..., 1:] += lin[..., nfft - w + 1:]
        assert out.dtype == np.float32
        return out

    return f


def _side(win, other_side, kw):
    geo = {k: kw[k] for k in _GEO if k in kw}
    with np.errstate(all="ignore"):
        return ovsg.shot_gather(win, norm=False, norm_amp=False, other_side=other_side, **geo)[0]


def _side_budget(win, other_side, kw):
    """Budget of one side of a gather under kw's norm / norm_amp."""
    c = _side(win, other_side, kw)
    with substituted(norm_product):
        b = _side(win, other_side, kw)
    x = win["x_axis"]
    prow = int(np.argmax(x >= kw["pivot"])) - int(np.argmax(x >= kw["start_x"]))
    with np.errstate(all="ignore"):
        if kw.get("norm", True):
            n2 = np.linalg.norm(c, axis=-1, keepdims=True)
            n1 = np.abs(c).sum(axis=-1, keepdims=True)
            c = c / n2
            b = (b / n2) * (1.0 + np.abs(c) * n1 / n2)
        if kw.get("norm_amp", True):
            k = int(np.argmax(c[prow])) if np.isfinite(c[prow]).all() else 0
            m = np.amax(c[prow])
            bm = b[prow, k]
            c = c / m
            b = b / np.abs(m) + np.abs(c) * bm / np.abs(m)
    return c, b


def budget_gather(win, **kw):
    """(ref, beta) of one pass: the oracle's gather and its per-lag budget, both [R, w] float64.  kw as for
    oracle.vsg.virtual_shot_gather."""
    with np.errstate(all="ignore"):
        ref = ovsg.virtual_shot_gather(win, **kw)[0]
        _, beta = _side_budget(win, False, kw)
        if kw.get("include_other_side", False):
            other, bo = _side_budget(win, True, kw)
            ok = np.linalg.norm(other, axis=-1) > 0
            beta = beta.copy()
            beta[ok] = (beta[ok] + bo[ok]) / 2
    return ref, beta


def restated_f32_gather(win, nfft, mutate=None, **kw):
    """The oracle's gather with every correlation in float32 at transform length nfft."""
    with substituted(circ_xcorr_f32(nfft, mutate)), np.errstate(all="ignore"):
        return ovsg.virtual_shot_gather(win, **kw)[0]


def stack_budget(refs, betas, weights=None):
    """(ref, beta, extra) of the weighted sum of gathers (default: their mean, oracle.vsg.stack)."""
    n = len(refs)
    weights = [1.0 / n] * n if weights is None else weights
    with np.errstate(all="ignore"):
        ref = sum(w * r for w, r in zip(weights, refs))
        beta = sum(w * b for w, b in zip(weights, betas))
        extra = U * sum(w * np.abs(r) for w, r in zip(weights, refs))
    return ref, beta, extra


def budget_stack(wins, slots, n_slot, **kw):
    """[(ref, beta, extra)] per class slot: class means of the passes' gathers as StackSchedule weights them."""
    slots = np.asarray(slots)
    per = [budget_gather(w, **kw) for w in wins]
    out = []
    for s in range(n_slot):
        idx = np.flatnonzero(slots == s)
        out.append(stack_budget([per[i][0] for i in idx], [per[i][1] for i in idx]))
    return out


_calibration = {}


def calibration():
    if not _calibration:
        with open(CALIBRATION) as f:
            _calibration.update(json.load(f))
    return _calibration


def constant(nfft, flags):
    """C of a (transform length, flag set): 16 x the restatement's recorded worst ratio."""
    return SAFETY * calibration()["ratio"][str(nfft)][flag_name(flags)]


def budget_ratio(got, ref, beta, nfft, flags, extra=0.0, slack=True):
    """(worst (|got - ref| - u |ref| - extra) / (u log2(nfft) beta) over the finite reference entries with a positive
    budget, number of finite reference entries without a budget); slack=False: the plain |got - ref| / (...) in which
    the restatement is calibrated.  Asserts the patterns of the non-finite entries and
    the exact zeros where the budget is 0."""
    got, ref, beta = (np.asarray(a, np.float64) for a in (got, ref, beta))
    assert got.shape == ref.shape == beta.shape, (got.shape, ref.shape, beta.shape)
    gio.gather_rel_err(got, ref)  # NaN / inf patterns
    fin = np.isfinite(ref)
    has = fin & np.isfinite(beta) & (beta >= 0)
    unbudgeted = int(fin.sum() - has.sum())
    zero = has & (beta == 0)
    assert (got[zero] == 0).all() and (ref[zero] == 0).all(), "entries with a zero budget must be exactly 0"
    pos = has & (beta > 0)
    if not pos.any():
        return 0.0, unbudgeted
    allow = U * np.abs(ref) + extra
    if flag_name(flags) == "raw":
        allow = allow + 2 * U * np.abs(ref)
    if not slack:
        allow = 0.0 * allow
    with np.errstate(all="ignore"):
        over = (np.abs(got - ref) - allow)[pos] / (U * np.log2(nfft) * beta[pos])
    return float(max(over.max(), 0.0)), unbudgeted


def assert_within_budget(tag, got, ref, beta, nfft, flags, extra=0.0, w=None):
    """The budget rule with C = constant(nfft, flags); prints the worst ratio in units of u log2(nfft) beta."""
    ratio, unbudgeted = budget_ratio(got, ref, beta, nfft, flags, extra)
    c = constant(nfft, flags)
    w = ref.shape[-1] if w is None else w
    print(f"VSGBUDGET w={w} nfft={nfft} flags={flag_name(flags)} ratio={ratio:.4f} C={c:.4f} [{tag}]")
    assert unbudgeted == 0, (tag, unbudgeted)
    assert ratio <= c, (tag, ratio, c)
    return ratio


# --- the calibration sweep (tools/measure_vsg_budget.py writes it, test_vsg_budget_host.py holds the helper to it) ---

EXTRA_CASES = [(2, "W499", 499, 1024), (2, "W500", 500, 500)]  # the production lengths, as rows of the lengths table
MULTS = (1, 2, 3)


def lengths_cases():
    """Every (wlen, clock, w, transform length) of the lengths test's table, plus w = 499 and 500."""
    from tests import test_vsg_lengths_gpu as lengths
    return list(lengths.TABLE) + EXTRA_CASES


def lengths_window(clock, i):
    """Oracle window of pass i of the lengths test's geometry."""
    from tests import test_vsg_lengths_gpu as lengths
    p = lengths._passes(clock)[i]
    return dict(data=p["host"], x_axis=p["x_axis"], t_axis=p["t_axis"], veh_state_x=p["veh_state_x"],
                veh_state_t=p["veh_state_t"])


def restatement_ratio(case, flags, mult, i):
    """(ratio, unbudgeted finite entries) of the float32 restatement at one pass of one calibration case."""
    from tests import test_vsg_lengths_gpu as lengths
    win, kw = lengths_window(case[1], i), lengths._kw(case, flags, mult)
    ref, beta = budget_gather(win, **kw)
    return budget_ratio(restated_f32_gather(win, case[3], **kw), ref, beta, case[3], flags, slack=False)
