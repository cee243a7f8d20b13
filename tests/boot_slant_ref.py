"""Float64 side of the phase-shift bootstrap tests (tests/test_boot_slant_gpu.py): the oracle chain
recorded gathers -> oracle.vsg.stack -> tests/slant_ref.slant, the derived end-to-end bound, and the audit of a ridge
walk's steps against the float64 image."""
import numpy as np

from tests import slant_ref

DX = 8.16


def oracle_image(gathers, s, e, dt, freqs, vels):
    """(stack rows [s, e], their phase-shift image with rows in descending velocity) of the float64 gathers of one
    draw: sum(images) / len(images), then map_fv_FD_slant_stack over all rows of the slice."""
    from oracle import vsg as ovsg
    stack = ovsg.stack(list(gathers))[s:e + 1]
    vel_desc = np.sort(np.asarray(vels, dtype=np.float64))[::-1]
    return stack, slant_ref.slant(stack, DX, dt, freqs, vel_desc, norm=False, rows=(0, stack.shape[0]))


def end_to_end_bound(stack):
    """The largest absolute difference the device image may show against oracle_image's, derived: every element of
    the device stack lies within 1e-4 max|stack| of the oracle's (the per-gather contract of the vsg tests; the stack
    adds and divides elementwise), the time DFT and the steering sum are linear with unit-modulus factors, so an
    image value moves by at most that times nt samples times n_row rows."""
    n_row, nt = stack.shape
    return 1e-4 * np.abs(stack).max() * nt * n_row


def audit_walk(dev_picks, ref_band, vels, sigma, tol, ref_idx=None, vref=None):
    """Every step of a device walk (its raw picks over the band) against the float64 image ``ref_band`` [nV, nb]
    (rows in descending velocity): the pick lies inside the window the device's own walk used -- all rows at the
    reference column, (v_prev - sigma, v_prev + sigma) around its previous pick after that, or the vref band -- and
    the reference image there is within ``tol`` of the reference maximum over that window.  ref_idx >= 0 (the
    backward, then the forward walk) or vref [nb].  Returns (steps audited, steps whose pick is not the reference's
    argmax of the window, largest shortfall)."""
    vel = np.sort(np.asarray(vels, dtype=np.float64))[::-1]
    nb = len(dev_picks)
    if vref is not None:
        order = list(range(nb))
    else:
        assert 0 <= ref_idx < nb
        order = [ref_idx] + list(range(ref_idx - 1, -1, -1)) + list(range(ref_idx + 1, nb))
    other, worst = 0, 0.0
    for i in order:
        if vref is not None:
            mask = (vel > vref[i] - sigma) & (vel < vref[i] + sigma)
        elif i == ref_idx:
            mask = np.ones(vel.shape, dtype=bool)
        else:
            prev = dev_picks[i + 1] if i < ref_idx else dev_picks[i - 1]
            mask = (vel > prev - sigma) & (vel < prev + sigma)
        hit = np.flatnonzero(vel == dev_picks[i])
        assert hit.size == 1, (i, dev_picks[i], "the pick is no velocity of the axis")
        d = int(hit[0])
        assert mask[d], (i, dev_picks[i], "device pick outside its own window")
        col = ref_band[:, i]
        short = float(col[mask].max() - col[d])
        assert short <= tol, (i, dev_picks[i], short, tol)
        other += int(np.flatnonzero(mask)[np.argmax(col[mask])] != d)
        worst = max(worst, short)
    return len(order), other, worst
