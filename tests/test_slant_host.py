"""Phase-shift dispersion, host side (no GPU): tests/slant_ref against the reference's recorded outputs
(tests/golden/slant.npz), the fixture's own conditions, the host arithmetic of das_diff_veh_amd.disp.SlantPlan against the
fixture's recorded values, the three frequency-bin rules, and the argument checks of dvh_disp_slant, which return before
any device work.

Tolerance: slant_ref and the reference evaluate the same float64 sum, slant_ref with the DFT as a direct sum and the
steering powers by recurrence: 1e-12 of the image maximum (measured: 1.2e-15), the margin of the f-k host pins.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import golden_io as gio
from tests import slant_ref

from tests.slant_ref import CASES, case


def rel_err(got, want):
    """gather_rel_err, NaN and inf patterns included."""
    return gio.gather_rel_err(got, want)


@pytest.mark.parametrize("name", CASES)
def test_slant_ref_reproduces_reference(name):
    g = gio.load("slant")
    data, dx, dt, freqs, vels, norm = case(g, name)
    want = g[f"{name}_out"]
    got = slant_ref.slant(data, dx, dt, freqs, vels, norm=norm)
    assert got.dtype == np.float64 and got.shape == want.shape == (vels.size, freqs.size)
    err = rel_err(got, want)
    print(f"case {name}: {err:.3g} of the image maximum")
    assert err <= 1e-12
    if name == "F":
        assert not want.any() and not g["F_out_plain"].any()
        assert not slant_ref.slant(data, dx, dt, freqs, vels, norm=False).any()
    if name == "G":
        assert np.isnan(want).all()
    if name == "C":     # one row: |D[0, f]| whatever the velocity, negative ones included
        assert np.array_equal(want[0], want[1]) and np.array_equal(want[0], want[2])


def test_fixture_conditions():
    """(a) the terms of the steering sum exceed the image maximum by at most 8: the factor behind the derived bound of
    the GPU test; (b) at most 10 % of the columns have a runner-up within 2e-6 of the maximum (one-row gathers tie in
    every column and are exempt).  Recomputed here from the recorded outputs."""
    g = gio.load("slant")
    for name in "ABCDE":
        data, dx, dt, freqs, vels, norm = case(g, name)
        ratio = slant_ref.coherence_ratio(data, dt, freqs, g[f"{name}_out"], norm=norm)
        ties = slant_ref.near_tie_fraction(g[f"{name}_out"])
        print(name, ratio, ties)
        assert abs(ratio - g[f"{name}_ratio"]) <= 1e-9 * ratio and ratio <= 8
        assert ties == g[f"{name}_ties"] and (ties <= 0.1 or name == "C")
    assert np.isnan(g["F_ratio"]) and np.isnan(g["G_ratio"])


def test_velocity_zero_raises():
    """The reference's ValueError for a velocity of 0, from the plan (before any device work) as from the restatement."""
    from das_diff_veh_amd.disp import SlantPlan
    with pytest.raises(ValueError, match="math domain error"):
        SlantPlan(25, 64, 8.16, 0.004, [5.0], [300.0, 0.0])
    with pytest.raises(ValueError, match="math domain error"):
        slant_ref.slant(np.ones((25, 64)), 8.16, 0.004, [5.0], [300.0, 0.0])


@pytest.mark.parametrize("name", CASES)
def test_slant_plan_matches_fixture(name):
    from das_diff_veh_amd.disp import SlantPlan
    g = gio.load("slant")
    data, dx, dt, freqs, vels, _ = case(g, name)
    p = SlantPlan(data.shape[0], data.shape[1], dx, dt, freqs, vels)
    assert p.nf == int(g[f"{name}_nf"]) == slant_ref.sizes(data.shape[1])
    assert np.array_equal(p.fidx, g[f"{name}_fidx"]) and np.array_equal(p.bins, g[f"{name}_bins"])
    assert (p.row0, p.n_row) == tuple(g[f"{name}_rows"])
    assert p.fb.dtype == np.int32 and np.array_equal(p.bins[p.fb], p.fidx) and p.n_fb == p.bins.size
    assert p.freqs.dtype == p.vels.dtype == np.float64 and np.array_equal(p.vels, vels)     # the caller's order
    # twiddles: bin nu of the nf-point DFT, cos | -sin interleaved, the angle reduced mod nf before the division
    t = np.arange(p.nt)
    ang = 2.0 * np.pi * ((np.outer(t, p.bins) % p.nf) / p.nf)
    assert p.wt.shape == (p.nt, 2 * p.n_fb)
    assert np.array_equal(p.wt[:, 0::2], np.cos(ang)) and np.array_equal(p.wt[:, 1::2], -np.sin(ang))


def test_slant_plan_rows_and_velocities():
    from das_diff_veh_amd.disp import SlantPlan
    kw = dict(nt=64, dx=8.16, dt=0.004, freqs=[5.0], vels=[300.0])
    for nch, rows, want in ((25, (6, 25), (6, 19)), (40, (6, 25), (6, 19)), (20, (6, 25), (6, 14)), (7, (6, 25), (6, 1)),
                            (6, (6, 25), (6, 0)), (5, (6, 25), (5, 0)), (49, (0, 49), (0, 49)), (25, (24, 25), (24, 1)),
                            (25, (10, 4), (10, 0))):
        p = SlantPlan(nch=nch, rows=rows, **kw)
        assert (p.row0, p.n_row) == want, (nch, rows)
    for bad in (0.0, -0.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="math domain error"):
            SlantPlan(25, 64, 8.16, 0.004, [5.0], [300.0, bad])
    assert SlantPlan(25, 64, 8.16, 0.004, [5.0], [-300.0]).vels[0] == -300.0


def test_bin_rules():
    """dt = 2**-8 makes every bin frequency exact (nt = 257: nf = 1 024, bins 0.25 Hz apart, Nyquist 128 Hz): a frequency
    exactly halfway between two bins takes the lower bin (the first minimum), one above Nyquist takes bin nf/2 - 1 (the
    largest positive frequency), a negative one a negative-frequency bin (index nf - k).  Case D of the fixture holds
    the same three at dt = 0.004."""
    from das_diff_veh_amd.disp import SlantPlan
    freqs = [1.625, 1.5, 1.75, 1.62, 1.63, 500.0, 128.0, 127.9, -5.0, -5.125, -127.9, -1000.0, 0.0]
    want = [6, 6, 7, 6, 7, 511, 511, 511, 1024 - 20, 1024 - 21, 512, 512, 0]
    p = SlantPlan(25, 257, 8.16, 2.0 ** -8, freqs, [300.0])
    assert p.nf == 1024 and p.fidx.tolist() == want
    assert slant_ref.bins(257, 2.0 ** -8, freqs)[1].tolist() == want
    g = gio.load("slant")
    fidx, freqs = g["D_fidx"], g["D_freqs"]
    assert freqs[-1] == 1.5869140625 and fidx[-1] == 6             # 6.5 bins of 1 / (1024 * 0.004) Hz
    assert freqs[0] == -5.0 and fidx[0] == 1024 - 20                 # -5 Hz: 20.48 bins below zero
    assert freqs[20] == 140.0 and fidx[20] == 511                    # above the 125 Hz Nyquist


def test_slant_argument_checks_need_no_gpu():
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    lib = _lib.load()
    P = ctypes.c_void_p
    D, fb, fr, ve, fv = P(0x10000), P(0x20000), P(0x30000), P(0x40000), P(0x50000)

    def call(D=D, B=1, nch=25, n_fb=4, row0=6, n_row=19, fb=fb, nF=3, nV=2, stride=6):
        return lib.dvh_disp_slant(D, B, nch, n_fb, row0, n_row, fb, fr, nF, ve, nV, 8.16, fv, stride, None)
    for kw, msg in ((dict(D=None), b"null"), (dict(fb=None), b"null"), (dict(B=-1), b"negative"),
                    (dict(n_row=-1), b"negative"), (dict(row0=-1), b"negative"), (dict(nF=-1), b"negative"),
                    (dict(row0=7), b"leave the gather"), (dict(nch=24), b"leave the gather"),
                    (dict(row0=2 ** 31 - 1, n_row=19), b"leave the gather"), (dict(n_fb=0), b"n_fb"),
                    (dict(B=2, stride=5), b"overlap")):
        assert call(**kw) == -2, kw
        assert msg in lib.dvh_last_error(), (kw, lib.dvh_last_error())
    assert call(B=0) == 0 and call(nF=0) == 0 and call(nV=0) == 0      # nothing to do: no launch
    assert lib.dvh_abi_version() == 2
