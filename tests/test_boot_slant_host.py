"""Bootstrap on the phase-shift transform, host side (no GPU): the refusals of the new keywords, which come before any
device work, and the dvh_slant_ridge prototype against its ctypes binding."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = [25, 50], 700, 500, 900, [80, 130], [2.5, 10], [14, 15], [None, None]


class _NoDevice:
    """Stands where the windows go: any use of it is device work that should not have begun."""

    def __len__(self):
        raise AssertionError("the windows were touched before the keyword was refused")

    __iter__ = __getitem__ = __len__


def test_unknown_transform_raises_before_device_work():
    from das_diff_veh_amd.apis.imaging_classes import bootstrap_disp, convergence_test, save_disp_imgs
    wins = _NoDevice()
    with pytest.raises(ValueError, match="transform"):
        bootstrap_disp(wins, 3, 4, *ARGS, transform="bogus")
    with pytest.raises(ValueError, match="transform"):
        convergence_test(3, wins, 4, *ARGS, transform="bogus")
    with pytest.raises(ValueError, match="transform"):
        save_disp_imgs(wins, "heavy", 2, 700, 500, 900, 150, "figs", transform="bogus")


def test_fused_walk_needs_the_slant_transform():
    from das_diff_veh_amd import bootstrap as bt
    from das_diff_veh_amd.apis.imaging_classes import bootstrap_disp, convergence_test
    wins = _NoDevice()
    with pytest.raises(ValueError, match="walk"):
        bootstrap_disp(wins, 3, 4, *ARGS, transform="fk", walk="fused")
    with pytest.raises(ValueError, match="walk"):
        bootstrap_disp(wins, 3, 4, *ARGS, walk="fused")           # transform defaults to "fk"
    with pytest.raises(ValueError, match="walk"):
        convergence_test(3, wins, 4, *ARGS, transform="fk", walk="fused")
    with pytest.raises(ValueError, match="walk"):
        bootstrap_disp(wins, 3, 4, *ARGS, transform="slant", walk="bogus")
    with pytest.raises(ValueError, match="walk"):
        bt.bootstrap_ridges(None, None, *ARGS[:1], *ARGS[4:], transform="fk", walk="fused")
    with pytest.raises(ValueError, match="walk"):
        bt.convergence(None, 3, 4, *ARGS[:1], *ARGS[4:], transform="fk", walk="fused")
    assert bt.check_transform("fk") == bt.check_transform("fk", "image") == bt.check_transform("slant", "image") == "image"
    assert bt.check_transform("slant", "fused") == "fused"
    assert bt.check_transform("slant") == bt.SLANT_WALK and bt.SLANT_WALK in ("fused", "image")


def test_slant_ridge_binding_matches_header():
    """dvh_slant_ridge as include/dvh.h declares it against das_diff_veh_amd._lib.SIGNATURES: argument count and,
    argument by argument, pointer / int32 / float64."""
    from das_diff_veh_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvh.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"\bint\s+dvh_slant_ridge\s*\(([^()]*)\)\s*;", hdr)
    assert m, "include/dvh.h does not declare dvh_slant_ridge"
    params = [p.strip() for p in m.group(1).split(",")]
    bound = _lib.SIGNATURES["dvh_slant_ridge"]
    assert len(params) == len(bound) == 22
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for p, b in zip(params, bound):
        want = ctypes.c_void_p if "*" in p else kinds[p.split()[0]]
        assert b is want, (p, b)
    # the arguments of dvh_disp_slant's spectra and of dvh_ridge's walk, by name
    names = [re.sub(r"[\s*]+", " ", p).split()[-1] for p in params]
    assert names == ["D", "B", "n_row", "n_fb", "fb", "freqs", "nF", "dx", "c0", "nb", "vel", "nV", "ref", "sigma",
                     "vel_max", "vref", "sg", "sgl", "out", "status", "picks", "stream"]


def test_slant_ridge_refusals_need_no_gpu():
    """The argument checks return before any device work (the GPU test repeats them with live buffers)."""
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    lib = _lib.load()
    P = ctypes.c_void_p
    a = dict(D=P(0x10000), B=1, n_row=19, n_fb=8, fb=P(0x20000), freqs=P(0x30000), nF=40, dx=8.16, c0=3, nb=26,
             vel=P(0x40000), nV=100, ref=5, sigma=25.0, vel_max=800.0, vref=None, sg=P(0x50000), sgl=25,
             out=P(0x60000), status=P(0x70000), picks=None, stream=None)
    cases = [(dict(D=None), -2), (dict(fb=None), -2), (dict(freqs=None), -2), (dict(vel=None), -2),
             (dict(out=None), -2), (dict(status=None), -2), (dict(B=-1), -2), (dict(n_row=-1), -2), (dict(nF=-1), -2),
             (dict(nV=-1), -2), (dict(n_fb=0), -2), (dict(nb=0), -2), (dict(c0=-1), -2), (dict(c0=15), -2),
             (dict(ref=26), -2), (dict(ref=-27), -2), (dict(sgl=24), -4), (dict(sgl=27), -4), (dict(sg=None), -4),
             (dict(nb=1025, nF=2000), -4), (dict(n_row=1025), -4)]
    for over, want in cases:
        assert lib.dvh_slant_ridge(*{**a, **over}.values()) == want, over
        assert lib.dvh_last_error()
    assert lib.dvh_slant_ridge(*{**a, "B": 0}.values()) == 0
