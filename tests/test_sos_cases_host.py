"""The case table of the sosfiltfilt section-count tests (tests/sos_cases.py) on the host: every design has the
section count, padlen and pole radius the GPU tests rely on, SciPy accepts and refuses the shortest records where
the table says, and the record lengths of the scan-regime test give the block counts and the scan kernels they are
meant to reach."""
import numpy as np
import pytest
import scipy.signal

from das_diff_veh_amd.preprocess import SOS_MFMA_MAX_POLE, _padlen
from tests import sos_cases as sc


@pytest.mark.parametrize("name", sc.DESIGNS)
def test_design_sections_padlen_and_poles(name):
    sos = sc.design(name)
    n_sec, padlen = sc.EXPECTED[name]
    assert sos.shape == (n_sec, 6) and 1 <= n_sec <= 16
    assert _padlen(sos) == padlen
    # a first-order factor: one b2 = 0 and one a2 = 0 (SciPy's pairing may put them in different sections)
    first_order = min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    assert first_order == (1 if name in sc.FIRST_ORDER else 0)
    # the matrix form is specified for poles inside DVH_SOS_MFMA_MAX_POLE
    assert sc.MAX_POLE == SOS_MFMA_MAX_POLE == 0.999
    radius = max(np.abs(np.roots(row[3:])).max() for row in sos)
    assert radius < sc.MAX_POLE, (name, radius)  # the largest, bp16's, is 0.99726


@pytest.mark.parametrize("name", sc.DESIGNS)
def test_padlen_is_scipys(name):
    """scipy.signal.sosfiltfilt refuses padlen samples with its padlen message and takes padlen + 1."""
    sos = sc.design(name)
    padlen = sc.EXPECTED[name][1]
    x = sc.record(name, 2, padlen + 1)
    with pytest.raises(ValueError, match=f"must be greater than padlen, which is {padlen}"):
        scipy.signal.sosfiltfilt(sos, x[:, :padlen], axis=1)
    assert scipy.signal.sosfiltfilt(sos, x, axis=1).shape == x.shape


def test_bandpass_designs_cover_every_section_count():
    assert sorted(sc.EXPECTED[n][0] for n in sc.BANDPASS) == list(range(1, 17))
    assert [sc.EXPECTED[n] for n in sc.FIRST_ORDER] == [(3, 18), (2, 12), (1, 6)]


def test_scan_limits():
    """The three dispatch limits of sosm_scan in block counts."""
    assert (sc.K_SM_L, sc.K_SCAN_MG, sc.K_SCAN_MQ, sc.K_SCAN_CAP) == (64, 16, 16, 4800)
    for n_sec in (1, 3, 9, 16):
        assert [sc.scan_kernel(nb, n_sec) for nb in (1, 2, 3, 18, 19, 258)] == ["none"] * 2 + ["matrix"] * 4
        assert sc.scan_kernel(259, n_sec) == ("staged" if n_sec == 16 else "resident")
    # group length of the matrix-pipe scan: 1 up to 18 blocks, 2 from 19, 16 at 258
    q16 = lambda nb: -(-(nb - 2) // sc.K_SCAN_MG)
    assert (q16(3), q16(18), q16(19), q16(258), q16(259)) == (1, 1, 2, 16, 17)
    assert [sc.last_resident_nb(n) for n in (1, 3, 9, 16)] == [2401, 801, 267, 151]
    for n_sec in (1, 3, 9):
        last = sc.last_resident_nb(n_sec)
        assert sc.scan_kernel(last, n_sec) == "resident" and sc.scan_kernel(last + 1, n_sec) == "staged"


def test_scan_block_counts_per_design():
    got = {name: [nb for nb, _ in sc.scan_block_counts(name)] for name in sc.SCAN_DESIGNS}
    assert got == {
        "bp1": [1, 2, 3, 18, 19, 258, 259, 2401, 2402],   # padlen 9
        "bp3": [1, 2, 3, 18, 19, 258, 259, 801, 802],     # padlen 21: 3 padlen = 63 < 64
        "bp9": [3, 18, 19, 258, 259, 267, 268],           # padlen 57: 172 samples at the least
        "bp16": [5, 18, 19, 258, 259],                    # padlen 99: 298 samples at the least; 259 is staged
        "lp5": [1, 2, 3, 18, 19, 258, 259, 801, 802],     # padlen 18
    }
    kernels = {name: {k for _, k in sc.scan_block_counts(name)} for name in sc.SCAN_DESIGNS}
    assert kernels["bp16"] == {"matrix", "staged"}
    assert kernels["bp9"] == {"matrix", "resident", "staged"}
    for name in ("bp1", "bp3", "lp5"):
        assert kernels[name] == {"none", "matrix", "resident", "staged"}


@pytest.mark.parametrize("cases", [sc.scan_cases, sc.scan_cases_f32])
def test_scan_record_lengths_give_their_block_counts(cases):
    seen = {}
    for name, nb, n_t in cases():
        n_sec, padlen = sc.EXPECTED[name]
        assert n_t > padlen
        assert sc.n_blocks(n_t, padlen) == nb, (name, nb, n_t)
        seen.setdefault((name, nb), []).append(n_t + 2 * padlen - sc.K_SM_L * (nb - 1))  # samples of the last block
    for (name, nb), tails in seen.items():
        padlen = sc.EXPECTED[name][1]
        assert tails[0] == sc.K_SM_L or nb == 1, (name, nb)  # last block full
        if sc.K_SM_L * (nb - 1) - 2 * padlen + 1 > padlen:
            assert tails == [sc.K_SM_L, 1], (name, nb)        # and holding one sample
    if cases is sc.scan_cases:
        assert max(n_t for _, _, n_t in cases()) == 64 * 2402 - 18 == 153710
        assert {(n, nb) for n, nb, _ in cases()} == {(n, nb) for n in sc.SCAN_DESIGNS
                                                     for nb, _ in sc.scan_block_counts(n)}
    else:
        assert {(n, nb) for n, nb, _ in cases()} == {
            ("bp1", 3), ("bp1", 259), ("bp3", 3), ("bp3", 259), ("bp3", 802), ("bp9", 3), ("bp9", 259),
            ("bp16", 5), ("bp16", 259), ("lp5", 3), ("lp5", 259), ("lp5", 802)}
