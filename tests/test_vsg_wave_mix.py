"""The block shape of the validated stack launch (dvh_vsg_stack_validated_waves, csrc/dvh_vsg.hip: pick_vstack), host
arithmetic only.  At w = 500 a launch that scans at least 30 000 window bytes per (pass, gather row) it correlates
runs 5 correlation + 3 scan waves per block, any other 7 + 1; the other fused lengths have one shape, the lengths
whose scan is its own launch none.  The return value is 16 x correlation waves + scan waves."""
from das_diff_veh_amd import _lib

W71, W53 = 16 * 7 + 1, 16 * 5 + 3


def _waves(w, n_win, n_ch, n_t, n_pass, R):
    return _lib.load().dvh_vsg_stack_validated_waves(w, n_win, n_ch, n_t, n_pass, R)


def test_bench_geometries():
    """synth10k (2 048 windows of 1 024 x 8 192, 1 023 rows: 32.8 KB per (pass, row)) is held by its scan; weights
    (3 790 windows of 60 x 5 500, 48 rows: 27.5 KB) by its correlation; a one-window scan is no scan to speak of."""
    assert _waves(500, 2048, 1024, 8192, 2048, 1023) == W53
    assert _waves(500, 3790, 60, 5500, 3790, 48) == W71
    assert _waves(500, 1, 1024, 8192, 2048, 1023) == W71


def test_threshold_is_bytes_per_pass_row():
    """4 n_win n_ch n_t >= 30 000 n_pass R, in 64-bit arithmetic; fewer scan windows than passes (unit scans) count
    as fewer bytes."""
    assert _waves(500, 1, 75, 100, 1, 1) == W53      # 30 000 B
    assert _waves(500, 1, 75, 100, 1, 2) == W71
    assert _waves(500, 1, 74, 100, 1, 1) == W71      # 29 600 B
    assert _waves(500, 10, 75, 100, 10, 1) == W53
    assert _waves(500, 9, 75, 100, 10, 1) == W71
    assert _waves(500, 2 ** 20, 2048, 16384, 2 ** 20, 2047) == W53  # 1.4e17 bytes: no 32-bit products
    assert _waves(500, 0, 0, 0, 0, 0) == W53  # an empty launch: either shape launches one idle block


def test_other_lengths():
    for w in (499, 257, 512, 2, 256):
        assert _waves(w, 2048, 1024, 8192, 2048, 1023) == W71
        assert _waves(w, 3790, 60, 5500, 3790, 48) == W71
    for w in (250, 1000, 513, 1024):  # the scan is a launch of its own
        assert _waves(w, 2048, 1024, 8192, 2048, 1023) == 0
    assert _waves(4096, 1, 1, 1, 1, 1) == 0  # no engine
