"""dvh_sosfiltfilt (the block recursion) and dvh_sosfiltfilt_plan / dvh_sosfiltfilt_planned (the matrix-pipe form)
through the C ABI at every section count 1-16, in float64 and float32, with first-order sections, at the shortest
records, at every scan the matrix form dispatches to, and on strided rows; designs and record lengths from
tests/sos_cases.py (pinned on the host by tests/test_sos_cases_host.py).  The reference is scipy.signal.sosfiltfilt
on the float64 copy of the uploaded rows; the tolerances are those of tests/test_prep_gpu.py: 1e-10 of the output's
maximum in float64, 2e-6 in float32.  (SciPy itself is within 1e-13 of an 80-bit restatement of the recursion for
every design here.)"""
import numpy as np
import pytest
import scipy.signal

from tests import sos_cases as sc

pytestmark = pytest.mark.gpu
TOL = {np.float64: 1e-10, np.float32: 2e-6}
FORMS = ["recursion", "matrix"]
DTYPES = [np.float64, np.float32]

_REFS = {}


def _case(name, n_rows, n_t, dtype):
    """(host rows in dtype, scipy's output of their float64 copy), computed once per (design, shape, dtype)."""
    key = (name, n_rows, n_t, np.dtype(dtype).name)
    if key not in _REFS:
        host = sc.record(name, n_rows, n_t, dtype)
        ref = scipy.signal.sosfiltfilt(sc.design(name), host.astype(np.float64), axis=1)
        host.setflags(write=False)
        ref.setflags(write=False)
        if host.nbytes > (8 << 20):  # the one large record is used once
            return host, ref
        _REFS[key] = (host, ref)
    return _REFS[key]


def _check(got, ref, dtype, label):
    assert got.dtype == dtype and got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"SOSERR {label} {np.dtype(dtype).name} {err:.3e}")
    assert err <= TOL[dtype], label


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sc.DESIGNS)
def test_every_section_count(device, name, form, dtype):
    """The 16 band-passes (1-16 sections) and the three designs with a first-order section (their input offset by
    100: the zi x[0] start state and the odd extension at work), 19 rows x 700 samples: the last 16-column tile of
    the matrix form is partial and spans rows."""
    host, ref = _case(name, 19, 700, dtype)
    got = sc.run_filtfilt(device, sc.design(name), host, form)
    _check(got, ref, dtype, f"{name} {form}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sc.DESIGNS)
def test_shortest_record(device, name, form):
    """n_t = padlen + 1 is filtered; n_t = padlen is refused with code -4 (which _lib.call raises as ValueError, with
    SciPy's message) and the rows are left as they were."""
    import torch

    from das_diff_veh_amd import _lib
    sos = sc.design(name)
    padlen = sc.EXPECTED[name][1]
    host, ref = _case(name, 5, padlen + 1, np.float64)
    got = sc.run_filtfilt(device, sos, host, form)
    _check(got, ref, np.float64, f"{name} {form} shortest")
    short = np.ascontiguousarray(host[:, :padlen])
    with pytest.raises(ValueError, match="must be greater than padlen"):
        sc.run_filtfilt(device, sos, short, form)
    # the return code itself, and the buffer after the refused call
    dev = torch.from_numpy(short.copy()).to(device)
    sos_t = torch.from_numpy(np.ascontiguousarray(sos)).to(device)
    zi_t = torch.from_numpy(np.ascontiguousarray(scipy.signal.sosfilt_zi(sos))).to(device)
    work = torch.empty(1 << 16, dtype=torch.float64, device=device)
    plan = torch.zeros(int(_lib.load().dvh_sosfiltfilt_plan_bytes(len(sos))) // 8, dtype=torch.float64, device=device)
    args = (_lib.ptr(dev), 1, 5, dev.stride(0), padlen, _lib.ptr(sos_t), len(sos), padlen, _lib.ptr(zi_t))
    if form == "recursion":
        rc = _lib.load().dvh_sosfiltfilt(*args, _lib.ptr(work), _lib.stream_of(device))
    else:
        rc = _lib.load().dvh_sosfiltfilt_planned(*args, _lib.ptr(plan), _lib.ptr(work), _lib.stream_of(device))
    assert rc == -4
    assert np.array_equal(dev.cpu().numpy(), short)


@pytest.mark.parametrize("name,nb,n_t", sc.scan_cases())
def test_scan_regimes(device, name, nb, n_t):
    """The matrix form at the block counts either side of every scan dispatch limit (no scan, the matrix-pipe scan
    at group lengths 1, 2 and 16, the LDS-resident scan, the staged scan), the last block full and holding one
    sample; float64, 5 rows."""
    host, ref = _case(name, 5, n_t, np.float64)
    got = sc.run_filtfilt(device, sc.design(name), host, "matrix")
    _check(got, ref, np.float64, f"{name} matrix nb={nb} n_t={n_t}")


@pytest.mark.parametrize("name,nb,n_t", sc.scan_cases_f32())
def test_scan_regimes_float32(device, name, nb, n_t):
    host, ref = _case(name, 5, n_t, np.float32)
    got = sc.run_filtfilt(device, sc.design(name), host, "matrix")
    _check(got, ref, np.float32, f"{name} matrix nb={nb} n_t={n_t}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows,n_t", [(45, 130), (1, 700)])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["bp1", "bp16"])
def test_strided_rows(device, name, form, n_rows, n_t, dtype):
    """Rows inside a wider buffer (row stride n_t + 2 x 24) whose view starts one element into the allocation: the
    24 columns either side of the rows, and the leading element, keep their 3.5."""
    pad = 24
    assert n_t > sc.EXPECTED[name][1]
    host, ref = _case(name, n_rows, n_t, dtype)
    buf = sc.run_filtfilt(device, sc.design(name), host, form, pad=pad, lead=1, fill=3.5)
    assert buf.shape == (n_rows, n_t + 2 * pad)
    assert np.all(buf[:, :pad] == 3.5) and np.all(buf[:, pad + n_t:] == 3.5)
    _check(buf[:, pad:pad + n_t], ref, dtype, f"{name} {form} strided {n_rows}x{n_t}")


def test_recursion_blocks_of_64_at_16_sections(device):
    """320 x 28 000 float64 rows: 9.0e6 extended samples, for which sos_block_len (csrc/dvh_sos.hip) takes blocks of
    L = 64 (ceil(9.0e6 / 262 144) = 35, rounded up to a multiple of 32), at the widest state (32 components)."""
    n_rows, n_t = 320, 28000
    n_ext = n_t + 2 * sc.EXPECTED["bp16"][1]
    per_lane = -(-n_rows * n_ext // (256 * 4 * 4 * 64))
    assert per_lane == 35 and -(-per_lane // 32) * 32 == 64
    host, ref = _case("bp16", n_rows, n_t, np.float64)
    got = sc.run_filtfilt(device, sc.design("bp16"), host, "recursion")
    _check(got, ref, np.float64, "bp16 recursion L=64")
