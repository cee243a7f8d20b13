"""Filter designs and record lengths of the sosfiltfilt section-count tests (tests/test_sos_cases_host.py pins the
table's arithmetic on the host, tests/test_sos_sections_gpu.py runs the kernels at it).  dt = 0.004 s throughout.

Designs (name: sections, padlen = 3 (2 n_sec + 1 - min(#b2 == 0, #a2 == 0)), as scipy.signal.sosfiltfilt pads):
  bp1 .. bp16   butter(N, [1.2, 30] 2 dt, 'bandpass'): N sections, padlen 6 N + 3
  lp5           butter(5, 30 2 dt, 'low'):   3 sections with a first-order factor (one b2 = 0, one a2 = 0), padlen 18
  hp3           butter(3, 1.2 2 dt, 'high'): 2 sections with a first-order factor, padlen 12
  lp1           butter(1, 30 2 dt, 'low'):   1 first-order section (b2 = a2 = 0), padlen 6

The matrix-pipe form (csrc/dvh_sosm.hip) cuts the extended row of n_t + 2 padlen samples into nb blocks of kSmL = 64
and finds the blocks' start states by a scan over nb - 1 end states, dispatched by sosm_scan:
  nb <= 2                               no scan (nb == 1: sosm_fa and sosm_bc are not launched either)
  ceil((nb - 2) / kScanMG) <= kScanMQ   sosm_scanm_kernel, the matrix-pipe scan: 16 groups of up to 16 blocks, nb <= 258
  (nb - 1) 2 NS <= kScanCap             sosm_scanr_kernel, the row's states resident in the LDS (4 800 doubles)
  else                                  sosm_scan_kernel, the staged scan
"""
import functools

import numpy as np

DT = 0.004
MAX_POLE = 0.999  # include/dvh.h DVH_SOS_MFMA_MAX_POLE: the matrix form is specified up to this pole radius
# csrc/dvh_sosm.hip
K_SM_L = 64          # kSmL: samples per block
K_SCAN_MG = 16       # kScanMG: groups of the matrix-pipe scan
K_SCAN_MQ = 16       # kScanMQ: its longest group
K_SCAN_CAP = 4800    # kScanCap: doubles of the LDS-resident scan

BANDPASS = [f"bp{n}" for n in range(1, 17)]
FIRST_ORDER = ["lp5", "hp3", "lp1"]  # designs with a section whose b2 = a2 = 0
DESIGNS = BANDPASS + FIRST_ORDER
# name: (sections, padlen)
EXPECTED = {**{f"bp{n}": (n, 6 * n + 3) for n in range(1, 17)}, "lp5": (3, 18), "hp3": (2, 12), "lp1": (1, 6)}
OFFSET = {"lp5": 100.0, "hp3": 100.0, "lp1": 100.0}  # constant added to the input of the first-order designs

SCAN_DESIGNS = ["bp1", "bp3", "bp9", "bp16", "lp5"]


@functools.lru_cache(maxsize=None)
def design(name):
    """The design's sos [n_sec, 6] (float64)."""
    import scipy.signal
    if name.startswith("bp"):
        return scipy.signal.butter(int(name[2:]), [1.2 * 2 * DT, 30 * 2 * DT], "bandpass", output="sos")
    if name == "lp5":
        return scipy.signal.butter(5, 30 * 2 * DT, "low", output="sos")
    if name == "hp3":
        return scipy.signal.butter(3, 1.2 * 2 * DT, "high", output="sos")
    if name == "lp1":
        return scipy.signal.butter(1, 30 * 2 * DT, "low", output="sos")
    raise KeyError(name)


def n_blocks(n_t, padlen):
    return -(-(n_t + 2 * padlen) // K_SM_L)


def scan_kernel(nb, n_sec):
    """Which scan sosm_scan launches for nb blocks of an n_sec-section filter."""
    if nb <= 2:
        return "none"
    if -(-(nb - 2) // K_SCAN_MG) <= K_SCAN_MQ:
        return "matrix"
    if (nb - 1) * 2 * n_sec <= K_SCAN_CAP:
        return "resident"
    return "staged"


def last_resident_nb(n_sec):
    return K_SCAN_CAP // (2 * n_sec) + 1


def scan_block_counts(name):
    """The block counts the scan-regime test visits for a design: (nb, the scan expected there).  nb = 1, 2 and 3
    only where the design's padlen leaves a record that short (n_t > padlen: 3 padlen < 64 nb); a design that cannot
    reach nb = 3 starts at its shortest record's block count instead."""
    n_sec, padlen = EXPECTED[name]
    nb_min = n_blocks(padlen + 1, padlen)
    nbs = [nb for nb in (1, 2, 3) if nb >= nb_min]
    if nb_min > 3:
        nbs.append(nb_min)
    nbs += [18, 19, 258, 259]          # group length 1 -> 2; the last matrix-pipe scan and the first past it
    if last_resident_nb(n_sec) > 259:  # the last LDS-resident scan and the first staged one
        nbs += [last_resident_nb(n_sec), last_resident_nb(n_sec) + 1]
    return [(nb, scan_kernel(nb, n_sec)) for nb in nbs]


def scan_lengths(name, nb):
    """Record lengths that give nb blocks: the last block full, and the last block holding one sample (or, where
    that record would be no longer than padlen, the shortest record sosfiltfilt accepts)."""
    _, padlen = EXPECTED[name]
    full = K_SM_L * nb - 2 * padlen
    one = max(K_SM_L * (nb - 1) - 2 * padlen + 1, padlen + 1)
    return [n for n in dict.fromkeys((full, one)) if n > padlen]


def scan_cases():
    """(design, nb, n_t) of the float64 scan-regime test."""
    return [(name, nb, n_t) for name in SCAN_DESIGNS for nb, _ in scan_block_counts(name)
            for n_t in scan_lengths(name, nb)]


def scan_cases_f32():
    """The float32 repeat: the first scan, the first block count past the matrix-pipe scan, and the staged scan of the
    3-section designs."""
    out = []
    for name in SCAN_DESIGNS:
        n_sec, _ = EXPECTED[name]
        nbs = [nb for nb, _ in scan_block_counts(name)]
        pick = [min(nb for nb in nbs if nb >= 3), 259]
        if n_sec == 3:
            pick.append(last_resident_nb(3) + 1)
        out += [(name, nb, n_t) for nb in pick for n_t in scan_lengths(name, nb)]
    return out


def record(name, n_rows, n_t, dtype=np.float64, seed=None):
    """The input recipe of tests/test_prep_gpu.py: standard_normal + sin(2 pi 7 t), plus the design's offset."""
    rng = np.random.default_rng(n_t if seed is None else seed)
    t = np.arange(n_t) * DT
    x = rng.standard_normal((n_rows, n_t)) + np.sin(2 * np.pi * 7.0 * t)[None, :] + OFFSET.get(name, 0.0)
    return x.astype(dtype)


def run_filtfilt(device, sos, host, form="matrix", plan_n_t=None, pad=0, lead=0, fill=3.5):
    """dvh_sosfiltfilt (form 'recursion') or dvh_sosfiltfilt_plan + dvh_sosfiltfilt_planned (form 'matrix', the plan
    formed for a record of plan_n_t samples, n_t by default) through the C ABI, on host's rows in host's dtype
    (float32 or float64).  The rows lie in a buffer of row stride n_t + 2 pad that starts lead elements into its
    allocation, every element outside the rows set to fill.  Returns the whole buffer [n_rows, n_t + 2 pad] after the
    call (with pad = 0: the filtered rows)."""
    import scipy.signal
    import torch

    from das_diff_veh_amd import _lib
    from das_diff_veh_amd.preprocess import _padlen
    n_rows, n_t = host.shape
    assert host.dtype in (np.float32, np.float64)
    padlen = _padlen(sos)
    sos_t = torch.from_numpy(np.ascontiguousarray(sos, dtype=np.float64)).to(device)
    zi_t = torch.from_numpy(np.ascontiguousarray(scipy.signal.sosfilt_zi(sos), dtype=np.float64)).to(device)
    stride = n_t + 2 * pad
    buf = np.full(lead + n_rows * stride, fill, host.dtype)
    buf[lead:].reshape(n_rows, stride)[:, pad:pad + n_t] = host
    alloc = torch.from_numpy(buf).to(device)
    dev = alloc[lead:].view(n_rows, stride)
    rows = dev[:, pad:pad + n_t]
    lib = _lib.load()
    nbytes = int(lib.dvh_sosfiltfilt_workspace(n_rows, n_t, len(sos), padlen))
    work = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=device)
    dtype = 0 if host.dtype == np.float32 else 1
    if form == "recursion":
        _lib.call("dvh_sosfiltfilt", _lib.ptr(rows), dtype, n_rows, rows.stride(0), n_t, _lib.ptr(sos_t), len(sos),
                  padlen, _lib.ptr(zi_t), _lib.ptr(work), _lib.stream_of(device))
    else:
        assert form == "matrix"
        plan = torch.empty(int(lib.dvh_sosfiltfilt_plan_bytes(len(sos))) // 8, dtype=torch.float64, device=device)
        _lib.call("dvh_sosfiltfilt_plan", _lib.ptr(sos_t), len(sos), _lib.ptr(zi_t),
                  n_t if plan_n_t is None else plan_n_t, padlen, _lib.ptr(plan), _lib.stream_of(device))
        _lib.call("dvh_sosfiltfilt_planned", _lib.ptr(rows), dtype, n_rows, rows.stride(0), n_t, _lib.ptr(sos_t),
                  len(sos), padlen, _lib.ptr(zi_t), _lib.ptr(plan), _lib.ptr(work), _lib.stream_of(device))
    out = alloc.cpu().numpy()
    if lead:
        assert np.all(out[:lead] == fill)
    return out[lead:].reshape(n_rows, stride)
