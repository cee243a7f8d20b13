"""dvh_cut_windows, dvh_mute_traj, dvh_mute_time and the batched mute of apis/dispersion_classes._device_windows at
the shapes, types and values where their paths change, against NumPy slicing, the oracle's mute_along_traj
(oracle/preprocess.py) and ``data *= tukey(n_t, alpha)``.

Bounds.  Everything here is a copy, a conversion or one multiplication, so the bound is equality of the bits:
  * a same-type cut returns the record's bits (NaN payloads, signalling NaNs, +-inf, -0.0 and denormals included);
    float64 -> float32 equals ``astype(np.float32)`` (round to nearest even, overflow to inf, denormal results),
    float32 -> float64 is exact;
  * a mute forms double(v) * taper (or * 0.0 outside the taper) and rounds once to the data's type, which is what
    NumPy's in-place multiplication of a float32 or float64 array by a float64 mask does.  -0.0, and the sign a zero
    gets from a negative sample, are compared as bits.
The one exception is the payload of a NaN that an operation creates or converts (inf * 0, NaN * 0, NaN cast to
another width): IEEE 754 leaves it open and the host and the device choose differently, so there the NaN positions
are compared and the bits of everything else.
Every output sits between canaries, the gaps between strided passes hold canaries too, and windows that are refused
keep theirs."""
import types

import numpy as np
import pytest
import scipy.signal

from oracle import preprocess as opre
from tests import mute_ref

pytestmark = pytest.mark.gpu
GUARD = 64
CANARY = -777.25          # exact in both types, outside the data's range
NP = {0: np.float32, 1: np.float64}


def _same_bits(got, ref, nan_bits=False):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    g, r = np.ascontiguousarray(got).view(u), np.ascontiguousarray(ref).view(u)
    if nan_bits:
        return bool((g == r).all())
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool((gn == rn).all() and (g[~rn] == r[~rn]).all())


def _specials(dtype):
    """Values a copy or a conversion can get wrong, as an array of dtype."""
    if dtype == np.float32:
        bits = np.array([0x7fc12345, 0xffc00001, 0x7f812345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001,
                         0x807fffff, 0x7f7fffff], dtype=np.uint32)
        return bits.view(np.float32)
    bits = np.array([0x7ff8000000012345, 0xfff8000000000001, 0x7ff0000000012345, 0x7ff0000000000000,
                     0xfff0000000000000, 0x8000000000000000, 0x0000000000000001, 0x800fffffffffffff],
                    dtype=np.uint64)
    vals = np.array([1e39, -1e39, 3.4028235677973366e38, 3.4028234e38, 1e-40, -1e-45, 7.006492321624085e-46, 1e-50,
                     1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24])   # ties and overflow
    return np.concatenate([bits.view(np.float64), vals])


def _record(rng, n_rows, row_stride, dtype, specials=True):
    wide = (np.round(rng.standard_normal((n_rows, row_stride)) * 256) / 256).astype(dtype)
    if specials and wide.size >= 64:
        sp = _specials(dtype)
        idx = rng.choice(wide.size, size=4 * len(sp), replace=False)
        wide.reshape(-1)[idx] = np.tile(sp, 4)
    return wide


# ------------------------------------------------------------------------------------------ dvh_cut_windows

def _cut(wide, col0, rec_n_t, starts, x_start, n_ch, n_t, out_code, sentinel=True):
    """The record is the column slice wide[:, col0:col0 + rec_n_t] of a wider buffer whose other columns hold a
    sentinel -> (out [n_win, n_ch, n_t] with refused windows left as CANARY, status)."""
    import torch

    from das_diff_veh_amd import _lib
    wide = wide.copy()
    if sentinel:
        wide[:, :col0] = 12345.0
        wide[:, col0 + rec_n_t:] = 12345.0
    in_code = 0 if wide.dtype == np.float32 else 1
    t = torch.from_numpy(wide).cuda()
    rec = t[:, col0:col0 + rec_n_t]
    st = torch.from_numpy(np.asarray(starts, dtype=np.int64)).cuda()
    n_win = len(starts)
    n = n_win * n_ch * n_t
    buf = torch.full((GUARD + n + GUARD,), CANARY, dtype=torch.float32 if out_code == 0 else torch.float64,
                     device="cuda")
    status = torch.zeros(1 + GUARD, dtype=torch.int32, device="cuda")
    _lib.call("dvh_cut_windows", _lib.ptr(rec), in_code, wide.shape[0], wide.shape[1], rec_n_t, _lib.ptr(st), n_win,
              x_start, n_ch, n_t, _lib.ptr(buf[GUARD:]), out_code, _lib.ptr(status), _lib.stream_of(t.device))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[GUARD + n:] == CANARY).all()
    stat = status.cpu().numpy()
    assert not stat[1:].any()
    return got[GUARD:GUARD + n].reshape(n_win, n_ch, n_t), int(stat[0]), wide


def _cut_ref(wide, col0, rec_n_t, starts, x_start, n_ch, n_t, out_code):
    out = np.full((len(starts), n_ch, n_t), CANARY, dtype=NP[out_code])
    bad = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for w, s in enumerate(starts):
            if 0 <= s <= rec_n_t - n_t:
                out[w] = wide[x_start:x_start + n_ch, col0 + s:col0 + s + n_t].astype(NP[out_code])
            else:
                bad = 1
    return out, bad


def _check_cut(wide, col0, rec_n_t, starts, x_start, n_ch, n_t, out_code):
    got, status, wide = _cut(wide, col0, rec_n_t, starts, x_start, n_ch, n_t, out_code)
    ref, bad = _cut_ref(wide, col0, rec_n_t, starts, x_start, n_ch, n_t, out_code)
    assert status == bad
    assert _same_bits(got, ref, nan_bits=wide.dtype == ref.dtype), (wide.dtype, ref.dtype, n_ch, n_t, x_start)
    assert not (got == 12345.0).any()
    return got


@pytest.mark.parametrize("in_code,out_code", [(0, 0), (1, 1), (1, 0), (0, 1)])
def test_cut_dtype_pairs(device, in_code, out_code):
    rng = np.random.default_rng(10 * in_code + out_code)
    rec_n_t, n_t, n_ch, n_rows = 1000, 257, 3, 6
    wide = _record(rng, n_rows, rec_n_t + 24, NP[in_code])
    starts = [0, rec_n_t - n_t, 100, 100, 300, 50, 101]               # both ends, repeated, overlapping, descending
    got = _check_cut(wide, 13, rec_n_t, starts, 2, n_ch, n_t, out_code)
    sp = _specials(NP[in_code])                                       # every special value, in one window of their own
    row = np.zeros((1, 64), dtype=NP[in_code])
    row[0, 5:5 + len(sp)] = sp
    got = _check_cut(row, 0, 64, [0, 3], 0, 1, 40, out_code)
    if (in_code, out_code) == (1, 0):
        assert np.isinf(got[0, 0, 5 + 8]) and got[0, 0, 5 + 12] == np.float32(1e-40) and got[0, 0, 5 + 15] == 0
        assert got[0, 0, 5 + 10] == np.float32(3.4028235e38) or np.isinf(got[0, 0, 5 + 10])


@pytest.mark.parametrize("n_t", [1, 255, 256, 257, 16384, 16385, 40000])
@pytest.mark.parametrize("n_ch", [1, 3])
def test_cut_shapes(device, n_t, n_ch):
    """n_t around the 256-thread block and past the 64 x 256 samples one pass of the grid covers; the first and the
    last legal channel and start; a record inside a wider buffer."""
    rng = np.random.default_rng(n_t + n_ch)
    rec_n_t, n_rows = n_t + 37, n_ch + 2
    wide = _record(rng, n_rows, rec_n_t + 11, np.float32)
    starts = [0, 37, 20, 20, 5, 36]
    for x_start in (0, n_rows - n_ch):
        _check_cut(wide, 5, rec_n_t, starts, x_start, n_ch, n_t, 0)
    with np.errstate(invalid="ignore"):                               # a signalling NaN widened
        wide64 = wide.astype(np.float64)
    _check_cut(wide64, 5, rec_n_t, starts[:3], 1, n_ch, n_t, 0)
    _check_cut(wide, 0, n_t, [0], 0, n_ch, n_t, 1)                    # the window is the whole record


def test_cut_invalid_starts_among_valid_ones(device):
    rng = np.random.default_rng(5)
    rec_n_t, n_t, n_ch = 300, 120, 2
    wide = _record(rng, 4, rec_n_t + 9, np.float64)
    starts = [0, -1, 10, rec_n_t - n_t + 1, rec_n_t - n_t, 2 ** 40, -2 ** 40, 180, rec_n_t]
    got, status, wide2 = _cut(wide, 4, rec_n_t, starts, 1, n_ch, n_t, 1)
    ref, bad = _cut_ref(wide2, 4, rec_n_t, starts, 1, n_ch, n_t, 1)
    assert status == 1 and bad == 1 and _same_bits(got, ref, nan_bits=True)
    for w in (1, 3, 5, 6, 8):
        assert (got[w] == CANARY).all()
    got, status, _ = _cut(wide, 4, rec_n_t, [0, 180, 10], 1, n_ch, n_t, 1)
    assert status == 0                                                # the same call without them


@pytest.mark.parametrize("n_win", [65535, 65536, 65537])
def test_cut_window_chunks(device, n_win):
    """More windows than gridDim.z takes: every window on either side of the chunk boundary is its own."""
    rec_n_t = 70001
    rec = np.arange(rec_n_t, dtype=np.float32)[None, :]               # the record holds its own sample index
    starts = (np.arange(n_win, dtype=np.int64) * 7919) % (rec_n_t - 1)
    got, status, _ = _cut(rec, 0, rec_n_t, starts, 0, 1, 2, 0, sentinel=False)
    assert status == 0
    assert np.array_equal(got[:, 0, 0], starts.astype(np.float32)) and np.array_equal(got[:, 0, 1], got[:, 0, 0] + 1)


def test_select_cut_windows(device):
    """select.cut_windows against rec[x0:x1, t0:t1] with Python's slice rules."""
    import torch

    from das_diff_veh_amd.select import cut_windows
    rng = np.random.default_rng(6)
    host = _record(rng, 10, 500, np.float64)
    t0 = np.array([0, 450, 400, 200, 300, -80, -600, 499, 120, 470])
    t1 = np.array([100, 550, 520, 200, 250, -30, 60, 900, 220, 520])  # clipped at the end, empty, negative bounds
    for rec in (torch.from_numpy(host).cuda(), torch.from_numpy(np.repeat(host, 2, axis=1)).cuda()[:, ::2]):
        assert rec.shape == (10, 500)
        for x_range in ((2, 7), (-4, -1), (3, 50), (-50, 4), (0, 10), (6, 6)):
            for out_dtype in (None, torch.float32):
                batches, where = cut_windows(rec, x_range, t0, t1, out_dtype=out_dtype)
                assert len(where) == len(t0)
                seen = set()
                for w, (length, j) in enumerate(where):
                    ref = host[x_range[0]:x_range[1], t0[w]:t1[w]]
                    assert length == ref.shape[1] and (length, j) not in seen
                    seen.add((length, j))
                    got = batches[length][j].cpu().numpy()
                    with np.errstate(over="ignore", invalid="ignore"):
                        ref = ref if out_dtype is None else ref.astype(np.float32)
                    assert _same_bits(got, np.ascontiguousarray(ref), nan_bits=out_dtype is None), (x_range, w)
                assert sum(b.shape[0] for b in batches.values()) == len(t0)
                assert set(batches) == {0, 1, 30, 50, 60, 100} and batches[100].shape[0] == 3


# ------------------------------------------------------------------------------------------ dvh_mute_traj

def _mute_traj(data, tabs, taper, gap, code=None):
    """dvh_mute_traj on data [n_pass, n_ch, n_t] laid out pass_stride = n_ch n_t + gap apart between canaries ->
    the muted passes."""
    import torch

    from das_diff_veh_amd import _lib
    from das_diff_veh_amd.preprocess import taper_on_device
    n_pass, n_ch, n_t = data.shape
    stride = n_ch * n_t + gap
    host = np.full(GUARD + n_pass * stride + GUARD, CANARY, dtype=data.dtype)
    body = host[GUARD:GUARD + n_pass * stride].reshape(n_pass, stride)
    body[:, :n_ch * n_t] = data.reshape(n_pass, -1)
    buf = torch.from_numpy(host).cuda()
    tab_t = torch.from_numpy(np.ascontiguousarray(tabs, dtype=np.int32)).cuda()
    taper_t = taper_on_device(taper, buf.device)
    _lib.call("dvh_mute_traj", _lib.ptr(buf[GUARD:]), 0 if data.dtype == np.float32 else 1, n_pass, stride, n_ch, n_t,
              _lib.ptr(tab_t), _lib.ptr(taper_t), _lib.stream_of(buf.device))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[GUARD + n_pass * stride:] == CANARY).all()
    body = got[GUARD:GUARD + n_pass * stride].reshape(n_pass, stride)
    assert (body[:, n_ch * n_t:] == CANARY).all()
    return body[:, :n_ch * n_t].reshape(n_pass, n_ch, n_t).copy()


def _mute_data(rng, shape, dtype):
    data = (np.round(rng.standard_normal(shape) * 256) / 256).astype(dtype)
    flat = data.reshape(-1)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype=dtype)
    n = min(flat.size // 2, 40 * len(sp))
    if n:
        flat[rng.choice(flat.size, size=n, replace=False)] = np.resize(sp, n)     # inside and outside the taper
    return data


@pytest.mark.parametrize("n_ch", [1, 2, 49, 120])
def test_mute_traj(device, n_ch):
    from das_diff_veh_amd.preprocess import mute_traj_table
    kinds = ["crossing", "inside", "left", "right", "two_points"]
    with np.errstate(invalid="ignore"):
        for i, n_t in enumerate([1, 255, 256, 257, 1000]):
            for dtype in (np.float32, np.float64):
                for n_pass, gap in ((1, 0), (3, 13)):
                    rng = np.random.default_rng(1000 * n_ch + n_t + n_pass)
                    data = _mute_data(rng, (n_pass, n_ch, n_t), dtype)
                    t_axis = 10.0 + 0.004 * np.arange(n_t)
                    if n_ch == 1:        # no channel spacing for the oracle to take: a table by hand, applied in NumPy
                        taper = scipy.signal.windows.tukey(5, 0.3)
                        tab = np.array([[(0, 1, (t + p) % 5) if (t + p) % 3 else (p % 2, p % 2, 0) for t in range(n_t)]
                                        for p in range(n_pass)], dtype=np.int32)
                        ref = np.stack([mute_ref.apply_table(data[p], tab[p], taper) for p in range(n_pass)])
                    else:
                        x_axis = 500.0 + 8.16 * np.arange(n_ch)
                        offset = 300 if n_ch > 2 else 20      # 36 channels of taper: clipped at both ends while crossing
                        tabs, ref = [], []
                        for p in range(n_pass):               # another trajectory for every pass
                            vx, vt = mute_ref.vehicle(kinds[(i + p + 4) % len(kinds)], x_axis, t_axis)
                            tab, taper = mute_traj_table(x_axis, t_axis, vx, vt, offset=offset)
                            tabs.append(tab)
                            ref.append(opre.mute_along_traj(data[p], x_axis, t_axis, vx, vt, offset=offset).astype(dtype))
                        tab, ref = np.stack(tabs), np.stack(ref)
                        if n_ch == 49 and n_t == 255:         # pass 0 crosses: its taper is cut at the first and the last channel
                            assert (tab[0, :, 0] == 0).any() and (tab[0, :, 2] > 0).any() and (tab[0, :, 1] == n_ch).any()
                    got = _mute_traj(data, tab, taper, gap)
                    assert _same_bits(got, ref), (n_ch, n_t, dtype, n_pass)


@pytest.mark.parametrize("offset,n_samp", [(0.5, 0), (1, 1), (2, 2), (3, 3), (7, 7), (15, 15), (40, 40)])
def test_mute_traj_taper_lengths(device, offset, n_samp):
    """Tapers of 0, 1, 2 and 3 channels, an odd one and ones longer than twice the window (7 channels 1 m apart),
    through the C ABI and through preprocess.mute_along_traj (an empty taper zeroes the window, as the reference
    does)."""
    from das_diff_veh_amd.preprocess import mute_along_traj, mute_traj_table
    n_ch, n_t = 7, 90
    x_axis = 500.0 + 1.0 * np.arange(n_ch)
    t_axis = 10.0 + 0.004 * np.arange(n_t)
    vx, vt = np.array([480.0, 530.0]), np.array([t_axis[0], t_axis[-1]])     # with delta_x = 20: across the window
    tab, taper = mute_traj_table(x_axis, t_axis, vx, vt, offset=offset)
    assert len(taper) == n_samp
    with np.errstate(invalid="ignore"):
        for dtype in (np.float32, np.float64):
            data = _mute_data(np.random.default_rng(n_samp), (1, n_ch, n_t), dtype)
            ref = opre.mute_along_traj(data[0], x_axis, t_axis, vx, vt, offset=offset).astype(dtype)
            assert _same_bits(_mute_traj(data, tab[None], taper, 5)[0], ref), (offset, dtype)
            win = types.SimpleNamespace(data=data[0].copy(), x_axis=x_axis, t_axis=t_axis, veh_state_x=vx, veh_state_t=vt)
            mute_along_traj(win, offset=offset)
            assert _same_bits(win.data, ref), (offset, dtype)
            if n_samp == 0:
                assert not np.nan_to_num(win.data, nan=0.0, posinf=0.0, neginf=0.0).any()


def test_mute_traj_grid_limits(device):
    """A launch takes at most 65 535 channels and 65 535 passes: one more of either is refused with -4 before
    anything runs, and the data is as it was."""
    import torch

    from das_diff_veh_amd import _lib
    data = torch.full((65536 + 2 * GUARD,), 3.0, dtype=torch.float32, device="cuda")
    tab = torch.tensor([[0, 1, 0]] * 65536, dtype=torch.int32, device="cuda")
    taper = torch.tensor([0.5], dtype=torch.float64, device="cuda")
    st = _lib.stream_of(data.device)
    for n_pass, n_ch in ((65536, 1), (1, 65536)):
        with pytest.raises(ValueError, match="too many"):
            _lib.call("dvh_mute_traj", _lib.ptr(data[GUARD:]), 0, n_pass, n_ch, n_ch, 1, _lib.ptr(tab), _lib.ptr(taper), st)
        assert _lib.load().dvh_mute_traj(_lib.ptr(data[GUARD:]), 0, n_pass, n_ch, n_ch, 1, _lib.ptr(tab), _lib.ptr(taper),
                                         st) == -4
        torch.cuda.synchronize()
        assert bool((data == 3.0).all())
    _lib.call("dvh_mute_traj", _lib.ptr(data[GUARD:]), 0, 65535, 1, 1, 1, _lib.ptr(tab), _lib.ptr(taper), st)   # the limit
    torch.cuda.synchronize()
    got = data.cpu().numpy()
    assert (got[GUARD:GUARD + 65535] == 1.5).all() and (got[:GUARD] == 3.0).all() and (got[GUARD + 65535:] == 3.0).all()


# ------------------------------------------------------------------------------------------ dvh_mute_time

def _mute_time(data, taper):
    import torch

    from das_diff_veh_amd import _lib
    n_t = data.shape[-1]
    host = np.full(GUARD + data.size + GUARD, CANARY, dtype=data.dtype)
    host[GUARD:GUARD + data.size] = data.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    tp = torch.from_numpy(np.ascontiguousarray(taper, dtype=np.float64)).cuda()
    _lib.call("dvh_mute_time", _lib.ptr(buf[GUARD:]), 0 if data.dtype == np.float32 else 1, data.size // n_t, n_t,
              _lib.ptr(tp), _lib.stream_of(buf.device))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[GUARD + data.size:] == CANARY).all()
    return got[GUARD:GUARD + data.size].reshape(data.shape)


@pytest.mark.parametrize("alpha", [0, 0.3, 1])
def test_mute_time(device, alpha):
    from das_diff_veh_amd.apis.data_classes import SurfaceWaveWindow
    with np.errstate(invalid="ignore"):
        for shape in ((3, 255), (1, 1), (5, 2), (7, 257), (4, 256), (2, 3, 50)):
            for dtype in (np.float32, np.float64):
                data = _mute_data(np.random.default_rng(shape[-1]), shape, dtype)
                taper = scipy.signal.windows.tukey(shape[-1], alpha)
                ref = data.copy()
                ref *= taper                                             # the reference's statement
                assert _same_bits(_mute_time(data, taper), ref), (shape, dtype, alpha)
                win = SurfaceWaveWindow.__new__(SurfaceWaveWindow)
                win.data, win.muted_along_time = data.copy(), False
                win.mute_along_time(alpha=alpha)
                assert win.muted_along_time and _same_bits(win.data, ref), (shape, dtype, alpha)


# ------------------------------------------------------------------------------------------ _device_windows

def test_device_windows_partial_mute(device):
    """Five same-shape windows of which the second and the fifth are muted already: the others are muted on the
    device copy (gathered, muted in one launch and scattered back), those two are the plain float32 copies, and the
    windows themselves are left alone."""
    from das_diff_veh_amd.apis.dispersion_classes import _device_windows
    n_ch, n_t, offset = 40, 130, 150
    x_axis = 500.0 + 8.16 * np.arange(n_ch)
    t_axis = 10.0 + 0.004 * np.arange(n_t)
    kinds = ["crossing", "inside", "two_points", "left", "crossing"]
    rng = np.random.default_rng(77)

    def windows(muted):
        out = []
        for i, kind in enumerate(kinds):
            vx, vt = mute_ref.vehicle(kind, x_axis, t_axis + 0.1 * i)
            data = (np.round(rng.standard_normal((n_ch, n_t)) * 256) / 256).astype(np.float32 if i % 2 else np.float64)
            out.append(types.SimpleNamespace(data=data, x_axis=x_axis, t_axis=t_axis + 0.1 * i, veh_state_x=vx,
                                             veh_state_t=vt, muted_along_traj=i in muted))
        return out

    for muted in ((1, 4), (), (0, 1, 2, 3, 4), (0,), (1, 2, 3, 4)):
        wins = windows(muted)
        keep = [w.data.copy() for w in wins]
        for idx in ([0, 1, 2, 3, 4], [4, 2, 1]):
            got = _device_windows(wins, idx, offset).cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (len(idx), n_ch, n_t)
            for k, i in enumerate(idx):
                w = wins[i]
                plain = w.data.astype(np.float32)
                ref = plain if i in muted else opre.mute_along_traj(
                    plain, w.x_axis, w.t_axis, w.veh_state_x, w.veh_state_t, offset=offset).astype(np.float32)
                assert _same_bits(got[k], ref), (muted, idx, i)
                if i not in muted:
                    assert not np.array_equal(got[k], plain)
            plain = _device_windows(wins, idx, None).cpu().numpy()         # no offset: nothing is muted
            assert all(_same_bits(plain[k], wins[i].data.astype(np.float32)) for k, i in enumerate(idx))
        assert all(np.array_equal(w.data, d) for w, d in zip(wins, keep))
