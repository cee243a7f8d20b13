"""Phase-shift dispersion on the device: map_fv_FD_slant_stack against the reference's recorded outputs
(tests/golden/slant.npz), and slant_maps, slant_class_means, Dispersion(transform="slant") and dvh_disp_slant itself
against tests/slant_ref (float64) on the same float32-exact values.

Two bounds per image, relative to the image maximum:
  CONTRACT 1e-4   the project's bound on an f-v image
  DERIVED  1e-6   float32 storage costs 2**-24; with ``norm`` the float32 row scale costs 2**-24 per row, which shows in
                  the image amplified by at most sum_ix |D[ix, f]| / max|image| <= 8 (condition (a) of the fixture,
                  tests/test_slant_host.py; asserted here for the data made in this file): (1 + 8) * 2**-24 = 5.4e-7.
                  The float64 sums add ~1e-14.
Picks: the device argmax over velocity of column j is accepted iff ref[pick, j] >= ref[:, j].max() - 2e-6 max|ref| -- only
candidates closer than twice the asserted error can swap; the count of strictly identical picks is printed.
NaN and inf patterns must agree (golden_io.gather_rel_err).
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import golden_io as gio
from tests import slant_ref
from tests.slant_ref import CASES, case

pytestmark = pytest.mark.gpu

CONTRACT, DERIVED = 1e-4, 1e-6
QUANT = 2.0 ** -8
DX, DT500 = 8.16, 0.003999999999997783
POISON = -7.0


def _check(got, want, what):
    """Both bounds, the patterns and the picks of one image."""
    err = gio.gather_rel_err(got, want)
    line = f"{what}: {err:.3g} of the image maximum"
    if np.isfinite(want).all() and want.shape[0] > 1 and want.max() > 0:
        cols = np.arange(want.shape[1])
        pick = np.asarray(got).argmax(axis=0)
        ok = want[pick, cols] >= want.max(axis=0) - 2e-6 * np.abs(want).max()
        line += f", {int((pick == want.argmax(axis=0)).sum())} of {cols.size} picks strictly identical"
        print(line)
        assert ok.all(), f"{what}: {(~ok).sum()} of {ok.size} picks miss the reference maximum"
    else:
        print(line)
    assert err < CONTRACT and err < DERIVED, (what, err)
    return err


def _gather(seed, nch, nt, dt=DT500):
    """A float32-exact gather (multiples of 2**-8): plane waves under a moving envelope plus noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(nt) * dt
    x = 0.6 * rng.standard_normal((nch, nt))
    for f, c in ((4.0, 310.0), (9.0, 420.0), (15.0, 560.0)):
        delay = (np.arange(nch) * DX / c)[:, None]
        x += 4.0 * np.exp(-0.5 * ((t - 0.3 * nt * dt - delay) / (0.12 * nt * dt)) ** 2) * \
            np.cos(2 * np.pi * f * (t - delay) + 0.7 * f)
    return np.round(x / QUANT) * QUANT


def _ref(data, dt, freqs, vels, norm, rows):
    """slant_ref's image, with condition (a) asserted where ``norm`` makes the derived bound depend on it."""
    want = slant_ref.slant(data, DX, dt, freqs, vels, norm=norm, rows=rows)
    if norm and want.size and np.isfinite(want).all() and want.max() > 0:
        ratio = slant_ref.coherence_ratio(data, dt, freqs, want, norm=True, rows=rows)
        assert ratio <= 8, ratio
    return want


@functools.lru_cache(maxsize=None)
def _case_a_batch():
    g = gio.load("slant")
    data, dx, dt, freqs, vels, norm = case(g, "A")
    batch = np.stack([data, _gather(41, 25, 500), _gather(42, 25, 500)])
    want = np.stack([_ref(d, dt, freqs, vels, True, (6, 25)) for d in batch])
    want.setflags(write=False)
    return batch, dt, freqs, vels, want


def _maps(device, batch, dt, freqs, vels, norm=True, rows=(6, 25)):
    import torch

    from das_diff_veh_amd.disp import SlantPlan, slant_maps
    batch = np.asarray(batch, dtype=np.float32)
    plan = SlantPlan(batch.shape[1], batch.shape[2], DX, dt, freqs, vels, rows=rows)
    out = slant_maps(torch.from_numpy(batch).to(device), plan, norm=norm)
    assert out.dtype == torch.float32 and tuple(out.shape) == (batch.shape[0], plan.nV, plan.nF)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_drop_in_matches_reference(device, name):
    from das_diff_veh_amd.modules.utils import map_fv_FD_slant_stack
    g = gio.load("slant")
    data, dx, dt, freqs, vels, norm = case(g, name)
    want = g[f"{name}_out"]
    got = map_fv_FD_slant_stack(data, dx, dt, freqs, vels, norm=norm)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got, equal_nan=True)   # the device's float32 values
    _check(got, want, f"case {name}")
    if name == "F":
        assert not got.any()
        plain = map_fv_FD_slant_stack(data, dx, dt, freqs, vels, norm=False)
        assert plain.shape == want.shape and not plain.any() and not g["F_out_plain"].any()
    if name == "G":
        assert np.isnan(got).all()
    if name == "A":     # a device tensor comes in as a host array does
        import torch
        again = map_fv_FD_slant_stack(torch.from_numpy(data.astype(np.float32)).to(device), dx, dt, freqs, vels)
        assert np.array_equal(again, got)


def test_batch_of_three_equals_single_calls(device):
    batch, dt, freqs, vels, want = _case_a_batch()
    got = _maps(device, batch, dt, freqs, vels)
    for b in range(3):
        _check(got[b], want[b], f"batch image {b}")
        assert np.array_equal(_maps(device, batch[b:b + 1], dt, freqs, vels)[0], got[b]), b
    assert np.array_equal(_maps(device, batch, dt, freqs, vels), got)      # two runs of one call
    import torch

    from das_diff_veh_amd.disp import SlantPlan, slant_maps
    plan = SlantPlan(25, 500, DX, dt, freqs, vels)
    x = torch.from_numpy(batch.astype(np.float32)).to(device)
    out = torch.full((3, vels.size, freqs.size), POISON, dtype=torch.float32, device=device)
    assert slant_maps(x, plan, out=out) is out and np.array_equal(out.cpu().numpy(), got)     # into a given buffer
    with pytest.raises(ValueError, match="out must be"):
        slant_maps(x, plan, out=out[:2])


def test_large_batch(device):
    """70 gathers on a 5 x 7 grid: one block of pairs, so the launcher gives every gather a z-slice of its own (70
    slices, one gather per lane).  The lane's loop over several gathers is test_gather_loop's."""
    freqs, vels = np.linspace(3.0, 19.0, 5), np.linspace(250.0, 850.0, 7)
    batch = np.stack([_gather(100 + b, 25, 64, 0.004) for b in range(70)])
    got = _maps(device, batch, 0.004, freqs, vels)
    worst = max(gio.gather_rel_err(got[b], _ref(batch[b], 0.004, freqs, vels, True, (6, 25))) for b in range(70))
    print(f"70 gathers: worst {worst:.3g}")
    assert worst < DERIVED
    for b in (0, 33, 69):
        assert np.array_equal(_maps(device, batch[b:b + 1], 0.004, freqs, vels)[0], got[b]), b


@pytest.mark.parametrize("rows", [(6, 25), (0, 25)])
def test_gather_loop(device, rows):
    """70 gathers on 280 x 250 pairs: 274 blocks of pairs, so the launcher (8 blocks per CU: 2 048 on 256 CUs) makes
    ceil(2 048 / 274) = 8 z-slices and a lane loops over gathers z, z + 8, ...: 9 of them in slices 0-5, 8 in slices 6
    and 7.  Rows (6, 25) are 19: the powers held in registers across the loop; rows (0, 25) are 25: the running power,
    restarted per gather.  Every image against slant_ref, and bit for bit the image of a call with that gather alone
    (one slice, one iteration) for the first and last gather of a slice and the last of the batch."""
    import torch
    freqs, vels = np.linspace(1.0, 30.0, 280), np.linspace(200.0, 1200.0, 250)
    B = 70
    gx = -(-freqs.size * vels.size // 256)
    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    gz = min(B, -(-8 * n_cu // gx))
    print(f"{n_cu} CUs: {gx} blocks of pairs, {gz} z-slices, {-(-B // gz)} gathers per lane at most")
    assert 1 < -(-B // gz) and B % gz, "the batch must loop inside a lane, unevenly over the slices"
    batch = np.stack([_gather(300 + b, 25, 64, 0.004) for b in range(B)])
    got = _maps(device, batch, 0.004, freqs, vels, rows=rows)
    worst = 0.0
    for b in range(B):
        worst = max(worst, gio.gather_rel_err(got[b], _ref(batch[b], 0.004, freqs, vels, True, rows)))
    print(f"rows {rows}: worst of {B} images {worst:.3g}")
    assert worst < DERIVED
    for b in (0, gz - 1, gz, B - gz, B - 1):
        assert np.array_equal(_maps(device, batch[b:b + 1], 0.004, freqs, vels, rows=rows)[0], got[b]), b


@pytest.mark.parametrize("nch,rows", [(49, (0, 49)), (25, (24, 25)), (24, (0, 24)), (25, (0, 25)), (25, (3, 3))])
def test_row_ranges(device, nch, rows):
    """49 and 25 rows: the running power inside the row loop; 24 rows: the last count with the powers in registers;
    one row; none."""
    freqs, vels = np.arange(0.8, 25, 0.8), np.arange(200, 1200, 37.)
    data = _gather(nch, nch, 500)
    for norm in (True, False):
        got = _maps(device, data[None], DT500, freqs, vels, norm=norm, rows=rows)[0]
        _check(got, _ref(data, DT500, freqs, vels, norm, rows), f"{nch} channels, rows {rows}, norm {norm}")
        if rows[0] == rows[1]:
            assert not got.any()


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_wide_column_spans(device, order):
    """300 frequencies a bin or more apart, so every lane of a wave reads a column of the spectrum of its own (the other
    tests' neighbouring lanes share bins); shuffled, the columns come in no order and the image keeps the caller's."""
    from das_diff_veh_amd.disp import SlantPlan
    freqs = np.linspace(0.5, 100.0, 300)
    if order == "shuffled":
        freqs = np.random.default_rng(3).permutation(freqs)
    vels = np.array([260.0, 410.0, 900.0])
    data = _gather(77, 25, 500)
    assert SlantPlan(25, 500, DX, DT500, freqs, vels).n_fb == 300
    for norm in (True, False):
        got = _maps(device, data[None], DT500, freqs, vels, norm=norm)[0]
        _check(got, _ref(data, DT500, freqs, vels, norm, (6, 25)), f"300 bins {order}, norm {norm}")


def test_class_means(device, monkeypatch):
    """slots [0, 1, 0, 1] of three classes: sum(images) / len in selection order, exactly as dvh_select_mean_var
    evaluates it on the per-pass device images; the third class has no pass and stays 0.  The same with the
    velocities taken in chunks of 3 rows."""
    import torch

    from das_diff_veh_amd import disp
    batch, dt, freqs, vels, want = _case_a_batch()
    batch = np.concatenate([batch, _gather(43, 25, 500)[None]])
    want = np.concatenate([want, _ref(batch[3], dt, freqs, vels, True, (6, 25))[None]])
    plan = disp.SlantPlan(25, 500, DX, dt, freqs, vels)
    x = torch.from_numpy(batch.astype(np.float32)).to(device)
    imgs = disp.slant_maps(x, plan).cpu().numpy()
    got = disp.slant_class_means(x, plan, [0, 1, 0, 1], 3).cpu().numpy()
    assert got.shape == (3, vels.size, freqs.size) and got.dtype == np.float32
    for s, (i, j) in enumerate(((0, 2), (1, 3))):
        assert np.array_equal(got[s], (imgs[i] + imgs[j]) / np.float32(2)), s
        _check(got[s], (want[i] + want[j]) / 2, f"class {s}")
    assert not got[2].any()
    monkeypatch.setattr(disp, "SLANT_CHUNK_BYTES", 4 * 4 * freqs.size * 3)
    assert np.array_equal(disp.slant_class_means(x, plan, [0, 1, 0, 1], 3).cpu().numpy(), got)
    full = disp.slant_class_means(x, plan, [1, 0, 0, 0], 2).cpu().numpy()
    assert np.array_equal(full[1], imgs[0])         # a class of one pass is that pass, bit for bit
    assert np.array_equal(full[0], (imgs[1] + imgs[2] + imgs[3]) / np.float32(3))
    with pytest.raises(ValueError, match="class slot"):
        disp.slant_class_means(x, plan, [0, 1, 0, 3], 3)


def test_dispersion_transform(device):
    from das_diff_veh_amd.apis.virtual_shot_gather import VirtualShotGather
    from das_diff_veh_amd.modules.utils import Dispersion, map_fv_FD_slant_stack
    from oracle.disp import pick_ok
    g = gio.load("slant")
    data, dx, dt, freqs, vels, norm = case(g, "A")
    d = Dispersion(data[6:25], dx, dt, freqs, vels, norm=norm, transform="slant")
    drop_in = map_fv_FD_slant_stack(data, dx, dt, freqs, vels, norm=norm)
    assert vels[0] < vels[-1] and d.fv_map.dtype == np.float32 and d.fv_map.shape == drop_in.shape
    assert np.array_equal(d.fv_map, drop_in[::-1])          # descending velocity: map_fv's row convention
    shuffled = np.random.default_rng(0).permutation(vels)
    assert np.array_equal(Dispersion(data[6:25], dx, dt, freqs, shuffled, norm=norm, transform="slant").fv_map, d.fv_map)
    with pytest.raises(ValueError, match="transform"):
        Dispersion(data, dx, dt, freqs, vels, transform="phase")
    with pytest.raises(ValueError, match="math domain error"):
        map_fv_FD_slant_stack(data, dx, dt, freqs, np.append(vels, 0.0))
    # the class stack of the w = 500 fixture, on the default grid of compute_disp_image
    v = gio.load("vsg_w500")
    vsg = VirtualShotGather._from_arrays(None, v["stack"], v["gather_x_axis"], v["gather_t_axis"])
    vsg.compute_disp_image(end_x=0, start_x=-200, transform="slant")
    s = np.abs(v["gather_x_axis"] + 200).argmin()
    e = np.abs(v["gather_x_axis"]).argmin()
    rows = np.asarray(v["stack"][s:e + 1], dtype=np.float32).astype(np.float64)
    fr, ve = np.arange(0.8, 25, 0.1), np.arange(200, 1200)
    want = slant_ref.slant(rows, 8.16, v["gather_t_axis"][1] - v["gather_t_axis"][0], fr, ve[::-1], norm=False,
                           rows=(0, len(rows)))
    assert vsg.disp.fv_map.shape == (1000, 242) and vsg.disp.transform == "slant"
    _check(vsg.disp.fv_map, want, f"vsg_w500 stack, {len(rows)} rows")
    vsg.compute_disp_image(end_x=0, start_x=-200)           # the default is still map_fv
    assert vsg.disp.transform == "fk"
    fk_map = vsg.disp.fv_map       # the f-k contract: 1e-4 of the maximum, every pick on the reference's maximum
    assert fk_map.shape == v["fv_map"].shape
    assert np.abs(fk_map.astype(np.float64) - v["fv_map"]).max() < CONTRACT * np.abs(v["fv_map"]).max()
    assert pick_ok(v["fv_map"], np.argmax(fk_map, axis=0)).all()


def _abi_call(lib, D, B, nch, n_fb, row0, n_row, fb, freqs, vels, fv, stride):
    from das_diff_veh_amd import _lib
    return lib.dvh_disp_slant(_lib.ptr(D), B, nch, n_fb, row0, n_row, _lib.ptr(fb), _lib.ptr(freqs), freqs.numel(),
                              _lib.ptr(vels), vels.numel(), DX, _lib.ptr(fv), stride, _lib.stream_of(fv.device))


def test_abi_rows_strides_and_statuses(device):
    """dvh_disp_slant on a spectrum made on the host: rows [6, 25) of 25 (row0 > 0), images b_stride = nF nV + 5 apart
    in a poisoned buffer whose gaps stay poisoned; the -2 statuses write nothing."""
    import torch

    from das_diff_veh_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    B, nch, n_fb, nF, nV = 2, 25, 6, 9, 5
    spec = rng.standard_normal((B, nch, n_fb)) + 1j * rng.standard_normal((B, nch, n_fb))
    fbh = rng.integers(0, n_fb, nF).astype(np.int32)
    freqs, vels = np.linspace(2.0, 22.0, nF), np.array([300.0, -410.0, 555.5, 720.0, 1000.0])
    w = np.exp(1j * (2 * np.pi * freqs[:, None] * DX / vels[None, :]))
    want = np.abs(sum(spec[:, 6 + r][:, fbh][:, :, None] * w[None] ** r for r in range(19))).transpose(0, 2, 1)
    inter = np.stack([spec.real, spec.imag], axis=-1).reshape(B * nch, 2 * n_fb)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    D, fb, fr, ve = t(inter), t(fbh), t(freqs), t(vels)
    stride = nF * nV + 5
    fv = torch.full((B * stride,), POISON, dtype=torch.float32, device=device)
    assert _abi_call(lib, D, B, nch, n_fb, 6, 19, fb, fr, ve, fv, stride) == 0
    out = fv.cpu().numpy().reshape(B, stride)
    assert (out[:, nF * nV:] == POISON).all()
    for b in range(B):
        err = gio.gather_rel_err(out[b, :nF * nV].reshape(nV, nF), want[b])
        print(f"ABI image {b}: {err:.3g}")
        assert err < 2.0 ** -23          # float32 storage of a float64 sum
    fv.fill_(POISON)
    for kw, msg in ((dict(row0=7), b"leave the gather"), (dict(n_fb=0), b"n_fb")):
        a = dict(nch=nch, n_fb=n_fb, row0=6, n_row=19)
        a.update(kw)
        assert _abi_call(lib, D, B, a["nch"], a["n_fb"], a["row0"], a["n_row"], fb, fr, ve, fv, stride) == -2
        assert msg in lib.dvh_last_error()
    torch.cuda.synchronize()
    assert bool((fv == POISON).all())
    assert _abi_call(lib, D, B, nch, n_fb, 25, 0, fb, fr, ve, fv, stride) == 0       # no rows: zeros
    out = fv.cpu().numpy().reshape(B, stride)
    assert not out[:, :nF * nV].any() and (out[:, nF * nV:] == POISON).all()
    with pytest.raises(ValueError, match="math domain error"):
        from das_diff_veh_amd.disp import SlantPlan
        SlantPlan(25, 500, DX, DT500, freqs, [300.0, 0.0])
    assert ctypes.CDLL(_lib.LIB_PATH).dvh_abi_version() == 2
