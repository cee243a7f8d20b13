"""dvh_rayleigh_sens on the device against the 80-digit oracle's derivatives (tests/golden/rayleigh_sens.npz,
tests/rayleigh_sens_ref.py): every case, period and mode, Euler's identities, the half-space, models of more than 64
and 128 directions, batches, the column mask, null outputs, padding rows and the Python fronts.

Errors are dimensionless as in tests/test_rayleigh_sens_host.py, |p (got - want)| / c, and held to its BOUND: ten
times the worst error measured on the host path."""
import numpy as np
import pytest
import torch

from tests import rayleigh_ref as ref
from tests import rayleigh_sens_ref as sref
from tests.test_rayleigh_sens_host import BOUND

pytestmark = pytest.mark.gpu

TOL = 1e-9  # the width dvh_rayleigh_modes refines to, and the bound on |c - c_ref| / c_ref
POISON = -777.25
PERIODS = np.array([1.0 / f for f in ref.FREQS])


@pytest.fixture(scope="module")
def golden():
    return sref.load_sens()


def modes(device, layers, periods, n_mode, c_min, dc=ref.DC):
    """dvh_rayleigh_modes, every mode wanted at every period -> c [M, P, n_mode] on the device."""
    from das_diff_veh_amd import _lib
    M, n_layer, _ = layers.shape
    need = torch.full((periods.numel(),), n_mode, dtype=torch.int32, device=device)
    c = torch.full((M, periods.numel(), n_mode), POISON, dtype=torch.float64, device=device)
    count = torch.empty((M, periods.numel()), dtype=torch.int32, device=device)
    _lib.call("dvh_rayleigh_modes", _lib.ptr(layers), M, n_layer, _lib.ptr(periods), periods.numel(), _lib.ptr(need),
              c_min, dc, TOL, n_mode, _lib.ptr(c), _lib.ptr(count), _lib.stream_of(device))
    return c


def sens(device, layers, periods, n_mode, c_min, par_mask=15, outputs="cup", c_in=None):
    """One dvh_rayleigh_sens launch over poisoned outputs on the roots of dvh_rayleigh_modes (or on c_in) ->
    dict(c_in, c, u, p) as NumPy, None for an output not in `outputs`."""
    from das_diff_veh_amd import _lib
    layers = np.ascontiguousarray(layers, np.float64)
    layers = layers[None] if layers.ndim == 2 else layers
    M, n_layer, _ = layers.shape
    L = torch.from_numpy(layers).to(device)
    T = torch.from_numpy(np.ascontiguousarray(periods, np.float64)).to(device)
    c = modes(device, L, T, n_mode, c_min) if c_in is None else torch.from_numpy(np.ascontiguousarray(c_in)).to(device)
    assert c.shape == (M, T.numel(), n_mode)
    out = {"c": torch.full_like(c, POISON) if "c" in outputs else None,
           "u": torch.full_like(c, POISON) if "u" in outputs else None,
           "p": torch.full(c.shape + (n_layer, 4), POISON, dtype=torch.float64, device=device)
           if "p" in outputs else None}
    _lib.call("dvh_rayleigh_sens", _lib.ptr(L), M, n_layer, _lib.ptr(T), T.numel(), _lib.ptr(c), n_mode, par_mask,
              TOL, _lib.ptr(out["c"]), _lib.ptr(out["u"]), _lib.ptr(out["p"]), _lib.stream_of(device))
    res = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    for v in res.values():
        assert v is None or not (v == POISON).any()  # no slot is left unwritten
    res["c_in"] = c.cpu().numpy()
    return res


def omega_c_omega(c, u):
    """omega dc/domega from U = c / (1 - (omega / c) dc/domega)."""
    return c * (1.0 - c / u)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def perturbed_notebooks(n, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        m = ref.CASES["notebook"][0]
        out.append(ref.make_layers(m[:-1, 0] * rng.uniform(0.8, 1.25, 5), m[:, 2] * rng.uniform(0.9, 1.1, 6)))
    return np.stack(out)


@pytest.mark.parametrize("name", list(ref.CASES) + ["grazing"])
def test_sens_matches_the_oracle(device, golden, name):
    """Every recorded period and mode of a case in one launch: dc/dp and U within BOUND, the polished root within
    1e-9, NaN exactly where the root is NaN."""
    if name == "grazing":
        g = golden["grazing"]
        layers, periods, n_mode = ref.CASES[sref.GRAZING_LAYERS][0], np.array([1.0 / g["freq"]]), sref.GRAZING_MODES
        want, c_min = [(g["c"], g["dcdw"], g["dcdp"])], g["c_min"]
    else:
        layers, periods, n_mode = ref.CASES[name][0], PERIODS, sref.MAX_MODES
        want, c_min = [golden[name, i] for i in range(len(ref.FREQS))], ref.c_min_of(name)
    r = sens(device, layers, periods, n_mode, c_min)
    worst = 0.0
    for i, (c, dcdw, dcdp) in enumerate(want):
        n, omega = c.size, 2.0 * np.pi / periods[i]
        for k in ("c_in", "c", "u"):
            assert np.isfinite(r[k][0, i, :n]).all() and np.isnan(r[k][0, i, n:]).all(), (name, i, k)
        assert np.isfinite(r["p"][0, i, :n]).all() and np.isnan(r["p"][0, i, n:]).all(), (name, i)
        if n == 0:
            continue
        got_c, got_u, got_p = r["c"][0, i, :n], r["u"][0, i, :n], r["p"][0, i, :n]
        assert (np.abs(got_c - c) <= TOL * c).all(), (name, i)
        want_u = c / (1.0 - omega / c * dcdw)
        e = max((np.abs(layers[None] * (got_p - dcdp)) / c[:, None, None]).max(),
                (np.abs(omega_c_omega(got_c, got_u) - omega * dcdw) / c).max(),
                (np.abs(got_u - want_u) / want_u).max())
        worst = max(worst, e)
        assert e <= BOUND, (name, i, e)
    print(f"{name}: largest dimensionless error {worst:.2e} (bound {BOUND:.2e})")


def test_eulers_identities(device):
    """c is homogeneous of degree 0 in (h, 1 / omega) and in rho and of degree 1 in (alpha, beta, omega); no oracle:
    sum h c_h = omega c_omega,  sum (alpha c_alpha + beta c_beta) + omega c_omega = c,  sum rho c_rho = 0."""
    models = perturbed_notebooks(7)
    r = sens(device, models, PERIODS[[1, 2, 4]], 3, 0.1)
    ok = np.isfinite(r["c"])
    assert ok.sum() >= 50 and same(np.isnan(r["u"]), ~ok)
    w = models[:, None, None] * r["p"]  # p_l dc/dp_l
    c, wcw = r["c"], omega_c_omega(r["c"], r["u"])
    worst = 0.0
    for e in (w[..., 0].sum(-1) - wcw, w[..., 1].sum(-1) + w[..., 2].sum(-1) + wcw - c, w[..., 3].sum(-1)):
        worst = max(worst, (np.abs(e[ok]) / c[ok]).max())
        assert (np.abs(e[ok]) <= BOUND * c[ok]).all(), (np.abs(e[ok]) / c[ok]).max()
    print(f"Euler identities: largest residual over c {worst:.2e} (bound {BOUND:.2e})")


@pytest.mark.parametrize("name", ["halfspace1", "halfspace3"])
def test_half_space_has_no_dispersion(device, name):
    """U = c, c_h = 0 and alpha c_alpha + beta c_beta = c (summed over the rows of the three-row half-space)."""
    layers = ref.CASES[name][0]
    r = sens(device, layers, PERIODS, 1, ref.c_min_of(name))
    c, u, p = r["c"][0, :, 0], r["u"][0, :, 0], r["p"][0, :, 0]
    assert np.isfinite(c).all()
    assert (np.abs(u - c) <= BOUND * c).all()
    assert (np.abs(layers[None, :, 0] * p[:, :, 0]) <= BOUND * c[:, None]).all()
    assert (np.abs((layers[None, :, 1:3] * p[:, :, 1:3]).sum((1, 2)) - c) <= BOUND * c).all()


@pytest.mark.parametrize("n_rows", [16, 32])
def test_more_directions_than_lanes(device, n_rows):
    """The notebook case cut into 16 rows (2 + 64 directions: a second round of two lanes) and into 32 rows (2 + 128:
    three rounds): every sub-row's c_h is its parent layer's, the sub-rows' c_alpha, c_beta and c_rho add up to the
    parent's, and U and the root are the six-row model's."""
    six = ref.CASES["notebook"][0]
    cuts = {16: [3, 3, 3, 3, 3], 32: [7, 6, 6, 6, 6]}[n_rows]
    rows, parent = [], []
    for l, n in enumerate(cuts):
        rows += [six[l] * [1.0 / n, 1.0, 1.0, 1.0]] * n
        parent += [l] * n
    cut = np.array(rows + [six[-1]])
    parent = np.array(parent + [5])
    assert cut.shape == (n_rows, 4)
    a = sens(device, six, PERIODS, 3, 0.1)
    b = sens(device, cut, PERIODS, 3, 0.1)
    ok = np.isfinite(a["c"][0])
    assert ok.sum() >= 12 and same(np.isfinite(b["c"][0]), ok)
    c = a["c"][0][ok]
    assert (np.abs(b["c"][0][ok] - c) <= BOUND * c).all() and (np.abs(b["u"][0][ok] - a["u"][0][ok]) <= BOUND * c).all()
    pa, pb = a["p"][0][ok], b["p"][0][ok]  # [n_root, rows, 4]
    assert (np.abs(six[parent, 0] * (pb[:, :, 0] - pa[:, parent, 0])) <= BOUND * c[:, None]).all()
    summed = np.stack([pb[:, parent == l, 1:].sum(1) for l in range(6)], 1)
    assert (np.abs(six[None, :, 1:] * (summed - pa[:, :, 1:])) <= BOUND * c[:, None, None]).all()


def batch_models():
    from tests.test_rayleigh_gpu import padded
    names = ["halfspace3", "one_layer", "notebook", "lvz", "dyadic"]
    return np.stack([padded(ref.CASES[n][0], 6) for n in names] + list(perturbed_notebooks(2)))


def test_batch_equals_single_launches(device):
    """7 models x 3 periods x 3 modes (63 waves, not a multiple of the block's 4): each wave equals its own launch bit
    for bit, the NaN ones included."""
    models = batch_models()
    periods = PERIODS[[0, 2, 4]]
    r = sens(device, models, periods, 3, 0.12)
    assert np.isnan(r["c"]).any() and np.isfinite(r["c"]).sum() > 40
    for a in range(7):
        for b in range(3):
            for m in range(3):
                one = sens(device, models[a], periods[b:b + 1], 1, 0.12, c_in=r["c_in"][a:a + 1, b:b + 1, m:m + 1])
                for k in "cup":
                    assert same(one[k][0, 0, 0], r[k][a, b, m]), (a, b, m, k)


def test_column_mask(device):
    """par_mask = 4, the notebook's velocity_s call: that column equals the full call's bit for bit, the others are
    NaN, and so for every other mask."""
    layers = ref.CASES["notebook"][0]
    full = sens(device, layers, PERIODS, 3, 0.1)
    for mask in (4, 1, 2, 8, 5, 10, 14, 0):
        r = sens(device, layers, PERIODS, 3, 0.1, par_mask=mask)
        assert same(r["c"], full["c"]) and same(r["u"], full["u"])
        for q in range(4):
            if (mask >> q) & 1:
                assert same(r["p"][..., q], full["p"][..., q]), (mask, q)
            else:
                assert np.isnan(r["p"][..., q]).all(), (mask, q)


def test_null_outputs(device):
    """Every output may be null, alone or with another: the rest equal the full call's bit for bit."""
    layers = ref.CASES["lvz"][0]
    full = sens(device, layers, PERIODS, 4, 0.144)
    for outputs in ("up", "cp", "cu", "c", "u", "p"):
        r = sens(device, layers, PERIODS, 4, 0.144, outputs=outputs)
        for k in "cup":
            assert (r[k] is None) == (k not in outputs)
            assert r[k] is None or same(r[k], full[k]), (outputs, k)


def test_padding_rows(device):
    """Zero-thickness rows are skipped: 0 in their own rows and not a bit of difference in the real ones."""
    from tests.test_rayleigh_gpu import padded
    layers = ref.CASES["lvz"][0]
    a = sens(device, layers, PERIODS, 4, 0.144)
    b = sens(device, padded(layers, 9), PERIODS, 4, 0.144)
    ok = np.isfinite(a["c"])
    assert same(a["c"], b["c"]) and same(a["u"], b["u"]) and same(a["p"], b["p"][..., 5:, :])
    assert (b["p"][ok][:, :5] == 0.0).all() and np.isnan(b["p"][~ok]).all()
    assert (b["p"][ok][:, -1, 0] == 0.0).all()  # the half-space's h


def test_nan_roots_and_periods(device):
    """A NaN or non-positive root or period gives NaN in every output of that wave and leaves the others alone."""
    layers = ref.CASES["one_layer"][0]
    good = sens(device, layers, PERIODS[3:], 2, 0.16)
    assert np.isfinite(good["c"]).all()
    c_in = good["c_in"].copy()
    c_in[0, 0, 1], c_in[0, 1, 0] = np.nan, -0.3
    r = sens(device, layers, PERIODS[3:], 2, 0.16, c_in=c_in)
    bad = np.array([[[False, True], [True, False]]])
    for k in "cup":
        assert np.isnan(r[k][bad]).all() and same(r[k][~bad], good[k][~bad]), k
    r = sens(device, layers, [PERIODS[3], 0.0], 2, 0.16, c_in=good["c_in"])
    for k in "cup":
        assert np.isnan(r[k][0, 1]).all() and same(r[k][0, 0], good[k][0, 0]), k


# ------------------------------------------------------------------------------------------------------ the Python fronts

def test_python_fronts(device, golden):
    from das_diff_veh_amd import inversion as inv
    layers = ref.CASES["notebook"][0]
    L, T = torch.from_numpy(layers[None]).to(device), torch.from_numpy(PERIODS).to(device)
    k, c = inv.rayleigh_sensitivity(L, T, 3, return_modes=True)
    u = inv.rayleigh_group(L, T, 3)
    assert k.shape == (1, 5, 3, 6, 4) and c.shape == u.shape == (1, 5, 3) and k.is_cuda and u.is_cuda
    # dc = 0.005 (the default) and the default c_min find the recorded roots: the oracle's derivatives again
    for i in range(5):
        gc, gw, gp = golden["notebook", i]
        n = min(gc.size, 3)
        cc = c[0, i, :n].cpu().numpy()
        assert (np.abs(layers[None] * (k[0, i, :n].cpu().numpy() - gp[:n])) <= BOUND * cc[:, None, None]).all()
        want_u = gc[:n] / (1.0 - gw[:n] * 2.0 * np.pi / PERIODS[i] / gc[:n])
        assert (np.abs(u[0, i, :n].cpu().numpy() - want_u) <= BOUND * want_u).all()
    # the parameter names select and order the columns
    ks = inv.rayleigh_sensitivity(L, T, 3, parameters=("velocity_s", "thickness"))
    assert ks.shape == (1, 5, 3, 6, 2) and same(ks.cpu().numpy(), k[..., [2, 0]].cpu().numpy())
    # PhaseSensitivity, as the notebook calls it
    ps = inv.PhaseSensitivity(*layers.T)
    for mode in (0, 2):
        s = ps(PERIODS[2], mode=mode, wave="rayleigh", parameter="velocity_s")
        assert s._fields == ("depth", "kernel", "period", "velocity", "mode", "wave", "type", "parameter")
        assert (s.period, s.mode, s.wave, s.type, s.parameter) == (PERIODS[2], mode, "rayleigh", "phase", "velocity_s")
        assert np.array_equal(s.depth, np.r_[0.0, np.cumsum(layers[:-1, 0])])
        assert same(s.kernel, k[0, 2, mode, :, 2].cpu().numpy()) and s.velocity == float(c[0, 2, mode])
        s.kernel[-1:] = 0.0  # the notebook mutes the half-space
        assert s.kernel[-1] == 0.0
    assert np.isnan(ps(PERIODS[0], mode=5).kernel).all()  # no such mode at 2.5 Hz
    # group_velocity is rayleigh_group, for a reversed view too
    for mode in (0, 2):
        gv = inv.group_velocity(PERIODS, *layers.T, mode=mode)
        assert isinstance(gv, np.ndarray) and same(gv, u[0, :, mode].cpu().numpy())
        assert same(inv.group_velocity(PERIODS[::-1], *layers.T, mode=mode)[::-1], gv)
    with pytest.raises(RuntimeError):
        inv.rayleigh_group(L.cpu(), T.cpu(), 3)  # device tensors only


def test_value_errors_before_device_work():
    from das_diff_veh_amd import inversion as inv
    layers = ref.CASES["one_layer"][0]
    ps = inv.PhaseSensitivity(*layers.T)
    with pytest.raises(ValueError, match="rayleigh"):
        ps(0.1, wave="love")
    with pytest.raises(ValueError, match="parameter"):
        ps(0.1, parameter="vs")
    with pytest.raises(ValueError, match="mode"):
        ps(0.1, mode=16)
    with pytest.raises(ValueError, match="parameter"):
        inv.rayleigh_sensitivity(None, None, 1, parameters=("velocity_s", "poisson"))
    with pytest.raises(ValueError):
        inv.PhaseSensitivity([0.1, 0.0], [2.0, 2.0], [1.0, 1.0], [1.0])
