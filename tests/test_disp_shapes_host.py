"""Host check of the plan arithmetic behind tests/test_disp_shapes_gpu.py: the GPU cases pick their gather shapes for
the kernel paths those shapes select (MFMA tile padding, the sampling kernels' staging limits, the tiled
contraction); if DispPlan derived other grids the GPU cases would go on passing while testing another dispatch."""
import pytest

from tests import disp_shapes as ds


@pytest.mark.parametrize("geom", sorted(ds.GEOMETRIES))
def test_disp_plan_geometry_table(geom):
    from das_diff_veh_amd.disp import DispPlan
    nch, nt = geom
    want = ds.GEOMETRIES[geom]
    freqs, vels = ds.axes()
    p = DispPlan(nch, nt, ds.DX, ds.DT, freqs, vels)
    assert dict(nk=p.nk, n_kb=p.n_kb, n_fb=p.n_fb, MT=p.MT, K2=p.K2) == want
    assert p.wt.shape == (nt, 2 * p.n_fb) and p.atab.shape == (2 * p.MT, p.K2)
    assert ds.fk_lds_bytes(p) == ds.FK_LDS[geom]
    assert (ds.fk_lds_bytes(p) > ds.FK_LDS_LIMIT) == (geom in ds.TILED)
    # the grid does not depend on how finely the same (f, v) ranges are sampled
    q = DispPlan(nch, nt, ds.DX, ds.DT, *ds.axes(260, 70))
    assert (q.n_kb, q.n_fb, q.m_lo, q.j_lo) == (p.n_kb, p.n_fb, p.m_lo, p.j_lo)


def test_disp_plan_bins_against_sampling_limits():
    """Each geometry of the f-v cases lies on its side of the batched kernel's 4 096 bins and the MFMA kernel's
    8 192; the frequency-tiled kernel's 64 KB of LDS holds the 6 400-bin grid and not the 12 640-bin ones."""
    bins = {g: v["n_kb"] * v["n_fb"] for g, v in ds.GEOMETRIES.items()}
    assert bins[(1, 500)] == 200 and bins[(17, 257)] == 3200 and bins[(33, 499)] == 6400
    assert bins[(65, 500)] == 12700 and bins[(25, 2000)] == 12640
    assert bins[(129, 500)] == 25300 and bins[(300, 500)] == 50600
    assert bins[(17, 257)] <= 4096 < bins[(33, 499)] <= 8192 < bins[(25, 2000)] < bins[(65, 500)]

    def tile_lds(n):  # dvh_disp_fv's lds_t: the grid, the 25 x 25 savgol operator, 4 velocity rows of samples
        return 8 * ((n + 1) & ~1) + 8 * ((25 * 25 + 1) & ~1) + 4 * 4 * (2 * 12 + 256 + 4)
    assert tile_lds(bins[(33, 499)]) <= 64 * 1024 < tile_lds(bins[(25, 2000)])


@pytest.mark.parametrize("nch", sorted(ds.FULL_GRID))
def test_full_grid_plan_of_public_fk(nch):
    from das_diff_veh_amd.disp import DispPlan
    want = ds.FULL_GRID[nch]
    p = DispPlan(nch, 16, ds.DX, ds.DT, [1.0] * 25, [1.0], full_grid=True)
    assert (p.nk, p.nf, p.n_kb, p.n_fb, p.MT, p.K2) == (want["nk"], 32, want["nk"], 32, want["nk"], want["K2"])
    assert ds.fk_lds_bytes(p) == want["lds"]
    assert (want["lds"] > ds.FK_LDS_LIMIT) == (nch >= 65)


def test_ragged_tiled_geometry():
    from das_diff_veh_amd.disp import DispPlan
    r = ds.RAGGED
    p = DispPlan(r["nch"], r["nt"], r["dx"], ds.DT, *ds.axes())
    assert dict(nk=p.nk, n_kb=p.n_kb, n_fb=p.n_fb, MT=p.MT, K2=p.K2) == {k: r[k] for k in ("nk", "n_kb", "n_fb", "MT", "K2")}
    assert ds.fk_lds_bytes(p) > ds.FK_LDS_LIMIT and p.MT % 64 == 16 and p.n_kb % 64 == 1
