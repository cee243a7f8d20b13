"""Which f-v sampling kernel runs, decided on the host: das_diff_veh_amd.disp.fv_choice (mfma, cells, else the
dvh_disp_fv chain) and dvh_disp_fv_pick (tiled, batched, per-image) at the shapes DESIGN.md names and on both sides of
every size threshold.  No GPU: the selection is arithmetic on the shape.  Nothing on the launch path reads the
environment."""
import ctypes
import glob
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DX, DT = 8.16, 0.003999999999997783
FORM = {"auto": 0, "per_image": 1, "not_tiled": 2, "batched": 3, "tiled": 4}  # include/dvh.h DVH_FV_*
NAME = {1: "per_image", 3: "batched", 4: "tiled"}


@pytest.fixture(scope="module")
def lib():
    from das_diff_veh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from das_diff_veh_amd.build import build
        build()
    return _lib


def _pick(lib, B, nF, nV, form="auto", ipb=0, n_kb=32, n_fb=100, sgl=25):
    f, g = ctypes.c_int32(-1), ctypes.c_int32(-1)
    lib.call("dvh_disp_fv_pick", B, n_kb, n_fb, nF, nV, sgl, FORM[form], ipb, ctypes.byref(f), ctypes.byref(g))
    return NAME.get(f.value, f.value), g.value


@pytest.fixture(scope="module")
def plans():
    from das_diff_veh_amd.disp import DispPlan
    mk = lambda nV, nF: DispPlan(25, 500, DX, DT, np.linspace(1.0, 25.0, nF), np.linspace(200.0, 1200.0, nV))  # noqa: E731
    return {"class": mk(1000, 242), "timelapse": mk(512, 1000)}


def test_fv_choice_at_the_design_shapes(lib, plans):
    """The bench's 3 class stacks of 1 000 x 242 keep the per-image kernel; 512 images of 512 x 1 000 (4 096 MFMA
    blocks) and the sliding bench's 1 512 of 1 000 x 242 (24 192) take the MFMA kernel."""
    from das_diff_veh_amd.disp import fv_choice
    assert fv_choice(plans["class"], 3) == ("per_image", 0)
    assert fv_choice(plans["timelapse"], 512) == ("mfma", 0)
    assert fv_choice(plans["class"], 1512) == ("mfma", 0)


def test_fv_choice_between_the_mfma_and_cell_thresholds(lib, plans):
    """MFMA_MIN_BLOCKS = 512 blocks of 64 velocities and the 4 096 blocks of (tile, 4 velocities, image) of the
    cell-staged kernel.  512 x 1 000: 8 MFMA blocks and 5 * 128 cell blocks per image, so 63 images (504, 40 320) run
    cells and 64 (512) mfma.  1 000 x 242: 16 and 1 * 250 per image, so 16 images (256, 4 000) stay with the chain,
    17 (272, 4 250) run cells, 31 (496) still, 32 (512) mfma."""
    from das_diff_veh_amd.disp import CELLS_MIN_BLOCKS, MFMA_MIN_BLOCKS, fv_choice
    assert (MFMA_MIN_BLOCKS, CELLS_MIN_BLOCKS) == (512, 4096)
    tl, cl = plans["timelapse"], plans["class"]
    assert [fv_choice(tl, B)[0] for B in (63, 64)] == ["cells", "mfma"]
    assert [fv_choice(cl, B)[0] for B in (16, 17, 31, 32)] == ["per_image", "cells", "cells", "mfma"]
    # named kernels run at any batch size, with the images per block asked for
    assert fv_choice(cl, 3, "mfma", 3) == ("mfma", 3) and fv_choice(cl, 3, "cells", 2) == ("cells", 2)
    assert fv_choice(tl, 512, "chain") == ("tiled", 40)      # 5 * 128 * 512 blocks over 8 192
    assert fv_choice(tl, 512, "not_tiled") == ("batched", 64)  # 128 chunks * 512 over 1 024
    assert fv_choice(tl, 512, "per_image") == ("per_image", 0)
    with pytest.raises(ValueError):
        fv_choice(tl, 512, "tile")


def test_fv_choice_needs_no_device(lib, plans, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: pytest.fail("fv_choice touched the device"))
    from das_diff_veh_amd.disp import fv_choice
    assert fv_choice(plans["class"], 3, "tiled")[0] == "tiled"
    assert not plans["class"]._dev


def test_pick_each_side_of_the_tiled_thresholds(lib):
    """work = B * tiles * ceil(nV / 4) >= 8 192 and tiles of TO >= 160 outputs.  nF = 200 is one tile of 200 and nV = 4
    one chunk, so work = B; nF = 156 and 157 round to tiles of 156 and 160.  Below either threshold the batched
    kernel takes the 8 191 / 8 192 (chunk, image) pairs, 8 images per block."""
    assert _pick(lib, 8192, 200, 4) == ("tiled", 1)
    assert _pick(lib, 8191, 200, 4) == ("batched", 8)
    assert _pick(lib, 8192, 157, 4) == ("tiled", 1)
    assert _pick(lib, 8192, 156, 4) == ("batched", 8)
    # 5 tiles * 128 chunks: 12 images are 7 680 units, 13 are 8 320 (2 images per block of ~8 k blocks)
    assert _pick(lib, 12, 1000, 512) == ("batched", 2)
    assert _pick(lib, 13, 1000, 512) == ("tiled", 2)
    # the named kernel ignores the threshold; "not_tiled" never tiles
    assert _pick(lib, 1, 156, 4, "tiled") == ("tiled", 1)
    assert _pick(lib, 1, 156, 4, "tiled", 3) == ("tiled", 3)
    assert _pick(lib, 8192, 200, 4, "not_tiled") == ("batched", 8)


def test_pick_each_side_of_the_batched_threshold(lib):
    """B * chunks >= 1 024 for the batched kernel: nF = 1 000 leaves one 4-velocity group per block, nV = 4 one
    chunk, and 5 tiles keep the work (5 B) under 8 192."""
    assert _pick(lib, 1024, 1000, 4) == ("batched", 1)
    assert _pick(lib, 1023, 1000, 4) == ("per_image", 0)
    assert _pick(lib, 1024, 1000, 4, "not_tiled") == ("batched", 1)
    assert _pick(lib, 1023, 1000, 4, "not_tiled") == ("per_image", 0)
    assert _pick(lib, 1, 1000, 4, "batched") == ("batched", 1)
    assert _pick(lib, 1, 1000, 4, "batched", 16) == ("batched", 16)
    assert _pick(lib, 4096, 1000, 4, "per_image") == ("per_image", 0)
    assert _pick(lib, 1, 1025, 4, "batched") == ("per_image", 0)  # more frequencies than the block's 1 024 threads


def test_pick_above_the_staged_grid_sizes(lib):
    """6 400 bins: above the batched kernel's 4 096, within the tiled kernel's 64 KB.  12 700 bins: above both.  A
    named kernel that cannot hold the grid falls through, tiled -> batched -> per-image."""
    big = dict(n_kb=64, n_fb=100)
    assert _pick(lib, 8192, 200, 4, **big) == ("tiled", 1)
    assert _pick(lib, 8192, 200, 4, "not_tiled", **big) == ("per_image", 0)
    assert _pick(lib, 8192, 200, 4, "batched", 3, **big) == ("per_image", 0)
    assert _pick(lib, 3, 200, 4, "tiled", **big) == ("tiled", 1)
    huge = dict(n_kb=127, n_fb=100)
    for form in FORM:
        assert _pick(lib, 8192, 200, 4, form, **huge) == ("per_image", 0), form


def test_window_each_side_of_the_tile_halo(lib):
    """A tiled block samples 12 frequencies to either side of its tile, so the tiled kernels filter windows up to 25.
    At 27 the chain goes on to the batched kernel, by size and when "tiled" is named (which keeps the batched kernel
    named: 3 images run it too); DispPlan.cell_tables refuses the plan, so "cells" takes the chain's choice by size;
    dvh_disp_fv_cells_as answers -4 before it touches its pointers."""
    from das_diff_veh_amd.disp import DispPlan, fv_choice
    for sgl in (5, 23, 25):
        assert _pick(lib, 8192, 200, 4, sgl=sgl) == ("tiled", 1), sgl
        assert _pick(lib, 3, 413, 9, "tiled", 3, sgl=sgl) == ("tiled", 3), sgl
    assert _pick(lib, 8192, 200, 4, sgl=27) == ("batched", 8)
    assert _pick(lib, 3, 413, 9, "tiled", 3, sgl=27) == ("batched", 1)
    assert _pick(lib, 3, 47, 9, "tiled", 3, sgl=27) == ("batched", 1)
    assert _pick(lib, 3, 413, 9, sgl=27) == ("per_image", 0)
    mk = lambda w, nF=413: DispPlan(25, 500, DX, DT, np.linspace(1.0, 25.0, nF), np.linspace(200.0, 1200.0, 9),  # noqa: E731
                                    sg_window=w)
    for w in (5, 23, 25):
        assert mk(w).cell_tables() is not None
        assert fv_choice(mk(w), 3, "cells", 3) == ("cells", 3) and fv_choice(mk(w), 3, "tiled", 3) == ("tiled", 3)
    wide = mk(27)
    assert wide.cell_tables() is None
    assert fv_choice(wide, 3, "cells", 3) == ("per_image", 0)
    assert fv_choice(wide, 3, "tiled", 3) == ("batched", 1)
    assert fv_choice(wide, 3, "batched", 3) == ("batched", 3) and fv_choice(wide, 3) == ("per_image", 0)
    # 4 096 images are 36 864 cell blocks: cells by size at 23, the batched kernel (8 192 chunks over 1 024) at 27
    assert fv_choice(mk(23), 4096) == ("cells", 0) and fv_choice(wide, 4096) == ("batched", 8)
    ct = mk(25).cell_tables()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    args = lambda sgl: (p, 3, 32, 100, p, 0.0, 1.0, p, 413, 9, p, p, sgl, ct["TO"], ct["n_tile"], 4, ct["max_cell"],  # noqa: E731
                        p, p, p, p, 0, None)
    with pytest.raises(ValueError, match="savgol window wider"):
        lib.call("dvh_disp_fv_cells_as", *args(27))
    with pytest.raises(ValueError, match="savgol window must be odd"):
        lib.call("dvh_disp_fv_cells_as", *args(24))


def test_pick_statuses(lib):
    """-4 (ValueError) for a window the kernels cannot filter and for more frequencies than the per-image kernel's
    160 KB of LDS hold (20 bytes each: 8 192); -2 for an unknown form; nothing to run reports form 0."""
    assert _pick(lib, 1, 8192, 4) == ("per_image", 0)
    with pytest.raises(ValueError, match="too many frequencies"):
        _pick(lib, 1, 8193, 4)
    with pytest.raises(ValueError, match="savgol window"):
        _pick(lib, 1, 200, 4, sgl=24)
    with pytest.raises(ValueError, match="savgol window"):
        _pick(lib, 1, 20, 4)
    f, g = ctypes.c_int32(), ctypes.c_int32()
    with pytest.raises(lib.DvhError, match="unknown f-v form"):
        lib.call("dvh_disp_fv_pick", 1, 32, 100, 200, 4, 25, 5, 0, ctypes.byref(f), ctypes.byref(g))
    assert _pick(lib, 0, 200, 4) == (0, 0) and _pick(lib, 3, 200, 0) == (0, 0)


def test_no_launch_reads_the_environment():
    """No getenv in the native sources; the dispersion, stack and staging modules do not read os.environ (the
    package's remaining reads say where the library and the compiler are, and engine.py's documented opt-in)."""
    srcs = sorted(glob.glob(os.path.join(ROOT, "das_diff_veh_amd", "csrc", "*")))
    assert len(srcs) > 10
    for path in srcs:
        assert "getenv" not in open(path).read(), path
    for mod in ("disp.py", "vsg.py", "device.py"):
        assert "environ" not in open(os.path.join(ROOT, "das_diff_veh_amd", mod)).read(), mod
