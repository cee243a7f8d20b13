"""GPU parity of the batched f-v sampling kernel (fv_batch_kernel) on BASELINE configs[4]'s grid:
512 velocities x 1,000 frequencies, many images per launch (weights reused across the images of a
block), against the oracle's map_fv (modules/utils.py:457-475): rel-err <= 1e-4, picks per the
SURVEY §8(d) tie rule."""
import numpy as np
import pytest

from tests import disp_shapes as ds

pytestmark = pytest.mark.gpu
TOL = 1e-4


# 40 images of 512 x 1 000 are 20 480 cell blocks and 320 MFMA blocks: by size the product takes the cell-staged
# kernel, dvh_disp_fv's own chain the tiled one (work 25 600 >= 8 192, tiles of 200), without it the batched one
BY_SIZE_40 = {None: "cells", "not_tiled": "batched", "chain": "tiled"}
# nF = 25 < 32: the MFMA kernel needs two 16-frequency tiles, so 3 images take the product's choice, per-image
FALLS_NF25 = {"mfma": "per_image"}


@pytest.mark.parametrize("mode", ds.FV_MODES)
@pytest.mark.parametrize("B,nv,nf", [(40, 512, 1000), (7, 300, 242), (5, 64, 1001), (3, 61, 25), (4, 33, 413),
                                     (3, 17, 32), (2, 16, 40), (5, 70, 47)])
def test_fv_batch_vs_oracle(device, B, nv, nf, mode):
    """mode: the kernel named to fv_maps (tests/disp_shapes.py FV_MODES) -- None = the product's choice, "tiled" the
    frequency-tiled kernel, "not_tiled" batched / per-image by size, "batched" with 3 and 16 images per block,
    "per_image", "cells" and "mfma" (where it applies, nF >= 32) with the launcher's and with 3 images per block,
    "chain" dvh_disp_fv's own choice.  fv_choice must name that kernel: at (40, 512, 1000) every mode its namesake."""
    from das_diff_veh_amd.disp import DispPlan, fv_maps
    from das_diff_veh_amd.synth import synth_gathers
    from oracle import disp as odisp
    nch, nt, dx, dt = 25, 500, 8.16, 0.003999999999997783
    freqs, vels = np.linspace(1.0, 25.0, nf), np.linspace(200.0, 1200.0, nv)
    plan = DispPlan(nch, nt, dx, dt, freqs, vels)
    ds.check_fv_choice(plan, B, mode, BY_SIZE_40 if B == 40 else ds.FV_FEW_IMAGES, FALLS_NF25 if nf == 25 else ())
    data = synth_gathers(B, nch, nt, dx, dt, device, seed=B)
    got = fv_maps(data, plan, **ds.fv_mode_kwargs(mode)).double().cpu().numpy()
    host = data.double().cpu().numpy()
    for b in sorted({0, 1, B // 2, B - 1}):
        ref = odisp.map_fv(host[b], dx, dt, freqs, vels)
        assert np.abs(got[b] - ref).max() / np.abs(ref).max() < TOL, b
        assert np.all(odisp.pick_ok(ref, got[b].argmax(axis=0))), b


# Savitzky-Golay windows other than the reference's 25: 5 the smallest (order 4), 23 the largest below the unrolled
# 25-tap path, 27 the smallest a tile's 12-frequency halo does not cover -- there "tiled" runs the batched kernel and
# "cells" (no cell tables) the choice by size.  "mfma" is built for 25 only.
WINDOW_MODES = [None, ("per_image", 0), ("batched", 3), ("tiled", 3), ("cells", 3)]
FALLS_W27 = {"tiled": "batched", "cells": "per_image"}
_WINDOW_REF = {}


def _window_case(nf, w, device):
    """(data, freqs, vels, oracle maps of images 0 and B - 1): made once per (nF, window), shared by the modes."""
    from das_diff_veh_amd.synth import synth_gathers
    from oracle import disp as odisp
    if (nf, w) not in _WINDOW_REF:
        B, nv, nch, nt, dx, dt = 3, 9, 25, 500, 8.16, 0.003999999999997783
        freqs, vels = np.linspace(1.0, 25.0, nf), np.linspace(200.0, 1200.0, nv)
        data = synth_gathers(B, nch, nt, dx, dt, device, seed=B)
        host = data.double().cpu().numpy()
        refs = {b: odisp.map_fv(host[b], dx, dt, freqs, vels, sg_window=w) for b in (0, B - 1)}
        _WINDOW_REF[(nf, w)] = (data, freqs, vels, refs)
    return _WINDOW_REF[(nf, w)]


@pytest.mark.parametrize("mode", WINDOW_MODES)
@pytest.mark.parametrize("w", [5, 23, 27])
@pytest.mark.parametrize("nf", [47, 413])
def test_fv_window_vs_oracle(device, nf, w, mode):
    """3 images of 9 velocities (a partial chunk of 4) x 47 frequencies (one tile) and 413 (three tiles of 140, the
    last of 133; two velocity groups in the batched kernel), nF % 4 != 0, at windows 5, 23 and 27: the rolled filter
    branch of the batched and the tiled kernels and the per-image kernel against oracle.map_fv at that window.  No
    pick assertion: SURVEY §8(d) states the pick contract for the reference's window."""
    from das_diff_veh_amd.disp import DispPlan, fv_maps
    data, freqs, vels, refs = _window_case(nf, w, device)
    B = data.shape[0]
    plan = DispPlan(25, 500, 8.16, 0.003999999999997783, freqs, vels, sg_window=w)
    ds.check_fv_choice(plan, B, mode, ds.FV_FEW_IMAGES, FALLS_W27 if w == 27 else ())
    got = fv_maps(data, plan, **ds.fv_mode_kwargs(mode)).double().cpu().numpy()
    for b, ref in refs.items():
        err = np.abs(got[b] - ref).max() / np.abs(ref).max()
        print(f"fv window {w} nF {nf} {mode} image {b}: rel-err {err:.3g}")
        assert err < TOL, b
