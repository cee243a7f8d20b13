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
