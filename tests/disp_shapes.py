"""Gather geometries of the dispersion shape tests (tests/test_disp_shapes_host.py pins the plan arithmetic on the
host, tests/test_disp_shapes_gpu.py runs the kernels at them).  dx = 8.16 m, dt = 0.004 s, freqs 1-25 Hz and
vels 200-1200 m/s unless a row says otherwise; the numbers are what DispPlan must derive:

  (nch, nt): nk, n_kb, n_fb, MT, K2

The |FK| grid has n_kb * n_fb bins.  The sampling kernels stage it: the batched kernel up to 4 096 bins, the MFMA
kernel up to 8 192, the frequency-tiled kernel up to 64 KB of LDS (about 7 900 bins); above them the per-image
kernel runs.  The contraction kernel keeps [K2][33] + [2 MT][33] doubles in LDS up to 160 KB and tiles above it.
"""
import numpy as np

DX, DT = 8.16, 0.004
FK_LDS_LIMIT = 160 * 1024

GEOMETRIES = {
    (1, 500): dict(nk=2, n_kb=2, n_fb=100, MT=16, K2=4),
    (2, 64): dict(nk=4, n_kb=2, n_fb=14, MT=16, K2=4),
    (15, 250): dict(nk=32, n_kb=16, n_fb=51, MT=16, K2=32),
    (16, 256): dict(nk=32, n_kb=16, n_fb=51, MT=16, K2=32),
    (17, 257): dict(nk=64, n_kb=32, n_fb=100, MT=32, K2=36),
    (25, 8): dict(nk=64, n_kb=32, n_fb=3, MT=32, K2=52),
    (25, 31): dict(nk=64, n_kb=32, n_fb=8, MT=32, K2=52),
    (33, 499): dict(nk=128, n_kb=64, n_fb=100, MT=64, K2=68),
    (65, 500): dict(nk=256, n_kb=127, n_fb=100, MT=128, K2=132),
    (25, 2000): dict(nk=64, n_kb=32, n_fb=395, MT=32, K2=52),
    (128, 500): dict(nk=256, n_kb=127, n_fb=100, MT=128, K2=256),
    (129, 500): dict(nk=512, n_kb=253, n_fb=100, MT=256, K2=260),
    (300, 500): dict(nk=1024, n_kb=506, n_fb=100, MT=512, K2=600),
}
# the contraction's LDS bytes when one block holds the whole operand and result
FK_LDS = {(1, 500): 9504, (2, 64): 9504, (15, 250): 16896, (16, 256): 16896, (17, 257): 26400, (25, 8): 30624,
          (25, 31): 30624, (33, 499): 51744, (65, 500): 102432, (25, 2000): 30624, (128, 500): 135168,
          (129, 500): 203808, (300, 500): 428736}
TILED = [(129, 500), (300, 500)]  # above FK_LDS_LIMIT: fk_contract_tiled_kernel

# the public fk() forms the full grid: n_kb = MT = nk, 16 samples give nf = n_fb = 32
FULL_GRID = {64: dict(nk=128, K2=128, lds=101376), 65: dict(nk=256, K2=132, lds=170016),
             130: dict(nk=512, K2=260, lds=338976)}

# 200 channels at dx = 3 m (wavenumbers below Nyquist): n_kb = 193 = 3 * 64 + 1 and MT = 208 = 3 * 64 + 16, so the
# tiled kernel's last block has one wavenumber and three of its four 16-row MFMA tiles lie outside the table
RAGGED = dict(nch=200, nt=64, dx=3.0, nk=512, n_kb=193, n_fb=14, MT=208, K2=400)


# The kernel selections the f-v sampling tests run: None = the product's choice, else (form, images_per_block) of
# das_diff_veh_amd.disp.fv_choice.  "not_tiled" and "chain" name no kernel, they narrow the choice made by size.
FV_MODES = [None, ("tiled", 0), ("not_tiled", 0), ("batched", 3), ("batched", 16), ("tiled", 3), ("per_image", 0),
            ("cells", 3), ("chain", 0), ("mfma", 0), ("mfma", 3)]
FV_FEW_IMAGES = {None: "per_image", "not_tiled": "per_image", "chain": "per_image"}  # a few small images, by size


def fv_mode_kwargs(mode):
    return {} if mode is None else dict(form=mode[0], images_per_block=mode[1])


def check_fv_choice(plan, B, mode, by_size=FV_FEW_IMAGES, falls=()):
    """fv_choice under ``mode`` names the kernel asked for, with the images per block asked for -- or, for a form
    listed in ``falls`` (a structural condition of that kernel fails at this shape), the kernel named there; the
    modes that name no kernel give ``by_size``'s.  Returns the kernel's name."""
    from das_diff_veh_amd.disp import fv_choice
    form, ipb = (None, 0) if mode is None else mode
    name, G = fv_choice(plan, B, **fv_mode_kwargs(mode))
    want = by_size[form] if form in by_size else dict(falls).get(form, form)
    assert name == want, (mode, name, want)
    if name == form and ipb:
        assert G == ipb, (mode, G)
    return name


def axes(nF=47, nV=33):
    return np.linspace(1.0, 25.0, nF), np.linspace(200.0, 1200.0, nV)


def fk_lds_bytes(plan):
    return 8 * 33 * (plan.K2 + 2 * plan.MT)
