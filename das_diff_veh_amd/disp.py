"""Batched dispersion (f-v) transform on device: host tables + the three dvh_disp_* kernels.

Host side does only integer/float64 bookkeeping with the reference's own expressions:
  nf = 2 ** (1 + ceil(log(nt, 2))), nk = 2 ** (1 + ceil(log(nch, 2)))      modules/utils.py:239-240
  fft_f = arange(-nf/2, nf/2) / nf / dt, fft_k = arange(-nk/2, nk/2) / nk / dx  :242-243
  queries (k = f / v, f) sorted ascending per frequency (interp2d.__call__), clamped to the grid
  FITPACK degree-1 basis h = (t_hi - q, q - t_lo) / (t_hi - t_lo)
  savgol_filter(25, 4, mode='interp') as a linear operator: interior taps (savgol_coeffs) and the
  two edge polynomial-fit matrices (_fit_edge)
Every FLOP on the data runs in the kernels (das_diff_veh_amd/csrc/dvh_disp.hip, dvh_fv.hip).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import scipy.signal
import torch

from . import _lib


def fk_sizes(nch, nt):
    nf = 2 ** (1 + math.ceil(math.log(nt, 2)))
    nk = 2 ** (1 + math.ceil(math.log(nch, 2)))
    return nf, nk


def fk_axes(nch, nt, dx, dt):
    nf, nk = fk_sizes(nch, nt)
    return np.arange(-nf / 2, nf / 2) / nf / dt, np.arange(-nk / 2, nk / 2) / nk / dx


def _intervals(grid, q):
    """fpbisp: clamp to [grid[0], grid[-1]] and pick l with grid[l] <= q < grid[l+1], l <= n - 2."""
    q = np.clip(q, grid[0], grid[-1])
    l = np.clip(np.searchsorted(grid, q, side="right") - 1, 0, grid.size - 2)
    return q, l


def savgol_operator(window_length=25, polyorder=4):
    """(h, E_left, E_right) of scipy.signal.savgol_filter(..., mode='interp') as linear maps."""
    h = scipy.signal.savgol_coeffs(window_length, polyorder)
    half = window_length // 2
    vfit = np.vander(np.arange(window_length, dtype=np.float64), polyorder + 1)
    pinv = np.linalg.pinv(vfit)
    el = np.vander(np.arange(0, half, dtype=np.float64), polyorder + 1) @ pinv
    er = np.vander(np.arange(window_length - half, window_length, dtype=np.float64), polyorder + 1) @ pinv
    return h[::-1].copy(), el, er


class DispPlan:
    """Everything the kernels need for one (nch, nt, dx, dt, freqs, vels) geometry."""

    def __init__(self, nch, nt, dx, dt, freqs, vels, sg_window=25, sg_order=4, full_grid=False):
        self.nch, self.nt, self.dx, self.dt = int(nch), int(nt), float(dx), float(dt)
        self.freqs = np.asarray(freqs, dtype=np.float64)
        self.vels = np.asarray(vels, dtype=np.float64)
        self.nF, self.nV = self.freqs.size, self.vels.size
        if self.nF < sg_window:
            raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
        nf, nk = fk_sizes(nch, nt)
        self.nf, self.nk = nf, nk
        fft_f, fft_k = fk_axes(nch, nt, dx, dt)
        self.fft_f, self.fft_k = fft_f, fft_k

        # frequency direction: one scalar query per output column
        fq, j0 = _intervals(fft_f, self.freqs)
        ones = np.ones(self.nV)
        kq = np.stack([np.sort(np.divide(ones * fr, self.vels), kind="mergesort") for fr in self.freqs])
        kqc, m0 = _intervals(fft_k, kq)
        self._m0 = m0
        if full_grid:
            j_lo, j_hi, m_lo, m_hi = 0, nf - 1, 0, nk - 1
        else:
            j_lo, j_hi = int(j0.min()), int(j0.max()) + 1
            m_lo, m_hi = int(m0.min()), int(m0.max()) + 1
        self.j_lo, self.m_lo = j_lo, m_lo
        self.n_fb = j_hi - j_lo + 1
        self.n_kb = m_hi - m_lo + 1
        flo, fhi = fft_f[j0], fft_f[j0 + 1]
        fy = 1.0 / (fhi - flo)
        self.fj = (j0 - j_lo).astype(np.int32)
        self.fw = np.stack([fy * (fhi - fq), fy * (fq - flo)], axis=1)
        self.kq = np.ascontiguousarray(kq)
        self.kgrid = np.ascontiguousarray(fft_k[m_lo:m_hi + 1])
        self.kmin, self.kmax = float(fft_k[0]), float(fft_k[-1])

        # time-DFT twiddles for the needed bins nu = (j - nf/2) mod nf
        nu = (np.arange(j_lo, j_hi + 1) - nf // 2) % nf
        t = np.arange(nt)
        ang = 2.0 * np.pi * ((np.outer(t, nu) % nf) / nf)
        wt = np.empty((nt, 2 * self.n_fb))
        wt[:, 0::2] = np.cos(ang)
        wt[:, 1::2] = -np.sin(ang)
        self.wt = wt

        # channel-contraction block matrix [[Er, -Ei], [Ei, Er]] for kappa = (m - nk/2) mod nk
        self.MT = 16 * ((self.n_kb + 15) // 16)
        self.K2 = 4 * ((2 * self.nch + 3) // 4)
        kappa = (np.arange(m_lo, m_hi + 1) - nk // 2) % nk
        th = 2.0 * np.pi * ((np.outer(kappa, np.arange(nch)) % nk) / nk)
        er, ei = np.cos(th), -np.sin(th)
        a = np.zeros((2 * self.MT, self.K2))
        a[:self.n_kb, :nch] = er
        a[:self.n_kb, nch:2 * nch] = -ei
        a[self.MT:self.MT + self.n_kb, :nch] = ei
        a[self.MT:self.MT + self.n_kb, nch:2 * nch] = er
        self.atab = a

        h, el, er_ = savgol_operator(sg_window, sg_order)
        self.sgl = sg_window
        self.sg = np.concatenate([h, el.ravel(), er_.ravel()])
        self.mk = (m0 - m_lo).astype(np.int32)  # FITPACK interval of every (f, v) query, compact-grid rows
        self._cells = None
        self._dev = {}

    # f-v blocks of the frequency-tiled kernel: 256 threads, 4 velocities, tiles of <= 200 outputs with a
    # 12-sample halo (one tile when the whole axis fits the block)
    TILE_THREADS, TILE_VT, TILE_PAD = 256, 4, 12

    def cell_tiles(self):
        """(n_tile, TO) of the cell-staged blocks: tiles, and outputs per tile (a multiple of 4)."""
        nt = 1 if self.nF <= self.TILE_THREADS else -(-self.nF // 200)
        return nt, (-(-self.nF // nt) + 3) & ~3

    def cell_tables(self):
        """Per (velocity chunk, frequency tile) block of dvh_disp_fv_cells: the FK cells its bilinear stencils
        read -- rows m, m + 1 of columns j, j + 1 for every (f, v) it samples -- column-major (each column's
        rows lo..hi contiguous), and per (f, v) the compact indices of (m, j) and (m, j + 1) with m.
        Returns a dict of numpy tables (cached), or None when a block would not fit or the Savitzky-Golay window
        reaches past the tile's halo (sg_window > 25)."""
        if self._cells is not None:
            return self._cells or None
        T, VT, pad = self.TILE_THREADS, self.TILE_VT, self.TILE_PAD
        nF, nV = self.nF, self.nV
        nt, TO = self.cell_tiles()
        ok = self.sgl <= min(nF, 2 * pad + 1)  # a tile's halo covers windows up to 25
        nvc = -(-nV // VT)
        n_ct = nvc * nt
        qidx = np.zeros((n_ct, T, VT, 4), dtype=np.int32)
        offs, ncell = [], np.zeros(n_ct, dtype=np.int32)
        for t in range(nt):
            f_lo, f_hi = t * TO, min(nF, t * TO + TO)
            s0, s1 = max(0, f_lo - pad), min(nF, max(f_hi + pad, self.sgl))
            ok &= (s1 - s0 <= T) and (nt == 1 or f_hi - f_lo >= pad + 1)
            fs = np.arange(s0, s1)
            for c in range(nvc):
                vs = np.arange(c * VT, min(nV, c * VT + VT))
                M = self.mk[np.ix_(fs, vs)].astype(np.int64)
                J = np.broadcast_to(self.fj[fs].astype(np.int64)[:, None], M.shape)
                cols = np.concatenate([J.ravel(), J.ravel() + 1])
                rows = np.concatenate([M.ravel(), M.ravel()])
                ucol, inv = np.unique(cols, return_inverse=True)
                lo = np.full(ucol.size, np.iinfo(np.int64).max)
                hi = np.full(ucol.size, -1)
                np.minimum.at(lo, inv, rows)
                np.maximum.at(hi, inv, rows + 1)
                cnt = hi - lo + 1
                start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
                col_of = np.repeat(ucol, cnt)
                row_of = np.arange(cnt.sum()) - np.repeat(start, cnt) + np.repeat(lo, cnt)
                ct = c * nt + t
                offs.append((row_of * self.n_fb + col_of).astype(np.int32))
                ncell[ct] = offs[-1].size
                c0, c1 = np.searchsorted(ucol, J), np.searchsorted(ucol, J + 1)
                qidx[ct, :fs.size, :vs.size, 0] = start[c0] + M - lo[c0]
                qidx[ct, :fs.size, :vs.size, 1] = start[c1] + M - lo[c1]
                qidx[ct, :fs.size, :vs.size, 2] = M
        # offs was filled tile-major: reorder to ct = c * nt + t
        order = [c * nt + t for t in range(nt) for c in range(nvc)]
        by_ct = [None] * n_ct
        for k, ct in enumerate(order):
            by_ct[ct] = offs[k]
        max_cell = int(ncell.max())
        ok &= max_cell <= 8192
        if not ok:
            self._cells = {}
            return None
        cell_off = np.zeros((n_ct, max_cell), dtype=np.int32)
        for ct, o in enumerate(by_ct):
            cell_off[ct, :o.size] = o
        self._cells = dict(TO=TO, n_tile=nt, max_cell=max_cell, cell_off=cell_off, n_cell=ncell, qidx=qidx)
        return self._cells

    def mfma_tables(self):
        """dvh_disp_fv_mfma's per-(f, v) tables (cached): the FITPACK degree-1 weights of every clamped query
        on its interval m, hx[f][v] = (fx * (khi - q), fx * (q - klo)) with fx = 1 / (khi - klo) -- the
        expressions the sampling kernels evaluate, so the values are bit-identical -- and the compact cell
        offset cb[f][v] = m * n_fb + fj[f]."""
        if getattr(self, "_mfma", None) is None:
            q = np.clip(self.kq, self.kmin, self.kmax)
            m = self.mk.astype(np.int64)
            klo, khi = self.kgrid[m], self.kgrid[m + 1]
            fx = 1.0 / (khi - klo)
            hx = np.stack([fx * (khi - q), fx * (q - klo)], axis=-1)
            cb = (m * self.n_fb + self.fj.astype(np.int64)[:, None]).astype(np.int32)
            self._mfma = dict(hx=np.ascontiguousarray(hx), cb=np.ascontiguousarray(cb))
        return self._mfma

    def tables(self, device, kind="base"):
        """The plan's tables on ``device`` (uploaded once per device and kind): "base" the twiddles, contraction
        matrix and query tables every launch reads, "mfma" mfma_tables(), "cells" cell_tables() (its integers as
        they are, its arrays as tensors)."""
        key = (kind, str(device))
        if key not in self._dev:
            host = {"base": lambda: dict(wt=self.wt, atab=self.atab, kgrid=self.kgrid, kq=self.kq, fj=self.fj,
                                         fw=self.fw, sg=self.sg),
                    "mfma": self.mfma_tables, "cells": self.cell_tables}[kind]()
            self._dev[key] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) if isinstance(v, np.ndarray)
                              else v for k, v in host.items()}
        return self._dev[key]


def _check(data, plan):
    if not data.is_cuda or data.dtype != torch.float32:
        raise ValueError("data must be a float32 device tensor (no CPU fallback)")
    if data.dim() != 3 or data.shape[1] != plan.nch or data.shape[2] != plan.nt or data.stride(2) != 1:
        raise ValueError(f"data must be [B, {plan.nch}, {plan.nt}] with a contiguous time axis")


FK_FORMS = {None: 0, "one_block": 1, "tiled": 2}  # include/dvh.h DVH_FK_FORM_*


def fk_grid(data, plan: DispPlan, norm=False, slots=None, weights=None, n_slot=None, contraction=None):
    """|FK| on the plan's compact grid: [B, n_kb, n_fb], or per-slot weighted sums [n_slot, ...].  ``contraction``
    names the channel-contraction kernel ("one_block", "tiled"; None: by table size, dvh_disp_fk's rule)."""
    _check(data, plan)
    dev = data.device
    tb = plan.tables(dev)
    B = data.shape[0]
    st = _lib.stream_of(dev)
    scale = None
    if norm:
        scale = torch.empty(B * plan.nch, dtype=torch.float32, device=dev)
        _lib.call("dvh_disp_row_l1", _lib.ptr(data), data.stride(0), data.stride(1), B, plan.nch, plan.nt,
                  _lib.ptr(scale), st)
    D = torch.empty((B * plan.nch, 2 * plan.n_fb), dtype=torch.float64, device=dev)
    _lib.call("dvh_disp_tdft", _lib.ptr(data), data.stride(0), data.stride(1), B, plan.nch, plan.nt,
              _lib.ptr(tb["wt"]), plan.n_fb, _lib.ptr(scale), _lib.ptr(D), st)
    if slots is None:
        FK = torch.empty((B, plan.n_kb, plan.n_fb), dtype=torch.float64, device=dev)
        sl = wt = None
    else:
        slots = np.asarray(slots, dtype=np.int64)
        if n_slot is None or slots.shape != (B,) or (B and (slots.min() < 0 or slots.max() >= n_slot)):
            raise ValueError("fk_grid: one class slot in [0, n_slot) per gather")
        FK = torch.zeros((n_slot, plan.n_kb, plan.n_fb), dtype=torch.float64, device=dev)
        sl = torch.as_tensor(slots.astype(np.int32), device=dev)
        wt = torch.as_tensor(np.asarray(weights, dtype=np.float32), device=dev)
    _lib.call("dvh_disp_fk_as", _lib.ptr(D), B, plan.nch, plan.n_fb, _lib.ptr(tb["atab"]), plan.MT, plan.K2,
              plan.n_kb, _lib.ptr(FK), _lib.ptr(sl), _lib.ptr(wt), 0 if n_slot is None else int(n_slot),
              FK_FORMS[contraction], st)
    return FK


MFMA_MIN_BLOCKS = 512  # (64-velocity block, image) pairs: two blocks per CU
CELLS_MIN_BLOCKS = 4096  # (frequency tile, 4-velocity chunk, image) blocks: a batch that fills the chip

# the kernels of the dvh_disp_fv chain by their include/dvh.h form (DVH_FV_*); "not_tiled" leaves the tiled kernel out
_CHAIN = {"per_image": 1, "not_tiled": 2, "batched": 3, "tiled": 4}
_CHAIN_NAME = {1: "per_image", 3: "batched", 4: "tiled"}
FORMS = (None, "mfma", "cells", "chain", *_CHAIN)


def _fv_staged(plan: DispPlan, B: int, form, images_per_block=0):
    """(name, G): "mfma" or "cells" where one of the two table-fed kernels runs, None for the dvh_disp_fv chain, and
    the images per block to pass on -- the caller's where ``form`` names the kernel that runs, else 0."""
    if form not in FORMS:
        raise ValueError(f"form must be one of {FORMS}")
    name = None
    # dvh_disp_fv_mfma: savgol window 25, nF >= 32, a compact FK grid of at most 8 192 bins
    mfma_ok = plan.sgl == 25 and plan.nF >= 32 and plan.n_kb * plan.n_fb <= 8192
    # dvh_disp_fv_cells for batches that fill the chip; few images (the bench's class stacks) keep the chain
    n_blocks = B * plan.cell_tiles()[0] * -(-plan.nV // DispPlan.TILE_VT)
    if mfma_ok and (form == "mfma" or (form is None and B * -(-plan.nV // 64) >= MFMA_MIN_BLOCKS)):
        name = "mfma"
    elif form == "cells" or (form in (None, "mfma") and n_blocks >= CELLS_MIN_BLOCKS):
        if plan.cell_tables() is not None:
            name = "cells"
    return name, int(images_per_block) if name is not None and form == name else 0


def fv_choice(plan: DispPlan, B: int, form=None, images_per_block=0):
    """(name, G): the f-v kernel fv_from_fk launches for B images of the plan -- "mfma", "cells", "tiled", "batched" or
    "per_image" -- and its images per block.  Host arithmetic only, no device.
    form None is the product's choice: mfma from MFMA_MIN_BLOCKS blocks on, cells from CELLS_MIN_BLOCKS on, else the
    dvh_disp_fv chain (tiled, batched, per-image by size: dvh_disp_fv_pick).  A form named by the caller (FORMS;
    "chain" = dvh_disp_fv's own choice, "not_tiled" = batched or per-image by size) runs wherever the kernel's
    structural conditions hold, whatever the batch size; where they do not (a Savitzky-Golay window other than 25
    for mfma, above 25 for cells and tiled among them), a refused "mfma" takes the product's choice among the others
    and every other refused form the chain, down to per_image.  images_per_block > 0 sets G of the kernel named by
    ``form``; G is 0 where the launcher counts for itself (mfma, cells) and for per_image."""
    name, G = _fv_staged(plan, B, form, images_per_block)
    if name is not None:
        return name, G
    f, g = C.c_int32(), C.c_int32()
    _lib.call("dvh_disp_fv_pick", B, plan.n_kb, plan.n_fb, plan.nF, plan.nV, plan.sgl, _CHAIN.get(form, 0),
              int(images_per_block), C.byref(f), C.byref(g))
    return _CHAIN_NAME.get(f.value), g.value


def _use_mfma(plan: DispPlan, B: int) -> bool:
    """fv_choice(plan, B)[0] == "mfma", under the name bench.py imports."""
    return _fv_staged(plan, B, None)[0] == "mfma"


def fv_from_fk(FK, plan: DispPlan, out=None, form=None, images_per_block=0):
    """The f-v images of |FK| [B, n_kb, n_fb] on the kernel fv_choice(plan, B, form, images_per_block) names."""
    dev = FK.device
    tb = plan.tables(dev)
    B = FK.shape[0]
    if out is None:
        out = torch.empty((B, plan.nV, plan.nF), dtype=torch.float32, device=dev)
    name, G = _fv_staged(plan, B, form, images_per_block)
    if name == "mfma":
        mt = plan.tables(dev, "mfma")
        _lib.call("dvh_disp_fv_mfma", _lib.ptr(FK), B, plan.n_kb, plan.n_fb, _lib.ptr(mt["hx"]), _lib.ptr(mt["cb"]),
                  plan.nF, plan.nV, _lib.ptr(tb["fw"]), _lib.ptr(tb["sg"]), plan.sgl, G, _lib.ptr(out),
                  _lib.stream_of(dev))
    elif name == "cells":
        c = plan.tables(dev, "cells")
        _lib.call("dvh_disp_fv_cells_as", _lib.ptr(FK), B, plan.n_kb, plan.n_fb, _lib.ptr(tb["kgrid"]), plan.kmin,
                  plan.kmax, _lib.ptr(tb["kq"]), plan.nF, plan.nV, _lib.ptr(tb["fw"]), _lib.ptr(tb["sg"]), plan.sgl,
                  c["TO"], c["n_tile"], DispPlan.TILE_VT, c["max_cell"], _lib.ptr(c["cell_off"]), _lib.ptr(c["n_cell"]),
                  _lib.ptr(c["qidx"]), _lib.ptr(out), G, _lib.stream_of(dev))
    else:
        _lib.call("dvh_disp_fv_as", _lib.ptr(FK), B, plan.n_kb, plan.n_fb, _lib.ptr(tb["kgrid"]), plan.kmin, plan.kmax,
                  _lib.ptr(tb["kq"]), plan.nF, plan.nV, _lib.ptr(tb["fj"]), _lib.ptr(tb["fw"]), _lib.ptr(tb["sg"]),
                  plan.sgl, _lib.ptr(out), _CHAIN.get(form, 0), int(images_per_block), _lib.stream_of(dev))
    return out


def fv_maps(data, plan: DispPlan, norm=False, form=None, images_per_block=0):
    """map_fv for every gather of the batch: [B, Nvel, Nfreq] float32 (rows = sorted-query order)."""
    return fv_from_fk(fk_grid(data, plan, norm=norm), plan, form=form, images_per_block=images_per_block)


def fv_class_means(data, plan: DispPlan, slots, n_slot, norm=False, counts=None, form=None, images_per_block=0):
    """Mean f-v image per class slot (sum(disps) / len): the transform after |FK| is linear, so the
    per-pass |FK| grids are averaged on device and sampled once per slot."""
    slots = np.asarray(slots, dtype=np.int64)
    counts = np.bincount(slots, minlength=n_slot) if counts is None else np.asarray(counts)
    w = np.where(counts[slots] > 0, 1.0 / np.maximum(counts[slots], 1), 0.0)
    return fv_from_fk(fk_grid(data, plan, norm=norm, slots=slots, weights=w, n_slot=n_slot), plan, form=form,
                      images_per_block=images_per_block)


# ---------------------------------------------------------------------------------------------
# Phase-shift (frequency-domain slant-stack) transform: map_fv_FD_slant_stack, modules/utils.py:429-454


class SlantPlan:
    """Host tables of the phase-shift transform for one (nch, nt, dx, dt, freqs, vels, rows) geometry, with the
    reference's own expressions:
      nf = 2 ** (1 + ceil(log(nt, 2))), f_idx = argmin |f - fftfreq(nf, dt)| per frequency        :437-451
    ``bins`` are the sorted unique f_idx (DFT bin numbers), ``fb`` each frequency's position among them, ``wt`` the
    time-DFT twiddles of those bins in dvh_disp_tdft's layout, and rows [row0, row0 + n_row) the gather rows
    ``rows`` = (start, stop) slices out of nch (the reference's data[6:25])."""

    def __init__(self, nch, nt, dx, dt, freqs, vels, rows=(6, 25)):
        self.nch, self.nt, self.dx, self.dt = int(nch), int(nt), float(dx), float(dt)
        self.freqs = np.ascontiguousarray(np.asarray(freqs, dtype=np.float64).ravel())
        self.vels = np.ascontiguousarray(np.asarray(vels, dtype=np.float64).ravel())
        self.nF, self.nV = self.freqs.size, self.vels.size
        if not np.isfinite(self.vels).all() or (self.vels == 0).any():
            raise ValueError("math domain error: every velocity must be finite and non-zero")
        start, stop, _ = slice(*rows).indices(self.nch)
        self.row0, self.n_row = start, max(0, stop - start)
        self.nf = nf = 2 ** (1 + math.ceil(math.log(self.nt, 2)))
        fft_freqs = np.fft.fftfreq(nf, d=self.dt)
        self.fidx = np.array([np.abs(f - fft_freqs).argmin() for f in self.freqs], dtype=np.int64)
        self.bins = np.unique(self.fidx)
        self.n_fb = self.bins.size
        self.fb = np.searchsorted(self.bins, self.fidx).astype(np.int32)
        ang = 2.0 * np.pi * ((np.outer(np.arange(self.nt), self.bins) % nf) / nf)
        wt = np.empty((self.nt, 2 * self.n_fb))
        wt[:, 0::2] = np.cos(ang)
        wt[:, 1::2] = -np.sin(ang)
        self.wt = wt
        self._dev = {}

    def tables(self, device):
        key = str(device)
        if key not in self._dev:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            self._dev[key] = dict(wt=t(self.wt), fb=t(self.fb), freqs=t(self.freqs), vels=t(self.vels))
        return self._dev[key]


def _slant_spectra(data, plan: SlantPlan, norm):
    """dvh_disp_tdft of the plan's rows at the plan's bins: D [B * n_row, 2 * n_fb] float64 (with ``norm`` of the rows
    divided by their L1 norm), or None when the transform has no rows or no frequencies."""
    _check(data, plan)
    if plan.n_row == 0 or plan.n_fb == 0:
        return None
    dev, B = data.device, data.shape[0]
    st = _lib.stream_of(dev)
    rows = data[:, plan.row0:plan.row0 + plan.n_row]
    scale = None
    if norm:
        scale = torch.empty(B * plan.n_row, dtype=torch.float32, device=dev)
        _lib.call("dvh_disp_row_l1", _lib.ptr(rows), rows.stride(0), rows.stride(1), B, plan.n_row, plan.nt,
                  _lib.ptr(scale), st)
    D = torch.empty((B * plan.n_row, 2 * plan.n_fb), dtype=torch.float64, device=dev)
    _lib.call("dvh_disp_tdft", _lib.ptr(rows), rows.stride(0), rows.stride(1), B, plan.n_row, plan.nt,
              _lib.ptr(plan.tables(dev)["wt"]), plan.n_fb, _lib.ptr(scale), _lib.ptr(D), st)
    return D


def _slant_launch(D, plan: SlantPlan, B, out, v0=0, v1=None):
    """dvh_disp_slant for the velocities [v0, v1) into ``out`` [B, v1 - v0, nF] (contiguous float32)."""
    v1 = plan.nV if v1 is None else v1
    tb = plan.tables(out.device)
    n_row = 0 if D is None else plan.n_row
    if D is None:
        D = torch.empty(2, dtype=torch.float64, device=out.device)  # never read: the sum has no rows
    _lib.call("dvh_disp_slant", _lib.ptr(D), B, n_row, max(plan.n_fb, 1), 0, n_row, _lib.ptr(tb["fb"]),
              _lib.ptr(tb["freqs"]), plan.nF, _lib.ptr(tb["vels"][v0:v1]), v1 - v0, plan.dx, _lib.ptr(out),
              (v1 - v0) * plan.nF, _lib.stream_of(out.device))
    return out


def slant_maps(data, plan: SlantPlan, norm=True, out=None):
    """map_fv_FD_slant_stack for every gather of the batch: [B, nV, nF] float32, rows in the plan's velocity order
    (into ``out``, a contiguous float32 device tensor of that shape, when given)."""
    D = _slant_spectra(data, plan, norm)
    B = data.shape[0]
    if out is None:
        out = torch.empty((B, plan.nV, plan.nF), dtype=torch.float32, device=data.device)
    elif (tuple(out.shape) != (B, plan.nV, plan.nF) or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != data.device):
        raise ValueError(f"out must be a contiguous float32 [{B}, {plan.nV}, {plan.nF}] tensor on the data's device")
    if out.numel() == 0:
        return out
    return _slant_launch(D, plan, B, out)


SLANT_CHUNK_BYTES = 256 << 20  # per-pass images held at a time by slant_class_means


def slant_class_means(data, plan: SlantPlan, slots, n_slot, norm=True):
    """Mean phase-shift image per class slot, sum(images) / len over the slot's passes in batch order
    ([n_slot, nV, nF] float32; a slot without passes is 0).  The magnitude is not linear in the data, so the per-pass
    images are formed -- for a chunk of velocities at a time, SLANT_CHUNK_BYTES of images -- and averaged by
    dvh_select_mean_var, each chunk into its rows of the result."""
    slots = np.asarray(slots, dtype=np.int64)
    B = data.shape[0]
    if slots.shape != (B,) or (B and (slots.min() < 0 or slots.max() >= n_slot)):
        raise ValueError("slant_class_means: one class slot in [0, n_slot) per gather")
    dev = data.device
    D = _slant_spectra(data, plan, norm)
    nV, nF = plan.nV, plan.nF
    out = torch.zeros((n_slot, nV, nF), dtype=torch.float32, device=dev)
    if B == 0 or out.numel() == 0:
        return out
    counts = np.bincount(slots, minlength=n_slot)
    filled = np.flatnonzero(counts)
    cnt = counts[filled].astype(np.int32)
    off = (np.cumsum(cnt) - cnt).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sel_t, off_t, cnt_t = t(np.argsort(slots, kind="stable").astype(np.int32)), t(off), t(cnt)
    means = out if filled.size == n_slot else torch.empty((filled.size, nV, nF), dtype=torch.float32, device=dev)
    vc = int(max(1, min(nV, SLANT_CHUNK_BYTES // (4 * B * nF))))
    img = torch.empty(B * vc * nF, dtype=torch.float32, device=dev)
    for v0 in range(0, nV, vc):
        v1 = min(nV, v0 + vc)
        _slant_launch(D, plan, B, img[:B * (v1 - v0) * nF].view(B, v1 - v0, nF), v0, v1)
        _lib.call("dvh_select_mean_var", _lib.ptr(img), (v1 - v0) * nF, (v1 - v0) * nF, _lib.ptr(sel_t), _lib.ptr(off_t),
                  _lib.ptr(cnt_t), filled.size, _lib.ptr(means[:, v0:v1]), nV * nF, _lib.stream_of(dev))
    if means is not out:
        out[t(filled)] = means
    return out
