"""Bootstrap / convergence resampling on the device.

The reference recomputes every virtual shot gather of every resample from scratch
(``bootstrap_disp``, apis/imaging_classes.py:8-48, called 30 x 60 times per class by the notebooks'
``convergence_test``, imaging_diff_speed.ipynb#cell30).  Here:

  1. the per-pass gathers of all windows are computed once (``dvh_vsg_gathers``) and kept in HBM
     (``GatherCache``; 96 KB per pass for the notebook geometry);
  2. a resample's stack -- ``sum(images) / len(images)`` of its ``random.sample`` draw -- is a gather-
     mean over the cached rows the dispersion image reads (``dvh_select_mean``, summed in draw order);
  3. the f-v images of all resamples go through the batched dispersion kernels in one launch each;
  4. every (resample, mode) ridge is walked by one wave (``dvh_ridge``): extract_ridge_ref_idx,
     modules/utils.py:621-678, with its strict velocity window, first-index argmax and savgol(25, 2).

``transform="slant"`` makes the same statistics on the phase-shift image (Dispersion(transform="slant")) instead of
the f-k image: either through the resamples' images and ``dvh_ridge`` (walk="image"), or, with the same results,
through ``dvh_slant_ridge`` (walk="fused"), whose walk computes the steering sums of the velocities it compares from
the stacks' spectra and forms no image (``plan_ridges``, ``slant_ridges``).

``stack="pws"`` replaces the mean of step 2 by the phase-weighted stack (Schimmel & Paulssen 1997): the mean times the
coherence of the drawn passes' instantaneous phases to ``power``, from the analytic signal of the cached rows
(``GatherCache.analytic``: ``dvh_hilbert_rows`` once per cache; ``dvh_select_pws`` per call).  Steps 3 and 4 are the same.

Random draws use Python's ``random`` exactly as the reference does (``random.sample(range(1, n), k)``,
index 0 never drawn), so seeding ``random`` reproduces the reference's resamples.
"""
from __future__ import annotations

import random
import time

import numpy as np
import torch

from . import _lib
from .device import default_device, to_device_f32
from .disp import DispPlan, SlantPlan, _slant_spectra, fk_grid, fv_from_fk, savgol_operator, slant_maps
from .plan import VsgParams, VsgPlan, pass_geometry
from .vsg import vsg_gathers

FREQS = np.arange(0.8, 25, 0.1)   # Dispersion defaults of compute_disp_image (apis/virtual_shot_gather.py:247)
VELS = np.arange(200, 1200)
_SG_RIDGE = None


def _sg_ridge():
    global _SG_RIDGE
    if _SG_RIDGE is None:
        h, el, er = savgol_operator(25, 2)
        _SG_RIDGE = np.concatenate([h, el.ravel(), er.ravel()])
    return _SG_RIDGE


def ridges(fv, freqs, vels, freq_lb, freq_ub, ref_freq_idx=None, sigma=25, vel_max=400, ref_vel=None,
           return_picks=False):
    """extract_ridge_ref_idx (modules/utils.py:621-678) for every image of ``fv`` [B, Nvel, Nfreq]
    (device float32, rows in the map's order = ``vels`` reversed) on the band lb <= f < ub.
    ``ref_freq_idx`` indexes the band; ``ref_vel`` is a callable of frequency (or an array over
    the band).  Returns float64 [B, n_band] on the host (and the raw picks before the smoothing
    with return_picks=True)."""
    return ridges_finish(ridges_launch(fv, freqs, vels, freq_lb, freq_ub, ref_freq_idx, sigma, vel_max, ref_vel,
                                       return_picks))


def ridges_finish(pending):
    """Host results of a ridges_launch (synchronises); raises as the reference does for an empty window."""
    out, status, picks = pending
    if int(status.max()) != 0:
        raise ValueError("attempt to get argmax of an empty sequence (no velocity inside a ridge window)")
    return (out.cpu().numpy(), picks.cpu().numpy()) if picks is not None else out.cpu().numpy()


def _walk_band(freqs, freq_lb, freq_ub, ref_freq_idx, ref_vel):
    """A walk's band lb <= f < ub as (first column c0, length nb), the kernels' reference index and the reference
    velocities over the band (or None)."""
    band = np.flatnonzero((freqs >= freq_lb) & (freqs < freq_ub))
    if band.size == 0:
        raise ValueError("empty frequency band")
    if not np.array_equal(band, np.arange(band[0], band[-1] + 1)):
        raise ValueError("the frequency band must be contiguous")
    c0, nb = int(band[0]), int(band.size)
    vr = None
    if ref_freq_idx is not None and ref_vel is not None:
        vr = ref_vel(freqs[band]) if callable(ref_vel) else np.asarray(ref_vel, dtype=np.float64)
        vr = np.asarray(vr, dtype=np.float64).reshape(nb)
    # ref_freq_idx=None -> vel_max mode (INT32_MIN); a negative index is a Python index into the band,
    # walked in the reference's loop order (modules/utils.py:662-671)
    ref = -2 ** 31 if ref_freq_idx is None else int(ref_freq_idx)
    if ref_freq_idx is not None and not -nb <= ref < nb:
        raise IndexError(f"index {ref} is out of bounds for axis 0 with size {nb}")
    return c0, nb, ref, vr


def ridges_launch(fv, freqs, vels, freq_lb, freq_ub, ref_freq_idx=None, sigma=25, vel_max=400, ref_vel=None,
                  return_picks=False):
    """The dvh_ridge launch of ridges() without the synchronising read-back: (out, status, picks) device
    tensors for ridges_finish, so that several modes' walks are queued before one wait."""
    if not isinstance(fv, torch.Tensor) or not fv.is_cuda or fv.dtype != torch.float32 or fv.dim() != 3:
        raise ValueError("fv must be a float32 device tensor [B, Nvel, Nfreq] (no CPU fallback)")
    freqs = np.asarray(freqs, dtype=np.float64)
    vel_desc = np.asarray(vels, dtype=np.float64)[::-1].copy()
    fv = fv.contiguous()  # rows [Nvel][Nfreq] as the kernel indexes them
    if vel_desc.size != fv.shape[1] or freqs.size != fv.shape[2]:
        raise ValueError("fv shape does not match (vels, freqs)")
    if vel_desc.size > 1 and not np.all(np.diff(vel_desc) < 0):
        raise ValueError("the device ridge walk needs strictly increasing vels")
    c0, nb, ref, vr = _walk_band(freqs, freq_lb, freq_ub, ref_freq_idx, ref_vel)
    dev = fv.device
    from .device import upload
    B = fv.shape[0]
    out = torch.empty((B, nb), dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    # the walk's host tables in one asynchronous copy: the launch is queued without waiting for the work before it
    tabs = upload([vel_desc, np.asarray(_sg_ridge(), dtype=np.float64)] + ([vr] if vr is not None else []), dev)
    vel_t, sg = tabs[0], tabs[1]
    vref = tabs[2] if vr is not None else None
    picks = torch.empty((B, nb), dtype=torch.float64, device=dev) if return_picks else None
    _lib.call("dvh_ridge", _lib.ptr(fv), fv.stride(0), B, fv.shape[1], fv.shape[2], c0, nb, _lib.ptr(vel_t), ref,
              float(sigma), float(vel_max), _lib.ptr(vref), _lib.ptr(sg), 25, _lib.ptr(out), _lib.ptr(status),
              _lib.ptr(picks), _lib.stream_of(dev))
    return out, status, picks


_DISP_PLANS = {}  # (nch, w, dt, freqs, vels) -> DispPlan, shared by GatherCache instances
_SLANT_PLANS = {}  # the same key -> SlantPlan over all rows, velocities descending
_STREAMS = {}
TRANSFORMS = ("fk", "slant")
SLANT_WALK = "fused"  # walk=None with transform="slant" (measured: tools/bench_boot_slant.py, profiles/boot_slant.json)


def check_transform(transform, walk=None):
    """The walk of a (transform, walk) pair -- "image": form the f-v images, then dvh_ridge; "fused": dvh_slant_ridge
    on the spectra -- or ValueError for a pair that does not exist.  No device work."""
    if transform not in TRANSFORMS:
        raise ValueError(f"transform must be 'fk' or 'slant', not {transform!r}")
    if transform == "fk":
        if walk not in (None, "image"):
            raise ValueError(f"transform='fk' samples a grid: walk must be None or 'image', not {walk!r}")
        return "image"
    if walk not in (None, "fused", "image"):
        raise ValueError(f"walk must be None, 'fused' or 'image', not {walk!r}")
    return SLANT_WALK if walk is None else walk


STACKS = ("linear", "pws")


def check_stack(stack, power=2.0):
    """The power of a (stack, power) pair as a float -- "linear": the mean sum(images) / len(images); "pws": the
    phase-weighted stack lin * c^power (dvh_select_pws), power 0 or at least 1 -- or ValueError for a stack that does
    not exist or a power the kernel refuses.  No device work."""
    if stack not in STACKS:
        raise ValueError(f"stack must be 'linear' or 'pws', not {stack!r}")
    try:
        p = float(power)
    except (TypeError, ValueError):
        raise ValueError(f"power must be a number, not {power!r}") from None
    if not (p == 0.0 or 1.0 <= p <= float(np.finfo(np.float32).max)):
        raise ValueError(f"power must be 0 or a finite value of at least 1, not {power!r}")
    return p


def _side_stream(device, k):
    """The k-th side stream of a device (created once)."""
    key = (str(device), k)
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device=device)
    return _STREAMS[key]


class GatherCache:
    """Per-pass gathers [n, R, W] of a window list on the device, computed once
    (VirtualShotGathersFromWindows.get_images' per-pass images: norm=False, two-sided).

    Windows whose time steps round to different lag lengths w (499 / 500 on real axes) share the cache: every
    gather sits zero-padded to the widest W, so that a resample's sum over the padded rows is the reference's
    sum(images) -- VirtualShotGather.__add__ adds the other images' first min(w) lags to the first image's
    (apis/virtual_shot_gather.py:195-199) -- on the first drawn pass's lag axis, whose width and time step its
    dispersion image then takes (compute_disp_image, :247-258)."""

    def __init__(self, windows, pivot, start_x, end_x, wlen=2, include_other_side=True, device=None):
        self.device = device or default_device()
        self.prm = VsgParams(pivot=pivot, start_x=start_x, end_x=end_x, wlen=wlen, norm=False,
                             include_other_side=include_other_side)
        geoms = [pass_geometry(w.x_axis, w.t_axis, w.veh_state_x, w.veh_state_t, self.prm) for w in windows]
        shapes = {tuple(np.shape(w.data)) for w in windows}
        if len(shapes) != 1:
            raise ValueError("bootstrap windows must share one shape")
        n_ch, n_t = shapes.pop()
        self.w_of = np.array([g.w for g in geoms], dtype=np.int64)
        by_w = {}
        for i, g in enumerate(geoms):
            by_w.setdefault(g.w, []).append(i)
        if len(by_w) == 1:
            self.plan = VsgPlan(geoms, self.prm, n_ch, n_t)
            self.G = vsg_gathers(to_device_f32([w.data for w in windows], self.device), self.plan)  # [n, R, w]
        else:
            plans = {w: VsgPlan([geoms[i] for i in idx], self.prm, n_ch, n_t) for w, idx in by_w.items()}
            if len({p.R for p in plans.values()}) != 1:
                raise ValueError("operands could not be broadcast together: passes produce gathers of different shapes")
            self.plan = plans[geoms[0].w]
            W = max(by_w)
            self.G = torch.zeros((len(windows), self.plan.R, W), dtype=torch.float32, device=self.device)
            for w, idx in by_w.items():
                g = vsg_gathers(to_device_f32([windows[i].data for i in idx], self.device), plans[w])
                self.G[torch.as_tensor(idx, device=self.device), :, :w] = g
        self.W = int(self.G.shape[-1])
        self.gx, self.gt = geoms[0].gather_x_axis, geoms[0].gather_t_axis
        # per lag length: the time axis of its first pass (a resample's image takes its first drawn pass's)
        self._gt_of = {}
        for g in geoms:
            self._gt_of.setdefault(g.w, g.gather_t_axis)
        self.n = len(windows)
        self._disp = {}
        self._H = None

    @classmethod
    def from_device(cls, data, x_axis, t_axis, trk_x, trk_t, trk_len, pivot, start_x, end_x, wlen=2,
                    include_other_side=True):
        """The cache of windows already resident as one float32 device tensor [n, C, T] on shared axes, with
        the index tables derived on the device from packed trajectories (plan.pack_trajectories layout,
        dvh_pass_geometry): no per-pass host work (the bench's bootstrap job)."""
        from .plan import DevicePlan
        self = cls.__new__(cls)
        self.device = data.device
        self.prm = VsgParams(pivot=pivot, start_x=start_x, end_x=end_x, wlen=wlen, norm=False,
                             include_other_side=include_other_side)
        self.plan = DevicePlan(x_axis, t_axis, trk_x, trk_t, trk_len, self.prm, data.shape[1])
        self.G = vsg_gathers(data, self.plan)
        x_axis, t_axis = np.asarray(x_axis, dtype=np.float64), np.asarray(t_axis, dtype=np.float64)
        pv, st = int(np.argmax(x_axis >= pivot)), int(np.argmax(x_axis >= start_x))
        dt = t_axis[1] - t_axis[0]
        self.gx = x_axis[st:st + self.plan.R] - x_axis[pv]
        self.gt = (np.arange(self.plan.w) - self.plan.w // 2) * dt
        self.n = data.shape[0]
        self.w_of = np.full(self.n, self.plan.w, dtype=np.int64)
        self.W = self.plan.w
        self._gt_of = {self.plan.w: self.gt}
        self._disp = {}
        self._H = None
        return self

    def disp_plan(self, start_x=-150, end_x=0, freqs=FREQS, vels=VELS, w=None):
        """compute_disp_image's nearest-offset channel slice and its DispPlan (dx = 8.16, :247-258) for the images
        of lag length w (default: the first pass's)."""
        w = int(self.w_of[0]) if w is None else int(w)
        s = int(np.abs(self.gx - start_x).argmin())
        e = int(np.abs(self.gx - end_x).argmin())
        key = (s, e, id(freqs), id(vels), w)
        if key not in self._disp:
            gt = self._gt_of[w]
            dt = float(gt[1] - gt[0])
            # plans are shared across caches of one geometry (a convergence test per class builds a new cache;
            # the plan's host tables and their device copies are the same)
            pkey = (e + 1 - s, w, dt, np.asarray(freqs, dtype=np.float64).tobytes(),
                    np.asarray(vels, dtype=np.float64).tobytes())
            if pkey not in _DISP_PLANS:
                if len(_DISP_PLANS) >= 16:
                    _DISP_PLANS.pop(next(iter(_DISP_PLANS)))
                _DISP_PLANS[pkey] = DispPlan(e + 1 - s, w, 8.16, dt, freqs, vels)
            self._disp[key] = (s, e, _DISP_PLANS[pkey])
        return self._disp[key]

    def slant_plan(self, start_x=-150, end_x=0, freqs=FREQS, vels=VELS, w=None):
        """disp_plan's channel slice with the SlantPlan of compute_disp_image(..., transform="slant") for a stack of
        lag length w: all rows of the slice, velocities in descending order, dx = 8.16."""
        w = int(self.w_of[0]) if w is None else int(w)
        s = int(np.abs(self.gx - start_x).argmin())
        e = int(np.abs(self.gx - end_x).argmin())
        key = ("slant", s, e, id(freqs), id(vels), w)
        if key not in self._disp:
            gt = self._gt_of[w]
            dt = float(gt[1] - gt[0])
            nch = e + 1 - s
            vel_desc = np.sort(np.asarray(vels, dtype=np.float64))[::-1]
            pkey = (nch, w, dt, np.asarray(freqs, dtype=np.float64).tobytes(), vel_desc.tobytes())
            if pkey not in _SLANT_PLANS:
                if len(_SLANT_PLANS) >= 16:
                    _SLANT_PLANS.pop(next(iter(_SLANT_PLANS)))
                _SLANT_PLANS[pkey] = SlantPlan(nch, w, 8.16, dt, freqs, vel_desc, rows=(0, nch))
            self._disp[key] = (s, e, _SLANT_PLANS[pkey])
        return self._disp[key]

    def _by_lag_length(self, first):
        """The resamples grouped by the lag length of their first drawn pass: [(w, rows or None)], rows None when
        every resample has the cache's width (one group, no gather of the stacks)."""
        wf = self.w_of[np.asarray(first, dtype=np.int64)]
        if np.all(wf == self.W):
            return [(self.W, None)]
        return [(int(w), np.flatnonzero(wf == w)) for w in np.unique(wf)]

    def images_of(self, stacks, first, start_x=-150, end_x=0, transform="fk"):
        """f-v images [B, Nvel, Nfreq] of resample stacks [B, nch, W] whose first drawn passes are ``first``: each
        on its first pass's lag axis (its width w and time step).  ``transform``: "fk" (map_fv) or "slant" (the
        phase-shift transform over all rows, rows in descending velocity)."""
        check_transform(transform)

        def image(stk, w):
            if transform == "slant":
                return slant_maps(stk, self.slant_plan(start_x, end_x, w=w)[2], norm=False)
            plan = self.disp_plan(start_x, end_x, w=w)[2]
            return fv_from_fk(fk_grid(stk, plan), plan)
        groups = self._by_lag_length(first)
        if groups[0][1] is None:
            return image(stacks, self.W)
        out = None
        for w, rows in groups:
            rt = torch.as_tensor(rows, device=self.device)
            fv = image(stacks[rt][:, :, :w], w)
            if out is None:
                out = torch.empty((stacks.shape[0],) + tuple(fv.shape[1:]), dtype=fv.dtype, device=fv.device)
            out[rt] = fv
        return out

    def analytic(self):
        """H [n, R, W]: the imaginary part of every cached row's analytic signal (dvh_hilbert_rows), each pass over
        its own w_of lags and 0 beyond, computed on the first call and kept."""
        if self._H is None:
            from .device import upload
            G = self.G.contiguous()
            H = torch.empty_like(G)
            R = int(G.shape[1])
            row_len, = upload([np.repeat(self.w_of, R).astype(np.int32)], self.device)
            _lib.call("dvh_hilbert_rows", _lib.ptr(G), self.W, self.n * R, self.W, _lib.ptr(row_len), _lib.ptr(H),
                      _lib.stream_of(self.device))
            self._H = H
        return self._H

    def _select_pws(self, s, e, sel_t, off_t, cnt_t, B, power, out):
        """dvh_select_pws of B draws over gather rows s..e into out [B, e + 1 - s, W]."""
        w, R = self.W, self.plan.R
        rows = (e + 1 - s) * w
        _lib.call("dvh_select_pws", _lib.ptr(self.G[:, s:e + 1, :]), _lib.ptr(self.analytic()[:, s:e + 1, :]), R * w,
                  rows, _lib.ptr(sel_t), _lib.ptr(off_t), _lib.ptr(cnt_t), B, power, _lib.ptr(out), rows,
                  _lib.stream_of(self.device))
        return out

    def phase_weighted_stack(self, power=2.0):
        """The phase-weighted stack of all passes in order over all R gather rows: [1, R, W]."""
        from .device import upload
        power = check_stack("pws", power)
        out = torch.empty((1, self.plan.R, self.W), dtype=torch.float32, device=self.device)
        sel_t, off_t, cnt_t = upload([np.arange(self.n, dtype=np.int32), np.zeros(1, np.int32),
                                      np.full(1, self.n, dtype=np.int32)], self.device)
        return self._select_pws(0, self.plan.R - 1, sel_t, off_t, cnt_t, 1, power, out)

    def resample_stacks(self, sel, start_x=-150, end_x=0, out=None, stack="linear", power=2.0):
        """Stacked gathers over the disp rows for every draw: sel [B, k] pass indices -> [B, nch, w] (into
        ``out``, a contiguous [B, nch, w] float32 device tensor, when given).  ``stack``: "linear" (the mean) or "pws"
        (the phase-weighted stack with ``power``, check_stack)."""
        power = check_stack(stack, power)
        sel = np.asarray(sel, dtype=np.int32)
        if sel.ndim != 2 or sel.size == 0 or sel.min() < 0 or sel.max() >= self.n:
            raise ValueError("selections must be [B, k] pass indices")
        s, e, _ = self.disp_plan(start_x, end_x)
        w, R = self.W, self.plan.R
        B, k = sel.shape
        if out is None:
            out = torch.empty((B, e + 1 - s, w), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (B, e + 1 - s, w) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 [{B}, {e + 1 - s}, {w}] tensor")
        if stack == "pws":
            from .device import upload
            sel_t, off_t, cnt_t = upload([sel.reshape(-1), np.arange(B, dtype=np.int32) * k,
                                          np.full(B, k, dtype=np.int32)], self.device)
            return self._select_pws(s, e, sel_t, off_t, cnt_t, B, power, out)
        sel_t = torch.as_tensor(sel, device=self.device)
        base = self.G[:, s:e + 1, :]
        _lib.call("dvh_select_mean", _lib.ptr(base), R * w, (e + 1 - s) * w, _lib.ptr(sel_t), B, k, _lib.ptr(out),
                  (e + 1 - s) * w, _lib.stream_of(self.device))
        return out

    def resample_stacks_sizes(self, sels, start_x=-150, end_x=0, out=None, stack="linear", power=2.0):
        """resample_stacks of several draw sets (sels: list of [B_k, k] arrays, e.g. one per bootstrap size) into
        consecutive rows of one [sum B_k, nch, w] buffer: every selection, with each resample's offset and size,
        crosses to the device in ONE asynchronous copy (device.upload) and all resamples are one
        dvh_select_mean_var launch (60 launches of 30 resamples each were latency-bound: 0.94 ms), or with
        stack="pws" one dvh_select_pws launch."""
        from .device import upload
        power = check_stack(stack, power)
        sels = [np.asarray(x, dtype=np.int32) for x in sels]
        if not sels or any(x.ndim != 2 or x.size == 0 for x in sels):
            raise ValueError("selections must be [B, k] pass indices")
        flat = np.concatenate([x.reshape(-1) for x in sels])
        if flat.min() < 0 or flat.max() >= self.n:
            raise ValueError("selections must be [B, k] pass indices")
        s, e, _ = self.disp_plan(start_x, end_x)
        w, R = self.W, self.plan.R
        B = sum(x.shape[0] for x in sels)
        rows = (e + 1 - s) * w
        if out is None:
            out = torch.empty((B, e + 1 - s, w), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (B, e + 1 - s, w) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 [{B}, {e + 1 - s}, {w}] tensor")
        cnt = np.concatenate([np.full(x.shape[0], x.shape[1], dtype=np.int32) for x in sels])
        off = np.concatenate([[0], np.cumsum(cnt[:-1], dtype=np.int64)]).astype(np.int32)
        sel_t, off_t, cnt_t = upload([flat, off, cnt], self.device)
        if stack == "pws":
            return self._select_pws(s, e, sel_t, off_t, cnt_t, B, power, out)
        base = self.G[:, s:e + 1, :]
        _lib.call("dvh_select_mean_var", _lib.ptr(base), R * w, rows, _lib.ptr(sel_t), _lib.ptr(off_t), _lib.ptr(cnt_t),
                  B, _lib.ptr(out), rows, _lib.stream_of(self.device))
        return out

    def resample_images(self, sel, start_x=-150, end_x=0, transform="fk", stack="linear", power=2.0):
        """f-v images [B, Nvel, Nfreq] of every draw's stack (compute_disp_image(end_x, start_x, transform))."""
        check_transform(transform)
        check_stack(stack, power)
        sel = np.asarray(sel, dtype=np.int32)
        return self.images_of(self.resample_stacks(sel, start_x, end_x, stack=stack, power=power), sel[:, 0], start_x,
                              end_x, transform)


def plan_ridges(stacks, plan: SlantPlan, freq_lb, freq_ub, ref_freq_idx, sigma, vel_max, ref_vel,
                return_picks=False):
    """ridges() of every mode on the phase-shift images slant_maps(stacks, plan, norm=False) would give, without the
    images: the walk computes the values it compares (dvh_slant_ridge), each equal bit for bit to the image's, so
    picks and ridges are those of ridges(slant_maps(...), plan.freqs, plan.vels[::-1], ...).  ``plan``: velocities
    in descending order.  freq_lb, freq_ub, ref_freq_idx (an index into the band, or None), sigma and ref_vel are
    sequences over the modes.  Returns the list over modes of ridges()'s results."""
    return slant_ridges_finish(plan_ridges_launch(stacks, plan, freq_lb, freq_ub, ref_freq_idx, sigma, vel_max,
                                                  ref_vel, return_picks))


def plan_ridges_launch(stacks, plan: SlantPlan, freq_lb, freq_ub, ref_freq_idx, sigma, vel_max, ref_vel,
                       return_picks=False, side_streams=False):
    """The launches of plan_ridges() without the read-back: per mode (out, status, picks) device tensors for
    ridges_finish.  The stacks' spectra are formed once (dvh_disp_tdft) and shared by the modes; the image tensor is
    never allocated.  side_streams=True queues each mode's walk on a stream of its own, as convergence() does."""
    from .device import upload
    if plan.nV > 1 and not np.all(np.diff(plan.vels) < 0):
        raise ValueError("the fused ridge walk needs a plan with strictly descending vels")
    n_mode = len(freq_lb)
    bands = [_walk_band(plan.freqs, freq_lb[m], freq_ub[m], ref_freq_idx[m], ref_vel[m]) for m in range(n_mode)]
    D = _slant_spectra(stacks, plan, False)
    dev, B = stacks.device, stacks.shape[0]
    n_row = 0 if D is None else plan.n_row
    if D is None:
        D = torch.empty(2, dtype=torch.float64, device=dev)  # never read: the sums have no rows
    tb = plan.tables(dev)
    tabs = upload([np.asarray(_sg_ridge(), dtype=np.float64)] + [b[3] for b in bands if b[3] is not None], dev)
    sg, rest = tabs[0], iter(tabs[1:])
    vref = [next(rest) if b[3] is not None else None for b in bands]

    def launch(m):
        c0, nb, ref, _ = bands[m]
        out = torch.empty((B, nb), dtype=torch.float64, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        picks = torch.empty((B, nb), dtype=torch.float64, device=dev) if return_picks else None
        _lib.call("dvh_slant_ridge", _lib.ptr(D), B, n_row, max(plan.n_fb, 1), _lib.ptr(tb["fb"]),
                  _lib.ptr(tb["freqs"]), plan.nF, plan.dx, c0, nb, _lib.ptr(tb["vels"]), plan.nV, ref,
                  float(sigma[m]), float(vel_max), _lib.ptr(vref[m]), _lib.ptr(sg), 25, _lib.ptr(out),
                  _lib.ptr(status), _lib.ptr(picks), _lib.stream_of(dev))
        return out, status, picks
    if side_streams:
        return _on_side_streams(dev, n_mode, launch, [D, sg] + [v for v in vref if v is not None])
    return [launch(m) for m in range(n_mode)]


def slant_ridges(cache: GatherCache, stacks, first, freq_lb, freq_ub, ref_freq_idx, sigma, vel_max, ref_vel,
                 start_x=-150, end_x=0, return_picks=False):
    """plan_ridges() for the resample stacks [B, nch, W] of a gather cache whose first drawn passes are ``first``:
    each on its first pass's lag axis, as images_of(..., transform="slant") images them."""
    return slant_ridges_finish(slant_ridges_launch(cache, stacks, first, freq_lb, freq_ub, ref_freq_idx, sigma,
                                                   vel_max, ref_vel, start_x, end_x, return_picks))


def slant_ridges_finish(pending):
    """Host results of a slant_ridges_launch / plan_ridges_launch, mode by mode (synchronises; raises as
    ridges_finish does)."""
    return [ridges_finish(p) for p in pending]


def slant_ridges_launch(cache: GatherCache, stacks, first, freq_lb, freq_ub, ref_freq_idx, sigma, vel_max, ref_vel,
                        start_x=-150, end_x=0, return_picks=False, side_streams=False):
    """The launches of slant_ridges() without the read-back.  A cache of one lag length is one plan_ridges_launch;
    a mixed one walks each length's resamples with that length's plan and puts the results back in draw order."""
    args = (freq_lb, freq_ub, ref_freq_idx, sigma, vel_max, ref_vel, return_picks, side_streams)
    groups = cache._by_lag_length(first)
    if groups[0][1] is None:
        return plan_ridges_launch(stacks, cache.slant_plan(start_x, end_x, w=cache.W)[2], *args)
    pend = None
    for w, rows in groups:
        rt = torch.as_tensor(rows, device=cache.device)
        part = plan_ridges_launch(stacks[rt][:, :, :w], cache.slant_plan(start_x, end_x, w=w)[2], *args)
        if pend is None:
            pend = [tuple(None if t is None else torch.empty((stacks.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype,
                                                             device=t.device) for t in p) for p in part]
        for full, got in zip(pend, part):
            for f, g in zip(full, got):
                if f is not None:
                    f[rt] = g
    return pend


def _on_side_streams(device, n, launch, inputs):
    """launch(k) for k < n, each on the device's k-th side stream after the work queued so far on the current stream,
    which then waits for all of them.  ``inputs``: the tensors the launches read; launch(k) returns the tensors it
    writes (or None entries)."""
    main = torch.cuda.current_stream(device)
    ready = torch.cuda.Event()
    ready.record(main)
    out = []
    for k in range(n):
        st = _side_stream(device, k)
        st.wait_event(ready)
        with torch.cuda.stream(st):
            out.append(launch(k))
            for t in out[-1]:
                if t is not None:
                    t.record_stream(main)
        for t in inputs:
            t.record_stream(st)
        main.wait_stream(st)
    return out


def _band_ref(ref_freq_idx, freq_lb):
    """bootstrap_disp's ref_freq_idx (an index into FREQS) as an index into the band that starts at freq_lb."""
    return ref_freq_idx - int(np.sum(FREQS < freq_lb))


def bootstrap_ridges(cache: GatherCache, sels, sigma, ref_freq_idx, freq_lb, freq_up, ref_vel, start_x=-150,
                     end_x=0, transform="fk", walk=None, stack="linear", power=2.0):
    """Ridge velocities per mode for draws ``sels`` [B, k]: list over modes of [B, n_band] arrays.  ``transform``
    selects the image the ridges are walked on ("fk": map_fv, "slant": the phase-shift transform); with "slant",
    ``walk`` selects how: "image" forms the images and walks them (dvh_ridge), "fused" computes the compared values
    inside the walk (dvh_slant_ridge) with the same results, None takes SLANT_WALK.  ``stack`` and ``power`` select the
    stack of every draw (check_stack): the mean, or the phase-weighted stack."""
    walk = check_transform(transform, walk)
    check_stack(stack, power)
    if walk == "fused":
        sels = np.asarray(sels, dtype=np.int32)
        refs = [_band_ref(ref_freq_idx[m], freq_lb[m]) for m in range(len(freq_lb))]
        return slant_ridges(cache, cache.resample_stacks(sels, start_x, end_x, stack=stack, power=power), sels[:, 0],
                            freq_lb, freq_up, refs, sigma, 800, ref_vel, start_x, end_x)
    fv = cache.resample_images(sels, start_x, end_x, transform, stack, power)
    out = []
    for m in range(len(freq_lb)):
        out.append(ridges(fv, FREQS, VELS, freq_lb[m], freq_up[m], ref_freq_idx=_band_ref(ref_freq_idx[m], freq_lb[m]),
                          sigma=sigma[m], vel_max=800, ref_vel=ref_vel[m]))
    return out


def convergence(cache: GatherCache, max_size, bt_times, sigma, ref_freq_idx, freq_lb, freq_up, ref_vel, start_x=-150,
                end_x=0, rand=random, phases=None, transform="fk", walk=None, stack="linear", power=2.0):
    """The notebooks' convergence_test (imaging_diff_speed.ipynb#cell30) on a gather cache: for bt_size =
    1..max_size, bt_times resamples (the same random.sample draws in the same order as the notebook's
    per-size bootstrap_disp calls), their ridges per mode, and the summed per-frequency std -> [n_modes,
    max_size].  All max_size x bt_times resamples go through ONE dispersion batch (select_mean per size
    into one buffer, one tdft / fk / f-v launch each, one ridge launch per mode), so the host synchronises
    once per mode instead of once per (size, mode).  ``phases`` (optional dict) receives torch events
    around the resample / dispersion / ridge parts for timing.  ``transform`` and ``walk`` as bootstrap_ridges takes
    them; the fused walk forms no images (its "disp1" event follows "select1" at once).  ``stack`` and ``power`` as
    bootstrap_ridges takes them; the analytic signal of the cache is formed before the "select0" event."""
    walk = check_transform(transform, walk)
    check_stack(stack, power)
    if stack == "pws":
        cache.analytic()
    t_draw = time.perf_counter()
    sels = draw_sizes(cache.n, range(1, max_size + 1), bt_times, rand)
    if phases is not None:
        phases["draw_host_s"] = time.perf_counter() - t_draw
    B = max_size * bt_times
    ev = (lambda name: phases.setdefault(name, torch.cuda.Event(enable_timing=True)).record()) if phases is not None \
        else (lambda name: None)
    ev("select0")
    stacks = cache.resample_stacks_sizes(sels, start_x, end_x, stack=stack, power=power)
    ev("select1")
    first = np.concatenate([x[:, 0] for x in sels])
    refs = [_band_ref(ref_freq_idx[m], freq_lb[m]) for m in range(len(freq_lb))]
    out = np.empty((len(freq_lb), max_size))
    # every mode's walk queued at once, each on its own stream: one walk is one wave per resample (1 800 waves,
    # a fraction of the chip), so the modes run side by side; one wait below
    if walk == "fused":
        ev("disp1")
        pend = slant_ridges_launch(cache, stacks, first, freq_lb, freq_up, refs, sigma, 800, ref_vel, start_x, end_x,
                                   side_streams=True)
    else:
        fv = cache.images_of(stacks, first, start_x, end_x, transform)
        ev("disp1")
        pend = _on_side_streams(cache.device, len(freq_lb), lambda m: ridges_launch(
            fv, FREQS, VELS, freq_lb[m], freq_up[m], ref_freq_idx=refs[m], sigma=sigma[m], vel_max=800,
            ref_vel=ref_vel[m]), [fv])
    ev("ridge1")
    for m, pd in enumerate(pend):
        r = np.asarray(ridges_finish(pd))
        # per size: the std over its bt_times resamples of each frequency's pick, summed over frequencies
        out[m] = np.std(r.reshape(max_size, bt_times, -1), axis=1).sum(axis=1)
    return out


def draw(n, bt_size, bt_times, rand=random):
    """The reference's draws: bt_times x random.sample(range(1, n), bt_size), bit for bit, formed by the
    library's host routine from the generator's Mersenne Twister state (dvh_random_sample), which is handed
    back so that ``rand`` continues exactly as after Python's own calls.  ``rand``: the ``random`` module or a
    random.Random instance."""
    return draw_sizes(n, [bt_size], bt_times, rand)[0]


def draw_sizes(n, sizes, bt_times, rand=random):
    """[draw(n, k, bt_times, rand) for k in sizes] with one read and one write-back of the generator state."""
    for k in sizes:
        if not 0 <= k <= max(n - 1, 0):
            raise ValueError("Sample larger than population or is negative")
    version, mt, gauss = rand.getstate()
    st = np.array(mt, dtype=np.uint32)
    outs = []
    for k in sizes:
        out = np.empty((bt_times, k), dtype=np.int64)
        _lib.call("dvh_random_sample", st.ctypes.data, 1, max(n - 1, 0), k, bt_times, out.ctypes.data)
        outs.append(out.astype(np.int32))
    rand.setstate((version, tuple(int(v) for v in st), gauss))
    return outs


def save_ridge_npz(file_name, freqs, freq_lb, freq_ub, reference_layout=False, **ridges):
    """The ridge-statistics npz of the notebooks (imaging_diff_speed.ipynb#cell27, data/<x0>_speeds.npz:
    ``freqs, freq_lb, freq_ub, vels_<class>``) for bootstrap_disp results.  ``ridges``: class name ->
    ridge_vel, bootstrap_disp's list over modes of per-resample ridge arrays (modes have different band
    lengths).  By default the file is pickle-free: ``vels_<class>`` is omitted and each mode is a dense
    ``vels_<class>_m<k>`` [n_resample, n_band_k] array (load with allow_pickle=False, load_ridge_npz).
    reference_layout=True writes ``vels_<class>`` as the notebook's ragged object array instead (np.savez
    pickles it; only the notebook's own np.load(allow_pickle=True) reads that)."""
    out = dict(freqs=np.asarray(freqs, dtype=np.float64), freq_lb=np.asarray(freq_lb),
               freq_ub=np.asarray(freq_ub))
    for name, per_mode in ridges.items():
        if reference_layout:
            arr = np.empty(len(per_mode), dtype=object)
            for k, rv in enumerate(per_mode):
                arr[k] = list(rv)
            out[f"vels_{name}"] = arr
        else:
            for k, rv in enumerate(per_mode):
                out[f"vels_{name}_m{k}"] = np.asarray(rv, dtype=np.float64).reshape(len(rv), -1)
    np.savez(file_name, **out)


def load_ridge_npz(file_name):
    """(freqs, freq_lb, freq_ub, {class: [per-mode [n_resample, n_band] arrays]}) of a pickle-free
    save_ridge_npz file (allow_pickle=False)."""
    with np.load(file_name, allow_pickle=False) as f:
        ridges = {}
        for key in sorted(k for k in f.files if k.startswith("vels_")):
            name, _, m = key[5:].rpartition("_m")
            ridges.setdefault(name, {})[int(m)] = f[key]
        return (f["freqs"], f["freq_lb"], f["freq_ub"],
                {n: [d[k] for k in sorted(d)] for n, d in ridges.items()})
