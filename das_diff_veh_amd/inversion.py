"""Rayleigh-wave forward model and swarm inversion on the device: the stage of inversion_diff_speed.ipynb and
inversion_diff_weight.ipynb (disba's ``surf96`` and evodcinv's ``EarthModel.invert``).

Neither disba nor evodcinv is restated.  What is computed here is this build's own definition, documented in DESIGN.md:

  forward    dvh_rayleigh_modes: the secular function of csrc/rayleigh.h (real motion-stress vectors, the analytic
             layer propagator, re-orthonormalised sublayers), scanned at c_k = fma(k, dc, c_min) below the half-space
             beta; mode m is the (m + 1)-th sign change, refined to ``tol`` relative.  Roots closer than ``dc`` vanish
             in pairs, as in surf96's search.  Pinned to an 80-digit Thomson-Haskell oracle (tests/rayleigh_ref.py).
  misfit     dvh_curve_misfit: sum_i w_i sqrt(mean_j(((obs - c) / sigma)^2)) / sum_i w_i over the curves, +inf for a
             model that lacks a sampled mode.
  optimizer  global-best particle swarm on the unit cube of the bounds with the constriction values w = 0.7298,
             c1 = c2 = 1.49618; positions clamped to the cube, parameters with equal bounds held fixed.  evodcinv's
             "cpso" adds a competitive restart of particles, which is not restated: ``optimizer="cpso"`` raises.

``rayleigh_modes`` and ``EarthModel.invert`` are device work (float64) with no CPU fallback; all ``maxrun`` runs advance
together as independent swarms of one batch, one dvh_rayleigh_modes and one dvh_curve_misfit launch per iteration,
and nothing is read back before the last iteration.

The notebooks' import swap::

    from das_diff_veh_amd.inversion import EarthModel, Layer, Curve, phase_velocity
    from das_diff_veh_amd.inversion import PhaseSensitivity, group_velocity

``rayleigh_sensitivity`` and ``rayleigh_group`` (dvh_rayleigh_sens: the derivatives of the secular function taken
through its own recurrences, csrc/rayleigh_tangent.h) give dc/dp of every layer value and the group velocity at the
roots of ``rayleigh_modes``; ``PhaseSensitivity`` and ``group_velocity`` are their NumPy fronts for the notebooks.

``EarthModel.refine`` (dvh_lm_normal, dvh_lm_solve: csrc/refine.h) is a damped Gauss-Newton descent of the misfit from
the swarm's models, ``InversionResult.run_best()`` or any rows of ``xs``; its objective, step and acceptance rule are
this build's own ("Gauss-Newton refinement").

``EarthModel.refine_sets`` (dvh_lm_normal_sets) is the same descent with an observation set per model: an ensemble of
curve sets, such as one per bootstrap resample (``sets_from_ridges``), refined in one batch, and ``EnsembleResult``
turns the refined models into a spread of profiles over depth.  The swarm itself still takes one curve set.

``EarthModel.refine_section`` (dvh_lm_solve_chain) refines ordered sets, the pivots along the fibre or the days of a
time lapse, as chains: neighbouring models are tied by first differences in the unit cube, a chain's step is one
block-tridiagonal solve, and ``SectionResult.section`` lays the profiles out as [chain, position, depth] (DESIGN.md,
"Laterally constrained refinement").
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .device import default_device

MAX_LAYERS = 32  # DVH_RAYLEIGH_MAX_LAYERS
MAX_MODES = 16   # DVH_RAYLEIGH_MAX_MODES
PSO_W, PSO_C1, PSO_C2 = 0.7298, 1.49618, 1.49618


# --------------------------------------------------------------------------------------------------- forward calls

def _modes_into(models, periods, need, c_min, dc, tol, n_mode, out_c, out_count):
    M, n_layer, _ = models.shape
    _lib.call("dvh_rayleigh_modes", _lib.ptr(models), M, n_layer, _lib.ptr(periods), periods.numel(), _lib.ptr(need),
              float(c_min), float(dc), float(tol), int(n_mode), _lib.ptr(out_c), _lib.ptr(out_count),
              _lib.stream_of(models.device))


def rayleigh_modes(models, periods, n_mode, dc=0.005, c_min=None, tol=1e-9, need=None, return_count=False):
    """Modal Rayleigh phase velocities (km/s) of layered models on the device.

    models   float64 device tensor [M, n_layer, 4] of (h km, vp km/s, vs km/s, rho g/cm^3); the last layer is the
             half-space
    periods  float64 device tensor [P] (s)
    need     None (all ``n_mode`` modes at every period) or int32 [P]: the modes wanted per period, 0 skips it
    c_min    where the scan starts; None takes 0.8 min(vs) of this call's models (one read-back)
    ->       [M, P, n_mode], NaN where a mode is not wanted or has no root below the model's half-space vs (and, with
             ``return_count``, the int32 [M, P] number of roots bracketed)
    """
    if not (isinstance(models, torch.Tensor) and models.is_cuda):
        raise RuntimeError("rayleigh_modes needs device tensors (no CPU fallback)")
    if models.dim() != 3 or models.shape[-1] != 4 or models.dtype != torch.float64:
        raise ValueError("models must be float64 [M, n_layer, 4]")
    if not 1 <= models.shape[1] <= MAX_LAYERS:
        raise ValueError(f"1 .. {MAX_LAYERS} layers")
    if not 1 <= int(n_mode) <= MAX_MODES:
        raise ValueError(f"1 .. {MAX_MODES} modes")
    dev = models.device
    models = models.contiguous()
    periods = torch.as_tensor(periods, dtype=torch.float64, device=dev).reshape(-1).contiguous()
    M, P = models.shape[0], periods.numel()
    if need is None:
        need = torch.full((P,), int(n_mode), dtype=torch.int32, device=dev)
    else:
        need = torch.as_tensor(need, device=dev).to(torch.int32).reshape(-1).contiguous()
        if need.numel() != P:
            raise ValueError("need must have one entry per period")
    out_c = torch.empty((M, P, int(n_mode)), dtype=torch.float64, device=dev)
    out_count = torch.empty((M, P), dtype=torch.int32, device=dev)
    if M and P:
        if c_min is None:
            c_min = 0.8 * float(models[:, :, 2].min())
        _modes_into(models, periods, need, c_min, dc, tol, n_mode, out_c, out_count)
    return (out_c, out_count) if return_count else out_c


def phase_velocity(period, thickness, velocity_p, velocity_s, density, mode=0, dc=0.005):
    """The notebooks' ``surf96(period, thickness, velocity_p, velocity_s, density, mode, 0, rayleigh, dc)`` call of
    plot_predicted_curve: NumPy in, the phase velocity (km/s) of Rayleigh mode ``mode`` at every period out, NaN where
    the mode does not exist (so the notebooks' ``c > 0`` filter drops it)."""
    dev = default_device()
    layers = np.stack([np.asarray(a, np.float64).reshape(-1) for a in (thickness, velocity_p, velocity_s, density)], 1)
    period = np.ascontiguousarray(np.asarray(period, np.float64).reshape(-1))  # the notebooks pass reversed views
    if not 0 <= int(mode) < MAX_MODES:
        raise ValueError(f"mode must be 0 .. {MAX_MODES - 1}")
    c = rayleigh_modes(torch.from_numpy(np.ascontiguousarray(layers[None])).to(dev), torch.from_numpy(period).to(dev),
                       int(mode) + 1, dc=dc)
    return c[0, :, int(mode)].cpu().numpy()


# ------------------------------------------------------------------------------------------------- misfit

@dataclass
class SampleTable:
    """The curves of one inversion as dvh_curve_misfit takes them (device tensors) over the union of their periods."""
    periods: torch.Tensor
    need: torch.Tensor
    n_mode: int
    sample_period: torch.Tensor
    sample_mode: torch.Tensor
    sample_obs: torch.Tensor
    sample_sigma: torch.Tensor
    sample_curve: torch.Tensor
    curve_weight: torch.Tensor


def sample_table(curves, device=None):
    """The union of the curves' periods, the modes needed at each (the highest any curve samples there, plus one) and
    the sample table in curve order."""
    dev = device or default_device()
    curves = list(curves)
    if not curves:
        raise ValueError("no curves")
    for c in curves:
        c.check()
    periods = np.unique(np.concatenate([c.period for c in curves]))
    need = np.zeros(periods.size, np.int32)
    sp, sm, so, ss, sc = [], [], [], [], []
    for i, c in enumerate(curves):
        at = np.searchsorted(periods, c.period)
        np.maximum.at(need, at, c.mode + 1)
        sp.append(at)
        sm.append(np.full(at.size, c.mode))
        so.append(c.data)
        ss.append(np.ones(at.size) if c.uncertainties is None else c.uncertainties)
        sc.append(np.full(at.size, i))

    def put(parts, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts), dtype=dtype)).to(dev)

    return SampleTable(torch.from_numpy(periods).to(dev), torch.from_numpy(need).to(dev), int(need.max()),
                       put(sp, np.int32), put(sm, np.int32), put(so, np.float64), put(ss, np.float64),
                       put(sc, np.int32), put([[c.weight for c in curves]], np.float64))


def curve_misfit(c, table, out=None):
    """dvh_curve_misfit of c [M, P, n_mode] (a rayleigh_modes result on ``table.periods``) -> float64 [M]."""
    M, P, n_mode = c.shape
    if P != table.periods.numel() or n_mode != table.n_mode or c.dtype != torch.float64 or not c.is_contiguous():
        raise ValueError("c must be contiguous float64 [M, len(table.periods), table.n_mode]")
    if out is None:
        out = torch.empty(M, dtype=torch.float64, device=c.device)
    _lib.call("dvh_curve_misfit", _lib.ptr(c), M, P, n_mode, _lib.ptr(table.sample_period),
              _lib.ptr(table.sample_mode), _lib.ptr(table.sample_obs), _lib.ptr(table.sample_sigma),
              _lib.ptr(table.sample_curve), table.sample_obs.numel(), _lib.ptr(table.curve_weight),
              table.curve_weight.numel(), _lib.ptr(out), _lib.stream_of(c.device))
    return out


# ------------------------------------------------------------------------------------------------- the notebooks' classes

class Layer:
    """Search bounds of one layer: thickness (km), S-wave velocity (km/s) and Poisson's ratio, each (low, high)."""

    def __init__(self, thickness, velocity_s, poisson=(0.2, 0.4)):
        self.thickness, self.velocity_s, self.poisson = (self._pair(v) for v in (thickness, velocity_s, poisson))
        if self.thickness[0] < 0.0 or self.velocity_s[0] <= 0.0 or not 0.0 <= self.poisson[0] <= self.poisson[1] < 0.5:
            raise ValueError("thickness >= 0, velocity_s > 0 and 0 <= poisson < 0.5")

    @staticmethod
    def _pair(v):
        lo, hi = (float(x) for x in v)
        if not lo <= hi:
            raise ValueError(f"bounds {v!r} are not (low, high)")
        return lo, hi

    def __repr__(self):
        return f"Layer(thickness={self.thickness}, velocity_s={self.velocity_s}, poisson={self.poisson})"


class Curve:
    """One observed dispersion curve: periods (s), velocities (km/s), mode number, wave and type, weight and
    uncertainties (km/s; None weighs every sample alike)."""

    def __init__(self, period, data, mode, wave, type, weight=1.0, uncertainties=None):
        self.period = np.asarray(period, np.float64).reshape(-1)
        self.data = np.asarray(data, np.float64).reshape(-1)
        self.mode, self.wave, self.type, self.weight = int(mode), wave, type, float(weight)
        self.uncertainties = None if uncertainties is None else np.asarray(uncertainties, np.float64).reshape(-1)
        self.check()

    def check(self):
        if self.wave != "rayleigh":
            raise ValueError(f"wave {self.wave!r}: only 'rayleigh' curves are inverted")
        if self.type != "phase":
            raise ValueError(f"type {self.type!r}: only 'phase' velocities are inverted")
        if not 0 <= self.mode < MAX_MODES:
            raise ValueError(f"mode must be 0 .. {MAX_MODES - 1}")
        if self.period.size == 0 or self.data.size != self.period.size:
            raise ValueError("period and data must have the same, non-zero length")
        if self.uncertainties is not None and self.uncertainties.size != self.period.size:
            raise ValueError("uncertainties must match period")
        if not (np.all(self.period > 0) and np.all(np.isfinite(self.data)) and self.weight > 0):
            raise ValueError("periods and weight must be positive, data finite")
        if self.uncertainties is not None and not np.all(self.uncertainties > 0):
            raise ValueError("uncertainties must be positive")


@dataclass
class InversionResult:
    """Every model the swarms evaluated, in (run, iteration, particle) order.

    xs       [n_eval, 3 n - 1]  parameters [h(0 .. n-2), vs(0 .. n-1), nu(0 .. n-1)]
    models   [n_eval, n, 4]     (h, vp, vs, rho) rows; ``model.T`` unpacks into phase_velocity's arguments
    misfits  [n_eval]
    model, misfit               the best of them
    global_misfits [maxrun, maxiter]  each run's best-so-far after every iteration, as the optimizer held it
    """
    xs: np.ndarray
    models: np.ndarray
    misfits: np.ndarray
    global_misfits: np.ndarray
    maxrun: int
    popsize: int
    maxiter: int
    timings: dict = field(default_factory=dict)

    @property
    def model(self):
        return self.models[int(np.argmin(self.misfits))]

    @property
    def misfit(self):
        return self.misfits.min()

    def run_best(self):
        """[maxrun, 3 n - 1]: the best model each run evaluated (its first, where several tie), the rows that
        ``EarthModel.refine`` starts from."""
        per_run = self.misfits.reshape(self.maxrun, -1)
        at = np.argmin(per_run, axis=1) + np.arange(self.maxrun) * per_run.shape[1]
        return self.xs[at].copy()


def starts_in_bounds(xs, lo, hi):
    """Whether every row of xs (NumPy or a tensor, [M, D]) lies within one ulp of the cube lo .. hi (NumPy [D]): the
    test ``EarthModel.refine`` applies to its starts.  lo + u (hi - lo), as ``invert`` forms its models, can round to
    one ulp above hi at u = 1."""
    below, above = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    if isinstance(xs, torch.Tensor):
        below, above = (torch.from_numpy(b).to(xs.device) for b in (below, above))
    return bool(((xs >= below) & (xs <= above)).all())


LM_MAX_PARAMS = 96  # DVH_LM_MAX_PARAMS
LM_MAX_CURVES = 64  # DVH_LM_MAX_CURVES
LM_RHO_FLOOR = 1e-12
LM_LAMBDA_MIN, LM_LAMBDA_MAX = 1e-12, 1e12


@dataclass
class RefineResult:
    """What ``EarthModel.refine`` returns for its M starts (NumPy arrays).

    xs, models        [M, 3 n - 1], [M, n, 4]  the refined models, inside the bounds; a start that was never improved
                      is returned as given (clamped, if it was an ulp outside)
    misfits           [M]  dvh_lm_normal's f at ``models`` (polished roots)
    start_misfits     [M]  the same at the starts
    history           [maxiter + 1, M]  the kept f after every iteration; row 0 is ``start_misfits``
    accepted          [maxiter, M] bool  whether the iteration's trial was taken
    lam               [M]  the damping after the last iteration
    status            [M] int32  bit 0: the start has f = +inf (a sampled mode is missing) and stayed where it was;
                      bit 1: the last damped system had no positive pivot (no step was taken from it)
    gradient, hessian [M, D], [M, D, D]  g and H of the final point, in the unit cube u of the bounds
    """
    xs: np.ndarray
    models: np.ndarray
    misfits: np.ndarray
    start_misfits: np.ndarray
    history: np.ndarray
    accepted: np.ndarray
    lam: np.ndarray
    status: np.ndarray
    gradient: np.ndarray
    hessian: np.ndarray
    timings: dict = field(default_factory=dict)


def lm_normal(c, dcdp, chain, table, rho_floor=LM_RHO_FLOOR):
    """dvh_lm_normal of c [M, P, n_mode] and dcdp [M, P, n_mode, n_layer, 4] (dvh_rayleigh_sens on ``table.periods``)
    and chain [M, 4 n_layer, D] -> (f [M], g [M, D], H [M, D, D], status int32 [M]) on the device."""
    M, P, n_mode = c.shape
    n_layer, D = dcdp.shape[3], chain.shape[2]
    if P != table.periods.numel() or n_mode != table.n_mode or dcdp.shape != (M, P, n_mode, n_layer, 4) or \
            chain.shape != (M, 4 * n_layer, D):
        raise ValueError("c [M, P, n_mode], dcdp [M, P, n_mode, n_layer, 4] and chain [M, 4 n_layer, D] on the table")
    for t in (c, dcdp, chain):
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("c, dcdp and chain must be contiguous float64 device tensors")
    dev = c.device
    f = torch.empty(M, dtype=torch.float64, device=dev)
    g = torch.empty((M, D), dtype=torch.float64, device=dev)
    H = torch.empty((M, D, D), dtype=torch.float64, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    _lib.call("dvh_lm_normal", _lib.ptr(c), _lib.ptr(dcdp), _lib.ptr(chain), M, P, n_mode, n_layer, D,
              _lib.ptr(table.sample_period), _lib.ptr(table.sample_mode), _lib.ptr(table.sample_obs),
              _lib.ptr(table.sample_sigma), _lib.ptr(table.sample_curve), table.sample_obs.numel(),
              _lib.ptr(table.curve_weight), table.curve_weight.numel(), float(rho_floor), _lib.ptr(f), _lib.ptr(g),
              _lib.ptr(H), _lib.ptr(status), _lib.stream_of(dev))
    return f, g, H, status


def lm_solve(H, g, lam, free):
    """dvh_lm_solve: (H + lam diag(d)) delta = -g over the parameters with free != 0 -> (delta [M, D], status [M])."""
    M, D = g.shape
    if H.shape != (M, D, D) or lam.shape != (M,) or free.shape != (D,) or free.dtype != torch.int32:
        raise ValueError("H [M, D, D], g [M, D], lam [M] and int32 free [D]")
    for t in (H, g, lam, free):
        if not t.is_contiguous() or not t.is_cuda or (t is not free and t.dtype != torch.float64):
            raise ValueError("H, g and lam must be contiguous float64 device tensors")
    delta = torch.empty_like(g)
    status = torch.empty(M, dtype=torch.int32, device=g.device)
    _lib.call("dvh_lm_solve", _lib.ptr(H), _lib.ptr(g), _lib.ptr(lam), _lib.ptr(free), M, D, _lib.ptr(delta),
              _lib.ptr(status), _lib.stream_of(g.device))
    return delta, status


def lm_solve_chain(H, g, u, lam, free, mu, link, chain_len):
    """dvh_lm_solve_chain: the damped step of C = M / chain_len chains of models tied by first differences (DESIGN.md,
    "Laterally constrained refinement") -> (delta [M, D], status int32 [C]).  Rows c chain_len + k of H [M, D, D],
    g [M, D] and u [M, D] (the unit cube) are the positions of chain c; lam is [C], free int32 [D], mu [D] and link
    [C, chain_len - 1] are the coupling and the link weights, all device tensors (mu and link >= 0: not checked
    here)."""
    M, D = g.shape
    L = int(chain_len)
    if L < 1 or M % L:
        raise ValueError(f"{M} rows are not chains of {chain_len}")
    C = M // L
    if H.shape != (M, D, D) or u.shape != (M, D) or lam.shape != (C,) or free.shape != (D,) or \
            free.dtype != torch.int32 or mu.shape != (D,) or link.shape != (C, L - 1):
        raise ValueError("H [M, D, D], g and u [M, D], lam [C], int32 free [D], mu [D] and link [C, chain_len - 1]")
    for t in (H, g, u, lam, free, mu, link):
        if not t.is_contiguous() or not t.is_cuda or (t is not free and t.dtype != torch.float64):
            raise ValueError("H, g, u, lam, mu and link must be contiguous float64 device tensors")
    delta = torch.empty_like(g)
    status = torch.empty(C, dtype=torch.int32, device=g.device)
    work = torch.empty(max(_lib.load().dvh_lm_solve_chain_workspace(M, D) // 8, 1), dtype=torch.float64,
                       device=g.device)
    if link.numel() == 0:  # chains of one position have no link, and an empty tensor has no address
        link = link.new_zeros(1)
    _lib.call("dvh_lm_solve_chain", _lib.ptr(H), _lib.ptr(g), _lib.ptr(u), _lib.ptr(lam), _lib.ptr(free),
              _lib.ptr(mu), _lib.ptr(link), C, L, D, _lib.ptr(work), _lib.ptr(delta), _lib.ptr(status),
              _lib.stream_of(g.device))
    return delta, status


def coupling_terms(u, mu, link):
    """The penalty and its gradient of chains in the unit cube (torch ops on any device): u [C, L, D], mu [D] (0 for a
    parameter that is not coupled, fixed ones included), link [C, L - 1] -> (P [C], q [C, L, D]) with
    P_c = 1/2 sum_k w_{c,k} sum_d mu_d (u_{k+1,d} - u_{k,d})^2 and q = dP/du."""
    du = u[:, 1:] - u[:, :-1]
    t = (link[:, :, None] * mu) * du
    q = torch.zeros_like(u)
    q[:, 1:] += t
    q[:, :-1] -= t
    return 0.5 * (t * du).sum(dim=(1, 2)), q


# ------------------------------------------------------------------------------------------------- observation sets

@dataclass
class ObservationSets:
    """K observation sets on one sample table (dvh_lm_normal_sets): ``table`` is ``sample_table`` of the templates,
    ``obs`` and ``sigma`` are float64 device tensors [K, S] in its sample order, NaN in ``obs`` for an absent sample."""
    table: SampleTable
    obs: torch.Tensor
    sigma: torch.Tensor

    @property
    def n_set(self):
        return self.obs.shape[0]


def _checked_sets(curves, data_sets, uncertainty_sets):
    """The host half of ``observation_sets``: every check, and (obs, sigma) as NumPy [K, S] in table order."""
    curves = list(curves)
    if not curves:
        raise ValueError("no curves")
    for c in curves:
        if not isinstance(c, Curve):
            raise TypeError("observation sets take Curve templates")
        c.check()

    def rows(parts, what):
        parts = list(parts)
        if len(parts) != len(curves):
            raise ValueError(f"{what}: one array per curve")
        parts = [np.asarray(p, np.float64) for p in parts]
        for p, c in zip(parts, curves):
            if p.ndim != 2 or p.shape != (parts[0].shape[0], c.period.size):
                raise ValueError(f"{what}: every array must be [K, len(curve.period)] with one K")
        return np.ascontiguousarray(np.concatenate(parts, axis=1))

    obs = rows(data_sets, "data_sets")
    if obs.shape[0] < 1:
        raise ValueError("at least one set (K >= 1)")
    if np.isinf(obs).any():
        raise ValueError("data must be finite, or NaN for an absent sample")
    if uncertainty_sets is None:
        own = [np.ones(c.period.size) if c.uncertainties is None else c.uncertainties for c in curves]
        sigma = np.ascontiguousarray(np.broadcast_to(np.concatenate(own), obs.shape))
    else:
        sigma = rows(uncertainty_sets, "uncertainty_sets")
        if sigma.shape != obs.shape:
            raise ValueError("uncertainty_sets must have the shapes of data_sets")
    at = np.isfinite(obs)
    if not (np.isfinite(sigma[at]).all() and (sigma[at] > 0).all()):
        raise ValueError("uncertainties must be positive and finite at every present sample")
    return obs, sigma


def _sets_on(curves, obs, sigma, dev):
    return ObservationSets(sample_table(curves, dev), torch.from_numpy(obs).to(dev), torch.from_numpy(sigma).to(dev))


def observation_sets(curves, data_sets, uncertainty_sets=None, device=None):
    """K observation sets of one group of curves, as ``lm_normal_sets`` takes them -> ObservationSets.

    curves            ``Curve`` templates: their period, mode, weight and uncertainties are used, their data is not
    data_sets         a list over the curves of [K, len(curve.period)] arrays (km/s); NaN marks a sample the set lacks
                      (a resample whose ridge has no pick there, a class without that mode's curve)
    uncertainty_sets  None (each curve's own uncertainties, or 1, shared by all sets) or arrays of the same shapes

    ValueError, before any device work, for shapes that do not match, K < 1, +-inf data or an uncertainty that is not
    positive and finite at a present sample."""
    obs, sigma = _checked_sets(curves, data_sets, uncertainty_sets)
    return _sets_on(list(curves), obs, sigma, device or default_device())


def lm_normal_sets(c, dcdp, chain, sets, model_set, rho_floor=LM_RHO_FLOOR):
    """dvh_lm_normal_sets: ``lm_normal`` with model m scored against row ``model_set[m]`` (an int32 device tensor [M])
    of ``sets`` (ObservationSets) -> (f [M], g [M, D], H [M, D, D], status int32 [M]) on the device."""
    table = sets.table
    M, P, n_mode = c.shape
    n_layer, D = dcdp.shape[3], chain.shape[2]
    if P != table.periods.numel() or n_mode != table.n_mode or dcdp.shape != (M, P, n_mode, n_layer, 4) or \
            chain.shape != (M, 4 * n_layer, D):
        raise ValueError("c [M, P, n_mode], dcdp [M, P, n_mode, n_layer, 4] and chain [M, 4 n_layer, D] on the table")
    for t in (c, dcdp, chain):
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("c, dcdp and chain must be contiguous float64 device tensors")
    S = table.sample_curve.numel()
    for t in (sets.obs, sets.sigma):
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda or t.dim() != 2 or \
                t.shape != (sets.n_set, S) or sets.n_set < 1:
            raise ValueError("sets.obs and sets.sigma must be contiguous float64 device tensors [K, S], K >= 1")
    if not isinstance(model_set, torch.Tensor) or model_set.shape != (M,) or model_set.dtype != torch.int32 or \
            not model_set.is_contiguous() or not model_set.is_cuda:
        raise ValueError("model_set must be a contiguous int32 device tensor [M]")
    dev = c.device
    f = torch.empty(M, dtype=torch.float64, device=dev)
    g = torch.empty((M, D), dtype=torch.float64, device=dev)
    H = torch.empty((M, D, D), dtype=torch.float64, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    _lib.call("dvh_lm_normal_sets", _lib.ptr(c), _lib.ptr(dcdp), _lib.ptr(chain), M, P, n_mode, n_layer, D,
              _lib.ptr(table.sample_period), _lib.ptr(table.sample_mode), _lib.ptr(sets.obs), _lib.ptr(sets.sigma),
              _lib.ptr(model_set), sets.n_set, _lib.ptr(table.sample_curve), S, _lib.ptr(table.curve_weight),
              table.curve_weight.numel(), float(rho_floor), _lib.ptr(f), _lib.ptr(g), _lib.ptr(H), _lib.ptr(status),
              _lib.stream_of(dev))
    return f, g, H, status


ProfileStats = namedtuple("ProfileStats", "mean std percentiles")


@dataclass
class EnsembleResult(RefineResult):
    """What ``EarthModel.refine_sets`` returns: RefineResult's fields for its M starts, and

    model_set  [M] int32  the set each row was refined against
    n_set      K, the number of sets
    """
    model_set: np.ndarray = None
    n_set: int = 0

    def best_per_set(self):
        """[K] row indices: per set the row of the lowest misfit among those refined against it (the first, where
        several tie), -1 for a set whose rows are all +inf or that no row names."""
        f = np.where(np.isnan(self.misfits), np.inf, self.misfits)
        best = np.full(self.n_set, -1, np.int64)
        for k in range(self.n_set):
            rows = np.flatnonzero(self.model_set == k)
            if rows.size and f[rows].min() < np.inf:
                best[k] = rows[np.argmin(f[rows])]
        return best

    def profiles(self, depths_km, parameter="velocity_s"):
        """[M, Z]: every row's layer value of ``parameter`` ("thickness", "velocity_p", "velocity_s" or "density") at
        each depth (km).  A depth on an interface takes the layer below; below the last interface it is the
        half-space's.  Host NumPy."""
        col, = _parameter_columns(parameter)
        z = np.asarray(depths_km, np.float64).reshape(-1)
        interfaces = np.cumsum(self.models[:, :-1, 0], axis=1)                     # [M, n - 1]
        layer = (z[None, None, :] >= interfaces[:, :, None]).sum(axis=1)           # [M, Z]
        return np.take_along_axis(self.models[:, :, col], layer, axis=1)

    def profile_stats(self, depths_km, parameter="velocity_s", percentiles=(0, 25, 50, 75, 100), rows=None):
        """Mean [Z], standard deviation [Z] and ``np.percentile`` [len(percentiles), Z] of ``profiles`` per depth over
        ``rows`` (default: ``best_per_set()`` without the sets that have none) -> ProfileStats."""
        if rows is None:
            rows = self.best_per_set()
            rows = rows[rows >= 0]
        rows = np.asarray(rows, np.int64).reshape(-1)
        if rows.size == 0:
            raise ValueError("no rows to take the statistics over")
        p = self.profiles(depths_km, parameter)[rows]
        return ProfileStats(p.mean(axis=0), p.std(axis=0), np.percentile(p, percentiles, axis=0))


@dataclass
class SectionResult(EnsembleResult):
    """What ``EarthModel.refine_section`` returns: EnsembleResult's fields for the M = n_chain chain_len rows (row
    c chain_len + k is position k of chain c), with ``accepted`` and ``lam`` of a chain repeated over its rows,
    ``gradient`` and ``hessian`` the data terms g_k and H_k (0 at a gap), and

    n_chain, chain_len   C and L
    coupling             [D] mu as given (a scalar broadcast); a fixed parameter takes no part whatever its mu
    link_weights         [C, L - 1] w
    gap                  [M] bool  rows whose set has no present sample
    objective, penalty   [C]  Phi_c and P_c at ``xs``
    objective_history    [maxiter + 1, C]  the kept Phi_c after every iteration; row 0 is the starts'
    chain_status         [C] int32  bit 0: the chain was not alive (a non-gap row starts at f = +inf, or every row is a
                         gap) and its rows are returned as given; bit 1: the last damped system had no positive pivot

    A gap row of a live chain has ``misfits`` (and its column of ``history``) NaN and status bit 2 (value 4): it is
    carried by its neighbours.  The rows of a chain that is not alive are what ``refine_sets`` returns for them."""
    n_chain: int = 0
    chain_len: int = 0
    coupling: np.ndarray = None
    link_weights: np.ndarray = None
    gap: np.ndarray = None
    objective: np.ndarray = None
    penalty: np.ndarray = None
    objective_history: np.ndarray = None
    chain_status: np.ndarray = None

    def section(self, depths_km, parameter="velocity_s"):
        """[C, L, Z]: ``profiles`` with the rows laid out as chains and positions."""
        p = self.profiles(depths_km, parameter)
        return p.reshape(self.n_chain, self.chain_len, p.shape[1])


def _checked_model_set(model_set, M, K):
    """``refine_sets``' model_set [M] within 0 .. K - 1 as int32 (None: M == K, start k on set k)."""
    if model_set is None:
        if M != K:
            raise ValueError(f"{M} starts for {K} sets: pass model_set")
        model_set = np.arange(K)
    model_set = np.asarray(model_set)
    if model_set.shape != (M,) or model_set.dtype.kind not in "iu" or \
            (M and not (0 <= model_set.min() and model_set.max() < K)):
        raise ValueError(f"model_set must be int [{M}] within 0 .. {K - 1}")
    return np.ascontiguousarray(model_set, np.int32)


def _checked_chains(M, D, chain_len, coupling, link_weights):
    """The chain arguments of ``refine_section`` -> (C, L, mu [D], w [C, L - 1]) as NumPy, or ValueError."""
    L = M if chain_len is None else int(chain_len)
    if L < 1 or M % L:
        raise ValueError(f"{M} rows are not chains of chain_len = {chain_len}")
    C = M // L
    mu = np.asarray(coupling, np.float64)
    if mu.shape not in ((), (D,)):
        raise ValueError(f"coupling must be a scalar or [{D}]")
    mu = np.array(np.broadcast_to(mu, (D,)))  # a copy: broadcast views are read-only
    w = np.ones((C, L - 1)) if link_weights is None else np.asarray(link_weights, np.float64)
    if w.shape not in ((L - 1,), (C, L - 1)):
        raise ValueError(f"link_weights must be [{L - 1}] or [{C}, {L - 1}]")
    w = np.array(np.broadcast_to(w, (C, L - 1)))
    for name, a in (("coupling", mu), ("link_weights", w)):
        if not (np.isfinite(a).all() and (a >= 0).all()):
            raise ValueError(f"{name} must be finite and not negative")
    return C, L, mu, w


def sets_from_ridges(freqs, freq_lb, freq_ub, ridges, modes, weights=None, uncertainties="std", stride=1):
    """The bridge from ``bootstrap.bootstrap_ridges`` to ``refine_sets``: one observation set per resample.

    freqs, freq_lb, freq_ub   the frequency axis (Hz) and the picked bands' bounds: band i is lb[i] <= f < ub[i]
    ridges         a list over the picked bands of [B, n_band] ridge velocities (m/s) on that band, NaN where a
                   resample has no pick
    modes          the Rayleigh mode number of each band's curve
    weights        the curves' weights (None: 1 each)
    uncertainties  "std": each template's uncertainties are the standard deviation over the resamples per frequency
                   (NaN ignored), a frequency where it is 0 taking the smallest positive one of its band, and None if
                   the band has none; None: no uncertainties
    stride         every stride-th frequency of a band is kept, counted from its first

    -> (curves, data_sets): ``Curve`` templates on ascending periods (the frequencies reversed, as the notebooks build
    theirs) with the resamples' mean as data, and per curve the [B, n] velocities in km/s.  NumPy only."""
    if uncertainties not in ("std", None):
        raise ValueError('uncertainties must be "std" or None')
    freqs = np.asarray(freqs, np.float64).reshape(-1)
    ridges = list(ridges)
    modes = list(modes)
    weights = [1.0] * len(ridges) if weights is None else list(weights)
    if not len(ridges) == len(modes) == len(weights) == len(freq_lb) == len(freq_ub) or not ridges:
        raise ValueError("one band bound, mode and weight per array of ridges, at least one")
    if int(stride) < 1:
        raise ValueError("stride >= 1")
    curves, data_sets = [], []
    for i, ridge in enumerate(ridges):
        band = freqs[(freqs >= freq_lb[i]) & (freqs < freq_ub[i])]
        ridge = np.asarray(ridge, np.float64)
        if ridge.ndim != 2 or ridge.shape[0] < 1 or ridge.shape[1] != band.size or band.size == 0:
            raise ValueError(f"ridges[{i}] must be [B, {band.size}] on its band, which must not be empty")
        if ridge.shape[0] != np.shape(ridges[0])[0]:
            raise ValueError("every band needs the same number of resamples")
        keep = slice(None, None, int(stride))
        period = (1.0 / band[keep])[::-1]
        data = np.ascontiguousarray(ridge[:, keep][:, ::-1] / 1000.0)
        if np.isinf(data).any() or not np.isfinite(data).any(axis=0).all():
            raise ValueError(f"ridges[{i}] must be finite or NaN, with a pick at every frequency in some resample")
        mean = np.nanmean(data, axis=0)
        sigma = None
        if uncertainties == "std":
            sigma = np.nanstd(data, axis=0)
            sigma = np.where(sigma > 0, sigma, sigma[sigma > 0].min()) if (sigma > 0).any() else None
        curves.append(Curve(period, mean, int(modes[i]), "rayleigh", "phase", weight=float(weights[i]),
                            uncertainties=sigma))
        data_sets.append(data)
    return curves, data_sets


class EarthModel:
    """evodcinv's EarthModel as the notebooks use it: add(Layer) top to bottom, configure(...), invert(curves)."""

    def __init__(self):
        self.layers = []
        self._configured = False

    def add(self, layer):
        if not isinstance(layer, Layer):
            raise TypeError("add() takes a Layer")
        if len(self.layers) == MAX_LAYERS:
            raise ValueError(f"at most {MAX_LAYERS} layers")
        self.layers.append(layer)
        return self

    def configure(self, optimizer="pso", misfit="rmse", density=None, optimizer_args=None, dc=0.005):
        """density: a callable of vp (km/s) made of arithmetic that a torch tensor takes, such as the notebooks'
        ``lambda vp: 1.56 + 0.186 * vp`` (it is applied to the swarm's device tensor inside the loop).
        optimizer_args: popsize, maxiter, seed (``workers`` is accepted and ignored)."""
        if optimizer == "cpso":
            raise ValueError('optimizer "cpso": its competitive restart is not restated here; pass optimizer="pso"')
        if optimizer != "pso":
            raise ValueError(f'optimizer {optimizer!r}: only "pso" is built')
        if misfit != "rmse":
            raise ValueError(f'misfit {misfit!r}: only "rmse" is built')
        if not callable(density):
            raise ValueError("density must be a callable of vp (evodcinv's named curves are not restated)")
        args = dict(popsize=10, maxiter=100, seed=None, workers=None)
        unknown = set(optimizer_args or {}) - set(args)
        if unknown:
            raise ValueError(f"unknown optimizer_args {sorted(unknown)}")
        args.update(optimizer_args or {})
        if int(args["popsize"]) < 2 or int(args["maxiter"]) < 1 or not float(dc) > 0.0:
            raise ValueError("popsize >= 2, maxiter >= 1 and dc > 0")
        self.density, self.dc = density, float(dc)
        self.popsize, self.maxiter, self.seed = int(args["popsize"]), int(args["maxiter"]), args["seed"]
        self._configured = True
        return self

    def bounds(self):
        """(low, high) of the parameter vector [h(0 .. n-2), vs(0 .. n-1), nu(0 .. n-1)]."""
        L = self.layers
        rows = [l.thickness for l in L[:-1]] + [l.velocity_s for l in L] + [l.poisson for l in L]
        b = np.array(rows, np.float64)
        return b[:, 0].copy(), b[:, 1].copy()

    def models_of(self, xs):
        """Parameters [..., 3 n - 1] (a device tensor) -> (h, vp, vs, rho) rows [..., n, 4]; the half-space's h is 0."""
        n = len(self.layers)
        h, vs, nu = xs[..., :n - 1], xs[..., n - 1:2 * n - 1], xs[..., 2 * n - 1:]
        vp = vs * torch.sqrt((2.0 - 2.0 * nu) / (1.0 - 2.0 * nu))
        rho = torch.as_tensor(self.density(vp), dtype=torch.float64, device=xs.device).expand_as(vp)
        h = torch.cat([h, torch.zeros_like(vs[..., :1])], dim=-1)
        return torch.stack([h, vp, vs, rho], dim=-1)

    def invert(self, curves, maxrun=1, profile=False):
        """``maxrun`` independent swarms of ``popsize`` particles for ``maxiter`` iterations -> InversionResult.
        ``profile`` records device events around every iteration's dvh_rayleigh_modes launch and the rest of the
        iteration (read after the last one) into ``result.timings`` (ms per iteration)."""
        if not self._configured:
            raise ValueError("configure() the model first")
        if len(self.layers) < 1:
            raise ValueError("add() at least one layer")
        if int(maxrun) < 1:
            raise ValueError("maxrun >= 1")
        curves = list(curves)
        for c in curves:  # before any device work
            if not isinstance(c, Curve):
                raise TypeError("invert() takes Curve objects")
            c.check()
        dev = default_device()
        tab = sample_table(curves, dev)
        R, N, T = int(maxrun), self.popsize, self.maxiter
        lo_h, hi_h = self.bounds()
        D = lo_h.size
        c_min = 0.8 * min(l.velocity_s[0] for l in self.layers)
        lo = torch.from_numpy(lo_h).to(dev)
        span = torch.from_numpy(hi_h - lo_h).to(dev)
        free = (span > 0).to(torch.float64)
        gen = torch.Generator(device=dev)
        if self.seed is None:
            gen.seed()
        else:
            gen.manual_seed(int(self.seed))

        def rand():
            return torch.rand((R, N, D), dtype=torch.float64, device=dev, generator=gen)

        u = rand() * free
        v = torch.zeros_like(u)
        pbest_u = u.clone()
        pbest_f = torch.full((R, N), float("inf"), dtype=torch.float64, device=dev)
        hist_x = torch.empty((T, R, N, D), dtype=torch.float64, device=dev)
        hist_f = torch.empty((T, R, N), dtype=torch.float64, device=dev)
        hist_g = torch.empty((T, R), dtype=torch.float64, device=dev)
        P = tab.periods.numel()
        c = torch.empty((R * N, P, tab.n_mode), dtype=torch.float64, device=dev)
        count = torch.empty((R * N, P), dtype=torch.int32, device=dev)
        events = []
        for it in range(T):
            x = hist_x[it]
            torch.addcmul(lo, u, span, out=x)
            models = self.models_of(x).reshape(R * N, len(self.layers), 4).contiguous()
            if profile:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
            _modes_into(models, tab.periods, tab.need, c_min, self.dc, 1e-9, tab.n_mode, c, count)
            if profile:
                ev[1].record()
            f = curve_misfit(c, tab, out=hist_f[it].view(-1)).view(R, N)
            better = f < pbest_f
            pbest_f = torch.where(better, f, pbest_f)
            pbest_u = torch.where(better[..., None], u, pbest_u)
            g_f, g_at = pbest_f.min(dim=1)
            hist_g[it] = g_f
            g_u = torch.gather(pbest_u, 1, g_at[:, None, None].expand(R, 1, D))
            v = (PSO_W * v + PSO_C1 * rand() * (pbest_u - u) + PSO_C2 * rand() * (g_u - u)) * free
            u = torch.clamp(u + v, 0.0, 1.0)
            if profile:
                ev[2].record()
                events.append(ev)
        # (T, R, N) -> (R, T, N): a run's evaluations are contiguous, in iteration order
        xs = hist_x.permute(1, 0, 2, 3).reshape(R * T * N, D)
        models = self.models_of(xs).cpu().numpy()
        res = InversionResult(xs.cpu().numpy(), models, hist_f.permute(1, 0, 2).reshape(-1).cpu().numpy(),
                              hist_g.t().contiguous().cpu().numpy(), R, N, T)
        if profile:
            torch.cuda.synchronize(dev)
            res.timings = dict(modes_ms=np.array([e[0].elapsed_time(e[1]) for e in events]),
                               rest_ms=np.array([e[1].elapsed_time(e[2]) for e in events]))
        return res

    def chain(self, xs, span=None):
        """The derivative of ``models_of``'s rows with respect to the unit cube u of the bounds (x = lo + u (hi - lo)):
        parameters [M, 3 n - 1] (a device or CPU tensor) -> [M, 4 n, D], row 4 l + q for column q of layer l.

        With g = sqrt((2 - 2 nu) / (1 - 2 nu)): dh/dh = dvs/dvs = 1, dvp/dvs = g, dvp/dnu = vs / (g (1 - 2 nu)^2) and
        drho = rho'(vp) dvp, each times the parameter's span; rho' is taken by autograd on the density callable (0 for
        one that returns a constant).  A fixed parameter's column and the half-space's h row are 0.  Torch ops only.
        ``span`` is hi - lo of ``bounds()`` as a tensor on xs's device, for a caller that holds it already."""
        n = len(self.layers)
        D = 3 * n - 1
        if not isinstance(xs, torch.Tensor) or xs.dim() != 2 or xs.shape[1] != D or xs.dtype != torch.float64:
            raise ValueError(f"xs must be a float64 tensor [M, {D}]")
        if span is None:
            lo_h, hi_h = self.bounds()
            span = torch.from_numpy(hi_h - lo_h).to(xs.device)
        xs = xs.detach()
        vs, nu = xs[:, n - 1:2 * n - 1], xs[:, 2 * n - 1:]
        g = torch.sqrt((2.0 - 2.0 * nu) / (1.0 - 2.0 * nu))
        with torch.enable_grad():
            vp = (vs * g).clone().requires_grad_(True)
            rho = self.density(vp)
            if isinstance(rho, torch.Tensor) and rho.requires_grad:
                drho, = torch.autograd.grad(rho.expand_as(vp).sum(), vp)
            else:
                drho = torch.zeros_like(vp)
        dvp_dvs = g * span[n - 1:2 * n - 1]
        dvp_dnu = vs / (g * (1.0 - 2.0 * nu) ** 2) * span[2 * n - 1:]
        out = torch.zeros((xs.shape[0], n, 4, D), dtype=torch.float64, device=xs.device)
        at = torch.arange(n, device=xs.device)
        out[:, at[:-1], 0, at[:-1]] = span[:n - 1]
        out[:, at, 1, n - 1 + at] = dvp_dvs
        out[:, at, 1, 2 * n - 1 + at] = dvp_dnu
        out[:, at, 2, n - 1 + at] = span[n - 1:2 * n - 1]
        out[:, at, 3, n - 1 + at] = drho * dvp_dvs
        out[:, at, 3, 2 * n - 1 + at] = drho * dvp_dnu
        return out.reshape(xs.shape[0], 4 * n, D)

    def refine(self, curves, xs, maxiter=20, lam0=1e-3, tol=1e-9, profile=False):
        """A damped Gauss-Newton (Levenberg-Marquardt) descent of the misfit from each row of ``xs`` -> RefineResult.

        xs       [M, 3 n - 1] inside the bounds, NumPy or a device tensor (rows of ``InversionResult.xs``, or
                 ``InversionResult.run_best()``).  ``invert`` forms lo + u (hi - lo), which at u = 1 can round to one
                 ulp above hi: a value within one ulp of the cube is taken and clamped into it.  The models returned
                 lie inside the bounds exactly
        maxiter  iterations; every model of the batch advances in lockstep (0 evaluates the starts only)
        lam0     the damping every model starts with
        tol      the relative width the roots are refined to, as in ``invert``

        DESIGN.md ("Gauss-Newton refinement") has the definitions.  Per iteration: dvh_lm_solve on the kept g and H,
        then at the trial points clamp(u + delta, 0, 1) the scan of ``invert`` (dvh_rayleigh_modes with its c_min, dc
        and need), dvh_rayleigh_sens, dvh_lm_normal and a torch.where selection: the trial is taken iff its f is
        lower (+inf never is), lambda is divided by 10 on acceptance and multiplied by 10 otherwise, within
        1e-12 .. 1e12.  Nothing is read back before the end.

        The residuals use the roots after dvh_rayleigh_sens's Newton step, so ``start_misfits`` may differ from
        ``invert``'s misfit of the same model by the root refinement width over sigma (tol c / sigma per sample).
        ``profile`` records device events around the launches into ``result.timings`` (ms per iteration)."""
        curves, xs = self._checked_problem(curves, xs, maxiter, lam0, tol, "refine()")
        tab = sample_table(curves, default_device())
        fields, timings = self._descend(tab, lambda c, dcdp, chain: lm_normal(c, dcdp, chain, tab), xs, maxiter, lam0,
                                        tol, profile)
        return RefineResult(*fields, timings=timings)

    def _checked_problem(self, curves, xs, maxiter, lam0, tol, who):
        """The argument checks of ``refine`` and ``refine_sets``, before any device work -> (curves, xs tensor)."""
        if not self._configured:
            raise ValueError("configure() the model first")
        n = len(self.layers)
        if n < 1:
            raise ValueError("add() at least one layer")
        D = 3 * n - 1
        if D > LM_MAX_PARAMS:
            raise ValueError(f"at most {LM_MAX_PARAMS} parameters")
        if int(maxiter) < 0 or not (float(lam0) > 0.0 and np.isfinite(lam0)) or \
                not (float(tol) > 0.0 and np.isfinite(tol)):
            raise ValueError("maxiter >= 0, lam0 and tol positive and finite")
        curves = list(curves)
        for c in curves:  # before any device work
            if not isinstance(c, Curve):
                raise TypeError(f"{who} takes Curve objects")
            c.check()
        if not 1 <= len(curves) <= LM_MAX_CURVES:
            raise ValueError(f"1 .. {LM_MAX_CURVES} curves")
        return curves, self._checked_starts(xs)

    def _checked_starts(self, xs):
        """xs [M, 3 n - 1] as a float64 tensor (on whichever device it was given), inside the bounds."""
        D = 3 * len(self.layers) - 1
        if isinstance(xs, torch.Tensor):
            if xs.dim() != 2 or xs.shape[1] != D or xs.dtype != torch.float64:
                raise ValueError(f"xs must be float64 [M, {D}]")
        else:
            xs = np.ascontiguousarray(xs, np.float64)
            if xs.ndim != 2 or xs.shape[1] != D:
                raise ValueError(f"xs must be [M, {D}]")
            xs = torch.from_numpy(xs)
        if not starts_in_bounds(xs, *self.bounds()):
            raise ValueError("xs must lie inside the bounds")
        return xs

    def _evaluator(self, tab, normal, xs, tol, profile):
        """What the loops of ``_descend`` and ``_descend_section`` share: the starts clamped into the cube on the
        table's device, lo, hi, span and the int32 free mask there, ``mark(ev)`` (a device event appended to ev when
        profiling) and ``normal_at(x, ev)``: models and chain of x, dvh_rayleigh_modes with ``invert``'s scan,
        dvh_rayleigh_sens and ``normal(c, dcdp, chain)``, with events between them."""
        dev = tab.periods.device
        n = len(self.layers)
        lo_h, hi_h = self.bounds()
        lo, hi = torch.from_numpy(lo_h).to(dev), torch.from_numpy(hi_h).to(dev)
        x = torch.minimum(torch.maximum(xs.to(dev), lo), hi).contiguous()
        M = x.shape[0]
        span = hi - lo
        free = (span > 0).to(torch.int32)
        c_min = 0.8 * min(l.velocity_s[0] for l in self.layers)
        P = tab.periods.numel()
        c0 = torch.empty((M, P, tab.n_mode), dtype=torch.float64, device=dev)
        count = torch.empty((M, P), dtype=torch.int32, device=dev)
        c1 = torch.empty_like(c0)
        dcdp = torch.empty((M, P, tab.n_mode, n, 4), dtype=torch.float64, device=dev)

        def mark(ev):
            if profile:
                ev.append(torch.cuda.Event(enable_timing=True))
                ev[-1].record()

        def normal_at(x, ev):
            models = self.models_of(x).contiguous()
            chain = self.chain(x, span)
            mark(ev)
            if M:
                _modes_into(models, tab.periods, tab.need, c_min, self.dc, tol, tab.n_mode, c0, count)
            mark(ev)
            if M:
                _lib.call("dvh_rayleigh_sens", _lib.ptr(models), M, n, _lib.ptr(tab.periods), P, _lib.ptr(c0),
                          tab.n_mode, 15, float(tol), _lib.ptr(c1), None, _lib.ptr(dcdp), _lib.stream_of(dev))
            mark(ev)
            out = normal(c1, dcdp, chain)
            mark(ev)
            return out

        return x, lo, hi, span, free, mark, normal_at

    def _descend(self, tab, normal, xs, maxiter, lam0, tol, profile):
        """The loop of ``refine`` and ``refine_sets`` from the checked starts ``xs`` on the table's periods:
        ``normal(c, dcdp, chain)`` is lm_normal on the table or lm_normal_sets on the models' sets.  -> the fields of
        RefineResult as NumPy arrays, in its order, and the timings."""
        dev = tab.periods.device
        x, lo, hi, span, free, mark, normal_at = self._evaluator(tab, normal, xs, tol, profile)
        M, T = x.shape[0], int(maxiter)
        marks = []
        u = torch.where(span > 0, (x - lo) / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(x))
        u = torch.clamp(u, 0.0, 1.0)
        f, g, H, start_status = normal_at(x, [])
        alive = start_status == 0
        lam = torch.full((M,), float(lam0), dtype=torch.float64, device=dev)
        history = torch.empty((T + 1, M), dtype=torch.float64, device=dev)
        accepted = torch.empty((T, M), dtype=torch.bool, device=dev)
        history[0] = f
        solve_status = torch.zeros(M, dtype=torch.int32, device=dev)
        ten = torch.tensor(10.0, dtype=torch.float64, device=dev)  # a tensor: lam / 10.0 would multiply by 0.1
        for it in range(T):
            ev = []
            mark(ev)
            delta, solve_status = lm_solve(H, g, lam, free)
            u_t = torch.clamp(u + delta, 0.0, 1.0)
            x_t = torch.minimum(torch.addcmul(lo, u_t, span), hi)  # lo + (hi - lo) can round to an ulp above hi
            f_t, g_t, H_t, _ = normal_at(x_t, ev)
            take = (f_t < f) & alive
            f = torch.where(take, f_t, f)
            g = torch.where(take[:, None], g_t, g)
            H = torch.where(take[:, None, None], H_t, H)
            u = torch.where(take[:, None], u_t, u)
            x = torch.where(take[:, None], x_t, x)
            lam = torch.where(take, torch.clamp(lam / ten, min=LM_LAMBDA_MIN),
                              torch.clamp(lam * ten, max=LM_LAMBDA_MAX))
            history[it + 1] = f
            accepted[it] = take
            mark(ev)
            marks.append(ev)
        status = (start_status & 1) | (solve_status & 2)
        host = lambda t: t.cpu().numpy()
        fields = (host(x), host(self.models_of(x)), host(f), host(history[0]), host(history), host(accepted),
                  host(lam), host(status), host(g), host(H))
        timings = {}
        if profile:
            torch.cuda.synchronize(dev)
            names = ("solve_ms", "modes_ms", "sens_ms", "normal_ms", "select_ms")
            timings = {name: np.array([e[k].elapsed_time(e[k + 1]) for e in marks]) for k, name in enumerate(names)}
        return fields, timings

    def refine_sets(self, curves, data_sets, xs, model_set=None, uncertainty_sets=None, maxiter=20, lam0=1e-3,
                    tol=1e-9, profile=False):
        """``refine`` with an observation set per model, all in one batch -> EnsembleResult.

        curves, data_sets, uncertainty_sets   the K sets as ``observation_sets`` takes them: ``Curve`` templates (their
                   period, mode, weight and uncertainties; not their data) and per curve a [K, len(period)] array of
                   velocities (km/s), NaN where a set lacks the sample
        xs         [M, 3 n - 1] starts inside the bounds, as ``refine`` takes them
        model_set  int [M], the set each start is refined against; several starts may name one set.  None: M == K
                   and start k refines set k

        The loop is ``refine``'s own with dvh_lm_normal_sets in place of dvh_lm_normal: row m of every result is what
        ``refine`` gives for start m alone against the curves of set ``model_set[m]`` (with every sample present, bit
        for bit).  The periods and the modes scanned are the templates', whatever a set lacks; a set without a present
        sample leaves its starts where they are, with status bit 0."""
        curves, xs = self._checked_problem(curves, xs, maxiter, lam0, tol, "refine_sets()")
        obs, sigma = _checked_sets(curves, data_sets, uncertainty_sets)
        K, M = obs.shape[0], xs.shape[0]
        model_set = _checked_model_set(model_set, M, K)
        dev = default_device()
        sets = _sets_on(curves, obs, sigma, dev)
        at = torch.from_numpy(model_set).to(dev)
        fields, timings = self._descend(sets.table, lambda c, dcdp, chain: lm_normal_sets(c, dcdp, chain, sets, at),
                                        xs, maxiter, lam0, tol, profile)
        return EnsembleResult(*fields, timings=timings, model_set=model_set, n_set=K)


    def _descend_section(self, tab, normal, xs, gap, mu, link, L, maxiter, lam0, tol, profile):
        """The loop of ``refine_section`` beside ``_descend``: the same evaluation of the trial points,
        dvh_lm_solve_chain for the step and acceptance per chain by Phi_c.  gap [M] bool, mu [D] and link [C, L - 1] are device tensors.
        -> the fields of RefineResult in its order, the chain fields as a dict, and the timings."""
        dev = tab.periods.device
        x, lo, hi, span, free, mark, normal_at = self._evaluator(tab, normal, xs, tol, profile)
        M, T, D = x.shape[0], int(maxiter), x.shape[1]
        C = M // L
        marks = []
        mu = torch.where(span > 0, mu, torch.zeros_like(mu))  # the penalty runs over the free parameters
        rows = lambda per_chain: per_chain.repeat_interleave(L)
        zero = torch.zeros((), dtype=torch.float64, device=dev)

        def without_gaps(f, g, H):  # a gap contributes f = 0, g = 0, H = 0 (lm_normal_sets flags it: +inf, status 1)
            return (torch.where(gap, zero, f), torch.where(gap[:, None], zero, g),
                    torch.where(gap[:, None, None], zero, H))

        def objective(f_data, u):
            P, _ = coupling_terms(u.view(C, L, D), mu, link)
            return f_data.view(C, L).sum(dim=1) + P, P

        u = torch.where(span > 0, (x - lo) / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(x))
        u = torch.clamp(u, 0.0, 1.0)
        f, g, H, start_status = normal_at(x, [])
        fd, g, H = without_gaps(f, g, H)
        ok = (start_status == 0) | gap
        alive = ok.view(C, L).all(dim=1) & (~gap).view(C, L).any(dim=1)
        phi, pen = objective(fd, u)
        lam = torch.full((C,), float(lam0), dtype=torch.float64, device=dev)
        history = torch.empty((T + 1, M), dtype=torch.float64, device=dev)
        phi_history = torch.empty((T + 1, C), dtype=torch.float64, device=dev)
        accepted = torch.empty((T, C), dtype=torch.bool, device=dev)
        history[0], phi_history[0] = f, phi
        solve_status = torch.zeros(C, dtype=torch.int32, device=dev)
        ten = torch.tensor(10.0, dtype=torch.float64, device=dev)
        for it in range(T):
            ev = []
            mark(ev)
            delta, solve_status = lm_solve_chain(H, g, u, lam, free, mu, link, L)
            u_t = torch.clamp(u + delta, 0.0, 1.0)
            x_t = torch.minimum(torch.addcmul(lo, u_t, span), hi)
            f_t, g_t, H_t, _ = normal_at(x_t, ev)
            fd_t, g_t, H_t = without_gaps(f_t, g_t, H_t)
            phi_t, pen_t = objective(fd_t, u_t)
            take_c = (phi_t < phi) & alive  # +inf at a non-gap position never is lower
            take = rows(take_c)
            f = torch.where(take, f_t, f)
            fd = torch.where(take, fd_t, fd)
            g = torch.where(take[:, None], g_t, g)
            H = torch.where(take[:, None, None], H_t, H)
            u = torch.where(take[:, None], u_t, u)
            x = torch.where(take[:, None], x_t, x)
            phi = torch.where(take_c, phi_t, phi)
            pen = torch.where(take_c, pen_t, pen)
            lam = torch.where(take_c, torch.clamp(lam / ten, min=LM_LAMBDA_MIN),
                              torch.clamp(lam * ten, max=LM_LAMBDA_MAX))
            history[it + 1], phi_history[it + 1] = f, phi
            accepted[it] = take_c
            mark(ev)
            marks.append(ev)
        carried = gap & rows(alive)  # a gap row of a live chain: no misfit of its own
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        history = torch.where(carried, nan, history)
        chain_status = ((~alive).to(torch.int32)) | (solve_status & 2)
        status = torch.where(carried, torch.full_like(start_status, 4), start_status & 1) | rows(solve_status & 2)
        host = lambda t: t.cpu().numpy()
        fields = (host(x), host(self.models_of(x)), host(history[T]), host(history[0]), host(history),
                  host(accepted.repeat_interleave(L, dim=1)), host(rows(lam)), host(status), host(g), host(H))
        more = dict(objective=host(phi), penalty=host(pen), objective_history=host(phi_history),
                    chain_status=host(chain_status))
        timings = {}
        if profile:
            torch.cuda.synchronize(dev)
            names = ("solve_ms", "modes_ms", "sens_ms", "normal_ms", "select_ms")
            timings = {name: np.array([e[k].elapsed_time(e[k + 1]) for e in marks]) for k, name in enumerate(names)}
        return fields, more, timings

    def refine_section(self, curves, data_sets, xs, chain_len=None, coupling=1.0, link_weights=None, model_set=None,
                       uncertainty_sets=None, maxiter=20, lam0=1e-3, tol=1e-9, profile=False):
        """``refine_sets`` with neighbouring rows tied together: a laterally constrained refinement of chains of models
        into a section -> SectionResult.

        curves, data_sets, xs, model_set, uncertainty_sets, maxiter, lam0, tol, profile   as ``refine_sets`` takes them
        chain_len     L: rows c L + k, k = 0 .. L - 1, of ``xs`` are the positions of chain c, in order along the fibre
                      (or in time).  None: one chain of all rows
        coupling      mu >= 0, a scalar or [3 n - 1] in the unit cube of the bounds: the weight of the squared first
                      difference of each parameter between neighbours.  0 leaves a parameter free of its neighbours
        link_weights  w >= 0, [L - 1] (every chain's) or [C, L - 1], default 1: the weight of each link.  0 cuts the
                      chain there; 1 / spacing^2 serves unevenly spaced positions

        Per chain the objective is Phi_c = sum_k f_k + 1/2 sum_k w_k sum_d mu_d (u_{k+1,d} - u_{k,d})^2 over the rows
        with data and the free parameters ("Laterally constrained refinement").  A row whose set has no
        present sample is a gap: it adds nothing to Phi_c and is carried by its neighbours through the penalty.  The
        step of a whole chain is one block-tridiagonal solve (dvh_lm_solve_chain) with one damping per chain; the trial
        of the whole chain is taken iff its Phi_c is lower, and lambda_c follows ``refine``'s rule.  A chain with a
        non-gap row whose start has f = +inf, or without any data, is returned as given (status bit 0).  With
        ``chain_len=1`` every row is ``refine_sets``' bit for bit.  Nothing is read back before the end.

        ValueError, before any device work: what ``refine_sets`` raises; M not a multiple of ``chain_len``; a coupling
        or link weight that is negative or not finite; a coupling that is neither a scalar nor [3 n - 1]; link weights
        that are neither [L - 1] nor [C, L - 1]."""
        curves, xs = self._checked_problem(curves, xs, maxiter, lam0, tol, "refine_section()")
        obs, sigma = _checked_sets(curves, data_sets, uncertainty_sets)
        K, M = obs.shape[0], xs.shape[0]
        model_set = _checked_model_set(model_set, M, K)
        C, L, mu, w = _checked_chains(M, xs.shape[1], chain_len, coupling, link_weights)
        gap = ~np.isfinite(obs[model_set]).any(axis=1)
        dev = default_device()
        sets = _sets_on(curves, obs, sigma, dev)
        at = torch.from_numpy(model_set).to(dev)
        fields, more, timings = self._descend_section(
            sets.table, lambda c, dcdp, chain: lm_normal_sets(c, dcdp, chain, sets, at), xs,
            torch.from_numpy(gap).to(dev), torch.from_numpy(mu).to(dev), torch.from_numpy(w).to(dev), L, maxiter, lam0,
            tol, profile)
        return SectionResult(*fields, timings=timings, model_set=model_set, n_set=K, n_chain=C, chain_len=L,
                             coupling=mu, link_weights=w, gap=gap, **more)


# ------------------------------------------------------------------------------------------------- sensitivities

PARAMETERS = ("thickness", "velocity_p", "velocity_s", "density")  # the columns of a layer row, by disba's names


def _parameter_columns(parameters):
    names = (parameters,) if isinstance(parameters, str) else tuple(parameters)
    for name in names:
        if name not in PARAMETERS:
            raise ValueError(f"parameter {name!r}: one of {PARAMETERS}")
    if not names or len(set(names)) != len(names):
        raise ValueError("parameters must be distinct names, at least one")
    return [PARAMETERS.index(name) for name in names]


def _sens(models, periods, n_mode, cols, want_u, dc, c_min, tol, need):
    """dvh_rayleigh_modes, then dvh_rayleigh_sens on its roots -> (polished c, U or None, dc/dp [..., 4] or None)."""
    c = rayleigh_modes(models, periods, n_mode, dc=dc, c_min=c_min, tol=tol, need=need)
    dev = models.device
    models = models.contiguous()
    periods = torch.as_tensor(periods, dtype=torch.float64, device=dev).reshape(-1).contiguous()
    M, n_layer, _ = models.shape
    out_c = torch.empty_like(c)
    out_u = torch.empty_like(c) if want_u else None
    out_p = torch.empty(c.shape + (n_layer, 4), dtype=torch.float64, device=dev) if cols else None
    if c.numel():
        _lib.call("dvh_rayleigh_sens", _lib.ptr(models), M, n_layer, _lib.ptr(periods), periods.numel(), _lib.ptr(c),
                  int(n_mode), sum(1 << q for q in cols), float(tol), _lib.ptr(out_c), _lib.ptr(out_u),
                  _lib.ptr(out_p), _lib.stream_of(dev))
    return out_c, out_u, out_p


def rayleigh_sensitivity(models, periods, n_mode, parameters=PARAMETERS, dc=0.005, c_min=None, tol=1e-9, need=None,
                         return_modes=False):
    """The derivative dc/dp of every modal phase velocity with respect to the layer values, on the device.

    models, periods, n_mode, dc, c_min, tol, need   as rayleigh_modes takes them
    parameters  names out of ("thickness", "velocity_p", "velocity_s", "density"), the order of the last axis
    ->          [M, P, n_mode, n_layer, len(parameters)] in km/s per unit of the parameter (km, km/s, g/cm^3), NaN where
                rayleigh_modes has no root; 0 for a row of zero thickness and for the half-space's thickness (and, with
                ``return_modes``, the roots [M, P, n_mode] after the kernel's Newton step)

    This is the derivative itself, -D_p / D_c of the secular function at the root (dvh_rayleigh_sens), this build's own
    definition of a sensitivity kernel: it is not scaled by the layer's thickness or value.
    """
    cols = _parameter_columns(parameters)
    c, _, dcdp = _sens(models, periods, n_mode, cols, False, dc, c_min, tol, need)
    dcdp = dcdp[..., cols].contiguous()
    return (dcdp, c) if return_modes else dcdp


def rayleigh_group(models, periods, n_mode, dc=0.005, c_min=None, tol=1e-9, need=None, return_modes=False):
    """Modal Rayleigh group velocities U = c / (1 - (omega / c) dc/domega) (km/s) on the device: [M, P, n_mode], NaN
    where rayleigh_modes has no root (and, with ``return_modes``, the roots after the kernel's Newton step)."""
    c, u, _ = _sens(models, periods, n_mode, [], True, dc, c_min, tol, need)
    return (u, c) if return_modes else u


def _layer_rows(thickness, velocity_p, velocity_s, density):
    rows = [np.asarray(a, np.float64).reshape(-1) for a in (thickness, velocity_p, velocity_s, density)]
    if len({r.size for r in rows}) != 1 or not 1 <= rows[0].size <= MAX_LAYERS:
        raise ValueError(f"thickness, velocity_p, velocity_s and density need one length, 1 .. {MAX_LAYERS}")
    return np.ascontiguousarray(np.stack(rows, 1))


def group_velocity(period, thickness, velocity_p, velocity_s, density, mode=0, dc=0.005):
    """The notebooks' ``surf96(period, thickness, velocity_p, velocity_s, density, mode, 1, rayleigh, dc)`` call
    (itype = 1) of plot_predicted_curve: NumPy in, the group velocity (km/s) of Rayleigh mode ``mode`` at every period
    out, NaN where the mode does not exist."""
    if not 0 <= int(mode) < MAX_MODES:
        raise ValueError(f"mode must be 0 .. {MAX_MODES - 1}")
    layers = _layer_rows(thickness, velocity_p, velocity_s, density)
    period = np.ascontiguousarray(np.asarray(period, np.float64).reshape(-1))  # the notebooks pass reversed views
    dev = default_device()
    u = rayleigh_group(torch.from_numpy(layers[None]).to(dev), torch.from_numpy(period).to(dev), int(mode) + 1, dc=dc)
    return u[0, :, int(mode)].cpu().numpy()


SensitivityKernel = namedtuple("SensitivityKernel", "depth kernel period velocity mode wave type parameter")


class PhaseSensitivity:
    """disba's ``PhaseSensitivity(thickness, velocity_p, velocity_s, density)`` as inversion_diff_weight.ipynb uses
    it: ``ps(t, mode=0, wave="rayleigh", parameter="velocity_s")`` -> SensitivityKernel.

    depth     the top of every layer (km)
    kernel    [n_layer] dc/dp of that layer's parameter (rayleigh_sensitivity's definition, the derivative itself; the
              half-space's thickness gives 0), NaN if the mode does not exist at ``t``; a NumPy array of its own, so
              ``s.kernel[-1:] = 0.0`` works
    velocity  the phase velocity the kernel was taken at
    """

    def __init__(self, thickness, velocity_p, velocity_s, density, dc=0.005):
        self.layers = _layer_rows(thickness, velocity_p, velocity_s, density)
        self.dc = float(dc)

    def __call__(self, t, mode=0, wave="rayleigh", parameter="velocity_s"):
        if wave != "rayleigh":
            raise ValueError(f"wave {wave!r}: only 'rayleigh' is built")
        if not isinstance(parameter, str):
            raise ValueError("parameter must be one name")
        _parameter_columns(parameter)
        if not 0 <= int(mode) < MAX_MODES:
            raise ValueError(f"mode must be 0 .. {MAX_MODES - 1}")
        dev = default_device()
        k, c = rayleigh_sensitivity(torch.from_numpy(self.layers[None]).to(dev),
                                    torch.tensor([float(t)], dtype=torch.float64, device=dev), int(mode) + 1,
                                    parameters=(parameter,), dc=self.dc, return_modes=True)
        depth = np.concatenate([[0.0], np.cumsum(self.layers[:-1, 0])])
        return SensitivityKernel(depth, k[0, 0, int(mode), :, 0].cpu().numpy(), float(t), float(c[0, 0, int(mode)]),
                                 int(mode), wave, "phase", parameter)
