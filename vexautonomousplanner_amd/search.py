"""Cross-entropy route search over batches of candidate trajectories (vap_search_sample, vap_search_update, include/vap.h).

``profile``, ``time_profile``, ``footprint.clearance``, ``footprint.conflicts`` and ``tracking.rollouts`` judge candidate
routes thousands at a time.  This module makes the candidates and acts on the verdicts: give ``refine`` a route, a field
scene and (optionally) a partner's routine and a follower, and it returns a faster route that still clears everything.

The search refines R routes ("problems") at a time with N candidates each.  Per iteration: the candidates' waypoints are
drawn around a mean (candidate 0 is the best route so far), profiled, time-profiled and checked by the existing calls, then
scored, ranked and the mean and sigma refitted to the E best.  Every step is enqueued on torch's current stream; nothing is
read on the host inside the loop, so the returned tensors are not synchronised either.

The cost of a candidate (seconds): w_time * duration + w_length * length, plus infeasible_base + w_violation * violation
when the candidate violates a margin, +inf when it is flagged, has no rows or a NaN term — any feasible candidate beats
any infeasible one, and among infeasible ones the smaller violation wins, which is how the search leaves a seed that
collides.  Units: feet, seconds.

Plain-node paths only: routes with reverse or turn nodes are not searched here.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from ._call import buffers, context_for, device_array, ptr
from .synth import DEFAULT_CONSTRAINTS

MAX_CANDIDATES = 4096


@dataclass
class Weights:
    """vap_search_weights: seconds per second of duration, seconds per foot of length, seconds per foot of violation, the
    step every infeasible candidate pays, and the margins (ft) below / the tracking error (ft) above which a candidate
    violates."""
    w_time: float = 1.0
    w_length: float = 1e-3
    w_violation: float = 1e3
    infeasible_base: float = 1e6
    clearance_margin: float = 0.05
    conflict_margin: float = 0.05
    tracking_tolerance: float = 0.25

    def validate(self):
        for name in ("w_time", "w_length", "w_violation", "infeasible_base"):
            v = float(getattr(self, name))
            if not (v >= 0 and np.isfinite(v)):
                raise ValueError(f"Weights.{name} must be >= 0 and finite (got {v!r})")
        for name in ("clearance_margin", "conflict_margin", "tracking_tolerance"):
            if not np.isfinite(float(getattr(self, name))):
                raise ValueError(f"Weights.{name} must be finite (got {getattr(self, name)!r})")
        return self

    def as_struct(self):
        return _lib.SearchWeights(float(self.w_time), float(self.w_length), float(self.w_violation), float(self.infeasible_base),
                                  float(self.clearance_margin), float(self.conflict_margin), float(self.tracking_tolerance))


@dataclass
class SearchConfig:
    """candidates N per problem and iteration (1..4096), elites E the refit uses (1..N), iterations, the smoothing alpha of
    the refit (1 = the elites' statistics alone), the clamp of a free coordinate's sigma (ft), the seed of the Philox
    stream, the cost's weights."""
    candidates: int = 256
    elites: int = 32
    iterations: int = 12
    alpha: float = 0.7
    sigma_min: float = 1e-3
    sigma_max: float = 2.0
    seed: int = 0
    weights: Weights = field(default_factory=Weights)

    def validate(self):
        if int(self.candidates) != self.candidates or not 1 <= int(self.candidates) <= MAX_CANDIDATES:
            raise ValueError(f"SearchConfig.candidates must be 1..{MAX_CANDIDATES} (got {self.candidates!r})")
        if int(self.elites) != self.elites or not 1 <= int(self.elites) <= int(self.candidates):
            raise ValueError(f"SearchConfig.elites must be 1..candidates (got {self.elites!r})")
        if int(self.iterations) != self.iterations or int(self.iterations) < 1:
            raise ValueError(f"SearchConfig.iterations must be >= 1 (got {self.iterations!r})")
        if not 0.0 <= float(self.alpha) <= 1.0:
            raise ValueError(f"SearchConfig.alpha must be in [0, 1] (got {self.alpha!r})")
        if not 0.0 <= float(self.sigma_min) <= float(self.sigma_max) or not np.isfinite(float(self.sigma_max)):
            raise ValueError(f"SearchConfig needs 0 <= sigma_min <= sigma_max < inf (got {self.sigma_min!r}, {self.sigma_max!r})")
        if not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError(f"SearchConfig.seed must fit 64 bits (got {self.seed!r})")
        if not isinstance(self.weights, Weights):
            raise TypeError("SearchConfig.weights must be a search.Weights")
        self.weights.validate()
        return self


def _vdtype(t):
    if t.dtype == torch.float32:
        return _lib.VAP_F32
    if t.dtype == torch.float64:
        return _lib.VAP_F64
    raise ValueError(f"waypoints must be float32 or float64 (got {t.dtype})")


def _dev64(t, dev, what, shape=None):
    """``t`` as a contiguous fp64 tensor on ``dev`` (None stays None)."""
    t = device_array(t, dev, torch.float64)
    if t is not None and shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


def sample(mean, sigma, candidates, dtype=torch.float32, seed=0, iteration=0, first_problem=0, best_waypoints=None,
           best_cost=None, out=None, ctx=None):
    """Candidate waypoints on the device (vap_search_sample): (R * candidates, W, 2) of ``dtype``, candidate (r, n) at row
    r * candidates + n, from ``mean`` and ``sigma`` (R, W, 2) fp64 device tensors.  Candidate 0 of a problem is
    ``best_waypoints[r]`` where ``best_cost[r]`` is finite, else the mean; a sigma of 0 pins a coordinate.  A candidate
    depends on (seed, iteration, first_problem + r, n, w) only.  ``out``: a tensor of the result's shape to fill."""
    if not isinstance(mean, torch.Tensor) or mean.device.type != "cuda" or mean.dtype != torch.float64 or mean.dim() != 3 or mean.shape[2] != 2:
        raise ValueError("mean must be an (R, W, 2) fp64 tensor on a HIP device")
    dev = mean.device
    R, W = int(mean.shape[0]), int(mean.shape[1])
    N = int(candidates)
    sigma = _dev64(sigma, dev, "sigma", (R, W, 2))
    mean = mean.contiguous()
    if out is None:
        out = torch.empty((R * N, W, 2), dtype=dtype, device=dev)
    elif tuple(out.shape) != (R * N, W, 2) or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous ({R * N}, {W}, 2) tensor on {dev}")
    vd = _vdtype(out)
    if best_waypoints is not None and (tuple(best_waypoints.shape) != (R, W, 2) or best_waypoints.dtype != out.dtype or
                                       not best_waypoints.is_contiguous()):
        raise ValueError(f"best_waypoints must be a contiguous ({R}, {W}, 2) {out.dtype} tensor")
    if best_cost is not None and (tuple(best_cost.shape) != (R,) or best_cost.dtype != torch.float64):
        raise ValueError(f"best_cost must be an ({R},) fp64 tensor")
    ctx = context_for(dev, ctx)
    _lib.check(ctx._L.vap_search_sample(ctx.handle, vd, R, N, W, ptr(mean), ptr(sigma), ptr(best_waypoints), ptr(best_cost),
                                        int(seed), int(iteration) & 0xFFFFFFFF, int(first_problem) & 0xFFFFFFFF, ptr(out)),
               "vap_search_sample")
    return out


_TERMS = ("counts", "meta", "flags", "clearance", "conflict_clearance", "tracking_worst")


def update(waypoints, problems, weights=None, counts=None, time_step=0.01, meta=None, flags=None, clearance=None,
           conflict_clearance=None, tracking_worst=None, mean=None, sigma=None, elites=1, alpha=1.0, sigma_min=0.0,
           sigma_max=float("inf"), best_cost=None, best_waypoints=None, best_terms=None, history=None, iteration=0,
           n_feasible=None, out=None, ctx=None):
    """Score, rank, refit, remember (vap_search_update) for ``problems`` = R problems whose N = B / R candidates are the
    rows of ``waypoints`` (B, W, 2).  The terms are per-candidate device tensors, any may be None: ``counts`` (B, k) or
    (B,) int32 with ``time_step``, ``meta`` (B, 4), ``flags`` (B,) int32, and (B,) fp64 ``clearance``,
    ``conflict_clearance``, ``tracking_worst``.  ``mean`` / ``sigma`` (R, W, 2) fp64 are refitted in place; ``best_cost``
    (R,), ``best_waypoints`` (R, W, 2), ``best_terms`` (R, 4) and column ``iteration`` of ``history`` (R, k) are updated in
    place; ``n_feasible``: an (R,) int32 tensor to fill.  Returns a dict: cost, violation (B,), order (R, N), n_feasible
    (R,); ``out`` keeps these buffers between calls."""
    wp = waypoints
    if not isinstance(wp, torch.Tensor) or wp.device.type != "cuda" or wp.dim() != 3 or wp.shape[2] != 2 or not wp.is_contiguous():
        raise ValueError("waypoints must be a contiguous (B, W, 2) tensor on a HIP device")
    dev = wp.device
    vd = _vdtype(wp)
    B, W = int(wp.shape[0]), int(wp.shape[1])
    R = int(problems)
    if R < 1 or B % R:
        raise ValueError(f"{B} candidates do not divide into {problems!r} problems")
    N = B // R
    weights = (weights if weights is not None else Weights()).validate()
    stride = 1
    if counts is not None:
        if counts.dtype != torch.int32 or counts.shape[0] != B or counts.dim() > 2 or not counts.is_contiguous():
            raise ValueError(f"counts must be a contiguous ({B}, k) or ({B},) int32 tensor")
        stride = int(counts.shape[1]) if counts.dim() == 2 else 1
    if flags is not None and (flags.dtype != torch.int32 or tuple(flags.shape) != (B,)):
        raise ValueError(f"flags must be a ({B},) int32 tensor")
    if meta is not None and (meta.dtype != torch.float64 or tuple(meta.shape) != (B, 4) or not meta.is_contiguous()):
        raise ValueError(f"meta must be a contiguous ({B}, 4) fp64 tensor")
    for name, t in (("clearance", clearance), ("conflict_clearance", conflict_clearance), ("tracking_worst", tracking_worst)):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (B,) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous ({B},) fp64 tensor")
    for name, t, shp, dt in (("mean", mean, (R, W, 2), torch.float64), ("sigma", sigma, (R, W, 2), torch.float64),
                             ("best_cost", best_cost, (R,), torch.float64), ("best_waypoints", best_waypoints, (R, W, 2), wp.dtype),
                             ("best_terms", best_terms, (R, 4), torch.float64), ("n_feasible", n_feasible, (R,), torch.int32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous {shp} {dt} tensor on {dev}")
    hist_stride = 0
    if history is not None:
        if history.dtype != torch.float64 or history.dim() != 2 or history.shape[0] != R or not history.is_contiguous():
            raise ValueError(f"history must be a contiguous ({R}, k) fp64 tensor")
        hist_stride = int(history.shape[1])
    shapes = {"cost": ((B,), torch.float64), "violation": ((B,), torch.float64), "order": ((R, N), torch.int32)}
    if n_feasible is None:
        shapes["n_feasible"] = ((R,), torch.int32)
    bufs = buffers(out, shapes, dev)
    res = {k: bufs[k] for k in shapes}
    if n_feasible is not None:
        res["n_feasible"] = n_feasible
    ws = weights.as_struct()
    ctx = context_for(dev, ctx)
    _lib.check(ctx._L.vap_search_update(
        ctx.handle, vd, R, N, W, ptr(wp), ptr(counts), stride, float(time_step), ptr(meta), ptr(flags), ptr(clearance),
        ptr(conflict_clearance), ptr(tracking_worst), C.byref(ws), int(elites), float(alpha), float(sigma_min),
        float(sigma_max), ptr(mean), ptr(sigma), ptr(res["cost"]), ptr(res["violation"]), ptr(res["order"]),
        ptr(res["n_feasible"]), ptr(best_cost), ptr(best_waypoints), ptr(best_terms), ptr(history), hist_stride,
        int(iteration) & 0xFFFFFFFF), "vap_search_update")
    return res


def rank(waypoints, problems=1, weights=None, out=None, ctx=None, **terms):
    """Rank this batch: the score-and-rank-only form of vap_search_update (no mean, no best-so-far).  ``waypoints`` (B, W, 2)
    gives the batch its shape and type; ``terms``: counts (+ time_step), meta, flags, clearance, conflict_clearance,
    tracking_worst as in ``update``.  Returns cost, violation (B,), order (problems, B / problems) and n_feasible."""
    for k in terms:
        if k not in _TERMS + ("time_step",):
            raise TypeError(f"rank() got an unexpected term {k!r}")
    return update(waypoints, problems, weights=weights, out=out, ctx=ctx, **terms)


def _sigma0(sigma0, R, W, pinned, pin_ends):
    s = np.asarray(sigma0, dtype=np.float64)
    if s.ndim == 0:
        s = np.full((R, W, 2), float(s))
    elif s.shape == (W, 2):
        s = np.broadcast_to(s, (R, W, 2)).copy()
    elif s.shape == (R, W, 2):
        s = s.copy()
    else:
        raise ValueError(f"sigma0 must be a scalar, ({W}, 2) or ({R}, {W}, 2), got {s.shape}")
    if not (np.isfinite(s).all() and (s >= 0).all()):
        raise ValueError("sigma0 must be finite and >= 0")
    if pin_ends:
        s[:, 0] = 0.0
        s[:, -1] = 0.0
    if pinned is not None:
        m = np.asarray(pinned).astype(bool)
        if m.shape == (W,):
            m = np.broadcast_to(m, (R, W))
        if m.shape != (R, W):
            raise ValueError(f"pinned must be ({W},) or ({R}, {W}), got {m.shape}")
        s[m] = 0.0
    return s


def refine(gen, seeds, sigma0, footprint, scene, constraints=DEFAULT_CONSTRAINTS, samples=None, dd=None, dt=0.01,
           capacity_rows=None, others=None, others_footprint=None, follower=None, perturbations=None, config=None,
           pinned=None, pin_ends=True, capacity=None, first_problem=0, curve_caps=None, robust_clearance=False,
           robust_conflicts=False, others_shift_rows=0, others_start_jitter=None):
    """Refine R routes by cross-entropy search on ``gen``'s device (a BatchedTrajectoryGenerator; its dtype is the
    waypoints').

      seeds          (R, W, 2) or (W, 2) waypoints in feet: the first mean, and candidate 0 of the first iteration
                     (``plan.seeds(...)["waypoints"]`` gives seeds that already go round the scene's obstacles)
      sigma0         the first sigma in feet: a scalar, (W, 2) or (R, W, 2); the first and last waypoint are pinned unless
                     ``pin_ends=False``; ``pinned`` (W,) or (R, W) bool pins more
      footprint, scene   the robot's polygon and the footprint.Scene of ``footprint.clearance``; the margin is
                     config.weights.clearance_margin
      constraints, samples= | dd=, capacity, dt, capacity_rows   as in ``profile`` and ``time_profile``
      others         the dict ``time_profile`` / ``insert_waits`` returned for the partner's routines (same dt): every
                     candidate is checked against all of them (``footprint.conflicts``; ``others_footprint`` default the
                     same robot); the margin is config.weights.conflict_margin
      follower, perturbations   a tracking.Follower or tracking.Pursuit and (K, 8) or (R * N, K, 8) records: the worst
                     tracking error of every candidate's rollouts enters the cost above config.weights.tracking_tolerance;
                     with a Pursuit a candidate with a rollout that never arrives (n_unfinished > 0) has the term +inf
      robust_clearance   needs ``follower``: every iteration runs ``tracking.rollout_clearance`` where it ran
                     ``tracking.rollouts``, and a candidate's clearance term is the smaller of its planned rows' clearance
                     and the worst clearance of its disturbed rollouts (the planned one alone where no rollout has rows),
                     so a route that clears the scene only when driven perfectly is no longer feasible.  The tracking term
                     is unchanged.  False: the sequence without it
      others_shift_rows   the partner starts that many rows late (any sign): passed to ``footprint.conflicts`` and to the
                     rollouts of ``robust_conflicts`` alike
      robust_conflicts   needs ``follower`` and ``others``: every iteration runs ``tracking.rollout_conflicts`` (where it ran
                     ``tracking.rollouts``; beside ``tracking.rollout_clearance`` with ``robust_clearance`` too, so the
                     rollouts then run twice), and a candidate's conflict term is the smaller of its planned rows' conflict
                     clearance and the worst of its disturbed rollouts (the planned one alone where no rollout has a valid
                     pair), so a route that passes the partner only when driven perfectly is no longer feasible
      others_start_jitter   with ``robust_conflicts``: (K,) int rows, rollout k meets a partner that starts
                     others_shift_rows + jitter[k] rows late (``rollout_shift``)
      config         a SearchConfig
      curve_caps     a drive.CurveCaps: every iteration's velocity rows are recomputed under these caps
                     (``gen.apply_curve_caps``) between ``profile`` and ``time_profile``; None: the sequence without it
      first_problem  the number of problem 0 in the random stream: R = 1 with first_problem = r draws what problem r of a
                     larger call draws
    Per iteration it enqueues sample, profile, time_profile, footprint clearance, conflicts (with ``others``), rollouts
    (with ``follower``) and update, reusing every buffer; nothing is synchronised or read on the host.  Returns a dict of
    device tensors: best_waypoints (R, W, 2), best_cost (R,) (+inf: no candidate ever had a finite cost), best_terms (R, 4)
    = duration, length, violation, candidate index of the best, feasible (R,) bool, history (R, iterations) (the best cost
    after each iteration, non-increasing), n_feasible (R, iterations), mean, sigma (R, W, 2), and the last iteration's cost
    (R, N) and order (R, N); with a tracking.Pursuit also the last iteration's n_unfinished (R, N).

    Plain-node paths only: routes with reverse or turn nodes are out of this search's scope."""
    from . import footprint as fp
    from . import tracking
    cfg = (config if config is not None else SearchConfig()).validate()
    if (samples is None) == (dd is None):
        raise ValueError("give exactly one of samples= or dd=")
    if follower is not None and perturbations is None:
        raise ValueError("follower needs perturbations (tracking.sample_perturbations)")
    if robust_clearance and follower is None:
        raise ValueError("robust_clearance needs a follower (and perturbations): it scores the rollouts' clearance")
    if robust_conflicts and follower is None:
        raise ValueError("robust_conflicts needs a follower (and perturbations): it scores the rollouts' clearance to the partner")
    if robust_conflicts and others is None:
        raise ValueError("robust_conflicts needs others: the partner's routines the rollouts are checked against")
    if others_start_jitter is not None and not robust_conflicts:
        raise ValueError("others_start_jitter is the rollouts' start jitter: it needs robust_conflicts=True")
    if int(others_shift_rows) != others_shift_rows:
        raise ValueError(f"others_shift_rows must be an int (got {others_shift_rows!r})")
    others_shift_rows = int(others_shift_rows)
    dev = gen.device
    s = np.asarray(seeds.detach().cpu().numpy() if isinstance(seeds, torch.Tensor) else seeds, dtype=np.float64)
    if s.ndim == 2:
        s = s[None]
    if s.ndim != 3 or s.shape[2] != 2 or s.shape[1] < 2 or not np.isfinite(s).all():
        raise ValueError(f"seeds must be finite (R, W, 2) or (W, 2) waypoints, got {s.shape}")
    R, W = int(s.shape[0]), int(s.shape[1])
    N, iters, wts = int(cfg.candidates), int(cfg.iterations), cfg.weights
    B = R * N
    mean = torch.as_tensor(np.ascontiguousarray(s), device=dev)
    sigma = torch.as_tensor(_sigma0(sigma0, R, W, pinned, pin_ends), device=dev)
    wp = torch.empty((B, W, 2), dtype=gen.tdtype, device=dev)
    best_wp = torch.zeros((R, W, 2), dtype=gen.tdtype, device=dev)
    best_cost = torch.full((R,), float("inf"), dtype=torch.float64, device=dev)
    best_terms = torch.full((R, 4), float("nan"), dtype=torch.float64, device=dev)
    history = torch.full((R, iters), float("inf"), dtype=torch.float64, device=dev)
    n_feas = torch.zeros((iters, R), dtype=torch.int32, device=dev)
    if perturbations is not None and not isinstance(perturbations, torch.Tensor):
        perturbations = torch.as_tensor(np.ascontiguousarray(perturbations, dtype=np.float64), device=dev)
    prof, tp, clr, conf, trk, upd, rcf = None, {}, {}, {}, {}, {}, {}
    pursuit = isinstance(follower, tracking.Pursuit)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    kw = {"samples": samples} if samples is not None else {"dd": dd, "capacity": capacity}
    for it in range(iters):
        sample(mean, sigma, N, seed=cfg.seed, iteration=it, first_problem=first_problem, best_waypoints=best_wp,
               best_cost=best_cost, out=wp, ctx=gen.ctx)
        prof = gen.profile(wp, constraints, out=prof, **kw)
        if curve_caps is not None:
            gen.apply_curve_caps(prof, curve_caps, constraints)
        gen.time_profile(prof, constraints, dt=dt, capacity_rows=capacity_rows, out=tp)
        fp.clearance(tp["rows"], tp["counts"], footprint, scene, margin=wts.clearance_margin, out=clr, ctx=gen.ctx)
        terms = {"clearance": clr["min_clearance"]}
        if others is not None:
            fp.conflicts(tp["rows"], tp["counts"], footprint, others["rows"], others["counts"], others_footprint,
                         margin=wts.conflict_margin, shift_rows=others_shift_rows, out=conf, ctx=gen.ctx)
            terms["conflict_clearance"] = conf["min_clearance"]
        if robust_conflicts:
            tracking.rollout_conflicts(tp["rows"], tp["counts"], follower, perturbations, footprint, others["rows"], others["counts"],
                                       others_footprint, margin=wts.conflict_margin, shift_rows=others_shift_rows,
                                       rollout_shift=others_start_jitter, time_step=dt, out=rcf, ctx=gen.ctx)
            wc = rcf["worst_conflict"]
            terms["conflict_clearance"] = torch.where(torch.isnan(wc), conf["min_clearance"], torch.minimum(conf["min_clearance"], wc))
            if not robust_clearance:
                trk = rcf                                  # the follower's own outputs are those of its plain call
        if robust_clearance:
            tracking.rollout_clearance(tp["rows"], tp["counts"], follower, perturbations, footprint, scene,
                                       margin=wts.clearance_margin, time_step=dt, out=trk, ctx=gen.ctx)
            wc = trk["worst_clearance"]
            terms["clearance"] = torch.where(torch.isnan(wc), clr["min_clearance"], torch.minimum(clr["min_clearance"], wc))
        elif follower is not None and not robust_conflicts:
            tracking.rollouts(tp["rows"], tp["counts"], follower, perturbations, time_step=dt, out=trk, ctx=gen.ctx)
        if follower is not None:
            # a pure-pursuit candidate whose rollouts do not all arrive is never an elite: its tracking term is +inf
            terms["tracking_worst"] = torch.where(trk["n_unfinished"] > 0, inf, trk["worst"]) if pursuit else trk["worst"]
        update(wp, R, weights=wts, counts=tp["counts"], time_step=dt, meta=prof["meta"], flags=prof["flags"], mean=mean,
               sigma=sigma, elites=cfg.elites, alpha=cfg.alpha, sigma_min=cfg.sigma_min, sigma_max=cfg.sigma_max,
               best_cost=best_cost, best_waypoints=best_wp, best_terms=best_terms, history=history, iteration=it,
               n_feasible=n_feas[it], out=upd, ctx=gen.ctx, **terms)
    out = {"best_waypoints": best_wp, "best_cost": best_cost, "best_terms": best_terms,
           "feasible": torch.isfinite(best_cost) & (best_terms[:, 2] == 0), "history": history, "n_feasible": n_feas.t(),
           "mean": mean, "sigma": sigma, "cost": upd["cost"].view(R, N), "order": upd["order"]}
    if pursuit:
        out["n_unfinished"] = trk["n_unfinished"].view(R, N)
    if robust_clearance:
        out["n_colliding"] = trk["n_colliding"].view(R, N)
    if robust_conflicts:
        out["n_conflicting"] = rcf["n_conflicting"].view(R, N)
    return out
