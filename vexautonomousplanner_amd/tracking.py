"""Closed-loop tracking rollouts of time-domain rows (vap_tracking_rollouts, include/vap.h).

The clearance checks of ``footprint`` judge the nominal rows ``time_profile`` / ``insert_waits`` write.  The robot does
not drive those rows: it feeds them to a path follower.  This module rolls a differential-drive robot with a RAMSETE
follower along every route of a batch, K times per route under K perturbation records (a start offset, a gain per wheel,
a track-width factor, a drive lag), on the device, and returns how far it strays — the margin the clearance calls need —
and, with ``executed=True``, the executed rows in the time-profile layout, which ``footprint.clearance`` and
``footprint.conflicts`` accept unchanged.

The model, step by step, is the header's: reference pose (x, y) = columns 6, 7, phi = -heading, v = column 2,
omega = -angular velocity; errors in the body frame; RAMSETE; wheel-speed saturation that keeps the curvature; a
first-order wheel lag and the exact arc per substep.  Units: feet, seconds, radians.

A second follower, pure pursuit (``Pursuit``, vap_pursuit_rollouts), goes through the same ``rollouts``: it is indexed by
where the robot is on the path, reads only the polyline (columns 6, 7) and the speeds (column 2), and takes a record's
slot 7 as that rollout's lookahead, so one call sweeps perturbations x lookaheads (``lookahead_sweep``).  It does not
execute reverse legs (``route_status`` bit 0), in-place turns or dwells.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._call import buffers, context_for, device_array, dptr, ptr, time_rows

MAX_ROLLOUTS = 4096
NOMINAL = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0)      # dx, dy, dphi, gain_left, gain_right, track_scale, tau, reserved


@dataclass
class Follower:
    """vap_follower: the robot's track width (ft), the RAMSETE gains b (1/ft^2) and zeta, the wheel speed limit (ft/s),
    the position error (ft) above which a rollout counts in ``n_exceeding``, the integration substeps per row and the
    rows the robot is given to settle on the last pose."""
    track_width: float = 1.0
    b: float = 2.0
    zeta: float = 0.7
    wheel_speed_max: float = 6.0
    tolerance: float = 0.25
    n_substeps: int = 2
    settle_rows: int = 50

    def validate(self):
        for name in ("track_width", "b", "zeta", "wheel_speed_max"):
            v = float(getattr(self, name))
            if not (v > 0 and np.isfinite(v)):
                raise ValueError(f"Follower.{name} must be positive and finite (got {v!r})")
        if np.isnan(float(self.tolerance)):
            raise ValueError("Follower.tolerance is NaN")
        if int(self.n_substeps) != self.n_substeps or not 1 <= int(self.n_substeps) <= 16:
            raise ValueError(f"Follower.n_substeps must be 1..16 (got {self.n_substeps!r})")
        if int(self.settle_rows) != self.settle_rows or not 0 <= int(self.settle_rows) <= 10000:
            raise ValueError(f"Follower.settle_rows must be 0..10000 (got {self.settle_rows!r})")
        return self

    def as_struct(self):
        return _lib.FollowerStruct(float(self.track_width), float(self.b), float(self.zeta), float(self.wheel_speed_max),
                                   float(self.tolerance), int(self.n_substeps), int(self.settle_rows))


@dataclass
class Pursuit:
    """vap_pursuit: the robot's track width (ft), the lookahead along the path's chord length (ft; a record's slot 7
    overrides it per rollout), the speed the command never falls below before arrival (ft/s), the distance to the last
    point at which the robot has arrived (ft), the wheel speed limit (ft/s), the cross-track error (ft) above which a
    rollout counts in ``n_exceeding``, the integration substeps per row and the rows past the plan's end the robot is
    given to arrive (a lagging drive arrives later than the plan)."""
    track_width: float = 1.0
    lookahead: float = 0.75
    min_speed: float = 0.1
    arrive_tolerance: float = 0.05
    wheel_speed_max: float = 6.0
    tolerance: float = 0.25
    n_substeps: int = 2
    settle_rows: int = 150

    def validate(self):
        for name in ("track_width", "lookahead", "wheel_speed_max"):
            v = float(getattr(self, name))
            if not (v > 0 and np.isfinite(v)):
                raise ValueError(f"Pursuit.{name} must be positive and finite (got {v!r})")
        for name in ("min_speed", "arrive_tolerance"):
            v = float(getattr(self, name))
            if not (v >= 0 and np.isfinite(v)):
                raise ValueError(f"Pursuit.{name} must be >= 0 and finite (got {v!r})")
        if np.isnan(float(self.tolerance)):
            raise ValueError("Pursuit.tolerance is NaN")
        if int(self.n_substeps) != self.n_substeps or not 1 <= int(self.n_substeps) <= 16:
            raise ValueError(f"Pursuit.n_substeps must be 1..16 (got {self.n_substeps!r})")
        if int(self.settle_rows) != self.settle_rows or not 0 <= int(self.settle_rows) <= 10000:
            raise ValueError(f"Pursuit.settle_rows must be 0..10000 (got {self.settle_rows!r})")
        return self

    def as_struct(self):
        return _lib.PursuitStruct(float(self.track_width), float(self.lookahead), float(self.min_speed),
                                  float(self.arrive_tolerance), float(self.wheel_speed_max), float(self.tolerance),
                                  int(self.n_substeps), int(self.settle_rows))


def sample_perturbations(B, K, pos_sigma=0.1, heading_sigma=0.05, gain_sigma=0.03, track_sigma=0.05, tau=0.05, seed=0,
                         nominal_first=True):
    """(B, K, 8) fp64 perturbation records drawn on the host with ``np.random.default_rng(seed)``: dx, dy ~ N(0,
    pos_sigma) ft, dphi ~ N(0, heading_sigma) rad, the wheel gains ~ 1 + N(0, gain_sigma), track_scale ~ 1 + N(0,
    track_sigma) (the three clipped to >= 0.5), the drive lag ``tau`` seconds for every record.  With ``nominal_first``
    rollout k = 0 of every route is the undisturbed record {0, 0, 0, 1, 1, 1, 0, 0}.  The same arguments give the same
    array."""
    B, K = int(B), int(K)
    if B < 0 or not 1 <= K <= MAX_ROLLOUTS:
        raise ValueError(f"B must be >= 0 and K in 1..{MAX_ROLLOUTS} (got {B}, {K})")
    for name, v in (("pos_sigma", pos_sigma), ("heading_sigma", heading_sigma), ("gain_sigma", gain_sigma),
                    ("track_sigma", track_sigma), ("tau", tau)):
        if not (float(v) >= 0 and np.isfinite(float(v))):
            raise ValueError(f"{name} must be >= 0 and finite (got {v!r})")
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, K, 6))
    p = np.zeros((B, K, 8), dtype=np.float64)
    p[..., 0:2] = z[..., 0:2] * float(pos_sigma)
    p[..., 2] = z[..., 2] * float(heading_sigma)
    p[..., 3:5] = np.maximum(1.0 + z[..., 3:5] * float(gain_sigma), 0.5)
    p[..., 5] = np.maximum(1.0 + z[..., 5] * float(track_sigma), 0.5)
    p[..., 6] = float(tau)
    if nominal_first:
        p[:, 0] = NOMINAL
    return p


def lookahead_sweep(perturbations, lookaheads):
    """The records of every perturbation x lookahead pair for a ``Pursuit`` call: ``perturbations`` (K, 8) or (B, K, 8)
    and ``lookaheads`` (M,) feet (0: the follower's own) give (K * M, 8) or (B, K * M, 8) fp64 records, pair (k, m) at
    k * M + m, slot 7 = lookaheads[m] and the other slots those of record k."""
    p = np.asarray(perturbations, dtype=np.float64)
    la = np.asarray(lookaheads, dtype=np.float64).reshape(-1)
    if p.ndim not in (2, 3) or p.shape[-1] != 8:
        raise ValueError(f"perturbations must be (K, 8) or (B, K, 8), got {p.shape}")
    if la.size < 1 or not (np.isfinite(la).all() and (la >= 0).all()):
        raise ValueError("lookaheads must be finite and >= 0")
    if p.shape[-2] * la.size > MAX_ROLLOUTS:
        raise ValueError(f"{p.shape[-2]} records x {la.size} lookaheads exceed {MAX_ROLLOUTS} rollouts per route")
    out = np.repeat(p, la.size, axis=-2)
    out[..., 7] = np.tile(la, p.shape[-2])
    return out


STAT_COLUMNS = ("max_error", "max_cross_track", "max_heading_error", "final_error", "final_heading_error")


PURSUIT_STAT_COLUMNS = ("max_cross_track", "final_error", "arrival_time", "lookahead")
PURSUIT_ROW_COLUMNS = ("max_row", "saturated_rows", "arrived_row", "closest_segment")


def _checked(follower, time_step):
    """(is it a Pursuit, time_step as a float) of a validated follower and time step."""
    if isinstance(follower, Pursuit):
        pursuit = True
    elif isinstance(follower, Follower):
        pursuit = False
    else:
        raise TypeError("follower must be a tracking.Follower or a tracking.Pursuit")
    follower.validate()
    time_step = float(time_step)
    if not (time_step > 0 and np.isfinite(time_step)):
        raise ValueError(f"time_step must be positive and finite (got {time_step!r})")
    return pursuit, time_step


def _records(perturbations, B, dev):
    """The records on ``dev`` as (tensor, shared, K): (B, K, 8), or (K, 8) shared by every route, K in 1..4096."""
    pert = device_array(perturbations, dev, torch.float64)
    shared = pert.dim() == 2
    if pert.dim() not in (2, 3) or pert.shape[-1] != 8 or (not shared and pert.shape[0] != B):
        raise ValueError(f"perturbations must be ({B}, K, 8) or (K, 8), got {tuple(pert.shape)}")
    K = int(pert.shape[-2])
    if not 1 <= K <= MAX_ROLLOUTS:
        raise ValueError(f"K = {K} rollouts per route (1..{MAX_ROLLOUTS})")
    return pert, shared, K


def _follower_shapes(B, K, pursuit):
    """The follower's own outputs: name -> (shape, dtype)."""
    shapes = {"stats": ((B, K, 6), torch.float64), "stat_rows": ((B, K, 4 if pursuit else 2), torch.int32), "worst": ((B,), torch.float64),
              "mean": ((B,), torch.float64), "worst_rollout": ((B,), torch.int32), "worst_row": ((B,), torch.int32),
              "n_exceeding": ((B,), torch.int32)}
    if pursuit:
        shapes["n_unfinished"] = ((B,), torch.int32)
        shapes["route_status"] = ((B,), torch.int32)
    return shapes


def _follower_views(res, pursuit):
    """The named columns of stats and stat_rows, as views."""
    for i, name in enumerate(PURSUIT_STAT_COLUMNS if pursuit else STAT_COLUMNS):
        res[name] = res["stats"][..., i]
    for i, name in enumerate(PURSUIT_ROW_COLUMNS if pursuit else ("max_row", "saturated_rows")):
        res[name] = res["stat_rows"][..., i]


def rollouts(rows, counts, follower, perturbations, time_step=0.01, executed=False, out=None, device=0, ctx=None):
    """Tracking rollouts of a batch of time-domain rows (vap_tracking_rollouts).

      rows           (B, capacity, 8) fp64 rows of time_profile / insert_waits — a device tensor (used in place) or a
                     host array (uploaded once); (n, 8) for a single trajectory
      counts         (B, k) int counts of that call (column 0 = rows), or (B,); None for a single trajectory
      follower       a Follower (RAMSETE) or a Pursuit (pure pursuit; see below)
      perturbations  (B, K, 8) records per route, or (K, 8) shared by every route (``sample_perturbations``); a device
                     tensor or a host array
      time_step      the rows' time step in seconds (time_profile's dt)
      executed       also return the executed rows: ``rows`` (B * K, capacity + settle_rows, 8) and ``counts``
                     (B * K, 2), rollout (b, k) at b * K + k — the dict can be passed to footprint.clearance /
                     footprint.conflicts (and the generator's footprint_clearance) as it is.  Rows past a rollout's
                     count are not written
      out            optional dict that keeps the call's buffers (stats, stat_rows, the per-route outputs, rows, counts, in
                     their batch shapes) between calls: a missing or mis-shaped entry is allocated into it, nothing else
                     in it is touched, and a later call with the same shapes allocates nothing
    Returns a dict of tensors: stats (B, K, 6) and its columns as views max_error, max_cross_track, max_heading_error,
    final_error, final_heading_error (B, K); stat_rows (B, K, 2) with views max_row and saturated_rows; per route (B,)
    worst, mean, worst_rollout, worst_row, n_exceeding.  A route without rows and an invalid record give NaN / -1 / 0.
    A single trajectory gives (K, ...) and 0-d tensors.  Work runs on torch's current stream and is not synchronised.

    With a ``Pursuit`` (vap_pursuit_rollouts) slot 7 of a record is that rollout's lookahead (``lookahead_sweep``) and
    the dict has: stats (B, K, 6) with views max_cross_track, final_error, arrival_time (NaN: never arrived), lookahead;
    stat_rows (B, K, 4) with views max_row, saturated_rows, arrived_row (-1: never), closest_segment; per route worst,
    mean, worst_rollout, worst_row, n_exceeding (over the cross-track error), n_unfinished (valid rollouts that never
    arrived) and route_status (bit 0: a negative speed, bit 1: a non-finite x, y or v; such a route gives NaN / -1 / 0)."""
    pursuit, time_step = _checked(follower, time_step)
    rows, counts, single, dev = time_rows(rows, counts, None, device)
    B, cap = int(rows.shape[0]), int(rows.shape[1])
    pert, shared, K = _records(perturbations, B, dev)
    cap_exec = cap + int(follower.settle_rows)
    shapes = _follower_shapes(B, K, pursuit)
    if executed:
        shapes["rows"] = ((B * K, cap_exec, 8), torch.float64)
        shapes["counts"] = ((B * K, 2), torch.int32)
    bufs = buffers(out, shapes, dev)       # the call's buffers; the returned dict is built apart from it
    res = {k: bufs[k] for k in shapes}
    ctx = context_for(dev, ctx)
    fs = follower.as_struct()
    if pursuit:
        _lib.check(ctx._L.vap_pursuit_rollouts(
            ctx.handle, B, cap, ptr(rows), ptr(counts), int(counts.shape[1]), time_step, C.byref(fs), K, int(shared), ptr(pert),
            ptr(res["stats"]), ptr(res["stat_rows"]), ptr(res["worst"]), ptr(res["mean"]), ptr(res["worst_rollout"]),
            ptr(res["worst_row"]), ptr(res["n_exceeding"]), ptr(res["n_unfinished"]), ptr(res["route_status"]), cap_exec,
            ptr(res.get("rows") if executed else None), ptr(res.get("counts") if executed else None)), "vap_pursuit_rollouts")
        _follower_views(res, True)
        return _single(res) if single else res
    _lib.check(ctx._L.vap_tracking_rollouts(
        ctx.handle, B, cap, ptr(rows), ptr(counts), int(counts.shape[1]), time_step, C.byref(fs), K, int(shared), ptr(pert),
        ptr(res["stats"]), ptr(res["stat_rows"]), ptr(res["worst"]), ptr(res["mean"]), ptr(res["worst_rollout"]),
        ptr(res["worst_row"]), ptr(res["n_exceeding"]), cap_exec, ptr(res.get("rows") if executed else None),
        ptr(res.get("counts") if executed else None)), "vap_tracking_rollouts")
    _follower_views(res, False)
    return _single(res) if single else res


def _single(res):
    for k in list(res):
        if k not in ("rows", "counts"):
            res[k] = res[k][0]
    return res


CLEAR_ROW_COLUMNS = ("clear_min_row", "clear_min_element", "clear_first_row", "clear_n_below")


def rollout_clearance(rows, counts, follower, perturbations, footprint, scene, margin=0.0, time_step=0.01, out=None, device=0,
                      ctx=None, cull=True):
    """Scene clearance of the disturbed rollouts (vap_rollout_clearance): does the robot still miss the post when it
    starts an inch off, one side runs weak and the drive lags?  ``rollouts(executed=True)`` followed by
    ``footprint.clearance`` answers that through B * K * (capacity + settle_rows) executed rows in memory; this call runs
    the same rollouts and takes the clearance of every executed row while it is on the chip.  No executed rows exist.

      rows, counts, follower, perturbations, time_step   as in ``rollouts`` (a Follower or a Pursuit)
      footprint, scene, margin, cull                     as in ``footprint.clearance``; a rollout whose clearance is below
                                                         ``margin`` counts as colliding
      out            optional dict that keeps the call's buffers between calls, as in ``rollouts``
    Returns everything ``rollouts`` returns for that follower (the same bits), and: clearance (B, K), the smallest
    clearance over the rollout's executed rows; clear_rows (B, K, 4) with views clear_min_row (the first row at it),
    clear_min_element (footprint.Scene.element_name), clear_first_row (the first row below ``margin``, -1: none),
    clear_n_below; per route (B,) worst_clearance (the smallest over k; the smallest k on a tie), worst_clear_rollout,
    worst_clear_row, worst_clear_element, mean_clearance, n_colliding (rollouts below ``margin``) and n_clear_valid (the
    rollouts that have rows: n_colliding / n_clear_valid is the collision share).  Per rollout these are the numbers
    ``footprint.clearance`` gives for the executed rows of ``rollouts(executed=True)``, bit for bit.  A rollout without
    rows gives NaN / -1 / 0, a route without one NaN / -1 / 0 / 0.  A single trajectory gives (K, ...) and 0-d tensors.
    Work runs on torch's current stream and is not synchronised."""
    from . import footprint as fp
    pursuit, time_step = _checked(follower, time_step)
    if not isinstance(scene, fp.Scene):
        raise TypeError("scene must be a footprint.Scene")
    foot = fp.convex_polygon(footprint, "footprint")
    margin = float(margin)
    if not np.isfinite(margin):
        raise ValueError(f"margin must be finite (got {margin!r})")
    rows, counts, single, dev = time_rows(rows, counts, None, device)
    B, cap = int(rows.shape[0]), int(rows.shape[1])
    pert, shared, K = _records(perturbations, B, dev)
    shapes = _follower_shapes(B, K, pursuit)
    shapes.update(clearance=((B, K), torch.float64), clear_rows=((B, K, 4), torch.int32), worst_clearance=((B,), torch.float64),
                  worst_clear_rollout=((B,), torch.int32), worst_clear_row=((B,), torch.int32),
                  worst_clear_element=((B,), torch.int32), mean_clearance=((B,), torch.float64), n_colliding=((B,), torch.int32),
                  n_clear_valid=((B,), torch.int32))
    bufs = buffers(out, shapes, dev)       # the call's buffers; the returned dict is built apart from it
    res = {k: bufs[k] for k in shapes}
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    fs = follower.as_struct()
    _lib.check(ctx._L.vap_rollout_clearance(
        ctx.handle, _lib.FOLLOWER_PURSUIT if pursuit else _lib.FOLLOWER_RAMSETE, C.cast(C.pointer(fs), C.c_void_p), B, cap,
        ptr(rows), ptr(counts), int(counts.shape[1]), time_step, K, int(shared), ptr(pert), len(foot), dptr(foot),
        *scene.c_args(), margin, ptr(res["stats"]), ptr(res["stat_rows"]), ptr(res["worst"]), ptr(res["mean"]),
        ptr(res["worst_rollout"]), ptr(res["worst_row"]), ptr(res["n_exceeding"]), ptr(res.get("n_unfinished")),
        ptr(res.get("route_status")), ptr(res["clearance"]), ptr(res["clear_rows"]), ptr(res["worst_clearance"]),
        ptr(res["worst_clear_rollout"]), ptr(res["worst_clear_row"]), ptr(res["worst_clear_element"]), ptr(res["mean_clearance"]),
        ptr(res["n_colliding"]), ptr(res["n_clear_valid"])), "vap_rollout_clearance")
    _follower_views(res, pursuit)
    for i, name in enumerate(CLEAR_ROW_COLUMNS):
        res[name] = res["clear_rows"][..., i]
    return _single(res) if single else res


CONFLICT_ROW_COLUMNS = ("conflict_other", "conflict_row", "conflict_n", "conflict_first_row")
CONFLICT_OTHERS_MAX = 16
CONFLICT_SHIFT_MAX = 1 << 24


def _shift_array(a, n, name, dev):
    """A per-route or per-rollout start shift as an (n,) int32 tensor on ``dev``; None stays None."""
    if a is None:
        return None
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name} must be integer rows (got dtype {a.dtype})")
    elif a.dtype.is_floating_point or a.dtype == torch.bool:
        raise ValueError(f"{name} must be integer rows (got dtype {a.dtype})")
    if tuple(a.shape) != (n,):
        raise ValueError(f"{name} must be ({n},), got {tuple(a.shape)}")
    return device_array(a, dev, torch.int32)


def rollout_conflicts(rows, counts, follower, perturbations, footprint, others_rows, others_counts, others_footprint=None,
                      margin=0.0, shift_rows=0, route_shift=None, rollout_shift=None, pairs=False, time_step=0.01, out=None,
                      device=0, ctx=None, cull=True):
    """Clearance of the disturbed rollouts to the partner's routines (vap_rollout_conflicts): does a disturbed run still
    miss my partner, whose start time is as uncertain as my own drive?  ``rollouts(executed=True)`` followed by
    ``footprint.conflicts`` answers that through every executed row in memory, packed a second time, one conflicts call
    per distinct shift; this call runs the same rollouts and takes the clearance to every partner route while the
    executed row is on the chip.  No executed rows exist.

      rows, counts, follower, perturbations, time_step   as in ``rollouts`` (a Follower or a Pursuit)
      footprint                     my robot's (n, 2) body-frame polygon, counter-clockwise
      others_rows, others_counts    side O as in ``footprint.conflicts``: (Bo, cap_o, 8) rows with (Bo, k) / (Bo,) counts, or
                                    one (n, 8) trajectory with counts None; 1 .. 16 routes, on the same time step
      others_footprint              side O's robot; None = the same as mine
      margin                        a pair whose clearance is below it conflicts
      shift_rows, route_shift, rollout_shift   side O starts shift_rows + route_shift[b] + rollout_shift[k] rows late for
                                    rollout (b, k): an int within +-2^24, (B,) ints or None, (K,) ints (shared by all
                                    routes) or None; the array entries are clamped into +-2^24
      pairs                         also return pair_clearance (B, K, Bo) and pair_rows (B, K, Bo, 2) = the first row at the
                                    pair's minimum, its first row below ``margin``
      out, ctx, cull                as in ``rollout_clearance``
    Returns everything ``rollouts`` returns for that follower (the same bits), and: conflict (B, K), the smallest clearance
    over the rollout's pairs and instants; conflict_rows (B, K, 4) with views conflict_other (the smallest o there),
    conflict_row, conflict_n (pairs below ``margin``), conflict_first_row (the earliest row any pair goes below it, -1:
    none); per route (B,) worst_conflict (the smallest over k; the smallest k on a tie), worst_conflict_rollout,
    worst_conflict_other, worst_conflict_row, mean_conflict, n_conflicting (rollouts below ``margin``) and n_conflict_valid.
    Per rollout these are the numbers ``footprint.conflicts`` gives for that executed route of ``rollouts(executed=True)``
    at that rollout's shift, bit for bit: instants run to max(n_a, n_o + s, 1), each robot parked at its first or last pose
    outside its own rows.  A rollout without rows gives NaN / -1 / 0, a route without one NaN / -1 / 0 / 0.  A single
    trajectory gives (K, ...) and 0-d tensors.  Work runs on torch's current stream and is not synchronised."""
    from . import footprint as fp
    pursuit, time_step = _checked(follower, time_step)
    foot_a, foot_o = fp._two_footprints(footprint, others_footprint, "all", names=("footprint", "others_footprint"))
    margin = float(margin)
    if not np.isfinite(margin):
        raise ValueError(f"margin must be finite (got {margin!r})")
    if int(shift_rows) != shift_rows or abs(int(shift_rows)) > CONFLICT_SHIFT_MAX:
        raise ValueError(f"shift_rows must be an int within +-{CONFLICT_SHIFT_MAX} (got {shift_rows!r})")
    shift_rows = int(shift_rows)
    rows, counts, single, dev = time_rows(rows, counts, None, device)
    B, cap = int(rows.shape[0]), int(rows.shape[1])
    pert, shared, K = _records(perturbations, B, dev)
    rows_o, counts_o, _, _ = time_rows(others_rows, others_counts, dev, device)
    Bo, cap_o = int(rows_o.shape[0]), int(rows_o.shape[1])
    if not 1 <= Bo <= CONFLICT_OTHERS_MAX:
        raise ValueError(f"others: {Bo} routes (1..{CONFLICT_OTHERS_MAX})")
    route_shift = _shift_array(route_shift, B, "route_shift", dev)
    rollout_shift = _shift_array(rollout_shift, K, "rollout_shift", dev)
    shapes = _follower_shapes(B, K, pursuit)
    shapes.update(conflict=((B, K), torch.float64), conflict_rows=((B, K, 4), torch.int32), worst_conflict=((B,), torch.float64),
                  worst_conflict_rollout=((B,), torch.int32), worst_conflict_other=((B,), torch.int32),
                  worst_conflict_row=((B,), torch.int32), mean_conflict=((B,), torch.float64), n_conflicting=((B,), torch.int32),
                  n_conflict_valid=((B,), torch.int32))
    if pairs:
        shapes.update(pair_clearance=((B, K, Bo), torch.float64), pair_rows=((B, K, Bo, 2), torch.int32))
    bufs = buffers(out, shapes, dev)       # the call's buffers; the returned dict is built apart from it
    res = {k: bufs[k] for k in shapes}
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    fs = follower.as_struct()
    _lib.check(ctx._L.vap_rollout_conflicts(
        ctx.handle, _lib.FOLLOWER_PURSUIT if pursuit else _lib.FOLLOWER_RAMSETE, C.cast(C.pointer(fs), C.c_void_p), B, cap,
        ptr(rows), ptr(counts), int(counts.shape[1]), time_step, K, int(shared), ptr(pert), len(foot_a), dptr(foot_a),
        Bo, cap_o, ptr(rows_o), ptr(counts_o), int(counts_o.shape[1]), len(foot_o), dptr(foot_o), margin, shift_rows,
        ptr(route_shift), ptr(rollout_shift), ptr(res["stats"]), ptr(res["stat_rows"]), ptr(res["worst"]), ptr(res["mean"]),
        ptr(res["worst_rollout"]), ptr(res["worst_row"]), ptr(res["n_exceeding"]), ptr(res.get("n_unfinished")),
        ptr(res.get("route_status")), ptr(res.get("pair_clearance")), ptr(res.get("pair_rows")), ptr(res["conflict"]),
        ptr(res["conflict_rows"]), ptr(res["worst_conflict"]), ptr(res["worst_conflict_rollout"]), ptr(res["worst_conflict_other"]),
        ptr(res["worst_conflict_row"]), ptr(res["mean_conflict"]), ptr(res["n_conflicting"]), ptr(res["n_conflict_valid"])),
        "vap_rollout_conflicts")
    _follower_views(res, pursuit)
    for i, name in enumerate(CONFLICT_ROW_COLUMNS):
        res[name] = res["conflict_rows"][..., i]
    return _single(res) if single else res
