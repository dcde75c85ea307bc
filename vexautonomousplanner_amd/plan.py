"""Seed routes through a scene, planned on a grid on the device (vap_plan_grid, vap_plan_seeds, vap_plan_occupancy,
vap_plan_seeds_occupied, vap_plan_travel, vap_plan_order, vap_plan_order_timed, include/vap.h).

``search.refine`` improves a route that is already roughly right: it draws candidates round a mean, coordinate by
coordinate, and cannot get round an obstacle that is larger than its sigma.  This module gives it the route to start from.
The robot is a disc of radius ``radius`` on a grid of ``cell``-sized squares over the scene's field box; a cell is free when
the disc at its centre clears the walls, polygons and circles of the ``footprint.Scene`` by ``margin``; a shortest 8-connected
path from the start's cell to the goal's is pulled taut by line of sight and resampled at equal arc into W waypoints.
``seeds(...)["waypoints"]`` goes straight into ``refine(seeds=...)``.

The disc stands in for the robot's footprint: ``circumscribed_radius`` is safe at every heading (and may not fit through a
gap the robot can pass lengthways), ``inscribed_radius`` is necessary but not sufficient.  The seeds are not checked routes:
the first and last segment join the exact start and goal to cell centres, so they may be off by half a cell, more when the
start or goal had to be snapped to the nearest free cell (a robot parked against a wall).  ``refine`` does the checking.

A partner's routine is no part of the scene: ``occupancy`` rasterises its time-domain rows onto the same grid (per cell the
first and last instant at which its footprint leaves the disc less than ``margin``), and ``seeds(occupancy=..., windows=...)``
keeps each problem off the cells occupied within its window of instants.

A routine is a start and a handful of sites: ``travel`` plans every ordered pair of P points at the price of P distance
fields, ``order`` finds the cheapest visiting order from any (P, P) cost matrix on the device, and ``routine`` chains the
two and gathers the legs in visiting order, ready for ``refine(seeds=...)``, without a host synchronisation.  ``order_timed``
orders the sites by the clock instead — the rows of the chained timeline, turns on the spot and dwells included, optionally
the most valuable sites within a budget of seconds — and ``timed_routine`` runs the whole chain from the scene to that
timeline.

Units: feet, in the scene's frame.  At most 16384 cells (the distance field of a problem lives in one workgroup's LDS).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._call import buffers, context_for, device_array, dptr, ptr, time_rows
from .footprint import Scene, _ccw_polygon, convex_polygon
from .synth import DEFAULT_CONSTRAINTS

MAX_CELLS = 16384
MAX_WAYPOINTS = 2048
FLAGS = {"degenerate": _lib.FLAG_DEGENERATE, "noconverge": _lib.FLAG_NOCONVERGE, "snapped_start": _lib.PLAN_SNAPPED_START,
         "snapped_goal": _lib.PLAN_SNAPPED_GOAL, "no_free": _lib.PLAN_NO_FREE, "unreachable": _lib.PLAN_UNREACHABLE,
         "vertices_truncated": _lib.PLAN_VERTICES_TRUNCATED, "order_infeasible": _lib.ORDER_INFEASIBLE}
MAX_POINTS = _lib.PLAN_TRAVEL_MAX_POINTS
MAX_SITES = _lib.PLAN_ORDER_MAX_SITES


def circumscribed_radius(footprint):
    """The largest distance from the tracked point (the body origin) to a vertex of the footprint polygon, feet: a disc of
    this radius contains the robot at every heading."""
    v = convex_polygon(footprint, "footprint")
    return float(np.sqrt((v * v).sum(axis=1)).max())


def inscribed_radius(footprint):
    """The smallest distance from the tracked point to an edge line of the footprint polygon, feet: the largest disc
    round the tracked point inside the robot.  The tracked point must lie inside the footprint."""
    v = convex_polygon(footprint, "footprint")
    e = np.roll(v, -1, axis=0) - v
    s = (v[:, 0] * e[:, 1] - v[:, 1] * e[:, 0]) / np.sqrt((e * e).sum(axis=1))   # inward distance of the origin per edge
    if not (s > 0).all():
        raise ValueError("the tracked point (the body origin) must lie inside the footprint")
    return float(s.min())


def grid_shape(scene, cell):
    """(ny, nx) of the grid over ``scene``'s field box."""
    ny, nx, _ = _check(scene, cell, 0.0, 0.0)
    return ny, nx


def _check(scene, cell, radius, margin):
    """Validate what both calls share; returns (ny, nx, the scene arguments of the C-ABI)."""
    if not isinstance(scene, Scene):
        raise TypeError("scene must be a footprint.Scene")
    if scene.field is None:
        raise ValueError("the planner needs a scene with a field box")
    cell, radius, margin = float(cell), float(radius), float(margin)
    if not (cell > 0 and np.isfinite(cell)):
        raise ValueError(f"cell must be positive and finite (got {cell!r})")
    if not (radius >= 0 and np.isfinite(radius)):
        raise ValueError(f"radius must be >= 0 and finite (got {radius!r})")
    if not np.isfinite(margin):
        raise ValueError(f"margin must be finite (got {margin!r})")
    f = scene.field
    nx, ny = int(np.ceil((f[2] - f[0]) / cell)), int(np.ceil((f[3] - f[1]) / cell))
    if nx * ny > MAX_CELLS:
        raise ValueError(f"a grid of {nx} x {ny} cells: at most {MAX_CELLS} cells (use a larger cell)")
    return ny, nx, scene.c_args() + (cell, radius, margin)


def clearance_grid(scene, cell, radius, margin=0.0, out=None, device=0, ctx=None):
    """The planner's grid (vap_plan_grid): ``clearance`` (ny, nx) fp64, the disc's clearance at every cell centre, and
    ``free`` (ny, nx) bool, clearance >= margin.  Row j, column i is the cell whose centre is (xmin + (i + 0.5) cell,
    ymin + (j + 0.5) cell).  Device tensors on torch's current stream, not synchronised; ``out`` keeps the buffers."""
    ny, nx, args = _check(scene, cell, radius, margin)
    dev = torch.device("cuda", device)
    res = buffers(out, {"clearance": ((ny, nx), torch.float64), "free_u8": ((ny, nx), torch.uint8)}, dev)
    ctx = context_for(dev, ctx)
    _lib.check(ctx._L.vap_plan_grid(ctx.handle, *args, ptr(res["clearance"]), ptr(res["free_u8"]), None, None), "vap_plan_grid")
    res["free"] = res["free_u8"].view(torch.bool)
    return res


def _waypoint_count(waypoints):
    W = int(waypoints)
    if W != waypoints or W < 2:
        raise ValueError(f"waypoints must be an integer >= 2 (got {waypoints!r})")
    if W > MAX_WAYPOINTS:
        raise ValueError(f"waypoints = {W}: at most {MAX_WAYPOINTS}")
    return W


def _points(p, dev, what):
    t = device_array(p, dev, torch.float64)
    single = t.dim() == 1
    if single:
        t = t.unsqueeze(0)
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f"{what} must be (R, 2) or (2,), got {tuple(p.shape) if hasattr(p, 'shape') else p!r}")
    return t, single


INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def occupancy(rows, counts, footprint, scene, cell, radius, margin=0.0, shift_rows=0, hold_first=False, hold_last=True,
              min_clearance=False, out=None, device=0, ctx=None, cull=True):
    """Time-domain rows rasterised onto the planner's grid (vap_plan_occupancy).

      rows, counts   the dict ``time_profile`` / ``insert_waits`` / ``tracking.rollouts(executed=True)`` returned (then
                     ``counts`` is None), or (B, capacity, 8) fp64 rows with their (B, k) or (B,) counts as
                     ``footprint.clearance`` takes them; (n, 8) rows with counts None for a single trajectory
      footprint      (n, 2) body-frame polygon of the robot that drives the rows, counter-clockwise, feet
      scene, cell    the grid: ``scene``'s field box over ``cell``-sized squares, as ``clearance_grid`` lays it out
      radius, margin the disc that will be planned (mine) and the clearance it wants: a row covers a cell when the disc at
                     the cell's centre clears the posed footprint by less than ``margin``
      shift_rows     row r stands at instant r + shift_rows
      hold_first     the robot stands at its first pose before instant shift_rows: first = INT_MIN where row 0 covers
      hold_last      it stays at its last pose: last = INT_MAX where the last row covers
      min_clearance  also return the smallest clearance of every cell over all rows (+inf without rows)
      out            optional dict of tensors of the shapes below to reuse; cull: VAP_OPT_FOOTPRINT_CULL (the same bits)
    Returns a dict of (ny, nx) device tensors: first, last (int32; INT_MAX / INT_MIN where never covered), count (int32,
    covering rows), blocked (bool: covered at some instant), and min_clearance (fp64) if asked.  All B routes go into the
    one grid.  Work runs on torch's current stream and is not synchronised."""
    if isinstance(rows, dict):
        if counts is not None:
            raise ValueError("counts comes with the dict of rows")
        rows, counts = rows["rows"], rows["counts"]
    ny, nx, _ = _check(scene, cell, radius, margin)
    foot = _ccw_polygon(footprint, "footprint")
    rows, counts, _, dev = time_rows(rows, counts, None, device, "occupancy")
    shift_rows = int(shift_rows)
    shapes = {"first": ((ny, nx), torch.int32), "last": ((ny, nx), torch.int32), "count": ((ny, nx), torch.int32)}
    if min_clearance:
        shapes["min_clearance"] = ((ny, nx), torch.float64)
    res = buffers(out, shapes, dev)
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    _lib.check(ctx._L.vap_plan_occupancy(
        ctx.handle, int(rows.shape[0]), int(rows.shape[1]), ptr(rows), ptr(counts), int(counts.shape[1]), len(foot), dptr(foot),
        dptr(scene.field), float(cell), float(radius), float(margin), shift_rows, int(bool(hold_first)), int(bool(hold_last)),
        ptr(res["first"]), ptr(res["last"]), ptr(res["count"]), ptr(res["min_clearance"] if min_clearance else None), None,
        None), "vap_plan_occupancy")
    res["blocked"] = res["first"] <= res["last"]
    return res


def seeds(starts, goals, scene, waypoints, radius, cell=0.25, margin=0.0, max_vertices=64, vertices=False, distance=False,
          out=None, device=0, ctx=None, occupancy=None, windows=None):
    """Seed routes for R (start, goal) pairs (vap_plan_seeds; with an occupancy vap_plan_seeds_occupied).

      starts, goals   (R, 2) or (2,) points in feet: device tensors (any float type, used as fp64) or host arrays
      scene           a footprint.Scene with a field box
      waypoints       W, the number of waypoints per route (2..2048); the first and last are the start and goal themselves
      radius          the disc that stands in for the robot, feet (``circumscribed_radius(footprint)``)
      cell, margin    the grid's cell size and the clearance a free cell needs, feet
      vertices        also return the pulled path's vertices (R, max_vertices, 2), NaN behind the last
      distance        also return every problem's distance field (R, ny, nx), +inf where blocked or unreached
      out             optional dict of tensors of the shapes below to reuse
      occupancy       what ``occupancy(...)`` returned for the same scene and cell (or a (first, last) pair of (ny, nx)
                      int32 device tensors): the cells a partner occupies, and when, are not free
      windows         (R, 2) or (2,) integers (t0, t1): problem r keeps off the cells occupied at some instant of
                      [t0, t1); None: at any instant.  Needs ``occupancy``
    Returns a dict of device tensors: waypoints (R, W, 2) fp64, length (R,) (the polyline's, +inf on failure), flags (R,)
    int32 (``plan.FLAGS``), n_vertices (R,) int32, feasible (R,) bool (a route was found), and the optional ones.  A failed
    problem (no free cell, unreachable goal, non-finite point) has NaN waypoints.  A single pair gives (W, 2) and 0-d
    tensors.  Work runs on torch's current stream and is not synchronised."""
    W = _waypoint_count(waypoints)
    max_vertices = int(max_vertices)
    if vertices and max_vertices < 2:
        raise ValueError(f"max_vertices must be >= 2 (got {max_vertices})")
    ny, nx, args = _check(scene, cell, radius, margin)
    given = [p.device for p in (starts, goals) if isinstance(p, torch.Tensor) and p.device.type == "cuda"]
    dev = given[0] if given else torch.device("cuda", device)
    starts, single = _points(starts, dev, "starts")
    goals, _ = _points(goals, dev, "goals")
    if starts.shape != goals.shape:
        raise ValueError(f"starts and goals must have the same shape, got {tuple(starts.shape)} and {tuple(goals.shape)}")
    R = int(starts.shape[0])
    shapes = {"waypoints": ((R, W, 2), torch.float64), "length": ((R,), torch.float64), "flags": ((R,), torch.int32),
              "n_vertices": ((R,), torch.int32)}
    if vertices:
        shapes["vertices"] = ((R, max_vertices, 2), torch.float64)
    if distance:
        shapes["distance"] = ((R, ny, nx), torch.float64)
    first, last, windows = _occupancy_args(occupancy, windows, R, ny, nx, dev)
    res = buffers(out, shapes, dev)
    outs = (ptr(res["waypoints"]), ptr(res["length"]), ptr(res["flags"]), ptr(res["n_vertices"]),
            ptr(res["vertices"] if vertices else None), ptr(res["distance"] if distance else None))
    ctx = context_for(dev, ctx)
    if occupancy is None:
        _lib.check(ctx._L.vap_plan_seeds(ctx.handle, R, W, ptr(starts), ptr(goals), *args, max_vertices, *outs), "vap_plan_seeds")
    else:
        _lib.check(ctx._L.vap_plan_seeds_occupied(ctx.handle, R, W, ptr(starts), ptr(goals), *args, max_vertices, ptr(first),
                                                  ptr(last), ptr(windows), *outs), "vap_plan_seeds_occupied")
    res["feasible"] = res["n_vertices"] > 0
    if single:
        res = {k: v[0] for k, v in res.items()}
    return res


def _occupancy_args(occupancy, windows, R, ny, nx, dev):
    """(first, last, windows) device tensors for the C-ABI, or three Nones without an occupancy."""
    if occupancy is None:
        if windows is not None:
            raise ValueError("windows needs an occupancy")
        return None, None, None
    first, last = (occupancy["first"], occupancy["last"]) if isinstance(occupancy, dict) else occupancy
    for t in (first, last):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.int32 or tuple(t.shape) != (ny, nx):
            raise ValueError(f"occupancy must be ({ny}, {nx}) int32 tensors on {dev} (plan.occupancy with the same scene and cell)")
    if windows is not None:
        windows = device_array(windows, dev, torch.int32)
        if windows.dim() == 1:
            windows = windows.unsqueeze(0).expand(R, 2)
        if tuple(windows.shape) != (R, 2):
            raise ValueError(f"windows must be ({R}, 2) or (2,), got {tuple(windows.shape)}")
        windows = windows.contiguous()
    return first.contiguous(), last.contiguous(), windows


def travel(points, scene, radius, cell=0.25, margin=0.0, waypoints=None, occupancy=None, windows=None, out=None, device=0,
           ctx=None):
    """All ordered pairs of P points per problem, at the price of P distance fields (vap_plan_travel).

      points          (R, P, 2) or (P, 2) points in feet, 2 <= P <= 16: a device tensor (any float type, used as fp64) or a
                      host array
      scene, radius, cell, margin   as ``seeds`` takes them
      waypoints       W: also return every pair's W waypoints (2..2048); None: lengths, flags and vertex counts only
      occupancy, windows   as ``seeds`` takes them; problem r's one window (R, 2) or (2,) holds for all its pairs
      out             optional dict of tensors of the shapes below to reuse
    Returns a dict of device tensors: travel (R, P, P) fp64, entry [r, a, b] the length of the seed route from point a to
    point b (+inf where there is none, 0 on the diagonal), flags (R, P, P) int32 (``plan.FLAGS``), n_vertices (R, P, P)
    int32, feasible (R, P, P) bool (travel is finite), and waypoints (R, P, P, W, 2) if asked.  Off the diagonal every entry
    is what ``seeds(points[r, a], points[r, b], ...)`` gives, bit for bit; the matrix is not symmetric.  A single (P, 2) set
    gives results without the leading axis.  Work runs on torch's current stream and is not synchronised."""
    W = 2 if waypoints is None else _waypoint_count(waypoints)
    ny, nx, args = _check(scene, cell, radius, margin)
    dev = points.device if isinstance(points, torch.Tensor) and points.device.type == "cuda" else torch.device("cuda", device)
    pts = device_array(points, dev, torch.float64)
    single = pts.dim() == 2
    if single:
        pts = pts.unsqueeze(0)
    if pts.dim() != 3 or pts.shape[2] != 2:
        raise ValueError(f"points must be (R, P, 2) or (P, 2), got {tuple(points.shape)}")
    R, P = int(pts.shape[0]), int(pts.shape[1])
    if not 2 <= P <= MAX_POINTS:
        raise ValueError(f"P = {P} points: 2..{MAX_POINTS}")
    shapes = {"travel": ((R, P, P), torch.float64), "flags": ((R, P, P), torch.int32), "n_vertices": ((R, P, P), torch.int32)}
    if waypoints is not None:
        shapes["waypoints"] = ((R, P, P, W, 2), torch.float64)
    first, last, windows = _occupancy_args(occupancy, windows, R, ny, nx, dev)
    res = buffers(out, shapes, dev)
    ctx = context_for(dev, ctx)
    _lib.check(ctx._L.vap_plan_travel(ctx.handle, R, P, W, ptr(pts), *args, 0, ptr(first), ptr(last), ptr(windows),
                                      ptr(res["travel"]), ptr(res["flags"]), ptr(res["n_vertices"]),
                                      ptr(res["waypoints"] if waypoints is not None else None)), "vap_plan_travel")
    res["feasible"] = torch.isfinite(res["travel"])
    if single:
        res = {k: v[0] for k, v in res.items()}
    return res


def before_masks(before, R, P):
    """(R, P) uint32 precedence masks from a list of (earlier, later) site pairs (the same for every problem): bit j - 1 of
    entry k says site j comes before site k.  Host only."""
    m = np.zeros(P, dtype=np.int64)
    for pair in before:
        if len(pair) != 2:
            raise ValueError(f"before must hold (earlier, later) pairs, got {pair!r}")
        j, k = int(pair[0]), int(pair[1])
        if not (1 <= j < P and 1 <= k < P):
            raise ValueError(f"before pair {pair!r}: sites are 1..{P - 1}")
        m[k] |= 1 << (j - 1)
    return np.broadcast_to(m.astype(np.uint32), (R, P)).copy()


def order(cost, end=None, before=None, out=None, ctx=None):
    """The cheapest order to visit M = P - 1 sites in, starting from point 0, by Held-Karp on the device (vap_plan_order).

      cost     (R, P, P) or (P, P) fp64 device tensor, cost[r, a, b] of going from point a to point b, 2 <= P <= 11: what
               ``travel`` returned, or anything made of it with torch on the device (seconds, dwell times, +inf for a
               forbidden leg; NaN and -inf count as +inf)
      end      None: the routine may end at any site; 1..M: it ends at that site
      before   precedence: an (R, P) or (P,) integer tensor or array of masks (bit j - 1 of entry k: site j before site k),
               or a list of (earlier, later) site pairs, turned into the masks on the host
      out      optional dict of tensors of the shapes below to reuse
    Returns a dict of device tensors: order (R, M) int32, the sites in visiting order (-1 where infeasible), total (R,) fp64
    (the left-to-right sum along the order; +inf where infeasible), flags (R,) int32 (``FLAGS["order_infeasible"]``) and
    feasible (R,) bool.  A single (P, P) matrix gives results without the leading axis.  Work runs on torch's current
    stream and is not synchronised."""
    if not isinstance(cost, torch.Tensor) or cost.device.type != "cuda":
        raise ValueError("cost must be a device tensor")
    dev = cost.device
    c = cost.to(dtype=torch.float64)
    single = c.dim() == 2
    if single:
        c = c.unsqueeze(0)
    if c.dim() != 3 or c.shape[1] != c.shape[2]:
        raise ValueError(f"cost must be (R, P, P) or (P, P), got {tuple(cost.shape)}")
    c = c.contiguous()
    R, P = int(c.shape[0]), int(c.shape[1])
    M = P - 1
    if not 1 <= M <= MAX_SITES:
        raise ValueError(f"P = {P} points: 2..{MAX_SITES + 1} (the start and at most {MAX_SITES} sites)")
    e = -1 if end is None else int(end)
    if end is not None and (e != end or not 1 <= e <= M):
        raise ValueError(f"end must be None or a site 1..{M} (got {end!r})")
    b = None
    if before is not None:
        if isinstance(before, (list, tuple)):                        # (earlier, later) pairs
            before = before_masks(before, R, P)
        b = device_array(before, dev, torch.int64)
        if b.dim() == 1:
            b = b.unsqueeze(0).expand(R, P)
        if tuple(b.shape) != (R, P):
            raise ValueError(f"before must be ({R}, {P}) or ({P},) masks or a list of (earlier, later) pairs, got {tuple(b.shape)}")
        b = (b & (2 ** MAX_SITES - 1)).to(torch.int32).contiguous()  # bits >= M are ignored anyway
    res = buffers(out, {"order": ((R, M), torch.int32), "total": ((R,), torch.float64), "flags": ((R,), torch.int32)}, dev)
    ctx = context_for(dev, ctx)
    _lib.check(ctx._L.vap_plan_order(ctx.handle, R, P, ptr(c), e, ptr(b), ptr(res["order"]), ptr(res["total"]),
                                     ptr(res["flags"])), "vap_plan_order")
    res["feasible"] = res["flags"] == 0
    if single:
        res = {k: v[0] for k, v in res.items()}
    return res


def routine(points, scene, waypoints, radius, cell=0.25, margin=0.0, occupancy=None, windows=None, end=None, before=None,
            leg_cost=None, out=None, device=0, ctx=None):
    """A routine's visiting order and the seed route of each leg: ``travel`` with waypoints, ``order`` on its lengths (or on
    ``leg_cost(travel)``, a callable on the (R, P, P) device tensor that returns the costs), then the M legs
    0 -> o_1 -> ... -> o_M gathered out of the travel's waypoints on the device.  points[.., 0, :] is where the routine
    starts, the other P - 1 <= 10 points are the sites.

    Returns what ``order`` returned (order, total, flags, feasible), the travel outputs under travel, travel_flags,
    n_vertices and waypoints, and legs (R, M, W, 2): ``legs.reshape(R * M, W, 2)`` is what ``refine(seeds=...)`` takes.  An
    infeasible problem has NaN legs.  Nothing here reads a result on the host."""
    if leg_cost is not None and not callable(leg_cost):
        raise TypeError("leg_cost must be a callable on the travel tensor")
    out = {} if out is None else out
    tr = travel(points, scene, radius, cell=cell, margin=margin, waypoints=waypoints, occupancy=occupancy, windows=windows,
                out=out.setdefault("_travel", {}), device=device, ctx=ctx)
    single = tr["travel"].dim() == 2
    if single:
        tr = {k: v[None] for k, v in tr.items()}
    t, wp = tr["travel"], tr["waypoints"]
    R = int(t.shape[0])
    od = order(t if leg_cost is None else leg_cost(t), end=end, before=before, out=out.setdefault("_order", {}), ctx=ctx)
    o = od["order"].to(torch.int64)
    feasible = od["feasible"]
    to = o.clamp(min=0)
    frm = torch.cat([torch.zeros_like(to[:, :1]), to[:, :-1]], dim=1)
    rows = torch.arange(R, device=t.device)[:, None]
    legs = wp[rows, frm, to]
    legs = torch.where(feasible[:, None, None, None], legs, torch.full_like(legs, float("nan")))
    res = {"order": od["order"], "total": od["total"], "flags": od["flags"], "feasible": feasible, "travel": t,
           "travel_flags": tr["flags"], "n_vertices": tr["n_vertices"], "waypoints": wp, "legs": legs}
    if single:
        res = {k: v[0] for k, v in res.items()}
    out.update(res)
    return res


MAX_TIMED_SITES = _lib.PLAN_ORDER_TIMED_MAX_SITES
_INT_MAX = 2147483647


def order_timed(rows, counts, leg, dwell=None, start_heading=None, value=None, budget=None, end=None, before=None,
                leg_flags=None, constraints=DEFAULT_CONSTRAINTS, dt=0.01, turn_min=math.radians(1.0), out=None, ctx=None):
    """The visiting order that takes the fewest ROWS of the chained timeline, by Held-Karp over (site set, last site, site
    before it) on the device (vap_plan_order_timed): per slot the rows of the turn on the spot (they depend on the heading
    the robot arrives with, so on the leg before, which no (P, P) cost matrix can carry), the leg's own rows and
    int(dwell / dt).  ``rows_total`` IS ``timeline.chain(...)["counts"][:, 0]`` for the returned order, and
    ``arrival_rows`` its ``map[:, :, 2]``.

      rows, counts   the L legs as ``time_profile`` returns them: (L, capacity, 8) fp64 device tensor or host array, with
                     (L, k) / (L,) counts (column 0 = rows), all on the time step ``dt``.  Any legs' rows will do: profile
                     ``search.refine``'s ``best_waypoints`` of all pairs first and the order is that of the refined legs
      leg            (R, P, P) or (P, P) int: the leg from point a to point b (point 0 = the start, 1..M = P - 1 <= 8 the
                     sites); column 0 and the diagonal are not read.  A leg outside [0, L), with a non-zero ``leg_flags``
                     entry, without rows, or whose first or last row the timeline would refuse, is forbidden
      dwell          (R, P) seconds spent at SITE j (entry 0 unused), device or host; None = none
      start_heading  (R,) the heading the robot stands at before the first leg, NaN = none; None = none
      value          (R, P) worth of site j in budget mode (NaN, negative, infinite: 0); None = 1 each
      budget         None: visit every site in the fewest rows.  Seconds (a scalar, an (R,) host array or device tensor):
                     the most valuable set of sites whose routine takes at most int(budget / dt) rows, then the fewest
                     rows, then the lowest set; turned into rows on the device, nothing is read back
      end, before    as ``order`` takes them
      leg_flags      (L,) int, e.g. the ``flags`` of the legs' profile; a non-zero entry forbids the leg
      constraints, dt, turn_min   as ``timeline.chain`` takes them
      out            optional dict of tensors of the shapes below to reuse
    Returns a dict of device tensors: order (R, M) int32 (the visited sites, then -1), n_visited (R,) int32, rows_total
    (R,) int32 (-1 where infeasible), arrival_rows (R, M) int32 (-1 behind the visited slots), value_total (R,) fp64, flags
    (R,) int32 (``FLAGS["order_infeasible"]``), feasible (R,) bool, and in seconds duration (R,) = rows_total * dt and
    arrival (R, M) = arrival_rows * dt (NaN where the rows are -1).  A single (P, P) ``leg`` gives results without the
    leading axis.  Work runs on torch's current stream and is not synchronised."""
    dt, turn_min = float(dt), float(turn_min)
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError(f"dt must be positive and finite (got {dt!r})")
    if not (turn_min >= 0 and math.isfinite(turn_min)):
        raise ValueError(f"turn_min must be >= 0 and finite (got {turn_min!r})")
    c = _lib.make_constraints(constraints)
    rows, counts, one_leg, dev = time_rows(rows, counts, None, 0, "legs")
    if one_leg:
        raise ValueError("rows must be (L, capacity, 8): a batch of legs")
    L, cap = int(rows.shape[0]), int(rows.shape[1])
    shape = tuple(leg.shape) if hasattr(leg, "shape") else np.shape(leg)
    single = len(shape) == 2
    if len(shape) not in (2, 3) or shape[-1] != shape[-2]:
        raise ValueError(f"leg must be (R, P, P) or (P, P), got {shape}")
    P = int(shape[-1])
    R = 1 if single else int(shape[0])
    M = P - 1
    if not 1 <= M <= MAX_TIMED_SITES:
        raise ValueError(f"P = {P} points: 2..{MAX_TIMED_SITES + 1} (the start and at most {MAX_TIMED_SITES} sites)")
    e = -1 if end is None else int(end)
    if end is not None and (e != end or not 1 <= e <= M):
        raise ValueError(f"end must be None or a site 1..{M} (got {end!r})")

    def arg(a, dtype, shp, what):
        if isinstance(a, torch.Tensor) and a.device.type == "cuda" and a.device != dev:
            raise ValueError(f"{what} is on {a.device}, the rows on {dev}")
        t = device_array(a, dev, dtype)
        if t is not None and single and t.dim() == len(shp) - 1:
            t = t.unsqueeze(0)
        if t is not None and tuple(t.shape) != shp:
            raise ValueError(f"{what} must be {shp}, got {tuple(t.shape)}")
        return None if t is None else t.contiguous()

    leg = arg(leg, torch.int32, (R, P, P), "leg")
    dwell = arg(dwell, torch.float64, (R, P), "dwell")
    value = arg(value, torch.float64, (R, P), "value")
    if start_heading is not None and single:
        start_heading = device_array(start_heading, dev, torch.float64).reshape(-1)
    start_heading = arg(start_heading, torch.float64, (R,), "start_heading")
    leg_flags = device_array(leg_flags, dev, torch.int32)
    if leg_flags is not None and tuple(leg_flags.shape) != (L,):
        raise ValueError(f"leg_flags must be ({L},), got {tuple(leg_flags.shape)}")
    b = None
    if before is not None:
        if isinstance(before, (list, tuple)):                        # (earlier, later) pairs
            before = before_masks(before, R, P)
        b = device_array(before, dev, torch.int64)
        if b.dim() == 1:
            b = b.unsqueeze(0).expand(R, P)
        if tuple(b.shape) != (R, P):
            raise ValueError(f"before must be ({R}, {P}) or ({P},) masks or a list of (earlier, later) pairs, got {tuple(b.shape)}")
        b = (b & (2 ** MAX_TIMED_SITES - 1)).to(torch.int32).contiguous()
    budget_rows = None
    if budget is not None:                                           # int(budget / dt), saturating; NaN and negatives: 0
        q = device_array(budget, dev, torch.float64)
        if q.numel() == 1:
            q = q.reshape(()).expand(R)
        if tuple(q.shape) != (R,):
            raise ValueError(f"budget must be a scalar or ({R},) seconds, got {tuple(q.shape)}")
        q = torch.nan_to_num(q / dt, nan=0.0, posinf=float(_INT_MAX), neginf=0.0)
        budget_rows = q.clamp(0.0, float(_INT_MAX)).to(torch.int32).contiguous()
    res = buffers(out, {"order": ((R, M), torch.int32), "n_visited": ((R,), torch.int32), "rows_total": ((R,), torch.int32),
                        "arrival_rows": ((R, M), torch.int32), "value_total": ((R,), torch.float64),
                        "flags": ((R,), torch.int32)}, dev)
    ctx = context_for(dev, ctx)
    _lib.check(ctx._L.vap_plan_order_timed(
        ctx.handle, R, P, L, cap, dt, C.byref(c), turn_min, ptr(rows), ptr(counts), int(counts.shape[1]), ptr(leg),
        ptr(leg_flags), ptr(dwell), ptr(start_heading), ptr(value), ptr(budget_rows), e, ptr(b), ptr(res["order"]),
        ptr(res["n_visited"]), ptr(res["rows_total"]), ptr(res["arrival_rows"]), ptr(res["value_total"]), ptr(res["flags"])),
        "vap_plan_order_timed")
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    res["feasible"] = res["flags"] == 0
    res["duration"] = torch.where(res["rows_total"] >= 0, res["rows_total"].to(torch.float64) * dt, nan)
    res["arrival"] = torch.where(res["arrival_rows"] >= 0, res["arrival_rows"].to(torch.float64) * dt, nan)
    if single:
        res = {k: v[0] for k, v in res.items()}
    return res


def timed_routine(gen, points, scene, waypoints, radius, cell=0.25, margin=0.0, occupancy=None, windows=None, dwell=None,
                  start_heading=None, value=None, budget=None, end=None, before=None, constraints=DEFAULT_CONSTRAINTS, dt=0.01,
                  turn_min=math.radians(1.0), dd=0.005, path_capacity=None, leg_capacity_rows=None, capacity_rows=None,
                  out=None):
    """A routine ordered by the clock and chained, in one call on ``gen``'s device and context: ``travel`` with waypoints,
    ``gen.profile`` and ``gen.time_profile`` of the (P - 1)^2 pairs that can be legs (not the diagonal or column 0, whose
    waypoints are degenerate), ``order_timed`` on their rows with the profile's and the travel's flags as ``leg_flags``,
    the legs and the per-slot dwells gathered in visiting order, and ``timeline.chain(..., n_legs=n_visited)``.

      points         (R, P, 2) or (P, 2): points[.., 0, :] is where the routine starts, the other P - 1 <= 8 are the sites
      scene, waypoints, radius, cell, margin, occupancy, windows   as ``travel`` takes them (``waypoints`` = W per leg)
      dwell, start_heading, value, budget, end, before, constraints, dt, turn_min   as ``order_timed`` takes them
      dd, path_capacity     the legs' profile grid (``gen.profile(dd=, capacity=)``)
      leg_capacity_rows     rows per leg of ``gen.time_profile`` (None: 4096); a leg that needs more is flagged and forbidden
      capacity_rows         rows per routine of the chained timeline, as ``timeline.chain`` takes it; required when ``dwell``
                            is a device tensor
    A pair the travel could not plan (its length is not finite) is profiled along the straight segment instead, so that
    every leg has rows, and is forbidden by its flag; a travel flag that only reports a snapped start or goal forbids
    nothing, as in ``routine``.
    Returns what ``order_timed`` returned, plus timeline (the dict of ``timeline.chain``), legs (R, M, W, 2) the seed routes
    in visiting order (NaN behind the visited slots; ``legs.reshape(R * M, W, 2)`` is what ``refine(seeds=...)`` takes),
    leg_index (R, M) int32 (-1 behind the visited slots), leg_matrix (R, P, P) int32, leg_rows / leg_counts / leg_flags of
    all R (P - 1)^2 profiled pairs, and the travel outputs under travel, travel_flags and waypoints.  Nothing here reads a
    result on the host."""
    from . import timeline
    out = {} if out is None else out
    dev = gen.device
    tr = travel(points, scene, radius, cell=cell, margin=margin, waypoints=waypoints, occupancy=occupancy, windows=windows,
                out=out.setdefault("_travel", {}), device=dev.index, ctx=gen.ctx)
    single = tr["travel"].dim() == 2
    if single:
        tr = {k: v[None] for k, v in tr.items()}
    t, wp = tr["travel"], tr["waypoints"]
    R, P = int(t.shape[0]), int(t.shape[1])
    M, W = P - 1, int(wp.shape[3])
    if M > MAX_TIMED_SITES:
        raise ValueError(f"P = {P} points: 2..{MAX_TIMED_SITES + 1} (the start and at most {MAX_TIMED_SITES} sites)")
    pairs = [(a, b) for a in range(P) for b in range(1, P) if a != b]            # the (P - 1)^2 pairs that can be legs
    pa = torch.tensor([p[0] for p in pairs], device=dev)
    pb = torch.tensor([p[1] for p in pairs], device=dev)
    n_pairs = len(pairs)
    mat = np.full((P, P), -1, dtype=np.int64)
    for k, (a, b) in enumerate(pairs):
        mat[a, b] = k
    mat = torch.as_tensor(mat, device=dev)
    base = torch.arange(R, device=dev)[:, None, None] * n_pairs
    leg_matrix = torch.where(mat[None] >= 0, mat[None] + base, mat[None]).to(torch.int32)
    pts = device_array(points, dev, torch.float64).reshape(R, P, 2)
    host_dwell = None if dwell is None or isinstance(dwell, torch.Tensor) else np.asarray(dwell, dtype=np.float64).reshape(R, P)
    dwell = None if dwell is None else device_array(dwell, dev, torch.float64).reshape(R, P)
    value = None if value is None else device_array(value, dev, torch.float64).reshape(R, P)
    start_heading = None if start_heading is None else device_array(start_heading, dev, torch.float64).reshape(R)
    planned = torch.isfinite(t[:, pa, pb])                                       # (R, n_pairs)
    along = torch.linspace(0.0, 1.0, W, dtype=torch.float64, device=dev)[None, None, :, None]
    straight = pts[:, pa][:, :, None, :] * (1.0 - along) + pts[:, pb][:, :, None, :] * along
    pair_wp = torch.where(planned[:, :, None, None], wp[:, pa, pb], straight)    # (R, n_pairs, W, 2)
    prof = gen.profile(pair_wp.reshape(R * n_pairs, W, 2).to(gen.tdtype).contiguous(), constraints, dd=dd, capacity=path_capacity)
    tp = gen.time_profile(prof, constraints, dt=dt, capacity_rows=leg_capacity_rows, out=out.setdefault("_time", {}))
    failed = torch.where(planned, torch.zeros_like(tr["flags"][:, pa, pb]),
                         tr["flags"][:, pa, pb] | FLAGS["unreachable"])
    leg_flags = prof["flags"] | failed.reshape(R * n_pairs)
    od = order_timed(tp["rows"], tp["counts"], leg_matrix, dwell=dwell, start_heading=start_heading, value=value, budget=budget,
                     end=end, before=before, leg_flags=leg_flags, constraints=constraints, dt=dt, turn_min=turn_min,
                     out=out.setdefault("_order", {}), ctx=gen.ctx)
    o = od["order"].to(torch.int64)
    used = o >= 1
    to = o.clamp(min=0)
    frm = torch.cat([torch.zeros_like(to[:, :1]), to[:, :-1]], dim=1)
    rr = torch.arange(R, device=dev)[:, None]
    leg_index = torch.where(used, leg_matrix[rr, frm, to], torch.full_like(leg_matrix[rr, frm, to], -1))
    slot_dwell = None
    if dwell is not None:
        slot_dwell = torch.where(used, dwell[rr, to], torch.zeros_like(dwell[rr, to]))
        if capacity_rows is None and host_dwell is not None:                      # the longest dwell sum any order can have
            with np.errstate(invalid="ignore"):
                host = host_dwell[:, 1:]
                steps = np.where(host > 0, np.floor(np.where(host > 0, host, 0.0) / dt), 0.0)
            cap_in = int(tp["rows"].shape[1])
            capacity_rows = M * cap_in + M * timeline.turn_rows(math.pi, constraints, dt) + int(min(steps.sum(axis=1).max(), 2.0 ** 31))
    tl = timeline.chain(tp["rows"], tp["counts"], leg_index, dwell=slot_dwell, start_heading=start_heading,
                        n_legs=od["n_visited"], constraints=constraints, dt=dt, turn_min=turn_min, capacity_rows=capacity_rows,
                        out=out.setdefault("_timeline", {}), device=dev.index, ctx=gen.ctx)
    legs = wp[rr, frm, to]
    legs = torch.where(used[:, :, None, None], legs, torch.full_like(legs, float("nan")))
    res = dict(od)
    res.update({"timeline": tl, "legs": legs, "leg_index": leg_index, "leg_matrix": leg_matrix, "leg_rows": tp["rows"],
                "leg_counts": tp["counts"], "leg_flags": leg_flags, "travel": t, "travel_flags": tr["flags"], "waypoints": wp})
    if single:
        res = {k: (v[0] if k in ("order", "n_visited", "rows_total", "arrival_rows", "value_total", "flags", "feasible",
                                 "duration", "arrival", "legs", "leg_index", "leg_matrix", "travel", "travel_flags", "waypoints")
                   else v) for k, v in res.items()}
    out.update(res)
    return res
