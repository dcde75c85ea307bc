"""The legs of a routine chained into one timeline, with in-place turns and dwells (vap_routine_timeline, include/vap.h).

``plan.routine`` returns a visiting order and one seed route per leg, ``search.refine`` improves each leg by itself, and
``time_profile`` gives every leg rows that start at its own time zero.  ``chain`` puts them back together: per slot of a
routine the turn on the spot from the heading the robot arrives with to the heading the next leg starts with (the
reference's own turn, MPG:319-346 and 487-507), the leg's rows at their place in time and distance, and the rows of the
dwell at the site.  The result has the rows and counts of ``time_profile``, so it goes where those go: ``footprint.
clearance`` (does the turning robot clear the post beside the site?), ``footprint.conflicts`` (a later leg against the
partner at its real start time), ``tracking.rollouts`` and ``plan.occupancy``.  ``dwell_to_clear`` asks the question a
crossing partner raises: how much longer must the robot stay at the previous site for the rest of the routine to clear it;
``schedule`` asks it for every slot at once: how long to wait in front of each so that the whole routine clears every partner
and ends as early as it can.

Nothing here reads the device: the visiting order may stay a device tensor from ``plan.order`` to the chained rows.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._call import buffers, context_for, device_array, dptr, ptr, time_rows
from .synth import DEFAULT_CONSTRAINTS

MAX_LEGS = _lib.TIMELINE_MAX_LEGS
MAX_DELAYS = _lib.SCHEDULE_MAX_DELAYS
FLAGS = {"truncated": _lib.FLAG_TRUNCATED, "bad_route": _lib.FLAG_BAD_ROUTE}


def turn_rows(angle, constraints=DEFAULT_CONSTRAINTS, dt=0.01):
    """Rows of an in-place turn of ``angle`` radians under ``constraints`` (MPG:319-346 over one_dim_mp_generator.py:4-69):
    the trapezoid's duration / dt + 1, rounded up."""
    c = _lib.make_constraints(constraints)
    arc = abs(float(angle)) * c.track_width / 2
    t_acc = c.max_vel / c.max_acc
    d_acc = 0.5 * c.max_acc * (t_acc * t_acc)
    if 2 * d_acc > arc:
        total = 2 * math.sqrt(arc / c.max_acc)
    else:
        total = 2 * t_acc + (arc - 2 * d_acc) / c.max_vel
    return int(math.ceil((total + dt) / dt))


def chain(rows, counts, legs, dwell=None, start_heading=None, n_legs=None, constraints=DEFAULT_CONSTRAINTS, dt=0.01,
          turn_min=math.radians(1.0), capacity_rows=None, out=None, device=0, ctx=None):
    """Chain legs into routines (vap_routine_timeline): per used slot m of routine r, [turn m] [leg m] [dwell m].

      rows, counts   the L legs as ``time_profile`` returns them: (L, capacity_in, 8) fp64 device tensor (used in place) or
                     host array (uploaded once), with (L, k) / (L,) counts (column 0 = rows).  All on the time step ``dt``
      legs           (R, M) int, device tensor or host array: the leg driven in slot m of routine r, 1 <= M <= 32.  A leg
                     may serve several slots and routines; an index outside [0, L) (the -1 of an infeasible ``plan.order``)
                     makes the routine bad
      dwell          (R, M) seconds spent at the end of slot m, device or host; None = none
      start_heading  (R,) the heading the robot stands at before slot 0 (it turns to leg 0's first heading), NaN = none;
                     None = none
      n_legs         (R,) slots used (the rest is ignored); None = M
      constraints    max_vel, max_acc and track_width shape the turn's trapezoid
      turn_min       a change of heading below this many radians inserts no turn
      capacity_rows  rows per routine in the output; None: M capacity_in + M half turns + the longest routine's dwell rows,
                     which needs ``dwell`` on the host: with a device tensor it must be given
      out            optional dict of tensors of the shapes below to fill (rows, counts, map, seam, flags)
    Returns a dict of device tensors: rows (R, capacity_rows, 8), counts (R, 2) int32 {rows, slots used}, map (R, M, 3)
    int32 (first output row of slot m's turn, leg and dwell block; -1 for an unused slot or a bad routine), seam (R, M, 3)
    (heading left over after the turn; x and y gap between the row in front and the leg's first row), flags (R,) uint32
    (FLAGS: bad_route, truncated), arrival (R, M) seconds at which site m is reached (NaN as map is -1) and duration (R,)
    seconds (NaN for a bad routine).  A truncated routine's rows below capacity_rows are those of an ample call; its map
    is not cut.  Work runs on torch's current stream and is not synchronised."""
    dt, turn_min = float(dt), float(turn_min)
    if not (dt > 0 and math.isfinite(dt)):
        raise ValueError(f"dt must be positive and finite (got {dt!r})")
    if not (turn_min >= 0 and math.isfinite(turn_min)):
        raise ValueError(f"turn_min must be >= 0 and finite (got {turn_min!r})")
    c = _lib.make_constraints(constraints)
    rows, counts, single, dev = time_rows(rows, counts, None, device, "legs")
    if single:
        raise ValueError("rows must be (L, capacity_in, 8): a batch of legs")
    L, cap_in = int(rows.shape[0]), int(rows.shape[1])
    shape = tuple(legs.shape) if hasattr(legs, "shape") else np.shape(legs)
    if len(shape) != 2 or not 1 <= shape[1] <= MAX_LEGS:
        raise ValueError(f"legs must be (R, M) with 1 <= M <= {MAX_LEGS}, got {tuple(shape)}")
    R, M = int(shape[0]), int(shape[1])

    def arg(a, dtype, shape, what):
        if isinstance(a, torch.Tensor) and a.device != dev:
            raise ValueError(f"{what} is on {a.device}, the rows on {dev}")
        t = device_array(a, dev, dtype)
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{what} must be {shape}, got {tuple(t.shape)}")
        return t

    legs = arg(legs, torch.int32, (R, M), "legs")
    dwell_host = None
    if dwell is not None and not isinstance(dwell, torch.Tensor):
        dwell_host = np.ascontiguousarray(dwell, dtype=np.float64)
    dwell = arg(dwell, torch.float64, (R, M), "dwell")
    start_heading = arg(start_heading, torch.float64, (R,), "start_heading")
    n_legs = arg(n_legs, torch.int32, (R,), "n_legs")
    if capacity_rows is None:
        if dwell is not None and dwell_host is None:
            raise ValueError("capacity_rows is required when dwell is a device tensor: its rows cannot be counted "
                             "without reading the device")
        capacity_rows = M * cap_in + M * turn_rows(math.pi, c, dt)
        if dwell_host is not None and dwell_host.size:
            with np.errstate(invalid="ignore"):
                steps = np.where(dwell_host > 0, np.floor(np.where(dwell_host > 0, dwell_host, 0.0) / dt), 0.0)
            capacity_rows += int(min(steps.sum(axis=1).max(), 2.0 ** 31))
    capacity_rows = int(capacity_rows)
    if capacity_rows < 0:
        raise ValueError(f"capacity_rows must be >= 0 (got {capacity_rows})")
    shapes = {"rows": ((R, capacity_rows, 8), torch.float64), "counts": ((R, 2), torch.int32), "map": ((R, M, 3), torch.int32),
              "seam": ((R, M, 3), torch.float64), "flags": ((R,), torch.int32)}
    res = buffers(out, shapes, dev)
    res["flags"].zero_()                          # the call ORs its bits in
    ctx = context_for(dev, ctx)
    _lib.check(ctx._L.vap_routine_timeline(
        ctx.handle, R, M, L, cap_in, capacity_rows, dt, C.byref(c), turn_min, ptr(rows), ptr(counts), int(counts.shape[1]),
        ptr(legs), ptr(n_legs), ptr(dwell), ptr(start_heading), ptr(res["rows"]), ptr(res["counts"]), ptr(res["map"]),
        ptr(res["seam"]), ptr(res["flags"])), "vap_routine_timeline")
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    at = res["map"][:, :, 2]
    res["arrival"] = torch.where(at >= 0, at.to(torch.float64) * dt, nan)
    bad = (res["flags"] & _lib.FLAG_BAD_ROUTE) != 0
    res["duration"] = torch.where(bad, nan, res["counts"][:, 0].to(torch.float64) * dt)
    return res


def dwell_to_clear(tl, slot, footprint, others_rows, others_counts, others_footprint=None, margin=0.0, max_delay_rows=256,
                   min_run=1, device=0, ctx=None):
    """The extra dwell that lets the rest of a routine clear the other robots (``footprint.earliest_start`` on the tails).

      tl             what ``chain`` returned
      slot           0 <= slot < M.  Everything from slot's turn block on, output row b = map[r, slot, 0], is delayed: the
                     dwell goes to slot - 1 (for slot = 0 the routine starts that much later)
      others_rows, others_counts, others_footprint   the other robots' rows on the timeline's clock and time step, as
                     ``footprint.conflicts`` takes its side O; footprint None = the same as ``footprint``
      margin, max_delay_rows, min_run   as in ``footprint.earliest_start``
    Per routine the tail of its own rows from b, waiting at its first pose, is swept against every other robot's rows from
    b on (one that has ended by b stands at its last row).  Returns (R,) seconds: (d + 0.5) dt for the fewest rows d that
    clear every other robot, so that ``chain`` turns it into exactly d rows; NaN where no delay up to max_delay_rows does,
    and for a routine that does not use the slot.  One routine at a time, all on the device: nothing is read on the host."""
    from . import footprint as fp
    rows, counts, at = tl["rows"], tl["counts"], tl["map"]
    R, cap = int(rows.shape[0]), int(rows.shape[1])
    slot = int(slot)
    if not 0 <= slot < int(at.shape[1]):
        raise ValueError(f"slot must be in [0, {int(at.shape[1])}) (got {slot})")
    o_rows, o_counts, _, dev = time_rows(others_rows, others_counts, rows.device, device, "others")
    Bo, cap_o = int(o_rows.shape[0]), int(o_rows.shape[1])
    dt = fp._time_step((rows, counts), (o_rows, o_counts))
    out = torch.full((R,), float("nan"), dtype=torch.float64, device=dev)
    if cap == 0:
        return out
    ar_a = torch.arange(cap, device=dev)
    ar_o = torch.arange(max(cap_o, 1), device=dev)
    n_o = o_counts[:, 0].clamp(0, cap_o).to(torch.int64)
    for r in range(R):
        b = at[r, slot, 0].to(torch.int64)
        used = b >= 0
        b = b.clamp(min=0)
        tail = rows[r].index_select(0, (b + ar_a).clamp(max=cap - 1)).unsqueeze(0)
        n_tail = torch.where(used, (counts[r, 0].to(torch.int64) - b).clamp(min=0), torch.zeros_like(b)).to(torch.int32).reshape(1, 1)
        if Bo and cap_o:
            j = torch.minimum(b + ar_o[None, :], (n_o - 1).clamp(min=0)[:, None])
            o_tail = torch.gather(o_rows, 1, j[:, :, None].expand(Bo, cap_o, 8))
            o_n = torch.where(n_o > 0, (n_o - b).clamp(min=1), torch.zeros_like(n_o)).to(torch.int32)
        else:
            o_tail, o_n = o_rows, o_counts[:, 0]
        e = fp.earliest_start(tail, n_tail, footprint, o_tail, o_n, others_footprint, margin=margin, max_delay_rows=max_delay_rows,
                              who="a", min_run=min_run, device=device, ctx=ctx)
        d = e["delay_rows"][0]
        out[r] = torch.where(d >= 0, (d.to(torch.float64) + 0.5) * dt, torch.full_like(dt, float("nan")))
    return out


def schedule(tl, footprint, others_rows, others_counts, others_footprint=None, margin=0.0, n_delays=256, delay_step=1,
             tables=False, out=None, device=0, ctx=None, cull=True):
    """The rows to wait in front of every slot of a routine so that all of it clears the other robots and it ends as early
    as possible (vap_schedule_tables + vap_schedule_solve; the definitions are in include/vap.h).

      tl             what ``chain`` returned, or a tuple (rows, counts, seg_start): rows and counts as ``footprint.conflicts``
                     takes its side A ((R, cap, 8) with (R, k) / (R,) counts, device or host), seg_start (R, M) int, device or
                     host, 1 <= M <= 32: the first row of segment m, -1 for an unused trailing slot (``tl["map"][:, :, 0]``)
      footprint      (n, 2) body-frame polygon of the routines' robot, counter-clockwise
      others_rows, others_counts, others_footprint   the other robots' rows on the routines' clock and time step, as
                     ``footprint.conflicts`` takes its side O; footprint None = the same as ``footprint``.  Every routine is
                     taken against every one of them
      margin         a clearance < margin blocks
      n_delays, delay_step   the window: cumulative delays of k * delay_step rows, k = 0 .. n_delays - 1 (<= 4096)
      tables         also return move and wait (R, M, n_delays): the clearance of driving segment m at cumulative delay k and
                     of standing in front of it during delay step u
      out            optional dict of tensors to fill (delay_rows, total_rows, clearance, n_seg, flags, move, wait)
    Returns a dict of device tensors: delay_rows (R, M) int32, the rows to wait in front of slot m (0 for unused slots; -1 in
    every slot when the window holds no schedule, or the routine has no rows, no slots or a bad slot list), total_rows (R,)
    their sum or -1, clearance (R,) the smallest clearance the schedule meets (NaN: none), n_seg (R,) slots used, flags (R,)
    (FLAGS: bad_route), start_delay_rows = delay_rows[:, 0], and dwell_add (R, M) seconds: dwell_add[:, m - 1] = (d_m + 0.5) dt
    for d_m = delay_rows[:, m] > 0, else 0 (``dwell_to_clear``'s convention; column M - 1 is 0), so that ``chain`` with
    dwell + dwell_add waits exactly d_m more rows at site m - 1.  THE CALLER'S OWN DWELL MUST BE A WHOLE NUMBER OF ROWS
    (a multiple of dt, or 0) for the sum to stay exact; the wait in front of slot 0 is not a dwell: shift the routine's start
    by start_delay_rows.  Nothing is read on the host; work runs on torch's current stream and is not synchronised."""
    from . import footprint as fp
    foot_a, foot_o = fp._two_footprints(footprint, others_footprint, names=("footprint", "others_footprint"))
    margin, n_delays, delay_step = float(margin), int(n_delays), int(delay_step)
    if not math.isfinite(margin):
        raise ValueError(f"margin must be finite (got {margin!r})")
    if not 1 <= n_delays <= MAX_DELAYS:
        raise ValueError(f"n_delays must be in [1, {MAX_DELAYS}] (got {n_delays})")
    if delay_step < 1 or (n_delays - 1) * delay_step > 2 ** 31 - 1:
        raise ValueError(f"delay_step must be >= 1 and (n_delays - 1) * delay_step below 2^31 (got {delay_step})")
    if isinstance(tl, dict):
        rows, counts, seg_start = tl["rows"], tl["counts"], tl["map"][:, :, 0]
    else:
        try:
            rows, counts, seg_start = tl
        except (TypeError, ValueError):
            raise ValueError("tl must be what chain returned or a tuple (rows, counts, seg_start)") from None
    rows, counts, o_rows, o_counts, _, dev, (R, cap, Bo, cap_o, _) = fp._two_sides(rows, counts, others_rows, others_counts, device,
                                                                                   names=("routines", "others"), batch="routines")
    if isinstance(seg_start, torch.Tensor) and seg_start.device != dev:
        raise ValueError(f"seg_start is on {seg_start.device}, the rows on {dev}")
    seg_start = device_array(seg_start, dev, torch.int32)
    if seg_start is None or seg_start.dim() != 2 or seg_start.shape[0] != R or not 1 <= seg_start.shape[1] <= MAX_LEGS:
        raise ValueError(f"seg_start must be ({R}, M) with 1 <= M <= {MAX_LEGS}, got "
                         f"{None if seg_start is None else tuple(seg_start.shape)}")
    M = int(seg_start.shape[1])
    shapes = {"delay_rows": ((R, M), torch.int32), "total_rows": ((R,), torch.int32), "clearance": ((R,), torch.float64),
              "n_seg": ((R,), torch.int32), "flags": ((R,), torch.int32)}
    res = buffers(out, shapes, dev)
    # the tables are the call's only R x M x n_delays memory; without ``tables`` they live for this call only
    tab = buffers(res if tables else None, {"move": ((R, M, n_delays), torch.float64), "wait": ((R, M, n_delays), torch.float64)}, dev)
    res["flags"].zero_()                          # the call ORs its bit in
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    _lib.check(ctx._L.vap_schedule_tables(
        ctx.handle, n_delays, delay_step, R, cap, ptr(rows), ptr(counts), int(counts.shape[1]), len(foot_a), dptr(foot_a),
        M, ptr(seg_start), Bo, cap_o, ptr(o_rows), ptr(o_counts), int(o_counts.shape[1]), len(foot_o), dptr(foot_o),
        ptr(tab["move"]), ptr(tab["wait"]), ptr(res["n_seg"]), ptr(res["flags"])), "vap_schedule_tables")
    _lib.check(ctx._L.vap_schedule_solve(
        ctx.handle, R, M, n_delays, delay_step, margin, ptr(tab["move"]), ptr(tab["wait"]), ptr(res["n_seg"]),
        ptr(res["delay_rows"]), ptr(res["total_rows"]), ptr(res["clearance"])), "vap_schedule_solve")
    d = res["delay_rows"]
    res["start_delay_rows"] = d[:, 0]
    dt = fp._time_step((rows, counts), (o_rows, o_counts))
    add = torch.zeros((R, M), dtype=torch.float64, device=dev)
    if M > 1:
        later = d[:, 1:]
        add[:, :M - 1] = torch.where(later > 0, (later.to(torch.float64) + 0.5) * dt, torch.zeros_like(add[:, :M - 1]))
    res["dwell_add"] = add
    return res
