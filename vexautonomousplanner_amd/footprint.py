"""Robot-footprint clearance of time-domain rows (vap_footprint_clearance, include/vap.h), and robot-to-robot clearance
between two batches of them (vap_footprint_conflicts, ``conflicts`` below), also over a window of start shifts
(vap_conflict_shifts: ``shifts`` and ``earliest_start``).

Which candidate trajectories are drivable: does the robot's body stay on the field and off the field elements at every
row?  The reference only previews the footprint (gui/path.py:764-809 PathWidget.draw_rect: the robot rectangle rotated to
the path direction, robot.width / robot.length in inches from config.yaml, gui/settings_widget.py:101-107); this module
checks it, on the device, for a whole batch of rows from ``BatchedTrajectoryGenerator.time_profile`` / ``insert_waits``.

Frame and pose (all lengths in feet, in the rows' own frame: the GUI's field frame, origin at the field centre, y down
the image): a row's robot sits at (x, y) = columns 6 and 7 with body angle phi = -heading (column 4; the reference writes
heading = -wrap(atan2(dy, dx) - pi * reversed), MPG:555-563, so phi is the direction the robot's front faces).  A body
point v maps to (x, y) + R(phi) v.

Clearance (signed, negative = contact) of a row against the wall (id -1), each convex polygon (ids 0..P-1) and each
circle (ids P..P+C-1) is defined in include/vap.h; a row's clearance is the minimum over them (the smallest id on a tie).
The check is discrete at the rows' dt: motion between rows is not swept; pass ``margin > 0`` for a guard band (one 10 ms
row moves at most max_vel * dt, 0.04 ft at 4 ft/s).
"""
import numpy as np
import torch

from . import _lib
from ._call import buffers, context_for, device_array, dptr, ptr, time_rows

# gui/path.py:366-367: the 2000 px field image spans 12.1090395251 ft
FIELD_FT = 12.1090395251
DEFAULT_FIELD = (-FIELD_FT / 2, -FIELD_FT / 2, FIELD_FT / 2, FIELD_FT / 2)
MAX_VERTICES = 16          # footprint and each polygon
MAX_POLYGONS = 256
MAX_POLYGON_VERTICES = 4096
MAX_CIRCLES = 256
ELEMENT_WALL = -1


def rectangle(width_in, length_in, forward_offset_in=0.0):
    """The robot's rectangle in the body frame, feet, counter-clockwise (4, 2): ``length_in`` runs along body x (the
    robot's front), ``width_in`` along body y, both in inches as in config.yaml's robot.length / robot.width; the
    rectangle's centre sits ``forward_offset_in`` inches ahead of the tracked point.

    The GUI's preview (gui/path.py:787-797) puts ``width`` along the path instead; both default to 18 in there, which
    hides the swap.  This helper follows the names: length is front to back."""
    w, l, o = float(width_in) / 12.0, float(length_in) / 12.0, float(forward_offset_in) / 12.0
    if not (w > 0 and l > 0) or not np.isfinite([w, l, o]).all():
        raise ValueError(f"robot width and length must be positive and finite (got {width_in!r}, {length_in!r})")
    return np.array([[o - l / 2, -w / 2], [o + l / 2, -w / 2], [o + l / 2, w / 2], [o - l / 2, w / 2]], dtype=np.float64)


def convex_polygon(vertices, what="polygon"):
    """``vertices`` (n, 2) as a convex, counter-clockwise fp64 array: a clockwise polygon is reversed; collinear or
    duplicate vertices, a non-convex or self-intersecting outline, fewer than 3 or more than 16 vertices raise
    ValueError (the checks of vap_footprint_clearance, which rejects clockwise input itself)."""
    v = np.array(vertices, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 2:
        raise ValueError(f"{what}: vertices must be (n, 2), got {v.shape}")
    n = v.shape[0]
    if n < 3 or n > MAX_VERTICES:
        raise ValueError(f"{what}: {n} vertices (3..{MAX_VERTICES})")
    if not np.isfinite(v).all():
        raise ValueError(f"{what}: non-finite vertex")
    area2 = float(np.sum(v[:, 0] * np.roll(v[:, 1], -1) - np.roll(v[:, 0], -1) * v[:, 1]))
    if area2 < 0:
        v = v[::-1].copy()
    e1 = np.roll(v, -1, axis=0) - v
    e2 = np.roll(e1, -1, axis=0)
    l1, l2 = np.hypot(e1[:, 0], e1[:, 1]), np.hypot(e2[:, 0], e2[:, 1])
    if (l1 == 0).any():
        raise ValueError(f"{what}: duplicate vertex")
    cr = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    if (np.abs(cr) <= 1e-12 * l1 * l2).any():
        raise ValueError(f"{what}: collinear vertices")
    if (cr < 0).any():
        raise ValueError(f"{what}: not convex")
    turn = np.sum(np.arctan2(cr, e1[:, 0] * e2[:, 0] + e1[:, 1] * e2[:, 1]))
    if abs(turn - 2 * np.pi) > 1e-6:
        raise ValueError(f"{what}: not a simple polygon (winds {turn / (2 * np.pi):.3f} times)")
    return v


class Scene:
    """The geometry every route of a clearance call is checked against.

      field     (xmin, ymin, xmax, ymax) feet; "default" = the GUI image's extent +-12.1090395251/2 ft
                (gui/path.py:366-367); None = no walls
      polygons  sequence of (n, 2) convex polygons, 3..16 vertices each (clockwise ones are reversed; decompose
                non-convex field elements into convex pieces)
      circles   (C, 3) array-like of (cx, cy, r), r > 0
    Validated here; more than 256 polygons, 4096 polygon vertices or 256 circles raise ValueError."""

    def __init__(self, field="default", polygons=(), circles=()):
        if isinstance(field, str):
            if field != "default":
                raise ValueError(f"field must be 'default', None or (xmin, ymin, xmax, ymax), got {field!r}")
            field = DEFAULT_FIELD
        if field is not None:
            f = np.array(field, dtype=np.float64).reshape(-1)
            if f.shape != (4,) or not np.isfinite(f).all() or not (f[0] < f[2] and f[1] < f[3]):
                raise ValueError(f"field must be a finite, non-empty (xmin, ymin, xmax, ymax), got {field!r}")
            field = f
        self.field = field
        polys = list(polygons)
        if len(polys) > MAX_POLYGONS:
            raise ValueError(f"{len(polys)} polygons: at most {MAX_POLYGONS}")
        self.polygons = [convex_polygon(p, f"polygon {i}") for i, p in enumerate(polys)]
        nv = sum(len(p) for p in self.polygons)
        if nv > MAX_POLYGON_VERTICES:
            raise ValueError(f"{nv} polygon vertices: at most {MAX_POLYGON_VERTICES}")
        c = np.array(circles, dtype=np.float64).reshape(-1, 3) if len(circles) else np.zeros((0, 3))
        if len(c) > MAX_CIRCLES:
            raise ValueError(f"{len(c)} circles: at most {MAX_CIRCLES}")
        if not np.isfinite(c).all():
            raise ValueError("circles must be finite")
        if (c[:, 2] <= 0).any():
            raise ValueError("circle radii must be > 0")
        self.circles = c
        self.poly_start = np.cumsum([0] + [len(p) for p in self.polygons]).astype(np.int32)
        self.poly_xy = (np.concatenate(self.polygons) if self.polygons else np.zeros((0, 2))).astype(np.float64)

    @property
    def n_polygons(self):
        return len(self.polygons)

    @property
    def n_circles(self):
        return len(self.circles)

    def c_args(self):
        """The six scene arguments of the C-ABI as a tuple: field, n_poly, poly_start, poly_xy, n_circle, circles (None for
        no field and for the empty arrays)."""
        return (dptr(self.field), self.n_polygons, self.poly_start.ctypes.data_as(_lib.ip), dptr(self.poly_xy), self.n_circles,
                dptr(self.circles))

    def element_name(self, eid):
        """'wall', 'polygon k' or 'circle k' for an element id."""
        eid = int(eid)
        if eid == ELEMENT_WALL:
            return "wall"
        if 0 <= eid < self.n_polygons:
            return f"polygon {eid}"
        if self.n_polygons <= eid < self.n_polygons + self.n_circles:
            return f"circle {eid - self.n_polygons}"
        raise ValueError(f"no element {eid}")


def clearance(rows, counts, footprint, scene, margin=0.0, per_row=False, out=None, device=0, ctx=None, cull=True):
    """Footprint clearance of a batch of time-domain rows (vap_footprint_clearance).

      rows       (B, capacity, 8) fp64 rows of time_profile / insert_waits — a device tensor (used in place) or a host
                 array (uploaded once); (n, 8) for a single trajectory
      counts     (B, k) int counts of that call (column 0 = rows), or (B,); None for a single trajectory (all n rows)
      footprint  (n, 2) body-frame polygon in feet (e.g. ``rectangle(18, 18)``), +x = the robot's front
      scene      a Scene
      margin     rows with clearance < margin count as below (first_row, n_below, feasible)
      per_row    also return row_clearance (B, capacity), NaN past counts
      out        optional dict of tensors of the shapes below to fill
      ctx        an _lib.Context (default: the device's shared context); cull: VAP_OPT_FOOTPRINT_CULL (outputs are the
                 same either way)
    Returns a dict of (B,) tensors: min_clearance, min_row, min_element, min_time (time of min_row), first_row,
    first_time, n_below, feasible (n_below == 0), and row_clearance if asked.  A route without rows gets NaN / -1 / 0
    (feasible).  Single trajectories give 0-d tensors (row_clearance (n,)).  Work runs on torch's current stream and is
    not synchronised."""
    if not isinstance(scene, Scene):
        raise TypeError("scene must be a footprint.Scene")
    foot = convex_polygon(footprint, "footprint")
    rows, counts, single, dev = time_rows(rows, counts, None, device)
    B, cap = int(rows.shape[0]), int(rows.shape[1])
    shapes = {"min_clearance": ((B,), torch.float64), "min_row": ((B,), torch.int32), "min_element": ((B,), torch.int32),
              "first_row": ((B,), torch.int32), "n_below": ((B,), torch.int32)}
    if per_row:
        shapes["row_clearance"] = ((B, cap), torch.float64)
    res = buffers(out, shapes, dev)
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    _lib.check(ctx._L.vap_footprint_clearance(
        ctx.handle, B, cap, ptr(rows), ptr(counts), int(counts.shape[1]), len(foot), dptr(foot),
        *scene.c_args(), float(margin), ptr(res.get("row_clearance") if per_row else None), ptr(res["min_clearance"]),
        ptr(res["min_row"]), ptr(res["min_element"]), ptr(res["first_row"]), ptr(res["n_below"])), "vap_footprint_clearance")
    res["feasible"] = res["n_below"] == 0
    res["min_time"] = _time_at(rows, res["min_row"])
    res["first_time"] = _time_at(rows, res["first_row"])
    if single:
        for k in list(res):
            res[k] = res[k][0]
    return res


def _ccw_polygon(vertices, what):
    """convex_polygon, but a clockwise outline raises like the C-ABI does instead of being reversed: with two robots in a
    call, a silently mirrored vertex order is more likely a mistake than a convention."""
    v = np.array(vertices, dtype=np.float64)
    if v.ndim == 2 and v.shape[1] == 2 and len(v) >= 3 and np.isfinite(v).all():
        if float(np.sum(v[:, 0] * np.roll(v[:, 1], -1) - np.roll(v[:, 0], -1) * v[:, 1])) < 0:
            raise ValueError(f"{what}: vertices must be counter-clockwise")
    return convex_polygon(v, what)


PAIRINGS = {"all": _lib.CONFLICT_ALL_PAIRS, "matched": _lib.CONFLICT_MATCHED}


def _two_footprints(footprint_a, footprint_o, pairing="all", names=("footprint_a", "footprint_o")):
    """Prologue of conflicts, shifts and timeline.schedule, part 1: both polygons (side O's None = side A's), ``pairing``."""
    foot_a = _ccw_polygon(footprint_a, names[0])
    foot_o = foot_a if footprint_o is None else _ccw_polygon(footprint_o, names[1])
    if not isinstance(pairing, str) or pairing not in PAIRINGS:
        raise ValueError(f"pairing must be 'all' or 'matched' (got {pairing!r})")
    return foot_a, foot_o


def _two_sides(rows_a, counts_a, rows_o, counts_o, device, pairing="all", names=("side A", "side O"), batch=None):
    """Part 2, behind the wrapper's own scalars so that the errors keep their order: both sides on one device, the matched
    check, the shapes (Ba, cap_a, Bo, cap_o, P).  ``batch`` names side A's routes where a single trajectory is refused."""
    given = [r.device for r in (rows_a, rows_o) if isinstance(r, torch.Tensor)]
    rows_a, counts_a, single, dev = time_rows(rows_a, counts_a, given[0] if given else None, device, names[0])
    if single and batch:
        raise ValueError(f"rows must be (R, capacity, 8): a batch of {batch}")
    rows_o, counts_o, _, _ = time_rows(rows_o, counts_o, dev, device, names[1])
    Ba, cap_a, Bo, cap_o = int(rows_a.shape[0]), int(rows_a.shape[1]), int(rows_o.shape[0]), int(rows_o.shape[1])
    if pairing == "matched" and Ba != Bo:
        raise ValueError(f"matched pairing needs as many routes on both sides (got {Ba} and {Bo})")
    return rows_a, counts_a, rows_o, counts_o, single, dev, (Ba, cap_a, Bo, cap_o, 1 if pairing == "matched" else Bo)


def conflicts(rows_a, counts_a, footprint_a, rows_o, counts_o, footprint_o=None, margin=0.0, shift_rows=0, pairing="all",
              pairs=False, out=None, device=0, ctx=None, cull=True):
    """Robot-to-robot clearance between two batches of time-domain rows (vap_footprint_conflicts): which of side A's
    candidates get along with the routines of side O ("others", e.g. the alliance partner)?

      rows_a, counts_a   side A as in ``clearance``: (Ba, cap_a, 8) device tensor or host array with (Ba, k) / (Ba,)
                         counts, or a single (n, 8) trajectory with counts None
      footprint_a        (n, 2) body-frame polygon of side A's robot, feet
      rows_o, counts_o   side O, the same conventions; its capacity and count stride may differ.  BOTH SIDES MUST BE ON THE
                         SAME TIME STEP (the dt of time_profile / insert_waits): row r of both is the same instant.  The two
                         sides may be the same tensors (all pairs inside one batch; ignore the diagonal)
      footprint_o        side O's robot; None = the same as side A
      margin             pairs with a clearance < margin somewhere conflict (n_conflicts, first_row, compatible)
      shift_rows         side O starts that many rows later (any sign); a robot that has not started or has finished stays
                         parked at its first / last pose
      pairing            "all": every (a, o), P = Bo; "matched": Ba == Bo, pairs (i, i), P = 1
      pairs              also return pair_clearance, pair_row, pair_first_row, each (Ba, P)
      out, ctx, cull     as in ``clearance``
    Returns a dict of (Ba,) tensors: min_clearance (over the route's pairs and rows), min_other (the smallest o there),
    min_row, min_time (min_row x the rows' time step, read from column 0: the time since side A's start), first_row (the earliest row any pair
    goes below margin, or -1), first_time, n_conflicts, compatible (n_conflicts == 0).  A route without a valid pair
    (no rows on either side) gets NaN / -1 / 0 (compatible).  A single side-A trajectory gives 0-d tensors ((P,) for the
    pair outputs).  Work runs on torch's current stream and is not synchronised."""
    foot_a, foot_o = _two_footprints(footprint_a, footprint_o, pairing)
    shift_rows = int(shift_rows)
    rows_a, counts_a, rows_o, counts_o, single, dev, (Ba, cap_a, Bo, cap_o, P) = _two_sides(rows_a, counts_a, rows_o, counts_o, device, pairing)
    shapes = {"min_clearance": ((Ba,), torch.float64), "min_other": ((Ba,), torch.int32), "min_row": ((Ba,), torch.int32),
              "n_conflicts": ((Ba,), torch.int32), "first_row": ((Ba,), torch.int32)}
    if pairs:
        shapes.update(pair_clearance=((Ba, P), torch.float64), pair_row=((Ba, P), torch.int32),
                      pair_first_row=((Ba, P), torch.int32))
    res = buffers(out, shapes, dev)
    if Bo == 0:                                   # nothing to meet: the C-ABI call is a no-op
        res["min_clearance"].fill_(float("nan"))
        for k in ("min_other", "min_row", "first_row"):
            res[k].fill_(-1)
        res["n_conflicts"].zero_()
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    pp = lambda k: ptr(res[k]) if pairs else None
    _lib.check(ctx._L.vap_footprint_conflicts(
        ctx.handle, PAIRINGS[pairing], shift_rows, float(margin),
        Ba, cap_a, ptr(rows_a), ptr(counts_a), int(counts_a.shape[1]), len(foot_a), dptr(foot_a),
        Bo, cap_o, ptr(rows_o), ptr(counts_o), int(counts_o.shape[1]), len(foot_o), dptr(foot_o),
        pp("pair_clearance"), pp("pair_row"), pp("pair_first_row"), ptr(res["min_clearance"]), ptr(res["min_other"]),
        ptr(res["min_row"]), ptr(res["n_conflicts"]), ptr(res["first_row"])), "vap_footprint_conflicts")
    res["compatible"] = res["n_conflicts"] == 0
    dt = _time_step((rows_a, counts_a), (rows_o, counts_o))
    for k, idx in (("min_time", res["min_row"]), ("first_time", res["first_row"])):
        t = idx.to(torch.float64) * dt
        res[k] = torch.where(idx >= 0, t, torch.full_like(t, float("nan")))
    if single:
        for k in list(res):
            res[k] = res[k][0]
    return res


HOLD_ALL = _lib.HOLD_A_FIRST | _lib.HOLD_A_LAST | _lib.HOLD_O_FIRST | _lib.HOLD_O_LAST
HOLD_CONFLICTS = _lib.HOLD_A_LAST | _lib.HOLD_O_FIRST | _lib.HOLD_O_LAST      # what ``conflicts`` does: 14
SCANS = {"up": 1, "down": -1}


def shifts(rows_a, counts_a, footprint_a, rows_o, counts_o, footprint_o=None, margin=0.0, shift_lo=0, n_shifts=1, shift_step=1,
           base=None, hold=HOLD_CONFLICTS, pairing="all", min_run=1, scan="up", table=False, pairs=False, out=None, device=0,
           ctx=None, cull=True):
    """Robot-to-robot clearance as a function of the start shift (vap_conflict_shifts): ``conflicts`` for a whole window
    of ``shift_rows`` in one pass over rows that are packed once, and the first shift at which a route of side A clears
    every route of side O it is paired with.

      rows_a .. footprint_o, margin, pairing, out, ctx, cull   as in ``conflicts``
      shift_lo, n_shifts, shift_step   window entry k = 0 .. n_shifts - 1 stands for side O starting
                         s = shift_lo + base[a] + k * shift_step rows later (negative: side A starts |s| rows later);
                         n_shifts <= 4096
      base               (Ba,) int, device or host: a per-route offset of the window; None = 0
      hold               which side stays on the field outside its own rows: a mask of _lib.HOLD_A_FIRST (1), HOLD_A_LAST
                         (2), HOLD_O_FIRST (4), HOLD_O_LAST (8).  14 (the default) is ``conflicts``' parking: the table is
                         then its pair_clearance at shift_rows = s, the same numbers.  15 also keeps side A at its first
                         pose while it waits to start
      min_run, scan      "up": ``first`` is the smallest k with k .. k + min_run - 1 inside the window and unblocked (the
                         clearance of every pair >= margin, or NaN); "down": the largest k with k - min_run + 1 .. k so
      table              also return route_table (Ba, n_shifts): the smallest clearance over the route's pairs per shift
      pairs              also return pair_table (Ba, P, n_shifts), pair_first and pair_safe (Ba, P)
    Returns a dict of (Ba,) tensors: first (int32, -1: none), first_shift (int64: the shift s of ``first``; 0 where there is
    none), n_safe (unblocked shifts of the window) and first_time (first_shift x the rows' time step; NaN where there is
    none).  A route without rows gets -1 / 0; one with rows and no valid pair is blocked nowhere.  A single side-A
    trajectory gives 0-d tensors.  Work runs on torch's current stream and is not synchronised."""
    foot_a, foot_o = _two_footprints(footprint_a, footprint_o, pairing)
    if not isinstance(scan, str) or scan not in SCANS:
        raise ValueError(f"scan must be 'up' or 'down' (got {scan!r})")
    shift_lo, n_shifts, shift_step, hold, min_run = int(shift_lo), int(n_shifts), int(shift_step), int(hold), int(min_run)
    rows_a, counts_a, rows_o, counts_o, single, dev, (Ba, cap_a, Bo, cap_o, P) = _two_sides(rows_a, counts_a, rows_o, counts_o, device, pairing)
    if isinstance(base, torch.Tensor) and base.device != dev:
        raise ValueError(f"base is on {base.device}, the rows on {dev}")
    base = device_array(base, dev, torch.int32)
    if base is not None and tuple(base.shape) != (Ba,):
        raise ValueError(f"base must be ({Ba},), got {tuple(base.shape)}")
    n = max(n_shifts, 0)
    shapes = {"first": ((Ba,), torch.int32), "n_safe": ((Ba,), torch.int32)}
    if table:
        shapes["route_table"] = ((Ba, n), torch.float64)
    if pairs:
        shapes.update(pair_table=((Ba, P, n), torch.float64), pair_first=((Ba, P), torch.int32), pair_safe=((Ba, P), torch.int32))
    res = buffers(out, shapes, dev)
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    want = lambda k: ptr(res[k]) if k in shapes else None
    _lib.check(ctx._L.vap_conflict_shifts(
        ctx.handle, PAIRINGS[pairing], hold, float(margin), shift_lo, shift_step, n_shifts, ptr(base), min_run, SCANS[scan],
        Ba, cap_a, ptr(rows_a), ptr(counts_a), int(counts_a.shape[1]), len(foot_a), dptr(foot_a),
        Bo, cap_o, ptr(rows_o), ptr(counts_o), int(counts_o.shape[1]), len(foot_o), dptr(foot_o),
        want("pair_table"), want("pair_first"), want("pair_safe"), want("route_table"), ptr(res["first"]), ptr(res["n_safe"])),
        "vap_conflict_shifts")
    if Bo == 0:                                   # nothing to meet: the C-ABI call is a no-op
        has = counts_a[:, 0] > 0
        k = (0 if scan == "up" else n_shifts - 1) if min_run <= n_shifts else -1
        res["first"].copy_(torch.where(has, k, -1))
        res["n_safe"].copy_(torch.where(has, n_shifts, 0))
        if table:
            res["route_table"].fill_(float("nan"))
    first = res["first"].to(torch.int64)
    s = shift_lo + first * shift_step
    if base is not None:
        s = s + base.to(torch.int64)
    res["first_shift"] = torch.where(first >= 0, s, torch.zeros_like(s))
    t = res["first_shift"].to(torch.float64) * _time_step((rows_a, counts_a), (rows_o, counts_o))
    res["first_time"] = torch.where(first >= 0, t, torch.full_like(t, float("nan")))
    if single:
        for k in list(res):
            res[k] = res[k][0]
    return res


def earliest_start(rows_a, counts_a, footprint_a, rows_o, counts_o, footprint_o=None, margin=0.0, max_delay_rows=256, who="a",
                   min_run=1, pairing="all", device=0, ctx=None, cull=True):
    """How long must one side wait for the two not to meet?  Per route of side A the fewest rows of delay d in
    0 .. max_delay_rows such that d .. d + min_run - 1 all keep every pair of the route at ``margin`` or more (``shifts``
    with hold = 15: whoever waits stands at its first pose, whoever has finished at its last).

      who   "o": side O starts d rows later (shifts 0 .. max_delay_rows, scanned up);
            "a": side A waits d rows at its first pose (shifts -max_delay_rows .. 0, scanned down)
    Returns a dict of (Ba,) tensors: delay_rows (int32, -1 where no such delay exists in the window) and delay_time
    (delay_rows x the rows' time step, NaN where none).  max_delay_rows + 1 <= 4096."""
    if who not in ("a", "o"):
        raise ValueError(f"who must be 'a' or 'o' (got {who!r})")
    D = int(max_delay_rows)
    if D < 0:
        raise ValueError(f"max_delay_rows must be >= 0 (got {max_delay_rows!r})")
    r = shifts(rows_a, counts_a, footprint_a, rows_o, counts_o, footprint_o, margin=margin, shift_lo=0 if who == "o" else -D,
               n_shifts=D + 1, hold=HOLD_ALL, pairing=pairing, min_run=min_run, scan="up" if who == "o" else "down",
               device=device, ctx=ctx, cull=cull)
    first = r["first"]
    delay = first if who == "o" else torch.where(first >= 0, D - first, torch.full_like(first, -1))
    return {"delay_rows": delay, "delay_time": r["first_time"].abs()}


def _time_step(*sides):
    """The rows' time step as a 0-d device tensor, without a host round trip: column 0 of rows 1 and 0 of a route with
    at least two rows (the largest such difference over both sides; they are all dt); NaN when no route has two rows."""
    best = None
    for rows, counts in sides:
        if rows.shape[0] == 0 or rows.shape[1] < 2:
            continue
        d = torch.where(counts[:, 0] >= 2, rows[:, 1, 0] - rows[:, 0, 0], torch.full_like(rows[:, 0, 0], float("-inf"))).max()
        best = d if best is None else torch.maximum(best, d)
    if best is None:
        return torch.tensor(float("nan"), dtype=torch.float64, device=sides[0][0].device)
    return torch.where(torch.isinf(best), torch.full_like(best, float("nan")), best)


def _time_at(rows, idx):
    """rows[b, idx[b], 0], NaN where idx[b] < 0."""
    B, cap = rows.shape[0], rows.shape[1]
    if cap == 0:
        return torch.full((B,), float("nan"), dtype=torch.float64, device=rows.device)
    i = idx.long().clamp(0, cap - 1)
    t = rows[torch.arange(B, device=rows.device), i, 0]
    return torch.where(idx >= 0, t, torch.full_like(t, float("nan")))
