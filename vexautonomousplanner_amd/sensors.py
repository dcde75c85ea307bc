"""Range-sensor readings of time-domain rows against the scene (vap_range_readings, include/vap.h).

Every other check of this package takes the robot's pose for known.  On a robot it comes from dead reckoning, and the usual
cure is a wall-facing distance sensor that re-zeroes one coordinate whenever it sees a wall it can trust.  ``readings`` says
what such a sensor would read at every row of a batch of routes, and summarises, per route, where a reset is possible: how
many rows give a valid reading, the first and last of them, and the longest stretch driven blind — per sensor, and for "x
observable" / "y observable" (some sensor valid on a wall that fixes that coordinate).

The beam is a single ray: it has no cone, the robot's own body is not seen, and motion between rows is not swept.  Frame and
pose are footprint.py's: feet, a row's robot at columns 6 and 7 with body angle phi = -heading (column 4), +x of the body
frame the robot's front.
"""
import math

import numpy as np
import torch

from . import _lib
from ._call import buffers, context_for, dptr, ptr, time_rows
from .footprint import Scene, _ccw_polygon, _time_step

VALID, NONE, NEAR, FAR, OBLIQUE, BLOCKED, BAD_POSE = (_lib.RANGE_VALID, _lib.RANGE_NONE, _lib.RANGE_NEAR, _lib.RANGE_FAR,
                                                      _lib.RANGE_OBLIQUE, _lib.RANGE_BLOCKED, _lib.RANGE_BAD_POSE)
STATUS_NAMES = ("valid", "none", "near", "far", "oblique", "blocked", "bad_pose")
MAX_SENSORS = _lib.RANGE_MAX_SENSORS
MAX_PARTNERS = _lib.RANGE_MAX_PARTNERS
ELEMENT_NONE, ELEMENT_WALL = -2, -1
FACE_XMIN, FACE_YMIN, FACE_XMAX, FACE_YMAX = 0, 1, 2, 3
CHANNEL_COLUMNS = ("n_ok", "first_ok", "last_ok", "gap_rows", "gap_row")
_CARDINAL = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}


class Sensor:
    """One distance sensor on the robot.

      x_in, y_in         the mount point in the body frame, inches (+x = the robot's front)
      direction_deg      the beam's direction in the body frame, degrees from +x towards +y; 0 / 90 / 180 / 270 (mod 360)
                         give exact unit vectors
      range_in           (r_min, r_max) inches: a reading outside this window is not valid
      max_incidence_deg  the largest accepted angle between the beam and the surface normal, 0..90 degrees
    Inches and degrees are converted here, on the host.  No default here is a measured property of a real sensor: take the
    window and the incidence limit from the data sheet or from a bench test of the part that is on the robot."""

    def __init__(self, x_in, y_in, direction_deg, range_in=(0.0, 78.0), max_incidence_deg=90.0):
        self.x_in, self.y_in, self.direction_deg = float(x_in), float(y_in), float(direction_deg)
        r = tuple(float(v) for v in range_in)
        if len(r) != 2:
            raise ValueError(f"range_in must be (r_min, r_max), got {range_in!r}")
        self.range_in = r
        self.max_incidence_deg = float(max_incidence_deg)
        if not all(math.isfinite(v) for v in (self.x_in, self.y_in, self.direction_deg, *r, self.max_incidence_deg)):
            raise ValueError("sensor parameters must be finite")
        if not 0.0 <= r[0] <= r[1]:
            raise ValueError(f"range_in must satisfy 0 <= r_min <= r_max, got {range_in!r}")
        if not 0.0 <= self.max_incidence_deg <= 90.0:
            raise ValueError(f"max_incidence_deg must be in [0, 90], got {max_incidence_deg!r}")

    def row(self):
        """The sensor as vap_range_readings takes it: (8,) fp64 {mx, my, ux, uy, r_min, r_max, min_cos, 0}, feet."""
        d = self.direction_deg % 360.0
        if d in _CARDINAL:
            ux, uy = _CARDINAL[d]
        else:
            a = math.radians(d)
            ux, uy = math.cos(a), math.sin(a)
            h = math.hypot(ux, uy)
            ux, uy = ux / h, uy / h
        m = self.max_incidence_deg
        min_cos = 0.0 if m == 90.0 else (1.0 if m == 0.0 else min(1.0, max(0.0, math.cos(math.radians(m)))))
        return np.array([self.x_in / 12.0, self.y_in / 12.0, ux, uy, self.range_in[0] / 12.0, self.range_in[1] / 12.0, min_cos, 0.0],
                        dtype=np.float64)

    def __repr__(self):
        return (f"Sensor({self.x_in!r}, {self.y_in!r}, {self.direction_deg!r}, range_in={self.range_in!r}, "
                f"max_incidence_deg={self.max_incidence_deg!r})")


def sensor_rows(sensors):
    """``sensors`` — a Sensor, a sequence of them, or an (n, 8) array of rows already in the C-ABI's form — as a validated
    (n, 8) fp64 array.  The checks are vap_range_readings' own."""
    if isinstance(sensors, Sensor):
        sensors = [sensors]
    if isinstance(sensors, (list, tuple)) and all(isinstance(s, Sensor) for s in sensors):
        a = np.stack([s.row() for s in sensors]) if len(sensors) else np.zeros((0, 8))
    else:
        a = np.array(sensors, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"sensors must be Sensor objects or an (n, 8) array, got shape {a.shape}")
    if not 1 <= a.shape[0] <= MAX_SENSORS:
        raise ValueError(f"{a.shape[0]} sensors (1..{MAX_SENSORS})")
    if not np.isfinite(a).all():
        raise ValueError("sensors: non-finite entry")
    for i, q in enumerate(a):
        if not abs(math.hypot(q[2], q[3]) - 1.0) <= 1e-12:
            raise ValueError(f"sensor {i}: the beam direction ({q[2]!r}, {q[3]!r}) is not a unit vector")
        if not 0.0 <= q[4] <= q[5]:
            raise ValueError(f"sensor {i}: window {q[4]!r} .. {q[5]!r} (0 <= r_min <= r_max)")
        if not 0.0 <= q[6] <= 1.0:
            raise ValueError(f"sensor {i}: min_cos {q[6]!r} outside [0, 1]")
    return np.ascontiguousarray(a)


def unpack(code):
    """A reading's code as (status, face, element): element -1 = the wall, 0.. = polygons, circles, partners in that order,
    -2 = none.  A code of -1 (a row past the route's count) gives (-1, -1, -2).  Works on ints, arrays and tensors."""
    if isinstance(code, torch.Tensor):
        past = code < 0
        neg = torch.full_like(code, -1)
        return (torch.where(past, neg, code & 15), torch.where(past, neg, (code >> 4) & 255),
                torch.where(past, torch.full_like(code, -2), (code >> 12) - 2))
    if isinstance(code, np.ndarray):
        past = code < 0
        return np.where(past, -1, code & 15), np.where(past, -1, (code >> 4) & 255), np.where(past, -2, (code >> 12) - 2)
    code = int(code)
    if code < 0:
        return -1, -1, -2
    return code & 15, (code >> 4) & 255, (code >> 12) - 2


def pack(status, face, element):
    """The code of (status, face, element): what ``unpack`` takes apart."""
    return int(status) | (int(face) << 4) | ((int(element) + 2) << 12)


def readings(rows, counts, sensors, scene, others=None, others_counts=None, others_footprint=None, shift_rows=0, per_row=False,
             out=None, device=0, ctx=None, cull=True):
    """What range sensors read along a batch of time-domain rows (vap_range_readings).

      rows, counts       (B, capacity, 8) fp64 rows of time_profile / insert_waits / routine_timeline / the rollouts' executed
                         rows with their counts, as in footprint.clearance: a device tensor (used in place) or a host array;
                         (n, 8) with counts None for a single trajectory
      sensors            a Sensor, a sequence of 1..8 of them, or an (n, 8) array of C-ABI sensor rows
      scene              a footprint.Scene
      others, others_counts, others_footprint, shift_rows
                         optional partner routines on the same time step, at most 16: rows, counts and one (n, 2) body-frame
                         footprint (counter-clockwise); every route sees every partner, partner o at row r stands at its own
                         row clamp(r - shift_rows, 0, n_o - 1); a partner without rows is absent
      per_row            also return range, cos_incidence (B, capacity, n_sens) fp64 and code (int32; ``unpack``): NaN / -1
                         past counts
      out, ctx, cull     as in footprint.clearance (outputs are the same with culling on and off)
    Returns a dict of device tensors: status_counts (B, n_sens, 8) int32 (rows per status 0..6), range_min, range_max
    (B, n_sens) fp64 over the valid readings (NaN: none), channels (B, n_sens + 2, 5) int32 = CHANNEL_COLUMNS — channel s: sensor
    s valid; n_sens: x observable; n_sens + 1: y observable — and gap_time, first_time, last_time (B, n_sens + 2) fp64:
    gap_rows, first_ok, last_ok times the rows' own time step (NaN where the row is -1 or no route has two rows).  A route
    without rows gets 0 / NaN / (0, -1, -1, 0, -1).  A single trajectory drops the batch axis.  Work runs on torch's current
    stream and is not synchronised."""
    if not isinstance(scene, Scene):
        raise TypeError("scene must be a footprint.Scene")
    sens = sensor_rows(sensors)
    ns = int(sens.shape[0])
    shift_rows = int(shift_rows)
    given = [r.device for r in (rows, others) if isinstance(r, torch.Tensor)]
    rows, counts, single, dev = time_rows(rows, counts, given[0] if given else None, device)
    B, cap = int(rows.shape[0]), int(rows.shape[1])
    foot_o, Bo, cap_o = None, 0, 0
    if others is not None:
        if others_footprint is None:
            raise ValueError("others_footprint is needed with others")
        foot_o = _ccw_polygon(others_footprint, "others_footprint")
        others, others_counts, _, _ = time_rows(others, others_counts, dev, device, "others")
        Bo, cap_o = int(others.shape[0]), int(others.shape[1])
        if Bo > MAX_PARTNERS:
            raise ValueError(f"{Bo} partners: at most {MAX_PARTNERS}")
    shapes = {"status_counts": ((B, ns, 8), torch.int32), "range_minmax": ((B, ns, 2), torch.float64),
              "channels": ((B, ns + 2, 5), torch.int32)}
    if per_row:
        shapes.update(range=((B, cap, ns), torch.float64), cos_incidence=((B, cap, ns), torch.float64),
                      code=((B, cap, ns), torch.int32))
    res = buffers(out, shapes, dev)
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    want = lambda k: ptr(res[k]) if per_row else None
    none = Bo == 0 or cap_o == 0
    _lib.check(ctx._L.vap_range_readings(
        ctx.handle, B, cap, ptr(rows), ptr(counts), int(counts.shape[1]), ns, dptr(sens),
        *scene.c_args(), 0 if none else Bo, 0 if none else cap_o, None if none else ptr(others), None if none else ptr(others_counts),
        1 if none else int(others_counts.shape[1]), 0 if none else len(foot_o), None if none else dptr(foot_o), shift_rows,
        want("range"), want("cos_incidence"), want("code"), ptr(res["status_counts"]), ptr(res["range_minmax"]),
        ptr(res["channels"])), "vap_range_readings")
    res["range_min"], res["range_max"] = res["range_minmax"][..., 0], res["range_minmax"][..., 1]
    dt = _time_step((rows, counts)) if none else _time_step((rows, counts), (others, others_counts))
    ch = res["channels"]
    nan = torch.full((B, ns + 2), float("nan"), dtype=torch.float64, device=dev)
    res["gap_time"] = ch[..., 3].to(torch.float64) * dt
    res["first_time"] = torch.where(ch[..., 1] >= 0, ch[..., 1].to(torch.float64) * dt, nan)
    res["last_time"] = torch.where(ch[..., 2] >= 0, ch[..., 2].to(torch.float64) * dt, nan)
    if single:
        for k in list(res):
            res[k] = res[k][0]
    return res
