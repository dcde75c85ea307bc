"""Can the drivetrain do this?  Curve caps for the velocity pass (vap_curve_caps) and the drive audit of time-domain rows
(vap_drive_audit), include/vap.h.

The reference's Constraints carry ``friction_coef`` and ``max_jerk`` and its forward_backward_pass reads neither; it also
computes the wheel speeds (MPG:594-599) and wheel accelerations (MPG:612-616) of every time-domain row and drops them.
``CurveCaps`` turns the friction coefficient into a lateral-acceleration cap of the velocity pass (and offers the
reference's dormant curvature-rate cap, MPG:41-50 on MPG:178-186); ``audit`` reports, per route, the peak wheel speed, wheel
acceleration, jerk, lateral acceleration v * omega and angular acceleration, the first row of each peak and the rows above a
limit.  Jerk is reported, not limited.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._call import buffers, context_for, device_array, ptr, time_rows
from .synth import DEFAULT_CONSTRAINTS

G_FT = 32.174           # standard gravity, ft/s^2
QUANTITIES = ("wheel_speed", "wheel_acc", "jerk", "lateral_acc", "angular_acc")      # the columns of every audit output
WHEEL_COLUMNS = ("wheel_left", "wheel_right", "wheel_acc_left", "wheel_acc_right", "acc", "jerk", "lateral_acc", "angular_acc")
STATUS_NONFINITE = 2    # d_route_status bit 1: a non-finite v or omega among the route's rows


def _c(constraints, name):
    c = _lib.make_constraints(constraints)
    return float(getattr(c, name))


class CurveCaps:
    """vap_curve_limits: the lateral-acceleration cap (ft/s^2) and the curvature-rate cap (rad/s^2) of ``apply_curve_caps``;
    +inf switches either off."""

    def __init__(self, lateral_acc_max=math.inf, angular_acc_max=math.inf):
        self.lateral_acc_max = float(lateral_acc_max)
        self.angular_acc_max = float(angular_acc_max)

    @classmethod
    def from_constraints(cls, c, g=G_FT, lateral=True, angular=False):
        """lateral: friction_coef * g; angular: the reference's max_angular_accel = 2 * max_acc / track_width (MPG:82)."""
        return cls(_c(c, "friction_coef") * float(g) if lateral else math.inf,
                   2.0 * _c(c, "max_acc") / _c(c, "track_width") if angular else math.inf)

    def validate(self):
        for name in ("lateral_acc_max", "angular_acc_max"):
            v = getattr(self, name)
            if not v > 0.0:
                raise ValueError(f"CurveCaps.{name} must be positive (inf: off), got {v!r}")
        return self

    def as_struct(self):
        self.validate()
        return _lib.CurveLimitsStruct(self.lateral_acc_max, self.angular_acc_max)

    def __repr__(self):
        return f"CurveCaps(lateral_acc_max={self.lateral_acc_max!r}, angular_acc_max={self.angular_acc_max!r})"


class Limits:
    """vap_drive_limits: the track width (feet) and the five limits of ``audit`` in the order of QUANTITIES; inf = never
    exceeded."""

    def __init__(self, track_width, wheel_speed_max=math.inf, wheel_acc_max=math.inf, jerk_max=math.inf,
                 lateral_acc_max=math.inf, angular_acc_max=math.inf):
        self.track_width = float(track_width)
        self.wheel_speed_max = float(wheel_speed_max)
        self.wheel_acc_max = float(wheel_acc_max)
        self.jerk_max = float(jerk_max)
        self.lateral_acc_max = float(lateral_acc_max)
        self.angular_acc_max = float(angular_acc_max)

    @classmethod
    def from_constraints(cls, c, g=G_FT):
        """wheel speed: max_vel, wheel acceleration: max_acc, jerk: max_jerk, lateral: friction_coef * g, angular:
        2 * max_acc / track_width (MPG:82)."""
        tw = _c(c, "track_width")
        return cls(tw, _c(c, "max_vel"), _c(c, "max_acc"), _c(c, "max_jerk"), _c(c, "friction_coef") * float(g),
                   2.0 * _c(c, "max_acc") / tw)

    def validate(self):
        if not (self.track_width > 0.0 and math.isfinite(self.track_width)):
            raise ValueError(f"Limits.track_width must be positive and finite, got {self.track_width!r}")
        for name in ("wheel_speed_max", "wheel_acc_max", "jerk_max", "lateral_acc_max", "angular_acc_max"):
            v = getattr(self, name)
            if not v >= 0.0:
                raise ValueError(f"Limits.{name} must be >= 0 (inf: never exceeded), got {v!r}")
        return self

    def as_struct(self):
        self.validate()
        return _lib.DriveLimitsStruct(self.track_width, self.wheel_speed_max, self.wheel_acc_max, self.jerk_max,
                                      self.lateral_acc_max, self.angular_acc_max)


def curve_caps(meta, curvature, caps, constraints=DEFAULT_CONSTRAINTS, samples=None, dtype=None, vcap_in=None, vcap_out=None,
               n_bound=None, device=0, ctx=None):
    """The cap row of B paths (vap_curve_caps): per sample min(incoming cap, sqrt(A / |curvature|), curvature-rate cap).

      meta       (B, 4) fp64 device tensor or host array: the profile call's meta (dd in column 2, samples in column 3)
      curvature  (B, S) fp32 or fp64 rows — a device tensor (used in place) or a host array; None: the fp64 rows the last
                 sampling call left on ``ctx`` (dtype "f32" with the fp64 recurrence only; give ``samples`` and ``dtype``)
      caps       a CurveCaps; constraints: max_vel is the incoming cap where ``vcap_in`` is None and the rate cap's ceiling
      vcap_in    (B, S) incoming row of the context's limit-row type (fp64 unless the all-fp32 recurrence is on), e.g.
                 ``apply_node_limits(...)["vcap"]``; ``vcap_out``: the tensor to fill (it may be ``vcap_in``: in place)
      n_bound    (B, 2) int32 tensor to fill, optional
    Returns (vcap_out, n_bound) — what ``vap_velocity_pass_limits`` takes as d_vcap, and the samples at which the lateral /
    the curvature-rate cap lies below the incoming row.  Work runs on torch's current stream and is not synchronised."""
    if not isinstance(caps, CurveCaps):
        raise TypeError("caps must be a drive.CurveCaps")
    cs = caps.as_struct()
    dev = meta.device if isinstance(meta, torch.Tensor) else torch.device("cuda", ctx.device if ctx is not None else device)
    meta = device_array(meta, dev, torch.float64)
    if meta.dim() != 2 or meta.shape[1] != 4:
        raise ValueError(f"meta must be (B, 4), got {tuple(meta.shape)}")
    B = int(meta.shape[0])
    if curvature is not None:
        tdt = curvature.dtype if isinstance(curvature, torch.Tensor) else torch.float64
        if tdt not in (torch.float32, torch.float64):
            raise ValueError(f"curvature must be fp32 or fp64 (got {tdt})")
        curvature = curvature if isinstance(curvature, torch.Tensor) and curvature.device == dev else device_array(curvature, dev, tdt)
        S = int(curvature.shape[1])
        if tuple(curvature.shape) != (B, S) or curvature.stride() != (S, 1):
            raise ValueError(f"curvature must be a contiguous ({B}, S) row block, got {tuple(curvature.shape)}")
    else:
        if samples is None or dtype is None:
            raise ValueError("without a curvature row, give samples= and dtype= of the call that left the rows on the context")
        tdt = torch.float64 if dtype in ("f64", "fp64", torch.float64) else torch.float32
        S = int(samples)
    vdt = _lib.VAP_F64 if tdt == torch.float64 else _lib.VAP_F32
    ctx = context_for(dev, ctx)
    L = ctx._L
    ldt = torch.float64 if L.vap_limit_rows_dtype(ctx.handle, vdt) == _lib.VAP_F64 else torch.float32
    for name, r in (("vcap_in", vcap_in), ("vcap_out", vcap_out)):
        if r is not None and (not isinstance(r, torch.Tensor) or tuple(r.shape) != (B, S) or r.dtype != ldt or r.device != dev
                              or r.stride() != (S, 1)):
            raise ValueError(f"{name} must be a contiguous ({B}, {S}) {ldt} tensor on {dev}")
    if vcap_out is None:
        vcap_out = torch.empty((B, S), dtype=ldt, device=dev)
    n_bound = buffers({"n_bound": n_bound}, {"n_bound": ((B, 2), torch.int32)}, dev)["n_bound"]
    c = _lib.make_constraints(constraints)
    _lib.check(L.vap_curve_caps(ctx.handle, vdt, B, S, C.byref(c), C.byref(cs), ptr(meta), ptr(curvature), ptr(vcap_in),
                                ptr(vcap_out), ptr(n_bound)), "vap_curve_caps")
    return vcap_out, n_bound


def audit(rows, counts, limits, time_step=None, per_row=False, out=None, device=0, ctx=None):
    """Drive audit of a batch of time-domain rows (vap_drive_audit).

      rows       (B, capacity, 8) fp64 rows of time_profile / insert_waits / routine_timeline / the rollouts' executed
                 rows — a device tensor (used in place) or a host array (uploaded once); (n, 8) for a single trajectory
      counts     (B, k) int counts of that call (column 0 = rows), or (B,); None for a single trajectory (all n rows)
      limits     a Limits
      time_step  the rows' time step; None: column 0 of rows 1 and 0 of a route with two rows (read on the host: the one
                 synchronisation of this call — pass it to stay asynchronous)
      per_row    also return wheel_rows (B, capacity, 8) = WHEEL_COLUMNS; rows at or above a route's count are not written
      out        optional dict of tensors of the shapes below to fill
    Returns a dict of device tensors: peak (B, 5) fp64, peak_row, n_over, first_over (B, 5) int32 in the order of
    QUANTITIES, status (B,) int32 (STATUS_NONFINITE: the route is treated as empty), and wheel_rows if asked.  A route
    without rows gets NaN / -1 / 0.  Single trajectories drop the batch axis.  Work runs on torch's current stream."""
    if not isinstance(limits, Limits):
        raise TypeError("limits must be a drive.Limits")
    lim = limits.as_struct()
    rows, counts, single, dev = time_rows(rows, counts, None, device)
    B, cap = int(rows.shape[0]), int(rows.shape[1])
    if time_step is None:
        from .footprint import _time_step
        time_step = float(_time_step((rows, counts)).item()) if B else 0.01
        if time_step != time_step:
            raise ValueError("no route has two rows to read the time step from: pass time_step=")
    shapes = {"peak": ((B, 5), torch.float64), "peak_row": ((B, 5), torch.int32), "n_over": ((B, 5), torch.int32),
              "first_over": ((B, 5), torch.int32), "status": ((B,), torch.int32)}
    if per_row:
        shapes["wheel_rows"] = ((B, cap, 8), torch.float64)
    res = buffers(out, shapes, dev)
    ctx = context_for(dev, ctx)
    _lib.check(ctx._L.vap_drive_audit(ctx.handle, B, cap, ptr(rows), ptr(counts), int(counts.shape[1]), float(time_step), C.byref(lim),
                                      ptr(res["peak"]), ptr(res["peak_row"]), ptr(res["n_over"]), ptr(res["first_over"]),
                                      ptr(res["status"]), ptr(res["wheel_rows"]) if per_row else None), "vap_drive_audit")
    if single:
        res = dict(res)
        for k in shapes:
            res[k] = res[k][0]
    return res
