"""Odometry rollouts: the follower steers on a dead-reckoned pose with range resets (vap_odometry_rollouts, include/vap.h).

``tracking.rollouts`` feeds the follower the true pose and ``sensors.readings`` says what a wall-facing distance sensor would
read along given rows.  This module closes the loop.  The RAMSETE follower of ``tracking`` steers on an estimate of the pose;
the estimate is integrated from the wheel speeds and the turn rate through an odometry record (an encoder factor per side, a
gyro scale and drift, a scale and bias of the range sensors); and whenever a sensor's reading agrees with what the estimate
expects of a field wall to within a gate, one coordinate of the estimate is pulled onto the reading.  The answer is "with
these sensors the robot ends within x ft of the goal", per rollout and per route, on the device.

Units: feet, seconds, radians; ``ResetRule`` takes inches and degrees and converts on the host, as ``sensors.Sensor`` does.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._call import buffers, context_for, device_array, dptr, ptr, time_rows
from .footprint import Scene
from .sensors import sensor_rows
from .tracking import MAX_ROLLOUTS, Follower, Pursuit, _records, _single

IDEAL = (1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0)     # enc_left, enc_right, heading_scale, heading_drift, range_scale, range_bias, 0, 0
MAX_SENSORS = _lib.RANGE_MAX_SENSORS
STAT_COLUMNS = ("max_error", "max_cross_track", "max_heading_error", "final_error", "final_heading_error", "max_estimate_error",
                "max_estimate_heading_error", "final_estimate_error")
ROW_COLUMNS = ("max_row", "saturated_rows", "resets_accepted", "resets_rejected")


class ResetRule:
    """vap_reset_rule: when a range reading resets the estimate.

      gate_in            the largest accepted |reading - expected reading|, inches
      max_incidence_deg  the largest accepted angle between the expected beam and the wall's normal, 0..90 degrees
      gain               the share of the difference that is corrected, 0..1 (1: the coordinate is set by the reading)
      every              resets are tried at rows r with r % every == 0, 1..10000
    Inches and degrees are converted here, on the host.  No default here is a measured property of a real robot."""

    def __init__(self, gate_in=3.0, max_incidence_deg=30.0, gain=1.0, every=1):
        self.gate_in, self.max_incidence_deg, self.gain = float(gate_in), float(max_incidence_deg), float(gain)
        if not (math.isfinite(self.gate_in) and self.gate_in >= 0.0):
            raise ValueError(f"gate_in must be >= 0 and finite (got {gate_in!r})")
        if not 0.0 <= self.max_incidence_deg <= 90.0:
            raise ValueError(f"max_incidence_deg must be in [0, 90] (got {max_incidence_deg!r})")
        if not 0.0 <= self.gain <= 1.0:
            raise ValueError(f"gain must be in [0, 1] (got {gain!r})")
        if int(every) != every or not 1 <= int(every) <= 10000:
            raise ValueError(f"every must be 1..10000 (got {every!r})")
        self.every = int(every)

    @property
    def gate(self):
        """The gate in feet."""
        return self.gate_in / 12.0

    @property
    def min_cos(self):
        """The smallest accepted cosine of the incidence angle (90 and 0 degrees give exactly 0 and 1)."""
        m = self.max_incidence_deg
        return 0.0 if m == 90.0 else (1.0 if m == 0.0 else min(1.0, max(0.0, math.cos(math.radians(m)))))

    def as_struct(self):
        return _lib.ResetRuleStruct(self.gate, self.min_cos, self.gain, self.every)

    def __repr__(self):
        return f"ResetRule({self.gate_in!r}, {self.max_incidence_deg!r}, {self.gain!r}, {self.every!r})"


def sample_records(B, K, enc_sigma=0.01, heading_scale_sigma=0.005, drift_sigma=0.002, range_scale_sigma=0.005,
                   range_bias_sigma=0.02, seed=0, device=None):
    """(B, K, 8) fp64 odometry records drawn on the host with ``np.random.default_rng(seed)``: the two encoder factors
    ~ 1 + N(0, enc_sigma), heading_scale ~ 1 + N(0, heading_scale_sigma), range_scale ~ 1 + N(0, range_scale_sigma) (the four
    clipped to >= 0.5), heading_drift ~ N(0, drift_sigma) rad/s, range_bias ~ N(0, range_bias_sigma) ft.  Record 0 of every
    route is the ideal one {1, 1, 1, 0, 1, 0, 0, 0}.  The same arguments give the same array.  ``device``: None returns the
    host array, anything else a tensor on that device.  No default here is a measured property of a real robot: take the
    sigmas from the robot's own logs."""
    B, K = int(B), int(K)
    if B < 0 or not 1 <= K <= MAX_ROLLOUTS:
        raise ValueError(f"B must be >= 0 and K in 1..{MAX_ROLLOUTS} (got {B}, {K})")
    for name, v in (("enc_sigma", enc_sigma), ("heading_scale_sigma", heading_scale_sigma), ("drift_sigma", drift_sigma),
                    ("range_scale_sigma", range_scale_sigma), ("range_bias_sigma", range_bias_sigma)):
        if not (float(v) >= 0 and np.isfinite(float(v))):
            raise ValueError(f"{name} must be >= 0 and finite (got {v!r})")
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, K, 6))
    p = np.zeros((B, K, 8), dtype=np.float64)
    p[..., 0:2] = np.maximum(1.0 + z[..., 0:2] * float(enc_sigma), 0.5)
    p[..., 2] = np.maximum(1.0 + z[..., 2] * float(heading_scale_sigma), 0.5)
    p[..., 3] = z[..., 3] * float(drift_sigma)
    p[..., 4] = np.maximum(1.0 + z[..., 4] * float(range_scale_sigma), 0.5)
    p[..., 5] = z[..., 5] * float(range_bias_sigma)
    p[:, 0] = IDEAL
    if device is None:
        return p
    return torch.as_tensor(p, device=torch.device("cuda", device) if isinstance(device, int) else device)


def _record_shape(a, what):
    shape = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
    if len(shape) not in (2, 3) or shape[-1] != 8:
        raise ValueError(f"{what} must be (B, K, 8) or (K, 8), got {shape}")
    if not 1 <= shape[-2] <= MAX_ROLLOUTS:
        raise ValueError(f"K = {shape[-2]} rollouts per route (1..{MAX_ROLLOUTS})")
    return shape


def rollouts(rows, counts, follower, perturbations, records, sensors=None, scene=None, rule=None, time_step=0.01, executed=False,
             estimates=False, out=None, device=0, ctx=None, cull=True):
    """Tracking rollouts in which the follower steers on a dead-reckoned pose with range resets (vap_odometry_rollouts).

      rows, counts, perturbations, time_step, out   as in ``tracking.rollouts``
      follower       a tracking.Follower (RAMSETE); a tracking.Pursuit raises TypeError
      records        (B, K, 8) odometry records per route, or (K, 8) shared by every route (``sample_records``), with the K of
                     ``perturbations``: rollout k runs under perturbation record k and odometry record k
      sensors        None (pure dead reckoning), or what ``sensors.readings`` takes: 1..8 Sensor objects or (n, 8) rows
      scene, rule    with sensors: the footprint.Scene the true beams are cast through (the estimate's expected reading
                     looks at its field walls only) and the ResetRule
      executed       also return the executed rows, ``rows`` (B * K, capacity + settle_rows, 8) and ``counts`` (B * K, 2),
                     as ``tracking.rollouts`` does
      estimates      also return ``estimate_rows`` (B * K, capacity + settle_rows, 4) = {heading, x, y, mask} of the estimate
                     at every row, bit s of mask set where sensor s reset it; rows past a rollout's count are not written
      cull           as in ``sensors.readings`` (the outputs are the same with culling on and off)
    Returns a dict of tensors: stats (B, K, 8) with views max_error, max_cross_track, max_heading_error, final_error,
    final_heading_error (the true pose against the plan, as ``tracking.rollouts``), max_estimate_error,
    max_estimate_heading_error, final_estimate_error (the estimate against the true pose); stat_rows (B, K, 4) with views
    max_row, saturated_rows, resets_accepted, resets_rejected; per route (B,) worst, mean, worst_rollout, worst_row,
    n_exceeding over max_error.  A route without rows and an invalid record give NaN / -1 / 0.  A single trajectory gives
    (K, ...) and 0-d tensors.  Work runs on torch's current stream and is not synchronised."""
    if isinstance(follower, Pursuit):
        raise TypeError("odometry rollouts take a tracking.Follower (RAMSETE); the pure-pursuit follower is not supported")
    if not isinstance(follower, Follower):
        raise TypeError("follower must be a tracking.Follower")
    follower.validate()
    time_step = float(time_step)
    if not (time_step > 0 and np.isfinite(time_step)):
        raise ValueError(f"time_step must be positive and finite (got {time_step!r})")
    sens, ns = None, 0
    if sensors is not None:
        sens = sensor_rows(sensors)
        ns = int(sens.shape[0])
        if not isinstance(scene, Scene):
            raise TypeError("scene must be a footprint.Scene when sensors are given")
        if not isinstance(rule, ResetRule):
            raise TypeError("rule must be an odometry.ResetRule when sensors are given")
    pshape, rshape = _record_shape(perturbations, "perturbations"), _record_shape(records, "records")
    if pshape[-2] != rshape[-2]:
        raise ValueError(f"perturbations give K = {pshape[-2]} rollouts per route, records K = {rshape[-2]}")
    rows, counts, single, dev = time_rows(rows, counts, None, device)
    B, cap = int(rows.shape[0]), int(rows.shape[1])
    pert, shared, K = _records(perturbations, B, dev)
    odo = device_array(records, dev, torch.float64)
    shared_odo = odo.dim() == 2
    if not shared_odo and odo.shape[0] != B:
        raise ValueError(f"records must be ({B}, K, 8) or (K, 8), got {tuple(odo.shape)}")
    cap_exec = cap + int(follower.settle_rows)
    shapes = {"stats": ((B, K, 8), torch.float64), "stat_rows": ((B, K, 4), torch.int32), "worst": ((B,), torch.float64),
              "mean": ((B,), torch.float64), "worst_rollout": ((B,), torch.int32), "worst_row": ((B,), torch.int32),
              "n_exceeding": ((B,), torch.int32)}
    if executed:
        shapes["rows"] = ((B * K, cap_exec, 8), torch.float64)
        shapes["counts"] = ((B * K, 2), torch.int32)
    if estimates:
        shapes["estimate_rows"] = ((B * K, cap_exec, 4), torch.float64)
    bufs = buffers(out, shapes, dev)       # the call's buffers; the returned dict is built apart from it
    res = {k: bufs[k] for k in shapes}
    ctx = context_for(dev, ctx)
    ctx.set_option(_lib.OPT_FOOTPRINT_CULL, 1 if cull else 0)
    fs = follower.as_struct()
    rs = rule.as_struct() if ns else None
    _lib.check(ctx._L.vap_odometry_rollouts(
        ctx.handle, B, cap, ptr(rows), ptr(counts), int(counts.shape[1]), time_step, C.byref(fs), K, int(shared), ptr(pert),
        int(shared_odo), ptr(odo), ns, dptr(sens), C.byref(rs) if ns else None,
        *(scene.c_args() if ns else (None, 0, None, None, 0, None)),
        ptr(res["stats"]), ptr(res["stat_rows"]), ptr(res["worst"]), ptr(res["mean"]), ptr(res["worst_rollout"]),
        ptr(res["worst_row"]), ptr(res["n_exceeding"]), cap_exec, ptr(res.get("rows")), ptr(res.get("counts")),
        ptr(res.get("estimate_rows"))), "vap_odometry_rollouts")
    for i, name in enumerate(STAT_COLUMNS):
        res[name] = res["stats"][..., i]
    for i, name in enumerate(ROW_COLUMNS):
        res[name] = res["stat_rows"][..., i]
    if single:
        _single(res)
        if "estimate_rows" in res:
            res["estimate_rows"] = bufs["estimate_rows"]
    return res
