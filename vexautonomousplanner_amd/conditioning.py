"""How far a path's velocity recurrence amplifies rounding (vap_velocity_conditioning, include/vap.h).

Every parity figure of this package holds "on the paths tried": the reference's recurrence (MPG:188-311) carries a finite
difference of its own state, and in curves tighter than 2 / track_width a last-bit difference of its inputs grows from step
to step.  ``probe`` measures that growth per path with twin sweeps — the literal recurrence on the rows as they are and on
copies whose curvature and heading differences are changed by a relative +-delta — and returns the conditioning number
``cond``: the largest relative change of a squared velocity divided by 2 delta.  ``cond * ETA`` predicts the relative
velocity difference between this library and the reference on the path; where cond is large the reference's own profile
oscillates from sample to sample.  DESIGN.md section 21 has the definition, the calibration of ETA and the measurements.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._call import buffers, context_for, device_array, ptr
from .synth import DEFAULT_CONSTRAINTS, END_VEL, START_VEL

FLAG_ILLCONDITIONED = 1024
PROBES = (1, 3, 7, 15)
# The input-noise level that turns cond into a predicted relative velocity error: 4 x the largest observed / cond measured
# on the MI355X in fp64 over the calibration sets of DESIGN.md section 21 (cond taken with 7 probes;
# tools/conditioning_calibrate.py).  The ratio spans 1e-16 .. 5.2e-11 over those paths (median 3e-14) and its largest
# value comes from a path whose rows, not whose recurrence, differ from the oracle's: cond * ETA is an upper bound that is
# loose by that width.  The limit it gives for a tolerance of 1e-6, 4.8e3, is below the 1e4 a default has to clear, so no
# default limit is shipped: callers of BatchedTrajectoryGenerator.conditioning name theirs.
ETA = 4 * 5.231713568809064e-11
F32_ROW_NOISE = 2.0 ** -24      # what an fp32 output row adds to the prediction


def limit_for(tol):
    """The cond at which the predicted error cond * ETA reaches ``tol``."""
    return float(tol) / ETA


def probe(meta, curvature, dtheta=None, constraints=DEFAULT_CONSTRAINTS, start_vel=START_VEL, end_vel=END_VEL, samples=None,
          dtype=None, vcap=None, acc_forward=None, acc_backward=None, dec_backward=None, probes=3, delta=2.0 ** -40, seed=0,
          first_path=0, limit=math.inf, per_sample=False, velocity=False, out=None, device=0, ctx=None):
    """Conditioning of B paths' velocity recurrences (vap_velocity_conditioning).

      meta         (B, 4) fp64 device tensor or host array: the profile call's meta (dd in column 2, samples in column 3)
      curvature, dtheta  (B, S) rows, fp64 or fp32 (widened: all arithmetic is fp64) — device tensors (used in place) or
                   host arrays; ``dtheta=None``: the rows the last sampling call left on ``ctx`` (then ``ctx`` is that
                   call's context, and ``curvature`` may be None where the context holds it too; give ``samples`` and
                   ``dtype`` ("f32" | "f64") where no row says them)
      vcap, acc_forward, acc_backward, dec_backward  the limit rows of vap_velocity_pass_limits, optional
      probes       1, 3, 7 or 15 perturbed sweeps beside the unperturbed one; ``delta``: a power of two in [2^-48, 2^-20]
      seed, first_path  path b's sign patterns depend on (seed, first_path + b) only
      limit        paths with cond > limit get FLAG_ILLCONDITIONED in ``flags`` (inf: none)
      per_sample   also return ``sensitivity`` (B, S); ``velocity``: also the unperturbed sweep's velocities (B, S)
      out          optional dict that keeps the call's buffers between calls (``flags`` is zeroed by every call)
    Returns a dict of device tensors: cond (B,) fp64, worst_sample, worst_probe, flags (B,) int32, and the rows asked for.
    Work runs on torch's current stream and is not synchronised."""
    probes = int(probes)
    if probes not in PROBES:
        raise ValueError(f"probes must be one of {PROBES} (got {probes!r})")
    if isinstance(meta, torch.Tensor):
        dev = meta.device
    else:
        dev = ctx_device(ctx, device)
    meta = device_array(meta, dev, torch.float64)
    if meta.dim() != 2 or meta.shape[1] != 4:
        raise ValueError(f"meta must be (B, 4), got {tuple(meta.shape)}")
    B = int(meta.shape[0])
    row = curvature if curvature is not None else dtheta
    if row is not None:
        tdt = row.dtype if isinstance(row, torch.Tensor) else torch.float64
        if tdt not in (torch.float32, torch.float64):
            raise ValueError(f"rows must be fp32 or fp64 (got {tdt})")
        S = int(row.shape[1])
    else:
        if samples is None or dtype is None:
            raise ValueError("without rows, give samples= and dtype= of the call that left them on the context")
        tdt = torch.float64 if dtype in ("f64", "fp64", torch.float64) else torch.float32
        S = int(samples)
    vdt = _lib.VAP_F64 if tdt == torch.float64 else _lib.VAP_F32
    curvature = device_array(curvature, dev, tdt)
    dtheta = device_array(dtheta, dev, tdt)
    for name, r in (("curvature", curvature), ("dtheta", dtheta)):
        if r is not None and tuple(r.shape) != (B, S):
            raise ValueError(f"{name} must be ({B}, {S}), got {tuple(r.shape)}")
    ctx = context_for(dev, ctx)
    L = _lib.lib()
    ldt = torch.float64 if L.vap_limit_rows_dtype(ctx.handle, vdt) == _lib.VAP_F64 else torch.float32
    vcap, acc_forward, acc_backward, dec_backward = (device_array(r, dev, ldt) for r in (vcap, acc_forward, acc_backward, dec_backward))
    shapes = {"cond": ((B,), torch.float64), "worst_sample": ((B,), torch.int32), "worst_probe": ((B,), torch.int32),
              "flags": ((B,), torch.int32)}
    if per_sample:
        shapes["sensitivity"] = ((B, S), torch.float64)
    if velocity:
        shapes["velocity"] = ((B, S), torch.float64)
    res = buffers(out, shapes, dev)
    res["flags"].zero_()
    c = _lib.make_constraints(constraints)
    _lib.check(L.vap_velocity_conditioning(ctx.handle, vdt, B, S, C.byref(c), float(start_vel), float(end_vel), ptr(meta),
                                           ptr(curvature), ptr(dtheta), ptr(vcap), ptr(acc_forward), ptr(acc_backward),
                                           ptr(dec_backward), probes, float(delta), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           int(first_path) & 0xFFFFFFFF, float(limit), ptr(res["cond"]), ptr(res["worst_sample"]),
                                           ptr(res["worst_probe"]), ptr(res["flags"]), ptr(res.get("sensitivity") if per_sample else None),
                                           ptr(res.get("velocity") if velocity else None)), "vap_velocity_conditioning")
    return res


def ctx_device(ctx, device):
    """The device of ``ctx``, or HIP device ``device``."""
    return torch.device("cuda", ctx.device if ctx is not None else device)
