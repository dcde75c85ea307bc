#!/usr/bin/env python3
"""Drive-limit timings (vap_curve_caps, vap_drive_audit; drive.py; include/vap.h).

The config-3 batch: 4096 paths of 32 waypoints, 10 000 samples, fp32 rows with the fp64 recurrence; its time-domain rows at
dt = 0.01 s with 2048 rows of capacity (about 5.2 M rows).  Each call is timed with device events over --reps calls after a
warm-up and repeated --rounds times (the median is reported, the rounds are listed):

  curve_caps_ms       vap_curve_caps on the context's fp64 curvature rows into a reused fp64 row (8 bytes read and 8 written
                      per sample, plus the count)
  route_limits_ms     vap_route_limits on the same batch (node max_velocity and stop, no acceleration rows): the call that
                      writes the same kind of row today — what curve_caps_ms is read against
  apply_curve_caps_ms BatchedTrajectoryGenerator.apply_curve_caps end to end: the cap row and the velocity pass on it;
                      velocity_limits_ms: that velocity pass alone
  audit_ms            drive.audit into reused buffers, peaks and counts only; audit_rows_ms: with the per-row columns
  copy_ms             a torch device copy of the rows tensor (64 bytes read and 64 written per row of CAPACITY, not of
                      count): the floor of any pass that reads every row and writes as many bytes
  copy_used_ms        a torch device copy of as many bytes as the audit with per-row columns has to move: 64 read and 64
                      written per existing row
  torch_peaks_ms      the same five peaks written in torch operations on the rows tensor (masked by the counts): the loop the
                      audit replaces.  An audit slower than this is a defect.

    python tools/drive_bench.py [--reps 20] [--rounds 5] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, W, S, CAP, DT = 4096, 32, 10000, 2048, 0.01


def torch_peaks(torch, rows, counts, T, h):
    """max |wheel speed|, |wheel acceleration|, |jerk|, |v omega|, |angular acceleration| per route, in torch operations."""
    v, w = rows[:, :, 2], rows[:, :, 5]
    live = torch.arange(rows.shape[1], device=rows.device)[None, :] < counts[:, :1]
    half = w * T / 2
    wl, wr = v - half, v + half
    z = torch.zeros_like(v[:, :1])
    h = torch.tensor(h, dtype=torch.float64, device=rows.device)       # a tensor: torch turns a division by a Python scalar into a product
    d = lambda a: (a - torch.cat([z, a[:, :-1]], dim=1)) / h
    b = d(v)
    qs = (torch.maximum(wl.abs(), wr.abs()), torch.maximum(d(wl).abs(), d(wr).abs()), d(b).abs(), (v * w).abs(), d(w).abs())
    neg = torch.full_like(v, -1.0)
    return torch.stack([torch.where(live, q, neg).max(dim=1).values for q in qs], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from _timing import timed
    from vexautonomousplanner_amd import _lib, drive
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "drive_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    dev = gen.device
    wp = torch.tensor(make_waypoints(B, W, 3), device=dev)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=S)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, dt=DT, capacity_rows=CAP)      # of the plain velocity rows
    out = {"paths": B, "waypoints": W, "samples": S, "capacity_rows": CAP, "dt": DT, "reps": a.reps, "rounds": a.rounds}
    L, c = _lib.lib(), _lib.make_constraints(DEFAULT_CONSTRAINTS)
    p = lambda t: C.c_void_p(t.data_ptr())

    # ---- the cap row beside vap_route_limits
    caps = drive.CurveCaps(3.0)
    vcap = torch.empty((B, S), dtype=torch.float64, device=dev)
    nb = torch.empty((B, 2), dtype=torch.int32, device=dev)
    cap_call = lambda: drive.curve_caps(res["meta"], None, caps, c, samples=S, dtype="f32", vcap_out=vcap, n_bound=nb, ctx=gen.ctx)
    out["curve_caps_ms"], out["curve_caps_rounds_ms"] = timed(cap_call, a.reps, a.rounds)
    out["curve_caps_gbs"] = 16.0 * B * S / out["curve_caps_ms"] / 1e6
    out["samples_bound"] = int(nb[:, 0].sum().item())
    rng = np.random.default_rng(1)
    d_mv = torch.tensor(np.where(rng.random((B, W)) < 0.3, rng.uniform(1.5, 3.5, (B, W)), 0.0), device=dev)
    stop = rng.random((B, W)) < 0.1
    stop[:, 0] = stop[:, -1] = False
    d_stop = torch.tensor(stop.astype(np.int32), device=dev)
    row2 = torch.empty((B, S), dtype=torch.float64, device=dev)

    def limits_call():
        _lib.check(L.vap_route_limits(gen.ctx.handle, _lib.VAP_F32, B, W, 0, S, None, p(res["meta"]), p(d_mv), None, p(d_stop), None, None,
                                      None, None, C.byref(c), 0.01, p(row2), None, None, None, None, None), "vap_route_limits")
    out["route_limits_ms"], out["route_limits_rounds_ms"] = timed(limits_call, a.reps, a.rounds)

    def vel_call():
        _lib.check(L.vap_velocity_pass_limits(gen.ctx.handle, _lib.VAP_F32, B, S, C.byref(c), 0.01, 0.01, p(res["meta"]), None, None,
                                              p(vcap), None, None, None, p(res["velocity"]), p(res["flags"])), "vap_velocity_pass_limits")
    out["velocity_limits_ms"], out["velocity_limits_rounds_ms"] = timed(vel_call, a.reps, a.rounds)
    out["apply_curve_caps_ms"], out["apply_curve_caps_rounds_ms"] = timed(lambda: gen.apply_curve_caps(res, caps, DEFAULT_CONSTRAINTS),
                                                                         a.reps, a.rounds)

    # ---- the audit beside a copy of its rows and beside torch
    rows, counts = tp["rows"], tp["counts"]
    n_rows = int(counts[:, 0].sum().item())
    out["rows"] = n_rows
    lim = drive.Limits.from_constraints(DEFAULT_CONSTRAINTS)
    lim.lateral_acc_max = 3.0
    buf, buf_rows = {}, {}
    out["audit_ms"], out["audit_rounds_ms"] = timed(lambda: drive.audit(rows, counts, lim, time_step=DT, out=buf, ctx=gen.ctx), a.reps, a.rounds)
    out["audit_rows_ms"], out["audit_rows_rounds_ms"] = timed(
        lambda: drive.audit(rows, counts, lim, time_step=DT, per_row=True, out=buf_rows, ctx=gen.ctx), a.reps, a.rounds)
    out["audit_gbs"] = 64.0 * n_rows / out["audit_ms"] / 1e6
    out["audit_rows_gbs"] = 128.0 * n_rows / out["audit_rows_ms"] / 1e6
    out["rows_over"] = buf["n_over"].sum(dim=0).tolist()
    dst = buf_rows["wheel_rows"]
    out["copy_ms"], out["copy_rounds_ms"] = timed(lambda: dst.copy_(rows), a.reps, a.rounds)
    out["copy_gbs"] = 128.0 * B * CAP / out["copy_ms"] / 1e6
    src = torch.empty(64 * n_rows, dtype=torch.uint8, device=dev)
    dst8 = dst.view(torch.uint8).reshape(-1)[:64 * n_rows]
    out["copy_used_ms"], out["copy_used_rounds_ms"] = timed(lambda: dst8.copy_(src), a.reps, a.rounds)
    T = lim.track_width
    out["torch_peaks_ms"], out["torch_peaks_rounds_ms"] = timed(lambda: torch_peaks(torch, rows, counts, T, DT), max(1, a.reps // 4), a.rounds)
    # the two agree on every route with rows (a route without rows: NaN here, -1 there)
    tpk = torch_peaks(torch, rows, counts, T, DT)
    has = (counts[:, 0] > 0) & (buf["status"] == 0)
    out["torch_agrees"] = bool(torch.equal(tpk[has], buf["peak"][has]))
    out["torch_max_rel_diff"] = float(((tpk[has] - buf["peak"][has]).abs() / buf["peak"][has].clamp(min=1e-300)).max().item())
    out["audit_over_copy_used"] = out["audit_rows_ms"] / out["copy_used_ms"]
    out["torch_over_audit"] = out["torch_peaks_ms"] / out["audit_ms"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
