#!/usr/bin/env python3
"""Tracking-rollout timings (vap_tracking_rollouts; include/vap.h).

Config 3's batch (4096 paths x 32 waypoints, 10000 samples) through profile -> time_profile (~5.2 M rows), rolled with the
default follower (2 substeps, 50 settle rows) under K = 16 and K = 64 perturbation records per route, with the executed
rows off and on.  Per configuration: the median of device-event-timed calls each followed by a synchronise (*_call_ms) and
the mean of back-to-back calls (*_ms); rollout-steps per second; this file's own count of fp64 operations per
rollout-step and what it would take at the MI355X's fp64 vector rate (the issue floor: with -ffp-contract=off nearly
every operation is its own instruction) and its ratio to the call time (*_fp64_issue_floor_over_call_ms: the mean of
back-to-back calls, launch included, not a kernel time); and for the executed rows the bytes written and what they would take at the
HBM rate measured for plain stores.  A configuration whose buffers do not fit is named in "not_measured" and on stderr.
Outputs of the repeated calls are compared bit for bit.

    python tools/tracking_bench.py [--reps 10] [--json out.json] [--rollouts 16,64]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 157.3e12 / 2       # vector fp64, flop/s with every instruction an FMA (2 flop)
FP64_ISSUE = FP64_PEAK / 2     # fp64 vector instructions per second
HBM_STORE = 6.0e12             # B/s, plain stores


def step_flops(n_substeps):
    """fp64 operations of one rollout-step, counted from the header's steps with the device library's routines at their
    usual sizes: sincos ~60 (argument reduction and two polynomials), sin ~40, hypot ~15, sqrt and a division ~10 each,
    the wrap's fmod ~25.  Per step: sincos(phi), the body-frame errors (8), the wrap, hypot, the three maxima (3),
    sincos(e_phi), sinc's division, the gain's sqrt, the control law (20), saturation (5).  Per substep: the two lags (4),
    v and omega (6 + a division), the half angle (2), sincos(phi + u), sin(u), sinc (12), the pose update (8)."""
    per_step = 60 + 8 + 25 + 15 + 3 + 60 + 10 + 10 + 20 + 5
    per_substep = 4 + 6 + 10 + 2 + 60 + 40 + 12 + 8
    return per_step + n_substeps * per_substep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rollouts", default="16,64")
    ap.add_argument("--paths", type=int, default=4096)
    a = ap.parse_args()
    import torch
    from vexautonomousplanner_amd import tracking
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "tracking_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    B = a.paths
    wp = torch.tensor(make_waypoints(B, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    torch.cuda.synchronize()
    follower = tracking.Follower()
    counts = tp["counts"][:, 0]
    n_rows = int(counts.sum().item())
    steps_per_k = int((counts + follower.settle_rows).sum().item())
    flops = step_flops(follower.n_substeps)
    out = {"routes": B, "rows": n_rows, "capacity": int(tp["rows"].shape[1]), "settle_rows": follower.settle_rows,
           "n_substeps": follower.n_substeps, "flop_per_rollout_step": flops}
    for K in [int(k) for k in a.rollouts.split(",")]:
        P = torch.tensor(tracking.sample_perturbations(B, K, seed=1), device=gen.device)
        steps = steps_per_k * K
        for executed in (False, True):
            key = f"k{K}{'_executed' if executed else ''}"
            bufs = {}
            try:
                for _ in range(2):
                    r = gen.tracking_rollouts(tp, follower, P, executed=executed, out=bufs)
                torch.cuda.synchronize()
            except torch.OutOfMemoryError:
                out[key + "_ms"] = None
                out.setdefault("not_measured", []).append(key)
                print(f"{key}: NOT MEASURED, the buffers ({steps * 64 / 1e9:.1f} GB of executed rows) did not fit on the device", file=sys.stderr)
                bufs = None
                torch.cuda.empty_cache()
                continue
            first = r["stats"].clone()
            ts = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = gen.tracking_rollouts(tp, follower, P, executed=executed, out=bufs)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            out[key + "_call_ms"] = float(np.median(ts))
            out[key + "_call_ms_min_max"] = [float(np.min(ts)), float(np.max(ts))]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                r = gen.tracking_rollouts(tp, follower, P, executed=executed, out=bufs)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            out[key + "_ms"] = ms
            assert torch.equal(first.view(torch.int64), r["stats"].view(torch.int64)), f"{key}: outputs differ between calls"
            out[key + "_rollout_steps"] = steps
            out[key + "_rollout_steps_per_s"] = steps / (ms * 1e-3)
            out[key + "_gflop"] = steps * flops / 1e9
            out[key + "_fp64_issue_floor_ms"] = steps * flops / FP64_ISSUE * 1e3
            out[key + "_fp64_issue_floor_over_call_ms"] = steps * flops / FP64_ISSUE / (ms * 1e-3)   # of call time, not kernel time
            if executed:
                out[key + "_bytes_written"] = steps * 64
                out[key + "_store_floor_ms"] = steps * 64 / HBM_STORE * 1e3
            else:
                out[f"k{K}_worst_ft"] = float(r["worst"].max().item())
                out[f"k{K}_mean_of_worst_ft"] = float(r["worst"].mean().item())
                out[f"k{K}_routes_exceeding"] = int((r["n_exceeding"] > 0).sum().item())
            del r
            bufs = None
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
