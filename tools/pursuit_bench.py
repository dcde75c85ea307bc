#!/usr/bin/env python3
"""Pure-pursuit rollout timings (vap_pursuit_rollouts) beside the RAMSETE call's (vap_tracking_rollouts), in one process
on the same rows.

Config 3's batch (4096 paths x 32 waypoints, 10000 samples) through profile -> time_profile (~5.2 M rows), rolled under
K = 16 and K = 64 perturbation records per route (sample_perturbations' defaults, tau = 50 ms), statistics only and with
the executed rows.  Both followers take their defaults (2 substeps; RAMSETE 50 settle rows, pursuit 150), and, so that
the two run the same number of steps, pursuit is also timed with 50 settle rows.  The calls of the two followers are
interleaved, repetition by repetition; per configuration and follower: the median of device-event-timed single calls
(*_call_ms) and the mean of back-to-back calls (*_ms), and pursuit's time over RAMSETE's.  Outputs of the repeated calls
are compared bit for bit.  A configuration whose buffers do not fit is named in "not_measured" and on stderr.

``--benign`` replaces config 3's random walks, on whose sharp turns some rollouts lose the path, by as many smooth
synthetic drives of 1280 rows (v = 2 ft/s and omega = 0 plus three sines each, integrated row by row), which both
followers follow.

    python tools/pursuit_bench.py [--reps 10] [--json out.json] [--rollouts 16,64] [--benign]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def benign_rows(torch, device, B, n, dt=0.01):
    """Smooth drives in the time-profile layout: v(t) = 2 + three sines of amplitude <= 0.5 ft/s, omega(t) three sines of
    amplitude <= 0.8 rad/s, integrated row by row from the origin; a seeded device generator, so every run has the same rows."""
    g = torch.Generator(device=device).manual_seed(1)
    t = torch.arange(n, dtype=torch.float64, device=device) * dt

    def U(lo, hi):
        return lo + (hi - lo) * torch.rand(B, 1, dtype=torch.float64, device=device, generator=g)

    v = 2.0 + sum(U(0, 0.5) * torch.sin(U(0.5, 4) * t + U(0, 6)) for _ in range(3))
    w = sum(U(0, 0.8) * torch.sin(U(0.5, 5) * t + U(0, 6)) for _ in range(3))
    phi = torch.cumsum(w * dt, dim=1) - w * dt
    rows = torch.zeros((B, n, 8), dtype=torch.float64, device=device)
    rows[:, :, 0], rows[:, :, 2], rows[:, :, 4], rows[:, :, 5] = t, v, -phi, -w
    rows[:, :, 1] = torch.cumsum(v * dt, dim=1) - v * dt
    rows[:, :, 6] = torch.cumsum(v * dt * torch.cos(phi), dim=1)
    rows[:, :, 7] = torch.cumsum(v * dt * torch.sin(phi), dim=1)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=device)
    counts[:, 0] = n
    return {"rows": rows, "counts": counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rollouts", default="16,64")
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--benign", action="store_true")
    a = ap.parse_args()
    import torch
    from vexautonomousplanner_amd import tracking
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "pursuit_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    B = a.paths
    if a.benign:
        tp = benign_rows(torch, gen.device, B, 1280)
    else:
        wp = torch.tensor(make_waypoints(B, 32, 3), device=gen.device)
        res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
        tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    torch.cuda.synchronize()
    followers = {"ramsete": tracking.Follower(), "pursuit": tracking.Pursuit(), "pursuit_settle50": tracking.Pursuit(settle_rows=50)}
    counts = tp["counts"][:, 0]
    out = {"batch": "benign" if a.benign else "config 3", "routes": B, "rows": int(counts.sum().item()), "capacity": int(tp["rows"].shape[1]),
           "settle_rows": {k: f.settle_rows for k, f in followers.items()}, "lookahead": followers["pursuit"].lookahead}

    def timed(f, P, executed, bufs, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            r = gen.tracking_rollouts(tp, f, P, executed=executed, out=bufs)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n, r

    for K in [int(k) for k in a.rollouts.split(",")]:
        P = torch.tensor(tracking.sample_perturbations(B, K, seed=1), device=gen.device)
        for executed in (False, True):
            key = f"k{K}{'_executed' if executed else ''}"
            bufs, first = {}, {}
            try:
                for name, f in followers.items():                 # warm up; the followers' buffers of one name share a shape
                    bufs[name] = {}
                    for _ in range(2):
                        r = gen.tracking_rollouts(tp, f, P, executed=executed, out=bufs[name])
                    first[name] = r["stats"].clone()
                torch.cuda.synchronize()
            except torch.OutOfMemoryError:
                out.setdefault("not_measured", []).append(key)
                print(f"{key}: NOT MEASURED, the buffers of the executed rows did not fit on the device", file=sys.stderr)
                bufs = first = None
                torch.cuda.empty_cache()
                continue
            single = {name: [] for name in followers}
            for _ in range(a.reps):                               # interleaved: the same noise for every follower
                for name, f in followers.items():
                    single[name].append(timed(f, P, executed, bufs[name], 1)[0])
            for name, f in followers.items():
                ms, r = timed(f, P, executed, bufs[name], a.reps)
                assert torch.equal(first[name].view(torch.int64), r["stats"].view(torch.int64)), f"{key} {name}: outputs differ between calls"
                steps = int((counts + f.settle_rows).sum().item()) * K
                out[f"{key}_{name}_ms"] = ms
                out[f"{key}_{name}_call_ms"] = float(np.median(single[name]))
                out[f"{key}_{name}_call_ms_min_max"] = [float(np.min(single[name])), float(np.max(single[name]))]
                out[f"{key}_{name}_rollout_steps"] = steps
                out[f"{key}_{name}_rollout_steps_per_s"] = steps / (ms * 1e-3)
                if not executed:
                    out[f"k{K}_{name}_worst_ft"] = float(r["worst"].max().item())
                    out[f"k{K}_{name}_routes_exceeding"] = int((r["n_exceeding"] > 0).sum().item())
                    if name != "ramsete":
                        out[f"k{K}_{name}_routes_unfinished"] = int((r["n_unfinished"] > 0).sum().item())
                del r
            for name in ("pursuit", "pursuit_settle50"):
                out[f"{key}_{name}_over_ramsete"] = out[f"{key}_{name}_ms"] / out[f"{key}_ramsete_ms"]
            bufs = first = None
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
