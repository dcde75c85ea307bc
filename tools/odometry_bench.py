#!/usr/bin/env python3
"""Odometry-rollout timings (vap_odometry_rollouts; odometry.py; include/vap.h).

The config-3 batch of tools/range_bench.py — 4096 paths of 32 waypoints, 10 000 samples, their time-domain rows at dt = 0.01 s
with 2048 rows of capacity, every route centred on the field — its scene (walls, 8 convex polygons, 4 circles) and its four
sensors, K = 16 and K = 64 rollouts per route under shared perturbation and odometry records.  Each call is timed with device
events over --reps calls after a warm-up and repeated --rounds times, in this one process (the median is reported, the rounds
are listed).  Per K:

  odometry_ms           odometry.rollouts with the four sensors, resets at every row, no rows written
  odometry_every10_ms   the same with resets at every tenth row
  dead_reckoning_ms     odometry.rollouts without sensors
  tracking_ms           tracking.rollouts alone (vap_tracking_rollouts, no rows written)
  pair_ms               tracking.rollouts(executed=True) + sensors.readings on the B * K executed rows: what the open-loop
                        question "where could the disturbed rollouts reset" costs without this call

    python tools/odometry_bench.py [--reps 5] [--rounds 3] [--ks 16,64] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, W, S, CAP, DT = 4096, 32, 10000, 2048, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ks", default="16,64")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from _timing import timed
    from footprint_bench import field_scene
    from vexautonomousplanner_amd import odometry, sensors, tracking
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "odometry_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    dev = gen.device
    wp = torch.tensor(make_waypoints(B, W, 3), device=dev)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=S)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, dt=DT, capacity_rows=CAP)
    rows, counts = tp["rows"].clone(), tp["counts"]
    valid = torch.arange(CAP, device=dev)[None, :] < counts[:, :1]
    xy = rows[..., 6:8]
    lo = torch.where(valid[..., None], xy, torch.full_like(xy, float("inf"))).amin(dim=1)
    hi = torch.where(valid[..., None], xy, torch.full_like(xy, -float("inf"))).amax(dim=1)
    rows[..., 6:8] -= ((lo + hi) / 2)[:, None, :]
    scene = field_scene()
    sens = [sensors.Sensor(7.0, 0.0, 0, (1.0, 80.0), 60.0), sensors.Sensor(-7.0, 0.0, 180, (1.0, 80.0), 60.0),
            sensors.Sensor(0.0, 7.0, 90, (1.0, 80.0), 60.0), sensors.Sensor(0.0, -7.0, 270, (1.0, 80.0), 60.0)]
    follower = tracking.Follower()
    out = {"paths": B, "capacity_rows": CAP, "rows": int(counts[:, 0].sum().item()), "sensors": len(sens), "polygons": scene.n_polygons,
           "circles": scene.n_circles, "settle_rows": follower.settle_rows, "reps": a.reps, "rounds": a.rounds}
    for K in (int(k) for k in a.ks.split(",")):
        P = torch.as_tensor(tracking.sample_perturbations(1, K, seed=3)[0], device=dev)
        O = odometry.sample_records(1, K, enc_sigma=0.02, seed=3, device=dev)[0]
        bufs = {k: {} for k in ("o", "o10", "d", "t", "p", "r")}
        kw = dict(time_step=DT, ctx=gen.ctx)
        odo = lambda key, every: odometry.rollouts(rows, counts, follower, P, O, sensors=sens, scene=scene,
                                                   rule=odometry.ResetRule(6.0, 60.0, 0.8, every), out=bufs[key], **kw)
        r = {}
        r["odometry_ms"], r["odometry_rounds_ms"] = timed(lambda: odo("o", 1), a.reps, a.rounds)
        r["odometry_every10_ms"], r["odometry_every10_rounds_ms"] = timed(lambda: odo("o10", 10), a.reps, a.rounds)
        r["dead_reckoning_ms"], r["dead_reckoning_rounds_ms"] = timed(
            lambda: odometry.rollouts(rows, counts, follower, P, O, out=bufs["d"], **kw), a.reps, a.rounds)
        r["tracking_ms"], r["tracking_rounds_ms"] = timed(lambda: tracking.rollouts(rows, counts, follower, P, out=bufs["t"], **kw), a.reps, a.rounds)

        def pair():
            ex = tracking.rollouts(rows, counts, follower, P, executed=True, out=bufs["p"], **kw)
            sensors.readings(ex["rows"], ex["counts"], sens, scene, out=bufs["r"], ctx=gen.ctx)

        r["pair_ms"], r["pair_rounds_ms"] = timed(pair, a.reps, a.rounds)
        r["odometry_over_pair"] = r["odometry_ms"] / r["pair_ms"]
        sr = bufs["o"]["stat_rows"]
        ok = sr[..., 0] >= 0
        r["rollouts"] = int(ok.sum().item())
        r["resets_accepted"], r["resets_rejected"] = int(sr[..., 2][ok].sum().item()), int(sr[..., 3][ok].sum().item())
        r["valid_readings_of_pair"] = int(bufs["r"]["status_counts"][..., 0].sum().item())
        for key, name in (("o", "sensors"), ("d", "dead_reckoning")):
            st = bufs[key]["stats"]
            r[f"median_final_error_{name}_ft"] = float(st[..., 3][ok].median().item())
            r[f"median_final_estimate_error_{name}_ft"] = float(st[..., 7][ok].median().item())
        out[f"K{K}"] = r
        del bufs
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
