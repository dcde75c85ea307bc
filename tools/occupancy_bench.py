#!/usr/bin/env python3
"""Occupancy timings (vap_plan_occupancy, plan.occupancy; include/vap.h).

Config 3's batch (4096 paths x 32 waypoints, 10000 samples) through profile -> time_profile (~5.2 M rows), rasterised
onto the 72 x 72 grid of tools/plan_bench.py (the +-6 ft field at cell = 2 in) for a disc of 0.75 ft wanting 0.05 ft, an
18 x 18 in footprint; all 4096 routes ("where do my candidates go") and the first 8 of them (a partner's routines), with
and without min_clearance.  Config 3's random walks start at (-5, -5) ft and leave the field, so most of their rows cover
nothing; the "centred_" runs move each route so that its extent is centred on the field, as tools/footprint_bench.py does.
Each call is timed with device events over --reps calls after a warm-up and repeated --rounds times (the median is
reported, the rounds are listed).

    python tools/occupancy_bench.py [--reps 20] [--rounds 5] [--json out.json]

The kernel's own time comes from a run under rocprofv3 --kernel-trace --stats (k_occupancy)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELD = (-6.0, -6.0, 6.0, 6.0)
CELL, RADIUS, MARGIN = 1.0 / 6.0, 0.75, 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from _timing import timed
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "occupancy_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    wp = torch.tensor(make_waypoints(4096, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    torch.cuda.synchronize()
    scene, foot = fp.Scene(field=FIELD), fp.rectangle(18, 18)
    rows_c = tp["rows"].clone()
    valid = torch.arange(rows_c.shape[1], device=gen.device)[None, :] < tp["counts"][:, :1]
    xy = rows_c[..., 6:8]
    lo = torch.where(valid[..., None], xy, torch.full_like(xy, float("inf"))).amin(dim=1)
    hi = torch.where(valid[..., None], xy, torch.full_like(xy, -float("inf"))).amax(dim=1)
    rows_c[..., 6:8] -= ((lo + hi) / 2)[:, None, :]
    out = {"grid": [72, 72], "cell_ft": CELL, "radius_ft": RADIUS, "margin_ft": MARGIN, "capacity": int(tp["rows"].shape[1]),
           "reps": a.reps, "rounds": a.rounds}

    for label, rows in (("", tp["rows"]), ("centred_", rows_c)):
        for B in (4096, 8):
            batch = {"rows": rows[:B].contiguous(), "counts": tp["counts"][:B].contiguous()}
            out[f"{label}b{B}_rows"] = int(batch["counts"][:, 0].sum().item())
            for mc in (False, True):
                buf = {}
                ms, rounds = timed(lambda: gen.plan_occupancy(batch, foot, scene, CELL, RADIUS, margin=MARGIN, min_clearance=mc, out=buf),
                                   a.reps, a.rounds)
                key = f"{label}b{B}_{'min_' if mc else ''}ms"
                out[key], out[key + "_rounds"] = ms, rounds
            out[f"{label}b{B}_covered_cells"] = int(buf["blocked"].sum().item())
            out[f"{label}b{B}_covering_pairs"] = int(buf["count"].sum(dtype=torch.int64).item())
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
