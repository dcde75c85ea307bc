#!/usr/bin/env python3
"""Grid-planner timings (vap_plan_grid, vap_plan_seeds, plan.clearance_grid, plan.seeds; include/vap.h).

The +-6 ft field at cell = 2 in (72 x 72 cells) with the polygons and posts of tools/footprint_bench.py's field scene, a
disc of 0.75 ft and margin 0.05 ft; R = 256 and R = 4096 random (start, goal) pairs, W = 32 waypoints.  Each call is timed
with device events over --reps calls after a warm-up and repeated --rounds times (the median is reported, the rounds are
listed):

  grid_ms          plan.clearance_grid: the scene's upload and k_plan_clearance
  seeds_ms         plan.seeds: the upload, k_plan_clearance into the free mask and k_plan_seeds for R problems
  cpu_ref_ms       tests/plan_ref.py on the first --cpu-problems of the same problems, per problem, on the host: for
                   information only (a NumPy + heapq statement of the definitions, not an optimised planner)

    python tools/plan_bench.py [--reps 50] [--rounds 5] [--cpu-problems 16] [--json out.json]

The kernels' own times come from a run under rocprofv3 --kernel-trace --stats (k_plan_clearance, k_plan_seeds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELD = (-6.0, -6.0, 6.0, 6.0)
CELL, RADIUS, MARGIN, W = 1.0 / 6.0, 0.75, 0.05, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-problems", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from _timing import timed
    from footprint_bench import field_scene
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import plan

    assert torch.cuda.is_available(), "plan_bench needs a HIP device"
    base = field_scene()
    scene = fp.Scene(field=FIELD, polygons=base.polygons, circles=base.circles)
    ny, nx = plan.grid_shape(scene, CELL)
    out = {"grid": [ny, nx], "cell_ft": CELL, "radius_ft": RADIUS, "margin_ft": MARGIN, "waypoints": W, "reps": a.reps,
           "rounds": a.rounds}

    gbuf = {}
    out["grid_ms"], out["grid_rounds_ms"] = timed(lambda: plan.clearance_grid(scene, CELL, RADIUS, MARGIN, out=gbuf), a.reps, a.rounds)
    out["free_cells"] = int(gbuf["free"].sum().item())
    rng = np.random.default_rng(7)
    for R in (256, 4096):
        pts = rng.uniform(-5.5, 5.5, (R, 2, 2))
        starts, goals = torch.as_tensor(pts[:, 0].copy(), device="cuda:0"), torch.as_tensor(pts[:, 1].copy(), device="cuda:0")
        buf = {}
        ms, rounds = timed(lambda: plan.seeds(starts, goals, scene, W, RADIUS, cell=CELL, margin=MARGIN, out=buf), a.reps, a.rounds)
        out[f"r{R}_seeds_ms"], out[f"r{R}_seeds_rounds_ms"] = ms, rounds
        out[f"r{R}_feasible"] = int(buf["feasible"].sum().item())
        out[f"r{R}_flags_or"] = int(np.bitwise_or.reduce(buf["flags"].cpu().numpy()))
        if R == 256 and a.cpu_problems > 0:
            import plan_ref as pr
            n = min(a.cpu_problems, R)
            kw = dict(field=FIELD, cell=CELL, polygons=scene.polygons, circles=[tuple(c) for c in scene.circles], radius=RADIUS)
            t0 = time.perf_counter()
            ref, _ = pr.seeds(pts[:n, 0], pts[:n, 1], margin=MARGIN, W=W, **kw)
            out["cpu_ref_ms_per_problem"] = (time.perf_counter() - t0) * 1e3 / n
            got = buf["waypoints"][:n].cpu().numpy()
            want = np.stack([r["waypoints"] for r in ref])
            out["cpu_ref_max_abs_diff"] = float(np.nanmax(np.abs(got - want))) if np.isfinite(want).any() else 0.0
            out["cpu_ref_same_failures"] = bool(np.array_equal(np.isnan(got), np.isnan(want)))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
