#!/usr/bin/env python3
"""Routine-planner timings (vap_plan_travel, vap_plan_order; plan.travel, plan.order; include/vap.h).

tools/plan_bench.py's scene and grid (the +-6 ft field at cell = 2 in, 72 x 72 cells, a disc of 0.75 ft, margin 0.05 ft),
P = 11 random free points per problem, W = 32 waypoints, R = 1, 64 and 1024 problems.  Each call is timed with device
events over --reps calls after a warm-up and repeated --rounds times (the median is reported, the rounds are listed):

  travel_ms        plan.travel: the upload, k_plan_clearance and k_plan_travel, R P fields for R P (P - 1) routes
  seeds_ms         the baseline: plan.seeds on the same R P (P - 1) (start, goal) pairs, a field per pair
  ratio            seeds_ms / travel_ms
  order_ms         plan.order at M = 10 on random matrices, R = 1 and 4096

    python tools/routine_bench.py [--reps 50] [--rounds 5] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELD = (-6.0, -6.0, 6.0, 6.0)
CELL, RADIUS, MARGIN, W, POINTS = 1.0 / 6.0, 0.75, 0.05, 32, 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from _timing import timed
    from footprint_bench import field_scene
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import plan

    assert torch.cuda.is_available(), "routine_bench needs a HIP device"
    base = field_scene()
    scene = fp.Scene(field=FIELD, polygons=base.polygons, circles=base.circles)
    ny, nx = plan.grid_shape(scene, CELL)
    out = {"grid": [ny, nx], "cell_ft": CELL, "radius_ft": RADIUS, "margin_ft": MARGIN, "waypoints": W, "points": POINTS,
           "reps": a.reps, "rounds": a.rounds}

    # random points on free cells
    free = plan.clearance_grid(scene, CELL, RADIUS, MARGIN)["free"].cpu().numpy()
    rng = np.random.default_rng(7)
    cand = rng.uniform(-5.5, 5.5, (64 * 1024 * POINTS, 2))
    ij = np.clip(np.floor((cand - np.array(FIELD[:2])) / CELL).astype(int), 0, [nx - 1, ny - 1])
    cand = cand[free[ij[:, 1], ij[:, 0]]]
    idx = torch.arange(POINTS, device="cuda:0")
    a_idx, b_idx = [t.reshape(-1) for t in torch.meshgrid(idx, idx, indexing="ij")]
    off = a_idx != b_idx
    a_idx, b_idx = a_idx[off], b_idx[off]
    for R in (1, 64, 1024):
        pts = torch.as_tensor(cand[:R * POINTS].reshape(R, POINTS, 2).copy(), device="cuda:0")
        starts, goals = pts[:, a_idx].reshape(-1, 2).contiguous(), pts[:, b_idx].reshape(-1, 2).contiguous()
        tbuf, sbuf = {}, {}
        t_ms, t_rounds = timed(lambda: plan.travel(pts, scene, RADIUS, cell=CELL, margin=MARGIN, waypoints=W, out=tbuf),
                               a.reps, a.rounds)
        s_ms, s_rounds = timed(lambda: plan.seeds(starts, goals, scene, W, RADIUS, cell=CELL, margin=MARGIN, out=sbuf),
                               a.reps, a.rounds)
        same = torch.equal(tbuf["waypoints"][:, a_idx, b_idx].reshape(-1, W, 2).view(torch.int64), sbuf["waypoints"].view(torch.int64))
        out[f"r{R}"] = {"pairs": int(starts.shape[0]), "travel_ms": t_ms, "travel_rounds_ms": t_rounds, "seeds_ms": s_ms,
                        "seeds_rounds_ms": s_rounds, "ratio": s_ms / t_ms, "same_bits": bool(same),
                        "feasible": int(tbuf["feasible"].sum().item())}
    for R in (1, 4096):
        cost = torch.as_tensor(rng.uniform(1.0, 20.0, (R, POINTS, POINTS)), device="cuda:0")
        obuf = {}
        o_ms, o_rounds = timed(lambda: plan.order(cost, out=obuf), a.reps, a.rounds)
        out[f"order_r{R}"] = {"sites": POINTS - 1, "order_ms": o_ms, "order_rounds_ms": o_rounds}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
