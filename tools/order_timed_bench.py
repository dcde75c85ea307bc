#!/usr/bin/env python3
"""Timed-order timings (vap_plan_order_timed; plan.order_timed, plan.timed_routine; include/vap.h).

  order_timed_ms   plan.order_timed at M = 8 on caller-written legs (256 shared legs of 50..300 rows with random end headings,
                   a random leg matrix per problem, dwells and a start heading), full mode and under a budget, R = 1 and 4096
  order_ms         plan.order at the same M and R on random matrices, in the same process: a round times one call and then
                   the other, so both see the same clocks.  There is no target; order_ms is what order_timed_ms is read
                   against (the timed table has M times the states and one more loop level)
  routine_ms       BatchedTrajectoryGenerator.plan_timed_routine end to end at tools/routine_bench.py's scene with P = 9 random
                   free points and W = 32 waypoints (travel, profile and time_profile of 64 legs, the order, the gather and
                   the chained timeline), R = 1 and --routines problems, next to plan_routine (travel and order only)

Each figure is the median over --rounds rounds of --reps calls between two device events, after a warm-up call.

    python tools/order_timed_bench.py [--reps 50] [--rounds 5] [--routines 16] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELD = (-6.0, -6.0, 6.0, 6.0)
CELL, RADIUS, MARGIN, W, POINTS = 1.0 / 6.0, 0.75, 0.05, 32, 9


def alternating(fns, reps, rounds):
    """{name: (median_ms, rounds_ms)}: a warm-up call of each, then per round every function in turn, ``reps`` calls between
    two device events."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / reps)
    return {k: (float(np.median(v)), [float(t) for t in v]) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--routines", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from footprint_bench import field_scene
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import plan
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator

    assert torch.cuda.is_available(), "order_timed_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    out = {"sites": POINTS - 1, "reps": a.reps, "rounds": a.rounds}
    rng = np.random.default_rng(11)

    # caller-written legs: only the first and the last row of a leg are read
    L, cap = 256, 300
    counts = rng.integers(50, cap + 1, L).astype(np.int32)
    rows = np.zeros((L, cap, 8))
    rows[:, 0, 4] = rng.uniform(-np.pi, np.pi, L)
    rows[np.arange(L), counts - 1, 4] = rng.uniform(-np.pi, np.pi, L)
    d_rows, d_counts = torch.as_tensor(rows, device=dev), torch.as_tensor(counts, device=dev)
    for R in (1, 4096):
        leg = torch.as_tensor(rng.integers(0, L, (R, POINTS, POINTS)).astype(np.int32), device=dev)
        dwell = torch.as_tensor(rng.uniform(0.0, 0.5, (R, POINTS)), device=dev)
        start = torch.as_tensor(rng.uniform(-np.pi, np.pi, R), device=dev)
        budget = torch.as_tensor(rng.uniform(4.0, 15.0, R), device=dev)
        cost = torch.as_tensor(rng.uniform(1.0, 20.0, (R, POINTS, POINTS)), device=dev)
        fbuf, bbuf, obuf = {}, {}, {}
        got = alternating({
            "order_timed": lambda: plan.order_timed(d_rows, d_counts, leg, dwell=dwell, start_heading=start, out=fbuf),
            "order_timed_budget": lambda: plan.order_timed(d_rows, d_counts, leg, dwell=dwell, start_heading=start, budget=budget, out=bbuf),
            "order": lambda: plan.order(cost, out=obuf)}, a.reps, a.rounds)
        out[f"r{R}"] = {"order_timed_ms": got["order_timed"][0], "order_timed_rounds_ms": got["order_timed"][1],
                        "order_timed_budget_ms": got["order_timed_budget"][0], "order_timed_budget_rounds_ms": got["order_timed_budget"][1],
                        "order_ms": got["order"][0], "order_rounds_ms": got["order"][1],
                        "ratio": got["order_timed"][0] / got["order"][0],
                        "mean_visited_under_budget": float(bbuf["n_visited"].double().mean().item())}

    # end to end at routine_bench's scene
    base = field_scene()
    scene = fp.Scene(field=FIELD, polygons=base.polygons, circles=base.circles)
    ny, nx = plan.grid_shape(scene, CELL)
    free = plan.clearance_grid(scene, CELL, RADIUS, MARGIN)["free"].cpu().numpy()
    cand = np.random.default_rng(7).uniform(-5.5, 5.5, (64 * a.routines * POINTS + 4096, 2))
    ij = np.clip(np.floor((cand - np.array(FIELD[:2])) / CELL).astype(int), 0, [nx - 1, ny - 1])
    cand = cand[free[ij[:, 1], ij[:, 0]]]
    gen = BatchedTrajectoryGenerator(0, "f32")
    out["routine"] = {"grid": [ny, nx], "waypoints": W, "points": POINTS}
    for R in sorted({1, a.routines}):
        pts = torch.as_tensor(cand[:R * POINTS].reshape(R, POINTS, 2).copy(), device=dev)
        dwell = torch.full((R, POINTS), 0.25, dtype=torch.float64, device=dev)
        start = torch.zeros(R, dtype=torch.float64, device=dev)
        tbuf, rbuf = {}, {}
        got = alternating({
            "timed": lambda: gen.plan_timed_routine(pts, scene, W, RADIUS, cell=CELL, margin=MARGIN, dwell=dwell, start_heading=start,
                                                    leg_capacity_rows=1024, capacity_rows=16384, path_capacity=8192, out=tbuf),
            "routine": lambda: gen.plan_routine(pts, scene, W, RADIUS, cell=CELL, margin=MARGIN, out=rbuf)},
            max(a.reps // 5, 2), a.rounds)
        out["routine"][f"r{R}"] = {"timed_routine_ms": got["timed"][0], "timed_routine_rounds_ms": got["timed"][1],
                                   "routine_ms": got["routine"][0], "routine_rounds_ms": got["routine"][1],
                                   "feasible": int(tbuf["feasible"].sum().item()),
                                   "flagged_legs": int((tbuf["leg_flags"] != 0).sum().item()),
                                   "mean_duration_s": float(torch.nan_to_num(tbuf["duration"], nan=0.0).mean().item())}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
