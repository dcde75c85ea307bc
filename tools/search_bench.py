#!/usr/bin/env python3
"""Route-search timings (vap_search_sample, vap_search_update, search.refine; include/vap.h).

Config 3's shape (4096 routes x 32 waypoints, 10000 samples, 2048 rows of capacity) on the field scene of
tools/footprint_bench.py with an 18 x 18 in robot, as one problem of 4096 candidates (R = 1) and as 16 problems of 256
(R = 16).  Per shape, in one process and alternating, each timed with device events over --iters iterations after a
warm-up and repeated --rounds times (the median is reported, the rounds are listed):

  search_ms_per_iteration   search.refine: sample, profile, time_profile, footprint clearance, update per iteration
  evaluation_ms             the same profile + time_profile + footprint_clearance calls alone, on the candidates of the
                            search's last iteration: what one evaluation cost before there was a search
  overhead_ms               the difference: the two search kernels, their launches and any host-side stall of the loop

    python tools/search_bench.py [--iters 20] [--rounds 5] [--json out.json]

The two kernels' own times come from a run under rocprofv3 --kernel-trace --stats (k_search_sample, k_search_update)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from footprint_bench import field_scene
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import search
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "search_bench needs a HIP device"
    assert a.iters >= 20, "time at least 20 iterations"
    gen = BatchedTrajectoryGenerator(0, "f32")
    scene, foot = field_scene(), fp.rectangle(18, 18)
    W, S, cap = 32, 10000, 2048
    out = {"waypoints": W, "samples": S, "capacity_rows": cap, "iterations_timed": a.iters, "rounds": a.rounds}
    for R, N in ((1, 4096), (16, 256)):
        seeds = make_waypoints(R, W, 3).astype(np.float64)
        cfg = search.SearchConfig(candidates=N, elites=max(8, N // 16), iterations=a.iters)
        margin = cfg.weights.clearance_margin

        def run_search():
            return gen.refine(seeds, 0.3, foot, scene, samples=S, capacity_rows=cap, config=cfg)

        last = run_search()                                   # warm-up: every buffer of the loop exists once
        wp = search.sample(last["mean"], last["sigma"], N, dtype=gen.tdtype, seed=cfg.seed, iteration=a.iters,
                           best_waypoints=last["best_waypoints"], best_cost=last["best_cost"], ctx=gen.ctx)
        prof, tp, clr = None, {}, {}

        def run_eval():
            nonlocal prof
            for _ in range(a.iters):
                prof = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=S, out=prof)
                gen.time_profile(prof, DEFAULT_CONSTRAINTS, capacity_rows=cap, out=tp)
                fp.clearance(tp["rows"], tp["counts"], foot, scene, margin=margin, out=clr, ctx=gen.ctx)

        run_eval()
        torch.cuda.synchronize()
        ts, te = [], []
        for _ in range(a.rounds):
            for fn, acc in ((run_search, ts), (run_eval, te)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) / a.iters)
        key = f"r{R}_n{N}"
        out[key + "_search_ms_per_iteration"] = float(np.median(ts))
        out[key + "_evaluation_ms"] = float(np.median(te))
        out[key + "_overhead_ms"] = float(np.median(ts) - np.median(te))
        out[key + "_search_rounds_ms"] = [float(t) for t in ts]
        out[key + "_evaluation_rounds_ms"] = [float(t) for t in te]
        h = last["history"].cpu().numpy()
        out[key + "_best_cost_first_last"] = [float(h[:, 0].mean()), float(h[:, -1].mean())]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
