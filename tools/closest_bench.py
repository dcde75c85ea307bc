#!/usr/bin/env python3
"""Closest-point projection timings (vap_route_closest / vap_closest_points; gui/path.py:658-727).

  1. the drop-in's single-query find_closest_point on config 1's path (c1_w8) — what a GUI mouse event costs — against
     the same search done the way a GUI bound to the scalar drop-in calls does it: 25*len(nodes)+1 + 501 calls of
     percent_to_parameter + get_point_at_parameter, each its own copy / launch / copy / synchronise (same process)
  2. the batch closest_points for config 3's batch (4096 paths x 32 waypoints) with Q random field queries per path, GUI
     and EXACT mode: median of CUDA-event-timed calls, queries/s, and GUI mode's share of the fp64 vector peak (half the
     157 TF fp32 vector figure; a GUI query is 25W+1+501 evaluations of ~60 fp64 flops)

    python tools/closest_bench.py [--reps 50] [--queries 64] [--json out.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_PEAK = 157.3e12 / 2
FLOPS_PER_EVAL = 60


def c1_manager():
    import golden_util as gu
    from vexautonomousplanner_amd.nodes import Node
    from vexautonomousplanner_amd.splines.spline_manager import QuinticHermiteSplineManager
    g = gu.load("c1_w8")
    m = QuinticHermiteSplineManager()
    assert m.build_path(np.asarray(g["waypoints"], dtype=float), [Node() for _ in g["waypoints"]], [])
    return m


def scalar_search(m, q):
    """gui/path.py:690-722 through the scalar drop-in accessors, one call per evaluation."""
    min_dist, cp, best = float("inf"), 0.0, 0.0
    n = 25 * len(m.nodes)
    for i in range(n + 1):
        percent = i / n
        t = m.percent_to_parameter(percent)
        p = m.get_point_at_parameter(t)
        d = math.hypot(p[0] - q[0], p[1] - q[1])
        if d < min_dist:
            min_dist, cp, best = d, percent, t
    start, end = max(0.0, cp - 0.02), min(1.0, cp + 0.02)
    step = (end - start) / 500
    for i in range(501):
        t = m.percent_to_parameter(start + i * step)
        p = m.get_point_at_parameter(t)
        d = math.hypot(p[0] - q[0], p[1] - q[1])
        if d < min_dist:
            min_dist, best = d, t
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--scalar-queries", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import make_waypoints
    out = {}
    rng = np.random.default_rng(0)

    # -- 1. drop-in, one query per call, config 1 ------------------------------------------------------------------
    m = c1_manager()
    qs = rng.uniform(-6.05, 6.05, (a.reps + 10, 2))
    for q in qs[:10]:
        m.find_closest_point(q)
    ts = []
    for q in qs[10:]:
        t0 = time.perf_counter()
        m.find_closest_point(q)
        ts.append(time.perf_counter() - t0)
    single_ms = float(np.median(ts)) * 1e3
    ts, agree = [], 0
    for q in qs[10:10 + a.scalar_queries]:
        t0 = time.perf_counter()
        t_s = scalar_search(m, q)
        ts.append(time.perf_counter() - t0)
        agree += int(t_s == m.find_closest_point(q)[1])
    scalar_ms = float(np.median(ts)) * 1e3
    out["dropin_c1_single_query_ms"] = single_ms
    out["dropin_c1_scalar_emulation_ms"] = scalar_ms
    out["dropin_c1_speedup"] = scalar_ms / single_ms
    out["dropin_c1_scalar_agrees"] = f"{agree}/{a.scalar_queries}"
    print(f"drop-in c1 find_closest_point: {single_ms:.4f} ms median ({a.reps} calls); scalar-call emulation "
          f"{scalar_ms:.2f} ms median ({a.scalar_queries} queries, {agree} same parameter) -> {scalar_ms / single_ms:.0f}x")

    # -- 2. batch, config 3 ----------------------------------------------------------------------------------------
    B, W, Q = 4096, 32, a.queries
    gen = BatchedTrajectoryGenerator(0, "f32")
    r = gen.profile(torch.tensor(make_waypoints(B, W, 3), device=gen.device), samples=6000)
    q = torch.tensor(rng.uniform(-6.05, 6.05, (B, Q, 2)), device=gen.device)
    res = {}
    for mode in ("gui", "exact"):
        for _ in range(3):
            gen.closest_points(r, q, mode=mode, out=res)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            gen.closest_points(r, q, mode=mode, out=res)
            e1.record()
        torch.cuda.synchronize()
        ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
        qps = B * Q / (ms * 1e-3)
        out[f"batch_c3_q{Q}_{mode}_ms"] = ms
        out[f"batch_c3_q{Q}_{mode}_queries_per_s"] = qps
        line = f"batch config 3 ({B} x {W}), Q={Q}, {mode:5s}: {ms:.3f} ms median ({a.reps} calls), {qps / 1e6:.1f} M queries/s"
        if mode == "gui":
            flops = B * Q * (25 * W + 1 + 501) * FLOPS_PER_EVAL
            share = flops / (ms * 1e-3) / FP64_PEAK
            out["batch_c3_gui_fp64_peak_share"] = share
            out["batch_c3_gui_fp64_floor_ms"] = flops / FP64_PEAK * 1e3
            line += f", {share * 100:.1f} % of the fp64 vector peak (floor {flops / FP64_PEAK * 1e3:.3f} ms)"
        print(line)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
