#!/usr/bin/env python3
"""Footprint-clearance timings (vap_footprint_clearance; include/vap.h).

Config 3's batch (4096 paths x 32 waypoints, 10000 samples) through profile -> time_profile (~5.2 M rows), checked
against a field-like scene: the walls of the GUI's field, 8 convex polygons of 3..8 vertices and 4 circles, with an
18 x 18 in robot, once as generated (the routes leave the field) and once with every route moved so that its extent is
centred on the field ("centred_").  Times the clearance call with culling on and off, with and without the per-row output: median of
CUDA-event-timed calls each followed by a synchronise (*_call_ms), and the mean of back-to-back calls (*_ms).  Also prints the brute-force work estimate (every element tested exactly at every row) and what
it would take at the MI355X's fp64 vector peak.

    python tools/footprint_bench.py [--reps 30] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK = 157.3e12 / 2       # vector fp64, flop/s


def field_scene():
    """A scene shaped like a game field: walls, 8 convex elements of 3..8 vertices, 4 round posts (seeded)."""
    from vexautonomousplanner_amd import footprint as fp
    rng = np.random.default_rng(2024)
    polys = []
    for k in range(8):
        n = 3 + k % 6                                   # 3..8 vertices
        a = np.arange(n) * 2 * np.pi / n + rng.uniform(-0.3, 0.3, n) * np.pi / n + rng.uniform(0, 2 * np.pi)
        c, r = rng.uniform(-4.5, 4.5, 2), rng.uniform(0.3, 0.9)
        polys.append(np.stack([c[0] + r * np.cos(a), c[1] + 0.7 * r * np.sin(a)], axis=1))
    circles = [(*rng.uniform(-4.5, 4.5, 2), rng.uniform(0.15, 0.4)) for _ in range(4)]
    return fp.Scene(polygons=polys, circles=circles)


def brute_force_flops(n_rows, n_foot, scene):
    """fp64 operations of testing every element exactly at every row: the separating-axis projections (2 multiplies, 1
    add and 2 min/max per vertex and axis) and the vertex-to-edge distances (~14 per pair, both ways) of each polygon,
    ~20 per footprint edge of each circle, ~8 per footprint vertex for the walls."""
    per_row = 8 * n_foot + 20 * n_foot * scene.n_circles
    for p in scene.polygons:
        m = len(p)
        per_row += (n_foot + m) * (n_foot + m) * 5 + 2 * n_foot * m * 14
    return float(n_rows) * per_row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    gen = BatchedTrajectoryGenerator(0, "f32")
    wp = torch.tensor(make_waypoints(4096, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    torch.cuda.synchronize()
    n_rows = int(tp["counts"][:, 0].sum().item())
    scene = field_scene()
    foot = fp.rectangle(18, 18)
    out = {"routes": 4096, "rows": n_rows, "capacity": int(tp["rows"].shape[1]), "polygons": scene.n_polygons,
           "polygon_vertices": int(scene.poly_start[-1]), "circles": scene.n_circles, "footprint_vertices": len(foot)}
    # config 3's random walks start at (-5, -5) ft and leave the field: every route is off it somewhere, and the wall's
    # negative clearance lets culling skip nearly every element.  The "centred_" runs move each route so that its extent
    # is centred on the field: most rows are then on the field, among the elements.
    rows_c = tp["rows"].clone()
    valid = torch.arange(rows_c.shape[1], device=gen.device)[None, :] < tp["counts"][:, :1]
    xy = rows_c[..., 6:8]
    lo = torch.where(valid[..., None], xy, torch.full_like(xy, float("inf"))).amin(dim=1)
    hi = torch.where(valid[..., None], xy, torch.full_like(xy, -float("inf"))).amax(dim=1)
    rows_c[..., 6:8] -= ((lo + hi) / 2)[:, None, :]
    centred = {"rows": rows_c, "counts": tp["counts"]}
    for label, batch in (("", tp), ("centred_", centred)):
        ref = None
        for cull in (True, False):
            for per_row in (False, True):
                bufs = {}
                for _ in range(3):
                    gen.footprint_clearance(batch, foot, scene, margin=0.04, per_row=per_row, out=bufs, cull=cull)
                torch.cuda.synchronize()
                ts = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    r = gen.footprint_clearance(batch, foot, scene, margin=0.04, per_row=per_row, out=bufs, cull=cull)
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                key = f"{label}cull_{'on' if cull else 'off'}{'_per_row' if per_row else ''}_ms"
                out[key.replace("_ms", "_call_ms")] = float(np.median(ts))
                # back to back: the host's part of a call (scene checks, packing, upload) overlaps the previous kernel
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    r = gen.footprint_clearance(batch, foot, scene, margin=0.04, per_row=per_row, out=bufs, cull=cull)
                e1.record()
                e1.synchronize()
                out[key] = e0.elapsed_time(e1) / a.reps
                summary = {k: r[k].clone() for k in ("min_clearance", "min_row", "min_element", "first_row", "n_below")}
                if ref is None:
                    ref = summary
                    out[label + "feasible_routes"] = int(r["feasible"].sum().item())
                    out[label + "routes_touching"] = int((r["min_clearance"] < 0).sum().item())
                    out[label + "rows_below_margin"] = int(r["n_below"].sum().item())
                else:
                    same = all(torch.equal(ref[k], summary[k]) for k in ("min_row", "min_element", "first_row", "n_below")) and \
                        torch.equal(ref["min_clearance"].view(torch.int64), summary["min_clearance"].view(torch.int64))
                    assert same, f"{key}: outputs differ from the first configuration"
    flops = brute_force_flops(n_rows, len(foot), scene)
    out["brute_force_gflop"] = flops / 1e9
    out["brute_force_at_fp64_peak_ms"] = flops / FP64_PEAK * 1e3
    out["rows_per_s_cull_on"] = n_rows / (out["cull_on_ms"] * 1e-3)
    out["rows_per_s_centred_cull_on"] = n_rows / (out["centred_cull_on_ms"] * 1e-3)
    out["cull_off_share_of_fp64_peak"] = flops / (out["cull_off_ms"] * 1e-3) / FP64_PEAK
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
