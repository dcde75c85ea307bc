#!/usr/bin/env python3
"""Robot-to-robot clearance timings (vap_footprint_conflicts; include/vap.h).

Config 3's batch (4096 paths x 32 waypoints, 10000 samples) through profile -> time_profile (~5.2 M rows) is side A, an
18 x 18 in robot.  The partner (15 x 16 in) runs routines of the same kind from the opposite corner of the field: the
same rows turned by 180 degrees about the field centre, starting 25 rows later.  Three inputs:

  (i)   4096 routes against 8 of the partner's
  (ii)  4096 x 4096 all pairs, with and without the per-pair matrices
  (iii) 512 x 512 all pairs with culling off: every row of every pair tested exactly, against the fp64 vector issue
        floor of that brute force (operation counts below, one vector instruction per operation: -ffp-contract=off)

Each figure is the median over --reps calls timed with device events, back to back (no synchronise between calls, one
at the end), after warm-up calls of every variant; culling on and off alternate call by call in the same process, and
their outputs are compared bit for bit.  On (ii) culling on must not be slower than culling off: asserted.

    python tools/conflict_bench.py [--reps 10] [--reps-off 3] [--json out.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_OPS = 157.3e12 / 2       # fp64 vector instructions x lanes per second (the FMA peak counts two per lane)
KEYS = ("min_clearance", "min_other", "min_row", "n_conflicts", "first_row")
PAIR_KEYS = ("pair_clearance", "pair_row", "pair_first_row")


def brute_force_ops(n_a, n_o):
    """fp64 operations of one exact row of one pair as vap_conflict.hip evaluates it when no axis ends the test early:
    the relative pose (14) and the second frame's (6); per axis its rotation into the other frame (6), 5 per vertex of
    the other polygon (2 multiplies, 1 add, min, max), the offset and own extent (6) and the overlap (6); per vertex of
    O its pose and edge in A's frame (12) and, per vertex of A, two point-to-segment distances of 15 and two min."""
    sat = n_a * (18 + 5 * n_o) + n_o * (18 + 5 * n_a)
    dist = n_o * (12 + n_a * 32)
    return 20 + sat + dist + 1


def alternate(torch, variants, reps, warmup=2):
    """Median ms per call of each variant: `reps` rounds, the variants one after another in each."""
    for f in variants.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reps-off", type=int, default=3, help="rounds of the inputs that include a culling-off call")
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
    counts = tp["counts"][:, 0]
    n_rows = int(counts.sum().item())
    foot_a, foot_o = fp.rectangle(18, 18), fp.rectangle(15, 16, 1)
    partner = {"rows": tp["rows"].clone(), "counts": tp["counts"]}
    partner["rows"][:, :, 6:8] *= -1.0
    partner["rows"][:, :, 4] -= math.pi
    shift, margin = 25, 0.04
    out = {"routes": 4096, "rows": n_rows, "capacity": int(tp["rows"].shape[1]), "shift_rows": shift, "margin": margin,
           "footprint_vertices": [len(foot_a), len(foot_o)]}

    def part(d, lo, hi):
        return {"rows": d["rows"][lo:hi], "counts": d["counts"][lo:hi]}

    def horizon_rows(ca, co):
        """sum over pairs of T = max(n_a, n_o + shift, 1)"""
        return int(torch.maximum(ca[:, None], co[None, :] + shift).clamp(min=1).sum().item())

    def run(side_a, side_o, pairs, cull, bufs):
        return gen.footprint_conflicts(side_a, foot_a, side_o, foot_o, margin=margin, shift_rows=shift, pairs=pairs, cull=cull,
                                       out=bufs)

    def same(x, y, keys):
        return all(torch.equal(x[k].view(torch.int64) if x[k].dtype == torch.float64 else x[k],
                               y[k].view(torch.int64) if y[k].dtype == torch.float64 else y[k]) for k in keys)

    # (i) 4096 x 8
    eight = part(partner, 0, 8)
    b_on, b_off = {}, {}
    t = alternate(torch, {"on": lambda: run(tp, eight, False, True, b_on), "off": lambda: run(tp, eight, False, False, b_off)}, a.reps)
    assert same(b_on, b_off, KEYS), "(i): culling changed the outputs"
    out["i_4096x8_cull_on_ms"], out["i_4096x8_cull_off_ms"] = t["on"], t["off"]
    out["i_pair_rows"] = horizon_rows(counts, counts[:8])
    out["i_compatible_routes"] = int((b_on["n_conflicts"] == 0).sum().item())

    # (iii) 512 x 512, culling off, against the issue floor
    a512, o512 = part(tp, 0, 512), part(partner, 0, 512)
    b3_on, b3_off = {}, {}
    t = alternate(torch, {"on": lambda: run(a512, o512, False, True, b3_on), "off": lambda: run(a512, o512, False, False, b3_off)}, a.reps)
    assert same(b3_on, b3_off, KEYS), "(iii): culling changed the outputs"
    pair_rows = horizon_rows(counts[:512], counts[:512])
    ops = float(pair_rows) * brute_force_ops(len(foot_a), len(foot_o))
    out.update(iii_512x512_cull_on_ms=t["on"], iii_512x512_cull_off_ms=t["off"], iii_pair_rows=pair_rows,
               iii_ops_per_pair_row=brute_force_ops(len(foot_a), len(foot_o)), iii_brute_force_gop=ops / 1e9,
               iii_issue_floor_ms=ops / FP64_VECTOR_OPS * 1e3, iii_cull_off_over_floor=t["off"] / (ops / FP64_VECTOR_OPS * 1e3))

    # (ii) 4096 x 4096, with and without the pair matrices, culling on and off alternated
    b_lean, b_full, b_lean_off, b_full_off = {}, {}, {}, {}
    t = alternate(torch, {"lean_on": lambda: run(tp, partner, False, True, b_lean), "lean_off": lambda: run(tp, partner, False, False, b_lean_off),
                          "pairs_on": lambda: run(tp, partner, True, True, b_full), "pairs_off": lambda: run(tp, partner, True, False, b_full_off)},
                  a.reps_off, warmup=1)
    assert same(b_lean, b_lean_off, KEYS) and same(b_full, b_full_off, KEYS + PAIR_KEYS) and same(b_lean, b_full, KEYS), \
        "(ii): culling or the pair matrices changed the outputs"
    out.update(ii_4096x4096_cull_on_ms=t["lean_on"], ii_4096x4096_cull_off_ms=t["lean_off"], ii_4096x4096_pairs_cull_on_ms=t["pairs_on"],
               ii_4096x4096_pairs_cull_off_ms=t["pairs_off"], ii_pair_rows=horizon_rows(counts, counts),
               ii_conflicting_pairs=int(b_lean["n_conflicts"].sum().item()),
               ii_compatible_routes=int((b_lean["n_conflicts"] == 0).sum().item()))
    out["ii_pair_rows_per_s_cull_on"] = out["ii_pair_rows"] / (t["lean_on"] * 1e-3)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    assert t["lean_on"] <= t["lean_off"] and t["pairs_on"] <= t["pairs_off"], "(ii): culling on is slower than culling off"


if __name__ == "__main__":
    main()
