#!/usr/bin/env python3
"""Timings of the fused rollout clearance (vap_rollout_clearance) beside the two-call pipeline it replaces, in one process
on the same rows.

Config 3's batch (4096 paths x 32 waypoints, 10000 samples) through profile -> time_profile (~5.2 M rows), an 18 x 18 in
robot, a scene of the field walls, 8 polygons and 4 circles laid beside rows of the batch, K = 16 and K = 64 records per
route (sample_perturbations' defaults, tau = 50 ms), both followers at their defaults (2 substeps).  Per configuration
and follower three things are timed, interleaved repetition by repetition, each as the median of device-event-timed
single calls:
  fused   tracking.rollout_clearance
  pair    tracking.rollouts(executed=True) followed by footprint.clearance on its rows
  plain   tracking.rollouts (statistics only: what the clearance costs on top)
The fused call's per-rollout clearance is compared with the pair's bit for bit.  Also reported: the bytes of executed rows
the pair allocates (the fused call allocates none).  A configuration whose executed rows do not fit is named in
"not_measured" and on stderr; the fused call and plain rollouts are still timed there.

Config 3's routes are some 40 ft of random walk each through one field, so with 12 elements on it nearly every rollout
passes one of them within the margin ("rollouts_colliding"); the walls' distance does not change that.

    python tools/rollout_clearance_bench.py [--reps 5] [--json out.json] [--rollouts 16,64] [--paths 4096]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_scene(fp, rows, counts, rng):
    """Walls a foot outside the box of every route's rows, 8 polygons and 4 circles, each about a robot's half-width beside
    a row of some route."""
    n = counts.astype(np.int64)
    live = np.nonzero(n > 20)[0]
    spots = []
    for b in rng.choice(live, 12, replace=False):
        r = int(rng.integers(5, n[b] - 5))
        phi = -rows[b, r, 4]
        off = rng.choice([-1.0, 1.0]) * (0.75 + 0.2 + rng.uniform(0.0, 0.4))
        spots.append((rows[b, r, 6] - off * np.sin(phi), rows[b, r, 7] + off * np.cos(phi)))
    polygons = []
    for cx, cy in spots[:8]:
        m = int(rng.integers(3, 7))
        ang = np.linspace(0, 2 * np.pi, m, endpoint=False) + rng.uniform(0, 1)
        polygons.append(np.stack([cx + 0.2 * np.cos(ang), cy + 0.2 * np.sin(ang)], axis=1))
    circles = [(cx, cy, 0.2) for cx, cy in spots[8:]]
    xy = np.concatenate([rows[b, :n[b], 6:8] for b in live])
    lo, hi = xy.min(axis=0) - 1.0, xy.max(axis=0) + 1.0
    return fp.Scene(field=(lo[0], lo[1], hi[0], hi[1]), polygons=polygons, circles=circles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rollouts", default="16,64")
    ap.add_argument("--paths", type=int, default=4096)
    a = ap.parse_args()
    import torch
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import tracking
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "rollout_clearance_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    B = a.paths
    wp = torch.tensor(make_waypoints(B, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    torch.cuda.synchronize()
    counts = tp["counts"][:, 0]
    foot = fp.rectangle(18, 18)
    margin = 0.05
    scene = make_scene(fp, tp["rows"].cpu().numpy(), counts.cpu().numpy(), np.random.default_rng(3))
    followers = {"ramsete": tracking.Follower(), "pursuit": tracking.Pursuit()}
    cap = int(tp["rows"].shape[1])
    out = {"batch": "config 3", "routes": B, "rows": int(counts.sum().item()), "capacity": cap, "margin": margin,
           "scene": {"walls": 1, "polygons": scene.n_polygons, "circles": scene.n_circles},
           "settle_rows": {k: f.settle_rows for k, f in followers.items()}}

    def ms_of(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for K in [int(k) for k in a.rollouts.split(",")]:
        P = torch.tensor(tracking.sample_perturbations(B, K, seed=1), device=gen.device)
        for name, f in followers.items():
            key = f"k{K}_{name}"
            fb, xb, cb, pb = {}, {}, {}, {}
            calls = {"fused": lambda: gen.rollout_clearance(tp, f, P, foot, scene, margin=margin, out=fb),
                     "plain": lambda: gen.tracking_rollouts(tp, f, P, out=pb)}

            def pair():
                ex = gen.tracking_rollouts(tp, f, P, executed=True, out=xb)
                return gen.footprint_clearance(ex, foot, scene, margin=margin, out=cb)

            out[f"{key}_pair_executed_row_bytes"] = B * K * (cap + f.settle_rows) * 64
            try:
                for _ in range(2):
                    pair()
                torch.cuda.synchronize()
                calls["pair"] = pair
            except torch.OutOfMemoryError:
                out.setdefault("not_measured", []).append(f"{key}_pair")
                print(f"{key}: pair NOT MEASURED, the executed rows did not fit on the device", file=sys.stderr)
                xb.clear()
                cb.clear()
                torch.cuda.empty_cache()
            for c in ("fused", "plain"):
                for _ in range(2):
                    calls[c]()
            torch.cuda.synchronize()
            single = {c: [] for c in calls}
            for _ in range(a.reps):                               # interleaved: the same noise for every call
                for c, fn in calls.items():
                    single[c].append(ms_of(fn)[0])
            for c in calls:
                out[f"{key}_{c}_call_ms"] = float(np.median(single[c]))
                out[f"{key}_{c}_call_ms_min_max"] = [float(np.min(single[c])), float(np.max(single[c]))]
            if "pair" in calls:
                same = torch.equal(fb["clearance"].view(torch.int64).view(-1), cb["min_clearance"].view(torch.int64))
                assert same, f"{key}: the fused clearance differs from the pair's"
                out[f"{key}_fused_over_pair"] = out[f"{key}_fused_call_ms"] / out[f"{key}_pair_call_ms"]
            out[f"{key}_fused_over_plain"] = out[f"{key}_fused_call_ms"] / out[f"{key}_plain_call_ms"]
            nv = fb["n_clear_valid"]
            out[f"{key}_routes_colliding"] = int((fb["n_colliding"] > 0).sum().item())
            out[f"{key}_rollouts_colliding"] = int(fb["n_colliding"].sum().item())
            out[f"{key}_rollouts_valid"] = int(nv.sum().item())
            print(f"{key}: fused {out[f'{key}_fused_call_ms']:.1f} ms, pair {out.get(f'{key}_pair_call_ms', float('nan')):.1f} ms, plain "
                  f"{out[f'{key}_plain_call_ms']:.1f} ms", file=sys.stderr, flush=True)
            fb = xb = cb = pb = None
            calls = None
            torch.cuda.empty_cache()
        del P
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
