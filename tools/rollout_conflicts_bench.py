#!/usr/bin/env python3
"""Timings of the fused rollout conflicts (vap_rollout_conflicts) beside the pair of calls it replaces, in one process on
the same rows.

Config 3's batch (4096 paths x 32 waypoints, 10000 samples) through profile -> time_profile (~5.2 M rows), an 18 x 18 in
robot, both followers at their defaults (2 substeps), K = 16, 32 and 64 records per route (sample_perturbations' defaults,
tau = 50 ms).  The partner (15 x 16 in) runs routines of the same kind from the opposite corner of the field
(tools/conflict_bench.py's: the same rows turned by 180 degrees about the field centre), Bo = 1 and 8 of them, 25 rows late.
Per configuration and follower, interleaved round by round, each the median of device-event-timed single calls after a
warm-up:
  fused   tracking.rollout_conflicts
  pair    tracking.rollouts(executed=True) followed by footprint.conflicts on its rows
  plain   tracking.rollouts (statistics only: what the conflicts cost on top)
The fused call's per-rollout conflict clearance is compared with the pair's bit for bit.  Also reported: the bytes of
executed rows and of packed side-A rows the pair moves and the fused call does not.  One further row per follower: a
K-distinct rollout_shift (one fused call) against the K conflicts calls, one per shift on the executed routes that carry
it, that it replaces (the executed rows are written once and not timed there).  A configuration whose executed rows do not
fit is named in "not_measured" and on stderr; the fused call and plain rollouts are still timed there.

    python tools/rollout_conflicts_bench.py [--reps 5] [--json out.json] [--rollouts 16,32,64] [--others 1,8] [--paths 4096]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rollouts", default="16,32,64")
    ap.add_argument("--others", default="1,8")
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--shift-rollouts", type=int, default=16, help="K of the per-rollout shift row")
    a = ap.parse_args()
    import torch
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import tracking
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "rollout_conflicts_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    B = a.paths
    wp = torch.tensor(make_waypoints(B, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    torch.cuda.synchronize()
    counts = tp["counts"][:, 0]
    foot_a, foot_o = fp.rectangle(18, 18), fp.rectangle(15, 16, 1)
    partner = {"rows": tp["rows"].clone(), "counts": tp["counts"]}
    partner["rows"][:, :, 6:8] *= -1.0
    partner["rows"][:, :, 4] -= math.pi
    shift, margin = 25, 0.04
    followers = {"ramsete": tracking.Follower(), "pursuit": tracking.Pursuit()}
    cap = int(tp["rows"].shape[1])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"batch": "config 3", "routes": B, "rows": int(counts.sum().item()), "capacity": cap, "margin": margin, "shift_rows": shift,
           "compute_units": cus, "settle_rows": {k: f.settle_rows for k, f in followers.items()}}

    def ms_of(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def timed(calls, key):
        for fn in calls.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        single = {c: [] for c in calls}
        for _ in range(a.reps):                               # interleaved: the same noise for every call
            for c, fn in calls.items():
                single[c].append(ms_of(fn)[0])
        for c in calls:
            out[f"{key}_{c}_call_ms"] = float(np.median(single[c]))
            out[f"{key}_{c}_call_ms_min_max"] = [float(np.min(single[c])), float(np.max(single[c]))]

    for K in [int(k) for k in a.rollouts.split(",")]:
        P = torch.tensor(tracking.sample_perturbations(B, K, seed=1), device=gen.device)
        out[f"k{K}_workgroups"] = (B + 256 // K - 1) // (256 // K) if K <= 256 else B * ((K + 255) // 256)
        for Bo in [int(o) for o in a.others.split(",")]:
            oth = {"rows": partner["rows"][:Bo], "counts": partner["counts"][:Bo]}
            for name, f in followers.items():
                key = f"k{K}_o{Bo}_{name}"
                fb, xb, cb, pb = {}, {}, {}, {}
                calls = {"fused": lambda: gen.rollout_conflicts(tp, f, P, foot_a, oth, foot_o, margin=margin, shift_rows=shift, out=fb),
                         "plain": lambda: gen.tracking_rollouts(tp, f, P, out=pb)}

                def pair():
                    ex = gen.tracking_rollouts(tp, f, P, executed=True, out=xb)
                    return gen.footprint_conflicts(ex, foot_a, oth, foot_o, margin=margin, shift_rows=shift, out=cb)

                out[f"{key}_pair_executed_row_bytes"] = B * K * (cap + f.settle_rows) * 64
                out[f"{key}_pair_packed_a_bytes"] = B * K * ((max(cap + f.settle_rows, cap + shift) + 63) // 64 * 64) * 32
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
                timed(calls, key)
                if "pair" in calls:
                    same = torch.equal(fb["conflict"].view(torch.int64).view(-1), cb["min_clearance"].view(torch.int64))
                    assert same, f"{key}: the fused conflict clearance differs from the pair's"
                    out[f"{key}_fused_over_pair"] = out[f"{key}_fused_call_ms"] / out[f"{key}_pair_call_ms"]
                out[f"{key}_fused_over_plain"] = out[f"{key}_fused_call_ms"] / out[f"{key}_plain_call_ms"]
                out[f"{key}_rollouts_conflicting"] = int(fb["n_conflicting"].sum().item())
                out[f"{key}_rollouts_valid"] = int(fb["n_conflict_valid"].sum().item())
                print(f"{key}: fused {out[f'{key}_fused_call_ms']:.1f} ms, pair {out.get(f'{key}_pair_call_ms', float('nan')):.1f} ms, plain "
                      f"{out[f'{key}_plain_call_ms']:.1f} ms", file=sys.stderr, flush=True)
                fb = xb = cb = pb = None
                calls = None
                torch.cuda.empty_cache()
        del P

    # a K-distinct rollout shift: one fused call against the K conflicts calls it replaces
    K, Bo = a.shift_rollouts, 1
    P = torch.tensor(tracking.sample_perturbations(B, K, seed=1), device=gen.device)
    oth = {"rows": partner["rows"][:Bo], "counts": partner["counts"][:Bo]}
    jitter = torch.arange(K, dtype=torch.int32, device=gen.device) * 7 - 7 * (K // 2)
    for name, f in followers.items():
        key = f"shift_k{K}_{name}"
        fb = {}
        try:
            ex = gen.tracking_rollouts(tp, f, P, executed=True)
            per = [{"rows": ex["rows"][k::K].contiguous(), "counts": ex["counts"][k::K].contiguous()} for k in range(K)]
            del ex
            torch.cuda.synchronize()
        except torch.OutOfMemoryError:
            out.setdefault("not_measured", []).append(key)
            print(f"{key}: NOT MEASURED, the executed rows did not fit on the device", file=sys.stderr)
            continue
        cbs = [{} for _ in range(K)]

        def k_calls():
            for k in range(K):
                gen.footprint_conflicts(per[k], foot_a, oth, foot_o, margin=margin, shift_rows=shift + 7 * k - 7 * (K // 2), out=cbs[k])

        timed({"fused": lambda: gen.rollout_conflicts(tp, f, P, foot_a, oth, foot_o, margin=margin, shift_rows=shift, rollout_shift=jitter, out=fb),
               "k_conflicts": k_calls}, key)
        for k in range(K):
            assert torch.equal(fb["conflict"][:, k].contiguous().view(torch.int64), cbs[k]["min_clearance"].view(torch.int64)), (key, k)
        out[f"{key}_k_conflicts_over_fused"] = out[f"{key}_k_conflicts_call_ms"] / out[f"{key}_fused_call_ms"]
        print(f"{key}: fused {out[f'{key}_fused_call_ms']:.1f} ms, {K} conflicts calls {out[f'{key}_k_conflicts_call_ms']:.1f} ms (executed rows "
              f"already written)", file=sys.stderr, flush=True)
        per = cbs = fb = None
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
