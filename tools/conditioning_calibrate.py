"""Calibrate conditioning.ETA: on the device in fp64, observed_b / cond_b over three sets of paths —
the 2048-path config-3 sweep and the 160-case fuzz slice of tests/test_gpu_sweeps.py (observed: the largest relative velocity
error against the oracle) and fixture big_w2048_p2 (against the real reference's row) — with cond taken with 7 probes.
Prints the largest ratio over the paths with observed >= 1e-9 (ETA is 4 x that), the histogram of the ratio over all paths,
the share of each set that a limit of tol / ETA flags with the default 3 probes, and the paths of largest cond / observed.

  python tools/conditioning_calibrate.py [--tol 1e-6] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from oracle import oracle  # noqa: E402
from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator  # noqa: E402
from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints  # noqa: E402


NOTES = []


def measure(gen, wp, ref_velocity, n_samples, sets, name, **kw):
    """observed and cond (7 probes and 3) of every path of one profile() call; ref_velocity (B, cap) with rows of n_samples."""
    r = gen.profile(torch.tensor(wp, dtype=torch.float64, device=gen.device), **kw)
    c7 = gen.conditioning(r, constraints=kw.get("constraints", DEFAULT_CONSTRAINTS), start_vel=kw.get("start_vel", 0.01),
                          end_vel=kw.get("end_vel", 0.01), probes=7, limit=float("inf"))["cond"].cpu().numpy()
    c3 = gen.conditioning(r, constraints=kw.get("constraints", DEFAULT_CONSTRAINTS), start_vel=kw.get("start_vel", 0.01),
                          end_vel=kw.get("end_vel", 0.01), probes=3, limit=float("inf"))["cond"].cpu().numpy()
    v = r["velocity"].cpu().numpy()
    for b in range(len(wp)):
        n = int(n_samples[b])
        obs = float(np.max(np.abs(v[b, :n] - ref_velocity[b][:n]) / ref_velocity[b][:n])) if n else 0.0
        sets.setdefault(name, []).append((obs, float(c7[b]), float(c3[b])))
        NOTES.append((float(c7[b]), obs, f"{name} path {b}: W={wp.shape[1]} N={n} " + " ".join(f"{k}={v}" for k, v in kw.items() if k in ("dd", "start_vel", "end_vel"))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gen = BatchedTrajectoryGenerator(0, "f64")
    sets = {}
    # the config-3 sweep of tests/test_gpu_sweeps.py
    wp = make_waypoints(2048, 32, 12345).astype(np.float32).astype(np.float64)
    ref = oracle.profile_batch(wp, 10000, DEFAULT_CONSTRAINTS, n_threads=16, want=("velocity",))
    measure(gen, wp, ref["velocity"], [10000] * 2048, sets, "config3_sweep", constraints=DEFAULT_CONSTRAINTS, samples=10000,
            want=("curvature", "velocity"))
    print("config-3 sweep done", flush=True)
    # its fuzz slice (the same generator calls in the same order)
    rng = np.random.default_rng(20261004)
    for case in range(160):
        W = int(rng.choice([2, 3, 4, 5, 8, 13, 32, 57, 113]))
        S = int(rng.choice([2, 3, 7, 64, 255, 256, 257, 1000, 1024, 1025, 4096, 4097, 10000, 20481]))
        B = int(rng.integers(1, 9)) if S <= 10000 else 1
        seed = int(rng.integers(0, 1 << 30))
        cons = list(DEFAULT_CONSTRAINTS)
        if rng.random() < 0.5:
            cons[0] = float(rng.uniform(1.0, 8.0))
            cons[1] = float(rng.uniform(2.0, 16.0))
            cons[2] = float(rng.uniform(2.0, 16.0))
            cons[5] = float(rng.uniform(0.5, 2.0))
        wp = make_waypoints(B, W, seed).astype(np.float32).astype(np.float64)
        sv, ev = 0.01, 0.01
        if rng.random() < 0.3:
            sv, ev = float(rng.uniform(0.01, 2.0)), float(rng.uniform(0.01, 2.0))
        use_dd = S <= 4097 and rng.random() < 0.3
        if use_dd:
            dd = float(rng.uniform(0.002, 0.02))
            per = []
            for b in range(B):
                op = oracle.OraclePath(wp[b])
                op.rebuild_tables()
                per.append(op.forward_backward(cons, dd=dd, start_vel=sv, end_vel=ev)["velocity"])
            measure(gen, wp, per, [len(p) for p in per], sets, "fuzz_slice", constraints=cons, dd=dd, capacity=max(len(p) for p in per) + 3,
                    start_vel=sv, end_vel=ev, want=("curvature", "velocity"))
        else:
            ref = oracle.profile_batch(wp, S, cons, start_vel=sv, end_vel=ev, n_threads=8, want=("velocity",))
            measure(gen, wp, ref["velocity"], [S] * B, sets, "fuzz_slice", constraints=cons, samples=S, start_vel=sv, end_vel=ev,
                    want=("curvature", "velocity"))
    print("fuzz slice done", flush=True)
    import golden_util as gu
    g = gu.load("big_w2048_p2")
    N = int(g["n_samples"])
    measure(gen, g["waypoints"][None], [g["velocity_full"]], [N], sets, "big_w2048_p2", constraints=g["constraints"], dd=float(g["dd"]),
            capacity=N + 2, want=("curvature", "velocity"))
    rows = [x for v in sets.values() for x in v]
    cal = [(o / c7, o, c7) for o, c7, _ in rows if o >= 1e-9 and c7 > 0]
    worst = max(cal) if cal else (float("nan"),) * 3
    eta = 4 * worst[0]
    limit = args.tol / eta
    ratios = np.array([o / c7 for o, c7, _ in rows if o > 0 and c7 > 0])
    edges = np.arange(-20, -9)
    hist, _ = np.histogram(np.log10(ratios), bins=edges)
    rep = {"paths": len(rows), "paths_with_observed_ge_1e-9": len(cal), "largest_ratio": worst[0], "at_observed": worst[1],
           "at_cond7": worst[2], "eta": eta, "tol": args.tol, "limit": limit,
           "log10_ratio_histogram": {f"[{int(a)},{int(a) + 1})": int(h) for a, h in zip(edges[:-1], hist)},
           "ratio_min_median_max": [float(ratios.min()), float(np.median(ratios)), float(ratios.max())],
           "sets": {k: {"paths": len(v), "observed_max": max(o for o, _, _ in v), "cond7_median": float(np.median([c for _, c, _ in v])),
                        "cond7_max": max(c for _, c, _ in v), "cond3_max": max(c for _, _, c in v),
                        "flagged_share_k3": float(np.mean([c > limit for _, _, c in v]))} for k, v in sets.items()}}
    rep["largest_cond7"] = [{"cond7": c, "observed": o, "path": t} for c, o, t in sorted(NOTES, reverse=True)[:8]]
    rep["largest_observed"] = [{"cond7": c, "observed": o, "path": t} for c, o, t in sorted(NOTES, key=lambda x: -x[1])[:5]]
    rep["limit_note"] = "a limit below 1e4 is not shipped as a default (DESIGN.md section 21)" if limit < 1e4 else "default limit = tol / eta"
    print(json.dumps(rep, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
