#!/usr/bin/env python3
"""Routine-timeline timings (vap_routine_timeline; timeline.chain; include/vap.h).

The legs are the time-domain rows of the config-3 batch (4096 paths of 32 waypoints, 10 000 samples, dt = 0.01 s, 2048 rows
of capacity); R = 1024 routines of M = 4 random legs each, and R = 1 with M = 4, every slot with a dwell of 0.3 s and a start
heading, so every slot has its three blocks.  Each call is timed with device events over --reps calls after a warm-up and
repeated --rounds times (the median is reported, the rounds are listed):

  chain_ms         timeline.chain into reused buffers: the call as a user makes it (k_routine_timeline, the flag reset and
                   the arrival / duration tensors)
  bytes            what the call has to move: 64 bytes read per leg row and 64 bytes written per output row
  chain_gbs        bytes / chain_ms
  copy_ms, copy_gbs  a plain torch device copy that moves the same number of bytes (half read, half written), in the same run:
                   what the figure is read against.  There is no target.

    python tools/timeline_bench.py [--reps 50] [--rounds 5] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, DWELL, DT = 4, 0.3, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from _timing import timed
    from vexautonomousplanner_amd import timeline
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "timeline_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    wp = torch.tensor(make_waypoints(4096, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, dt=DT, capacity_rows=2048)
    L = int(tp["rows"].shape[0])
    out = {"legs": L, "leg_rows": int(tp["counts"][:, 0].sum().item()), "slots": M, "dwell_s": DWELL, "dt": DT, "reps": a.reps,
           "rounds": a.rounds}

    rng = np.random.default_rng(7)
    for R in (1, 1024):
        legs = torch.as_tensor(rng.integers(0, L, (R, M)).astype(np.int32), device=gen.device)
        start = torch.as_tensor(rng.uniform(-3.0, 3.0, R), device=gen.device)
        dwell = np.full((R, M), DWELL)
        buf = {}
        call = lambda: timeline.chain(tp["rows"], tp["counts"], legs, dwell=dwell, start_heading=start, dt=DT, out=buf, ctx=gen.ctx)
        d = call()
        torch.cuda.synchronize()
        assert int(d["flags"].max().item()) == 0
        rows_out = int(d["counts"][:, 0].sum().item())
        rows_in = int(tp["counts"][:, 0][legs.long()].sum().item())
        nbytes = 64 * (rows_in + rows_out)
        dwell_d = torch.as_tensor(dwell, device=gen.device)    # as a device tensor: no upload inside the timed call
        cap = int(d["rows"].shape[1])
        call = lambda: timeline.chain(tp["rows"], tp["counts"], legs, dwell=dwell_d, start_heading=start, dt=DT, capacity_rows=cap,
                                      out=buf, ctx=gen.ctx)
        c_ms, c_rounds = timed(call, a.reps, a.rounds)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=gen.device)
        dst = torch.empty_like(src)
        p_ms, p_rounds = timed(lambda: dst.copy_(src), a.reps, a.rounds)
        out[f"r{R}"] = {"rows_in": rows_in, "rows_out": rows_out, "bytes": nbytes, "chain_ms": c_ms, "chain_rounds_ms": c_rounds,
                        "chain_gbs": nbytes / c_ms / 1e6, "copy_ms": p_ms, "copy_rounds_ms": p_rounds, "copy_gbs": nbytes / p_ms / 1e6}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
