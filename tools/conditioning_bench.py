"""Time vap_velocity_conditioning (K = 3) at config 3's shape and at config 5's per-GPU share, beside vap_velocity_pass under
VAP_VELOCITY_SEQ_LITERAL — one probe's chain, a lane per path — on the same fp64 rows in the same process.  Device events,
median of 5 rounds after one warm-up.  Prints one JSON line per shape.

  python tools/conditioning_bench.py [--probes 3] [--rounds 5] [--scratch-mb 512]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vexautonomousplanner_amd import _lib, conditioning  # noqa: E402
from vexautonomousplanner_amd._call import ptr  # noqa: E402
from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator  # noqa: E402
from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, END_VEL, START_VEL, make_waypoints  # noqa: E402

SHAPES = {"config3": (4096, 32, 10000, 3), "config5_share": (131072, 8, 1024, 5)}


def timed(fn, rounds):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scratch-mb", type=int, default=None, help="VAP_OPT_CONDITIONING_SCRATCH_MB (default: the library's 512)")
    args = ap.parse_args()
    L = _lib.lib()
    for name, (B, W, S, seed) in SHAPES.items():
        gen = BatchedTrajectoryGenerator(0, "f64")
        if args.scratch_mb is not None:
            gen.ctx.set_option(_lib.OPT_CONDITIONING_SCRATCH_MB, args.scratch_mb)
        launches = -(-B // max(1, min(B, ((args.scratch_mb or 512) << 20) // ((args.probes + 1) * S * 8))))
        wp = torch.tensor(make_waypoints(B, W, seed), dtype=torch.float64, device=gen.device)
        r = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=S, want=("curvature", "velocity"))
        out = {}
        t_cond, all_cond = timed(lambda: conditioning.probe(r["meta"], r["curvature"], None, probes=args.probes, out=out, ctx=gen.ctx),
                                 args.rounds)
        gen.set_velocity_kernel("seq_literal")
        c = _lib.make_constraints(DEFAULT_CONSTRAINTS)
        vel = torch.empty_like(r["velocity"])

        def literal():
            gen.ctx.set_stream(torch.cuda.current_stream(gen.device).cuda_stream)
            _lib.check(L.vap_velocity_pass(gen.ctx.handle, _lib.VAP_F64, B, S, C.byref(c), START_VEL, END_VEL, ptr(r["meta"]),
                                           ptr(r["curvature"]), None, None, ptr(vel), ptr(r["flags"])), "vap_velocity_pass")
        t_lit, all_lit = timed(literal, args.rounds)
        cond = out["cond"]
        print(json.dumps({"shape": name, "paths": B, "waypoints": W, "samples": S, "probes": args.probes, "launches": launches,
                          "conditioning_ms": round(t_cond, 3), "seq_literal_ms": round(t_lit, 3), "ratio": round(t_cond / t_lit, 3),
                          "conditioning_rounds_ms": [round(x, 3) for x in all_cond], "seq_literal_rounds_ms": [round(x, 3) for x in all_lit],
                          "cond_median": float(cond.median().item()), "cond_max": float(cond.max().item())}), flush=True)
        del gen, r, out, vel, wp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
