#!/usr/bin/env python3
"""Range-sensor timings (vap_range_readings; sensors.py; include/vap.h).

The config-3 batch: 4096 paths of 32 waypoints, 10 000 samples, its time-domain rows at dt = 0.01 s with 2048 rows of
capacity (about 5.2 M rows), every route moved so that its extent is centred on the field (as generated the routes leave
it: tools/footprint_bench.py); the scene of that bench — walls, 8 convex polygons, 4 circles — and four sensors (front, back,
left, right).  Each call is timed with device events over --reps calls after a warm-up and repeated --rounds times, in this
one process (the median is reported, the rounds are listed):

  summary_ms            sensors.readings into reused buffers, summaries only, culling on;  summary_nocull_ms: culling off
  per_row_ms            with the per-reading outputs (range, cos_incidence, code), culling on;  per_row_nocull_ms: off
  partners_ms           summaries only, with 8 partner routines (the batch's first 8 routes) in the beams
  clearance_ms          vap_footprint_clearance of an 18 x 18 in robot on the same rows and scene, culling on
  copy_summary_ms       a torch device copy that moves as many bytes as the call must for the summaries: the 24 bytes of
                        columns 4, 6, 7 per row (the copy reads 12 and writes 12; the rows are 64-byte records, so the call
                        itself fetches whole 64-byte lines: copy_lines_ms moves 64 per row)
  copy_per_row_ms       likewise with the per-reading outputs: 24 read and 20 n_sens written per row

    python tools/range_bench.py [--reps 10] [--rounds 5] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, W, S, CAP, DT = 4096, 32, 10000, 2048, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from _timing import timed
    from footprint_bench import field_scene
    from vexautonomousplanner_amd import footprint as fp, sensors
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

    assert torch.cuda.is_available(), "range_bench needs a HIP device"
    gen = BatchedTrajectoryGenerator(0, "f32")
    dev = gen.device
    wp = torch.tensor(make_waypoints(B, W, 3), device=dev)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=S)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, dt=DT, capacity_rows=CAP)
    rows, counts = tp["rows"].clone(), tp["counts"]
    valid = torch.arange(CAP, device=dev)[None, :] < counts[:, :1]
    xy = rows[..., 6:8]
    lo = torch.where(valid[..., None], xy, torch.full_like(xy, float("inf"))).amin(dim=1)
    hi = torch.where(valid[..., None], xy, torch.full_like(xy, -float("inf"))).amax(dim=1)
    rows[..., 6:8] -= ((lo + hi) / 2)[:, None, :]
    n_rows = int(counts[:, 0].sum().item())
    scene = field_scene()
    sens = [sensors.Sensor(7.0, 0.0, 0, (1.0, 80.0), 60.0), sensors.Sensor(-7.0, 0.0, 180, (1.0, 80.0), 60.0),
            sensors.Sensor(0.0, 7.0, 90, (1.0, 80.0), 60.0), sensors.Sensor(0.0, -7.0, 270, (1.0, 80.0), 60.0)]
    ns = len(sens)
    out = {"paths": B, "capacity_rows": CAP, "rows": n_rows, "sensors": ns, "polygons": scene.n_polygons,
           "polygon_vertices": int(scene.poly_start[-1]), "circles": scene.n_circles, "reps": a.reps, "rounds": a.rounds}
    bufs = {k: {} for k in ("s", "sn", "r", "rn", "p")}
    call = lambda key, **kw: sensors.readings(rows, counts, sens, scene, out=bufs[key], ctx=gen.ctx, **kw)
    out["summary_ms"], out["summary_rounds_ms"] = timed(lambda: call("s"), a.reps, a.rounds)
    out["summary_nocull_ms"], out["summary_nocull_rounds_ms"] = timed(lambda: call("sn", cull=False), a.reps, a.rounds)
    out["per_row_ms"], out["per_row_rounds_ms"] = timed(lambda: call("r", per_row=True), a.reps, a.rounds)
    out["per_row_nocull_ms"], out["per_row_nocull_rounds_ms"] = timed(lambda: call("rn", per_row=True, cull=False), a.reps, a.rounds)
    foot = fp.rectangle(18, 18)
    partners = dict(others=rows[:8], others_counts=counts[:8], others_footprint=foot)
    out["partners_ms"], out["partners_rounds_ms"] = timed(lambda: call("p", **partners), a.reps, a.rounds)
    same = lambda x, y, keys: all(torch.equal(x[k].view(torch.int64 if x[k].dtype == torch.float64 else torch.int32),
                                              y[k].view(torch.int64 if y[k].dtype == torch.float64 else torch.int32)) for k in keys)
    summary_keys = ("status_counts", "range_minmax", "channels")
    out["cull_same_bits"] = same(bufs["s"], bufs["sn"], summary_keys) and same(bufs["r"], bufs["rn"], summary_keys + ("range", "cos_incidence", "code"))
    out["per_row_same_summaries"] = same(bufs["s"], bufs["r"], summary_keys)
    sc = bufs["s"]["status_counts"].sum(dim=(0, 1)).tolist()
    out["readings_per_status"] = sc[:7]
    out["readings_blocked_with_partners"] = int(bufs["p"]["status_counts"][..., 5].sum().item())
    ch = bufs["s"]["channels"]
    out["routes_x_observable_somewhere"] = int((ch[:, ns, 0] > 0).sum().item())
    out["median_blind_rows_x"] = float(ch[:, ns, 3].double().median().item())
    cb = {}
    out["clearance_ms"], out["clearance_rounds_ms"] = timed(lambda: fp.clearance(rows, counts, foot, scene, out=cb, ctx=gen.ctx), a.reps, a.rounds)
    src = torch.empty(12 * n_rows, dtype=torch.uint8, device=dev)                         # a copy reads and writes each byte
    dst = torch.empty_like(src)
    out["copy_summary_ms"], out["copy_summary_rounds_ms"] = timed(lambda: dst.copy_(src), a.reps, a.rounds)
    src1 = torch.empty(32 * n_rows, dtype=torch.uint8, device=dev)
    dst1 = torch.empty_like(src1)
    out["copy_lines_ms"], out["copy_lines_rounds_ms"] = timed(lambda: dst1.copy_(src1), a.reps, a.rounds)
    src2 = torch.empty((24 + 20 * ns) // 2 * n_rows, dtype=torch.uint8, device=dev)
    dst2 = torch.empty_like(src2)
    out["copy_per_row_ms"], out["copy_per_row_rounds_ms"] = timed(lambda: dst2.copy_(src2), a.reps, a.rounds)
    out["readings_per_s"] = ns * n_rows / (out["summary_ms"] * 1e-3)
    out["summary_over_clearance"] = out["summary_ms"] / out["clearance_ms"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
