"""Timing shared by the tools/*_bench.py scripts."""
import numpy as np
import torch


def timed(fn, reps, rounds):
    """(median_ms, rounds_ms) of ``fn()``: one warm-up call (code objects, buffers), then ``rounds`` times ``reps`` calls
    back to back between two device events; a round's figure is its time per call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return float(np.median(ts)), [float(t) for t in ts]
