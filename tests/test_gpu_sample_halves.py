"""The sampler evaluates a thread's four consecutive samples as two pairs ({0,1} then {2,3}).  Every output of the
smallest shapes at which such a split can go wrong is pinned bit for bit — sha256 prefixes recorded on the GPU from the
build before the split (tests/golden/sample_halves_hashes.json; `python tests/test_gpu_sample_halves.py OUT.json`
records them from the build in the tree) — and, where the oracle covers the shape, held to the tolerances of
test_gpu_parity.py as well.

Shapes (B = 3 paths, default constraints, unless said otherwise; a tile is 1020 written samples, a thread has 4):
  S = 4, 5              one thread, with and without the 16-byte store
  S = 1019, 1020        one tile, unaligned and aligned
  S = 1021              a second tile of one sample: the neighbour hand-over across tiles
  S = 2041              three tiles: first / middle / last (also in the fp64 and the all-fp32 modes)
  S = 3064              aligned rows of four tiles: the second takes the kernel's interior-tile body
  W = 2, 5              the shortest paths
  W = 115               coefficient blocks outside LDS (more than kLdsCoefSegments = 112 segments)
  dd = 0.0046           the reference's grid, rows of 3072 and 3071: paths of 942, 849 and 1062 samples — the last sample is
                        sample 1 of its thread (942, and 1062 in the second tile) or sample 0 (849) — and zero-filled tiles
  B = 8192, S = 1024, W = 8   the two-paths-per-workgroup instantiation
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sample_halves_hashes.json")
ROWS = ("x", "y", "heading", "curvature", "velocity")
DD, DD_N = 0.0046, (942, 849, 1062)

# id: (B, W, seed, mode, grid) with grid = ("S", samples) or ("dd", dd, capacity)
CASES = {
    "S4": (3, 8, 61, "f32", ("S", 4)),
    "S5": (3, 8, 61, "f32", ("S", 5)),
    "S1019": (3, 8, 61, "f32", ("S", 1019)),
    "S1020": (3, 8, 61, "f32", ("S", 1020)),
    "S1021": (3, 8, 61, "f32", ("S", 1021)),
    "S2041": (3, 8, 61, "f32", ("S", 2041)),
    "S2041_f64": (3, 8, 61, "f64", ("S", 2041)),
    "S2041_f32r32": (3, 8, 61, "f32r32", ("S", 2041)),
    "S3064": (3, 8, 61, "f32", ("S", 3064)),
    "W2_S1021": (3, 2, 62, "f32", ("S", 1021)),
    "W5_S1021": (3, 5, 63, "f32", ("S", 1021)),
    "W115_S2041": (3, 115, 64, "f32", ("S", 2041)),
    "dd_cap3072": (3, 8, 61, "f32", ("dd", DD, 3072)),
    "dd_cap3071": (3, 8, 61, "f32", ("dd", DD, 3071)),
    "B8192_S1024_W8": (8192, 8, 65, "f32", ("S", 1024)),
}
TOL = {"f32": 1e-5, "f32r32": 1e-5, "f64": 1e-9}


def _waypoints(case):
    from vexautonomousplanner_amd.synth import make_waypoints
    B, W, seed = CASES[case][:3]
    return make_waypoints(B, W, seed)


@functools.lru_cache(maxsize=None)
def run_case(case):
    """The rows, meta and flags of one case as NumPy arrays (read-only; shared by the tests of the case)."""
    import torch
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    mode, grid = CASES[case][3:]
    gen = BatchedTrajectoryGenerator(0, "f64" if mode == "f64" else "f32", recurrence="f32" if mode == "f32r32" else "f64")
    wp = torch.tensor(_waypoints(case), dtype=gen.tdtype, device="cuda:0")
    if grid[0] == "S":
        out = gen.profile(wp, constraints=DEFAULT_CONSTRAINTS, samples=grid[1])
    else:
        out = gen.profile(wp, constraints=DEFAULT_CONSTRAINTS, dd=grid[1], capacity=grid[2])
    torch.cuda.synchronize()
    got = {k: np.ascontiguousarray(out[k].cpu().numpy()) for k in ROWS + ("meta", "flags")}
    for a in got.values():
        a.setflags(write=False)
    return got


def hashes_of(got):
    return {k: hashlib.sha256(got[k].tobytes()).hexdigest()[:16] for k in sorted(got)}


def check_fields(got, ref, tol, what):
    """The measures of test_gpu_parity.py."""
    g = {k: np.asarray(got[k], dtype=np.float64) for k in ROWS}
    e = {"v": np.max(np.abs(g["velocity"] - ref["velocity"]) / np.abs(ref["velocity"])),
         "k": np.max(np.abs(g["curvature"] - ref["curvature"]) / np.maximum(np.abs(ref["curvature"]), 1e-2)),
         "h": np.max(np.abs(g["heading"] - ref["heading"])) / np.pi,
         "x": np.max(np.abs(g["x"] - ref["x"]) / np.maximum(np.abs(ref["x"]), 1.0)),
         "y": np.max(np.abs(g["y"] - ref["y"]) / np.maximum(np.abs(ref["y"]), 1.0))}
    msg = what + ": " + " ".join(f"{k} {v:.2e}" for k, v in e.items())
    print(msg)
    assert np.all(np.isfinite(g["velocity"])) and all(v <= tol for v in e.values()), msg


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_rows_equal_the_build_before_the_split(case):
    with open(FIXTURE) as f:
        pinned = json.load(f)
    got = run_case(case)
    assert not got["flags"].any()
    assert hashes_of(got) == pinned[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][4][0] == "S"])
def test_rows_against_the_oracle(case):
    from oracle import oracle
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    B, _, _, mode, grid = CASES[case]
    n = min(B, 64)          # (the big batch: its first paths — a path's rows do not depend on its place in the batch)
    got = run_case(case)
    ref = oracle.profile_batch(_waypoints(case)[:n].astype(np.float64), grid[1], DEFAULT_CONSTRAINTS, n_threads=8)
    np.testing.assert_allclose(got["meta"][:n, 1], ref["total_length"], rtol=1e-14)
    check_fields({k: got[k][:n] for k in ROWS}, ref, TOL[mode], case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][4][0] == "dd"])
def test_ragged_rows_against_the_oracle(case):
    """Paths that end mid-thread, and the zero-filled tiles past them."""
    from oracle import oracle
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    got = run_case(case)
    wp = _waypoints(case).astype(np.float64)
    assert tuple(got["meta"][:, 3].astype(int)) == DD_N
    assert DD_N[0] % 4 == 2 and (DD_N[2] - 1020) % 4 == 2 and DD_N[1] % 4 == 1
    for b, N in enumerate(DD_N):
        p = oracle.OraclePath(wp[b])
        p.rebuild_tables()
        ref = p.forward_backward(DEFAULT_CONSTRAINTS, DD)
        assert len(ref["velocity"]) == N
        check_fields({k: got[k][b][:N] for k in ROWS}, ref, 1e-5, f"{case} path {b}")
        for k in ROWS:
            assert not got[k][b][N:].any(), (k, b)


if __name__ == "__main__":
    # record the fixture from the build in the tree
    sys.path.insert(0, os.path.dirname(HERE))
    rec = {}
    for c in CASES:
        rec[c] = hashes_of(run_case(c))
        print(c, rec[c], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
