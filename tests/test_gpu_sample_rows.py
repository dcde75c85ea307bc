"""The sampler's rows are pinned bit for bit: sha256 prefixes of every output of small seeded batches, recorded from the
build before the sampler's table search and walk were straight-lined (they must not move a bit: the fp64 side rows feed
an amplifying recurrence, and the index path rounds like NumPy's)."""
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints  # noqa: E402

PINNED = {
    # (B, W, S, seed, dtype): {output: sha256(bytes)[:16]}
    (64, 5, 3001, 11, "f32"): {"curvature": "a1f694c6b5a9144c", "heading": "2baf229d4b729c74", "velocity": "0b290f8f6ae105d6",
                               "x": "773666ba7adbe766", "y": "cc06472d64b991ee"},
    (64, 5, 3001, 11, "f64"): {"curvature": "5f6c90089a766300", "heading": "b69b3934ea0afc59", "velocity": "c5f90375d01cca34",
                               "x": "93287028e67329e4", "y": "2e577885aa6cb038"},
    (16, 8, 513, 15, "f32"): {"curvature": "36ca89a5aa953f7f", "heading": "5b16821c557b3afe", "velocity": "55c90e252c0ece9b",
                              "x": "dfdaa4fdcb73f404", "y": "d60d71f83b727ba0"},
    (37, 40, 2047, 12, "f32"): {"curvature": "b0e2bb37a4321928", "heading": "1e97b7fe83ff1a6f", "velocity": "0653f5c68abdbcec",
                                "x": "09256653402a2a8c", "y": "4417deda77dd41b8"},
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(PINNED), ids=lambda c: "B%d_W%d_S%d_%s" % (c[0], c[1], c[2], c[4]))
def test_sample_rows_are_pinned(case):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    B, W, S, seed, dt = case
    tdt = torch.float32 if dt == "f32" else torch.float64
    wp = torch.tensor(make_waypoints(B, W, seed), dtype=tdt, device="cuda:0")
    out = BatchedTrajectoryGenerator(0, dt).profile(wp, constraints=DEFAULT_CONSTRAINTS, samples=S)
    torch.cuda.synchronize()
    got = {k: hashlib.sha256(np.ascontiguousarray(out[k].cpu().numpy()).tobytes()).hexdigest()[:16] for k in PINNED[case]}
    assert got == PINNED[case]
