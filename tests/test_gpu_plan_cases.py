"""GPU: the grid planner's kernels (k_plan_clearance, k_plan_seeds, k_plan_travel of vap_plan.hip) on the cluttered scenes,
mazes, full batches and extreme grids of tests/plan_cases.py, against tests/plan_ref.py and tests/occupancy_ref.py.
tests/test_plan_cases_cpu.py shows on the reference alone what each case reaches.

The conventions are those of tests/test_gpu_plan.py, unchanged: every scene first asserts ON THE REFERENCE that no cell has
|clearance - margin| < 1e-9, then asks for the same free mask; from the mask on the distance field (+inf included), flags,
n_vertices and the vertices are the same bits; the clearance, the length and the waypoints lie within max(1e-13, 8 D) of
the float64 reference, D = |float64 - longdouble| of the reference; waypoints 0 and W - 1 are bit copies of the start and
the goal.  Nothing is excused and no cell is left out.  The only sampling is of which problems the CPU reference
recomputes under an occupancy (600 of 2200 seeds, 6 of 70 travel problems), seeded, at least half of them past the first
1024 — the device's results are compared bit for bit among themselves on all of them.

Every test prints the largest |device - reference| and the largest D it has seen so far per quantity, on a line starting
with "PLAN".  On an MI355X: 0 for the clearance, the length and the waypoints of every case (the same bits), against a
largest D of 7.7e-16 ft (clearance), 5.4e-14 ft (length) and 1.1e-13 ft (waypoints, serpentine(19)); the file takes 10 s,
its longest test 1.7 s (DESIGN.md section 15 has the table of cases)."""
import numpy as np
import pytest

import occupancy_ref as oc
import order_ref as orf
import plan_cases as pc
import plan_ref as pr
import test_gpu_plan as tgp
import test_gpu_routine as tgr

pytestmark = pytest.mark.gpu

P, host, bits, within, scene_of, check_problem = tgp.P, tgp.host, tgp.bits, tgp.within, tgp.scene_of, tgp.check_problem
WORST = {k: [0.0, 0.0] for k in ("clearance", "length", "waypoints")}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def note(kind, got, ref, ref_ld):
    """Keep the largest |device - reference| and the largest D of a quantity (``within`` has asserted on them)."""
    ref = np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    if fin.any():
        WORST[kind][0] = max(WORST[kind][0], float(np.abs(np.asarray(got, dtype=np.float64)[fin] - ref[fin]).max()))
        WORST[kind][1] = max(WORST[kind][1], float(np.abs(ref[fin] - np.asarray(ref_ld, dtype=np.longdouble)[fin]).max()))


def report(name):
    print(f"PLAN {name}: so far largest |device - reference| / largest D: " +
          ", ".join(f"{k} {v[0]:.3e} / {v[1]:.3e}" for k, v in WORST.items()))


def check(name, out, r, ref, start, goal, W):
    """Problem r of a device result against its reference dict."""
    check_problem(name, out, r, ref, start, goal, W)
    note("waypoints", out["waypoints"][r], ref["waypoints"], ref["waypoints_ld"])
    note("length", out["length"][r], ref["length"], ref["length_ld"])


def check_grid(name, sc):
    c, ld, free, gap = pc.grids(sc)
    assert gap >= pc.GAP, (name, gap)                                # no cell an ulp could flip
    out = P().clearance_grid(scene_of(sc), sc["cell"], sc["radius"], sc["margin"])
    assert np.array_equal(host(out["free"]), free), name
    within(name + " clearance", host(out["clearance"]), c, ld)
    note("clearance", host(out["clearance"]), c, ld)
    return free


def same_bytes(a, b, what):
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


def rows(out, sl):
    return {k: v[sl] for k, v in out.items()}


# ---------------------------------------------------------------- 1. the grid at every chunk shape

@pytest.mark.parametrize("name", list(pc.CHUNK_CASES))
def test_grid_at_every_chunk_shape(torch_mod, name):
    free = check_grid(name, pc.chunk_scene(name))
    assert free.shape == (48, 48)
    report(name)


# ---------------------------------------------------------------- 2. seeds in clutter

@pytest.mark.parametrize("name", pc.SEEDS_CASES)
def test_seeds_in_clutter(torch_mod, name):
    sc, W = pc.chunk_scene(name), pc.CLUTTER_W
    assert pc.grids(sc)[3] >= pc.GAP
    starts, goals = pc.clutter_problems(name)
    ref, _ = pr.seeds(starts, goals, margin=sc["margin"], W=W, **pr.scene_args(sc))
    out = tgp.device_seeds(sc, starts, goals, W)
    for r in range(len(ref)):
        check(f"{name} problem {r}", out, r, ref[r], starts[r], goals[r], W)
    report("clutter " + name)


# ---------------------------------------------------------------- 3. long lists

@pytest.mark.parametrize("n_walls", list(pc.MAZES))
def test_long_lists(torch_mod, n_walls):
    sc, free, base = pc.maze_reference(n_walls)
    assert len(base["cells"]) > pc.MAZES[n_walls] and base["flags"] == 0
    whole = {}
    for W in pc.MAZE_W:
        out = tgp.device_seeds(sc, sc["start"], sc["goal"], W, max_vertices=128)
        assert out["waypoints"].shape == (1, W, 2)
        check(f"serpentine({n_walls}) W = {W}", out, 0, pc.with_waypoints(sc, base, W), sc["start"], sc["goal"], W)
        whole[W] = out
    if n_walls == 19:                                                # 72 vertices: cut at the default 64, the route unchanged
        W = 33
        cut = tgp.device_seeds(sc, sc["start"], sc["goal"], W)
        ref = pc.with_waypoints(sc, base, W, max_vertices=64)
        assert ref["flags"] == pr.VERTICES_TRUNCATED and int(cut["flags"][0]) == pr.VERTICES_TRUNCATED
        check(f"serpentine({n_walls}) truncated", cut, 0, ref, sc["start"], sc["goal"], W)
        for k in ("waypoints", "length", "n_vertices", "distance"):
            assert np.array_equal(cut[k].view(np.uint8), whole[W][k].view(np.uint8)), k
        assert np.array_equal(bits(cut["vertices"]), bits(whole[W]["vertices"][:, :64]))
    report(f"serpentine({n_walls})")


# ---------------------------------------------------------------- 4. full batches

@pytest.mark.parametrize("seed", pc.BATCH_SEEDS)
def test_full_batches(torch_mod, seed):
    sc, starts, goals, ref, _ = pc.batch_reference(seed)
    R, W = len(starts), pc.BATCH_W
    assert R == 2200
    out = tgp.device_seeds(sc, starts, goals, W)
    for r in range(R):
        check(f"seed {seed} problem {r}", out, r, ref[r], starts[r], goals[r], W)
    same_bytes(out, tgp.device_seeds(sc, starts, goals, W), "repeated")
    for r0 in range(0, R, pc.BLOCKS):                                # no workgroup of these calls takes a second problem
        part = tgp.device_seeds(sc, starts[r0:r0 + pc.BLOCKS], goals[r0:r0 + pc.BLOCKS], W)
        same_bytes(part, rows(out, slice(r0, r0 + pc.BLOCKS)), f"problems from {r0}")
    report(f"full batch {seed}")


# ---------------------------------------------------------------- 5. full batches with an occupancy

@pytest.fixture(scope="module")
def occupied(torch_mod):
    sc, starts, goals, _, free = pc.batch_reference(pc.OCCUPIED_SEED)
    first, last = pc.synthetic_occupancy(free.shape)
    occ = tuple(torch_mod.tensor(a, dtype=torch_mod.int32, device="cuda") for a in (first, last))
    return sc, starts, goals, free, first, last, occ


def occupied_seeds(sc, starts, goals, W, occ, windows):
    out = P().seeds(np.atleast_2d(starts), np.atleast_2d(goals), scene_of(sc), W, sc["radius"], cell=sc["cell"], margin=sc["margin"],
                    vertices=True, distance=True, occupancy=occ, windows=windows)
    return {k: host(v) for k, v in out.items()}


def test_full_batch_with_an_occupancy(torch_mod, occupied):
    sc, starts, goals, free, first, last, occ = occupied
    W, windows = pc.BATCH_W, pc.batch_windows()
    idx = pc.occupied_sample(pc.OCCUPIED_SEED)
    assert len(idx) >= 600 and (idx >= pc.BLOCKS).sum() * 2 >= len(idx)
    ref = pc.occupied_reference(sc, starts, goals, windows, free, first, last, idx)
    out = occupied_seeds(sc, starts, goals, W, occ, windows)
    for r in idx:
        check(f"occupied problem {r}, window {tuple(int(t) for t in windows[r])}", out, r, ref[int(r)], starts[r], goals[r], W)
    same_bytes(out, occupied_seeds(sc, starts, goals, W, occ, windows), "repeated")
    for r in idx[np.linspace(0, len(idx) - 1, 64).astype(int)]:      # single calls with the one window
        one = occupied_seeds(sc, starts[r], goals[r], W, occ, windows[r])
        same_bytes(one, rows(out, slice(r, r + 1)), f"problem {r} alone")
    report("occupied batch")


# ---------------------------------------------------------------- 6. travel with an occupancy over more than 1024 items

def test_travel_with_an_occupancy_over_1120_items(torch_mod, occupied):
    sc, _, _, free, first, last, occ = occupied
    W = pc.TRAVEL_W
    points, windows = pc.travel_problems(pc.OCCUPIED_SEED)
    assert points.shape[0] * points.shape[1] == 1120
    tr = tgr.device_travel(sc, points, W, occupancy=occ, windows=windows)
    tgr.check_against_seeds("travel 70 x 16", sc, points, tr, W, occupancy=occ, windows=windows)
    for r in pc.travel_sample(pc.OCCUPIED_SEED):
        ref = orf.travel(points[r], sc["field"], sc["cell"], oc.window_free(free, first, last, windows[r]), W)
        tgr.check_against_reference(f"travel problem {r}", tr, r, ref)
        note("length", tr["travel"][r], orf.stack(ref, "length"), orf.stack(ref, "length_ld", np.longdouble))
        note("waypoints", tr["waypoints"][r], orf.stack(ref, "waypoints"), orf.stack(ref, "waypoints_ld", np.longdouble))
    same_bytes(tr, tgr.device_travel(sc, points, W, occupancy=occ, windows=windows), "repeated")
    report("travel")


# ---------------------------------------------------------------- 7. extreme grids

@pytest.mark.parametrize("name", list(pc.extreme_cases()))
def test_extreme_grids(torch_mod, name):
    sc, pts, shape = pc.extreme_cases()[name]
    free = check_grid(name, sc)
    assert free.shape == shape and P().grid_shape(scene_of(sc), sc["cell"]) == shape
    W, pairs = 5, pc.pairs_of(len(pts))
    starts, goals = pts[[a for a, _ in pairs]], pts[[b for _, b in pairs]]
    ref = [pr.plan(s, g, sc["field"], sc["cell"], free, W) for s, g in zip(starts, goals)]
    out = tgp.device_seeds(sc, starts, goals, W)
    assert out["distance"].shape[1:] == shape
    for r in range(len(pairs)):
        check(f"{name} pair {pairs[r]}", out, r, ref[r], starts[r], goals[r], W)
    if name.startswith("1x1"):                                       # more problems than workgroups on the one-cell grid, whose
        k = np.arange(pc.BLOCKS + 6) % len(pairs)                     # sums c_0, c_1 need a cell more than the field has
        many = tgp.device_seeds(sc, starts[k], goals[k], W)
        for r in range(len(k)):
            check(f"{name} problem {r}", many, r, ref[k[r]], starts[k[r]], goals[k[r]], W)
    if name == "1x1 blocked":
        assert (out["flags"] == pr.NO_FREE).all() and np.isnan(out["waypoints"]).all()
    for sub in (pts[:2], pts):                                       # P = 2, and all the points
        tr = tgr.device_travel(sc, sub[None], W)
        tgr.check_against_seeds(name, sc, sub[None], tr, W)
        tgr.check_against_reference(f"{name} travel P = {len(sub)}", tr, 0, orf.travel(sub, sc["field"], sc["cell"], free, W))
    report(name)
