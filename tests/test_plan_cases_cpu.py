"""The cases of plan_cases.py on the reference alone (no GPU): they reach what they claim.

test_gpu_plan_cases.py holds the grid planner's kernels to tests/plan_ref.py and tests/occupancy_ref.py on the scenes and
problems of plan_cases.py.  That proves something only while those inputs reach the branches of vap_plan.hip they are
there for; a later change of a seed or a size must not empty them quietly.  So, on the reference alone:
  * no cell of any scene lies within 1e-9 of the margin (nothing is excused; a seed that fails this is moved);
  * the polygon counts are 32, 33, 64, 65 and 256, one chunk is exactly 512 vertex rows, the largest scene is 4096 vertices
    and 256 circles, and the polygons of a second chunk and the circles each change the mask;
  * the mazes trace more than 1026 and more than 2050 cells, relax for more sweeps than that, and the first pull batch of
    1024 candidates sees nothing from the start cell;
  * the full batches have unreachable, clean, many-vertex and two-vertex problems by the hundred, and workgroups whose
    second problem differs in kind from the first, in both orders;
  * the windows of problems r and r + 1024 give different masks; one walls the start off;
  * the extreme grids have the shapes 1 x 1, 1 x 48 and 48 x 1 and the outcomes they are there for.
The floors are caps, not measurements; every test prints what it measured on a line starting with "PLAN"."""
import numpy as np
import pytest

import occupancy_ref as oc
import order_ref as orf
import plan_cases as pc
import plan_ref as pr


def is_strictly_convex_ccw(p):
    e1 = np.roll(p, -1, axis=0) - p
    e2 = np.roll(e1, -1, axis=0)
    cr = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    turn = np.arctan2(cr, (e1 * e2).sum(axis=1)).sum()
    return bool((cr > 1e-12 * np.hypot(*e1.T) * np.hypot(*e2.T)).all()) and abs(turn - 2 * np.pi) < 1e-6


@pytest.mark.parametrize("name", list(pc.CHUNK_CASES))
def test_chunk_scenes(name):
    sc = pc.chunk_scene(name)
    _, n_poly, n_circle, verts = pc.CHUNK_CASES[name]
    counts = [len(p) for p in sc["polygons"]]
    c, ld, free, gap = pc.grids(sc)
    print(f"PLAN {name}: {len(counts)} polygons, {sum(counts)} vertices, {len(sc['circles'])} circles; smallest |clearance - margin| {gap:.3e}; "
          f"{int(free.sum())} of {free.size} cells free; largest D {float(np.abs(c - ld).max()):.3e}")
    assert gap >= pc.GAP and free.shape == (48, 48)
    assert len(counts) == n_poly and len(sc["circles"]) == n_circle and all(is_strictly_convex_ccw(p) for p in sc["polygons"])
    assert np.array_equal(free, ld >= sc["margin"])
    if verts is None:                                                # 3 .. 16 vertices, every eighth polygon a 16-gon
        assert all(n == 16 for n in counts[7::8]) and min(counts) <= 5 and len(set(counts)) >= 8
        if n_poly > 32:                                              # the second chunk's first vertex row: no round number
            assert sum(counts[:32]) % 16 != 0
    else:
        assert counts == [16] * n_poly
    def oblique_edges(p):                                            # edges more than 5 % off both axes
        e = np.roll(p, -1, axis=0) - p
        return int((np.abs(e).min(axis=1) > 0.05 * np.hypot(e[:, 0], e[:, 1])).sum())
    assert sum(1 for p in sc["polygons"] if oblique_edges(p) >= 3) >= 30
    # every chunk of 32 polygons, and the circles, decide cells of their own
    parts = [pr.clearance_grid(**pr.scene_args(dict(sc, polygons=sc["polygons"][k0:k0 + 32], circles=[]))) for k0 in range(0, n_poly, 32)]
    parts.append(pr.clearance_grid(**pr.scene_args(dict(sc, polygons=[]))))      # the walls and the circles
    assert np.array_equal(np.minimum.reduce(parts), c)
    for k in range(len(parts) - 1):
        assert ((np.minimum.reduce(parts[:k] + parts[k + 1:]) >= sc["margin"]) != free).any(), k
    if n_circle:
        assert (np.minimum.reduce(parts[:-1]) >= sc["margin"]).sum() > free.sum()


def test_chunk_counts_and_limits():
    got = {n: (len(pc.chunk_scene(n)["polygons"]), sum(len(p) for p in pc.chunk_scene(n)["polygons"]), len(pc.chunk_scene(n)["circles"]))
           for n in pc.CHUNK_CASES}
    assert sorted({g[0] for g in got.values()}) == [32, 33, 64, 65, 256]
    assert got["32x16gon+0"] == (32, 512, 0) and got["256x16gon+256"] == (256, 4096, 256)
    assert max(g[2] for n, g in got.items() if n != "256x16gon+256") == 40


@pytest.mark.parametrize("name", pc.SEEDS_CASES)
def test_clutter_problems(name):
    sc = pc.chunk_scene(name)
    starts, goals = pc.clutter_problems(name)
    ref, free = pr.seeds(starts, goals, margin=sc["margin"], W=pc.CLUTTER_W, **pr.scene_args(sc))
    clean = sum(1 for r in ref if r["flags"] == 0)
    bent = sum(1 for r in ref if r["n_vertices"] > 2)
    hidden = sum(1 for r in ref if r["n_vertices"] > 2 and not pr.visible(free, r["cells"][0], r["cells"][-1]))
    print(f"PLAN clutter {name}: {len(ref)} problems, {clean} clean, {bent} with more than 2 vertices, up to "
          f"{max(r['n_vertices'] for r in ref)} vertices, {sum(1 for r in ref if r['flags'] & pr.UNREACHABLE)} unreachable")
    assert len(ref) == 48 and clean >= 10 and bent >= 30 and hidden == bent


@pytest.mark.parametrize("n_walls", list(pc.MAZES))
def test_mazes(n_walls):
    sc, free, ref = pc.maze_reference(n_walls)
    cells = ref["cells"]
    goal = pr.cell_of(sc["goal"], sc["field"], sc["cell"])
    d, sweeps = pr.jacobi(free, sc["cell"], goal)
    print(f"PLAN serpentine({n_walls}): smallest |clearance - margin| {pc.grids(sc)[3]:.3e}, {len(cells)} traced cells, {ref['n_vertices']} "
          f"vertices, {sweeps} Jacobi sweeps, length {ref['length']:.4f} ft")
    assert free.shape == (128, 128) and ref["flags"] == 0
    assert len(cells) > pc.MAZES[n_walls] and sweeps > pc.MAZES[n_walls] and ref["n_vertices"] > 2 * n_walls
    assert np.array_equal(d.view(np.int64), ref["distance"].view(np.int64))          # Jacobi reaches Dijkstra's bits
    assert not any(pr.visible(free, cells[0], b) for b in cells[-1024:])             # the first pull batch finds nothing
    if n_walls == 19:
        assert 64 < ref["n_vertices"] <= 128                                           # truncated at the default, whole at 128
        cut = pc.with_waypoints(sc, ref, 2, max_vertices=64)
        assert cut["flags"] == pr.VERTICES_TRUNCATED and np.isfinite(cut["vertices"]).all()
    # with_waypoints is plan_ref.plan at another W
    again = pr.plan(sc["start"], sc["goal"], sc["field"], sc["cell"], free, 33, 128, fields={goal: ref["distance"]}) if n_walls == 9 else None
    if again is not None:
        other = pc.with_waypoints(sc, ref, 33)
        assert all(np.array_equal(np.asarray(again[k]), np.asarray(other[k]), equal_nan=True)
                   for k in ("flags", "n_vertices", "vertices", "waypoints", "length", "waypoints_ld", "length_ld"))


@pytest.mark.parametrize("seed", pc.BATCH_SEEDS)
def test_full_batches(seed):
    sc, starts, goals, ref, free = pc.batch_reference(seed)
    R, fl = len(ref), pc.BATCH_FLOORS
    unreachable = sum(1 for r in ref if r["flags"] & pr.UNREACHABLE)
    clean = sum(1 for r in ref if r["flags"] == 0)
    many = sum(1 for r in ref if r["n_vertices"] > 3)
    two = sum(1 for r in ref if r["n_vertices"] == 2)
    snapped = sum(1 for r in ref if r["flags"] & (pr.SNAPPED_START | pr.SNAPPED_GOAL))
    ok = np.array([pc.kind(r) for r in ref])
    first, second = ok[:pc.BLOCKS], ok[pc.BLOCKS:2 * pc.BLOCKS]
    ok_after_not, not_after_ok = int((~first & second).sum()), int((first & ~second).sum())
    third = int((ok[2 * pc.BLOCKS:] != second[:R - 2 * pc.BLOCKS]).sum())
    print(f"PLAN batch seed {seed}: smallest |clearance - margin| {pc.grids(sc)[3]:.3e}, {int(free.sum())} of {free.size} cells free; of {R} problems "
          f"{unreachable} unreachable, {clean} clean, {snapped} snapped, {many} with more than 3 vertices, {two} with exactly 2, up to "
          f"{max(r['n_vertices'] for r in ref)}; workgroups with a route after none {ok_after_not}, none after a route {not_after_ok}, "
          f"third problem of another kind {third}")
    assert free.shape == (24, 24) and R == 2200 > 2 * pc.BLOCKS
    assert unreachable >= fl["unreachable"] and clean >= fl["clean"] and many >= fl["more_than_3_vertices"] and two >= fl["exactly_2_vertices"]
    assert ok_after_not >= fl["kinds_differ"] and not_after_ok >= fl["kinds_differ"] and third >= 1
    assert ((starts < -3.0) | (starts > 3.0)).any(axis=1).sum() >= 100               # clamped
    # the hand-placed problems, twice: as a workgroup's first problem and as its second
    hp = pc.hand_placed(sc, free)
    for base in (0, pc.BLOCKS + 100):
        got = {name: ref[base + k] for k, (name, _, _, _) in enumerate(hp)}
        assert all(got[n]["flags"] == pr.FLAG_DEGENERATE and got[n]["n_vertices"] == 0 for n in ("nan start", "nan goal", "inf start"))
        assert got["start = goal"]["flags"] == 0 and got["start = goal"]["length"] == 0.0 and got["start = goal"]["n_vertices"] == 2
        assert got["one cell"]["flags"] == 0 and got["one cell"]["n_vertices"] == 2 and len(got["one cell"]["cells"]) == 1
        assert got["start inside an obstacle"]["flags"] & pr.SNAPPED_START and got["goal inside an obstacle"]["flags"] & pr.SNAPPED_GOAL
        assert got["both inside one obstacle"]["flags"] & (pr.SNAPPED_START | pr.SNAPPED_GOAL) == pr.SNAPPED_START | pr.SNAPPED_GOAL
        for k, (name, _, _, _) in enumerate(hp):
            assert np.array_equal(starts[base + k], starts[k], equal_nan=True) and np.array_equal(goals[base + k], goals[k], equal_nan=True)
    # an early end and a route share a workgroup, in both orders
    partner = [pc.kind(ref[k]) != pc.kind(ref[k + pc.BLOCKS]) for k in range(len(hp))]
    before = [pc.kind(ref[k + 100]) != pc.kind(ref[k + 100 + pc.BLOCKS]) for k in range(len(hp))]
    assert all(partner[:3]) and all(before[:3]) and ref[pc.BLOCKS]["n_vertices"] > 3 and ref[100]["n_vertices"] > 3
    # a snap whose nearest free cell is a tie decided by the lower index
    xs, ys = pr.centres(sc["field"], sc["cell"])
    ties = 0
    for r, s, g in zip(ref, starts, goals):
        for bit, p in ((pr.SNAPPED_START, s), (pr.SNAPPED_GOAL, g)):
            if r["flags"] & bit and np.isfinite(p).all():
                d2 = np.where(free, (xs[None, :] - p[0]) ** 2 + (ys[:, None] - p[1]) ** 2, np.inf)
                ties += int((d2 == d2.min()).sum() > 1)
    print(f"PLAN batch seed {seed}: {ties} snaps decided by the tie rule")
    assert ties >= 1


def window_masks(free, first, last):
    return [oc.window_free(free, first, last, w) for w in pc.WINDOW_SET]


def test_occupied_batches():
    sc, starts, goals, static_ref, free = pc.batch_reference(pc.OCCUPIED_SEED)
    first, last = pc.synthetic_occupancy(free.shape)
    masks = window_masks(free, first, last)
    names = [m.tobytes() for m in masks]
    assert len(set(names)) == len(names)                             # every window its own mask
    assert np.array_equal(masks[0], free) and pc.WINDOW_SET[0][0] == pc.WINDOW_SET[0][1]           # the empty window
    assert pc.WINDOW_SET[1] == (oc.INT_MIN, oc.INT_MAX) and np.array_equal(masks[1], free & ~(first <= last))
    windows = pc.batch_windows()
    R = len(starts)
    assert all(tuple(windows[r]) != tuple(windows[r + pc.BLOCKS]) for r in range(R - pc.BLOCKS))
    idx = pc.occupied_sample(pc.OCCUPIED_SEED)
    assert len(idx) >= 600 and len(set(idx.tolist())) == len(idx) and (idx >= pc.BLOCKS).sum() * 2 >= len(idx)
    ref = pc.occupied_reference(sc, starts, goals, windows, free, first, last, idx)
    # a window walls the start off: a route in the static scene, none behind the column
    walled = [r for r in idx if pc.kind(static_ref[r]) and ref[r]["flags"] & pr.UNREACHABLE and not masks[pc.WINDOW_SET.index(tuple(windows[r]))][:, pc.WALL_COLUMN].any()]
    changed = sum(1 for r in idx if pc.kind(ref[r]) and pc.kind(static_ref[r]) and ref[r]["length"] != static_ref[r]["length"])
    differ = sum(1 for r in idx if r + pc.BLOCKS in ref and pc.kind(ref[r]) != pc.kind(ref[r + pc.BLOCKS]))
    print(f"PLAN occupied batch: {len(idx)} sampled, {sum(1 for r in idx if pc.kind(ref[r]))} with a route, {len(walled)} walled off by the column, "
          f"{changed} routes of another length than in the static scene, {differ} sampled workgroups whose two problems differ in kind; "
          f"cells free per window {[int(m.sum()) for m in masks]}")
    assert len(walled) >= 20 and changed >= 50 and differ >= 3
    assert sum(1 for r in idx if pc.kind(ref[r])) >= 200


def test_travel_problems():
    sc, _, _, _, free = pc.batch_reference(pc.OCCUPIED_SEED)
    points, windows = pc.travel_problems(pc.OCCUPIED_SEED)
    assert points.shape == (70, 16, 2) and points.shape[0] * points.shape[1] == 1120 > pc.BLOCKS
    items = np.arange(1120)
    r_of = items // 16
    assert all(tuple(windows[r_of[it]]) != tuple(windows[r_of[it + pc.BLOCKS]]) for it in range(1120 - pc.BLOCKS))
    sample = pc.travel_sample(pc.OCCUPIED_SEED)
    assert len(sample) == pc.TRAVEL_REFERENCE_PROBLEMS and (sample >= 64).sum() == 3 and len(set(sample.tolist())) == 6
    first, last = pc.synthetic_occupancy(free.shape)
    r = int(sample[-1])
    ref = orf.travel(points[r], sc["field"], sc["cell"], oc.window_free(free, first, last, windows[r]), pc.TRAVEL_W)
    fl = orf.stack(ref, "flags", np.int64)
    nv = orf.stack(ref, "n_vertices", np.int64)
    print(f"PLAN travel problem {r}, window {tuple(int(t) for t in windows[r])}: {int((nv > 0).sum())} of 240 pairs with a route, {int((fl & pr.UNREACHABLE > 0).sum())} "
          f"unreachable, up to {int(nv.max())} vertices")
    assert (nv > 2).sum() >= 20


@pytest.mark.parametrize("name", list(pc.extreme_cases()))
def test_extreme_grids(name):
    sc, pts, shape = pc.extreme_cases()[name]
    c, ld, free, gap = pc.grids(sc)
    assert gap >= pc.GAP and free.shape == shape and pr.grid_shape(sc["field"], sc["cell"]) == shape[::-1]
    pairs = pc.pairs_of(len(pts))
    ref = [pr.plan(pts[a], pts[b], sc["field"], sc["cell"], free, 5) for a, b in pairs]
    flags = [r["flags"] for r in ref]
    print(f"PLAN {name}: smallest |clearance - margin| {gap:.3e}, {int(free.sum())} of {free.size} cells free, flags {sorted(set(flags))}, "
          f"up to {max(len(r['cells']) for r in ref)} traced cells")
    if name == "1x1":
        assert free.all() and all(f == 0 and r["n_vertices"] == 2 and len(r["cells"]) == 1 for f, r in zip(flags, ref))
    elif name == "1x1 blocked":
        assert not free.any() and set(flags) == {pr.NO_FREE}
    elif name.endswith("plug"):
        assert (~free).sum() == 1 and not free.reshape(-1)[28]
        assert any(f & pr.UNREACHABLE for f in flags) and any(f == 0 for f in flags)
        out = ref[pairs.index((2, 0))]                               # out of the blocked cell's centre: cells 27 and 29 tie
        assert out["flags"] == pr.SNAPPED_START and out["cells"][0] == ((27, 0) if shape[0] == 1 else (0, 27))
        assert ref[pairs.index((2, 1))]["flags"] == pr.SNAPPED_START | pr.UNREACHABLE
    else:
        assert free.all() and set(flags) == {0}
        assert max(len(r["cells"]) for r in ref) == 48 and all(r["n_vertices"] == 2 for r in ref)
