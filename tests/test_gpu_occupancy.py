"""GPU: vap_plan_occupancy and vap_plan_seeds_occupied (plan.occupancy, plan.seeds(occupancy=, windows=),
BatchedTrajectoryGenerator.plan_occupancy) against the NumPy reference of tests/occupancy_ref.py and tests/plan_ref.py, and
end to end into the route search.

What is exact and what is not.  A row covers a cell iff clearance < margin: every test first asserts ON THE REFERENCE that
no (row, cell) pair has |clearance - margin| < 1e-9, so an ulp (the device's sincos against NumPy's sin and cos) cannot
flip a pair, and then asks for first, last, count and blocked bit for bit.  min_clearance involves sincos, sqrt and a
division: within max(1e-13, 8 D) of the float64 reference, D = |float64 - longdouble| of the reference (the convention of
tests/test_gpu_plan.py).  From the occupancy on, the windowed free mask is integer comparisons, so the seeds compare as in
test_gpu_plan.py: flags, n_vertices, vertices and the distance field bit for bit, waypoints and length within the convention.

End to end (the reference loop of tests/search_ref.py on the CPU with an evaluate that adds tests/conflict_ref.py's clearance;
oracle + NumPy; scene B of plan_ref, W = 9, N = 64, E = 8, alpha 0.7, 12 iterations, sigma0 = 0.5 ft, an 18 x 18 in robot,
clearance margin 0.1 ft, conflict margin 0.05 ft; the partner, the same robot, parked for good at (0.143, 1.324), heading 0,
on the static seed, which passes the post on its north side; the planner's disc 0.75 ft with 0.1 ft of margin for the scene
and for the occupancy alike — neither had to be changed):
  planned seed (south of the post, 4 vertices, 8.7443 ft): cost 1 000 042.4 (clearance 0.0608 ft: the disc is not the
    square; conflict clearance 1.05 ft), feasible from the 1st iteration (5 of 64), 64 of 64 from the 8th, 3.1688 s after 12;
    the best route alone clears the partner by 1.20 ft.
  static seed (north, through the partner): cost 1 001 583.2, conflict clearance -1.4952 ft; the reference loop stays
    infeasible for 8 iterations and ends at 5.1414 s.  The device test asserts nothing about refine from this seed."""
import numpy as np
import pytest

import conflict_ref as cr
import occupancy_ref as oc
import plan_ref as pr
import test_gpu_footprint as tgf
import test_gpu_plan as tgp

pytestmark = pytest.mark.gpu

S = oc.CROSSING
GRIDS = {"48x48": pr.FIELD, "48x38": (-6.0, -3.5, 6.0, 6.0), "ragged": (-6.0, -6.0, 5.9, 6.0)}
TRIANGLE = np.array([[0.9, 0.0], [-0.45, 0.6], [-0.45, -0.7]])
GON16 = np.array([[0.8 * np.cos(a + 0.1), 0.7 * np.sin(a + 0.1)] for a in 2 * np.pi * np.arange(16) / 16])
KEYS = ("first", "last", "count")
P, host, bits, within, scene_of = tgp.P, tgp.host, tgp.bits, tgp.within, tgp.scene_of
WORST = {"diff": 0.0, "D": 0.0}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def east_rows(n=217, x0=-4.0, step=0.031):
    return oc.make_rows(x0 + step * np.arange(n), np.full(n, 1.003), np.full(n, 0.02))


def padded(routes, cap):
    rows = np.full((len(routes), cap, 8), np.nan)
    for b, r in enumerate(routes):
        rows[b, :len(r)] = r[:cap]
    return rows


def field_scene(field):
    from vexautonomousplanner_amd import footprint as fp
    return fp.Scene(field=field)


def device_occ(rows, counts, foot, field, cell=S["cell"], **kw):
    a = dict(radius=S["radius"], margin=S["margin"], min_clearance=True)
    a.update(kw)
    radius = a.pop("radius")
    out = P().occupancy(rows, counts, foot, field_scene(field), cell, radius, **a)
    return {k: host(v) for k, v in out.items()}


def check_occupancy(name, got, rows, counts, foot, field, cell=S["cell"], **kw):
    """The device's dict against the reference; the reference's own gap first."""
    a = dict(footprint=foot, field=field, cell=cell, radius=S["radius"], margin=S["margin"])
    a.update(kw)
    ref = oc.occupancy(rows, counts, **a)
    assert ref["gap"] >= 1e-9, (name, ref["gap"])                    # no pair an ulp could flip
    for k in KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (name, k)
    assert got["blocked"].dtype == np.bool_ and np.array_equal(got["blocked"], ref["blocked"]), name
    if "min_clearance" in got:
        ld = oc.occupancy(rows, counts, ftype=np.longdouble, **a)
        for k in KEYS:
            assert np.array_equal(ld[k], ref[k]), (name, k)
        d = within(name + " min_clearance", got["min_clearance"], ref["min_clearance"], ld["min_clearance"])
        fin = np.isfinite(ref["min_clearance"])
        WORST["diff"] = max(WORST["diff"], d)
        if fin.any():
            WORST["D"] = max(WORST["D"], float(np.abs(ref["min_clearance"][fin] - ld["min_clearance"][fin]).max()))
        print(f"{name}: gap {ref['gap']:.3e}, {int(ref['blocked'].sum())} cells covered; so far largest difference {WORST['diff']:.3e}, D {WORST['D']:.3e}")
    return ref


# ---------------------------------------------------------------- parity with the reference

@pytest.mark.parametrize("grid", list(GRIDS))
def test_crossing_partner(torch_mod, grid):
    rows = oc.crossing_rows()[None]
    got = device_occ(rows, [217], oc.SQUARE, GRIDS[grid])
    ref = check_occupancy("crossing " + grid, got, rows, [217], oc.SQUARE, GRIDS[grid])
    if grid == "48x48":
        assert ref["blocked"].sum() == 457 and abs(ref["gap"] - 1.16e-4) < 1e-6
    # without the minimum the kernel visits the covered box only: the same integers
    lean = device_occ(rows, [217], oc.SQUARE, GRIDS[grid], min_clearance=False)
    assert "min_clearance" not in lean
    for k in KEYS + ("blocked",):
        assert np.array_equal(lean[k], got[k]), k


@pytest.mark.parametrize("grid", list(GRIDS))
def test_three_routes_one_empty_one_count_above_capacity(torch_mod, grid):
    rows = padded([oc.crossing_rows(), oc.crossing_rows()[:40], east_rows()], 217)
    counts = np.array([[217, 7], [0, 7], [100000, 7]], dtype=np.int32)              # stride 2; 0 rows; clamped to 217
    got = device_occ(rows, counts, oc.SQUARE, GRIDS[grid], hold_first=True, shift_rows=-7)
    check_occupancy("three routes " + grid, got, rows, counts[:, 0], oc.SQUARE, GRIDS[grid], hold_first=True, shift_rows=-7)


@pytest.fixture(scope="module", params=["feat_turn", "feat_reverse"])
def golden_route(torch_mod, request):
    """The device's own time_profile and insert_waits rows of a golden route with a turn node (in-place turn rows) and of one
    with a reverse node (the heading is the direction of travel turned by pi), moved onto the field."""
    gen, g, tp, out = tgf.full_rows(torch_mod, request.param, copies=1)
    moved = []
    for d in (tp, out):
        rows = d["rows"].clone()
        rows[:, :, 6] += 5.013
        rows[:, :, 7] += 2.507
        moved.append({"rows": rows, "counts": d["counts"]})
    return request.param, gen, moved


@pytest.mark.parametrize("grid", list(GRIDS))
def test_golden_route_rows_of_the_device(torch_mod, golden_route, grid):
    route, gen, moved = golden_route
    for name, d in zip(("time_profile", "insert_waits"), moved):                       # counts of stride 2 and of stride 3
        rows, n = host(d["rows"]), int(d["counts"][0, 0])
        r = rows[0, :n]
        turning, reversed_ = int(((r[:, 2] == 0) & (np.abs(r[:, 5]) > 0)).sum()), int((r[:, 2] < 0).sum())
        if name == "insert_waits":
            assert turning > 0 if route == "feat_turn" else reversed_ > 0
        out = gen.plan_occupancy(d, oc.SQUARE, field_scene(GRIDS[grid]), S["cell"], S["radius"], margin=S["margin"], min_clearance=True)
        got = {k: host(v) for k, v in out.items()}
        check_occupancy(f"{route} {name} {grid} ({n} rows, {turning} turning, {reversed_} reversed)", got, rows, [n], oc.SQUARE, GRIDS[grid])


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("foot", ["triangle", "16-gon"])
def test_other_footprints(torch_mod, grid, foot):
    f = TRIANGLE if foot == "triangle" else GON16
    rows = padded([oc.crossing_rows(), east_rows(130)], 217)
    got = device_occ(rows, [217, 130], f, GRIDS[grid])
    check_occupancy(f"{foot} {grid}", got, rows, [217, 130], f, GRIDS[grid])


@pytest.mark.parametrize("grid", list(GRIDS))
def test_route_that_leaves_the_field(torch_mod, grid):
    rows = east_rows(300, x0=-3.0, step=0.043)[None]                                   # ends at x = 9.9, 3.9 ft past the box
    got = device_occ(rows, [300], oc.SQUARE, GRIDS[grid])
    ref = check_occupancy("leaving " + grid, got, rows, [300], oc.SQUARE, GRIDS[grid])
    assert ref["blocked"].any() and not ref["blocked"][:, -1].all() and (ref["last"] != oc.INT_MAX).all()   # it parks outside


# ---------------------------------------------------------------- determinism and composition

def test_two_calls_composition_shift_and_culling(torch_mod):
    routes = [oc.crossing_rows(), east_rows(150), oc.make_rows(np.full(90, 3.017), np.full(90, -2.011), 0.035 * np.arange(90))]
    rows, counts, field = padded(routes, 217), [217, 150, 90], GRIDS["ragged"]
    kw = dict(hold_first=True)
    all_k = KEYS + ("min_clearance", "blocked")
    a = device_occ(rows, counts, oc.SQUARE, field, **kw)
    b = device_occ(rows, counts, oc.SQUARE, field, **kw)
    off = device_occ(rows, counts, oc.SQUARE, field, cull=False, **kw)
    for k in all_k:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        assert np.array_equal(a[k].view(np.uint8), off[k].view(np.uint8)), ("cull", k)
    check_occupancy("composition", a, rows, counts, oc.SQUARE, field, **kw)
    single = [device_occ(r[None], [len(r)], oc.SQUARE, field, **kw) for r in routes]
    assert np.array_equal(a["first"], np.minimum.reduce([s["first"] for s in single]))
    assert np.array_equal(a["last"], np.maximum.reduce([s["last"] for s in single]))
    assert np.array_equal(a["count"], sum(s["count"] for s in single))
    assert np.array_equal(bits(a["min_clearance"]), bits(np.minimum.reduce([s["min_clearance"] for s in single])))
    for sh in (5, -5):
        s = device_occ(rows, counts, oc.SQUARE, field, shift_rows=sh, **kw)
        for k in ("first", "last"):
            fixed = (a[k] == oc.INT_MIN) | (a[k] == oc.INT_MAX)
            assert np.array_equal(s[k][fixed], a[k][fixed]) and np.array_equal(s[k][~fixed], a[k][~fixed] + sh), (sh, k)
        assert (a["first"] == oc.INT_MIN).any() and (a["last"] == oc.INT_MAX).any()
        assert np.array_equal(s["count"], a["count"]) and np.array_equal(bits(s["min_clearance"]), bits(a["min_clearance"]))
    # nothing to rasterise: the never-covered values
    for e in (device_occ(np.zeros((0, 8, 8)), np.zeros((0, 1), dtype=np.int32), oc.SQUARE, field),
              device_occ(rows, [0, 0, 0], oc.SQUARE, field), device_occ(np.zeros((2, 0, 8)), [0, 0], oc.SQUARE, field)):
        assert (e["first"] == oc.INT_MAX).all() and (e["last"] == oc.INT_MIN).all() and (e["count"] == 0).all()
        assert np.isposinf(e["min_clearance"]).all() and not e["blocked"].any()


def test_parked_partner_equals_a_scene_polygon(torch_mod):
    from vexautonomousplanner_amd import footprint as fp
    for x, y, h in ((0.013, -1.007, -(np.pi / 2 + 0.03)), (3.1, 2.2, 0.4), (-5.6, 5.5, 2.0)):
        rows = oc.make_rows([x], [y], [h])
        assert oc.occupancy([rows], None, oc.SQUARE, S["field"], S["cell"], S["radius"], S["margin"])["gap"] >= 1e-9
        occ = P().occupancy(rows, None, oc.SQUARE, field_scene(S["field"]), S["cell"], S["radius"], margin=S["margin"])
        square = oc.pose(rows, oc.SQUARE)[0]
        c = pr.clearance_grid(S["field"], S["cell"], polygons=[square], radius=S["radius"])
        assert np.abs(c - S["margin"]).min() >= 1e-9
        with_poly = P().clearance_grid(fp.Scene(field=S["field"], polygons=[square]), S["cell"], S["radius"], S["margin"])
        without = P().clearance_grid(field_scene(S["field"]), S["cell"], S["radius"], S["margin"])
        blocked = host(occ["blocked"])
        assert blocked.any() and np.array_equal(host(with_poly["free"]), host(without["free"]) & ~blocked)
        assert (host(occ["last"])[blocked] == oc.INT_MAX).all() and (host(occ["first"])[blocked] == 0).all()


# ---------------------------------------------------------------- windowed seeds

def occupied_seeds(sc, starts, goals, W, occupancy, windows, **over):
    s = dict(sc, **over)
    out = P().seeds(np.atleast_2d(starts), np.atleast_2d(goals), scene_of(s), W, s["radius"], cell=s["cell"], margin=s["margin"],
                    vertices=True, distance=True, occupancy=occupancy, windows=windows)
    return {k: host(v) for k, v in out.items()}


WINDOWS = [(oc.INT_MIN, oc.INT_MAX), (0, 60), (0, 120), (150, 217), (120, 120), (0, 300)]
GOAL_IN_LANE = (0.05, 2.95)      # free in scene C, inside the partner's last pose plus disc: blocked by the held last row


def test_windowed_seeds_match_reference(torch_mod):
    torch = torch_mod
    sc, W = pr.SCENE_C, 9
    _, _, free = tgp.reference_grid(sc)
    rows = oc.crossing_rows()
    ref_occ = oc.occupancy([rows], None, oc.SQUARE, sc["field"], sc["cell"], sc["radius"], sc["margin"])
    assert ref_occ["gap"] >= 1e-9
    occ = P().occupancy(rows, None, oc.SQUARE, scene_of(sc), sc["cell"], sc["radius"], margin=sc["margin"])
    assert np.array_equal(host(occ["first"]), ref_occ["first"]) and np.array_equal(host(occ["last"]), ref_occ["last"])
    starts = np.repeat(np.array([sc["start"]]), 6, axis=0)
    goals = np.repeat(np.array([sc["goal"]]), 6, axis=0)
    goals[5] = GOAL_IN_LANE
    ref, masks = oc.seeds(starts, goals, WINDOWS, sc["field"], sc["cell"], free, ref_occ["first"], ref_occ["last"], W=W)
    static, _ = pr.seeds([sc["start"]], [sc["goal"]], margin=sc["margin"], W=W, **pr.scene_args(sc))
    lengths = [r["length"] for r in ref]
    print("windowed seeds: flags", [r["flags"] for r in ref], "vertices", [r["n_vertices"] for r in ref], "lengths", lengths)
    # what the reference says about the problems: the partner ends parked beside the wall's top, so the whole horizon and
    # the late window climb higher than the wall alone asks for (18.64 ft against 17.54 ft); while it is still south
    # (rows 0 .. 59) and in the empty window the static route stands; rows 0 .. 119 lie between; the goal in the lane is snapped
    assert all(r["flags"] == 0 for r in ref[:5]) and ref[5]["flags"] == pr.SNAPPED_GOAL
    assert lengths[0] == lengths[3] > lengths[2] > lengths[1] + 0.5 and lengths[0] > static[0]["length"] + 1.0
    assert lengths[1] == static[0]["length"] == lengths[4] and np.array_equal(masks[4], free)
    assert free[pr.cell_of(GOAL_IN_LANE, sc["field"], sc["cell"])[::-1]] and not masks[5][pr.cell_of(GOAL_IN_LANE, sc["field"], sc["cell"])[::-1]]
    out = occupied_seeds(sc, starts, goals, W, occ, np.array(WINDOWS))
    for r in range(6):
        tgp.check_problem(f"window {WINDOWS[r]}", out, r, ref[r], starts[r], goals[r], W)
    # six single calls, bit for bit; windows=None is the whole horizon
    for r in range(6):
        one = occupied_seeds(sc, starts[r], goals[r], W, occ, np.array(WINDOWS[r]))
        for k in out:
            assert np.array_equal(one[k][0:1].view(np.uint8), out[k][r:r + 1].view(np.uint8)), (r, k)
    whole = occupied_seeds(sc, starts[0], goals[0], W, (occ["first"], occ["last"]), None)
    for k in out:
        assert np.array_equal(whole[k][0:1].view(np.uint8), out[k][0:1].view(np.uint8)), k
    # without an occupancy, and with one that covers nothing, the call is plan.seeds bit for bit
    plain = tgp.device_seeds(sc, starts, goals, W)
    none = occupied_seeds(sc, starts, goals, W, None, None)
    never = (torch.full((48, 48), oc.INT_MAX, dtype=torch.int32, device="cuda"), torch.full((48, 48), oc.INT_MIN, dtype=torch.int32, device="cuda"))
    empty = occupied_seeds(sc, starts, goals, W, never, np.array(WINDOWS))
    for k in plain:
        assert np.array_equal(plain[k].view(np.uint8), none[k].view(np.uint8)), k
        assert np.array_equal(plain[k].view(np.uint8), empty[k].view(np.uint8)), k
    tgp.check_problem("static", plain, 0, static[0], starts[0], goals[0], W)
    # a window that walls the start off: a column of cells occupied from instant 0 on
    first, last = never[0].clone(), never[1].clone()
    first[:, 10] = 0
    last[:, 10] = oc.INT_MAX
    ref_wall, _ = oc.seeds(starts[:2], goals[:2], [(0, 50), (-9, 0)], sc["field"], sc["cell"], free, host(first), host(last), W=W)
    wall = occupied_seeds(sc, starts[:2], goals[:2], W, (first, last), np.array([(0, 50), (-9, 0)]))
    assert ref_wall[0]["flags"] == pr.UNREACHABLE and ref_wall[1]["flags"] == 0
    for r in range(2):
        tgp.check_problem(f"walled {r}", wall, r, ref_wall[r], starts[r], goals[r], W)
    with pytest.raises(ValueError):
        P().seeds(starts, goals, scene_of(sc), W, sc["radius"], windows=np.array(WINDOWS))
    with pytest.raises(ValueError):
        P().seeds(starts, goals, scene_of(sc), W, sc["radius"], cell=0.5, occupancy=occ)


def test_the_lds_limit_with_two_windows(torch_mod):
    """128 x 128 cells: the 128 KB field, both bitsets and the move bytes, 148 KB of LDS."""
    sc = dict(pr.SCENE_C, cell=12.0 / 128)
    _, _, free = tgp.reference_grid(sc)
    rows = oc.crossing_rows()
    ref_occ = oc.occupancy([rows], None, oc.SQUARE, sc["field"], sc["cell"], sc["radius"], sc["margin"])
    assert ref_occ["gap"] >= 1e-9 and free.shape == (128, 128)
    occ = P().occupancy(rows, None, oc.SQUARE, scene_of(sc), sc["cell"], sc["radius"], margin=sc["margin"])
    for k in ("first", "last"):
        assert np.array_equal(host(occ[k]), ref_occ[k]), k
    starts, goals, windows = np.array([sc["start"]] * 2), np.array([sc["goal"]] * 2), [(0, 60), (oc.INT_MIN, oc.INT_MAX)]
    for W in (5, 9):
        ref, _ = oc.seeds(starts, goals, windows, sc["field"], sc["cell"], free, ref_occ["first"], ref_occ["last"], W=W)
        assert ref[0]["flags"] == 0 and ref[1]["flags"] == 0 and ref[1]["length"] > ref[0]["length"] + 0.1
        out = occupied_seeds(sc, starts, goals, W, occ, np.array(windows))
        for r in range(2):
            tgp.check_problem(f"128x128 window {windows[r]}", out, r, ref[r], starts[r], goals[r], W)


# ---------------------------------------------------------------- end to end

PARTNER = (0.143, 1.324)


def test_occupancy_planned_seed_makes_the_search_feasible(torch_mod):
    """Scene B with the partner parked on the static seed (module docstring): its one row goes to plan_occupancy and to
    refine(others=...) alike.  The static seed's own cost is infeasible on the conflict term; from the occupancy-planned
    seed the reference loop is feasible from the first iteration, so the device run must end feasible, with a
    non-increasing history, and its best route must clear the partner by the conflict margin on its own rows."""
    torch = torch_mod
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import search
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    sc, W = pr.SCENE_B, 9
    gen = BatchedTrajectoryGenerator(0, "f32")
    foot = fp.rectangle(18, 18)
    prow = oc.make_rows([PARTNER[0]], [PARTNER[1]], [0.0])
    others = {"rows": torch.tensor(prow[None], device=gen.device), "counts": torch.tensor([[1, 0]], dtype=torch.int32, device=gen.device)}
    assert oc.occupancy([prow], None, oc.SQUARE, sc["field"], sc["cell"], sc["radius"], sc["margin"])["gap"] >= 1e-9
    occ = gen.plan_occupancy(others, foot, scene_of(sc), sc["cell"], sc["radius"], margin=sc["margin"])
    kw = dict(cell=sc["cell"], margin=sc["margin"], vertices=True)
    static = gen.plan_seeds(np.array([sc["start"]]), np.array([sc["goal"]]), scene_of(sc), W, sc["radius"], **kw)
    planned = gen.plan_seeds(np.array([sc["start"]]), np.array([sc["goal"]]), scene_of(sc), W, sc["radius"], occupancy=occ, **kw)
    assert bool(static["feasible"][0]) and bool(planned["feasible"][0])
    assert float(static["vertices"][0, 1, 1]) > 1.0 and float(planned["vertices"][0, 1, 1]) < -1.0          # north; south
    w = search.Weights(clearance_margin=0.1, conflict_margin=0.05)

    def cost_of(routes):
        wp = torch.as_tensor(host(routes), dtype=gen.tdtype, device=gen.device)
        res = gen.profile(wp, dd=0.005, capacity=8192)
        tp = gen.time_profile(res, dt=0.01, capacity_rows=2048)
        clr = gen.footprint_clearance(tp, foot, scene_of(sc), margin=w.clearance_margin)
        conf = gen.footprint_conflicts(tp, foot, others, margin=w.conflict_margin)
        rk = search.rank(wp, 1, weights=w, counts=tp["counts"], time_step=0.01, meta=res["meta"], flags=res["flags"],
                         clearance=clr["min_clearance"], conflict_clearance=conf["min_clearance"])
        return float(rk["cost"][0]), float(rk["violation"][0]), float(conf["min_clearance"][0]), tp
    c_static, v_static, conf_static, _ = cost_of(static["waypoints"])
    print(f"static seed: cost {c_static:.1f}, violation {v_static:.4f} ft, conflict clearance {conf_static:.4f} ft")
    assert c_static > 1e6 and v_static > 0 and conf_static < w.conflict_margin                               # through the partner
    cfg = search.SearchConfig(candidates=64, elites=8, iterations=12, alpha=0.7, weights=w)
    out = gen.refine(planned["waypoints"], 0.5, foot, scene_of(sc), dd=0.005, dt=0.01, capacity=8192, capacity_rows=2048,
                     others=others, config=cfg)
    torch.cuda.synchronize()
    h = host(out["history"])[0]
    print(f"planned seed: best {float(out['best_cost'][0]):.4f} s, history {h.tolist()}, n_feasible {host(out['n_feasible'])[0].tolist()}")
    assert (np.diff(h) <= 0).all()
    assert bool(out["feasible"][0]) and np.isfinite(h[-1]) and h[-1] < 1e6
    # independently: the best route profiled alone, its own rows against the partner by the two references
    c_best, v_best, conf_best, tp = cost_of(out["best_waypoints"])
    n = int(tp["counts"][0, 0])
    rows = host(tp["rows"])[0, :n]
    ref_conf = cr.conflicts(rows[None], [n], foot, prow[None], [1], foot, w.conflict_margin, 0)["min_clearance"][0]
    import footprint_ref as fr
    square = foot + np.array(PARTNER)
    ref_gap = fr.row_clearance(rows, foot, None, [square], ())[0].min()
    print(f"best route alone: {n} rows, conflict clearance {conf_best:.4f} (conflict_ref {ref_conf:.4f}, footprint_ref {ref_gap:.4f}) ft")
    assert v_best == 0.0 and ref_conf >= w.conflict_margin and ref_gap >= w.conflict_margin - 1e-9
