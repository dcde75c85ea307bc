"""GPU: every call family that reads a scene gets its own bytes when the calls share one context's scene block.

footprint.clearance, sensors.readings, plan.clearance_grid, plan.seeds and plan.travel all pack their scene through
scene_block (vap_footprint.h) into the context's one pinned host block and one device block, each with its own prefix (a
footprint, a partner's footprint, none) and its own reader.  Each (call, scene) pair runs once alone on a fresh context;
then all of them run on a single context, neighbours in the sequence differing in family and in scene, the scenes in the
order S1, S2, S0, S2, S1 so that the host block grows, is reused while smaller and is reused at full size.  Every output
byte of the shared run is the solo run's, NaN payloads included: there are no tolerances.

The planner's mask is clearance >= margin, so as in test_gpu_plan.py the reference first shows that no cell centre of a scene
lies within 1e-9 of the margin."""
import numpy as np
import pytest

import plan_ref as pr
import scene_cases as sc

FIELD = (-6.0, -6.0, 6.0, 6.0)                      # 12 ft
CELL, RADIUS, MARGIN = 1.0, 0.3, 0.05               # a 12 x 12 grid
ORDER = ("S1", "S2", "S0", "S2", "S1")
FAMILIES = ("clearance", "readings", "grid", "seeds", "travel")
SPOTS = [(-4.25 + 1.7 * i, -4.25 + 1.7 * j) for j in range(6) for i in range(6)]


def scene_parts(name):
    """(polygons, circles) of S0 (empty), S1 (one circle) and S2: 33 small convex polygons, more than one 32-polygon chunk
    of k_plan_clearance, one of them with 16 vertices, and two circles."""
    if name == "S0":
        return [], []
    if name == "S1":
        return [], [(0.4, -0.3, 0.5)]
    polys = [sc.ngon(3 + k % 6, 0.22 + 0.01 * (k % 7), x, y, phase=0.37 * k) for k, (x, y) in enumerate(SPOTS[:32])]
    polys.append(sc.oval16(0.4, 0.25) + np.array(SPOTS[32]))
    return polys, [(*SPOTS[33], 0.3), (*SPOTS[34], 0.2)]


def reference_gap(name):
    """The smallest |clearance - margin| over the cell centres, on the reference."""
    polys, circles = scene_parts(name)
    c = pr.clearance_grid(FIELD, CELL, polys, circles, RADIUS)
    assert c.shape == (12, 12)
    return float(np.abs(c - MARGIN).min())


def test_no_cell_within_1e9_of_the_margin():
    """On the reference alone: an ulp of the clearance cannot flip a cell of any scene, and S2 is what it is there for."""
    polys, circles = scene_parts("S2")
    assert len(polys) == 33 and max(len(p) for p in polys) == 16 and len(circles) == 2
    for name in ("S0", "S1", "S2"):
        gap = reference_gap(name)
        print("SCENE_BLOCK", name, "smallest |clearance - margin|", gap)
        assert gap >= 1e-9
    free = [pr.clearance_grid(FIELD, CELL, *scene_parts(n), RADIUS) >= MARGIN for n in ("S0", "S1", "S2")]
    assert (free[0] != free[1]).any() and (free[1] != free[2]).any() and free[2].any()


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(33)
    rows = sc.walks(rng, 2, 48, (0.0, 0.0), 3.0)
    partner = sc.walks(rng, 1, 48, (1.0, 1.0), 1.0)
    return dict(rows=rows, counts=np.array([48, 40], dtype=np.int32), partner=partner, partner_counts=np.array([48], dtype=np.int32),
                starts=np.array([[-5.5, -5.5], [5.2, -4.8], [0.4, -0.3]]), goals=np.array([[5.5, 5.5], [-5.1, 4.9], [-4.6, 0.2]]),
                points=np.array([[[-5.5, -5.5], [5.5, 5.5], [0.4, -0.3]], [[5.2, -4.8], [-5.1, 4.9], [2.2, 2.4]]]))


def run(family, scene, inp, ctx):
    """One call of `family` on `ctx`; its output tensors by name, not synchronised."""
    from vexautonomousplanner_amd import footprint, plan, sensors
    if family == "clearance":
        return footprint.clearance(inp["rows"], inp["counts"], sc.SQUARE, scene, margin=0.1, per_row=True, ctx=ctx)
    if family == "readings":
        two = [sensors.Sensor(6.0, 0.0, 0.0), sensors.Sensor(0.0, 6.0, 90.0, max_incidence_deg=60.0)]
        return sensors.readings(inp["rows"], inp["counts"], two, scene, others=inp["partner"], others_counts=inp["partner_counts"],
                                others_footprint=sc.UNIT, per_row=True, ctx=ctx)
    if family == "grid":
        return plan.clearance_grid(scene, CELL, RADIUS, MARGIN, ctx=ctx)
    if family == "seeds":
        return plan.seeds(inp["starts"], inp["goals"], scene, 5, RADIUS, cell=CELL, margin=MARGIN, vertices=True, distance=True, ctx=ctx)
    return plan.travel(inp["points"], scene, RADIUS, cell=CELL, margin=MARGIN, waypoints=5, ctx=ctx)


def as_bytes(res):
    return {k: res[k].cpu().numpy().tobytes() for k in sorted(res)}


@pytest.mark.gpu
def test_shared_scene_block_gives_every_family_its_own_bytes(inputs):
    import torch

    from vexautonomousplanner_amd import _lib, footprint
    assert torch.cuda.is_available()
    scenes = {}
    for name in ("S0", "S1", "S2"):
        assert reference_gap(name) >= 1e-9
        polys, circles = scene_parts(name)
        scenes[name] = footprint.Scene(field=FIELD, polygons=polys, circles=circles)
    solo = {}
    for family in FAMILIES:
        for name in scenes:
            ctx = _lib.Context(0)
            res = run(family, scenes[name], inputs, ctx)
            ctx.synchronize()
            solo[family, name] = as_bytes(res)
            ctx.close()
    torch.cuda.synchronize()
    for family in FAMILIES:                                            # the scenes are told apart by every family
        assert solo[family, "S0"] != solo[family, "S1"] and solo[family, "S1"] != solo[family, "S2"], family

    ctx = _lib.Context(0)
    shared = []
    for n in range(len(FAMILIES) * len(ORDER)):                        # neighbours differ in family and in scene
        family, name = FAMILIES[n % 5], ORDER[(n // 5 + n % 5) % 5]
        shared.append((family, name, run(family, scenes[name], inputs, ctx)))
    ctx.synchronize()
    assert [name for family, name, _ in shared if family == FAMILIES[0]] == list(ORDER)
    total = 0
    for n, (family, name, res) in enumerate(shared):
        got, want = as_bytes(res), solo[family, name]
        assert got.keys() == want.keys()
        for k in want:
            assert got[k] == want[k], (n, family, name, k)
            total += len(want[k])
    print("SCENE_BLOCK", len(shared), "calls on one context,", total, "bytes equal to the solo runs")
    ctx.close()
    torch.cuda.synchronize()
