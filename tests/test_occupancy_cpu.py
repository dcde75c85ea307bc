"""CPU: the product declares and exports vap_plan_occupancy and vap_plan_seeds_occupied and both refuse bad arguments
before a device is touched; the NumPy reference of the occupancy (tests/occupancy_ref.py) against the definitions of
include/vap.h and against tests/plan_ref.py; the crossing scenario through plan_ref.plan on the windowed mask.

The crossing scenario (occupancy_ref.CROSSING): a field of +-6 ft, cell 0.25 ft, an 18 x 18 in partner at x = 0.013,
y = -5 + 0.007 + 0.03 r for the 217 rows r = 0 .. 216 (10 ms rows, 3 ft/s north), heading -(pi/2 + 0.03); I am a disc of
0.75 ft wanting 0.1 ft, from (-4.5, -3) to (4.5, -3).  Smallest |clearance - margin| over all 499 968 (row, cell) pairs
1.16e-4; 457 cells covered; a cell's first covering row runs from 0 to 213."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import occupancy_ref as oc
import plan_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = oc.CROSSING


def grid_centres(field=S["field"], cell=S["cell"]):
    return np.meshgrid(*pr.centres(field, cell))


def occ(rows, counts=None, **kw):
    a = dict(footprint=oc.SQUARE, field=S["field"], cell=S["cell"], radius=S["radius"], margin=S["margin"])
    a.update(kw)
    return oc.occupancy(rows, counts, **a)


@pytest.fixture(scope="module")
def crossing():
    return occ([oc.crossing_rows()])


def test_header_declares_and_library_exports_both_calls():
    from vexautonomousplanner_amd import _lib, plan
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    text = open(os.path.join(ROOT, "include", "vap.h")).read()
    for name in ("vap_plan_occupancy", "vap_plan_seeds_occupied"):
        assert re.search(r"^int %s\(vap_ctx \*ctx," % name, text, re.M), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert "draw_rect" in text[text.index("routes rasterised onto the planner's grid"):]       # the reference function is cited
    assert callable(plan.occupancy) and callable(BatchedTrajectoryGenerator.plan_occupancy)
    assert np.array_equal(oc.SQUARE, __import__("vexautonomousplanner_amd.footprint", fromlist=["x"]).rectangle(18, 18))


def test_both_calls_check_their_arguments_before_the_device():
    """By value, with a NULL context and pointers that are never dereferenced."""
    from vexautonomousplanner_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)
    dbl = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_lib.dp)
    sq, field = oc.SQUARE, np.array(S["field"])

    def occupancy(B=1, cap=8, rows=one, counts=one, stride=1, foot=sq, fld=field, cell=0.25, radius=0.75, margin=0.1, shift=0,
                  out=one):
        return L.vap_plan_occupancy(None, B, cap, rows, counts, stride, len(foot), dbl(foot), dbl(fld) if fld is not None else None,
                                    cell, radius, margin, shift, 0, 1, out, out, out, out, None, None)
    INV, UNS = _lib.VAP_ERR_INVALID, _lib.VAP_ERR_UNSUPPORTED
    assert occupancy(B=-1) == INV and occupancy(cap=-1) == INV and occupancy(stride=0) == INV
    assert occupancy(rows=None) == INV and occupancy(counts=None) == INV
    assert occupancy(foot=sq[::-1]) == INV and occupancy(foot=sq[:2]) == INV          # clockwise; two vertices
    assert occupancy(fld=None) == INV and occupancy(fld=np.array([1.0, 0, 0, 1])) == INV
    assert occupancy(cell=0.0) == INV and occupancy(cell=np.nan) == INV and occupancy(radius=-0.1) == INV
    assert occupancy(margin=np.inf) == INV
    assert occupancy(cell=0.09) == UNS                                                  # 134 x 134 cells
    assert occupancy(cap=oc.INT_MAX) == UNS and occupancy(cap=8, shift=oc.INT_MAX - 8) == UNS and occupancy(shift=oc.INT_MIN) == UNS
    nx, ny = C.c_int(0), C.c_int(0)                                                    # the shape only: no context needed
    assert L.vap_plan_occupancy(None, 1, 8, one, one, 1, 4, dbl(sq), dbl(field), 0.25, 0.75, 0.1, 0, 0, 1, None, None, None, None,
                                C.byref(nx), C.byref(ny)) == _lib.VAP_OK and (nx.value, ny.value) == (48, 48)
    assert occupancy() == INV                                                           # valid arguments: stopped by the NULL context

    def seeds(R=1, W=5, first=one, last=one, cell=0.25, starts=one):
        return L.vap_plan_seeds_occupied(None, R, W, starts, one, dbl(field), 0, None, None, 0, None, cell, 0.75, 0.1, 64, first, last,
                                         None, one, None, None, None, None, None)
    assert seeds(first=None) == INV and seeds(last=None) == INV                         # exactly one of the two
    assert seeds(R=-1) == INV and seeds(W=1) == INV and seeds(W=2049) == UNS and seeds(starts=None) == INV
    assert seeds(cell=0.0) == INV and seeds(cell=0.09) == UNS


def test_one_held_row_blocks_what_the_posed_square_blocks_as_a_scene_polygon():
    for x, y, h in ((0.013, -1.007, -(np.pi / 2 + 0.03)), (3.1, 2.2, 0.4), (-5.6, 5.5, 2.0)):      # the last one overlaps the wall
        rows = oc.make_rows([x], [y], [h])
        o = occ([rows])
        assert o["gap"] > 1e-9
        square = oc.pose(rows, oc.SQUARE)[0]
        with_poly = pr.clearance_grid(S["field"], S["cell"], polygons=[square], radius=S["radius"]) >= S["margin"]
        without = pr.clearance_grid(S["field"], S["cell"], radius=S["radius"]) >= S["margin"]
        assert np.array_equal(with_poly, without & ~o["blocked"]) and o["blocked"].any()
        assert np.array_equal(oc.window_free(without, o["first"], o["last"]), with_poly)
        # one row: first = 0, last = held, count = 1 where blocked
        assert (o["first"][o["blocked"]] == 0).all() and (o["last"][o["blocked"]] == oc.INT_MAX).all()
        assert np.array_equal(o["count"], o["blocked"].astype(np.int64))
        # the clearance itself is plan_ref's polygon distance minus the radius, bit for bit
        px, py = grid_centres()
        assert np.array_equal(o["min_clearance"], pr.polygon_distance(px, py, square) - S["radius"])


def test_sentinels_shift_holds_empty_routes_and_clamped_counts(crossing):
    rows = oc.crossing_rows()
    o = crossing
    nb = ~o["blocked"]
    assert (o["first"][nb] == oc.INT_MAX).all() and (o["last"][nb] == oc.INT_MIN).all() and (o["count"][nb] == 0).all()
    assert o["blocked"].sum() == 457 and np.array_equal(o["blocked"], o["count"] > 0)
    assert abs(o["gap"] - 1.16e-4) < 1e-6 and o["pairs"] == 217 * 48 * 48
    assert o["first"][o["blocked"]].min() == 0 and o["first"][o["blocked"]].max() == 213
    held = o["last"] == oc.INT_MAX
    assert held.any() and np.array_equal(held, occ([rows[-1:]])["blocked"])             # exactly the last row's cells
    assert (o["last"][o["blocked"] & ~held] <= 216).all()
    # no holds: plain instants; hold_first: row 0's cells
    plain = occ([rows], hold_last=False)
    assert plain["last"].max() == 216 and np.array_equal(plain["first"], o["first"]) and np.array_equal(plain["count"], o["count"])
    assert np.array_equal(plain["last"][~held], o["last"][~held])
    hf = occ([rows], hold_first=True)
    row0 = occ([rows[:1]])["blocked"]
    assert np.array_equal(hf["first"] == oc.INT_MIN, row0) and np.array_equal(hf["first"][~row0], o["first"][~row0])
    assert np.array_equal(hf["count"], o["count"]) and np.array_equal(hf["last"], o["last"])
    # shift_rows moves every instant and leaves the holds and the never-covered values
    for sh in (5, -5):
        s = occ([rows], shift_rows=sh, hold_first=True)
        for key, ref in (("first", hf["first"]), ("last", hf["last"])):
            fixed = (ref == oc.INT_MIN) | (ref == oc.INT_MAX)
            assert np.array_equal(s[key][fixed], ref[fixed]) and np.array_equal(s[key][~fixed], ref[~fixed] + sh)
        assert np.array_equal(s["count"], o["count"])
    # an empty route, no route at all, and a count above the capacity (clamped) or below 0
    for e in (occ([rows], counts=[0]), occ([]), occ([rows], counts=[-3])):
        assert (e["first"] == oc.INT_MAX).all() and (e["last"] == oc.INT_MIN).all() and (e["count"] == 0).all()
        assert np.isposinf(e["min_clearance"]).all() and not e["blocked"].any() and e["gap"] == np.inf
    big = occ([rows], counts=[10 ** 6])
    for k in ("first", "last", "count", "min_clearance"):
        assert np.array_equal(big[k], o[k])
    part = occ([rows], counts=[100])
    assert np.array_equal(part["last"] == oc.INT_MAX, occ([rows[99:100]])["blocked"]) and part["count"].sum() < o["count"].sum()
    # a row with a non-finite pose covers nothing and is no part of the minimum
    bad = rows.copy()
    bad[50, 6] = np.nan
    bad[60, 4] = np.inf
    nf = occ([bad])
    assert np.isfinite(nf["min_clearance"]).all() and nf["pairs"] == 215 * 48 * 48 and nf["count"].sum() < o["count"].sum()


def test_union_of_three_routes_is_min_max_sum():
    rows = oc.crossing_rows()
    east = oc.make_rows(-4.0 + 0.031 * np.arange(150), np.full(150, 1.003), np.full(150, 0.02))
    turn = oc.make_rows(np.full(90, 3.017), np.full(90, -2.011), 0.035 * np.arange(90))    # an in-place turn
    routes = [rows, east, turn]
    alone = [occ([r], shift_rows=3, hold_first=True) for r in routes]
    both = occ(routes, shift_rows=3, hold_first=True)
    assert both["gap"] > 1e-9 and both["gap"] == min(a["gap"] for a in alone)
    assert np.array_equal(both["first"], np.minimum.reduce([a["first"] for a in alone]))
    assert np.array_equal(both["last"], np.maximum.reduce([a["last"] for a in alone]))
    assert np.array_equal(both["count"], sum(a["count"] for a in alone))
    assert np.array_equal(both["min_clearance"], np.minimum.reduce([a["min_clearance"] for a in alone]))
    assert np.array_equal(both["blocked"], alone[0]["blocked"] | alone[1]["blocked"] | alone[2]["blocked"])
    # as one padded array with counts: the same
    cap = 217
    padded = np.full((3, cap, 8), np.nan)
    for b, r in enumerate(routes):
        padded[b, :len(r)] = r
    again = occ(padded, counts=[217, 150, 90], shift_rows=3, hold_first=True)
    for k in ("first", "last", "count", "min_clearance"):
        assert np.array_equal(again[k], both[k])
    # the longdouble run decides every pair the same way
    ld = occ(routes, shift_rows=3, hold_first=True, ftype=np.longdouble)
    for k in ("first", "last", "count"):
        assert np.array_equal(ld[k], both[k])
    assert np.abs(ld["min_clearance"] - both["min_clearance"]).max() < 1e-14


def test_window_mask_definition():
    free = np.array([[True, True, True, False, True, True]])
    first = np.array([[oc.INT_MAX, 10, 10, 10, oc.INT_MIN, 30]])
    last = np.array([[oc.INT_MIN, 20, oc.INT_MAX, 20, 5, 30]])
    W = lambda w: oc.window_free(free, first, last, w)[0].tolist()
    assert W(None) == [True, False, False, False, False, False]
    assert W((0, 10)) == [True, True, True, False, False, True]            # t1 is exclusive: first < t1
    assert W((0, 11)) == [True, False, False, False, False, True]
    assert W((20, 30)) == [True, False, False, False, True, True]          # t0 is inclusive: last >= t0
    assert W((21, 30)) == [True, True, False, False, True, True]
    assert W((21, 31)) == [True, True, False, False, True, False]
    assert W((15, 15)) == W((16, 15)) == [True, True, True, False, True, True]   # an empty window blocks nothing
    assert W((oc.INT_MIN, oc.INT_MAX)) == W(None)


ROUTES = [("static", 2, 9.0, None), ((150, 217), 2, 9.0, None), (None, 4, 16.502272539475065, 3.125),
          ((0, 60), 4, 9.968444857779264, None), ((0, 120), 5, 11.876690717513696, None)]


@pytest.mark.parametrize("window,n_vertices,length,y_mid", ROUTES, ids=[str(r[0]) for r in ROUTES])
def test_crossing_scenario_routes(crossing, window, n_vertices, length, y_mid):
    free = pr.clearance_grid(S["field"], S["cell"], radius=S["radius"]) >= S["margin"]
    mask = free if window == "static" else oc.window_free(free, crossing["first"], crossing["last"], window)
    p = pr.plan(S["start"], S["goal"], S["field"], S["cell"], mask, 9)
    print(window, p["n_vertices"], repr(p["length"]), p["vertices"][:p["n_vertices"]].tolist())
    assert p["flags"] == 0 and p["n_vertices"] == n_vertices and p["length"] == length
    if y_mid is not None:
        assert (p["vertices"][1:3, 1] == y_mid).all()                       # over the top of the partner's whole lane
    if window == (0, 60):
        assert (p["vertices"][1:3, 1] < -1.0).all()                         # behind the partner, which has moved on north
    # the seeds reference with windows gives the same routes as the masks one by one
    out, _ = oc.seeds([S["start"]], [S["goal"]], None if window in ("static", None) else [window], S["field"], S["cell"], free,
                      *((crossing["first"], crossing["last"]) if window != "static" else (np.full(free.shape, oc.INT_MAX), np.full(free.shape, oc.INT_MIN))), W=9)
    assert out[0]["length"] == length and out[0]["n_vertices"] == n_vertices
