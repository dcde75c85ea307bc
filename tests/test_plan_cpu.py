"""CPU: the NumPy reference of the grid planner (tests/plan_ref.py) against known answers and the definitions of
include/vap.h; that the product exposes vap_plan_grid / vap_plan_seeds and refuses bad arguments by value, without a
device; and the Python surface's argument errors.

Scenes B and C (plan_ref.SCENE_B / SCENE_C) are the ones the device tests use: a field of +-6 ft, rho = 0.75 ft, margin
0.1 ft, cell 0.25 ft (48 x 48).  B: one post at the origin, start (-4, 0), goal (4, 0).  C: a wall from the bottom edge up to
y = 2, a triangle and a post; start (-4.5, -3), goal (4.5, -3); the only way is over the wall's top."""
import ctypes as C

import numpy as np
import pytest

import plan_ref as pr

H = 0.25


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def octile(n_diag, n_axis, h, memo={}):
    """The octile closed form by the relaxation's own additions: n_diag diagonal and n_axis axis costs added from 0, the
    smallest sum over the orders they can come in."""
    if (n_diag, n_axis) == (0, 0):
        return 0.0
    key = (n_diag, n_axis, h)
    if key not in memo:
        memo[key] = min(octile(n_diag - 1, n_axis, h) + h * pr.SQRT2 if n_diag else np.inf,
                        octile(n_diag, n_axis - 1, h) + h if n_axis else np.inf)
    return memo[key]


@pytest.mark.parametrize("h", [0.25, 12.0 / 128, 0.1])
def test_empty_field_is_the_octile_closed_form(h):
    """Without obstacles d is min(|di|, |dj|) diagonal and ||di| - |dj|| axis costs: the same bits from the heap, from
    Jacobi sweeps and from the closed form."""
    free = np.ones((9, 11), dtype=bool)
    g = (4, 3)
    d = pr.dijkstra(free, h, g)
    dj, _ = pr.jacobi(free, h, g)
    assert np.array_equal(bits(d), bits(dj))
    want = np.array([[octile(min(abs(i - g[0]), abs(j - g[1])), abs(abs(i - g[0]) - abs(j - g[1])), h) for i in range(11)]
                     for j in range(9)])
    assert np.array_equal(bits(d), bits(want))
    assert d[3, 4] == 0.0 and d[3, 5] == h and d[4, 5] == h * pr.SQRT2 and d[3, 6] == h + h


def test_no_corner_is_cut():
    """Two free cells that touch only at a corner, with both axis cells blocked, do not reach each other."""
    free = np.array([[1, 0], [0, 1]], dtype=bool)
    d = pr.dijkstra(free, H, (0, 0))
    assert d[0, 0] == 0.0 and np.isinf(d[1, 1])
    assert not pr.allowed(free, 0, 0, 4)
    # one blocked axis cell is enough
    free = np.array([[1, 1], [0, 1]], dtype=bool)
    assert not pr.allowed(free, 0, 0, 4)
    d = pr.dijkstra(free, H, (0, 0))
    assert d[1, 1] == H + H
    assert pr.allowed(np.ones((2, 2), dtype=bool), 0, 0, 4)
    res = pr.plan((0.1, 0.1), (0.4, 0.4), (0.0, 0.0, 0.5, 0.5), H, np.array([[1, 0], [0, 1]], dtype=bool), 3)
    assert res["flags"] == pr.UNREACHABLE and res["n_vertices"] == 0 and np.isnan(res["waypoints"]).all() and np.isinf(res["length"])


def test_supercover_visibility():
    free = np.ones((6, 8), dtype=bool)
    assert pr.visible(free, (0, 0), (7, 5)) and pr.visible(free, (7, 5), (0, 0))
    # axis: only the cells of the row or column count
    row = free.copy()
    row[2, 3] = False
    assert not pr.visible(row, (0, 2), (7, 2)) and not pr.visible(row, (7, 2), (0, 2))
    assert pr.visible(row, (0, 1), (7, 1)) and pr.visible(row, (3, 0), (3, 1)) and not pr.visible(row, (3, 0), (3, 5))
    # an exact diagonal also takes the two cells beside each corner it passes (<=, the supercover)
    for blocked in ((1, 0), (0, 1), (2, 1), (1, 2)):
        m = free.copy()
        m[blocked[1], blocked[0]] = False
        assert not pr.visible(m, (0, 0), (2, 2)) and not pr.visible(m, (2, 2), (0, 0))
    m = free.copy()
    m[0, 2] = m[2, 0] = False
    assert pr.visible(m, (0, 0), (2, 2))
    # a knight's move (2, 1): the segment passes through (1, 0) and (1, 1), and touches nothing else
    for blocked, vis in (((1, 0), False), ((1, 1), False), ((0, 1), True), ((2, 0), True)):
        m = free.copy()
        m[blocked[1], blocked[0]] = False
        assert pr.visible(m, (0, 0), (2, 1)) == vis and pr.visible(m, (2, 1), (0, 0)) == vis
    # the other diagonal direction
    m = free.copy()
    m[1, 4] = False
    assert not pr.visible(m, (5, 0), (3, 2)) and not pr.visible(m, (3, 2), (5, 0)) and pr.visible(m, (7, 0), (5, 2))


def test_trace_takes_the_first_move_on_a_tie():
    free = np.ones((5, 5), dtype=bool)
    # start two columns right of the goal, one row up... a knight's offset has two paths of equal cost:
    # (-1, 0) then (-1, -1), or (-1, -1) then (-1, 0); move 2 = (-1, 0) comes before move 6 = (-1, -1)
    g, s = (1, 1), (3, 2)
    d = pr.dijkstra(free, H, g)
    assert d[2, 2] + H == d[1, 2] + H * pr.SQRT2                   # the tie is exact
    assert pr.trace(free, d, H, s) == [(3, 2), (2, 2), (1, 1)]
    # mirrored: (1, 0) [move 0] before (1, 1) [move 4]
    d = pr.dijkstra(free, H, (3, 3))
    assert pr.trace(free, d, H, (1, 2)) == [(1, 2), (2, 2), (3, 3)]
    # straight down: move 3 only
    assert pr.trace(free, d, H, (3, 4)) == [(3, 4), (3, 3)]
    assert pr.trace(free, d, H, (3, 3)) == [(3, 3)]


def test_snapping_ties_go_to_the_lowest_index():
    field = (0.0, 0.0, 1.0, 1.0)
    free = np.ones((4, 4), dtype=bool)
    free[1, 1] = False
    # the centre of the blocked cell (0.375, 0.375): four axis neighbours tie exactly; index j * nx + i lowest = (1, 0)
    assert pr.nearest_free(free, (0.375, 0.375), field, H) == (1, 0)
    free[0, 1] = False
    assert pr.nearest_free(free, (0.375, 0.375), field, H) == (0, 1)
    assert pr.nearest_free(free, (0.40, 0.375), field, H) == (2, 1)
    res = pr.plan((0.375, 0.375), (0.9, 0.9), field, H, free, 4)
    assert res["flags"] == pr.SNAPPED_START and res["cells"][0] == (0, 1)
    assert np.array_equal(res["vertices"][0], [0.375, 0.375]) and np.array_equal(res["waypoints"][0], [0.375, 0.375])
    res = pr.plan((0.9, 0.9), (0.375, 0.375), field, H, free, 4)
    assert res["flags"] == pr.SNAPPED_GOAL and res["cells"][-1] == (0, 1) and np.array_equal(res["waypoints"][-1], [0.375, 0.375])
    assert pr.plan((0.1, 0.1), (0.9, 0.9), field, H, np.zeros((4, 4), dtype=bool), 4)["flags"] == pr.NO_FREE
    assert pr.plan((np.nan, 0.1), (0.9, 0.9), field, H, free, 4)["flags"] == pr.FLAG_DEGENERATE
    # a point outside the box is clamped to the border cell
    assert pr.cell_of((-3.0, 9.0), field, H) == (0, 3)


def test_resample_ends_arcs_and_w2():
    v = np.array([[0.1, 0.2], [3.1, 4.2], [3.1, 4.2], [3.1, 10.2]])       # a zero-length segment in the middle
    for W in (2, 3, 7, 12):
        wp, L = pr.resample(v, W)
        assert L == 5.0 + 0.0 + 6.0 and wp.shape == (W, 2)
        assert np.array_equal(bits(wp[0]), bits(v[0])) and np.array_equal(bits(wp[-1]), bits(v[-1]))
        step = np.hypot(*np.diff(wp, axis=0).T)
        if W == 12:                                                       # 1 ft apart: the corner is hit exactly
            assert np.allclose(step, 1.0, rtol=0, atol=1e-14)
        # equal arcs ALONG the polyline
        arc = [0.0]
        for p in wp[1:]:
            arc.append(np.hypot(*(p - v[0])) if p[1] <= 4.2 and p[0] < 3.1 else 5.0 + (p[1] - 4.2))
        assert np.allclose(np.diff(arc), L / (W - 1), rtol=0, atol=1e-13)
        ld, Lld = pr.resample(v, W, np.longdouble)
        assert np.abs(ld - wp).max() < 1e-14 and abs(Lld - L) < 1e-14
    same = np.array([[1.0, 2.0], [1.0, 2.0]])
    wp, L = pr.resample(same, 4)
    assert L == 0.0 and (wp == same[0]).all()


@pytest.mark.parametrize("sc,sweeps,d_start,n_cells,n_vertices",
                         [(pr.SCENE_B, 38, 9.035533905932736, 33, 4), (pr.SCENE_C, 69, 17.63172798364529, 62, 8)], ids=["B", "C"])
def test_scene_fields_jacobi_equals_dijkstra(sc, sweeps, d_start, n_cells, n_vertices):
    c = pr.clearance_grid(**pr.scene_args(sc))
    ld = pr.clearance_grid(ftype=np.longdouble, **pr.scene_args(sc))
    assert c.shape == (48, 48) and np.abs(c - sc["margin"]).min() > 0.02 and float(np.abs(ld - c).max()) < 1e-14
    free = c >= sc["margin"]
    s, g = pr.cell_of(sc["start"], sc["field"], sc["cell"]), pr.cell_of(sc["goal"], sc["field"], sc["cell"])
    assert free[s[1], s[0]] and free[g[1], g[0]]
    d = pr.dijkstra(free, sc["cell"], g)
    dj, n = pr.jacobi(free, sc["cell"], g)
    assert n == sweeps and np.array_equal(bits(d), bits(dj))
    assert d[s[1], s[0]] == d_start and np.isinf(d[~free]).all()
    res, fr = pr.seeds([sc["start"]], [sc["goal"]], margin=sc["margin"], W=9, **pr.scene_args(sc))
    r = res[0]
    assert np.array_equal(fr, free) and r["flags"] == 0 and len(r["cells"]) == n_cells and r["n_vertices"] == n_vertices
    # the pulled route's own segments clear everything between cell centres
    for a, b in zip(r["pulled"][:-1], r["pulled"][1:]):
        assert pr.visible(free, a, b)
    assert r["length"] < d_start and np.array_equal(r["waypoints"][[0, -1]], np.array([sc["start"], sc["goal"]]))
    if sc is pr.SCENE_C:                                                  # over the wall's top
        assert r["vertices"][:n_vertices, 1].max() > 2.5 and (np.abs(r["vertices"][:n_vertices, 0]) < 1.0).any()


def test_vertices_truncated_flag_and_shared_cell():
    sc = pr.SCENE_C
    res, _ = pr.seeds([sc["start"], (3.05, 3.05)], [sc["goal"], (3.2, 3.2)], margin=sc["margin"], W=5, max_vertices=4, **pr.scene_args(sc))
    assert res[0]["flags"] == pr.VERTICES_TRUNCATED and res[0]["n_vertices"] == 8 and np.isfinite(res[0]["vertices"]).all()
    full, _ = pr.seeds([sc["start"]], [sc["goal"]], margin=sc["margin"], W=5, **pr.scene_args(sc))
    assert np.array_equal(res[0]["waypoints"], full[0]["waypoints"]) and np.array_equal(res[0]["vertices"], full[0]["vertices"][:4])
    assert res[1]["flags"] == 0 and res[1]["n_vertices"] == 2 and len(res[1]["cells"]) == 1
    assert np.array_equal(res[1]["vertices"][:2], [[3.05, 3.05], [3.2, 3.2]])


def test_product_declares_the_plan_calls():
    from vexautonomousplanner_amd import _lib, plan
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    L = _lib.lib()
    assert "vap_plan_grid" in _lib.EXPORTS and "vap_plan_seeds" in _lib.EXPORTS
    assert hasattr(L, "vap_plan_grid") and hasattr(L, "vap_plan_seeds")
    assert callable(plan.seeds) and callable(plan.clearance_grid) and callable(BatchedTrajectoryGenerator.plan_seeds)
    assert (_lib.PLAN_SNAPPED_START, _lib.PLAN_SNAPPED_GOAL, _lib.PLAN_NO_FREE, _lib.PLAN_UNREACHABLE,
            _lib.PLAN_VERTICES_TRUNCATED) == (pr.SNAPPED_START, pr.SNAPPED_GOAL, pr.NO_FREE, pr.UNREACHABLE, pr.VERTICES_TRUNCATED)
    header = open(_lib.HERE + "/../include/vap.h").read()
    for name, v in (("SNAPPED_START", 16), ("SNAPPED_GOAL", 32), ("NO_FREE", 64), ("UNREACHABLE", 128), ("VERTICES_TRUNCATED", 256)):
        assert f"#define VAP_PLAN_{name} {v}u" in header


def _abi():
    from vexautonomousplanner_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)
    dbl = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    keep = []

    def scene(field=pr.FIELD, polygons=(), circles=(), cell=0.25, radius=0.75, margin=0.1):
        f = None if field is None else dbl(field)
        start = np.cumsum([0] + [len(p) for p in polygons]).astype(np.int32)
        xy = dbl(np.concatenate(polygons)) if len(polygons) else dbl(np.zeros((0, 2)))
        cc = dbl(circles).reshape(-1, 3) if len(circles) else dbl(np.zeros((0, 3)))
        keep.extend([f, start, xy, cc])
        p = lambda a: a.ctypes.data_as(_lib.dp) if a is not None and a.size else None
        return [p(f), len(polygons), start.ctypes.data_as(_lib.ip), p(xy), len(cc), p(cc), cell, radius, margin]

    def seeds(R=1, W=5, max_vertices=8, vertices=None, starts=one, goals=one, wp=one, **kw):
        st = L.vap_plan_seeds(None, R, W, starts, goals, *scene(**kw), max_vertices, wp, None, None, None, vertices, None)
        return st, L.vap_last_error().decode()

    def grid(out=(None, None), **kw):
        nx, ny = C.c_int(-1), C.c_int(-1)
        st = L.vap_plan_grid(None, *scene(**kw), out[0], out[1], C.byref(nx), C.byref(ny))
        return st, L.vap_last_error().decode(), nx.value, ny.value
    return _lib, one, seeds, grid


def test_entry_points_check_their_arguments_before_the_device():
    """Every VAP_ERR_INVALID / VAP_ERR_UNSUPPORTED case of the header, by value, with a null context.  A call whose
    arguments are all good gets as far as the context and fails there ("null context"): that tells the argument errors
    from the context's."""
    _lib, one, seeds, grid = _abi()
    INV, UNS = _lib.VAP_ERR_INVALID, _lib.VAP_ERR_UNSUPPORTED
    st, msg = seeds()
    assert st == INV and "null context" in msg                       # good arguments: stopped by the context only

    def refused(call, status, **kw):
        st, msg = call(**kw)[:2]
        assert st == status and "null context" not in msg, (kw, st, msg)

    for kw in (dict(cell=0.0), dict(cell=-0.25), dict(cell=np.nan), dict(cell=np.inf), dict(radius=-0.1), dict(radius=np.nan),
               dict(radius=np.inf), dict(margin=np.nan), dict(margin=np.inf), dict(field=None),
               dict(field=(-6, -6, np.nan, 6)), dict(field=(6, -6, -6, 6)), dict(circles=[(0, 0, 0.0)]),
               dict(circles=[(0, np.inf, 1.0)]), dict(polygons=[np.array([[0, 0], [0, 1], [1, 0.0]])]),       # clockwise
               dict(polygons=[np.array([[0, 0], [1, 0.0]])])):
        refused(seeds, INV, **kw)
        refused(grid, INV, **kw)
    for kw in (dict(W=1), dict(W=0), dict(R=-1), dict(starts=None), dict(goals=None), dict(wp=None),
               dict(vertices=one, max_vertices=1)):
        refused(seeds, INV, **kw)
    for kw in (dict(cell=12.0 / 129), dict(cell=1e-6), dict(field=(-6, -6, 6, 6.001), cell=12.0 / 128),
               dict(circles=[(0, 0, 0.1)] * 257), dict(polygons=[np.array([[0, 0], [1, 0], [0, 1.0]])] * 257)):
        refused(seeds, UNS, **kw)
        refused(grid, UNS, **kw)
    refused(seeds, UNS, W=2049)
    assert seeds(W=2048)[0] == INV and "null context" in seeds(W=2048)[1] and "null context" in seeds(W=2)[1]
    # the grid's shape needs no context; the limit is nx * ny = 16384
    assert grid() == (_lib.VAP_OK, grid()[1], 48, 48)
    assert grid(cell=12.0 / 128)[2:] == (128, 128) and grid(cell=12.0 / 128)[0] == _lib.VAP_OK
    assert grid(field=(-6, -6, 5.9, 6))[2:] == (48, 48) and grid(field=(-6, -6, 5.9, 3.1), cell=0.5)[2:] == (24, 19)
    st, msg = grid(out=(one, one))[:2]
    assert st == INV and "null context" in msg


def test_plan_module_argument_errors():
    from vexautonomousplanner_amd import footprint as fp
    from vexautonomousplanner_amd import plan
    sc = fp.Scene(field=pr.FIELD, circles=[(0.0, 0.0, 0.5)])
    pts = np.zeros((1, 2))
    with pytest.raises(TypeError):
        plan.seeds(pts, pts, "scene", 5, 0.75)
    with pytest.raises(ValueError, match="field box"):
        plan.seeds(pts, pts, fp.Scene(field=None), 5, 0.75)
    with pytest.raises(ValueError, match="field box"):
        plan.clearance_grid(fp.Scene(field=None), 0.25, 0.75)
    for kw in (dict(waypoints=1), dict(waypoints=2049), dict(waypoints=4.5), dict(cell=0.0), dict(cell=float("nan")), dict(radius=-1.0),
               dict(radius=float("inf")), dict(margin=float("nan")), dict(cell=12.0 / 129), dict(vertices=True, max_vertices=1)):
        args = dict(waypoints=5, radius=0.75)
        args.update(kw)
        with pytest.raises(ValueError):
            plan.seeds(pts, pts, sc, args.pop("waypoints"), args.pop("radius"), **args)
    for kw in (dict(cell=-1.0), dict(radius=float("nan")), dict(cell=0.01)):
        args = dict(cell=0.25, radius=0.75)
        args.update(kw)
        with pytest.raises(ValueError):
            plan.clearance_grid(sc, **args)
    assert plan.grid_shape(sc, 0.25) == (48, 48) and plan.grid_shape(fp.Scene(field=(-6, -6, 5.9, 3.1)), 0.5) == (19, 24)
    sq = fp.rectangle(18, 18)
    assert plan.circumscribed_radius(sq) == pytest.approx(0.75 * np.sqrt(2), rel=1e-15) and plan.inscribed_radius(sq) == 0.75
    assert plan.inscribed_radius(fp.rectangle(12, 18, 3)) == 0.5 and plan.circumscribed_radius(fp.rectangle(12, 18, 3)) == pytest.approx(np.hypot(1.0, 0.5))
    with pytest.raises(ValueError):
        plan.inscribed_radius(fp.rectangle(12, 18, 12))                  # the tracked point is outside the body
