"""Deterministic families of clearance cases for the two exact geometries: a footprint against a static scene
(vap_footprint.h: poly_clearance, circle_clearance, row_clearance[_capped]) and two moving footprints against each other
(vap_conflict.h: pair_clearance, sat_axes).  Shared by tests/test_scene_cases_cpu.py, which proves on the references alone
that every family holds what it is named for, and tests/test_gpu_clearance_scenes.py, which holds the kernels to them.

A static case is a dict: name, rows (B, cap, 8), counts (B,), foot, field (or None), polygons, circles, margin, X, and
``expect`` where the family has closed forms.  A pair case: name, rows_a, counts_a, foot_a, rows_o, counts_o, foot_o,
margin, X, expect.  X is the largest coordinate magnitude in the case (poses, vertices, centres plus radii), and

    tol(X) = max(1e-12, 16 * eps * X),   eps = 2**-52

is what a kernel may differ from the float64 reference by: the a-priori rounding of a short dot product of world
coordinates.  At field scale it is the neighbouring tests' TOL.  The float64 references hold a quarter of it against their
own long double evaluation (test_scene_cases_cpu.py)."""
import functools
import math

import numpy as np

import conflict_ref as cr
import footprint_ref as fr
import test_gpu_footprint as tgf

EPS = 2.0 ** -52
FAR = (2.0 ** 10, 2.0 ** 17, 2.0 ** 23)
SHIFTS = (0, 5, -5)
SQUARE = tgf.SQUARE                                                                   # 1.5 ft
UNIT = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])                 # 1 ft
TWO = 2.0 * UNIT                                                                      # 2 ft
SLIVER = np.array([[-2.0, -0.0004], [2.0, -0.0004], [2.0, 0.0004], [-2.0, 0.0004]])   # 4 ft x 0.0008 ft


def tol(X):
    return max(1e-12, 16.0 * EPS * float(X))


def ambiguous(X):
    """An index is compared where the reference's best and runner-up differ by more than this: the neighbouring tests'
    AMBIGUOUS, and at least twice tol(X): closer than that, the kernel's and the reference's own rounding can order the two
    differently (at X = 2^23 one ulp of a coordinate is 1.9e-9 ft)."""
    return max(1e-9, 2.0 * tol(X))


def box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def ngon(m, radius, cx=0.0, cy=0.0, phase=0.0):
    a = phase + 2.0 * np.pi * np.arange(m) / m
    return np.stack([cx + radius * np.cos(a), cy + radius * np.sin(a)], axis=1)


def oval16(rx, ry):
    """An irregular 16-vertex convex outline on an ellipse."""
    k = np.arange(16)
    a = 2.0 * np.pi * k / 16 + 0.1 * np.sin(3.0 * k)
    return np.stack([rx * np.cos(a), ry * np.sin(a)], axis=1)


def rows_of(heading, x, y):
    """(n, 8) rows from per-row heading, x, y (scalars broadcast)."""
    h, x, y = np.broadcast_arrays(np.asarray(heading, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    r = np.zeros((len(h), 8))
    r[:, 0], r[:, 4], r[:, 6], r[:, 7] = 0.01 * np.arange(len(h)), h, x, y
    return r


def stack(routes, cap=None):
    """(B, cap, 8) rows and (B,) counts from routes of different lengths; rows past a count are NaN."""
    cap = cap or max(len(r) for r in routes)
    out = np.full((len(routes), cap, 8), np.nan)
    for b, r in enumerate(routes):
        out[b, :len(r)] = r
    return out, np.array([len(r) for r in routes], dtype=np.int32)


def walks(rng, B, cap, centre, spread, step=0.05):
    """Random-walk poses as tgf.random_rows, started within `spread` of `centre`."""
    rows = tgf.random_rows(rng, B, cap)
    for b in range(B):
        rows[b, :, 6:8] += np.asarray(centre) + rng.uniform(-spread, spread, 2) - rows[b, 0, 6:8]
        if step != 0.05:
            rows[b, :, 6:8] = rows[b, 0, 6:8] + (rows[b, :, 6:8] - rows[b, 0, 6:8]) * (step / 0.05)
    return rows


def _amax(*arrays):
    v = [np.abs(np.asarray(a, dtype=np.float64)).ravel() for a in arrays]
    v = np.concatenate([a[np.isfinite(a)] for a in v] + [np.zeros(1)])
    return float(v.max())


def static_case(name, rows, counts, foot, field, polygons, circles, margin, **extra):
    rows, counts = np.ascontiguousarray(rows, dtype=np.float64), np.asarray(counts, dtype=np.int32)
    circles = np.asarray(circles, dtype=np.float64).reshape(-1, 3)
    polygons = [np.asarray(p, dtype=np.float64) for p in polygons]
    live = [rows[b, :counts[b], 6:8] for b in range(len(rows))]
    X = _amax(*live, *polygons, [] if field is None else field, np.abs(circles[:, :2]) + circles[:, 2:3])
    return dict(name=name, rows=rows, counts=counts, foot=np.asarray(foot, dtype=np.float64), field=None if field is None else tuple(float(v) for v in field),
                polygons=polygons, circles=circles, margin=float(margin), X=X, **extra)


def pair_case(name, rows_a, counts_a, foot_a, rows_o, counts_o, foot_o, margin, **extra):
    rows_a, rows_o = np.ascontiguousarray(rows_a, dtype=np.float64), np.ascontiguousarray(rows_o, dtype=np.float64)
    counts_a, counts_o = np.asarray(counts_a, dtype=np.int32), np.asarray(counts_o, dtype=np.int32)
    live = [r[b, :c[b], 6:8] for r, c in ((rows_a, counts_a), (rows_o, counts_o)) for b in range(len(r))]
    return dict(name=name, rows_a=rows_a, counts_a=counts_a, foot_a=np.asarray(foot_a, dtype=np.float64), rows_o=rows_o, counts_o=counts_o,
                foot_o=np.asarray(foot_o, dtype=np.float64), margin=float(margin), X=_amax(*live, foot_a, foot_o), **extra)


# ---- references -------------------------------------------------------------------------------------------------------
def static_reference(case, ftype=np.float64):
    """fr.route_summary of every route (one evaluation over all rows of the case); float64 results are kept on the case."""
    key = ("ref", np.dtype(ftype).name)
    if key not in case:
        n = [int(c) for c in case["counts"]]
        allrows = np.concatenate([case["rows"][b, :n[b]] for b in range(len(n))] + [np.zeros((0, 8))])
        kw = dict(field=case["field"], polygons=case["polygons"], circles=case["circles"])
        # a repeated pose is evaluated once: the same numbers in, the same bits out (a NaN pose gives NaN whatever the rest)
        poses = np.nan_to_num(allrows[:, [4, 6, 7]], nan=np.inf)
        _, first, inverse = np.unique(poses, axis=0, return_index=True, return_inverse=True)
        v, el, gap = (a[inverse.ravel()] for a in fr.row_clearance(allrows[first], case["foot"], ftype=ftype, **kw))
        at = np.concatenate([[0], np.cumsum(n)])
        case[key] = [fr.summarise(v[at[b]:at[b + 1]], el[at[b]:at[b + 1]], gap[at[b]:at[b + 1]], case["margin"]) if n[b] else
                     fr.route_summary(case["rows"][b], 0, case["foot"], margin=case["margin"], **kw) for b in range(len(n))]
    return case[key]


def pair_reference(case, shift=0, matched=False, margin=None, ftype=np.float64):
    margin = case["margin"] if margin is None else margin
    key = ("ref", shift, matched, margin, np.dtype(ftype).name)
    if key not in case:
        n = min(len(case["rows_a"]), len(case["rows_o"])) if matched else None
        case[key] = cr.conflicts(case["rows_a"][:n], case["counts_a"][:n], case["foot_a"], case["rows_o"][:n], case["counts_o"][:n],
                                 case["foot_o"], margin, shift, matched=matched, ftype=ftype)
    return case[key]


def static_D(case):
    """The largest |float64 - long double| over the case's per-row clearances."""
    d = 0.0
    for a, b in zip(static_reference(case), static_reference(case, np.longdouble)):
        if len(a["rows"]):
            assert np.array_equal(np.isnan(a["rows"]), np.isnan(b["rows"]))
            d = max(d, float(np.nanmax(np.abs(a["rows"] - b["rows"]), initial=0.0)))
    return d


def pair_D(case, shift=0):
    a, b = pair_reference(case, shift), pair_reference(case, shift, ftype=np.longdouble)
    d = 0.0
    for k in a["pair_rows"]:
        assert np.array_equal(np.isnan(a["pair_rows"][k]), np.isnan(b["pair_rows"][k]))
        d = max(d, float(np.nanmax(np.abs(a["pair_rows"][k] - b["pair_rows"][k]), initial=0.0)))
    return d


# ---- static: exact ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact():
    """Heading 0, coordinates multiples of 2^-10, a 2 ft square robot, axis-parallel boxes with edges of 1 and 2 ft, dyadic
    circles: every operation of the definition is exact (row 2's triangle has inexact normals, but the axis that decides
    it is the robot's own and its vertex lies on the robot's edge, so its row is exactly 0 too).  One row per class, each in
    its own 16 ft cell; ``expect``: (clearance, element) per row."""
    cells = 16.0 * np.arange(11)
    sq2 = math.sqrt(2.0)
    # per row: robot offset in its cell, the element (relative to the cell), the clearance, the element's kind
    spec = [((0, 0), box(1, -1, 3, 1), 0.0),                       # edge flush on edge
            ((0, 0), box(1, 1, 2, 2), 0.0),                        # vertex on vertex
            ((0, 0), np.array([[1.0, 0.0], [3.0, -1.0], [3.0, 1.0]]), 0.0),   # a vertex on the interior of the robot's edge
            ((0, 0), box(1.125, -1, 3.125, 1), 0.125),             # separated by 2^-3 in x
            ((0, 0), box(2, 2, 3, 3), sq2),                        # separated diagonally by (1, 1)
            ((0, 0), box(0.75, -1, 2.75, 1), -0.25),               # overlapping by 2^-2
            ((0, 7.0), None, 0.0),                                 # flush on the wall (ymax = 8)
            ((0, 7.25), None, -0.25),                              # 2^-2 through the wall
            ((0, 0), (2.0, 0.0, 1.0), 0.0),                        # a circle tangent to an edge
            ((0, 0), (1.75, 2.0, 1.25), 0.0),                      # a circle tangent at a vertex (3-4-5)
            ((0, 0), (0.5, 0.0, 0.25), -0.75)]                     # a circle's centre inside the robot
    polygons, circles, x, y, expect = [], [], [], [], []
    n_poly = sum(1 for _, e, _ in spec if isinstance(e, np.ndarray))
    for k, (off, e, v) in enumerate(spec):
        x.append(cells[k] + off[0])
        y.append(off[1])
        if e is None:
            expect.append((v, -1))
        elif isinstance(e, np.ndarray):
            expect.append((v, len(polygons)))
            polygons.append(e + [cells[k], 0.0])
        else:
            expect.append((v, n_poly + len(circles)))
            circles.append((cells[k] + e[0], e[1], e[2]))
    rows = rows_of(0.0, x, y)[None]
    return static_case("exact", rows, [len(spec)], TWO, (-16.0, -8.0, 176.0, 8.0), polygons, circles, 2.0 ** -4, expect=expect)


# ---- static: ties -----------------------------------------------------------------------------------------------------
TIE_R0 = (0, 63, 64, 255, 256, 300)
TIE_ROWS = 700


@functools.lru_cache(maxsize=None)
def ties():
    """Per variant six routes of 700 rows (every thread of the 256-thread workgroup holds two or three): the 2 ft robot
    comes in from the left along y = 0 at heading 0, 2^-6 ft a row, and stands at the origin from row r0 to the end.  At the
    standing pose polygons 3 and 200 (two copies of one box), two equal circles and, in one variant, the wall give the same
    clearance exactly (dyadic data); on the way in everything is farther.  The margin lies 2^-7 above the plateau.
    ``expect`` per variant: plateau, min_element."""
    out = []
    for name, plateau, wall, twins in (("apart", 0.5, False, True), ("contact", -0.25, False, True), ("wall", 0.5, True, True),
                                       ("circle", -0.25, False, False)):
        edge = 1.0 + plateau                                   # the x of the tied faces
        polygons = [ngon(3 + k % 14, 1.0, 64.0 + 4.0 * (k % 16), 64.0 + 4.0 * (k // 16), 0.1 * k) for k in range(201)]
        if twins:
            polygons[3] = box(edge, -1, edge + 2, 1)
            polygons[200] = polygons[3].copy()
        circles = [(edge + 1.0, 0.0, 1.0), (edge + 1.0, 0.0, 1.0)]
        field = (-64.0, -64.0, edge if wall else 192.0, 192.0)
        routes = [rows_of(0.0, -np.maximum(r0 - np.arange(TIE_ROWS), 0) / 64.0, 0.0) for r0 in TIE_R0]
        rows, counts = stack(routes)
        out.append(static_case("ties_" + name, rows, counts, TWO, field, polygons, circles, plateau + 2.0 ** -7,
                               expect=dict(plateau=plateau, element=-1 if wall else (3 if twins else 201))))
    return out


# ---- static: containment ----------------------------------------------------------------------------------------------
TRIANGLE = ngon(3, 0.25 / math.sqrt(3.0), 20.0, 0.0, 0.4)              # 0.25 ft edges
CONTAIN_ROWS = 300


@functools.lru_cache(maxsize=None)
def containment():
    """Four routes of 300 rows, each a slow walk with turning heading through one element, 20 ft apart: the 1.5 ft robot
    into and out of a 16-gon of radius 3 ft; over a 0.25 ft triangle; into and out of a circle of r = 5 ft; over a circle of
    r = 0.1 ft.  The walk's distance from the element's centre falls to 0 at row 110.6 and rises again."""
    t = np.arange(CONTAIN_ROWS) / (CONTAIN_ROWS - 1.0)
    routes = []
    for b, rho_max in enumerate((5.2, 1.6, 7.0, 1.6)):
        rho = rho_max * np.abs(t - 0.37) / 0.63
        th = 0.7 + 5.0 * t + b
        routes.append(rows_of(0.3 + 4.0 * t - b, 20.0 * b + rho * np.cos(th), rho * np.sin(th)))
    rows, counts = stack(routes)
    return static_case("containment", rows, counts, SQUARE, None, [ngon(16, 3.0, 0.0, 0.0, 0.1), TRIANGLE],
                       [(40.0, 0.0, 5.0), (60.0, 0.0, 0.1)], 0.05)


# ---- static: shapes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shapes():
    """Random-walk poses (8 routes of 120 rows each) around: 16-vertex polygons under a 16-vertex robot; a triangle robot; a
    4 ft x 0.0008 ft sliver; a 1e-3 ft pentagon; a 1e3 ft square whose edge passes within a foot of the routes."""
    out = []
    rng = np.random.default_rng(2024)
    B, cap = 8, 120
    counts = np.full(B, cap)
    # the polygons are narrower than the robot, so a saturated row takes its value from the polygon's own extent
    polys = [tgf.random_convex(rng, 16, 5.0 * (k % 3) - 5.0, 5.0 * (k // 3) - 2.5, rng.uniform(0.5, 0.9)) for k in range(6)]
    out.append(static_case("shapes_16", walks(rng, B, cap, (0, 0), 5.0), counts, oval16(1.4, 1.1), (-10.0, -10.0, 10.0, 10.0), polys,
                           [(-2.5, 0.0, 0.3)], 0.1))
    polys = [tgf.random_convex(rng, int(rng.integers(9, 17)), *c, 0.7) for c in ((-1.5, 1.0), (1.5, -1.0))]
    out.append(static_case("shapes_triangle", walks(rng, B, cap, (0, 0), 2.0), counts, ngon(3, 0.8, 0.1, 0.0, 0.2), (-5.0, -5.0, 5.0, 5.0),
                           polys, [(0.0, 0.0, 0.2), (2.0, 2.0, 0.5)], 0.1))
    c, s = math.cos(0.3), math.sin(0.3)
    sliver = SLIVER @ np.array([[c, s], [-s, c]]) + [1.0, 0.5]
    out.append(static_case("shapes_sliver", walks(rng, B, cap, (1.0, 0.5), 1.5), counts, SQUARE, None, [sliver], [], 0.1))
    out.append(static_case("shapes_pentagon", walks(rng, B, cap, (-2.0, 1.0), 1.0, step=0.02), counts, SQUARE, None,
                           [ngon(5, 1e-3 / (2.0 * math.sin(math.pi / 5)), -2.0, 1.0, 0.3)], [], 0.1))
    big = box(1.5, -500.0, 1001.5, 500.0)
    out.append(static_case("shapes_big", walks(rng, B, cap, (0.3, 0.0), 0.6, step=0.02), counts, SQUARE, None, [big], [], 0.1))
    return out


# ---- static: full -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full():
    """The scene limits: 256 polygons of 16 vertices (4096 vertices) on a 16 x 16 lattice 4 ft apart, 256 circles between
    them, walls, a 16-vertex robot.  Two routes of 300 rows run past polygon 255, circle 255 (element 511) and into the
    wall, one each way, holding every pose for three rows (the brute-force reference costs 20 ms a pose here); three routes
    of 20 rows stay with one of the three.  ``expect``: the short routes' elements."""
    polygons = [ngon(16, 0.6, 4.0 * (k % 16), 4.0 * (k // 16), 0.05 * k) for k in range(256)]
    circles = [(4.0 * (k % 16) + 2.0, 4.0 * (k // 16) + 2.0, 0.5) for k in range(256)]
    t = (np.arange(300) // 3) / 99.0
    u = np.arange(20) / 19.0
    routes = [rows_of(0.4 + 3.0 * t, 58.5 + 6.1 * t, 61.0 + 0.1 * np.sin(7.0 * t)),
              rows_of(-1.0 - 2.5 * t, 64.55 - 6.0 * t, 60.95 + 0.05 * np.cos(9.0 * t)),
              rows_of(0.2 + 2.0 * u, 59.5 + 1.0 * u, 61.0), rows_of(1.0 - 2.0 * u, 61.6 + 0.8 * u, 61.0),
              rows_of(0.5 + 2.0 * u, 64.2 + 0.4 * u, 61.0)]
    rows, counts = stack(routes)
    return static_case("full", rows, counts, oval16(0.45, 0.3), (-3.0, -3.0, 65.0, 65.0), polygons, circles, 0.05, expect=(255, 511, -1))


# ---- far: quantised to 2^-20 ft and translated by (X, -X) -----------------------------------------------------------------
def _q(a):
    return np.round(np.asarray(a, dtype=np.float64) * 2.0 ** 20) / 2.0 ** 20


def far_static(case, X):
    rows = case["rows"].copy()
    rows[:, :, 6], rows[:, :, 7] = _q(rows[:, :, 6]) + X, _q(rows[:, :, 7]) - X
    f = case["field"]
    field = None if f is None else (_q(f[0]) + X, _q(f[1]) - X, _q(f[2]) + X, _q(f[3]) - X)
    circles = _q(case["circles"]) + [X, -X, 0.0]
    return static_case(f"{case['name']}_far{int(X)}", rows, case["counts"], case["foot"], field, [_q(p) + [X, -X] for p in case["polygons"]],
                       circles, case["margin"])


@functools.lru_cache(maxsize=None)
def far(X):
    """``shapes`` and ``containment`` quantised and translated: exact translations, so the geometry at X is that at 0.
    Returns (case at X, case at 0) pairs."""
    return [(far_static(c, X), far_static(c, 0.0)) for c in shapes() + [containment()]]


def far_pair(case, X):
    a, o = case["rows_a"].copy(), case["rows_o"].copy()
    for r in (a, o):
        r[:, :, 6], r[:, :, 7] = _q(r[:, :, 6]) + X, _q(r[:, :, 7]) - X
    return pair_case(f"{case['name']}_far{int(X)}", a, case["counts_a"], case["foot_a"], o, case["counts_o"], case["foot_o"], case["margin"])


@functools.lru_cache(maxsize=None)
def pair_far(X):
    return [(far_pair(c, X), far_pair(c, 0.0)) for c in pair_shapes()]


# ---- pairs: exact -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_exact():
    """A 1 ft square (side A) against a parked 2 ft square at the origin, heading 0, dyadic poses: a flush pass-by along the
    top edge, corner to corner along the diagonal, an overlap of 2^-2, and centred inside (minus the narrower extent).
    ``expect``: per A route (clearance, row, first row below the margin 2^-4) and the per-row closed forms."""
    xs = -3.0 + np.arange(25) / 4.0
    d = np.abs(8 - np.arange(17)) / 8.0
    routes = [rows_of(0.0, xs, 1.5), rows_of(0.0, 1.5 + d, 1.5 + d), rows_of(0.0, [1.25], 0.0), rows_of(0.0, [0.0], 0.0)]
    per_row = [np.maximum(np.abs(xs) - 1.5, 0.0), np.sqrt(2.0 * d * d), np.array([-0.25]), np.array([-1.0])]
    rows_a, counts_a = stack(routes)
    rows_o, counts_o = stack([rows_of(0.0, [0.0], 0.0)] * 4)
    return pair_case("pair_exact", rows_a, counts_a, UNIT, rows_o, counts_o, TWO, 2.0 ** -4,
                     expect=dict(pair=[(0.0, 6, 6), (0.0, 8, 8), (-0.25, 0, 0), (-1.0, 0, 0)], per_row=per_row))


# ---- pairs: plateau ---------------------------------------------------------------------------------------------------
PLATEAU_R0 = (0, 63, 64, 130)
PLATEAU_ROWS = 400


@functools.lru_cache(maxsize=None)
def pair_plateau():
    """400 rows (seven 64-row blocks).  Stand: A (1.5 ft) comes in along x at 2^-5 ft a row and from row r0 stands at O's
    exact pose, O stands throughout; heading 0, so every row is exact: -(1.5 - k / 32) while they overlap, k rows before r0.
    The margin -1 - 2^-7 is first crossed 15 rows before r0.  Parallel: two 1 ft squares 2 ft apart laterally travel at
    +2^-6 ft a row: every row is exactly 1.0, whatever the shift."""
    r = np.arange(PLATEAU_ROWS)
    a, counts = stack([rows_of(0.0, np.maximum(r0 - r, 0) / 32.0, 0.0) for r0 in PLATEAU_R0])
    o, counts_o = stack([rows_of(0.0, np.zeros(PLATEAU_ROWS), 0.0)] * 4)
    stand = pair_case("pair_plateau_stand", a, counts, SQUARE, o, counts_o, SQUARE, -1.0 - 2.0 ** -7,
                      expect=dict(clearance=-1.5, row=list(PLATEAU_R0), first=[max(r0 - 15, 0) for r0 in PLATEAU_R0]))
    a, counts = stack([rows_of(0.0, r / 64.0, 0.0), rows_of(0.0, r / 64.0, 4.0)])
    o, counts_o = stack([rows_of(0.0, r / 64.0, 2.0), rows_of(0.0, r / 64.0, 6.0)])
    parallel = pair_case("pair_plateau_parallel", a, counts, UNIT, o, counts_o, UNIT, 1.0, expect=dict(clearance=1.0))
    return stand, parallel


# ---- pairs: shapes ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_shapes():
    """Random-walk poses: a triangle against a 16-gon, a square against a sliver, a 20 ft robot against a 0.01 ft one (apart,
    overlapping and contained).  The narrower robot is side O: the reference evaluates in O's frame, where O's own extents
    are the same numbers at every row, as both extents are in the kernel."""
    rng = np.random.default_rng(77)
    out = []
    for name, fa, fo, spread in (("triangle_16gon", ngon(3, 0.7, 0.1, 0.0, 0.2), oval16(0.8, 0.6), 2.0), ("square_sliver", SQUARE, SLIVER, 2.5)):
        a, o = walks(rng, 6, 150, (0, 0), spread), walks(rng, 5, 130, (0, 0), spread)
        ca, co = rng.integers(40, 151, 6), rng.integers(40, 131, 5)
        ca[0], co[0] = 150, 130
        out.append(pair_case("pair_" + name, a, ca, fa, o, co, fo, 0.1))
    # the small robot's routes start 2 .. 16 ft from the large one's centre, abeam one of its edges: inside it, across an edge,
    # outside; routes 2 .. 4 start at the edge and creep, 2e-3 ft a row, so that rows fall inside the 0.01 ft between touching
    # and saturated
    a = np.concatenate([walks(rng, 1, 150, (d * math.cos(b * math.pi / 2), d * math.sin(b * math.pi / 2)), 0.005 if 2 <= b <= 4 else 0.2,
                              step=0.002 if 2 <= b <= 4 else 0.05) for b, d in enumerate((2.0, 9.6, 9.99, 10.0, 10.01, 10.4, 13.0, 16.0))])
    o = walks(rng, 3, 130, (0, 0), 0.01, step=0.0005)
    o[:, :, 4] = 0.002 * o[:, :, 4]                                 # the large robot creeps and hardly turns: its edges stay near x, y = +-10
    out.append(pair_case("pair_large_small", o, rng.integers(60, 131, 3), 20.0 * UNIT, a, np.full(8, 150), 0.01 * UNIT, 0.1))
    return out


# ---- pairs: others ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_others():
    """24 O routes (two 16-route tiles) parked on a lattice 4 ft apart; O 9 is a copy of O 3 and O 20 of O 2.  A 0 passes
    O 3's place and A 1 passes O 2's, 0.3 ft off their corners, with turning heading: min_other is 3 and 2 (the smaller twin,
    inside a tile and across tiles), and at the margin 0.5 exactly the twins conflict."""
    o = [rows_of(0.1 * k, [4.0 * (k % 6)] * 3, [4.0 * (k // 6)] * 3) for k in range(24)]
    o[9], o[20] = o[3].copy(), o[2].copy()
    t = np.arange(100) / 99.0
    a = [rows_of(0.3 + 1.1 * t, 11.0 + 2.1 * t, 1.25 + 0.07 * t), rows_of(-0.2 - 0.9 * t, 9.0 - 2.1 * t, -1.2 - 0.05 * t)]
    rows_a, counts_a = stack(a)
    rows_o, counts_o = stack(o)
    return pair_case("pair_others", rows_a, counts_a, UNIT, rows_o, counts_o, UNIT, 0.5, expect=dict(min_other=[3, 2], n_conflicts=[2, 2]))


# ---- NaN rows ---------------------------------------------------------------------------------------------------------
NAN_BLOCK = (128, 192)


@functools.lru_cache(maxsize=None)
def nan_rows():
    """Routes of 300 rows with NaN poses in the middle.  Static: the 1.5 ft robot drives along y = 0 past a circle (abeam at
    row 75 one way, 224 the other) and a triangle that comes nearer (abeam inside rows 128 .. 191).  Route 0 has single NaNs in
    column 4, 6 and 7 and the whole block 128 .. 191 NaN, its minimum before the block; route 1 the same the other way, its
    minimum after; route 2 a NaN exactly at the row that would be its minimum; route 3 only NaN rows.  Pairs: these routes
    against a parked robot and against a moving one with NaN rows of its own (a whole 64-row block, and singles)."""
    t = np.arange(300) / 299.0
    fwd = rows_of(0.1 + 2.0 * t, -1.5 + 6.0 * t, 0.02 * np.sin(5.0 * t))
    back = rows_of(-0.4 - 2.0 * t, 4.5 - 6.0 * t, 0.02 * np.cos(4.0 * t))
    kw = dict(foot=SQUARE, field=(-6.0, -6.0, 6.0, 6.0), polygons=[ngon(3, 0.3, 1.7, -1.0, 0.5)], circles=[(0.0, 1.2, 0.3)], margin=0.2)
    r0, r1, r2, r3 = fwd.copy(), back.copy(), fwd.copy(), fwd.copy()
    for r in (r0, r1):
        r[NAN_BLOCK[0]:NAN_BLOCK[1], [4, 6, 7]] = np.nan
    r0[10, 4], r0[60, 6], r0[250, 7] = np.nan, np.nan, np.nan
    r1[5, 7], r1[200, 4], r1[280, 6] = np.nan, np.nan, np.nan
    whole = fr.route_summary(fwd, 300, kw["foot"], kw["field"], kw["polygons"], kw["circles"])
    r2[whole["min_row"], 6] = np.nan
    r3[:, [4, 6, 7]] = np.nan
    rows, counts = stack([r0, r1, r2, r3])
    static = static_case("nan_rows", rows, counts, kw["foot"], kw["field"], kw["polygons"], kw["circles"], kw["margin"],
                         masked_min_row=whole["min_row"])
    o1 = rows_of(0.5 - 1.0 * t, 4.0 - 5.0 * t, -1.7 + 0.3 * t)
    o1[64:128, [4, 6, 7]] = np.nan
    o1[3, 6], o1[150, 4], o1[299, 7] = np.nan, np.nan, np.nan
    rows_o, counts_o = stack([rows_of(0.2, [0.0], [1.7]), o1])
    pair = pair_case("nan_rows_pair", rows, counts, SQUARE, rows_o, counts_o, UNIT, 0.2)
    return static, pair
