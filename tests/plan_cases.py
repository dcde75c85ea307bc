"""The seeded scenes and problems under which the grid planner (vap_plan.hip) is held to tests/plan_ref.py and
tests/occupancy_ref.py: shared by test_plan_cases_cpu.py (which proves ON THE REFERENCE ALONE that the cases reach the
branches they are here for) and test_gpu_plan_cases.py (which runs the kernels on the same inputs).  Plain NumPy; nothing
here touches a device.

Why these cases: the planner's other tests run three hand-made scenes on an open field (at most 6 polygons, one circle,
64 problems, a couple of hundred traced cells, W <= 9).  On those k_plan_clearance's polygon loop runs one chunk, no
workgroup of k_plan_seeds takes a second problem, plan_pull tests one batch of candidates, and nearly every pair of cells
is visible.  A scene is a dict of field, cell, polygons, circles, radius and margin, as plan_ref.scene_args takes it."""
import functools

import numpy as np

import occupancy_ref as oc
import plan_ref as pr
from range_cases import random_convex

GAP = 1e-9                        # no cell's clearance lies this close to the margin: the condition of test_gpu_plan.py
BLOCKS = 1024                     # kPlanMaxBlocks: workgroup b takes problems b, b + 1024, b + 2048


def clutter(seed, n_poly, n_circle, field, verts=None, poly_size=(0.15, 0.45), circle_size=(0.08, 0.3)):
    """Random strictly convex counter-clockwise polygons of 3..16 vertices at random orientations (every eighth a 16-gon, so
    the vertex counts vary within a chunk of 32 and a chunk's first vertex row is no round number; ``verts``: all of that
    many) and random circles, centred anywhere in the field box.  Returns dict(field, polygons, circles)."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = field
    polys = []
    for k in range(n_poly):
        n = verts if verts is not None else (16 if k % 8 == 7 else int(rng.integers(3, 17)))
        polys.append(random_convex(rng, n, rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(*poly_size)))
    circles = [(rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(*circle_size)) for _ in range(n_circle)]
    return dict(field=field, polygons=polys, circles=circles)


# ---- the 48 x 48 grid at every chunk shape of k_plan_clearance (kPlanChunkPolys = 32 polygons in LDS at a time) --------------
# name -> (seed, polygons, circles, vertices of every polygon or None): one chunk that is full; one chunk whose vertex rows
# fill the 32 KB buffer exactly (32 x 16 = 512); a second chunk of one polygon; two full chunks; a third of one polygon; the
# documented limits of 256 polygons, 4096 polygon vertices and 256 circles (the 8 KB circle block).
CHUNK_CASES = {
    "32+3": (1, 32, 3, None),
    "32x16gon+0": (2, 32, 0, 16),
    "33+2": (3, 33, 2, None),
    "64+5": (4, 64, 5, None),
    "65+40": (5, 65, 40, None),
    "256x16gon+256": (6, 256, 256, 16),
}
SEEDS_CASES = ("33+2", "65+40")   # cluttered enough to plan in; the 256 + 256 scene leaves almost nothing free


@functools.lru_cache(maxsize=None)
def chunk_scene(name):
    seed, n_poly, n_circle, verts = CHUNK_CASES[name]
    return dict(clutter(seed, n_poly, n_circle, pr.FIELD, verts), cell=0.25, radius=0.2, margin=0.05)


def grids(sc):
    """(clearance, clearance in longdouble, free mask, the smallest |clearance - margin|) of a scene, by the reference."""
    kw = pr.scene_args(sc)
    c = pr.clearance_grid(**kw)
    return c, pr.clearance_grid(ftype=np.longdouble, **kw), c >= sc["margin"], float(np.abs(c - sc["margin"]).min())


def random_problems(seed, n, field, beyond=0.0):
    """(starts, goals), each (n, 2), uniform in the field box grown by ``beyond`` on every side."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(field[:2]) - beyond, np.array(field[2:]) + beyond
    p = rng.uniform(lo, hi, (n, 2, 2))
    return p[:, 0].copy(), p[:, 1].copy()


CLUTTER_W = 7


def clutter_problems(name):
    """48 random (start, goal) pairs in the field of a cluttered 48 x 48 scene."""
    return random_problems(77 + SEEDS_CASES.index(name), 48, pr.FIELD)


# ---- mazes: lists of more than 1024 and more than 2048 traced cells --------------------------------------------------------
def serpentine(n_walls):
    """The 128 x 128 grid over +-6 ft with ``n_walls`` rectangles 0.2 ft thick, evenly spaced, attached alternately to the
    bottom and the top wall and leaving a gap of 1 ft at the other: one corridor that runs the height of the field
    n_walls + 1 times.  The start and the goal stand at the bottom of the two end corridors (n_walls odd: both of them are
    closed at the bottom)."""
    polys = []
    for k in range(n_walls):
        x = -6.0 + 12.0 * (k + 1) / (n_walls + 1)
        y0, y1 = (-6.0, 5.0) if k % 2 == 0 else (-5.0, 6.0)
        polys.append(np.array([[x - 0.1, y0], [x + 0.1, y0], [x + 0.1, y1], [x - 0.1, y1]]))
    half = 6.0 / (n_walls + 1) - 0.05                                # the middle of an end corridor, from the side wall
    return dict(field=pr.FIELD, cell=12.0 / 128, polygons=polys, circles=[], radius=0.1, margin=0.02,
                start=(-6.0 + half, -5.0), goal=(6.0 - half, -5.0))


MAZES = {9: 1026, 19: 2050}       # walls -> the traced list is longer than this: two and three pull batches of 1024
MAZE_W = (2, 33, 1025, 2048)      # no interior waypoint; a few; the waypoint loop's second stride; MAX_WAYPOINTS


@functools.lru_cache(maxsize=None)
def maze_reference(n_walls, max_vertices=128):
    """(scene, free, plan_ref.plan dict at W = 2) of a maze."""
    sc = serpentine(n_walls)
    _, _, free, gap = grids(sc)
    assert gap >= GAP
    return sc, free, pr.plan(sc["start"], sc["goal"], sc["field"], sc["cell"], free, 2, max_vertices)


def with_waypoints(sc, ref, W, max_vertices=None):
    """The reference dict ``ref`` of a problem at another W (and cut to another max_vertices): the same field, cells and
    pulled cells, resampled by plan_ref.resample in float64 and in longdouble."""
    out = dict(ref)
    if max_vertices is not None:
        v = pr.vertices_of(ref["pulled"], sc["start"], sc["goal"], sc["field"], sc["cell"])
        out["vertices"] = np.full((max_vertices, 2), np.nan)
        out["vertices"][:min(len(v), max_vertices)] = v[:max_vertices]
        out["flags"] = (ref["flags"] & ~pr.VERTICES_TRUNCATED) | (pr.VERTICES_TRUNCATED if len(v) > max_vertices else 0)
    for ftype, wk, lk in ((np.float64, "waypoints", "length"), (np.longdouble, "waypoints_ld", "length_ld")):
        v = pr.vertices_of(ref["pulled"], sc["start"], sc["goal"], sc["field"], sc["cell"], ftype)
        out[wk], out[lk] = pr.resample(v, W, ftype)
    return out


# ---- full batches: more problems than workgroups --------------------------------------------------------------------------
BATCH_FIELD = (-3.0, -3.0, 3.0, 3.0)
BATCH_SEEDS = (12, 14)            # scenes with closed pockets: test_plan_cases_cpu.py holds them to the floors below
OCCUPIED_SEED = 12                # the scene of the batches with an occupancy and of the travel
BATCH_R, BATCH_W = 2200, 6
BATCH_FLOORS = dict(unreachable=50, clean=400, more_than_3_vertices=400, exactly_2_vertices=400, kinds_differ=20)


@functools.lru_cache(maxsize=None)
def batch_scene(seed):
    """The 24 x 24 cluttered grid: 14 polygons and 6 circles on +-3 ft."""
    return dict(clutter(seed, 14, 6, BATCH_FIELD, poly_size=(0.15, 0.6), circle_size=(0.1, 0.35)), cell=0.25, radius=0.15, margin=0.05)


def hand_placed(sc, free):
    """[(name, start, goal, does the device reach the trace)]: the problems that end early or sit on an edge of the
    arithmetic.  ``free`` picks a blocked cell and two far free cells of this scene."""
    f, h = sc["field"], sc["cell"]
    xs, ys = pr.centres(f, h)
    blocked = np.argwhere(~free)
    inner = blocked[(blocked.min(axis=1) > 0) & (blocked[:, 0] < free.shape[0] - 1) & (blocked[:, 1] < free.shape[1] - 1)]
    bj, bi = (int(v) for v in inner[len(inner) // 2])                # a blocked cell off the border: inside an obstacle
    fr = np.argwhere(free)
    (aj, ai), (cj, ci) = (int(v) for v in fr[0]), (int(v) for v in fr[-1])
    a, c, b = (xs[ai], ys[aj]), (xs[ci], ys[cj]), (xs[bi], ys[bj])
    return [("nan start", (np.nan, 0.0), c, False),
            ("nan goal", a, (0.5, np.nan), False),
            ("inf start", (np.inf, 0.0), c, False),
            ("start = goal", a, a, True),
            ("one cell", (a[0] - 0.1, a[1] - 0.1), (a[0] + 0.1, a[1] + 0.1), True),
            ("lattice lines", (f[0] + 5 * h, f[1] + 7 * h), (f[0] + 19 * h, f[1] + 17 * h), True),
            ("xmax and ymax", (f[2], f[3]), (f[0], f[1]), True),
            ("on xmax", (f[2], a[1]), a, True),
            ("start inside an obstacle", b, c, True),
            ("goal inside an obstacle", a, b, True),
            ("both inside one obstacle", b, (b[0] + 0.05, b[1] - 0.05), True),
            ("far outside", (f[0] - 40.0, f[3] + 40.0), c, True)]


@functools.lru_cache(maxsize=None)
def batch_problems(seed):
    """(starts, goals) of BATCH_R problems on batch_scene(seed): drawn a little beyond the field box, so that clamping and
    snapping occur; the hand-placed problems at r = 0 .. 11 (random problems behind them at r + 1024) and again at
    r = 1124 .. 1135 (random problems before them at r - 1024), so both orders meet in one workgroup."""
    sc = batch_scene(seed)
    starts, goals = random_problems(1000 + seed, BATCH_R, sc["field"], beyond=0.2)
    free = grids(sc)[2]
    hp = hand_placed(sc, free)
    for base in (0, BLOCKS + 100):
        for k, (_, s, g, _) in enumerate(hp):
            starts[base + k], goals[base + k] = s, g
    # the three non-finite problems share their workgroups with a long route for certain: to the first free cell from
    # the free cell farthest from it
    xs, ys = pr.centres(sc["field"], sc["cell"])
    aj, ai = (int(v) for v in np.argwhere(free)[0])
    d = pr.dijkstra(free, sc["cell"], (ai, aj))
    fj, fi = np.unravel_index(int(np.argmax(np.where(np.isfinite(d), d, -1.0))), d.shape)
    for k in (BLOCKS, BLOCKS + 1, BLOCKS + 2, 100, 101, 102):
        starts[k], goals[k] = (xs[fi], ys[fj]), (xs[ai], ys[aj])
    return starts, goals


@functools.lru_cache(maxsize=None)
def batch_reference(seed):
    """(scene, starts, goals, plan_ref.plan dicts, free) of a full batch; the distance fields are shared by goal cell."""
    sc = batch_scene(seed)
    starts, goals = batch_problems(seed)
    _, _, free, gap = grids(sc)
    assert gap >= GAP
    fields = {}
    ref = [pr.plan(s, g, sc["field"], sc["cell"], free, BATCH_W, fields=fields) for s, g in zip(starts, goals)]
    return sc, starts, goals, ref, free


def kind(ref):
    """Whether the device's workgroup goes through trace, pull and resample for this problem (a route was found)."""
    return ref["n_vertices"] > 0


# ---- full batches with an occupancy ------------------------------------------------------------------------------------------
NEVER = (oc.INT_MAX, oc.INT_MIN)
WALL_COLUMN = 9


def synthetic_occupancy(shape=(24, 24)):
    """(first, last) int64 (ny, nx): a whole column occupied over [0, 100] (it walls the field in two), a block of cells over
    [100, 200], a row over [150, 400], a block held until instant 50 from the beginning of time, single cells at scattered
    instants."""
    first = np.full(shape, NEVER[0], dtype=np.int64)
    last = np.full(shape, NEVER[1], dtype=np.int64)
    first[:, WALL_COLUMN], last[:, WALL_COLUMN] = 0, 100
    first[3:9, 14:19], last[3:9, 14:19] = 100, 200
    first[16, 11:], last[16, 11:] = 150, 400
    first[18:22, 1:5], last[18:22, 1:5] = oc.INT_MIN, 50
    rng = np.random.default_rng(5)
    for _ in range(30):
        j, i, t = int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1])), int(rng.integers(0, 500))
        if i != WALL_COLUMN:
            first[j, i], last[j, i] = min(first[j, i], t), max(last[j, i], t + int(rng.integers(0, 40)))
    return first, last


# the empty window; the whole horizon; before the column stands; the column alone; the column and the block; the row;
# the block and the row; after everything but a few single cells; the column's first instant
WINDOW_SET = [(120, 120), (oc.INT_MIN, oc.INT_MAX), (-500, 0), (0, 60), (90, 140), (210, 390), (120, 160), (401, 1000), (-40, 1)]


def batch_windows(R=BATCH_R):
    """(R, 2): problem r takes window (r + r // 1024) of WINDOW_SET in turn, so r and r + 1024 never share one."""
    r = np.arange(R)
    return np.array(WINDOW_SET, dtype=np.int64)[(r + r // BLOCKS) % len(WINDOW_SET)]


def occupied_sample(seed, n=600):
    """Seeded indices of the problems the reference recomputes: half below 1024, half from 1024 on, the hand-placed ones
    and their partners in the same workgroup among them."""
    rng = np.random.default_rng(seed)
    fixed = np.concatenate([np.arange(12), np.arange(12) + BLOCKS, np.arange(12) + 100, np.arange(12) + BLOCKS + 100, [2048, BATCH_R - 1]])
    lo = rng.choice(np.setdiff1d(np.arange(BLOCKS), fixed), n // 2 - 24, replace=False)
    hi = rng.choice(np.setdiff1d(np.arange(BLOCKS, BATCH_R), fixed), n // 2 - 26, replace=False)
    return np.sort(np.concatenate([fixed, lo, hi]))


def occupied_reference(sc, starts, goals, windows, free, first, last, idx, W=BATCH_W):
    """{r: plan_ref.plan dict} for the problems ``idx`` by occupancy_ref.seeds, a window's distance fields shared."""
    out, fields = {}, {}
    for r in idx:
        ref, _ = oc.seeds(starts[r:r + 1], goals[r:r + 1], windows[r:r + 1], sc["field"], sc["cell"], free, first, last, W=W,
                          fields=fields.setdefault(tuple(int(t) for t in windows[r]), {}))
        out[int(r)] = ref[0]
    return out


# ---- travel with an occupancy over more than 1024 items ----------------------------------------------------------------------
TRAVEL_R, TRAVEL_P, TRAVEL_W = 70, 16, 4                              # 1120 (problem, goal) items: 96 workgroups take two
TRAVEL_REFERENCE_PROBLEMS = 6


def travel_problems(seed):
    """(points (70, 16, 2), windows (70, 2)): points drawn a little beyond the field box; problem r's window is entry r of
    WINDOW_SET in turn, so a workgroup's second item (64 problems on) has another one."""
    sc = batch_scene(seed)
    starts, _ = random_problems(2000 + seed, TRAVEL_R * TRAVEL_P, sc["field"], beyond=0.2)
    points = starts.reshape(TRAVEL_R, TRAVEL_P, 2)
    points[3, 5] = (np.nan, 0.0)                                     # a goal and a start no pair can use
    windows = np.array(WINDOW_SET, dtype=np.int64)[np.arange(TRAVEL_R) % len(WINDOW_SET)]
    return points, windows


def travel_sample(seed):
    """Six seeded problems for the reference: three whose items are all first items of their workgroups, three whose items
    (index r * 16 + b >= 1024: r >= 64) are second ones."""
    rng = np.random.default_rng(seed)
    return np.sort(np.concatenate([rng.choice(64, 3, replace=False), 64 + rng.choice(TRAVEL_R - 64, 3, replace=False)]))


# ---- extreme grids -------------------------------------------------------------------------------------------------------------
def _strip(vertical, circles):
    f = (0.0, -6.0, 0.25, 6.0) if vertical else (-6.0, 0.0, 6.0, 0.25)
    cs = [(c[1], c[0], c[2]) if vertical else c for c in circles]
    return dict(field=f, cell=0.25, polygons=[], circles=cs, radius=0.05, margin=0.02)


def _along(vertical, pts):
    return np.array([(p[1], p[0]) if vertical else p for p in pts], dtype=np.float64)


PASSAGE = [(1.1, 0.0, 0.04)]      # a post at the edge of the strip: every centre keeps its clearance, the strip stays open
PLUG = [(1.1, 0.1, 0.1)]          # a post in the strip: cell 28 is blocked, nothing passes
# along the strip: two points on either side of the post; the centre of cell 28 (blocked by the plug: cells 27 and 29 tie, the
# lower index wins); cell 28's lattice line; two points of one cell; points beyond both ends
STRIP_POINTS = [(-5.3, 0.1), (4.9, 0.2), (1.125, 0.125), (1.0, 0.12), (2.6, 0.13), (-7.0, 0.3), (6.5, -0.2), (2.7, 0.2)]


def extreme_cases():
    """name -> (scene, points (P, 2), expected grid shape (ny, nx)).  The problems of a case are all ordered pairs of its
    points, which is also what plan.travel plans."""
    one = dict(field=pr.FIELD, cell=12.0, polygons=[], circles=[], radius=0.5, margin=0.1)
    pts1 = np.array([(-4.0, 1.0), (3.0, -2.0), (7.0, 7.0)])
    cases = {"1x1": (one, pts1, (1, 1)),
             "1x1 blocked": (dict(one, circles=[(0.3, -0.2, 0.5)]), pts1, (1, 1))}
    for vertical, tag in ((False, "1x48"), (True, "48x1")):
        shape = (48, 1) if vertical else (1, 48)
        for name, circles in (("open", []), ("passage", PASSAGE), ("plug", PLUG)):
            cases[f"{tag} {name}"] = (_strip(vertical, circles), _along(vertical, STRIP_POINTS), shape)
    return cases


def pairs_of(n):
    return [(a, b) for a in range(n) for b in range(n) if a != b]
