"""Deterministic inputs that put vap_plan_occupancy and the window mask of vap_plan_seeds_occupied / vap_plan_travel
(include/vap.h) ON their decisions, shared by test_occupancy_cases_cpu.py (the NumPy reference of occupancy_ref.py alone: what
each family holds) and test_gpu_occupancy_cases.py (the kernels against that reference, as bits, nothing excused).

Why bits.  Every pose has heading 0.0, for which sin and cos are exact in every library.  Positions, footprint vertices, field,
cell, radius and margin are dyadic; edge lengths are powers of two or 1.5 ft; the corner distances that matter are dyadic
Pythagorean triples ((0.375, 0.5) -> 0.625).  A division and a sqrt round once, the same on the device and in NumPy, and the
library is built without contraction.  The CPU test asserts for every case that the float64 and the longdouble run of the
reference agree in first, last, count and blocked, and (``licensed``) that nothing before the last sqrt and the - radius
depends on the precision; min_clearance then agrees bit for bit too (D = 0) except where the minimum is an irrational corner
distance, which the longdouble run rounds twice and which is checked against the exactly rounded value in rationals.  From
that the device is held to the float64 reference with no tolerance, although clearances sit exactly on the margin (``gap`` = 0
is the point of the ties).

A case is a dict: rows (B, capacity, 8), counts (B,), foot, field, cell, radius, margin, shift_rows, hold_first, hold_last:
``reference`` runs occupancy_ref.occupancy on it.  ``FAMILIES`` maps a family's name to a function that returns its named
cases.  The ``many`` family keeps its routes as a few distinct ones and an index (``many_rows`` expands them), and its
expected values come from the reference on the distinct (route, count) pairs times their multiplicity (``many_expected``).
``windows`` returns the two occupancies, the static scene and the problems of the window family."""
import functools

import numpy as np

import occupancy_ref as oc
import plan_ref as pr
from scene_cases import FAR

INT_MIN, INT_MAX = oc.INT_MIN, oc.INT_MAX
KEYS = ("first", "last", "count")
ALL_KEYS = KEYS + ("min_clearance", "blocked")
up = lambda v: float(np.nextafter(v, np.inf))

FIELD = (-4.0, -4.0, 4.0, 4.0)
CELL, RADIUS = 0.25, 0.5
SQUARE2 = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])          # 2 ft: edges of length 2
RECT = np.array([[0.0, -0.25], [2.0, -0.25], [2.0, 0.25], [0.0, 0.25]])           # off centre: the largest |vertex| is no half diagonal
SMALL = np.array([[-0.25, -0.25], [0.25, -0.25], [0.25, 0.25], [-0.25, 0.25]])    # 0.5 ft
FEET = {"square2": SQUARE2, "square18": oc.SQUARE, "rect": RECT}
MARGINS = (0.125, 0.375, 0.0, -0.25)
# the issue's table for the 2 ft square: margin -> (pairs with clearance exactly the margin, covered pairs, blocked cells)
TIES_PINNED = {0.125: (576, 17960, 416), 0.375: (450, 23441, 480), 0.0: (2324, 14304, 352), -0.25: (2342, 9855, 288)}
CORNER_TIES_PINNED = 108                                                            # of the 576 at margin 0.125


def make_case(rows, counts=None, foot=SQUARE2, field=FIELD, cell=CELL, radius=RADIUS, margin=0.125, shift_rows=0, hold_first=False,
              hold_last=False):
    """rows: a (B, capacity, 8) array or a list of (n, 8) routes (padded with NaN rows behind their counts)."""
    if isinstance(rows, list):
        cap = max(len(r) for r in rows)
        packed = np.full((len(rows), cap, 8), np.nan)
        for b, r in enumerate(rows):
            packed[b, :len(r)] = r
        counts = [len(r) for r in rows] if counts is None else counts
        rows = packed
    return dict(rows=np.ascontiguousarray(rows, dtype=np.float64), counts=np.asarray(counts, dtype=np.int32), foot=foot, field=field,
                cell=cell, radius=radius, margin=margin, shift_rows=int(shift_rows), hold_first=bool(hold_first), hold_last=bool(hold_last))


def reference(case, ftype=np.float64):
    return oc.occupancy(case["rows"], case["counts"], case["foot"], case["field"], case["cell"], case["radius"], case["margin"],
                        case["shift_rows"], case["hold_first"], case["hold_last"], ftype)


def pair_clearance(case, ftype=np.float64):
    """(n, ny, nx): the clearance of every (row, cell) pair of a case of ONE route whose rows all take part."""
    assert len(case["rows"]) == 1
    px, py = np.meshgrid(*pr.centres(case["field"], case["cell"], ftype))
    r = case["rows"][0, :int(case["counts"][0])]
    return oc.row_clearance(oc.pose(r, case["foot"], ftype), px, py, case["radius"], ftype)


_LICENSED = {}


def licensed(case):
    """The licence to compare min_clearance as bits, for a case of ONE route.  Asserts for every (row, cell) pair of the rows that
    take part that the largest signed edge distance and, outside the footprint, the smallest squared distance are the same
    VALUES in float64 and in longdouble: nothing before the sqrt depends on the precision.  What is left is sqrt and - radius,
    one correctly rounded operation each, on the device as in NumPy.  Where the sqrt is irrational the longdouble run, rounded
    to a double afterwards, may differ in the last bit (it rounds twice); every such cell of the minimum is checked against the
    exactly rounded value in rationals instead.  Returns (cells, that number of cells)."""
    from fractions import Fraction as Fr

    from range_exact_cases import fl, sqrt_rounded
    n = int(min(max(int(case["counts"][0]), 0), case["rows"].shape[1]))
    key = (case["rows"][0, :n].tobytes(), case["foot"].tobytes(), case["field"], case["cell"], case["radius"])
    if key in _LICENSED:
        return _LICENSED[key]
    r = case["rows"][0, :n]
    r = r[oc.taking_part(r, case["foot"])]
    ncell, twice = 0, 0
    if len(r):
        parts = {}
        for ftype in (np.float64, np.longdouble):
            px, py = np.meshgrid(*pr.centres(case["field"], case["cell"], ftype))
            parts[ftype] = oc.row_parts(oc.pose(r, case["foot"], ftype), px, py, ftype)
        (s64, d64), (sl, dl) = parts[np.float64], parts[np.longdouble]
        out = s64 > 0
        assert np.array_equal(s64.astype(np.longdouble), sl) and np.array_equal(d64[out].astype(np.longdouble), dl[out])
        rad = case["radius"]
        c64 = np.where(out, np.sqrt(d64), s64) - rad
        cl = (np.where(out, np.sqrt(dl), sl) - np.longdouble(rad)).min(axis=0).astype(np.float64)
        k = c64.argmin(axis=0)
        m64 = c64.min(axis=0)
        ncell = m64.size
        for j, i in np.argwhere(m64 != cl):
            assert out[k[j, i], j, i]
            want = fl(Fr(sqrt_rounded(Fr(float(d64[k[j, i], j, i])))) - Fr(rad))
            assert want == m64[j, i], (j, i, want, m64[j, i])
            twice += 1
    _LICENSED[key] = (ncell, twice)
    return _LICENSED[key]


def same(a, b, keys=ALL_KEYS, zero_sign=True):
    """The first key in which two output dicts differ (integers equal, doubles the same bits), or None.  zero_sign False: -0.0
    and +0.0 are one value.  A clearance of zero is the largest of several signed edge distances of which more than one can be a
    zero, of either sign (a centre on a vertex); IEEE 754 leaves the sign of max(-0, +0) open, NumPy returns either, the device's
    maximum +0, and the header says 'the largest s', for which the two zeros are one number."""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            return k
        if x.dtype.kind == "f" or y.dtype.kind == "f":
            x, y = (np.ascontiguousarray(v, dtype=np.float64) + (0.0 if not zero_sign else -0.0) for v in (x, y))
            x, y = x.view(np.int64), y.view(np.int64)
        if not np.array_equal(x, y):
            return k
    return None


def merged(parts):
    """B routes in one call: the elementwise min / max / sum / min of the single calls."""
    out = {"first": np.minimum.reduce([p["first"] for p in parts]), "last": np.maximum.reduce([p["last"] for p in parts]),
           "count": sum(p["count"] for p in parts)}
    if all("min_clearance" in p for p in parts):
        out["min_clearance"] = np.minimum.reduce([p["min_clearance"] for p in parts])
    out["blocked"] = out["first"] <= out["last"]
    return out


# ---- 1. ties ------------------------------------------------------------------------------------------------------------------
def tie_rows(dx=0.0, dy=0.0):
    """130 rows at x = -3 + r / 16, y = 0.125, heading 0: the cell centres are odd multiples of 1/8, so every offset of a
    centre from a row is a multiple of 1/16 in x and of 1/4 in y."""
    n = 130
    return oc.make_rows(-3.0 + np.arange(n) / 16.0 + dx, np.full(n, 0.125 + dy), np.zeros(n))


def ties_family():
    cases = {}
    for fname, foot in FEET.items():
        for m in MARGINS:
            cases[f"ties {fname} {m:g}"] = make_case([tie_rows()], foot=foot, margin=m, hold_first=True, hold_last=True)
            cases[f"ties {fname} {m:g} above"] = make_case([tie_rows()], foot=foot, margin=up(m), hold_first=True, hold_last=True)
        cases[f"ties {fname} -4"] = make_case([tie_rows()], foot=foot, margin=-4.0, hold_first=True, hold_last=True)     # reach < 0
    # one row of the 2 ft square at (0.125, 0.125): the centre (1.125, 0.125) lies on its edge, (1.125, 1.125) on its vertex and
    # (0.125, 0.125) deep inside (the signed-distance branch: -1).  Margin = that clearance, and the double above it
    one = oc.make_rows([0.125], [0.125], [0.0])
    for name, radius, m in (("on the edge", 0.0, 0.0), ("on the edge, disc", 0.5, -0.5), ("deep inside", 0.5, -1.5)):
        cases[f"ties {name}"] = make_case([one], radius=radius, margin=m, hold_last=True)
        cases[f"ties {name} above"] = make_case([one], radius=radius, margin=up(m), hold_last=True)
    return cases


FEATURE_CELLS = {"edge": (16, 20), "vertex": (20, 20), "inside": (16, 16)}          # (j, i) of the three centres above


def tie_counts(case):
    """(ties, covered, corner ties) over the (row, cell) pairs of a one-route case; a corner tie is a tie at a centre outside
    the footprint's x range AND its y range (the nearest point is a vertex: the clearance came through the sqrt of two squares)."""
    c = pair_clearance(case)
    tie = c == case["margin"]
    px, py = np.meshgrid(*pr.centres(case["field"], case["cell"]))
    r = case["rows"][0, :len(c)]
    fx, fy = case["foot"][:, 0], case["foot"][:, 1]
    ox = (px[None] < (r[:, 6] + fx.min())[:, None, None]) | (px[None] > (r[:, 6] + fx.max())[:, None, None])
    oy = (py[None] < (r[:, 7] + fy.min())[:, None, None]) | (py[None] > (r[:, 7] + fy.max())[:, None, None])
    return int(tie.sum()), int((c < case["margin"]).sum()), int((tie & ox & oy).sum())


# ---- 2. chunks ----------------------------------------------------------------------------------------------------------------
CHUNK_CAP = 192
CHUNK_COUNTS = (1, 63, 64, 65, 127, 128, 129, 192, 0, -3, 192 + 500)
HOLDS = ((False, False), (True, False), (False, True), (True, True))


def chunk_rows():
    """(11, 192, 8): route b at y = -2.875 + b / 2, x = -3.5 + r / 32.  Every row of the capacity is a real pose, so a row read
    behind its count would show."""
    r = np.arange(CHUNK_CAP)
    return np.stack([oc.make_rows(-3.5 + r / 32.0, np.full(CHUNK_CAP, -2.875 + 0.5 * b), np.zeros(CHUNK_CAP)) for b in range(len(CHUNK_COUNTS))])


def chunks_family():
    rows, cases = chunk_rows(), {}
    for hf, hl in HOLDS:
        tag = f"hold {int(hf)}{int(hl)}"
        cases[f"chunks all {tag}"] = make_case(rows, CHUNK_COUNTS, hold_first=hf, hold_last=hl, shift_rows=-7)
        for b, n in enumerate(CHUNK_COUNTS):
            cases[f"chunks n={n} {tag}"] = make_case(rows[b:b + 1], [n], hold_first=hf, hold_last=hl, shift_rows=-7)
    return cases


# ---- 3. instants --------------------------------------------------------------------------------------------------------------
INSTANT_CAP = 130
SHIFT_LOW, SHIFT_HIGH = INT_MIN + 1, INT_MAX - INSTANT_CAP - 1                       # the accepted extremes
SHIFT_REFUSED = (INT_MIN, INT_MAX - INSTANT_CAP)


def instants_family():
    cases = {}
    for name, shift in (("low", SHIFT_LOW), ("high", SHIFT_HIGH)):
        for hf, hl in ((True, True), (False, False)):
            cases[f"instants {name} hold {int(hf)}{int(hl)}"] = make_case([tie_rows()], shift_rows=shift, hold_first=hf, hold_last=hl)
    return cases


# ---- 4. non-finite and collapsed poses --------------------------------------------------------------------------------------------
BAD_N = 150
BAD_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
BAD_COLUMNS = {"heading": 4, "x": 6, "y": 7}
BAD_PLACES = {"row 0": [0], "last row": [BAD_N - 1], "chunk 1": list(range(64, 128)), "route": list(range(BAD_N))}
COLLAPSED = (2.0 ** 60, -2.0 ** 60, 1e300, -1e300)


def bad_base():
    r = np.arange(BAD_N)
    return oc.make_rows(-3.5 + r / 32.0, np.full(BAD_N, 0.125), np.zeros(BAD_N))


def nonfinite_family():
    """The base route, and the base route with some rows' poses spoilt: ``spoilt`` lists them.  Holds on: a spoilt row 0 (last
    row) must hold nothing, and the hold must not pass to its neighbour."""
    cases = {"bad base": dict(make_case([bad_base()], hold_first=True, hold_last=True), spoilt=[])}
    for vname, v in BAD_VALUES.items():
        for cname, col in BAD_COLUMNS.items():
            for pname, where in BAD_PLACES.items():
                rows = bad_base()
                rows[where, col] = v
                cases[f"bad {vname} {cname} {pname}"] = dict(make_case([rows], hold_first=True, hold_last=True), spoilt=where)
    return cases


def collapsed_family():
    """Finite poses so large that the posed vertices fall onto one point, or onto one line: an edge of squared length 0."""
    cases = {}
    everything = bad_base()
    spots = iter(range(3, BAD_N, 11))
    for v in COLLAPSED:
        for axes in ((6,), (7,), (6, 7)):
            rows = bad_base()
            rows[70, list(axes)] = v
            cases[f"collapsed {v:g} {'xy'[axes[0] - 6] if len(axes) == 1 else 'both'}"] = dict(make_case([rows], hold_first=True, hold_last=True), spoilt=[70])
            everything[next(spots), list(axes)] = v
    cases["collapsed twelve"] = dict(make_case([everything], hold_first=True, hold_last=True), spoilt=list(range(3, BAD_N, 11))[:12])
    for place, where in (("row 0", [0]), ("last row", [BAD_N - 1])):
        rows = bad_base()
        rows[where, 6] = 1e300
        cases[f"collapsed 1e300 x {place}"] = dict(make_case([rows], hold_first=True, hold_last=True), spoilt=where)
    return cases


def by_segments(case):
    """What the header asks of a route with spoilt rows, without the reference's own rule: every run [a, b) of good rows as a
    route of its own at shift + a, the first hold only on a run that starts at row 0, the last only on one that ends at row n."""
    rows, n = case["rows"][0], int(case["counts"][0])
    good = np.ones(n, dtype=bool)
    good[case["spoilt"]] = False
    parts = [reference(dict(case, rows=rows[None, :0], counts=np.array([0], dtype=np.int32)))]            # no rows: the never-covered values
    a = 0
    while a < n:
        if not good[a]:
            a += 1
            continue
        b = a
        while b < n and good[b]:
            b += 1
        parts.append(reference(dict(case, rows=rows[a:b][None], counts=np.array([b - a], dtype=np.int32), shift_rows=case["shift_rows"] + a,
                                    hold_first=case["hold_first"] and a == 0, hold_last=case["hold_last"] and b == n)))
        a = b
    return merged(parts)


# ---- 5. far -------------------------------------------------------------------------------------------------------------------
def far_family():
    """The ties of the 2 ft square with field and rows alike moved by (X, X)."""
    cases = {}
    for X in FAR:
        field = tuple(v + X for v in FIELD)
        for m in (0.125, up(0.125)):
            cases[f"far {X:g} {'above' if m != 0.125 else 'at'}"] = make_case([tie_rows(X, X)], field=field, margin=m, hold_first=True, hold_last=True)
    return cases


def far_base(name):
    return family("ties")["ties square2 0.125 above" if name.endswith("above") else "ties square2 0.125"]


# ---- 6. many ------------------------------------------------------------------------------------------------------------------
MANY_FIELD = (-1.0, -1.0, 1.0, 1.0)
MAX_BLOCKS = 1 << 16                                                                  # the kernel's cap on workgroups


def many_family():
    """More work items (64-row chunks) than the kernel starts workgroups.  The routes behind work item 65 536 are distinct ones
    that no earlier route equals, so a grid-stride loop that stops early shows.
      ones   66 000 routes of capacity 1; count 0 on every third, 1 or 5 (clamped) on the others
      pairs  33 000 routes of capacity 65 and count 65: two chunks each, the second is row 64 alone (the held last row)"""
    B1 = 66000
    pts = [(-0.875 + 0.25 * (k % 4), -0.625 + 0.5 * (k // 4)) for k in range(8)] + [(0.5625, 0.8125), (-1.375, 0.0), (0.9375, -0.9375), (0.0, 1.5)]
    distinct = np.stack([oc.make_rows([x], [y], [0.0]) for x, y in pts])              # (12, 1, 8)
    b = np.arange(B1)
    index = np.where(b < MAX_BLOCKS, b % 8, 8 + b % 4)
    counts = np.where(b % 3 == 0, 0, np.where(b % 5 == 0, 5, 1))
    ones = dict(make_case(distinct[:1], [1], foot=SMALL, field=MANY_FIELD, radius=0.125, margin=0.125, hold_first=True, hold_last=True, shift_rows=11),
                distinct=distinct, index=index, counts=counts.astype(np.int32), rows=None)
    B2, cap = 33000, 65
    r = np.arange(cap)
    routes = [oc.make_rows(-1.5 + r / 32.0 + 0.125 * k, np.full(cap, -0.875 + 0.25 * k), np.zeros(cap)) for k in range(6)]
    routes += [oc.make_rows(np.full(cap, 0.8125), -1.25 + r / 32.0, np.zeros(cap)), oc.make_rows(1.0 - r / 32.0, np.full(cap, 0.9375), np.zeros(cap))]
    b = np.arange(B2)
    index = np.where(2 * b < MAX_BLOCKS, b % 6, 6 + b % 2)
    pairs = dict(make_case(np.stack(routes)[:1], [cap], foot=SMALL, field=MANY_FIELD, radius=0.125, margin=0.125, hold_last=True),
                 distinct=np.stack(routes), index=index, counts=np.full(B2, cap, dtype=np.int32), rows=None)
    return {"many ones": ones, "many pairs": pairs}


def many_rows(case):
    return np.ascontiguousarray(case["distinct"][case["index"]])


def many_expected(case):
    """The reference on every distinct (route, clamped count) alone, the counts times the multiplicity."""
    cap = case["distinct"].shape[1]
    n = np.clip(case["counts"].astype(np.int64), 0, cap)
    key, mult = np.unique(case["index"].astype(np.int64) * (cap + 1) + n, return_counts=True)
    parts = []
    for k, m in zip(key, mult):
        p = reference(dict(case, rows=case["distinct"][k // (cap + 1)][None], counts=np.array([k % (cap + 1)], dtype=np.int32)))
        parts.append(dict(p, count=p["count"] * int(m)))
    return merged(parts)


# ---- 7. minimum ---------------------------------------------------------------------------------------------------------------
def minimum_family():
    """One route of 2 560 rows, 40 chunks: 16 passes over a 16 x 16 grid (field +-2) in steps of 1/8 ft from x = -10 to x = 10 and
    back, a quarter of a foot further north each pass: most chunks lie wholly outside the field, up to 8 ft off it, so the box of
    a chunk is weighed against the cells' running minimum."""
    k = np.arange(160)
    xs = np.concatenate([(-10.0 + k / 8.0) if p % 2 == 0 else (10.0 - k / 8.0) for p in range(16)])
    ys = np.repeat(-1.875 + 0.25 * np.arange(16), 160)
    rows = oc.make_rows(xs, ys, np.zeros(len(xs)))
    return {"minimum": make_case([rows], foot=SMALL, field=(-2.0, -2.0, 2.0, 2.0), radius=0.125, margin=0.125, hold_last=True)}


# ---- 8. windows ---------------------------------------------------------------------------------------------------------------
# the seeds' own disc and margin: no cell of the box is tied, and the cells the route leaves last (x = 3.625) are free of the wall
WINDOW_SCENE = dict(field=FIELD, polygons=[], circles=[], radius=0.25, margin=0.1, cell=CELL)
WINDOW_W = 5
WINDOW_CELL = (16, 16)                                                                # (j, i): the centre (0.125, 0.125)
ENDS = (((-3.25, -3.25), (3.25, 3.25)), ((3.25, -3.25), (-3.25, 3.25)), ((0.1, -3.3), (0.1, 3.3)), ((-3.3, 0.1), (3.3, 0.1)))


@functools.lru_cache(maxsize=None)
def windows():
    """The ties' route at margin 0.125 without holds (``plain``) and with both (``held``), and the problems: a list of (name,
    which occupancy, (t0, t1)); ``pairs`` lists neighbouring windows (name a, name b, what separates them)."""
    plain = make_case([tie_rows()])
    held = make_case([tie_rows()], hold_first=True, hold_last=True)
    ref = reference(plain)
    f, l = int(ref["first"][WINDOW_CELL]), int(ref["last"][WINDOW_CELL])
    assert 0 < f < l < 129
    w = [("before 0", "plain", (-5, 0)), ("to 0", "plain", (-5, 1)), ("from 129", "plain", (129, 200)), ("from 130", "plain", (130, 200)),
         ("up to f", "plain", (0, f)), ("up to f + 1", "plain", (0, f + 1)), ("at f", "plain", (f, f + 1)), ("from l", "plain", (l, 200)),
         ("from l + 1", "plain", (l + 1, 200)), ("at l", "plain", (l, l + 1)), ("empty 60", "plain", (60, 60)), ("empty 61", "plain", (61, 60)),
         ("lowest plain", "plain", (INT_MIN, INT_MIN + 1)), ("highest plain", "plain", (INT_MAX - 1, INT_MAX)),
         ("lowest held", "held", (INT_MIN, INT_MIN + 1)), ("highest held", "held", (INT_MAX - 1, INT_MAX))]
    pairs = [("before 0", "to 0", ("first", 0)), ("from 130", "from 129", ("last", 129)), ("up to f", "up to f + 1", ("first", f)),
             ("from l + 1", "from l", ("last", l)), ("lowest plain", "lowest held", ("first", INT_MIN)),
             ("highest plain", "highest held", ("last", INT_MAX))]
    problems = [dict(name=name, occ=which, window=win, start=ENDS[k % 4][0], goal=ENDS[k % 4][1]) for k, (name, which, win) in enumerate(w)]
    # two edge windows for vap_plan_travel, each with the neighbour that a wrong comparison would turn it into: the legs run
    # through the cells row 0 covers (first = 0), and up the column x = 3.625 that the route leaves last (last = 129)
    travel = [dict(window=(-5, 0), neighbour=(-5, 1), points=[(-3.25, -3.25), (-3.25, 3.25), (3.25, 0.1)]),
              dict(window=(129, 200), neighbour=(130, 200), points=[(3.625, -3.25), (3.625, 3.25), (-3.25, 0.1)])]
    return dict(plain=plain, held=held, f=f, l=l, problems=problems, pairs=pairs, travel=travel)


def static_free():
    sc = WINDOW_SCENE
    return pr.clearance_grid(sc["field"], sc["cell"], radius=sc["radius"]) >= sc["margin"]


FAMILIES = {"ties": ties_family, "chunks": chunks_family, "instants": instants_family, "nonfinite": nonfinite_family,
            "collapsed": collapsed_family, "far": far_family, "many": many_family, "minimum": minimum_family}


@functools.lru_cache(maxsize=None)
def family(name):
    """The named cases of a family, built once."""
    return FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def cached_reference(fam, name, long=False):
    return reference(family(fam)[name], np.longdouble if long else np.float64)
