"""The seeded inputs of the range-sensor tests, shared by test_range_cpu.py (which holds the reference alone to the cap on
excused readings) and test_gpu_range.py (which runs the kernel on the same inputs).  Plain NumPy: scenes are dicts of
field / polygons / circles, sensors are (n, 8) rows in the C-ABI's form."""
import numpy as np

FIELD_FT = 12.1090395251
HALF = FIELD_FT / 2
FIELD = (-HALF, -HALF, HALF, HALF)
SQUARE = np.array([[-0.75, -0.75], [0.75, -0.75], [0.75, 0.75], [-0.75, 0.75]])
# front, back, left, right: mounted 0.6 ft from the tracked point, window 0.1 .. 8 ft, incidence up to 60 degrees
SENSORS4 = np.array([[0.6, 0.0, 1.0, 0.0, 0.1, 8.0, 0.5, 0.0],
                     [-0.6, 0.0, -1.0, 0.0, 0.1, 8.0, 0.5, 0.0],
                     [0.0, 0.6, 0.0, 1.0, 0.1, 8.0, 0.5, 0.0],
                     [0.0, -0.6, 0.0, -1.0, 0.1, 8.0, 0.5, 0.0]])
RANDOM_SEEDS = (11, 12, 13, 14, 15, 16)        # six scenes x 12 routes of capacity 120 x 4 sensors
MAX_EXCUSED = 0.01                             # of a test's readings
MAX_TOUCHED = 0.10                             # of a test's routes


def random_convex(rng, n, cx, cy, radius):
    """A strictly convex n-gon: sorted angles on a rotated ellipse, counter-clockwise."""
    while True:
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        if np.min(np.diff(np.concatenate([a, a[:1] + 2 * np.pi]))) > 0.5 / n:
            break
    rx, ry, rot = radius, radius * rng.uniform(0.4, 1.0), rng.uniform(0, np.pi)
    p = np.stack([rx * np.cos(a), ry * np.sin(a)], axis=1)
    R = np.array([[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]])
    return p @ R.T + [cx, cy]


def random_scene(rng, n_poly=8, n_circle=4, verts=None, radius=(0.3, 1.2)):
    polys = [random_convex(rng, int(rng.integers(3, 9)) if verts is None else verts, *rng.uniform(-HALF + 1, HALF - 1, 2),
                           rng.uniform(*radius)) for _ in range(n_poly)]
    circles = np.array([(*rng.uniform(-HALF + 1, HALF - 1, 2), rng.uniform(0.1, 0.6)) for _ in range(n_circle)]).reshape(-1, 3)
    return {"field": FIELD, "polygons": polys, "circles": circles}


def random_rows(rng, B, cap, spread=0.05):
    """Random poses, each route a short random walk (rows of a route stay close, like real rows)."""
    rows = np.zeros((B, cap, 8))
    for b in range(B):
        p = rng.uniform(-HALF + 0.5, HALF - 0.5, 2)
        rows[b, :, 6:8] = p + np.cumsum(rng.normal(0, spread, (cap, 2)), axis=0)
        rows[b, :, 4] = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.normal(0, 0.05, cap))
        rows[b, :, 0] = np.arange(cap) * 0.01
    return rows


def random_case(seed, B=12, cap=120):
    """One of the random cases: a scene of 8 polygons + 4 circles, B random-walk routes, counts including 0, 1 and cap."""
    rng = np.random.default_rng(seed)
    scene = random_scene(rng)
    rows = random_rows(rng, B, cap)
    counts = rng.integers(2, 41, B).astype(np.int32)         # short routes: a grazing reading excuses a whole route's summary
    counts[[1, 4, 7, 9, 10, 11]] = 0, 1, cap, 63, 64, 65
    return {"scene": scene, "rows": rows, "counts": counts, "sensors": SENSORS4}


def scene_size_case(over):
    """A scene under (10 polygons of 16 vertices) or over (100 of them) the kernel's LDS budget for the packed scene."""
    rng = np.random.default_rng(21 + int(over))
    scene = random_scene(rng, 100 if over else 10, 4, verts=16, radius=(0.2, 0.5))
    rows = random_rows(rng, 60, 70)
    counts = rng.integers(1, 13, 60).astype(np.int32)        # many short routes: a dense scene excuses most long ones
    counts[[0, 13]] = 70, 65
    return {"scene": scene, "rows": rows, "counts": counts, "sensors": SENSORS4}


# ---- crafted validity patterns for the tilings --------------------------------------------------------------------------------
TILING_SENSORS = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 3.0, 0.0, 0.0],       # faces +x: valid 1 ft from the wall, FAR 5 ft from it
                           [0.0, 0.0, 0.0, 1.0, 0.0, 3.0, 0.0, 0.0]])      # faces +y likewise


def edge_pattern(n, phase):
    """ok[r] over n rows: not-ok runs that end at, begin at and straddle every multiple of 64 (so every 256 and 1024 too),
    some spanning whole waves, several of equal length (the earliest must win)."""
    ok = np.ones(n, dtype=bool)
    for e in range(64, n + 64, 64):
        kind = (e // 64 + phase) % 5
        lo, hi = {0: (e - 3, e), 1: (e, e + 3), 2: (e - 2, e + 2), 3: (e - 70, e + 70), 4: (e - 1, e + 1)}[kind]
        ok[max(lo, 0):min(hi, n)] = False
    if phase % 3 == 1:
        ok[:5] = False                     # a leading run
    if phase % 3 == 2:
        ok[max(n - 7, 0):] = False         # a trailing run
    return ok


def pattern_rows(ok_x, ok_y, cap):
    """Rows at heading 0 whose +x sensor is valid where ok_x and whose +y sensor is valid where ok_y (TILING_SENSORS)."""
    n = len(ok_x)
    rows = np.full((cap, 8), np.nan)
    rows[:, 0] = np.arange(cap) * 0.01
    rows[:n, 4] = 0.0
    rows[:n, 6] = np.where(ok_x, HALF - 1.0, HALF - 5.0)
    rows[:n, 7] = np.where(ok_y, HALF - 1.0, HALF - 5.0)
    return rows


def tiling_case(kind):
    """"long": one route of 5000 rows; "short": 1200 routes of <= 40 rows; "steps": 520 routes of capacity 1100, three of them
    long, so that a tile takes several 256-row steps and ends at row 1024."""
    rng = np.random.default_rng(31)
    if kind == "long":
        cap, ns = 5000, [5000]
    elif kind == "short":
        cap, ns = 40, [int(v) for v in rng.integers(0, 41, 1200)]
        ns[:4] = [0, 1, 40, 39]
    else:
        cap, ns = 1100, [int(v) for v in rng.integers(0, 41, 520)]
        ns[3], ns[200], ns[519] = 1100, 1025, 700
    rows = np.zeros((len(ns), cap, 8))
    oks = []
    for b, n in enumerate(ns):
        if kind == "short":
            ok_x, ok_y = rng.random(n) < 0.6, rng.random(n) < 0.5
            if b % 7 == 0:
                ok_x[:] = False
            if b % 11 == 0:
                ok_y[:] = True
        else:
            ok_x, ok_y = edge_pattern(n, b), edge_pattern(n, b + 2)
        rows[b] = pattern_rows(ok_x, ok_y, cap)
        oks.append((ok_x, ok_y))
    scene = {"field": FIELD, "polygons": [], "circles": np.zeros((0, 3))}
    return {"scene": scene, "rows": rows, "counts": np.array(ns, dtype=np.int32), "sensors": TILING_SENSORS, "ok": oks}


def partner_case():
    """Two partners with different counts and a third without rows, crossing the beams of 8 routes."""
    rng = np.random.default_rng(41)
    scene = random_scene(rng, 3, 2)
    rows = random_rows(rng, 20, 90)
    counts = rng.integers(2, 31, 20).astype(np.int32)
    counts[[0, 2, 3, 11]] = 90, 0, 1, 65
    others = random_rows(rng, 3, 60, spread=0.08)
    others[:, :, 6:8] *= 0.5                       # near the middle of the field, where the beams pass
    others_counts = np.array([[60, 0], [25, 0], [0, 0]], dtype=np.int32)
    return {"scene": scene, "rows": rows, "counts": counts, "sensors": SENSORS4, "others": others, "others_counts": others_counts,
            "others_foot": SQUARE}


def reference(rr, case, shift_rows=0, **kw):
    """range_ref.readings of a case (kw: its ftype and ambiguous)."""
    sc = case["scene"]
    return rr.readings(case["rows"], case["counts"], case["sensors"], sc["field"], sc["polygons"], sc["circles"],
                       case.get("others"), case.get("others_counts"), case.get("others_foot"), shift_rows, **kw)


# ---- random scenes away from the origin -----------------------------------------------------------------------------------------
TRANSLATIONS = (2.0 ** 10, 2.0 ** 17)          # ft, along both axes
TRANSLATED_SEEDS = RANDOM_SEEDS[:2]
TOL = 1e-12                                    # test_gpu_range.py's, the floor of the measured tolerance
_TOLERANCE = {}


def translated_case(seed, d):
    """random_case(seed) moved by (d, d): field, polygons, circles and poses, each rounded to a double once."""
    case = random_case(seed)
    sc = case["scene"]
    rows = case["rows"].copy()
    rows[:, :, 6:8] += d
    circles = sc["circles"].copy()
    circles[:, :2] += d
    scene = {"field": tuple(v + d for v in sc["field"]), "polygons": [p + d for p in sc["polygons"]], "circles": circles}
    return {**case, "scene": scene, "rows": rows}


def translation_tolerance(rr, d):
    """(D, tol, ambiguous) of the translation d: D = the largest |float64 reference - long-double reference| of a range or a
    cosine over the translated seeds, on the readings both precisions decide alike and the float64 one does not excuse;
    tol = max(TOL, 8 D), the project's convention; a reading is excused below a margin of max(1e-9, 2 tol)."""
    if d not in _TOLERANCE:
        D = 0.0
        for seed in TRANSLATED_SEEDS:
            case = translated_case(seed, d)
            r64, rld = reference(rr, case), reference(rr, case, ftype=np.longdouble)
            keep = r64["live"][:, :, None] & ~r64["excused"] & (r64["element"] != -2)
            for k in ("status", "face", "element"):
                keep &= r64[k] == rld[k]
            for k in ("t", "cos"):
                D = max(D, float(np.max(np.abs(r64[k].astype(np.longdouble) - rld[k])[keep])))
        tol = max(TOL, 8.0 * D)
        _TOLERANCE[d] = (D, tol, max(1e-9, 2.0 * tol))
    return _TOLERANCE[d]


def excused_shares(ref, summ):
    """(share of live readings excused, share of routes with a touched summary)."""
    live = ref["live"]
    n_read = int(live.sum()) * ref["status"].shape[2]
    n_exc = int(ref["excused"].sum())
    return (n_exc / n_read if n_read else 0.0), float(summ["touched"].any(axis=1).mean())
