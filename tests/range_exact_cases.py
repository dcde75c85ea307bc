"""Deterministic inputs that put the ray cast of vap_range_readings (include/vap.h, "reading" and "status") ON its decisions, and
an exact checker of those rules, shared by test_range_exact_cpu.py (the reference against the checker) and
test_gpu_range_exact.py (the kernel against the reference, nothing excused).

Every case has heading exactly 0.0, beams (+-1, 0) and (0, +-1), and coordinates, mounts and radii that are small dyadic
numbers.  Then cos phi = 1, sin phi = -0, and every product and sum of the header's formulas is exact in fp64 (the checker
asserts it), so contracting a product and a sum into one FMA cannot change a bit.  What rounds: the one division of a
candidate's t, the sqrt of a circle and the subtraction after it, the unit normal of an edge (hypot, two divisions, on the
host), and the circle's cosine (one sum, one difference, one division).  Each is a single correctly rounded operation on exact
operands, so reference and kernel must agree bit for bit on range and cosine and exactly on status, face and element.

One case leaves the cardinal beams: a tie between the x and the y wall needs a beam with two non-zero components.
``corner_case`` casts (q, q), q = fl(sqrt(1/2)), from points at equal distances from both walls of a scene without obstacles:
tx and ty are the same division, bit for bit.

A case is range_cases' dict: scene (field, polygons, circles), rows (B, cap, 8), counts, sensors (n, 8), optionally others,
others_counts, others_foot.  ``FAMILIES`` maps a family's name to a function that returns its named cases.

The checker (``exact_readings``) is independent of range_ref.py: it restates the header in fractions.Fraction, one ray at a
time.  A quotient is rounded once (float(Fraction) is correctly rounded), a circle's t is fl(-b -+ fl(sqrt(disc))) with disc
asserted to be a double, and every float intermediate is asserted to equal its rational value.  Its rules can be switched to
their neighbours (``RULES``) to show that a family notices."""
import collections
import functools
import math
from fractions import Fraction as Fr

import numpy as np

FIELD = (-6.0, -6.0, 6.0, 6.0)
CARDINAL = ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0))


# ---- building blocks ----------------------------------------------------------------------------------------------------------
def square(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])


def diamond(cx, cy, h):
    return np.array([[cx + h, cy], [cx, cy + h], [cx - h, cy], [cx, cy - h]])


def octagon(cx, cy, u):
    return np.array([[u, -2 * u], [2 * u, -u], [2 * u, u], [u, 2 * u], [-u, 2 * u], [-2 * u, u], [-2 * u, -u], [-u, -2 * u]]) + [cx, cy]


def gon16(cx, cy, unit):
    """A strictly convex 16-gon on a lattice of ``unit``: four edge directions a quadrant, (3,1) (2,1) (1,1) (1,2) and their
    quarter turns; centred on (cx, cy)."""
    e = [(3, 1), (2, 1), (1, 1), (1, 2)]
    for _ in range(3):
        e += [(-y, x) for x, y in e[-4:]]
    v = np.cumsum(np.array([(0, 0)] + e[:-1], dtype=np.float64), axis=0)
    v -= (v.min(axis=0) + v.max(axis=0)) / 2
    return v * unit + [cx, cy]


def sensors_of(*rows):
    """(mx, my, ux, uy, r_min, r_max, min_cos) rows as the C-ABI's (n, 8)."""
    return np.array([list(r) + [0.0] for r in rows], dtype=np.float64)


def cardinal_sensors(r_min=0.0, r_max=64.0, min_cos=0.0, mount=0.0):
    return sensors_of(*[(mount * ux, mount * uy, ux, uy, r_min, r_max, min_cos) for ux, uy in CARDINAL])


def make_case(scene, routes, sensors, cap=None, others=None, others_foot=None):
    """routes: a list of (n, 2) pose arrays, one per route (heading 0).  Rows past a route's count hold NaN poses.  others: a
    list of (n_o, 2) partner poses."""
    cap = max([len(r) for r in routes] + [1]) if cap is None else cap
    rows = np.full((len(routes), cap, 8), np.nan)
    rows[:, :, 0] = np.arange(cap) * 0.01
    rows[:, :, 1:4] = 0.0
    rows[:, :, 5] = 0.0
    for b, r in enumerate(routes):
        r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
        rows[b, :len(r), 4] = 0.0
        rows[b, :len(r), 6:8] = r
    case = {"scene": scene, "rows": rows, "counts": np.array([len(r) for r in routes], dtype=np.int32),
            "sensors": np.asarray(sensors, dtype=np.float64)}
    if others is not None:
        cap_o = max(len(o) for o in others)
        orows = np.zeros((len(others), cap_o, 8))
        orows[:, :, 0] = np.arange(cap_o) * 0.01
        for o, p in enumerate(others):
            orows[o, :len(p), 6:8] = p
        case.update(others=orows, others_counts=np.array([len(o) for o in others], dtype=np.int32),
                    others_foot=np.asarray(others_foot, dtype=np.float64))
    return case


def scene_of(polygons=(), circles=(), field=FIELD):
    return {"field": field, "polygons": [np.asarray(p, dtype=np.float64) for p in polygons],
            "circles": np.asarray(circles, dtype=np.float64).reshape(-1, 3)}


# ---- lattice --------------------------------------------------------------------------------------------------------------------
LATTICE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 300)
LATTICE_SENSORS = sensors_of((0.5, 0.0, 1.0, 0.0, 0.25, 8.0, 0.5), (-0.5, 0.125, -1.0, 0.0, 0.0, 4.0, 0.0),
                             (0.0, 0.375, 0.0, 1.0, 1.0, 6.0, 1.0), (-0.0, -0.5, 0.0, -1.0, 0.5, 3.5, 0.5))


def lattice_scene():
    """Squares, diamonds and an octagon on multiples of 1/4 ft, circles of radius 5/8."""
    return scene_of([square(1.0, 1.0, 2.0, 2.0), square(-3.0, -0.5, -2.0, 0.5), square(-1.25, 3.0, 0.25, 4.5), diamond(3.0, -2.0, 1.0),
                     diamond(-3.5, -3.5, 0.75), octagon(0.0, -3.5, 0.5)],
                    [(3.5, 3.5, 0.625), (-4.0, 2.5, 0.625), (0.0, 0.5, 0.625), (4.5, 0.0, 0.625)])


def lattice_poses(rng, n, pool=None):
    """Poses on multiples of 1/8 ft inside the field (mounts reach 1/2 ft)."""
    if pool is not None:
        return pool[rng.integers(0, len(pool), n)]
    return rng.integers(-44, 45, (n, 2)) / 8.0


def lattice_case(counts=LATTICE_COUNTS, seed=101):
    rng = np.random.default_rng(seed)
    return make_case(lattice_scene(), [lattice_poses(rng, n) for n in counts], LATTICE_SENSORS, cap=max(counts))


def lattice_family():
    return {"lattice": lattice_case()}


# ---- ties -----------------------------------------------------------------------------------------------------------------------
BODY = square(-0.75, -0.75, 0.75, 0.75)


def ties_scene_case():
    """Twin polygons, a polygon face against a circle at the same t, a circle touching the wall, an obstacle face on the wall."""
    twin = square(2.0, -1.0, 3.0, 1.0)
    scene = scene_of([twin, twin.copy(), square(5.0, 2.0, 6.0, 3.0), square(-1.0, 5.0, 1.0, 6.0)],
                     [(2.625, 0.0, 0.625),          # touches the twins' face x = 2 at y = 0
                      (5.375, -3.0, 0.625),         # touches the wall x = 6 at y = -3
                      (-3.0, -5.375, 0.625)])       # touches the wall y = -6 at x = -3
    routes = [
        # twins (element 0), the circle behind their face (the polygon stays), rays that miss the circle's tangent point
        [(0.0, 0.0), (0.0, 0.5), (0.0, -1.0), (0.0, 1.0), (2.5, -3.0), (2.5, 3.0), (4.0, 0.0), (2.625, 0.0), (2.5, 0.0)],
        # inside the circles that touch a wall: the way out is on the wall (the wall stays); and from outside them
        [(5.5, -3.0), (5.375, -3.0), (5.0, -3.0), (-3.0, -5.5), (-3.0, -5.375), (-3.0, -5.0), (4.0, -3.0), (-3.0, -4.0)],
        # inside the squares whose face lies on a wall, on that face, and along it
        [(5.5, 2.5), (5.25, 2.0), (6.0, 2.5), (6.0, 0.0), (6.0, 4.0), (0.0, 5.5), (0.5, 6.0), (-2.0, 6.0), (1.0, 5.5), (5.0, 2.5)],
    ]
    return make_case(scene, routes, cardinal_sensors(r_max=16.0))


def ties_partner_case():
    """A partner that coincides with polygon 0 at some rows (the polygon stays: not blocked), stands strictly nearer at others
    (status 5), and a second partner behind the polygon."""
    scene = scene_of([square(2.25, -0.75, 3.75, 0.75)], [(0.0, -3.0, 0.625)])
    n = 12
    near = [(3.0, 0.0)] * 4 + [(1.5, 0.0)] * 4 + [(3.0, 0.5)] * 2 + [(0.0, 3.0)] * 2
    behind = [(4.5, 0.0)] * n
    routes = [[(0.0, 0.0)] * n, [(0.0, 0.75)] * n, [(3.0, 2.0)] * n, [(-2.0, -0.75)] * 5]
    return make_case(scene, routes, cardinal_sensors(r_max=16.0), others=[near, behind], others_foot=BODY)


def ties_twin_partners_case():
    """16 partners at one pose: the first partner's element."""
    scene = scene_of([square(-4.0, -4.0, -3.0, -3.0)], [(4.0, 4.0, 0.625)])
    others = [[(3.0, 0.0), (0.0, 3.0), (0.0, 3.0)]] * 16
    routes = [[(0.0, 0.0)] * 3, [(3.0, -3.0), (1.0, 3.0)], [(0.0, 0.75), (0.0, -0.75), (3.75, 0.0)]]
    return make_case(scene, routes, cardinal_sensors(r_max=16.0), others=others, others_foot=BODY)


def ties_family():
    return {"ties scene": ties_scene_case(), "ties partner": ties_partner_case(), "ties 16 partners": ties_twin_partners_case()}


# ---- vertices -------------------------------------------------------------------------------------------------------------------
def vertices_family():
    g = gon16(2.0, 2.0, 0.125)
    sliver = np.array([[-2.0, -4.0], [2.0, -4.0], [0.0, -4.0 + 1.0 / 64]])
    thin = np.array([[-4.0, 1.0], [-4.0 + 1.0 / 32, 1.0], [-4.0 + 1.0 / 32, 4.0], [-4.0, 4.0]])
    scene = scene_of([diamond(3.0, -2.0, 1.0), square(-3.0, -1.0, -2.0, 1.0), g, sliver, thin,
                      np.array([[-1.0, -1.0], [0.5, -1.5], [1.0, 0.0], [0.0, 1.0]])])
    # beams through every vertex of every polygon: a pose on the vertex's row, one on its column (the four beams of each)
    routes = []
    for p in scene["polygons"]:
        r = []
        for vx, vy in p:
            r += [(-5.5, vy), (vx, -5.5), (5.5, vy), (vx, 5.5)]
        routes.append(r)
    # along the lines of the axis-parallel edges, from both ends and from inside the edge
    routes.append([(-5.0, -1.0), (-5.0, 1.0), (-3.0, -5.0), (-2.0, -5.0), (-2.5, 1.0), (-2.0, 0.0), (-5.0, -4.0), (5.0, -4.0), (0.5, -4.0),
                   (-4.0, -5.0), (-4.0 + 1.0 / 32, 5.0), (-4.0, 2.0)])
    return {"vertices": make_case(scene, routes, cardinal_sensors(r_max=16.0))}


# ---- origins --------------------------------------------------------------------------------------------------------------------
def corner_case():
    """The one case off the cardinal beams: (q, q), q = fl(sqrt(1/2)), and its three quarter turns, from points as far from
    the x wall as from the y wall; no obstacles.  tx and ty are the same quotient."""
    q = math.sqrt(0.5)
    sens = sensors_of(*[(0.0, 0.0, sx * q, sy * q, 0.0, 64.0, 0.0) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))])
    d = [0.0, 0.125, 1.0, 2.5, 5.875, 6.0]
    routes = [[(6.0 - a, 6.0 - a) for a in d] + [(-6.0 + a, 6.0 - a) for a in d],
              [(-6.0 + a, -6.0 + a) for a in d] + [(6.0 - a, -6.0 + a) for a in d] + [(1.0, 0.0), (0.0, -2.0)]]
    return make_case(scene_of(), routes, sens)


def origins_family():
    scene = scene_of([square(1.0, 1.0, 3.0, 3.0), diamond(-3.0, 2.0, 1.0), square(8.0, -1.0, 9.0, 1.0)],
                     [(-2.0, -3.0, 0.625), (3.0, -3.0, 1.25), (0.0, 9.0, 0.625)])
    walls = [(6.0, 0.0), (-6.0, 0.5), (0.25, 6.0), (-0.25, -6.0), (6.0, 6.0), (-6.0, 6.0), (-6.0, -6.0), (6.0, -6.0)]
    outside = [(7.0, 0.0), (6.125, 0.0), (10.0, 0.5), (0.0, 7.0), (0.0, 11.0), (-7.0, -7.0), (8.5, 0.0), (7.0, 4.0), (-7.0, 2.0),
               (6.0 + 2.0 ** -20, 0.0)]
    inside = [(2.0, 2.0), (1.5, 2.75), (-3.0, 2.0), (-3.5, 2.25), (-2.0, -3.0), (-2.25, -2.75), (3.0, -3.0), (3.75, -2.0)]
    on = [(1.0, 2.0), (3.0, 1.5), (2.0, 1.0), (2.5, 3.0), (1.0, 1.0), (3.0, 3.0), (-2.5, 2.5), (-4.0, 2.0), (-3.0, 3.0),
          (-1.375, -3.0), (-2.625, -3.0), (-2.0, -2.375), (-2.0, -3.625), (3.0, -1.75), (4.0, -2.25), (2.0, -3.75)]
    plus = make_case(scene, [walls, outside, inside, on], cardinal_sensors(r_max=16.0))
    # the same poses through mounts of -0.0 and +0.0, and mounts that put the origin on the wall from a pose beside it
    zero = sensors_of((-0.0, 0.0, 1.0, 0.0, 0.0, 16.0, 0.0), (0.0, -0.0, -1.0, 0.0, 0.0, 16.0, 0.0), (-0.0, -0.0, 0.0, 1.0, 0.0, 16.0, 0.0),
                      (0.5, 0.0, 1.0, 0.0, 0.0, 16.0, 0.0), (0.0, -0.25, 0.0, -1.0, 0.0, 16.0, 0.0), (-0.5, 0.25, -1.0, 0.0, 0.0, 16.0, 0.0))
    mounted = make_case(scene, [walls + on, [(5.5, 0.0), (5.5, 5.75), (-5.5, -5.75), (0.0, -5.75), (0.5, 2.0), (3.5, 1.75), (-2.5, -3.0)]], zero)
    return {"origins": plus, "origins mounted": mounted, "origins corner": corner_case()}


# ---- tangent --------------------------------------------------------------------------------------------------------------------
def tangent_family():
    """Circles of radius 5 * 2^-k: offsets of 5 * 2^-k are tangent (disc = 0), offsets of 3 * 2^-k and 4 * 2^-k give sqrt(disc)
    = 4 * 2^-k and 3 * 2^-k exactly."""
    ks = (2, 3, 4, 5)
    centres = [(-3.0, -3.0), (3.0, -3.0), (3.0, 3.0), (-3.0, 3.0)]
    circles = [(cx, cy, 5.0 * 2.0 ** -k) for (cx, cy), k in zip(centres, ks)]
    routes = []
    for (cx, cy, r), k in zip(circles, ks):
        u = 2.0 ** -k
        offs = [m * u for m in (-6, -5, -4, -3, 0, 3, 4, 5, 6)]
        routes.append([(0.0, cy + o) for o in offs] + [(cx + o, 0.0) for o in offs] + [(cx + o, cy) for o in offs] + [(cx, cy + o) for o in offs])
    return {"tangent": make_case(scene_of([], circles), routes, cardinal_sensors(r_max=16.0))}


# ---- thresholds -----------------------------------------------------------------------------------------------------------------
def thresholds_family():
    """Readings of known t and cosine, written down here and not taken from any code under test:
      pose (0, 0): +x reads the wall at t = 6, cos 1; -y reads the 3-4-5 edge of polygon 0 at t = 2, cos = fl(4 / 5);
                   +y reads polygon 1's slanted edge at t = fl(7 / 3), cos = fl(3 / fl(sqrt(10)));
      pose (0.5, 0): +x reads 5.5.
    Each sensor puts one threshold on the reading, or one ulp to either side of it (np.nextafter on the threshold)."""
    tri = np.array([[-1.5, -4.0], [2.5, -4.0], [2.5, -1.0]])             # edge 2: from (2.5, -1) along (-4, -3), n = (-3, 4) / 5;
    # it passes x = 0 at y = -1 - 3 * 2.5 / 4 = -2.875: -y reads t = 2.875, cos = |ny| = fl(4 / 5)
    slant = np.array([[-1.0, 2.0], [2.0, 3.0], [-1.0, 3.0]])             # edge 0: e = (3, 1): at x = 0 y = 2 + 1 / 3, t = fl(7 / 3)
    scene = scene_of([tri, slant])
    up, dn = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    t_wall, t_edge, t_third = 6.0, 2.875, 7.0 / 3.0
    c_edge = 4.0 / 5.0
    c_third = 3.0 / math.sqrt(10.0)

    def around(beam, t, c):
        ux, uy = beam
        return [(0.0, 0.0, ux, uy, r_min, r_max, mc) for r_min, r_max, mc in (
            (t, 64.0, 0.0), (up(t), 64.0, 0.0), (dn(t), 64.0, 0.0),          # t == r_min is valid, above it NEAR
            (0.0, t, 0.0), (0.0, up(t), 0.0), (0.0, dn(t), 0.0),             # t == r_max is valid, below it FAR
            (t, t, 0.0), (0.0, 64.0, c))]                                    # the window a single point; cos == min_cos

    def around_cos(beam, c):
        ux, uy = beam
        return [(0.0, 0.0, ux, uy, 0.0, 64.0, mc) for mc in (c, up(c), dn(c))] if c < 1.0 else \
               [(0.0, 0.0, ux, uy, 0.0, 64.0, mc) for mc in (c, dn(c))]
    routes = [[(0.0, 0.0), (0.5, 0.0), (0.0, 0.0)]]
    cases = {"thresholds wall": make_case(scene, routes, sensors_of(*around((1.0, 0.0), t_wall, 1.0))),
             "thresholds edge": make_case(scene, routes, sensors_of(*around((0.0, -1.0), t_edge, c_edge))),
             "thresholds third": make_case(scene, routes, sensors_of(*around((0.0, 1.0), t_third, c_third))),
             "thresholds cos": make_case(scene, routes, sensors_of(*(around_cos((1.0, 0.0), 1.0) + around_cos((0.0, -1.0), c_edge) +
                                                                     around_cos((0.0, 1.0), c_third))))}
    return cases


# ---- wide -----------------------------------------------------------------------------------------------------------------------
WIDE_B, WIDE_CAP = 1024, 300
PAD_POLYGONS = 16


def wide_counts():
    rng = np.random.default_rng(103)
    counts = rng.integers(0, 13, WIDE_B)
    counts[np.arange(40) * 25 + 3] = np.tile([255, 256, 257, 300], 10)
    return counts


def wide_case(padded=False):
    """The lattice scene under 1024 routes of capacity 300: B * tiles4 >= 1024 selects the four-step tile.  Poses come from a
    pool of 256 lattice poses.  padded: 16 far-away 16-gons behind the scene's own polygons take the packed scene past the LDS
    budget; they are never hit (every pose is inside the field), and the circles' element indices move up by 16."""
    rng = np.random.default_rng(104)
    pool = lattice_poses(rng, 256)
    scene = lattice_scene()
    if padded:
        scene["polygons"] = scene["polygons"] + [gon16(100.0 + 4.0 * (i % 4), 100.0 + 4.0 * (i // 4), 0.125) for i in range(PAD_POLYGONS)]
    return make_case(scene, [lattice_poses(rng, n, pool) for n in wide_counts()], LATTICE_SENSORS, cap=WIDE_CAP)


def packed_doubles(scene):
    return sum(4 + 8 * len(p) for p in scene["polygons"]) + 4 * len(scene["circles"])


def wide_family():
    return {"wide": wide_case(False), "wide padded": wide_case(True)}


# ---- moved ----------------------------------------------------------------------------------------------------------------------
TRANSLATIONS = (2.0 ** 10, 2.0 ** 17, 2.0 ** 23)
SCALES = (2.0 ** -10, 2.0 ** 10)
MOVED_LATTICE_COUNTS = (0, 1, 63, 64, 65, 257)


def translated(case, d):
    """The case moved by (d, d), field, partners and all."""
    sc = case["scene"]
    out = dict(case)
    out["scene"] = {"field": tuple(v + d for v in sc["field"]), "polygons": [p + d for p in sc["polygons"]],
                    "circles": sc["circles"] + [d, d, 0.0] if len(sc["circles"]) else sc["circles"]}
    out["rows"] = case["rows"].copy()
    out["rows"][:, :, 6:8] += d
    if "others" in case:
        out["others"] = case["others"].copy()
        out["others"][:, :, 6:8] += d
    return out


def scaled(case, f):
    """The case scaled by f about the origin: scene, poses, mounts, windows and the partners' footprint."""
    sc = case["scene"]
    out = dict(case)
    out["scene"] = {"field": tuple(v * f for v in sc["field"]), "polygons": [p * f for p in sc["polygons"]], "circles": sc["circles"] * f}
    out["rows"] = case["rows"].copy()
    out["rows"][:, :, 6:8] *= f
    out["sensors"] = case["sensors"].copy()
    out["sensors"][:, [0, 1, 4, 5]] *= f
    if "others" in case:
        out["others"] = case["others"].copy()
        out["others"][:, :, 6:8] *= f
        out["others_foot"] = case["others_foot"] * f
    return out


def moved_bases():
    bases = {"lattice": lattice_case(MOVED_LATTICE_COUNTS, seed=105)}
    bases.update(ties_family())
    return bases


def moved_variants():
    """(base name, kind, amount, case) of every moved case."""
    for name, base in moved_bases().items():
        for d in TRANSLATIONS:
            yield name, "translated", d, translated(base, d)
        for f in SCALES:
            yield name, "scaled", f, scaled(base, f)


def moved_family():
    cases = {f"moved {name} base": c for name, c in moved_bases().items()}
    cases.update({f"moved {name} {kind} {amount:g}": c for name, kind, amount, c in moved_variants()})
    return cases


FAMILIES = {"lattice": lattice_family, "ties": ties_family, "vertices": vertices_family, "origins": origins_family,
            "tangent": tangent_family, "thresholds": thresholds_family, "wide": wide_family, "moved": moved_family}


@functools.lru_cache(maxsize=None)
def family(name):
    """The named cases of a family, built once."""
    return FAMILIES[name]()


# ---- the exact checker ----------------------------------------------------------------------------------------------------------
# The header's rules and their neighbours.  True is the header's side.
RULES = {"w_inclusive": True,            # 0 <= w <= 1 (False: 0 < w < 1)
         "t_inclusive": True,            # t >= 0 (False: t > 0)
         "den_zero_skips": True,         # den = 0: no candidate (never switched: the quotient does not exist)
         "first_wins_edges": True,       # an edge replaces the best only on a strictly smaller t (False: on a tie too)
         "first_wins_circles": True,     # the same for a circle
         "wall_tie_x": True,             # tx == ty: the x side (False: the y side)
         "box_inclusive": True,          # the origin on the box counts as inside
         "disc_inclusive": True,         # disc >= 0 (False: disc > 0)
         "near_strict": True,            # t < r_min is NEAR (False: t <= r_min)
         "far_strict": True,             # t > r_max is FAR (False: t >= r_max)
         "oblique_strict": True}         # cos < min_cos is OBLIQUE (False: cos <= min_cos)
VALID, NONE, NEAR, FAR, OBLIQUE, BLOCKED, BAD_POSE = range(7)


def fl(q):
    """The double nearest to a rational (ties to even): the one rounding of a division or a sum."""
    return q.numerator / q.denominator


def sqrt_rounded(q):
    """The correctly rounded sqrt of a rational that is a double, checked against the squares of its neighbours' midpoints."""
    f = fl(q)
    assert Fr(f) == q, ("sqrt of a value that is no double", q)
    s = math.sqrt(f)
    if s > 0.0:
        lo, hi = (Fr(s) + Fr(math.nextafter(s, 0.0))) / 2, (Fr(s) + Fr(math.nextafter(s, math.inf))) / 2
        assert lo * lo <= q <= hi * hi, (q, s)
    return s


class Checker:
    """The header's reading of one case, one ray at a time, in exact arithmetic."""

    def __init__(self, case, shift_rows=0, check_exact=True, **rules):
        assert set(rules) <= set(RULES), rules
        self.rule = dict(RULES, **rules)
        self.check = check_exact
        self.case = case
        self.shift = int(shift_rows)
        sc = case["scene"]
        self.field = None if sc["field"] is None else tuple(float(v) for v in sc["field"])
        self.polygons = [self._edges([(float(x), float(y)) for x, y in p]) for p in sc["polygons"]]
        self.circles = [tuple(float(v) for v in c) for c in np.asarray(sc["circles"], dtype=np.float64).reshape(-1, 3)]
        self.n_scene = len(self.polygons) + len(self.circles)
        self.memo = {}
        self.flags = collections.Counter()

    # every float intermediate the families rely on equals its rational value
    def ex(self, f, q, what):
        if self.check:
            assert Fr(f) == q, (what, f, q)
        return q

    def _edges(self, verts):
        """[(ax, ay, ex, ey, nx, ny)] of a polygon's edges in order: a and e as doubles (e exact), n the unit normal as the host
        packs it, fl(ey / len), fl(-ex / len) with len = fl(hypot)."""
        out = []
        m = len(verts)
        for j in range(m):
            (ax, ay), (bx, by) = verts[j], verts[(j + 1) % m]
            ex, ey = bx - ax, by - ay
            self.ex(ex, Fr(bx) - Fr(ax), "edge x")
            self.ex(ey, Fr(by) - Fr(ay), "edge y")
            length = sqrt_rounded(Fr(ex) * Fr(ex) + Fr(ey) * Fr(ey))
            out.append((ax, ay, ex, ey, fl(Fr(ey) / Fr(length)), fl(Fr(-ex) / Fr(length))))
        return out

    def offer(self, best, t, cos, face, el, kind, first_wins):
        """best = (t, cos, face, el, kind) or None; returns the new best.  Records ties."""
        if best is None:
            return (t, cos, face, el, kind)
        if t == best[0]:
            self.tie_flags.add("tie " + (f"{best[4]} edges" if best[3] == el else f"{best[4]} > {kind}"))
        if t < best[0] or (not first_wins and t == best[0]):
            return (t, cos, face, el, kind)
        return best

    def wall(self, ox, oy, ux, uy):
        if self.field is None:
            return None
        xmin, ymin, xmax, ymax = self.field
        r = self.rule
        on_box = (ox in (xmin, xmax) and ymin <= oy <= ymax) or (oy in (ymin, ymax) and xmin <= ox <= xmax)
        inside = xmin <= ox <= xmax and ymin <= oy <= ymax
        if on_box:
            self.tie_flags.add("origin on the box")
        if not inside or (on_box and not r["box_inclusive"]):
            return None
        tx = ty = math.inf
        fx, fy = 0, 1
        if ux != 0.0:
            wall_x = xmax if ux > 0.0 else xmin
            tx, fx = fl(self.ex(wall_x - ox, Fr(wall_x) - Fr(ox), "wall x") / Fr(ux)), (2 if ux > 0.0 else 0)
        if uy != 0.0:
            wall_y = ymax if uy > 0.0 else ymin
            ty, fy = fl(self.ex(wall_y - oy, Fr(wall_y) - Fr(oy), "wall y") / Fr(uy)), (3 if uy > 0.0 else 1)
        if tx == ty:
            self.tie_flags.add("tie wall corner")
        y_side = ty < tx or (not r["wall_tie_x"] and ty == tx)
        if y_side:
            return (ty, abs(uy), fy, -1, "wall")
        return (tx, abs(ux), fx, -1, "wall")

    def edge(self, best, e, ox, oy, ux, uy, face, el, kind):
        ax, ay, ex, ey, nx, ny = e
        r = self.rule
        Ox, Oy, Ux, Uy, Ax, Ay, Ex, Ey = (Fr(v) for v in (ox, oy, ux, uy, ax, ay, ex, ey))
        den = self.ex(ux * ey - uy * ex, Ux * Ey - Uy * Ex, "den")
        dx, dy = ax - ox, ay - oy
        Dx, Dy = self.ex(dx, Ax - Ox, "dx"), self.ex(dy, Ay - Oy, "dy")
        wn = self.ex(dx * uy - dy * ux, Dx * Uy - Dy * Ux, "wn")
        if den == 0:
            if wn == 0:
                self.tie_flags.add("beam along an edge's line")
            return best
        w = wn / den
        if not (0 <= w <= 1 if r["w_inclusive"] else 0 < w < 1):
            return best
        tn = self.ex(dx * ey - dy * ex, Dx * Ey - Dy * Ex, "tn")
        tq = tn / den
        if not (tq >= 0 if r["t_inclusive"] else tq > 0):
            return best
        if w == 0 or w == 1:
            self.tie_flags.add("hit on a vertex")
        if tq == 0:
            self.tie_flags.add("origin on an edge")
        cos = abs(fl(self.ex(ux * nx + uy * ny, Ux * Fr(nx) + Uy * Fr(ny), "u . n")))
        return self.offer(best, fl(tq), cos, face, el, kind, r["first_wins_edges"])

    def circle(self, best, c, ox, oy, ux, uy, el):
        cx, cy, rad = c
        r = self.rule
        Ox, Oy, Ux, Uy, Cx, Cy, R = (Fr(v) for v in (ox, oy, ux, uy, cx, cy, rad))
        dx, dy = ox - cx, oy - cy
        Dx, Dy = self.ex(dx, Ox - Cx, "circle dx"), self.ex(dy, Oy - Cy, "circle dy")
        b_f, q_f = dx * ux + dy * uy, (dx * dx + dy * dy) - rad * rad
        b = self.ex(b_f, Dx * Ux + Dy * Uy, "b")
        q = self.ex(q_f, (Dx * Dx + Dy * Dy) - R * R, "q")
        disc = self.ex(b_f * b_f - q_f, b * b - q, "disc")
        if disc < 0 or (disc == 0 and not r["disc_inclusive"]):
            return best
        if disc == 0:
            self.tie_flags.add("tangent circle")
        if q == 0:
            self.tie_flags.add("origin on a circle")
        sq = Fr(sqrt_rounded(disc))
        t = fl(-b - sq)
        if t < 0.0:
            t = fl(-b + sq)
        if not t >= 0.0:
            return best
        # cos_inc = |u . (o + t u - centre)| / r, operation by operation: t u is exact, the sum and the difference round
        T = Fr(t)
        tux, tuy = self.ex(t * ux, T * Ux, "t ux"), self.ex(t * uy, T * Uy, "t uy")
        px, py = fl(Fr(fl(Ox + tux)) - Cx), fl(Fr(fl(Oy + tuy)) - Cy)
        dot = self.ex(ux * px + uy * py, Ux * Fr(px) + Uy * Fr(py), "u . (hit - centre)")
        cos = fl(abs(dot) / R)
        return self.offer(best, t, cos, 0, el, "circle", r["first_wins_circles"])

    def ray(self, ox, oy, ux, uy, partners):
        """(t, cos, face, element, flags) or None-filled: the header's candidates 1-4 in order."""
        key = (ox, oy, ux, uy, partners)
        if key in self.memo:
            return self.memo[key]
        self.tie_flags = set()
        best = self.wall(ox, oy, ux, uy)
        for k, edges in enumerate(self.polygons):
            # wn of an edge is its first vertex's side of the beam's line: with every vertex strictly on one side no edge has a
            # w in [0, 1] (an exact shortcut, it changes no result)
            side = [(Fr(e[0]) - Fr(ox)) * Fr(uy) - (Fr(e[1]) - Fr(oy)) * Fr(ux) for e in edges]
            if all(v > 0 for v in side) or all(v < 0 for v in side):
                continue
            for j, e in enumerate(edges):
                best = self.edge(best, e, ox, oy, ux, uy, j, k, "polygon")
        for k, c in enumerate(self.circles):
            best = self.circle(best, c, ox, oy, ux, uy, len(self.polygons) + k)
        for o, verts in partners:
            for j, e in enumerate(self._edges(list(verts))):
                best = self.edge(best, e, ox, oy, ux, uy, j, self.n_scene + o, "partner")
        out = (best, frozenset(self.tie_flags))
        self.memo[key] = out
        return out

    def partners_at(self, r):
        """((o, posed vertices)) of the partners at row r: heading 0, so a vertex is p + v, exactly."""
        case = self.case
        if "others" not in case:
            return ()
        out = []
        oc = np.asarray(case["others_counts"]).reshape(len(case["others"]), -1)[:, 0]
        for o in range(len(case["others"])):
            n_o = int(min(max(oc[o], 0), case["others"].shape[1]))
            if n_o == 0:
                continue
            ro = min(max(r - self.shift, 0), n_o - 1)
            h, px, py = (float(case["others"][o, ro, c]) for c in (4, 6, 7))
            assert h == 0.0
            verts = []
            for vx, vy in case["others_foot"]:
                x, y = px + float(vx), py + float(vy)
                self.ex(x, Fr(px) + Fr(float(vx)), "partner vertex x")
                self.ex(y, Fr(py) + Fr(float(vy)), "partner vertex y")
                verts.append((x, y))
            out.append((o, tuple(verts)))
        return tuple(out)

    def reading(self, x, y, sensor, partners):
        """(status, face, element, t, cos) of one sensor at the pose (heading 0, x, y)."""
        mx, my, bx, by, r_min, r_max, min_cos = (float(v) for v in sensor[:7])
        c, s = 1.0, -0.0                                         # cos and sin of phi = -0.0
        ox, oy = x + (c * mx - s * my), y + (s * mx + c * my)
        ux, uy = c * bx - s * by, s * bx + c * by
        self.ex(ox, Fr(x) + Fr(mx), "origin x")
        self.ex(oy, Fr(y) + Fr(my), "origin y")
        self.ex(ux, Fr(bx), "beam x")
        self.ex(uy, Fr(by), "beam y")
        best, flags = self.ray(ox, oy, ux, uy, partners)
        self.flags.update(flags)
        if best is None:
            return NONE, 0, -2, math.nan, math.nan
        t, cos, face, el, _ = best
        r = self.rule
        if el >= self.n_scene:
            status = BLOCKED
        else:
            for name, hit in (("t == r_min", t == r_min), ("t == r_max", t == r_max), ("cos == min_cos", cos == min_cos)):
                if hit:
                    self.flags[name] += 1
            if t < r_min or (not r["near_strict"] and t == r_min):
                status = NEAR
            elif t > r_max or (not r["far_strict"] and t == r_max):
                status = FAR
            elif cos < min_cos or (not r["oblique_strict"] and cos == min_cos):
                status = OBLIQUE
            else:
                status = VALID
        return status, face, el, t, cos


def exact_readings(case, shift_rows=0, check_exact=True, **rules):
    """The header's readings of a case, in range_ref.readings' layout: status, face, element, t, cos as (B, cap, ns) arrays
    (-1 / -1 / -2 / NaN / NaN past the counts), and ``flags``, a Counter of the decisions met (once per reading)."""
    ck = Checker(case, shift_rows, check_exact, **rules)
    rows, sens = case["rows"], np.asarray(case["sensors"], dtype=np.float64).reshape(-1, 8)
    B, cap = rows.shape[:2]
    ns = len(sens)
    counts = np.clip(np.asarray(case["counts"]).reshape(B, -1)[:, 0], 0, cap)
    out = {"status": np.full((B, cap, ns), -1, dtype=np.int64), "face": np.full((B, cap, ns), -1, dtype=np.int64),
           "element": np.full((B, cap, ns), -2, dtype=np.int64), "t": np.full((B, cap, ns), np.nan), "cos": np.full((B, cap, ns), np.nan)}
    for b in range(B):
        for r in range(int(counts[b])):
            h, x, y = (float(rows[b, r, c]) for c in (4, 6, 7))
            assert h == 0.0 and math.isfinite(x) and math.isfinite(y)
            partners = ck.partners_at(r)
            for s in range(ns):
                st, fa, el, t, cos = ck.reading(x, y, sens[s], partners)
                out["status"][b, r, s], out["face"][b, r, s], out["element"][b, r, s] = st, fa, el
                out["t"][b, r, s], out["cos"][b, r, s] = t, cos
    out["flags"] = ck.flags
    return out


def same_readings(a, b, keys=("status", "face", "element", "t", "cos"), zero_sign=True):
    """The first difference between two readings dicts (bit for bit on t and cos, every NaN one NaN), or None.  zero_sign False:
    -0.0 and +0.0 are one value (the header leaves the sign of a zero open; the checker's quotients have none)."""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            x, y = x.astype(np.float64), y.astype(np.float64)
            if not zero_sign:
                x, y = x + 0.0, y + 0.0
            nx, ny = np.isnan(x), np.isnan(y)
            x, y = np.where(nx, -1, x.view(np.int64)), np.where(ny, -1, y.view(np.int64))
        bad = np.argwhere(x != y)
        if len(bad):
            i = tuple(bad[0])
            return k, i, a[k][i], b[k][i], len(bad)
    return None


# ---- moved: the identities ---------------------------------------------------------------------------------------------------
def cos_moves_with_the_frame(base_case, ref, d):
    """The readings whose cosine is NOT a translation invariant: a circle's cos_inc is taken at the hit point o + t u, in the
    frame's own coordinates, and that sum is exact after a move by d only when t is a multiple of ulp(d)."""
    n_poly, n_circ = len(base_case["scene"]["polygons"]), len(base_case["scene"]["circles"])
    circle = (ref["element"] >= n_poly) & (ref["element"] < n_poly + n_circ)
    step = np.spacing(d)
    with np.errstate(invalid="ignore"):
        return circle & (np.nan_to_num(ref["t"]) % step != 0.0)


def check_moved(base_case, base, kind, amount, moved, what):
    """Translation: range, cosine and code bit for bit.  Scaling by a power of two: codes and cosines, and the ranges times it."""
    keys = ("status", "face", "element")
    assert same_readings(base, moved, keys) is None, (what, same_readings(base, moved, keys))
    if kind == "scaled":
        assert same_readings(dict(base, t=base["t"] * amount), moved, ("t", "cos")) is None, what
        return 0
    assert same_readings(base, moved, ("t",)) is None, what
    loose = cos_moves_with_the_frame(base_case, base, amount)
    cos = np.where(loose, base["cos"], moved["cos"])
    assert same_readings(base, dict(moved, cos=cos), ("cos",)) is None, what
    # there the hit point moves by at most half an ulp of 2 d, and the cosine by that over the radius (5/8 ft and more)
    assert (np.abs(base["cos"] - moved["cos"])[loose] <= 2 * np.spacing(2 * amount) / 0.625).all(), what
    return int(loose.sum())
