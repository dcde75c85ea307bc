"""Deterministic inputs that put the follower rollouts (include/vap.h: vap_tracking_rollouts, vap_pursuit_rollouts,
vap_odometry_rollouts, vap_rollout_clearance) ON their decisions, and an exact checker of those rules, shared by
test_rollout_exact_cpu.py (the NumPy references against the checker) and test_gpu_rollout_exact.py (the kernels against the
references, nothing excused).

A compiler may contract a * b + c into an FMA and NumPy does not.  The library is built with -ffp-contract=off today, but the
families do not lean on that flag: kernel and reference are held to the same bits only where every product that feeds a sum
is exact.  Two kinds of route give that:

  stationary   every row has the same pose, heading 0.0 and v = omega = 0: RAMSETE's k is 0 and (with min_speed 0) pure
               pursuit's speed is 0, so the robot never moves whatever its start offset; the errors are the offsets themselves.
               A heading offset is combined only with dx = dy = 0 (cos and sin of it then multiply zeros), a lateral offset
               only with this kind of route.
  on-axis      points along +x at heading 0.0, dy = dphi = 0, tau = 0; time_step = 1/16, two substeps; the gains, the track
               scale, b = 16, zeta = 0.5, v = 2 and so k = 2 zeta sqrt(b) v = 8 are powers of two.  Then sin phi = 0, cos phi = 1,
               omega = 0 and sinc(0) = 1 throughout, and every product has a power of two as one factor.

One of (e_x, e_y) is always zero, so hypot and sqrt(dx^2 + dy^2) return |e| and nothing is claimed about a device library's
hypot.  What rounds, once each and the same in both: the wrap's a + pi, the + 2 pi after a negative fmod and the - pi after it
(fmod itself is exact); a quotient (the scale wheel_speed_max / m, pure pursuit's t, f and kappa); a sqrt (always of a perfect
square here); and, in the cases marked ``strict`` False, a sum (an offset of 1/4 halved over more rows than a double has bits,
a robot moving at the double below 2 ft/s).

Three decisions are reached by these inputs but cannot be seen in any output, so RULES has no switch for them and no test
guards them: the strict < of the lookahead advance (a target exactly on a vertex is f = 1 on segment il or f = 0 on il + 1, or
on a zero-length segment: the same point), the >= of ``s* >= c_(n-1)`` (on the tie both branches give P_(n-1)) and the tie of
max(v_t, min_speed) (both sides are the same number).

The sinc branch switch at |x| = 1e-4 is left out: the two branches differ by x^4 / 120 there, 1e-18, below half an ulp of 1.

A case is a dict: kind ("ramsete", "pursuit", "odometry"), rows (B, cap, 8), counts (B,), f (the reference's follower dict), P
(B, K, 8), dt, strict; for odometry O (B, K, 8), sensors ((ns, 8) or None), field, rule (odometry_ref.rule plus gate_in and
max_incidence_deg for odometry.ResetRule); with ``clear`` (foot, field, polygons, margin) the call is vap_rollout_clearance.
``FAMILIES`` maps a family's name to a function that returns its named cases.

``reference`` runs the NumPy references (tracking_ref, pursuit_ref, odometry_ref, footprint_ref) rollout by rollout and the
summaries route by route.  ``exact`` is independent of them: it restates the header's steps for one-dimensional motion in
fractions.Fraction (class Exact), asserts that every product is a double, rounds once at each operation named above, asserts
(strict) that every other intermediate equals its rational value, and replaces each library call by its exact value on these
inputs (cos 0 = 1, sin 0 = 0, sinc 0 = 1, exp(-inf) = 0, hypot(a, 0) = |a|).  A rational has no signed zero, so the checker is
compared with -0.0 == +0.0; the kernel is held to the reference's sign.  Its rules can be switched to their neighbours
(``RULES``) to show that a family notices."""
import functools
import math
from fractions import Fraction as Fr

import numpy as np

import footprint_ref as fr
import odometry_ref as orf
import pursuit_ref as pr
import rollout_clearance_ref as rcr
import tracking_ref as tr
from range_exact_cases import fl, sqrt_rounded

PI = math.pi
TWO_PI = 2.0 * math.pi
DT = 1.0 / 16
V = 2.0
STEP = V * DT                         # 1/8 ft a row
NOMINAL, IDEAL = tr.NOMINAL, orf.IDEAL
up = lambda v: float(np.nextafter(v, np.inf))
dn = lambda v: float(np.nextafter(v, -np.inf))


# ---- building blocks ----------------------------------------------------------------------------------------------------------
def follower(kind, **kw):
    """Powers of two throughout; pure pursuit: lookahead 1/2, arrive_tolerance 1/8, min_speed 1/4 (0 on a stationary route)."""
    if kind == "pursuit":
        f = dict(track_width=1.0, lookahead=0.5, min_speed=0.25, arrive_tolerance=0.125, wheel_speed_max=8.0, tolerance=0.25,
                 n_substeps=2, settle_rows=3)
    else:
        f = dict(track_width=1.0, b=16.0, zeta=0.5, wheel_speed_max=8.0, tolerance=0.25, n_substeps=2, settle_rows=3)
    f.update(kw)
    return f


def still_route(n, x=1.0, y=0.5):
    rows = np.zeros((n, 8))
    rows[:, 0] = np.arange(n) * DT
    rows[:, 6], rows[:, 7] = x, y
    return rows


def axis_route(xs, v=V):
    xs = np.asarray(xs, dtype=np.float64)
    rows = np.zeros((len(xs), 8))
    rows[:, 0] = np.arange(len(xs)) * DT
    rows[:, 2] = v
    rows[:, 6] = xs
    rows[:, 1] = np.abs(np.diff(xs, prepend=xs[0])).cumsum()
    return rows


def records(*items, base=NOMINAL):
    """A record per item: {slot: value} over the base record."""
    out = np.tile(np.asarray(base, dtype=np.float64), (len(items), 1))
    for k, it in enumerate(items):
        for slot, v in it.items():
            out[k, slot] = v
    return out


def offsets(values, slot=0):
    return records(*[{slot: v} for v in values])


def make_case(kind, routes, f, P, strict=True, O=None, sensors=None, field=None, rule=None, clear=None, counts=None):
    """routes: a list of (n, 8) rows; P (K, 8) for every route or (B, K, 8)."""
    cap = max(len(r) for r in routes)
    rows = np.full((len(routes), cap, 8), np.nan)
    for b, r in enumerate(routes):
        rows[b, :len(r)] = r
    B = len(routes)
    P = np.asarray(P, dtype=np.float64)
    P = np.broadcast_to(P, (B,) + P.shape[-2:]).copy()
    case = dict(kind=kind, rows=rows, counts=np.array([len(r) for r in routes] if counts is None else counts, dtype=np.int32), f=f, P=P,
                dt=DT, strict=strict, clear=clear)
    if kind == "odometry":
        O = np.asarray(IDEAL if O is None else O, dtype=np.float64)
        case.update(O=np.broadcast_to(O, P.shape).copy(), sensors=None if sensors is None else np.asarray(sensors, dtype=np.float64),
                    field=field, rule=rule)
    return case


def three(name, routes, P, strict=True, kinds=("ramsete", "odometry", "pursuit"), still=True, **fkw):
    """The same routes and records under every follower."""
    out = {}
    for kind in kinds:
        kw = dict(fkw)
        if kind == "pursuit":
            kw.pop("b", None), kw.pop("zeta", None)
            if still:
                kw.setdefault("min_speed", 0.0)
        out[f"{name} {kind}"] = make_case(kind, routes, follower(kind, **kw), P, strict=strict)
    return out


# ---- wrap ---------------------------------------------------------------------------------------------------------------------
WRAP_DPHI = (PI, up(PI), dn(PI), -PI, up(-PI), dn(-PI), 3 * PI, -3 * PI, 2 * PI, 0.0, -0.0, 1e6, -1e6, 5.5, -7.25)


def wrap_family():
    return three("wrap", [still_route(5)], offsets(WRAP_DPHI, slot=2))


# ---- first stays --------------------------------------------------------------------------------------------------------------
def tied(K, at, low=0.25, high=0.5):
    v = np.full(K, low)
    v[list(at)] = high
    return offsets(v)


EPS = 2.0 ** -53
MEAN_SMALL = {5: (1, 2, 3, 4), 256: (100, 101, 200, 201), 300: (254, 255, 256, 257)}      # where dx = 2^-53; k = 0 has dx = 1, the rest 0


def mean_records(K, small):
    v = np.zeros(K)
    v[0], v[list(small)] = 1.0, EPS
    return offsets(v)


def first_family():
    route = [still_route(5)]
    cases = three("first K5", route, offsets((0.25, 0.5, 0.5, 0.25, 0.5)))
    cases.update(three("first K5 below", route, offsets((0.25, 0.5, 0.5, 0.25, 0.5)), tolerance=dn(0.25)))
    # 85 routes of three rollouts a workgroup, and two more: even routes K identical records, odd ones (1/4, 1/2, 1/2)
    P = np.stack([tied(3, ()) if b % 2 == 0 else tied(3, (1, 2)) for b in range(87)])
    cases.update(three("first K3 B87", [still_route(5)] * 87, P))
    cases.update(three("first K256", [still_route(5)] * 2, np.stack([tied(256, ()), tied(256, (200, 255))])))
    cases.update(three("first K257", route, tied(257, (255, 256))))
    cases.update(three("first K300", [still_route(5)] * 2, np.stack([tied(300, (255, 256)), tied(300, (256, 299))])))
    # the mean is the ascending-k sum: 1 + 2^-53 is 1 (a tie, to even) however often it is added, 2^-53 + 2^-53 first is not lost
    origin = [still_route(5, 0.0, 0.5)]
    for K, small in MEAN_SMALL.items():
        cases.update(three(f"first mean K{K}", origin, mean_records(K, small)))
    return cases


# ---- thresholds of the drive ---------------------------------------------------------------------------------------------------
def drive_family():
    xs = np.arange(6) * STEP
    cases = {}
    for kind in ("ramsete", "odometry", "pursuit"):
        own = kind == "pursuit"
        for name, route, wmax, strict in (("at", xs, V, True), ("below", xs if own else xs[:2], dn(V), False), ("half", xs if own else xs[:1], V / 2, True)):
            # RAMSETE falls behind once it is saturated, and k e_x then makes a command whose product with the scale is no double:
            # at half the speed from row 1 on (one row there), at the double below from row 2 on (two rows; at row 1 the command
            # 2 + 2^-53 still rounds to 2).  Pure pursuit's command does not look at e_x: six rows
            cases[f"drive {name} {kind}"] = make_case(kind, [axis_route(route)], follower(kind, wheel_speed_max=wmax), records({}), strict=strict)
    cases["drive min_speed pursuit"] = make_case("pursuit", [axis_route(xs)], follower("pursuit", min_speed=V), records({}))
    return cases


# ---- contraction across tiles --------------------------------------------------------------------------------------------------
TILE_ROWS = (1, 2, 63, 64, 65, 129)
CONTRACT_OFFSETS = (0.25, -0.25, 0.5, -0.5)


def contraction_family():
    """K = 64: four routes a workgroup in tiles of 64 rows.  An offset halves every row under RAMSETE (k dt = 1/2)."""
    routes = [axis_route(np.arange(n) * STEP) for n in TILE_ROWS]
    P = offsets(np.tile(CONTRACT_OFFSETS, 16))
    cases = {}
    for settle in (0, 10):
        cases.update(three(f"contraction settle {settle}", routes, P, strict=False, still=False, settle_rows=settle))
    return cases


# ---- record validity -----------------------------------------------------------------------------------------------------------
TINY = 5e-324


def validity_records(positive, nonneg, base):
    """The lattice over a record: every slot NaN, +inf, -inf; the positive slots at 0.0, -0.0, -1, 5e-324; the slots that may be
    zero at -0.0, 5e-324, -5e-324; a base record between every two and an offset one at both ends."""
    items = [{0: 0.25}]
    for slot in range(8):
        items += [{slot: v} for v in (math.nan, math.inf, -math.inf)]
    for slot in positive:
        items += [{slot: v} for v in (0.0, -0.0, -1.0, TINY)]
    for slot in nonneg:
        items += [{slot: v} for v in (-0.0, TINY, -TINY)]
    out = []
    for it in items:
        out += [it, {}]
    return records(*out, base=base)


def validity_family():
    route = [still_route(4)]
    P = np.concatenate([validity_records((3, 4, 5), (6,), NOMINAL), records({7: -1.0}, {7: TINY}, {0: 0.5})])
    cases = three("validity", route, P)
    O = validity_records((0, 1, 2, 4), (), IDEAL)
    cases["validity odometry records"] = make_case("odometry", route, follower("odometry"), np.tile(records({0: 0.25}), (len(O), 1)), O=O)
    return cases


# ---- pure pursuit's pointers ---------------------------------------------------------------------------------------------------
def pointers_family():
    line = np.arange(9) * STEP
    mid = np.concatenate([line[:3], [line[2]] * 3, line[3:]])
    end = np.concatenate([line, [line[-1]] * 3])
    cases = {}
    for name, xs, kw in (("vertices", line, {}), ("arrive below", line, dict(arrive_tolerance=dn(0.125))), ("repeats mid", mid, {}),
                         ("repeats end", end, {}), ("n1", line[:1], {}), ("n2", line[:2], {}), ("still", None, dict(min_speed=0.0))):
        route = still_route(4) if xs is None else axis_route(xs)
        cases[f"pointers {name}"] = make_case("pursuit", [route], follower("pursuit", **kw), offsets((0.0, STEP, 2 * STEP, -STEP)))
    return cases


# ---- odometry's gate -----------------------------------------------------------------------------------------------------------
GATE_FIELD = (-6.0, -6.0, 6.0, 6.0)


def reset_rule(gate, min_cos_deg=0.0, gain=1.0, every=1):
    """odometry_ref.rule with the inches odometry.ResetRule turns into exactly ``gate`` feet."""
    r = orf.rule(gate, 1.0 if min_cos_deg == 0.0 else 0.0, gain, every)
    g = 12.0 * gate
    for cand in (g, up(g), dn(g), up(up(g)), dn(dn(g))):
        if cand / 12.0 == gate:
            r.update(gate_in=cand, max_incidence_deg=min_cos_deg)
            return r
    raise AssertionError(("no inches for the gate", gate))


def gate_family():
    """A stationary route of 7 rows and 5 settle rows at (2, 1), one sensor looking along +x at the wall x = 6: the true robot
    reads 4 - dx, the estimate expects 4, |z - expected| = |dx|.  The rule's min_cos is 1.0: the wall is perpendicular."""
    route = [still_route(7, 2.0, 1.0)]
    P = offsets((0.25, -0.5, 0.0, -0.25))
    f = follower("odometry", settle_rows=5)
    open_ = [[0.0, 0.0, 1.0, 0.0, 0.0, 64.0, 1.0, 0.0]]
    window = [[0.0, 0.0, 1.0, 0.0, 3.75, 3.75, 1.0, 0.0]]          # r_min = r_max = the reading of dx = 1/4
    mk = lambda sens, rule: make_case("odometry", route, f, P, sensors=sens, field=GATE_FIELD, rule=rule)
    return {"gate at": mk(open_, reset_rule(0.25)), "gate below": mk(open_, reset_rule(dn(0.25))),
            "gate half gain": mk(open_, reset_rule(0.25, gain=0.5)), "gate every 5": mk(open_, reset_rule(0.25, every=5)),
            "gate half gain every 5": mk(open_, reset_rule(0.5, gain=0.5, every=5)), "gate window": mk(window, reset_rule(0.25))}


# ---- clearance fold ------------------------------------------------------------------------------------------------------------
CLEAR_FIELD = (-8.0, -8.0, 8.0, 8.0)
CLEAR_POLYGONS = (np.array([[1.0, -2.0], [2.0, -2.0], [2.0, 2.0], [1.0, 2.0]]),         # 1/4 ft off the square robot's right side
                  np.array([[-2.0, -2.0], [-1.0, -2.0], [-1.0, 2.0], [-2.0, 2.0]]))     # 1/4 ft off its left side: a tie
CLEAR_RECORDS = ({}, {1: 0.25}, {0: -0.125}, {0: 0.125})                                 # 1/4 (element 0), 1/4, 1/8 (element 1), 1/8 (element 0)


def clear_family():
    """A stationary 18 in square robot at the origin between two walls.  Layouts: one workgroup (the split kernel), K = 300 (the
    reduce kernel), and 300 workgroups of K = 256 (more than the device has CUs: the lane kernel)."""
    cases = {}
    for kind in ("ramsete", "pursuit"):
        f = follower(kind, **(dict(min_speed=0.0) if kind == "pursuit" else {}))
        for name, n, B, K in (("small", 5, 3, 4), ("K300", 5, 2, 300), ("lanes", 6, 300, 256)):
            P = np.tile(records(*CLEAR_RECORDS), (K // 4, 1))
            Pb = np.stack([np.roll(P, b % 3, axis=0) for b in range(B)])
            for mname, margin in (("at", 0.25), ("above", up(0.25))):
                clear = dict(foot=rcr.SQUARE, field=CLEAR_FIELD, polygons=CLEAR_POLYGONS, margin=margin)
                cases[f"clear {name} {mname} {kind}"] = make_case(kind, [still_route(n, 0.0, 0.0)] * B, f, Pb, clear=clear)
        # the mean clearance is the ascending-k sum: one wall whose face is the double above 3/4.  The robot at the origin is 2^-53
        # off it; record 0 starts the robot at x = -(1 - 2^-53), exactly 1 ft off it (its far side, x - 3/4, rounds: not strict)
        clear = dict(foot=rcr.SQUARE, field=CLEAR_FIELD, polygons=(np.array([[up(0.75), -2.0], [2.0, -2.0], [2.0, 2.0], [up(0.75), 2.0]]),), margin=0.25)
        for K in (5, 300):
            P = records(*([{0: -dn(1.0)}] + [{}] * (K - 1)))
            cases[f"clear mean K{K} {kind}"] = make_case(kind, [still_route(5, 0.0, 0.0)], f, P, strict=False, clear=clear)
    return cases


FAMILIES = {"wrap": wrap_family, "first": first_family, "drive": drive_family, "contraction": contraction_family,
            "validity": validity_family, "pointers": pointers_family, "gate": gate_family, "clear": clear_family}


@functools.lru_cache(maxsize=None)
def family(name):
    """The named cases of a family, built once."""
    return FAMILIES[name]()


# ---- the outputs of a case, from per-rollout results -----------------------------------------------------------------------------
SUMMARY = ("worst", "mean", "worst_rollout", "worst_row", "n_exceeding")
CLEAR_SUMMARY = ("worst_clearance", "worst_clear_rollout", "worst_clear_row", "worst_clear_element", "mean_clearance", "n_colliding",
                 "n_clear_valid")


def keys_of(case):
    keys = ["stats", "stat_rows", "rows", "counts"] + list(SUMMARY)
    if case["kind"] == "pursuit":
        keys += ["n_unfinished", "route_status"]
    if case["kind"] == "odometry":
        keys += ["est_rows"]
    if case["clear"]:
        keys += ["clearance", "clear_rows"] + list(CLEAR_SUMMARY)
    return keys


def n_of(case, b):
    return int(min(max(int(case["counts"][b]), 0), case["rows"].shape[1]))


def assemble(case, rollout, summary, fold):
    """rollout(b, k) -> dict of one rollout's stats, stat_rows, rows (T, 8), count[, est (T, 4), clearance, clear_rows]; summary(stats
    (K, .), stat_rows (K, .)) and fold(clearance (K,), clear_rows (K, 4)) -> the per-route dicts."""
    B, K = case["P"].shape[:2]
    per = [[rollout(b, k) for k in range(K)] for b in range(B)]
    stack = lambda key: np.array([[per[b][k][key] for k in range(K)] for b in range(B)])
    out = {"stats": stack("stats"), "stat_rows": stack("stat_rows").astype(np.int64), "counts": stack("count").reshape(B * K).astype(np.int64)}
    out["rows"] = stack("rows").reshape(B * K, -1, 8)
    if case["kind"] == "odometry":
        out["est_rows"] = stack("est").reshape(B * K, -1, 4)
    summ = [summary(out["stats"][b], out["stat_rows"][b]) for b in range(B)]
    for key in summ[0]:
        out[key] = np.array([s[key] for s in summ])
    if case["kind"] == "pursuit":
        out["route_status"] = np.array([pr.route_status(case["rows"][b], n_of(case, b)) for b in range(B)])
    if case["clear"]:
        out["clearance"], out["clear_rows"] = stack("clearance"), stack("clear_rows").astype(np.int64)
        folds = [fold(out["clearance"][b], out["clear_rows"][b]) for b in range(B)]
        for key in CLEAR_SUMMARY:
            out[key] = np.array([s[key] for s in folds])
    return out


def padded(a, T, width):
    out = np.full((T, width), np.nan)
    out[:len(a)] = a
    return out


def memo_key(case, b, k):
    extra = (case["O"][b, k].tobytes(),) if case["kind"] == "odometry" else ()
    return (case["rows"][b].tobytes(), int(case["counts"][b]), case["P"][b, k].tobytes()) + extra


# ---- the NumPy references ---------------------------------------------------------------------------------------------------------
def reference(case):
    """The outputs of a case by tracking_ref / pursuit_ref / odometry_ref (float64), footprint_ref on the executed rows and the
    references' summaries.  Equal (route, record) pairs are computed once."""
    kind, f, dt = case["kind"], case["f"], case["dt"]
    T = case["rows"].shape[1] + int(f["settle_rows"])
    memo = {}

    def rollout(b, k):
        key = memo_key(case, b, k)
        if key in memo:
            return memo[key]
        rows, n, p = case["rows"][b], n_of(case, b), case["P"][b, k]
        with np.errstate(all="ignore"):
            if kind == "odometry":
                scene = orf.PackedScene(case["field"]) if case["sensors"] is not None else None
                r = orf.rollouts(rows[None], [n], f, p[None, None], case["O"][b, k][None, None], case["sensors"], scene, case["rule"], dt,
                                 executed=True, estimates=True)
                out = dict(stats=r["stats"][0, 0], stat_rows=r["stat_rows"][0, 0], rows=r["rows"][0], count=int(r["counts"][0]), est=r["est_rows"][0])
            else:
                r = (tr if kind == "ramsete" else pr).rollout(rows, n, f, p, dt, executed=True)
                out = dict(stats=r["stats"][0], stat_rows=r["stat_rows"][0], rows=padded(r["rows"][0], T, 8), count=int(r["counts"][0]))
        if case["clear"]:
            c = case["clear"]
            s = fr.route_summary(out["rows"], out["count"], c["foot"], field=c["field"], polygons=c["polygons"], margin=c["margin"])
            out.update(clearance=s["min_clearance"], clear_rows=[s["min_row"], s["min_element"], s["first_row"], s["n_below"]])
        memo[key] = out
        return out

    summary = lambda st, sr: (pr if kind == "pursuit" else tr).route_summary(st, sr, f["tolerance"])
    return assemble(case, rollout, summary, lambda c, cr: rcr.fold(c, cr, case["clear"]["margin"]))


# ---- the exact checker ------------------------------------------------------------------------------------------------------------
# The header's rules and their neighbours.  True is the header's side.
RULES = {"max_first": True,           # the row of the maximum: a strictly larger error replaces (False: >=, the last row)
         "sat_strict": True,           # m > wheel_speed_max saturates (False: >=)
         "wrap_low": True,             # the wrap maps onto [-pi, pi) (False: (-pi, pi])
         "gain_strict": True,          # the wheel gains and the odometry record's factors > 0 (False: >= 0; track_scale divides)
         "tau_inclusive": True,        # tau >= 0 (False: > 0)
         "slot7_inclusive": True,      # pure pursuit: slot 7 >= 0 (False: > 0)
         "worst_first": True,          # the worst rollout: a strictly larger error replaces (False: >=, the last k)
         "exceed_strict": True,        # e > tolerance counts (False: >=)
         "mean_ascending": True,       # the means are one running sum in ascending k (False: in descending k)
         "closest_tie": True,          # the closest segment advances on D1 <= D (False: <)
         "arrive_inclusive": True,     # |P_last - p| <= arrive_tolerance (False: <)
         "gate_inclusive": True,       # |z - th| <= gate (False: <)
         "min_cos_inclusive": True,    # cosh >= min_cos (False: >)
         "near_strict": True,          # t < r_min is no reading (False: <=)
         "far_strict": True,           # t > r_max is no reading (False: >=)
         "clear_first": True,          # a rollout's clearance: a strictly smaller value replaces (False: <=, the last row)
         "below_strict": True,         # clearance < margin counts (False: <=)
         "clear_worst_first": True,    # the route's worst clearance: strictly smaller (False: <=, the last k)
         "element_first": True}        # the smallest element id on a tie (False: the largest)


class Exact:
    """Arithmetic on doubles through rationals.  A product must be a double; a sum must be one too unless it is ``named`` or
    the case is not strict; a quotient and a sqrt round once."""

    def __init__(self, strict, rule):
        self.strict, self.rule = strict, rule

    def mul(self, a, b):
        q = Fr(a) * Fr(b)
        f = fl(q)
        assert Fr(f) == q, ("a product that is no double", a, b)
        return f

    def add(self, a, b, named=False):
        q = Fr(a) + Fr(b)
        f = fl(q)
        assert named or not self.strict or Fr(f) == q, ("a sum that rounds", a, b)
        return f

    def sub(self, a, b, named=False):
        return self.add(a, -b, named)

    def div(self, a, b):
        return fl(Fr(a) / Fr(b))

    def sqrt(self, a):
        return sqrt_rounded(Fr(a))

    def sumsq(self, a, b):
        """a^2 + b^2.  With one of them zero the other's square may round: fma(a, a, 0) and fl(a a) + 0 are the same rounding."""
        if a == 0 or b == 0:
            return fl(Fr(a) * Fr(a) + Fr(b) * Fr(b))
        return self.add(self.mul(a, a), self.mul(b, b))

    def norm(self, a, b):
        """hypot and sqrt(a^2 + b^2) with one of them zero."""
        assert a == 0 or b == 0, ("two non-zero error components", a, b)
        return max(abs(a), abs(b))

    def wrap(self, a):
        t = self.add(a, PI, named=True)
        m = math.fmod(t, TWO_PI)
        q = Fr(t) / Fr(TWO_PI)
        whole = abs(q.numerator) // q.denominator * (1 if q >= 0 else -1)          # towards zero
        assert Fr(m) == Fr(t) - whole * Fr(TWO_PI), ("fmod", t)
        if m < 0:
            m = self.add(m, TWO_PI, named=True)
        r = self.sub(m, PI, named=True)
        return PI if (r == -PI and not self.rule["wrap_low"]) else r


def record_valid(p, rule, pursuit):
    if not all(math.isfinite(v) for v in p):
        return False
    pos = (lambda v: v > 0) if rule["gain_strict"] else (lambda v: v >= 0)
    ok = pos(p[3]) and pos(p[4]) and p[5] > 0 and (p[6] >= 0 if rule["tau_inclusive"] else p[6] > 0)
    return ok and (not pursuit or (p[7] >= 0 if rule["slot7_inclusive"] else p[7] > 0))


def odometry_valid(o, rule):
    pos = (lambda v: v > 0) if rule["gain_strict"] else (lambda v: v >= 0)
    return all(math.isfinite(v) for v in o) and pos(o[0]) and pos(o[1]) and pos(o[2]) and pos(o[4])


class Plant:
    """The plant of include/vap.h for motion along x: omega is asserted to be zero, and the robot moves only at heading 0."""

    def __init__(self, A, f, p, row0, dt):
        assert row0[4] == 0.0 and row0[5] == 0.0
        self.A, self.dt, self.nsub = A, dt, int(f["n_substeps"])
        self.h = A.div(dt, self.nsub)
        assert Fr(self.h) * self.nsub == Fr(dt)
        self.gl, self.gr, self.tts = p[3], p[4], A.mul(f["track_width"], p[5])
        # a = 1 - exp(-h / tau): 1 for tau = 0, and for a tau so small that exp underflows to exactly 0
        assert p[6] == 0.0 or Fr(self.h) / Fr(p[6]) > 800, ("a lag", p[6])
        self.x, self.y, self.phi = A.add(row0[6], p[0]), A.add(row0[7], p[1]), A.add(0.0, p[2])
        self.wl = self.wr = float(row0[2])
        self.dist = self.vprev = 0.0
        self.wmax, self.nsat = f["wheel_speed_max"], 0

    def speed(self):
        A = self.A
        left, right = A.mul(self.gl, self.wl), A.mul(self.gr, self.wr)
        assert A.div(A.sub(right, left), self.tts) == 0.0
        return A.div(A.add(left, right), 2.0)

    def row(self, r):
        A = self.A
        v = self.speed()
        out = [A.mul(r, self.dt), self.dist, v, A.div(A.sub(v, self.vprev), self.dt) if r > 0 else 0.0, -A.wrap(self.phi), 0.0, self.x, self.y]
        self.vprev = v
        return out

    def drive(self, cl, cr):
        """Saturation, then the substeps (tau = 0: the wheels take the command)."""
        A = self.A
        m = max(abs(cl), abs(cr))
        if m > self.wmax or (m == self.wmax and not A.rule["sat_strict"]):
            scale = A.div(self.wmax, m)
            cl, cr = A.mul(cl, scale), A.mul(cr, scale)
            self.nsat += 1
        for _ in range(self.nsub):
            self.wl = A.add(self.wl, A.mul(A.sub(cl, self.wl), 1.0))
            self.wr = A.add(self.wr, A.mul(A.sub(cr, self.wr), 1.0))
            d = A.mul(A.mul(self.speed(), self.h), 1.0)
            assert d == 0.0 or self.phi == 0.0
            self.x = A.add(self.x, d)
            self.dist = A.add(self.dist, abs(d))


class Maximum:
    def __init__(self, first):
        self.v, self.row, self.first = -math.inf, -1, first

    def take(self, e, r):
        if e > self.v or (e == self.v and not self.first):
            self.v, self.row = e, r


def exact_track(A, rows, n, f, p, dt, odo=None, sensors=None, field=None, reset=None):
    """vap_tracking_rollouts' steps 1-7 for one rollout, or vap_odometry_rollouts' with ``odo``."""
    rule = A.rule
    pl = Plant(A, f, p, rows[0], dt)
    settle, total = int(f["settle_rows"]), n + int(f["settle_rows"])
    assert (rows[:n, 4] == 0.0).all() and (rows[:n, 5] == 0.0).all() and (rows[:n, 7] == rows[0, 7]).all()
    yr = float(rows[0, 7])
    two_zeta, b = A.mul(2.0, f["zeta"]), f["b"]
    maxe, maxey, maxeph, maxest, maxestph = (Maximum(rule["max_first"]) for _ in range(5))
    hx, hy = float(rows[0, 6]), yr
    nacc = nrej = 0
    out_rows, est_rows = [], []
    for r in range(total):
        xr, vr = float(rows[min(r, n - 1), 6]), (float(rows[r, 2]) if r < n else 0.0)
        mask = 0
        if odo is not None and sensors is not None and r % reset["every"] == 0:
            assert pl.phi == 0.0
            xmin, ymin, xmax, ymax = field
            for s, (mx, my, ux, uy, r_min, r_max, min_cos, _) in enumerate(sensors):
                assert (ux, uy) == (1.0, 0.0)
                ox, oy = A.add(pl.x, mx), A.add(pl.y, my)
                if not (xmin <= ox <= xmax and ymin <= oy <= ymax):
                    continue
                t = A.sub(xmax, ox)
                if t < r_min or (t == r_min and not rule["near_strict"]) or t > r_max or (t == r_max and not rule["far_strict"]) or 1.0 < min_cos:
                    continue
                z = A.add(A.mul(odo[4], t), odo[5])
                eox, eoy = A.add(hx, mx), A.add(hy, my)
                accept = False
                if xmin <= eox <= xmax and ymin <= eoy <= ymax:
                    th = A.sub(xmax, eox)
                    diff = abs(A.sub(z, th))
                    accept = (1.0 >= reset["min_cos"] if rule["min_cos_inclusive"] else 1.0 > reset["min_cos"]) and \
                             (diff <= reset["gate"] if rule["gate_inclusive"] else diff < reset["gate"])
                if accept:
                    hx = A.add(hx, A.mul(A.mul(reset["gain"], A.sub(th, z)), 1.0))
                    mask |= 1 << s
                    nacc += 1
                else:
                    nrej += 1
        # errors: at heading 0 the body frame is the world's; with a heading offset there is no position offset
        dx, dy = A.sub(xr, pl.x), A.sub(yr, pl.y)
        if pl.phi != 0.0:
            assert dx == 0.0 and dy == 0.0
        eph = A.wrap(A.sub(0.0, pl.phi))
        maxe.take(A.norm(dx, dy), r)
        maxey.take(abs(dy), r)
        maxeph.take(abs(eph), r)
        if odo is not None:
            maxest.take(A.norm(A.sub(hx, pl.x), A.sub(hy, pl.y)), r)
            maxestph.take(abs(A.wrap(A.sub(0.0, pl.phi))), r)
            est_rows.append([0.0, hx, hy, float(mask & 255)])
            cdx, cdy, ceph = A.sub(xr, hx), A.sub(yr, hy), 0.0               # the follower sees the estimate, whose heading stays 0
        else:
            cdx, cdy, ceph = dx, dy, eph
        out_rows.append(pl.row(r))
        # RAMSETE: omega_r = 0; cos e_phi multiplies v_r, k multiplies e_phi, b v_r sinc(e_phi) multiplies e_y
        kk = A.mul(two_zeta, A.sqrt(A.mul(A.mul(b, vr), vr)))
        assert ceph == 0.0 or (vr == 0.0 and kk == 0.0)
        assert vr == 0.0 or cdy == 0.0
        vc = A.add(vr, A.mul(kk, cdx))
        pl.drive(vc, vc)
        if odo is not None:                                                   # the estimate's substeps: no drift, omega = 0
            assert odo[3] == 0.0
            for _ in range(pl.nsub):
                hv = A.div(A.add(A.mul(odo[0], A.mul(pl.gl, pl.wl)), A.mul(odo[1], A.mul(pl.gr, pl.wr))), 2.0)
                hx = A.add(hx, A.mul(A.mul(hv, pl.h), 1.0))
            # (the plant's wheels do not change within a row once tau = 0, so the estimate may follow after the plant)
    xl = float(rows[n - 1, 6])
    stats = [maxe.v, maxey.v, maxeph.v, A.norm(A.sub(xl, pl.x), A.sub(yr, pl.y)), abs(A.wrap(A.sub(0.0, pl.phi))), 0.0]
    stat_rows = [maxe.row, pl.nsat]
    if odo is not None:
        stats = stats[:5] + [maxest.v, maxestph.v, A.norm(A.sub(hx, pl.x), A.sub(hy, pl.y))]
        stat_rows += [nacc, nrej]
    return dict(stats=stats, stat_rows=stat_rows, rows=out_rows, count=total, est=est_rows)


def exact_pursuit(A, rows, n, f, p, dt):
    """vap_pursuit_rollouts' steps 1-7 for one rollout on a polyline along x."""
    rule = A.rule
    pl = Plant(A, f, p, rows[0], dt)
    total = n + int(f["settle_rows"])
    X, Vp, Y = [float(v) for v in rows[:n, 6]], [float(v) for v in rows[:n, 2]], float(rows[0, 7])
    assert (rows[:n, 7] == Y).all()
    T, L = f["track_width"], (p[7] if p[7] > 0 else f["lookahead"])
    S = [A.sub(X[i + 1], X[i]) for i in range(n - 1)]
    LEN = [A.sqrt(A.mul(s, s)) for s in S]
    c = [0.0]
    for ln in LEN:
        c.append(A.add(c[-1], ln))
    uend = 1.0
    for i in range(n - 2, -1, -1):
        if LEN[i] > 0:
            uend = A.div(S[i], LEN[i])
            break
    ey = A.sub(pl.y, Y)

    def project(i):
        ss = A.mul(S[i], S[i])
        t = 0.0 if ss == 0 else min(max(A.div(A.mul(A.sub(pl.x, X[i]), S[i]), ss), 0.0), 1.0)
        ex = A.sub(pl.x, A.add(X[i], A.mul(t, S[i])))
        return t, A.sumsq(ex, ey)

    maxe = Maximum(rule["max_first"])
    ic = il = 0
    arrived = -1
    out_rows = []
    for r in range(total):
        if n >= 2:
            while ic < n - 2:
                d1, d0 = project(ic + 1)[1], project(ic)[1]
                if not (d1 <= d0 if rule["closest_tie"] else d1 < d0):
                    break
                ic += 1
            t, D = project(ic)
            ect = A.sqrt(D)
            vt = A.add(Vp[ic], A.mul(t, A.sub(Vp[ic + 1], Vp[ic])))
            sc = A.add(c[ic], A.mul(t, LEN[ic]))
            at_end = ic == n - 2 and t == 1.0
        else:
            ect, vt, sc, at_end = A.norm(A.sub(pl.x, X[0]), ey), Vp[0], 0.0, True
        maxe.take(ect, r)
        out_rows.append(pl.row(r))
        dend = A.norm(A.sub(X[n - 1], pl.x), A.sub(Y, pl.y))
        if arrived < 0 and (at_end or dend < f["arrive_tolerance"] or (dend == f["arrive_tolerance"] and rule["arrive_inclusive"])):
            arrived = r
        cl = cr = 0.0
        if arrived < 0:
            assert pl.phi == 0.0
            star = A.add(sc, L)
            il = max(il, ic)
            while il < n - 2 and c[il + 1] < star:
                il += 1
            if star >= c[n - 1]:
                gx = A.add(X[n - 1], A.mul(A.sub(star, c[n - 1]), uend))
            else:
                fr_ = 0.0 if LEN[il] == 0 else min(max(A.div(A.sub(star, c[il]), LEN[il]), 0.0), 1.0)
                gx = A.add(X[il], A.mul(fr_, S[il]))
            dx, dy = A.sub(gx, pl.x), A.sub(Y, pl.y)
            a2 = A.sumsq(dx, dy)
            kap = 0.0 if a2 == 0 else A.div(A.mul(2.0, dy), a2)
            sp = max(vt, f["min_speed"])
            turn = A.div(A.mul(A.mul(sp, kap), T), 2.0)
            cl, cr = A.sub(sp, turn), A.add(sp, turn)
        pl.drive(cl, cr)
    stats = [maxe.v, A.norm(A.sub(X[n - 1], pl.x), A.sub(Y, pl.y)), A.mul(arrived, dt) if arrived >= 0 else math.nan, L, 0.0, 0.0]
    return dict(stats=stats, stat_rows=[maxe.row, pl.nsat, arrived, ic], rows=out_rows, count=total)


def exact_clearance(A, x, y, clear):
    """(clearance, element) of the square robot at heading 0 against the walls and axis-parallel rectangles beside it."""
    rule = A.rule
    half = float(clear["foot"][:, 0].max())
    assert sorted(map(tuple, np.abs(clear["foot"]).tolist())) == [(half, half)] * 4
    x0, x1, y0, y1 = A.sub(x, half), A.add(x, half), A.sub(y, half), A.add(y, half)
    xmin, ymin, xmax, ymax = clear["field"]
    cand = [(min(A.sub(x0, xmin), A.sub(xmax, x1), A.sub(y0, ymin), A.sub(ymax, y1)), -1)]
    for k, q in enumerate(clear["polygons"]):
        qx0, qy0, qx1, qy1 = (float(v) for v in (q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()))
        gx, gy = max(A.sub(qx0, x1), A.sub(x0, qx1)), max(A.sub(qy0, y1), A.sub(y0, qy1))
        assert (gx > 0) != (gy > 0), "a rectangle beside the robot, not diagonal to it and not touching"
        cand.append((max(gx, gy), k))
    best = min(v for v, _ in cand)
    ids = [e for v, e in cand if v == best]
    return best, (min(ids) if rule["element_first"] else max(ids))


def exact_fold_rows(A, res, clear):
    rule, margin = A.rule, clear["margin"]
    best, row, el, first, nb = math.inf, -1, -1, -1, 0
    for r in range(res["count"]):
        v, e = exact_clearance(A, res["rows"][r][6], res["rows"][r][7], clear)
        assert res["rows"][r][4] == 0.0
        if v < margin or (v == margin and not rule["below_strict"]):
            nb += 1
            first = r if first < 0 else first
        if v < best or (v == best and not rule["clear_first"]):
            best, row, el = v, r, e
    return dict(clearance=best if row >= 0 else math.nan, clear_rows=[row, el if row >= 0 else -1, first, nb])


def running_sum(A, terms):
    """One running sum from 0.0, every addition rounded, in ascending k (the neighbour: descending)."""
    total = 0.0
    for v in (terms if A.rule["mean_ascending"] else terms[::-1]):
        total = A.add(total, v, named=True)
    return total


def exact_summary(A, stats, stat_rows, tolerance, pursuit):
    rule = A.rule
    worst, wk, wrow, terms, cnt, nex, nun = -math.inf, -1, -1, [], 0, 0, 0
    for k in range(len(stats)):
        if stat_rows[k][0] < 0:
            continue
        e = float(stats[k][0])
        if e > worst or (e == worst and not rule["worst_first"]):
            worst, wk, wrow = e, k, int(stat_rows[k][0])
        terms.append(e)
        cnt += 1
        nex += int(e > tolerance or (e == tolerance and not rule["exceed_strict"]))
        nun += int(pursuit and stat_rows[k][2] < 0)
    total = running_sum(A, terms)
    out = dict(worst=worst if cnt else math.nan, mean=A.div(total, cnt) if cnt else math.nan, worst_rollout=wk, worst_row=wrow, n_exceeding=nex)
    if pursuit:
        out["n_unfinished"] = nun
    return out


def exact_fold(A, clearance, clear_rows, margin):
    rule = A.rule
    worst, wk, wrow, wel, terms, cnt, ncol = math.inf, -1, -1, -1, [], 0, 0
    for k in range(len(clearance)):
        if clear_rows[k][0] < 0:
            continue
        c = float(clearance[k])
        if c < worst or (c == worst and not rule["clear_worst_first"]):
            worst, wk, wrow, wel = c, k, int(clear_rows[k][0]), int(clear_rows[k][1])
        terms.append(c)
        cnt += 1
        ncol += int(c < margin or (c == margin and not rule["below_strict"]))
    total = running_sum(A, terms)
    return dict(worst_clearance=worst if cnt else math.nan, worst_clear_rollout=wk, worst_clear_row=wrow, worst_clear_element=wel,
                mean_clearance=A.div(total, cnt) if cnt else math.nan, n_colliding=ncol, n_clear_valid=cnt)


def exact(case, **rules):
    """The header's outputs of a case in ``reference``'s layout, in exact arithmetic; ``rules`` switches rules to their neighbours."""
    assert set(rules) <= set(RULES), rules
    A = Exact(case["strict"], dict(RULES, **rules))
    kind, f, dt = case["kind"], case["f"], case["dt"]
    T = case["rows"].shape[1] + int(f["settle_rows"])
    nan_stats = {"ramsete": (6, 2), "pursuit": (6, 4), "odometry": (8, 4)}[kind]
    memo = {}

    def rollout(b, k):
        key = memo_key(case, b, k)
        if key in memo:
            return memo[key]
        rows, n = case["rows"][b], n_of(case, b)
        p = [float(v) for v in case["P"][b, k]]
        o = [float(v) for v in case["O"][b, k]] if kind == "odometry" else None
        ok = n > 0 and record_valid(p, A.rule, kind == "pursuit") and (o is None or odometry_valid(o, A.rule))
        if kind == "pursuit" and pr.route_status(rows, n):
            ok = False
        if not ok:
            out = dict(stats=[math.nan] * nan_stats[0], stat_rows=[-1] * nan_stats[1], rows=[], count=0, est=[])
        elif kind == "pursuit":
            out = exact_pursuit(A, rows, n, f, p, dt)
        else:
            out = exact_track(A, rows, n, f, p, dt, o, case.get("sensors"), case.get("field"), case.get("rule"))
        if case["clear"]:
            out.update(exact_fold_rows(A, out, case["clear"]))
        out["rows"] = padded(np.array(out["rows"], dtype=np.float64).reshape(-1, 8), T, 8)
        out["est"] = padded(np.array(out.get("est", []), dtype=np.float64).reshape(-1, 4), T, 4)
        memo[key] = out
        return out

    summary = lambda st, sr: exact_summary(A, st, sr, f["tolerance"], kind == "pursuit")
    return assemble(case, rollout, summary, lambda c, cr: exact_fold(A, c, cr, case["clear"]["margin"]))


def same(a, b, keys, zero_sign=True):
    """The first difference between two output dicts over ``keys`` (floats bit for bit, every NaN one NaN), or None.  zero_sign
    False: -0.0 and +0.0 are one value."""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if x.dtype.kind == "f" or y.dtype.kind == "f":
            x, y = x.astype(np.float64), y.astype(np.float64)
            if not zero_sign:
                x, y = x + 0.0, y + 0.0
            x, y = np.where(np.isnan(x), -1, x.view(np.int64)), np.where(np.isnan(y), -1, y.view(np.int64))
        bad = np.argwhere(x != y)
        if len(bad):
            i = tuple(bad[0])
            return k, i, np.asarray(a[k])[i], np.asarray(b[k])[i], len(bad)
    return None
