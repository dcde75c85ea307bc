"""CPU: the definitions of vap_plan_order_timed (include/vap.h) through tests/order_timed_ref.py — its two statements (brute
force and Held-Karp) against each other on random integer problems with planted ties, the brute force's rows and arrivals
against tests/timeline_ref.py's chain for every sequence of a small problem, the worked A / B case on legs from the oracle,
and the entry point's argument errors by value, without a device.  Everything compared is an integer or an fp64 sum formed
in a stated order: no tolerances."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import order_ref as orf
import order_timed_ref as otr
import test_timeline_cpu as tc
import timeline_ref as tr

CONS = tc.CONS
SLOW = (1.0,) + CONS[1:]           # max_vel = 1: every turn reaches it (the trapezoid branch)
HEADINGS = (0.0, -0.0, 1.0, -2.0, 3.0, -3.0, math.pi, -math.pi, 1.0 + math.radians(0.9), 1.0 + math.radians(1.1))
COUNTS = (1, 5, 5, 7, 9, 12)
OUTPUTS = ("order", "n_visited", "rows_total", "arrival_rows", "value_total", "flags")


def same(a, b):
    """Every output of two solutions: integers equal, value_total the same bits or NaN in both."""
    for k in OUTPUTS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "value_total":
            x, y = x.astype(np.float64), y.astype(np.float64)
            ok = x.shape == y.shape and bool(((x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))).all())
        else:
            ok = x.shape == y.shape and np.array_equal(x.astype(np.int64), y.astype(np.int64))
        assert ok, (k, x, y)
    return True


def random_legs(rng, L, cap, counts=COUNTS, headings=HEADINGS):
    """L caller-written legs: only the first and the last row are read, the rest stays NaN.  Counts and headings come from
    small sets, so equal totals are common.  Returns rows (L, cap, 8), counts (L, 2) int32, flags (L,) uint32."""
    rows = np.full((L, cap, 8), np.nan)
    cnt = rng.choice(counts, size=L).astype(np.int32)
    for l in range(L):
        c = min(int(cnt[l]), cap)
        if c <= 0:
            continue
        for at in {0, c - 1}:
            rows[l, at] = 0.0
            rows[l, at, 6:8] = rng.uniform(-5, 5, 2)
        rows[l, 0, 4] = rng.choice(headings)
        if c > 1:
            rows[l, c - 1, 4] = rng.choice(headings)
    return rows, np.stack([cnt, np.full(L, -99, dtype=np.int32)], axis=1), np.zeros(L, dtype=np.uint32)


def spoil(rng, rows, counts, flags, how_many):
    """Make some legs unusable, each in one of the ways the header lists.  Returns the spoilt leg numbers."""
    L = len(rows)
    which = rng.choice(np.arange(3, L), size=min(how_many, L - 3), replace=False)     # legs 0..2 stay the tie makers
    for n, l in enumerate(which):
        kind = n % 5
        c = max(int(counts[l, 0]), 1)
        if kind == 0:
            flags[l] = 4
        elif kind == 1:
            counts[l, 0] = 0
        elif kind == 2:
            counts[l, 0] = -3
        elif kind == 3:
            rows[l, rng.choice([0, c - 1]), 6] = np.nan
        else:
            rows[l, rng.choice([0, c - 1]), 4] = 7.0
    return which


def random_problems(rng, R, M, L, cap=16, spoilt=0, bad_index=0.1, **kw):
    """R problems of M sites over L >= 4 shared legs; a fraction of the leg matrix points outside [0, L).  Legs 0..2 are
    alike (5 rows, heading 1.0 at both ends) and about a third of the problems use only them: every order ties there."""
    P = M + 1
    rows, counts, flags = random_legs(rng, L, cap, **kw)
    for l in range(3):
        counts[l, 0] = 5
        rows[l, :5] = 0.0
        rows[l, :5, 4] = 1.0
    spoil(rng, rows, counts, flags, spoilt)
    leg = rng.integers(0, L, size=(R, P, P)).astype(np.int32)
    for r in range(R):
        if rng.random() < 0.35:
            leg[r] = rng.integers(0, 3, size=(P, P))
    out = rng.random((R, P, P)) < bad_index
    leg[out] = rng.choice([-1, L, L + 7, -2 ** 31], size=int(out.sum()))
    dwell = rng.choice([0.0, 0.05, 0.05, 0.019, np.nan, -1.0, 0.1], size=(R, P))
    start = rng.choice(list(HEADINGS) + [np.nan, np.nan], size=R)
    value = rng.choice([1.0, 1.0, 2.0, 0.5, 3.0, 0.0], size=(R, P))
    before = np.zeros((R, P), dtype=np.uint32)
    for r in range(R):
        if rng.random() < 0.5:
            j, k = rng.choice(np.arange(1, P), size=2, replace=False) if M > 1 else (1, 1)
            if j != k:
                before[r, k] |= np.uint32(1 << (j - 1))
    return dict(rows=rows, counts=counts, leg=leg, leg_flags=flags, dwell=dwell, start_heading=start, value=value, before=before)


def solve(pb, method, constraints=CONS, dt=0.01, budget_rows=None, end=None, **over):
    kw = dict(dwell=pb["dwell"], start_heading=pb["start_heading"], value=pb["value"], before=pb["before"],
              leg_flags=pb["leg_flags"])
    kw.update(over)
    return otr.solve(pb["rows"], pb["counts"], pb["leg"], constraints, dt=dt, budget_rows=budget_rows, end=end, method=method, **kw)


# ---------------------------------------------------------------- the two statements agree

@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6])
def test_brute_force_equals_held_karp(M):
    rng = np.random.default_rng(100 + M)
    R = 10 if M < 6 else 4
    seen_ties = 0
    for trial, (cons, dt) in enumerate([(CONS, 0.01), (SLOW, 0.02)]):
        pb = random_problems(rng, R, M, L=3 * M + 2, spoilt=2 if M > 2 else 0, bad_index=0.05)
        for end in (None, M, 1):
            full_b, full_d = solve(pb, "brute", cons, dt, end=end), solve(pb, "dp", cons, dt, end=end)
            assert same(full_b, full_d)
            top = int(max(full_b["rows_total"].max(), 40))
            for budget in (np.zeros(R, dtype=np.int64), rng.integers(0, top + 20, size=R), np.full(R, 10 ** 6), np.full(R, -5)):
                assert same(solve(pb, "brute", cons, dt, budget_rows=budget, end=end),
                            solve(pb, "dp", cons, dt, budget_rows=budget, end=end))
        # how often the tie rules decided: sequences of the full set with the winner's rows
        for r in range(R):
            p = otr.Problem(pb["rows"], pb["counts"][:, 0], pb["leg"][r], cons, dt, math.radians(1.0), pb["dwell"][r],
                            pb["start_heading"][r], pb["value"][r], None, None, pb["before"][r], pb["leg_flags"])
            totals = [g[0] for g in (p.sequence(s) for s in itertools.permutations(range(1, M + 1))) if g is not None]
            seen_ties += len(totals) > 1 and totals.count(min(totals)) > 1
    if M >= 3:
        assert seen_ties > 0                                            # the planted ties are there


def test_ample_budget_with_positive_values_is_full_mode():
    rng = np.random.default_rng(7)
    pb = random_problems(rng, 12, 4, L=14, bad_index=0.0)
    pb["value"] = rng.choice([1.0, 2.0, 0.25], size=pb["value"].shape)
    full = solve(pb, "brute")
    ample = solve(pb, "brute", budget_rows=np.full(12, otr.INT_MAX))
    feasible = full["flags"] == 0
    assert feasible.sum() >= 6
    for k in ("order", "n_visited", "rows_total", "arrival_rows", "value_total"):
        assert np.array_equal(full[k][feasible], ample[k][feasible]), k
    # an infeasible full problem still has its best subset under a budget
    assert (ample["flags"] == 0).all()


def test_budget_rules_by_hand():
    """Two sites, legs of 10 rows each way, no turns (all headings equal), no dwell."""
    leg_rows = [tc.straight_leg(10, (0, 0), 0.5, 1.0, 0.01) for _ in range(4)] + [tc.straight_leg(4, (0, 0), 0.5, 1.0, 0.01)]
    rows, counts = tc.pack(leg_rows)
    leg = np.array([[[-1, 0, 1], [-1, -1, 2], [-1, 3, -1]]])           # 0->1: 10, 0->2: 10, 1->2: 10, 2->1: 10
    s = lambda **kw: otr.solve(rows, counts, leg, CONS, method="brute", **kw)
    assert s()["order"].tolist() == [[2, 1]] and s()["rows_total"].tolist() == [20]          # 1, 2 ties with 2, 1: the lowest LAST site
    assert s(budget_rows=[0])["n_visited"].tolist() == [0] and s(budget_rows=[0])["value_total"].tolist() == [0.0]
    assert s(budget_rows=[0])["rows_total"].tolist() == [0] and s(budget_rows=[0])["flags"].tolist() == [0]
    assert s(budget_rows=[9])["n_visited"].tolist() == [0]
    assert s(budget_rows=[10])["order"].tolist() == [[1, -1]]                                # equal value and rows: lowest S
    assert s(budget_rows=[19])["order"].tolist() == [[1, -1]] and s(budget_rows=[20])["n_visited"].tolist() == [2]
    v = np.array([[0.0, 1.0, 1.5]])
    assert s(budget_rows=[10], value=v)["order"].tolist() == [[2, -1]] and s(budget_rows=[10], value=v)["value_total"].tolist() == [1.5]
    bad = np.array([[0.0, np.nan, -2.0]])
    assert s(budget_rows=[100], value=bad)["n_visited"].tolist() == [0]                      # nothing is worth a row
    assert s(budget_rows=[9], end=1)["flags"].tolist() == [otr.INFEASIBLE]                   # must end at 1, nothing fits
    assert s(budget_rows=[9], end=1)["rows_total"].tolist() == [-1] and np.isnan(s(budget_rows=[9], end=1)["value_total"][0])
    # site 1 waits for the worthless site 2: taking 1 means taking 2 first
    forced = s(budget_rows=[100], value=np.array([[0.0, 1.0, 0.0]]), before=np.array([[0, 2, 0]], dtype=np.uint32))
    assert forced["order"].tolist() == [[2, 1]] and forced["value_total"].tolist() == [1.0]
    assert s(start_heading=[7.0])["flags"].tolist() == [otr.INFEASIBLE]
    assert s(start_heading=[7.0], budget_rows=[100])["flags"].tolist() == [otr.INFEASIBLE]   # the empty routine is bad as well


# ---------------------------------------------------------------- the rows are the timeline's

def pair_legs(points, dt, speed=2.0, curve=0.4):
    """One synthesised leg per ordered pair of points: straight, at the pair's bearing plus a kink in the last row, so that
    arrival and departure headings differ.  Returns rows, counts and the (P, P) leg matrix."""
    P = len(points)
    legs, mat = [], np.full((P, P), -1, dtype=np.int32)
    for a in range(P):
        for b in range(1, P):
            if a == b:
                continue
            d = np.subtract(points[b], points[a])
            length = float(np.hypot(*d))
            n = max(int(length / speed / dt), 2)
            l = tc.straight_leg(n, points[a], -math.atan2(d[1], d[0]), length, dt)
            l[-1, 4] += curve * ((a + 2 * b) % 3 - 1)
            mat[a, b] = len(legs)
            legs.append(l)
    rows, counts = tc.pack(legs)
    return rows, counts, mat


@pytest.mark.parametrize("cons,dt", [(CONS, 0.01), (SLOW, 0.02)], ids=["triangle-10ms", "trapezoid-20ms"])
def test_every_sequence_against_the_timeline(cons, dt):
    points = [(0.0, 0.0), (1.0, 0.2), (-0.5, 0.8), (0.3, -0.9)]
    rows, counts, mat = pair_legs(points, dt)
    dwell = np.array([9.9, 0.13, 0.0, 0.055])
    for h0 in (float("nan"), 2.5):
        p = otr.Problem(rows, counts, mat, cons, dt, math.radians(1.0), dwell, h0, None, None, None, None, None)
        n_seq = 0
        for k in (1, 2, 3):
            for seq in itertools.permutations((1, 2, 3), k):
                total, arrivals = p.sequence(seq)
                stops = (0,) + seq
                legs = [[int(mat[stops[m], stops[m + 1]]) for m in range(k)] + [-1] * (3 - k)]
                ref = tr.chain(rows, counts, legs, cons, dt=dt, dwell=[[dwell[s] for s in seq] + [0.0] * (3 - k)],
                               start_heading=[h0], n_legs=[k])
                assert ref["flags"][0] == 0 and int(ref["counts"][0, 0]) == total == int(ref["total"][0])
                assert ref["map"][0, :k, 2].tolist() == arrivals and ref["counts"][0, 1] == k
                n_seq += 1
        assert n_seq == 15
        # and the winner of either statement is the cheapest of them
        for method in ("brute", "dp"):
            got = otr.solve(rows, counts, mat[None], cons, dt=dt, dwell=dwell[None], start_heading=[h0], method=method)
            best = min(p.sequence(s)[0] for s in itertools.permutations((1, 2, 3)))
            assert got["rows_total"][0] == best and got["n_visited"][0] == 3
    # a forbidden leg in the sequence is the timeline's bad routine
    flags = np.zeros(len(rows), dtype=np.uint32)
    flags[mat[1, 2]] = 1
    p = otr.Problem(rows, counts, mat, cons, dt, math.radians(1.0), None, None, None, None, None, None, flags)
    assert p.sequence((1, 2, 3)) is None and p.sequence((2, 1, 3)) is not None


# ---------------------------------------------------------------- the worked case

AB_POINTS = {0: (0.0, 0.0), 1: (3.0, 0.0), 2: (-3.2, 0.0)}              # site 1 = A, site 2 = B; the robot faces -x


def ab_case(profile):
    """rows, counts, the (3, 3) leg matrix of the A / B case; profile(waypoints (3, 2)) -> (n, 8) rows."""
    legs, mat = [], np.full((3, 3), -1, dtype=np.int32)
    for a, b in ((0, 1), (0, 2), (1, 2), (2, 1)):
        mat[a, b] = len(legs)
        legs.append(profile(np.linspace(AB_POINTS[a], AB_POINTS[b], 3)))
    rows, counts = tc.pack(legs)
    return rows, counts, mat


def test_the_length_order_is_the_slower_one():
    from oracle import oracle
    rows, counts, mat = ab_case(lambda wp: oracle.OraclePath(wp).generate_motion_profile(CONS, dt=0.01)[0])
    assert counts.tolist() == [122, 127, 202, 202]                       # 0->A, 0->B, A->B, B->A, from the oracle
    length = np.array([[0.0, 3.0, 3.2], [3.0, 0.0, 6.2], [3.2, 6.2, 0.0]])
    assert orf.order(length)[0] == [1, 2] and orf.order(length)[1] == 9.2
    half = tr.turn_shape(math.pi, CONS[0], CONS[1], CONS[5], 0.01)[3]
    assert half == 92 and tr.turn_shape(math.pi / 2, CONS[0], CONS[1], CONS[5], 0.01)[3] == 65
    p = otr.Problem(rows, counts, mat, CONS, 0.01, math.radians(1.0), None, math.pi, None, None, None, None, None)
    ab, ba = p.sequence((1, 2)), p.sequence((2, 1))
    assert ab == (122 + 202 + 2 * half, [half + 122, 2 * half + 122 + 202]) and ba == (127 + 202 + half, [127, 127 + half + 202])
    assert ab[0] - ba[0] == 87                                           # 0.87 s on 0.2 ft
    for method in ("brute", "dp"):
        got = otr.solve(rows, counts, mat[None], CONS, start_heading=[math.pi], method=method)
        assert got["order"].tolist() == [[2, 1]] and got["rows_total"].tolist() == [421] and got["arrival_rows"].tolist() == [[127, 421]]
    # without a start heading the first half turn is gone and the length order is the faster one again
    assert otr.solve(rows, counts, mat[None], CONS, method="brute")["order"].tolist() == [[1, 2]]


# ---------------------------------------------------------------- the product

def test_product_declares_the_call():
    from vexautonomousplanner_amd import _lib, plan
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    L = _lib.lib()
    assert "vap_plan_order_timed" in _lib.EXPORTS and hasattr(L, "vap_plan_order_timed")
    assert callable(plan.order_timed) and callable(plan.timed_routine) and callable(BatchedTrajectoryGenerator.plan_timed_routine)
    header = open(_lib.HERE + "/../include/vap.h").read()
    assert "#define VAP_PLAN_ORDER_TIMED_MAX_SITES 8" in header
    assert plan.MAX_TIMED_SITES == _lib.PLAN_ORDER_TIMED_MAX_SITES == otr.MAX_SITES == 8
    assert otr.INFEASIBLE == _lib.ORDER_INFEASIBLE


def test_entry_point_checks_its_arguments_before_the_device():
    """Every VAP_ERR_INVALID / VAP_ERR_UNSUPPORTED case of the header, by value, with a null context.  A call whose
    arguments are all good gets as far as the context and fails there ("null context")."""
    from vexautonomousplanner_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)
    INV, UNS = _lib.VAP_ERR_INVALID, _lib.VAP_ERR_UNSUPPORTED

    def call(R=1, P=4, L_=9, cap=8, dt=0.01, cons=CONS, turn_min=0.01, rows=one, counts=one, stride=2, leg=one, leg_flags=None,
             dwell=None, start=None, value=None, budget=None, end=-1, before=None, order=one, n_visited=one, rows_total=one,
             arrival=one, value_total=one, flags=None):
        c = _lib.Constraints(*cons) if cons is not None else None
        st = L.vap_plan_order_timed(None, R, P, L_, cap, dt, C.byref(c) if c is not None else None, turn_min, rows, counts, stride,
                                    leg, leg_flags, dwell, start, value, budget, end, before, order, n_visited, rows_total,
                                    arrival, value_total, flags)
        return st, L.vap_last_error().decode()

    def refused(status, **kw):
        st, msg = call(**kw)
        assert st == status and "null context" not in msg, (kw, st, msg)

    def reaches_the_context(**kw):
        st, msg = call(**kw)
        assert st == INV and "null context" in msg, (kw, st, msg)

    reaches_the_context()
    reaches_the_context(P=2, end=1)
    reaches_the_context(P=9, end=8, leg_flags=one, dwell=one, start=one, value=one, budget=one, before=one, flags=one)
    reaches_the_context(R=0, rows=None, counts=None, leg=None, order=None, n_visited=None, rows_total=None, arrival=None,
                        value_total=None)
    reaches_the_context(L_=0, rows=None, counts=None)
    reaches_the_context(turn_min=0.0)
    slow = (1e-3,) + CONS[1:]
    for kw in (dict(P=1), dict(P=0), dict(R=-1), dict(L_=-1), dict(cap=-1), dict(stride=0), dict(end=0), dict(end=4), dict(end=-2),
               dict(dt=0.0), dict(dt=-0.01), dict(dt=np.nan), dict(dt=np.inf), dict(turn_min=-0.1), dict(turn_min=np.nan),
               dict(turn_min=np.inf), dict(cons=None), dict(cons=(0.0,) + CONS[1:]), dict(cons=CONS[:1] + (np.nan,) + CONS[2:]),
               dict(cons=CONS[:5] + (0.0,)), dict(rows=None), dict(counts=None), dict(leg=None), dict(order=None),
               dict(n_visited=None), dict(rows_total=None), dict(arrival=None), dict(value_total=None), dict(dt=1e-9),
               dict(cons=slow, dt=1e-4)):
        refused(INV, **kw)
    for kw in (dict(P=10), dict(P=11, end=10), dict(P=17)):
        refused(UNS, **kw)
