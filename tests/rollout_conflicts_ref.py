"""NumPy statement of vap_rollout_conflicts (include/vap.h) by composition, as the header defines it: the follower's
reference rollout with executed rows (tests/tracking_ref.py or tests/pursuit_ref.py), then, per rollout with its own start
shift, the robot-to-robot reference (tests/conflict_ref.py) of that one executed route against side O, then the per-route
fold in ascending k.

Also the fixed cases the CPU and the GPU tests share: the known-answer case, the partner routes laid against the rollout
layouts of tests/rollout_clearance_ref.py (LAYOUTS / layout_case, imported and unchanged) and the shift sets."""
import functools

import numpy as np

import conflict_ref as cr
import pursuit_ref as pr
import rollout_clearance_ref as rc
import tracking_ref as tr
from rollout_clearance_ref import DT, LAYOUTS, SQUARE, layout_case, ref_follower      # noqa: F401 (the tests' names)

SHIFT_MAX = 1 << 24
MARGIN = 0.1
CAP, SETTLE = 120, 20          # layout_case's capacity and ref_follower's settle rows
CAP_O = 700
OTHERS = (1, 3, 16)            # the partner counts of the GPU comparison; the smaller sets are prefixes of the largest
ROUTE_KEYS = ("worst_conflict", "worst_conflict_rollout", "worst_conflict_other", "worst_conflict_row", "mean_conflict",
              "n_conflicting", "n_conflict_valid")


def sums(shift_rows, route_shift, rollout_shift, B, K):
    """(B, K) int64: shift_rows + route_shift[b] + rollout_shift[k], the array entries clamped into +-2^24 first."""
    s = np.full((B, K), int(shift_rows), dtype=np.int64)
    if route_shift is not None:
        s += np.clip(np.asarray(route_shift, dtype=np.int64), -SHIFT_MAX, SHIFT_MAX)[:, None]
    if rollout_shift is not None:
        s += np.clip(np.asarray(rollout_shift, dtype=np.int64), -SHIFT_MAX, SHIFT_MAX)[None, :]
    return s


def fold(conflict, conflict_rows, margin):
    """The per-route outputs from one route's (K,) conflict clearances and (K, 4) conflict rows: the valid rollouts
    (conflict row >= 0) in ascending k; a strictly smaller value replaces; one running sum."""
    worst, wk, wo, wrow, total, cnt, ncon = np.inf, -1, -1, -1, np.float64(0), 0, 0
    for k in range(len(conflict)):
        if conflict_rows[k, 1] < 0:
            continue
        c = np.float64(conflict[k])
        if c < worst:
            worst, wk, wo, wrow = c, k, int(conflict_rows[k, 0]), int(conflict_rows[k, 1])
        total = total + c
        cnt += 1
        ncon += int(c < margin)
    if cnt == 0:
        return dict(worst_conflict=np.nan, worst_conflict_rollout=-1, worst_conflict_other=-1, worst_conflict_row=-1,
                    mean_conflict=np.nan, n_conflicting=0, n_conflict_valid=0)
    return dict(worst_conflict=worst, worst_conflict_rollout=wk, worst_conflict_other=wo, worst_conflict_row=wrow,
                mean_conflict=total / cnt, n_conflicting=ncon, n_conflict_valid=cnt)


def rollout_pairs(exec_rows, n_a, foot, rows_o, counts_o, foot_o, margin, shift):
    """One rollout's executed rows (cap_exec, 8) and count against side O at its own shift: the conflict reference's dict
    for that one route of side A."""
    return cr.conflicts(np.asarray(exec_rows, dtype=np.float64)[None], [int(n_a)], foot, rows_o, counts_o, foot_o, margin=margin, shift=int(shift))


def compose(executed, counts, foot, rows_o, counts_o, foot_o, margin, shifts):
    """K executed routes (K, cap_exec, 8) with their counts and shifts (K,): pair_clearance (K, Bo), pair_rows (K, Bo, 2),
    conflict (K,), conflict_rows (K, 4), the references' dicts as ``per``, and the fold's outputs."""
    K, Bo = len(counts), len(rows_o)
    per = [rollout_pairs(executed[k], counts[k], foot, rows_o, counts_o, foot_o, margin, shifts[k]) for k in range(K)]
    out = dict(per=per, pair_clearance=np.array([p["pair_clearance"][0] for p in per], dtype=np.float64).reshape(K, Bo),
               pair_rows=np.array([np.stack([p["pair_row"][0], p["pair_first_row"][0]], axis=1) for p in per], dtype=np.int64).reshape(K, Bo, 2),
               conflict=np.array([p["min_clearance"][0] for p in per], dtype=np.float64),
               conflict_rows=np.array([[p["min_other"][0], p["min_row"][0], p["n_conflicts"][0], p["first_row"][0]] for p in per],
                                      dtype=np.int64).reshape(K, 4))
    out.update(fold(out["conflict"], out["conflict_rows"], margin))
    return out


def route(rows, n, kind, f, P, foot, rows_o, counts_o, foot_o=None, margin=0.0, shifts=None, time_step=DT):
    """One route: ``kind`` "ramsete" (f: tracking_ref.follower) or "pursuit" (f: pursuit_ref.pursuit), records P (K, 8),
    ``shifts`` (K,) rows (None: 0).  Returns ``compose``'s dict with the follower's reference dict as ``rollout``."""
    mod = {"ramsete": tr, "pursuit": pr}[kind]
    r = mod.rollout(rows, n, f, P, time_step, executed=True)
    K = len(np.atleast_2d(P))
    shifts = np.zeros(K, dtype=np.int64) if shifts is None else np.asarray(shifts, dtype=np.int64)
    out = compose(np.asarray(r["rows"], dtype=np.float64), [int(c) for c in r["counts"]], foot, np.asarray(rows_o, dtype=np.float64),
                  counts_o, foot if foot_o is None else foot_o, margin, shifts)
    out["rollout"] = r
    return out


# ---- the known-answer case -------------------------------------------------------------------------------------------
# A straight drive along x at 2 ft/s from the origin under the RAMSETE follower, two 1.5 ft squares.  The partner is parked
# (one row) beside the START row, its near edge KNOWN_G above the robot's upper edge and its front edge KNOWN_EPS ahead of
# the robot's rear edge: centre (-1.5 + eps, 1.5 + g).  Row 0's pose is the record's own start pose, so a record that starts
# dy to the left (towards the partner) has the clearance g - dy there, one subtraction of exactly posed corners: 1e-12 holds
# with room.  It is the rollout's minimum: one row later the robot has driven 0.02 ft, past the partner's front edge, and
# the distance is corner to corner, which grows with that gap faster than the follower's first turn back to the line
# swings the rear corner out (4.8e-5 ft at row 1, on this reference; with the partner squarely abeam, 0.029 ft by row 25).
KNOWN_G, KNOWN_EPS, KNOWN_DYS, KNOWN_N, KNOWN_SETTLE = 0.25, 0.001, (0.0, 0.1, 0.02), 100, 20
KNOWN_MARGIN = 0.2             # 0.25 clear, 0.15 below, 0.23 clear: one of three below


def known_case():
    """rows (n, 8), records (3, 8), the parked partner's rows (1, 1, 8) and counts, the expected clearances (3,)."""
    n = KNOWN_N
    rows = np.zeros((n, 8))
    t = np.arange(n) * DT
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 6] = t, 2.0 * t, 2.0, 2.0 * t
    P = np.tile(tr.NOMINAL, (3, 1))
    P[:, 1] = KNOWN_DYS
    P[:, 6] = 0.05
    partner = np.zeros((1, 1, 8))
    partner[0, 0, 6], partner[0, 0, 7] = -1.5 + KNOWN_EPS, 1.5 + KNOWN_G
    expect = np.array([KNOWN_G - dy for dy in KNOWN_DYS])
    return rows, P, partner, np.array([1], dtype=np.int32), expect


def crossing_case():
    """The same drive and a partner that drives down the line x = KNOWN_CROSS_X across the route at 2 ft/s, reaching y = 0
    at its row KNOWN_CROSS_ROW.  Started on time (shift 0) it crosses long after the robot has passed (the robot is parked
    at x = 1.98 by then: 0.08 ft clear); started KNOWN_CROSS_JITTER rows (negative: early) it is on the route at the instant
    the robot is there: a contact."""
    rows, P, _, _, _ = known_case()
    m = 2 * KNOWN_CROSS_ROW
    partner = np.zeros((1, m, 8))
    t = np.arange(m) * DT
    partner[0, :, 0], partner[0, :, 1], partner[0, :, 2] = t, 2.0 * t, 2.0
    partner[0, :, 4] = np.pi / 2                        # heading = -phi: driving towards -y
    partner[0, :, 6] = KNOWN_CROSS_X
    partner[0, :, 7] = 2.0 * (KNOWN_CROSS_ROW - np.arange(m)) * DT
    return rows, P[:1], partner, np.array([m], dtype=np.int32)


KNOWN_CROSS_X, KNOWN_CROSS_ROW = 0.4, 300             # the robot is at x = 0.4 at its row 20
KNOWN_CROSS_JITTER = 20 - KNOWN_CROSS_ROW


# ---- the partner routes and shifts of the GPU comparison --------------------------------------------------------------
def _line(p0, p1, n_at_p1, n, cap):
    """(cap, 8) rows of a straight drive at constant speed from p0 that passes p1 at row n_at_p1, n rows of it."""
    d = (np.asarray(p1) - np.asarray(p0)) / float(n_at_p1)
    r = np.arange(cap)
    rows = np.zeros((cap, 8))
    speed = float(np.hypot(*d)) / DT
    rows[:, 0], rows[:, 1], rows[:, 2] = r * DT, r * DT * speed, speed
    rows[:, 4] = -np.arctan2(d[1], d[0])
    rows[:, 6], rows[:, 7] = p0[0] + d[0] * r, p0[1] + d[1] * r
    rows[n:] = np.nan
    return rows


def live_routes(rows, counts):
    cap = rows.shape[1]
    return [b for b in range(len(rows)) if min(int(counts[b]), cap) >= 60 and not (rows[b, :min(int(counts[b]), cap), 2] < 0).any()]


def partners(rows, counts, seed, Bo=16, cap_o=CAP_O):
    """Side O for a layout case: (Bo, cap_o, 8) rows and (Bo, 2) counts (stride 2), Bo <= 16 a prefix of the 16.
      0      a slow straight drive of cap_o rows that starts beside a live route's row r1 (about the margin off its flank) and
             passes beside that route's last pose at its own row 400, its heading the route's at either place: parked at its
             start it is met early, at a row below the shift; started on time it reaches the route's end long after the
             rollout has stopped there, in the tail
      1      no rows (count 0): an invalid pair
      2      one row: a robot parked beside a row of a live route, about the margin off its flank
      3      count cap_o + 500 (clamped), a drive across the field from 9 ft outside it
      4      count -3: an invalid pair
      5      a NaN heading in one row
      5 .. 7   smooth random drives of 30 .. 200 rows among the routes
      8 ..   such drives 7 .. 12 ft away: the rows the bounding circles cull"""
    rng = np.random.default_rng(seed)
    cap = rows.shape[1]
    live = live_routes(rows, counts)
    out = np.full((16, cap_o, 8), np.nan)
    cnt = np.zeros((16, 2), dtype=np.int32)
    cnt[:, 1] = -9                                      # the stride's other column is never read
    b = int(rng.choice(live))
    n = min(int(counts[b]), cap)
    r1 = int(rng.integers(n // 4, n // 2))

    def beside(row, off, b=b):
        phi = -rows[b, row, 4]
        side = rng.choice([-1.0, 1.0])
        return np.array([rows[b, row, 6] - side * off * np.sin(phi), rows[b, row, 7] + side * off * np.cos(phi)])

    out[0] = _line(beside(r1, 1.5 + MARGIN + rng.uniform(-0.05, 0.1)), beside(n - 1, 1.5 + MARGIN + rng.uniform(-0.05, 0.1)), 400, cap_o, cap_o)
    cnt[0, 0] = cap_o
    out[0, :200, 4], out[0, 200:, 4] = rows[b, r1, 4], rows[b, n - 1, 4]      # square to the route where it passes: the gaps are the offsets'
    b2 =int(rng.choice(live))
    r2 = min(int(counts[b2]), cap) // 2
    out[2, 0] = rows[b2, r2]
    out[2, 0, 6:8] = beside(r2, 1.5 + MARGIN + rng.uniform(-0.05, 0.1), b2)
    cnt[2, 0] = 1
    far = rng.uniform(0, 2 * np.pi)
    out[3] = _line(9.0 * np.array([np.cos(far), np.sin(far)]), rng.uniform(-2, 2, 2), 350, cap_o, cap_o)
    cnt[3, 0] = cap_o + 500
    out[4] = _line(rng.uniform(-5, 5, 2), rng.uniform(-2, 2, 2), 100, 50, cap_o)
    cnt[4, 0] = -3
    m = rc.synth_rows(rng, 11, 200)
    for i in range(5, 16):
        k = int(rng.integers(30, 201))
        out[i, :k] = m[i - 5, :k]
        if i >= 8:
            away = rng.uniform(0, 2 * np.pi)
            out[i, :k, 6:8] += rng.uniform(7, 12) * np.array([np.cos(away), np.sin(away)])
        cnt[i, 0] = k
    out[5, int(cnt[5, 0]) // 2, 4] = np.nan
    return out[:Bo].copy(), cnt[:Bo].copy(), b


def shift_set(n_a, n_o=CAP_O):
    """The 8 distinct start shifts of a comparison, for the executed count n_a of the route partner 0 was laid against and
    partner 0's rows n_o: 0 (n_o + s - n_a about 600: the tail over many tiles); a negative shift beyond -n_o (the partner
    parked at its end throughout); a shift beyond n_a (the rollout parked before the partner moves); n_o + s - n_a = 1, 63,
    64, 65 (the tail across a block's boundary); and one that ends the partner's drive inside the rollout's."""
    return [0, -(n_o + 37), n_a + 60] + [n_a - n_o + d for d in (1, 63, 64, 65)] + [n_a - n_o - 40]


def layout_shifts(kind, K, B, b_ref, counts, mode):
    """(shift_rows, route_shift, rollout_shift) of one comparison.  ``mode``: "route" (d_route_shift alone: route b takes
    entry b mod 8 of the set), "rollout" (d_rollout_shift alone: rollout k takes entry k mod 8), "host" (shift_rows alone:
    entry (K + B) mod 8), "all" (the sums of "route", delivered as shift_rows = 7, rollout_shift = 5 for every k and the
    rest per route)."""
    S = np.array(shift_set(min(max(int(counts[b_ref]), 0), CAP) + SETTLE), dtype=np.int64)
    if mode == "route":
        return 0, S[np.arange(B) % 8].astype(np.int32), None
    if mode == "rollout":
        return 0, None, S[np.arange(K) % 8].astype(np.int32)
    if mode == "host":
        return int(S[(K + B) % 8]), None, None
    assert mode == "all"
    return 7, (S[np.arange(B) % 8] - 12).astype(np.int32), np.full(K, 5, dtype=np.int32)


def primary_mode(K):
    """The delivery whose sums the CPU test holds to bite: per rollout where a route has enough of them, else per route."""
    return "rollout" if K >= 8 else "route"


# (kind, K, B) -> the partner seed: the first of 1, 2, ... for which, on the reference alone, what
# test_rollout_conflicts_cpu.py's test_the_cases_bite asserts holds for Bo = 1, 3 and 16.
PARTNER_SEEDS = {("ramsete", 1, 300): 2, ("ramsete", 3, 100): 1, ("ramsete", 16, 20): 1, ("ramsete", 64, 6): 1, ("ramsete", 300, 3): 1,
                 ("pursuit", 3, 100): 1, ("pursuit", 16, 20): 1, ("pursuit", 300, 3): 18}
assert set(PARTNER_SEEDS) == {(kind, K, B) for kind, K, B, _ in LAYOUTS}


@functools.lru_cache(maxsize=None)
def layout_rollouts(kind, K, B):
    """The reference's executed rows of a layout case, once: per route the follower's reference dict."""
    rows, counts, P = layout_case(kind, K, B)
    mod = {"ramsete": tr, "pursuit": pr}[kind]
    f = ref_follower(kind)
    return [mod.rollout(rows[b], counts[b], f, P[b], DT, executed=True) for b in range(B)]


def layout_reference(kind, K, B, seed, mode=None):
    """Per route of a layout case ``compose``'s dict against the 16 partners of ``seed`` at the sums of ``mode`` (None: the
    primary one).  Pairs do not depend on each other, so the answer for Bo = 1 or 3 is the first 1 or 3 columns."""
    rows, counts, P = layout_case(kind, K, B)
    rows_o, counts_o, b_ref = partners(rows, counts, seed)
    s = sums(*layout_shifts(kind, K, B, b_ref, counts, mode or primary_mode(K)), B, K)
    ro = layout_rollouts(kind, K, B)
    return [compose(np.asarray(ro[b]["rows"], dtype=np.float64), [int(c) for c in ro[b]["counts"]], SQUARE, rows_o, counts_o[:, 0],
                    SQUARE, MARGIN, s[b]) for b in range(B)], s


def prefix(pair_clearance, pair_rows, Bo, margin=MARGIN):
    """One rollout's per-rollout outputs from the first Bo pairs of its (16,) pair outputs: conflict, conflict_rows (4,)."""
    best, other, row, ncon, first = np.inf, -1, -1, 0, -1
    for o in range(Bo):
        if pair_rows[o, 0] < 0:
            continue
        c = pair_clearance[o]
        if c < best:
            best, other, row = c, o, int(pair_rows[o, 0])
        ncon += int(c < margin)
        f = int(pair_rows[o, 1])
        if f >= 0 and (first < 0 or f < first):
            first = f
    return (best if other >= 0 else np.nan), np.array([other, row, ncon, first])


def bites(kind, K, B, seed):
    """Bo -> the counts test_the_cases_bite asserts on, from the reference alone at the primary delivery's sums: rollouts in
    contact, rollouts clear of the margin, routes whose rollouts are mixed (K = 1: min(conflicting, clear) routes), rollouts
    whose minimum falls in the tail (row >= n_a), rollouts whose minimum falls before the partner starts (row < s)."""
    per, s = layout_reference(kind, K, B, seed)
    n_a = np.array([[int(c) for c in r["counts"]] for r in layout_rollouts(kind, K, B)])
    out = {}
    for Bo in OTHERS:
        c, rows4 = np.full((B, K), np.nan), np.full((B, K, 4), -1)
        for b in range(B):
            for k in range(K):
                c[b, k], rows4[b, k] = prefix(per[b]["pair_clearance"][k], per[b]["pair_rows"][k], Bo)
        valid = rows4[..., 1] >= 0
        ncon, nval = (valid & (c < MARGIN)).sum(axis=1), valid.sum(axis=1)
        mixed = int(((ncon > 0) & (ncon < nval)).sum()) if K > 1 else int(min((ncon > 0).sum(), ((nval > 0) & (ncon == 0)).sum()))
        out[Bo] = dict(contact=int((valid & (c < 0)).sum()), clear=int((valid & (c > MARGIN)).sum()), mixed=mixed,
                       tail=int((valid & (rows4[..., 1] >= n_a)).sum()), before=int((valid & (rows4[..., 1] < s)).sum()))
    return out


# ---- the golden routes' partner ---------------------------------------------------------------------------------------
GOLDEN_JITTER = np.array([0, 0, 15, -15, 40, -40, 120, -120] * 2, dtype=np.int32)      # (16,) rollout shifts, 7 distinct


def mirrored(rows, counts):
    """The same routes mirrored in the line y = y0, 0.8 ft above the routes' highest point: (x, 2 y0 - y), heading and
    angular velocity negated.  Two 1.5 ft squares at that point at the same instant are 0.1 ft apart."""
    rows = np.array(rows, dtype=np.float64)
    n = [min(max(int(c), 0), rows.shape[1]) for c in counts]
    y0 = max(np.nanmax(rows[b, :n[b], 7]) for b in range(len(rows))) + 0.8
    rows[..., 7] = 2.0 * y0 - rows[..., 7]
    rows[..., 4], rows[..., 5] = -rows[..., 4], -rows[..., 5]
    return rows, np.array(n, dtype=np.int32)
