"""Plain Python / NumPy statement of vap_plan_order_timed (include/vap.h): a routine's visiting order by the clock, in the
integer rows of its timeline.  Imports nothing from the package.  The turn, the dwell and the usable-row rule are
tests/timeline_ref.py's own (wrap_delta, turn_shape, dwell_steps, _usable), not restated.

Two statements of the same definitions: ``solve(..., method="brute")`` enumerates every subset and permutation and applies
the tie rules as one sort key; ``method="dp"`` is Held-Karp over (site set, last site, site before it) with the lowest
parent under a strict <.  Everything compared is an integer or an fp64 sum formed in a stated order."""
import itertools
import math

import numpy as np

import timeline_ref as tr

INFEASIBLE = 512
INT_MAX = tr.INT_MAX
MAX_SITES = 8


class Problem:
    """One problem r: n, hf, hl per (a, b) (n = 0: forbidden), the dwell rows, the start heading, values, masks, end, budget."""

    def __init__(self, rows, counts, leg, constraints, dt, turn_min, dwell, start_heading, value, budget, end, before, leg_flags):
        P = leg.shape[0]
        L, cap = rows.shape[0], rows.shape[1]
        self.P, self.M = P, P - 1
        self.cons, self.dt, self.turn_min = constraints, dt, turn_min
        self.n = np.zeros((P, P), dtype=np.int64)
        self.hf, self.hl = np.zeros((P, P)), np.zeros((P, P))
        for a in range(P):
            for b in range(1, P):
                li = int(leg[a, b])
                if a == b or li < 0 or li >= L or (leg_flags is not None and int(leg_flags[li]) != 0):
                    continue
                c = min(int(counts[li]), cap)
                if c <= 0:
                    continue
                first, last = rows[li, 0], rows[li, c - 1]
                if all(tr._usable(float(x[4])) and math.isfinite(x[6]) and math.isfinite(x[7]) for x in (first, last)):
                    self.n[a, b], self.hf[a, b], self.hl[a, b] = c, float(first[4]), float(last[4])
        self.w = [0] + [tr.dwell_steps(float(dwell[j]), dt) if dwell is not None else 0 for j in range(1, P)]
        self.h0 = float("nan") if start_heading is None else float(start_heading)
        self.bad_start = not (math.isnan(self.h0) or tr._usable(self.h0))
        self.val = [0.0] * P
        for j in range(1, P):
            x = 1.0 if value is None else float(value[j])
            self.val[j] = x if (x >= 0.0 and math.isfinite(x)) else 0.0
        self.before = [0] * P
        if before is not None:
            self.before = [int(before[k]) & ((1 << self.M) - 1) for k in range(P)]
        self.end = -1 if end is None else int(end)
        self.budget = None if budget is None else max(int(budget), 0)
        self._turn = {}

    def turn(self, h_front, h_first):
        """Rows of the turn in front of a leg: the timeline's rule."""
        if math.isnan(h_front):
            return 0
        key = (h_front, h_first)
        if key not in self._turn:
            d = tr.wrap_delta(h_first - h_front)
            self._turn[key] = 0 if abs(d) < self.turn_min else tr.turn_shape(-d, self.cons[0], self.cons[1], self.cons[5], self.dt)[3]
        return self._turn[key]

    def value_of(self, S):
        v = 0.0
        for j in range(1, self.P):
            if S >> (j - 1) & 1:
                v = v + self.val[j]
        return v

    def sequence(self, seq):
        """(rows, arrivals) of the sequence of sites, or None if it is not admissible (the budget is not looked at)."""
        if self.bad_start or (self.end >= 1 and (not seq or seq[-1] != self.end)):
            return None
        total, h, prev, seen, arrivals = 0, self.h0, 0, 0, []
        for s in seq:
            if self.n[prev, s] <= 0 or self.before[s] & ~seen:
                return None
            total += self.turn(h, float(self.hf[prev, s])) + int(self.n[prev, s])
            arrivals.append(total)
            total += self.w[s]
            h, prev, seen = float(self.hl[prev, s]), s, seen | 1 << (s - 1)
        return (total, arrivals) if total < INT_MAX else None


def _set_of(seq):
    S = 0
    for s in seq:
        S |= 1 << (s - 1)
    return S


def brute(p):
    """The best sequence by enumeration: (seq, rows, arrivals, value) or None."""
    best = None
    sizes = [p.M] if p.budget is None else range(0, p.M + 1)
    for k in sizes:
        for seq in itertools.permutations(range(1, p.P), k):
            got = p.sequence(seq)
            if got is None or (p.budget is not None and got[0] > p.budget):
                continue
            S = _set_of(seq)
            value = p.value_of(S)
            key = ((-value, got[0], S) if p.budget is not None else (got[0],)) + (tuple(reversed(seq)),)
            if best is None or key < best[0]:
                best = (key, seq, got[0], got[1], value)
    return None if best is None else best[1:]


def held_karp(p):
    """The same by the table: g[(S, j, i)] the fewest rows over S standing on j having come from i (i = 0: the start)."""
    M, P = p.M, p.P
    g, par = {}, {}
    if not p.bad_start:
        for j in range(1, P):
            if p.n[0, j] > 0 and p.before[j] == 0:
                v = p.turn(p.h0, float(p.hf[0, j])) + int(p.n[0, j]) + p.w[j]
                if v < INT_MAX:
                    g[(1 << (j - 1), j, 0)] = v
    by_size = sorted(range(1, 1 << M), key=lambda S: bin(S).count("1"))
    for S in by_size:
        sites = [j for j in range(1, P) if S >> (j - 1) & 1]
        if len(sites) < 2:
            continue
        for j in sites:
            rest = S ^ 1 << (j - 1)
            if p.before[j] & ~rest:
                continue
            for i in sites:
                if i == j or p.n[i, j] <= 0:
                    continue
                best, bp = None, None
                for h in ([0] if rest == 1 << (i - 1) else [x for x in sites if x not in (i, j)]):
                    base = g.get((rest, i, h))
                    if base is None:
                        continue
                    v = base + p.turn(float(p.hl[h, i]), float(p.hf[i, j])) + int(p.n[i, j]) + p.w[j]
                    if v < INT_MAX and (best is None or v < best):
                        best, bp = v, h
                if best is not None:
                    g[(S, j, i)], par[(S, j, i)] = best, bp
    full = (1 << M) - 1
    win = None
    if p.budget is not None and p.end < 1 and not p.bad_start:
        win = ((-0.0, 0, 0, 0, 0), None)
    for (S, j, i), rows in g.items():
        if p.end >= 1 and j != p.end:
            continue
        if p.budget is None:
            if S != full:
                continue
            key = (0.0, rows, S, j, i)
        else:
            if rows > p.budget:
                continue
            key = (-p.value_of(S), rows, S, j, i)
        if win is None or key < win[0]:
            win = (key, (S, j, i))
    if win is None:
        return None
    if win[1] is None:
        return (), 0, [], 0.0
    S, j, i = win[1]
    total, value = g[(S, j, i)], p.value_of(S)
    seq, arrivals = [], []
    while True:
        seq.append(j)
        arrivals.append(g[(S, j, i)] - p.w[j])
        if i == 0:
            break
        h = par[(S, j, i)]
        S, j, i = S ^ 1 << (j - 1), i, h
    return tuple(reversed(seq)), total, list(reversed(arrivals)), value


def solve(rows, counts, leg, constraints, dt=0.01, turn_min=math.radians(1.0), dwell=None, start_heading=None, value=None,
          budget_rows=None, end=None, before=None, leg_flags=None, method="brute"):
    """rows (L, cap, 8), counts (L,) or (L, k), leg (R, P, P) -> dict of order (R, M), n_visited (R,), rows_total (R,),
    arrival_rows (R, M), value_total (R,), flags (R,), as the header states the outputs.  dwell, value, before (R, P);
    start_heading, budget_rows (R,)."""
    rows = np.asarray(rows, dtype=np.float64)
    counts = np.asarray(counts).reshape(len(rows), -1)[:, 0].astype(np.int64) if len(rows) else np.zeros(0, dtype=np.int64)
    leg = np.asarray(leg, dtype=np.int64)
    R, P = leg.shape[0], leg.shape[1]
    M = P - 1
    assert 1 <= M <= MAX_SITES
    out = {"order": np.full((R, M), -1, dtype=np.int32), "n_visited": np.zeros(R, dtype=np.int32),
           "rows_total": np.full(R, -1, dtype=np.int32), "arrival_rows": np.full((R, M), -1, dtype=np.int32),
           "value_total": np.full(R, np.nan), "flags": np.zeros(R, dtype=np.uint32)}
    for r in range(R):
        p = Problem(rows, counts, leg[r], constraints, dt, turn_min, None if dwell is None else dwell[r],
                    None if start_heading is None else start_heading[r], None if value is None else value[r],
                    None if budget_rows is None else budget_rows[r], end, None if before is None else before[r], leg_flags)
        got = brute(p) if method == "brute" else held_karp(p)
        if got is None:
            out["flags"][r] = INFEASIBLE
            continue
        seq, total, arrivals, val = got
        k = len(seq)
        out["order"][r, :k], out["arrival_rows"][r, :k] = seq, arrivals
        out["n_visited"][r], out["rows_total"][r], out["value_total"][r] = k, total, val
    return out


def budget_rows(budget, dt):
    """Seconds to rows: int(budget / dt) saturating, negative or NaN as given by the comparison (0 rows)."""
    q = float(budget) / dt
    if not q > 0:
        return 0
    return int(q) if q < float(INT_MAX) else INT_MAX
