"""NumPy / plain-Python reference of a routine's wait schedule (include/vap.h, vap_schedule_tables / vap_schedule_solve),
written from the definitions on top of shift_ref.clearance_matrix.

  ``segments``  the used slots of a slot map and whether they are a legal cut of the routine's rows
  ``tables``    move and wait, instant by instant in plain Python
  ``solve``     the boolean recurrence over (slot, cumulative delay) and its backtrack
  ``brute``     every delay vector of the window, the tie-break as a sort key: what ``solve`` must equal
"""
import itertools

import numpy as np

import shift_ref as sr


def segments(seg_start, n):
    """(S, [b_0 .. b_S], bad) of one routine with n rows.  n == 0 or S == 0: (0, [], False)."""
    seg_start = [int(x) for x in seg_start]
    used = [x >= 0 for x in seg_start]
    S = sum(used)
    if n == 0 or S == 0:
        return 0, [], False
    b = seg_start[:S]
    bad = not all(used[:S]) or b[0] != 0 or any(b[m] <= b[m - 1] for m in range(1, S)) or not b[-1] < n
    if bad:
        return 0, [], True
    return S, b + [n], False


def _fold(best, v):
    return v if v == v and (best is None or v < best) else best


def tables(rows_a, n, seg_start, foot_a, rows_o, counts_o, foot_o, C, q, matrices=None, key=None):
    """(move (M, C), wait (M, C), n_seg, bad) of one routine against every partner.  ``matrices`` / ``key``: an optional dict
    that keeps the clearance matrices between calls on the same rows."""
    M = len(seg_start)
    move, wait = np.full((M, C), np.nan), np.full((M, C), np.nan)
    n = int(np.clip(n, 0, len(rows_a)))
    S, b, bad = segments(seg_start, n)
    if S == 0:
        return move, wait, 0, bad
    mats = []
    for p in range(len(rows_o)):
        n_o = int(np.clip(counts_o[p], 0, rows_o.shape[1]))
        if n_o == 0:
            continue
        k_ = (key, p)
        if matrices is not None and k_ in matrices:
            mats.append(matrices[k_])
        else:
            mats.append(sr.clearance_matrix(rows_a, n, foot_a, rows_o[p], n_o, foot_o))
            if matrices is not None:
                matrices[k_] = mats[-1]
    for m in range(S):
        hold = max(b[m] - 1, 0)
        for k in range(C):
            best = None
            for Mx in mats:
                n_o = Mx.shape[1]
                for i in range(b[m], b[m + 1]):
                    best = _fold(best, Mx[i, min(i + k * q, n_o - 1)])
                if m == S - 1:
                    for t in range(n + k * q, n_o):
                        best = _fold(best, Mx[n - 1, t])
            move[m, k] = np.nan if best is None else best
            best = None
            for Mx in mats:
                n_o = Mx.shape[1]
                for t in range(b[m] + k * q, b[m] + (k + 1) * q):
                    best = _fold(best, Mx[hold, min(t, n_o - 1)])
            wait[m, k] = np.nan if best is None else best
    return move, wait, S, bad


def _result(ks, move, wait, S, q):
    M = move.shape[0]
    if ks is None:
        return [-1] * M, -1, float("nan")
    d, best, prev = [0] * M, None, 0
    for m in range(S):
        d[m] = (ks[m] - prev) * q
        best = _fold(best, move[m, ks[m]])
        for u in range(prev, ks[m]):
            best = _fold(best, wait[m, u])
        prev = ks[m]
    return d, ks[S - 1] * q, float("nan") if best is None else float(best)


def solve(move, wait, S, margin, q=1):
    """(delay_rows [M], total_rows, clearance) by the recurrence G_m[k] = F_{m-1}[k] or (G_m[k-1] and ok(wait[m][k-1])),
    F_m[k] = ok(move[m][k]) and G_m[k], F_{-1} = {0}."""
    move, wait = np.asarray(move, dtype=np.float64), np.asarray(wait, dtype=np.float64)
    M, C = move.shape
    S = int(np.clip(S, 0, M))
    if S == 0:
        return _result(None, move, wait, S, q)
    ok = lambda v: not (v < margin)
    F = []
    prev = [k == 0 for k in range(C)]
    for m in range(S):
        G = [False] * C
        for k in range(C):
            G[k] = prev[k] or (k > 0 and G[k - 1] and ok(wait[m, k - 1]))
        prev = [ok(move[m, k]) and G[k] for k in range(C)]
        F.append(prev)
    ends = [k for k in range(C) if F[S - 1][k]]
    if not ends:
        return _result(None, move, wait, S, q)
    ks = [0] * S
    ks[S - 1] = ends[0]
    for m in range(S - 1, 0, -1):
        k = ks[m]
        while not (F[m - 1][k] and all(ok(wait[m, u]) for u in range(k, ks[m]))):
            k -= 1
        ks[m - 1] = k
    return _result(ks, move, wait, S, q)


def brute(move, wait, S, margin, q=1):
    """The same by enumeration of every 0 <= k_0 <= .. <= k_{S-1} < C."""
    move, wait = np.asarray(move, dtype=np.float64), np.asarray(wait, dtype=np.float64)
    M, C = move.shape
    S = int(np.clip(S, 0, M))
    if S == 0:
        return _result(None, move, wait, S, q)
    ok = lambda v: not (v < margin)
    valid = []
    for ks in itertools.combinations_with_replacement(range(C), S):
        prev, good = 0, True
        for m in range(S):
            good = ok(move[m, ks[m]]) and all(ok(wait[m, u]) for u in range(prev, ks[m]))
            if not good:
                break
            prev = ks[m]
        if good:
            valid.append(ks)
    if not valid:
        return _result(None, move, wait, S, q)
    # the smallest k_{S-1}; then the largest k_{S-2}, then the largest k_{S-3}, ...
    valid.sort(key=lambda ks: (ks[S - 1],) + tuple(-ks[m] for m in range(S - 2, -1, -1)))
    return _result(list(valid[0]), move, wait, S, q)


def composed_tables(table_of, n, seg_start, C, q):
    """move and wait of one routine as a composition of shift tables.  ``table_of(lo, hi, shifts, hold)`` returns, per
    shift, the smallest shift-table entry over the partners of the routine's rows [lo, hi) taken as a route of their own
    (NaN ignored; NaN when there is none)."""
    M = len(seg_start)
    move, wait = np.full((M, C), np.nan), np.full((M, C), np.nan)
    S, b, bad = segments(seg_start, n)
    for m in range(S):
        move[m] = table_of(b[m], b[m + 1], [-(b[m] + k * q) for k in range(C)], 14 if m == S - 1 else 12)
        h = max(b[m] - 1, 0)
        w = np.asarray(table_of(h, h + 1, [-(b[m] + j) for j in range(C * q)], 12), dtype=np.float64).reshape(C, q)
        with np.errstate(all="ignore"):
            wait[m] = np.where(np.isnan(w).all(axis=1), np.nan, np.nanmin(np.where(np.isnan(w), np.inf, w), axis=1))
    return move, wait, S, bad
