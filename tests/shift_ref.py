"""NumPy / plain-Python reference of the clearance over a window of start shifts (include/vap.h, vap_conflict_shifts),
written from its definitions on top of conflict_ref.relative_clearance.

The definition is stated twice.  Both read the pair's clearance matrix M[i][j] (A row i against O row j, every entry by
conflict_ref.relative_clearance), so they agree exactly or one of them is wrong:

  ``table_direct``  instant by instant in plain Python: t = min(0, s) .. max(n_a, n_o + s) - 1, i = t, j = t - s, each
                    index outside its rows either clamped (its hold bit set) or the instant dropped
  ``table_fast``    the examined instants of a shift are one interval of t; index arrays, one nanmin per shift

``scan`` is first / safe of a blocked mask; ``sweep`` every output of the call for two batches."""
import numpy as np

import conflict_ref as cr

A_FIRST, A_LAST, O_FIRST, O_LAST = 1, 2, 4, 8


def clearance_matrix(rows_a, n_a, foot_a, rows_o, n_o, foot_o):
    """M (n_a, n_o): the clearance between A's row i and O's row j."""
    a = np.asarray(rows_a, dtype=np.float64)[:n_a][:, [4, 6, 7]]
    o = np.asarray(rows_o, dtype=np.float64)[:n_o][:, [4, 6, 7]]
    ii, jj = np.meshgrid(np.arange(n_a), np.arange(n_o), indexing="ij")
    return cr.relative_clearance(a[ii.ravel()], o[jj.ravel()], foot_a, foot_o).reshape(n_a, n_o)


def examined(n_a, n_o, s, hold):
    """The (i, j) of every examined instant of a valid pair at shift s, in order of t."""
    out = []
    for t in range(min(0, s), max(n_a, n_o + s)):
        i, j = t, t - s
        if i < 0:
            if not hold & A_FIRST:
                continue
            i = 0
        if i >= n_a:
            if not hold & A_LAST:
                continue
            i = n_a - 1
        if j < 0:
            if not hold & O_FIRST:
                continue
            j = 0
        if j >= n_o:
            if not hold & O_LAST:
                continue
            j = n_o - 1
        out.append((i, j))
    return out


def table_direct(M, s, hold):
    best = None
    for i, j in examined(M.shape[0], M.shape[1], s, hold):
        v = M[i, j]
        if v == v and (best is None or v < best):
            best = v
    return np.nan if best is None else float(best)


def table_fast(M, shifts, hold):
    n_a, n_o = M.shape
    out = np.full(len(shifts), np.nan)
    for k, s in enumerate(shifts):
        s = int(s)
        tb, te = min(0, s), max(n_a, n_o + s)
        if not hold & A_FIRST:
            tb = max(tb, 0)
        if not hold & A_LAST:
            te = min(te, n_a)
        if not hold & O_FIRST:
            tb = max(tb, s)
        if not hold & O_LAST:
            te = min(te, n_o + s)
        if tb >= te:
            continue
        t = np.arange(tb, te)
        v = M[np.clip(t, 0, n_a - 1), np.clip(t - s, 0, n_o - 1)]
        v = v[~np.isnan(v)]
        if len(v):
            out[k] = v.min()
    return out


def scan(blocked, min_run, direction):
    """(first, safe) of a window of blocked flags: direction +1 the smallest k with k .. k + min_run - 1 inside the window
    and unblocked, -1 the largest k with k - min_run + 1 .. k so; -1 when there is none."""
    b = [bool(x) for x in blocked]
    n = len(b)
    if direction > 0:
        ok = [k for k in range(n) if k + min_run <= n and not any(b[k:k + min_run])]
    else:
        ok = [k for k in range(n) if k - min_run + 1 >= 0 and not any(b[k - min_run + 1:k + 1])]
    first = -1 if not ok else (ok[0] if direction > 0 else ok[-1])
    return first, n - sum(b)


def sweep(rows_a, counts_a, foot_a, rows_o, counts_o, foot_o=None, margin=0.0, shift_lo=0, n_shifts=1, shift_step=1, base=None,
          hold=14, matched=False, min_run=1, direction=1, matrices=None):
    """Every output of vap_conflict_shifts.  ``matrices``: an optional dict that keeps M per (ia, io) between calls on the
    same rows."""
    foot_o = foot_a if foot_o is None else foot_o
    rows_a, rows_o = np.asarray(rows_a, dtype=np.float64), np.asarray(rows_o, dtype=np.float64)
    Ba, Bo = len(rows_a), len(rows_o)
    assert not matched or Ba == Bo
    P = 1 if matched else Bo
    out = dict(pair_table=np.full((Ba, P, n_shifts), np.nan), pair_first=np.full((Ba, P), -1), pair_safe=np.zeros((Ba, P), dtype=int),
               route_table=np.full((Ba, n_shifts), np.nan), route_first=np.full(Ba, -1), route_safe=np.zeros(Ba, dtype=int))
    for ia in range(Ba):
        n_a = int(np.clip(counts_a[ia], 0, rows_a.shape[1]))
        if n_a == 0:
            continue
        s = shift_lo + (0 if base is None else int(base[ia])) + shift_step * np.arange(n_shifts)
        blocked = np.zeros(n_shifts, dtype=bool)
        for p in range(P):
            io = ia if matched else p
            n_o = int(np.clip(counts_o[io], 0, rows_o.shape[1]))
            if n_o == 0:
                continue
            key = (ia, io)
            if matrices is not None and key in matrices:
                M = matrices[key]
            else:
                M = clearance_matrix(rows_a[ia], n_a, foot_a, rows_o[io], n_o, foot_o)
                if matrices is not None:
                    matrices[key] = M
            tab = table_fast(M, s, hold)
            out["pair_table"][ia, p] = tab
            b = tab < margin                                   # NaN never blocks
            out["pair_first"][ia, p], out["pair_safe"][ia, p] = scan(b, min_run, direction)
            blocked |= b
            out["route_table"][ia] = np.fmin(out["route_table"][ia], tab)
        out["route_first"][ia], out["route_safe"][ia] = scan(blocked, min_run, direction)
    return out


def crossing(n=161):
    """The analytic case: 1 ft squares at heading 0; A drives along y = 0 and O along x = 0, 1/16 ft per row, both
    through the origin at row 80."""
    t = np.arange(n, dtype=np.float64)
    a, o = np.zeros((n, 8)), np.zeros((n, 8))
    a[:, 0] = o[:, 0] = 0.01 * t
    a[:, 6] = -5.0 + t / 16.0
    o[:, 7] = -5.0 + t / 16.0
    unit = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])
    return a, o, unit
