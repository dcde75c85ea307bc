"""NumPy / plain-Python statement of the routine calls (vap_plan_travel, vap_plan_order, include/vap.h).

``order`` is the Held-Karp recurrence exactly as the header writes it: f[{j}][j] = c[0][j], f[S][j] the minimum over the
predecessors i in increasing order under a strict < of one fp64 addition, the last site ``end`` or the lowest j with the
smallest f[F][j], the order from the parents.  ``brute`` is what it must equal: the smallest left-to-right sum over all
admissible permutations.  ``travel`` builds the P x P matrix of ``plan_ref.plan`` dicts, one distance field per goal cell."""
import itertools

import numpy as np

import plan_ref as pr

INFEASIBLE = 512


def sanitise(cost):
    """NaN and -inf count as +inf."""
    c = np.array(cost, dtype=np.float64)
    c[np.isnan(c) | np.isneginf(c)] = np.inf
    return c


def masks_of(before, M):
    """before[k] for k = 0..M with entry 0 and bits >= M dropped."""
    if before is None:
        return [0] * (M + 1)
    return [0] + [int(before[k]) & ((1 << M) - 1) for k in range(1, M + 1)]


def order(cost, end=-1, before=None):
    """(order [M], total, flags) of one problem; cost (P, P), end -1 or 1..M, before (P,) masks or None."""
    c = sanitise(cost)
    M = c.shape[0] - 1
    bf = masks_of(before, M)
    full = (1 << M) - 1
    f = np.full((full + 1, M + 1), np.inf)
    par = np.zeros((full + 1, M + 1), dtype=np.int64)
    for S in sorted(range(1, full + 1), key=lambda s: bin(s).count("1")):
        for j in range(1, M + 1):
            if not S >> (j - 1) & 1:
                continue
            rest = S ^ (1 << (j - 1))
            if bf[j] & ~rest:
                continue
            if rest == 0:
                f[S, j] = c[0, j]
                continue
            best, bp = np.inf, 0
            for i in range(1, M + 1):
                if rest >> (i - 1) & 1:
                    v = f[rest, i] + c[i, j]
                    if v < best:
                        best, bp = v, i
            f[S, j], par[S, j] = best, bp
    last = end
    if end < 0:
        last = 1
        for j in range(2, M + 1):
            if f[full, j] < f[full, last]:
                last = j
    total = f[full, last]
    if total == np.inf:
        return [-1] * M, np.inf, INFEASIBLE
    out, S, j = [0] * M, full, last
    for k in range(M - 1, -1, -1):
        out[k] = j
        S, j = S ^ (1 << (j - 1)), int(par[S, j])
    return out, float(total), 0


def order_batch(costs, ends, befores=None):
    """``order`` for R problems at once, the same recurrence with NumPy over the problems: costs (R, P, P), befores (R, P) or
    None, ends a list of end values.  Returns {end: (orders (R, M), totals (R,), flags (R,))}; the table is built once."""
    c = sanitise(costs)
    R, M = c.shape[0], c.shape[1] - 1
    bf = np.zeros((R, M + 1), dtype=np.int64) if befores is None else np.asarray(befores, dtype=np.int64) & ((1 << M) - 1)
    full = (1 << M) - 1
    f = np.full((full + 1, M + 1, R), np.inf)
    par = np.zeros((full + 1, M + 1, R), dtype=np.int64)
    for S in sorted(range(1, full + 1), key=lambda s: bin(s).count("1")):
        for j in range(1, M + 1):
            if not S >> (j - 1) & 1:
                continue
            rest = S ^ (1 << (j - 1))
            ok = (bf[:, j] & ~rest) == 0
            if rest == 0:
                f[S, j] = np.where(ok, c[:, 0, j], np.inf)
                continue
            best, bp = np.full(R, np.inf), np.zeros(R, dtype=np.int64)
            for i in range(1, M + 1):
                if rest >> (i - 1) & 1:
                    v = f[rest, i] + c[:, i, j]
                    upd = v < best
                    best, bp = np.where(upd, v, best), np.where(upd, i, bp)
            f[S, j], par[S, j] = np.where(ok, best, np.inf), bp
    out = {}
    for end in ends:
        if end >= 0:
            last = np.full(R, end, dtype=np.int64)
        else:
            last = np.ones(R, dtype=np.int64)
            for j in range(2, M + 1):
                last = np.where(f[full, j] < f[full, last, np.arange(R)], j, last)
        total = f[full, last, np.arange(R)]
        orders = np.full((R, M), -1, dtype=np.int64)
        for r in np.flatnonzero(np.isfinite(total)):
            S, j = full, int(last[r])
            for k in range(M - 1, -1, -1):
                orders[r, k] = j
                S, j = S ^ (1 << (j - 1)), int(par[S, j, r])
        out[end] = (orders, total, np.where(np.isfinite(total), 0, INFEASIBLE))
    return out


def admissible(M, end=-1, before=None):
    """(n, M) int array of the permutations of 1..M that respect ``before`` and ``end``."""
    bf = masks_of(before, M)
    keep = []
    for p in itertools.permutations(range(1, M + 1)):
        if end >= 0 and p[-1] != end:
            continue
        seen, ok = 0, True
        for j in p:
            if bf[j] & ~seen:
                ok = False
                break
            seen |= 1 << (j - 1)
        if ok:
            keep.append(p)
    return np.array(keep, dtype=np.int64).reshape(len(keep), M)


def brute(cost, end=-1, before=None):
    """(smallest left-to-right sum c[0][o1] + c[o1][o2] + ... over the admissible permutations, those permutations, their
    sums); +inf without an admissible one."""
    c = sanitise(cost)
    M = c.shape[0] - 1
    perms = admissible(M, end, before)
    if len(perms) == 0:
        return np.inf, perms, np.zeros(0)
    s = c[0, perms[:, 0]]
    for k in range(1, M):
        s = s + c[perms[:, k - 1], perms[:, k]]                         # one fp64 addition per leg, in order
    return float(s.min()), perms, s


def tie_rule_order(perms, sums):
    """Among the cheapest permutations the one the two tie rules pick when every sum is exact (integer costs): the lowest
    last site, then the lowest site before it, and so on back."""
    best = perms[sums == sums.min()]
    return list(min(best, key=lambda p: tuple(p[::-1])))


def random_problem(rng, M, integer=False):
    """A cost matrix with +inf, NaN and -inf entries, precedence masks and an end, some of them infeasible."""
    P = M + 1
    c = rng.integers(1, 4, (P, P)).astype(np.float64) if integer else rng.uniform(0.1, 10.0, (P, P))
    kind = rng.integers(0, 4)
    if kind >= 1:
        c[rng.random((P, P)) < 0.15] = np.inf
    if kind == 2:
        c[rng.random((P, P)) < 0.05] = np.nan
    if kind == 3:
        c[rng.random((P, P)) < 0.05] = -np.inf
    before = np.zeros(P, dtype=np.uint32)
    if rng.random() < 0.6 and M > 1:
        for _ in range(int(rng.integers(1, M))):
            j, k = rng.integers(1, P, 2)
            if j != k or rng.random() < 0.05:                           # now and then a site before itself: a cycle
                before[k] |= np.uint32(1 << (j - 1))
    before[0] = np.uint32(rng.integers(0, 2 ** 16))                     # entry 0 and the bits >= M are ignored
    before[1:] |= np.uint32(int(rng.integers(0, 2 ** 8)) << M)
    end = int(rng.integers(1, P)) if rng.random() < 0.5 else -1
    return c, end, before


def travel(points, field, cell, free, W):
    """P x P ``plan_ref.plan`` dicts of one problem: entry [a][b] is start = point a, goal = point b, one field per goal
    cell; the diagonal is length 0, flags 0, n_vertices 0 and the point itself W times."""
    P = len(points)
    fields, out = {}, [[None] * P for _ in range(P)]
    for b in range(P):
        for a in range(P):
            if a == b:
                wp = np.repeat(np.asarray(points[b], dtype=np.float64)[None], W, axis=0)
                out[a][b] = {"flags": 0, "n_vertices": 0, "length": 0.0, "length_ld": np.longdouble(0), "waypoints": wp,
                             "waypoints_ld": wp.astype(np.longdouble), "pulled": [], "cells": []}
            else:
                out[a][b] = pr.plan(points[a], points[b], field, cell, free, W, fields=fields)
    return out


def stack(tr, key, dtype=np.float64):
    """The P x P array of one key of ``travel``'s dicts."""
    return np.array([[np.asarray(e[key], dtype=dtype) for e in row] for row in tr], dtype=dtype)


# A closed pocket on a 12 x 12 grid: four rectangles round the 2 x 2 cells at the origin; a ring of free cells outside.
POCKET = dict(field=(-1.5, -1.5, 1.5, 1.5), cell=0.25, radius=0.2, margin=0.05, circles=[],
              polygons=[np.array([[-0.75, -0.75], [0.75, -0.75], [0.75, -0.5], [-0.75, -0.5]]),
                        np.array([[-0.75, 0.5], [0.75, 0.5], [0.75, 0.75], [-0.75, 0.75]]),
                        np.array([[-0.75, -0.5], [-0.5, -0.5], [-0.5, 0.5], [-0.75, 0.5]]),
                        np.array([[0.5, -0.5], [0.75, -0.5], [0.75, 0.5], [0.5, 0.5]])])
POCKET_POINTS = np.array([[-1.125, -1.125], [0.125, 0.125], [1.125, 1.0], [-1.0, 1.125]])   # point 1 is inside
# One post on a 12 x 12 grid.
POST = dict(field=(-1.5, -1.5, 1.5, 1.5), cell=0.25, radius=0.2, margin=0.05, polygons=[], circles=[(0.0, 0.0, 0.3)])
# Scene C of plan_ref: five points, point 2 parked against the left wall (its cell is blocked: it is snapped).
POINTS_C = np.array([[-4.5, -3.0], [4.5, -3.0], [-5.9, -3.0], [2.0, 4.0], [-2.0, -4.5]])


def free_of(sc):
    """The free mask of a scene dict, after asserting that no cell lies within 1e-9 of the margin."""
    c = pr.clearance_grid(**pr.scene_args(sc))
    assert np.abs(c - sc["margin"]).min() >= 1e-9
    return c >= sc["margin"]
