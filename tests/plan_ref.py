"""NumPy + heapq statement of the grid planner (vap_plan_grid, vap_plan_seeds, include/vap.h): the clearance grid, the free
mask, the 8-connected distance field (a heap Dijkstra, and a Jacobi relaxation that must reach the same bits), snapping,
the trace, the line-of-sight pull and the equal-arc resample.

Everything an integer or a single IEEE addition decides (free mask given the clearance, distance field, trace, pull,
vertices) is exact in fp64.  The clearance, the length and the waypoints also run in ``ftype`` = np.longdouble: the
difference of the two is the reference's own rounding error."""
import heapq
import math

import numpy as np

MOVES = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
SQRT2 = 1.4142135623730951
MAX_CELLS = 16384
FLAG_DEGENERATE, FLAG_NOCONVERGE = 1, 4
SNAPPED_START, SNAPPED_GOAL, NO_FREE, UNREACHABLE, VERTICES_TRUNCATED = 16, 32, 64, 128, 256


def grid_shape(field, cell):
    """(nx, ny)."""
    return math.ceil((field[2] - field[0]) / cell), math.ceil((field[3] - field[1]) / cell)


def centres(field, cell, ftype=np.float64):
    """The cell centres xs (nx,), ys (ny,)."""
    nx, ny = grid_shape(field, cell)
    f, h = [ftype(v) for v in field], ftype(cell)
    return f[0] + (np.arange(nx).astype(ftype) + ftype(0.5)) * h, f[1] + (np.arange(ny).astype(ftype) + ftype(0.5)) * h


def cell_of(p, field, cell):
    """The cell (i, j) of a point, clamped to the grid."""
    nx, ny = grid_shape(field, cell)
    i = int(min(max(math.floor((p[0] - field[0]) / cell), 0), nx - 1))
    j = int(min(max(math.floor((p[1] - field[1]) / cell), 0), ny - 1))
    return i, j


def polygon_distance(px, py, poly, ftype=np.float64):
    """Signed distance of points to a convex counter-clockwise polygon: outside, the smallest point-to-segment distance;
    inside, the largest signed distance to an edge line (<= 0)."""
    P = np.asarray(poly, dtype=np.float64).astype(ftype)
    smax = np.full(px.shape, -np.inf, dtype=ftype)
    d2 = np.full(px.shape, np.inf, dtype=ftype)
    for k in range(len(P)):
        a, e = P[k], P[(k + 1) % len(P)] - P[k]
        ll = e[0] * e[0] + e[1] * e[1]
        wx, wy = px - a[0], py - a[1]
        smax = np.maximum(smax, (wx * e[1] - wy * e[0]) / np.sqrt(ll))
        t = np.minimum(np.maximum((wx * e[0] + wy * e[1]) * (ftype(1) / ll), ftype(0)), ftype(1))
        dx, dy = wx - t * e[0], wy - t * e[1]
        d2 = np.minimum(d2, dx * dx + dy * dy)
    return np.where(smax > 0, np.sqrt(d2), smax)


def clearance_grid(field, cell, polygons=(), circles=(), radius=0.0, ftype=np.float64):
    """(ny, nx): the disc's clearance at every cell centre."""
    xs, ys = centres(field, cell, ftype)
    px, py = np.meshgrid(xs, ys)
    f = [ftype(v) for v in field]
    v = np.minimum(np.minimum(px - f[0], f[2] - px), np.minimum(py - f[1], f[3] - py))
    for P in polygons:
        v = np.minimum(v, polygon_distance(px, py, P, ftype))
    for c in circles:
        cx, cy, r = [ftype(x) for x in c]
        dx, dy = px - cx, py - cy
        v = np.minimum(v, np.sqrt(dx * dx + dy * dy) - r)
    return v - ftype(radius)


def allowed(free, i, j, k):
    """Move k from free cell (i, j): the target is free and, for a diagonal, so are the two axis cells beside it."""
    ny, nx = free.shape
    di, dj = MOVES[k]
    a, b = i + di, j + dj
    if not (0 <= a < nx and 0 <= b < ny) or not free[b, a]:
        return False
    return bool(free[j, a] and free[b, i]) if di and dj else True


def weights(cell):
    return [cell] * 4 + [cell * SQRT2] * 4


def dijkstra(free, cell, goal):
    """d (ny, nx) from the goal cell (i, j): each value one chain of fp64 additions along a path."""
    d = np.full(free.shape, np.inf)
    if not free[goal[1], goal[0]]:
        return d
    w = weights(cell)
    d[goal[1], goal[0]] = 0.0
    pq = [(0.0, goal[0], goal[1])]
    while pq:
        dv, i, j = heapq.heappop(pq)
        if dv > d[j, i]:
            continue
        for k, (di, dj) in enumerate(MOVES):
            if allowed(free, i, j, k):
                nd = dv + w[k]
                if nd < d[j + dj, i + di]:
                    d[j + dj, i + di] = nd
                    heapq.heappush(pq, (nd, i + di, j + dj))
    return d


def jacobi(free, cell, goal, max_sweeps=None):
    """The same field by Jacobi sweeps (every cell from the previous sweep's values): (d, sweeps until nothing changed)."""
    ny, nx = free.shape
    w = weights(cell)
    big = np.zeros((ny + 2, nx + 2), dtype=bool)
    big[1:-1, 1:-1] = free
    ok = []
    for k, (di, dj) in enumerate(MOVES):
        m = big[1:-1, 1:-1] & big[1 + dj:ny + 1 + dj, 1 + di:nx + 1 + di]
        if di and dj:
            m = m & big[1:-1, 1 + di:nx + 1 + di] & big[1 + dj:ny + 1 + dj, 1:-1]
        ok.append(m)
    d = np.full((ny, nx), np.inf)
    if free[goal[1], goal[0]]:
        d[goal[1], goal[0]] = 0.0
    sweeps = 0
    while max_sweeps is None or sweeps < max_sweeps:
        sweeps += 1
        pad = np.full((ny + 2, nx + 2), np.inf)
        pad[1:-1, 1:-1] = d
        new = d.copy()
        for k, (di, dj) in enumerate(MOVES):
            cand = np.where(ok[k], pad[1 + dj:ny + 1 + dj, 1 + di:nx + 1 + di] + w[k], np.inf)
            new = np.minimum(new, cand)
        if np.array_equal(new, d):
            return d, sweeps
        d = new
    return d, sweeps


def nearest_free(free, p, field, cell):
    """The free cell (i, j) nearest to p by dx dx + dy dy to its centre, the lowest j * nx + i on a tie; None without one."""
    if not free.any():
        return None
    xs, ys = centres(field, cell)
    dx, dy = xs[None, :] - p[0], ys[:, None] - p[1]
    d2 = np.where(free, dx * dx + dy * dy, np.inf)
    k = int(np.argmin(d2.reshape(-1)))
    return k % free.shape[1], k // free.shape[1]


def trace(free, d, cell, start):
    """The cells from start to the goal: always the allowed neighbour with the smallest d[u] + w, the first on a tie."""
    w = weights(cell)
    i, j = start
    path = [(i, j)]
    while d[j, i] > 0 and len(path) < free.size:
        best = None
        for k, (di, dj) in enumerate(MOVES):
            if allowed(free, i, j, k):
                c = d[j + dj, i + di] + w[k]
                if best is None or c < best[0]:
                    best = (c, i + di, j + dj)
        if best is None:
            break
        _, i, j = best
        path.append((i, j))
    return path


def visible(free, a, b):
    """Every cell of the bounding box of a and b on the supercover of the segment between their centres is free."""
    (i0, j0), (i1, j1) = a, b
    dx, dy = i1 - i0, j1 - j0
    jj, ii = np.mgrid[min(j0, j1):max(j0, j1) + 1, min(i0, i1):max(i0, i1) + 1]
    on = 2 * np.abs((ii - i0) * dy - (jj - j0) * dx) <= abs(dx) + abs(dy)
    return bool(free[jj[on], ii[on]].all())


def pull(free, path):
    out, a = [path[0]], 0
    while a < len(path) - 1:
        b = len(path) - 1
        while b > a + 1 and not visible(free, path[a], path[b]):
            b -= 1
        out.append(path[b])
        a = b
    return out


def vertices_of(pulled, start, goal, field, cell, ftype=np.float64):
    """(nv, 2): the start, the centres of the pulled cells between, the goal."""
    xs, ys = centres(field, cell, ftype)
    v = [[xs[i], ys[j]] for i, j in pulled]
    if len(v) < 2:
        v = [None, None]
    v[0], v[-1] = [ftype(start[0]), ftype(start[1])], [ftype(goal[0]), ftype(goal[1])]
    return np.array(v, dtype=ftype)


def resample(v, W, ftype=np.float64):
    """(waypoints (W, 2), length): equal arcs along the polyline v; the ends are v's own ends."""
    v = np.asarray(v, dtype=ftype)
    e = v[1:] - v[:-1]
    l = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    c = [ftype(0)]
    for x in l:
        c.append(c[-1] + x)
    L = c[-1]
    out = np.empty((W, 2), dtype=ftype)
    out[0], out[-1] = v[0], v[-1]
    for k in range(1, W - 1):
        s = (ftype(k) * L) / ftype(W - 1)
        out[k] = v[-1]
        for m in range(len(l)):
            if c[m + 1] >= s and l[m] > 0:
                out[k] = v[m] + ((s - c[m]) / l[m]) * e[m]
                break
    return out, L


def plan(start, goal, field, cell, free, W, max_vertices=64, fields=None):
    """One problem on a free mask.  Returns a dict: flags, n_vertices, vertices (max_vertices, 2) (NaN behind the last),
    distance (ny, nx) or None, waypoints (W, 2), length, and waypoints_ld, length_ld in np.longdouble from the same
    vertices.  ``fields``: a dict that caches distance fields by goal cell."""
    nanw = np.full((W, 2), np.nan)
    res = {"flags": 0, "n_vertices": 0, "vertices": np.full((max_vertices, 2), np.nan), "distance": None, "waypoints": nanw,
           "length": np.inf, "waypoints_ld": nanw.astype(np.longdouble), "length_ld": np.longdouble(np.inf), "cells": [],
           "pulled": []}
    if not np.isfinite([start[0], start[1], goal[0], goal[1]]).all():
        res["flags"] |= FLAG_DEGENERATE
        return res
    if not free.any():
        res["flags"] |= NO_FREE
        return res
    g = cell_of(goal, field, cell)
    if not free[g[1], g[0]]:
        g = nearest_free(free, goal, field, cell)
        res["flags"] |= SNAPPED_GOAL
    s = cell_of(start, field, cell)
    if not free[s[1], s[0]]:
        s = nearest_free(free, start, field, cell)
        res["flags"] |= SNAPPED_START
    if fields is not None and g in fields:
        d = fields[g]
    else:
        d = dijkstra(free, cell, g)
        if fields is not None:
            fields[g] = d
    res["distance"] = d
    if not np.isfinite(d[s[1], s[0]]):
        res["flags"] |= UNREACHABLE
        return res
    res["cells"] = trace(free, d, cell, s)
    res["pulled"] = pull(free, res["cells"])
    v = vertices_of(res["pulled"], start, goal, field, cell)
    res["n_vertices"] = len(v)
    res["vertices"][:min(len(v), max_vertices)] = v[:max_vertices]
    if len(v) > max_vertices:
        res["flags"] |= VERTICES_TRUNCATED
    res["waypoints"], res["length"] = resample(v, W)
    vl = vertices_of(res["pulled"], start, goal, field, cell, np.longdouble)
    res["waypoints_ld"], res["length_ld"] = resample(vl, W, np.longdouble)
    return res


def seeds(starts, goals, field, cell, polygons=(), circles=(), radius=0.0, margin=0.0, W=5, max_vertices=64):
    """vap_plan_seeds for R problems: a list of ``plan`` dicts, and the free mask."""
    free = clearance_grid(field, cell, polygons, circles, radius) >= margin
    fields = {}
    return [plan(s, g, field, cell, free, W, max_vertices, fields) for s, g in zip(np.atleast_2d(starts), np.atleast_2d(goals))], free


# The two scenes of the tests and of DESIGN.md (a field of +-6 ft, rho = 0.75 ft, margin 0.1 ft, cell 0.25 ft: 48 x 48).
FIELD = (-6.0, -6.0, 6.0, 6.0)
SCENE_B = dict(field=FIELD, polygons=[], circles=[(0.0, 0.0, 0.5)], radius=0.75, margin=0.1, cell=0.25,
               start=(-4.0, 0.0), goal=(4.0, 0.0))
SCENE_C = dict(field=FIELD, polygons=[np.array([[-0.5, -6.0], [0.5, -6.0], [0.5, 2.0], [-0.5, 2.0]]),
                                      np.array([[2.0, -1.0], [4.0, -0.5], [2.5, 1.0]])],
               circles=[(-3.0, 0.5, 0.6)], radius=0.75, margin=0.1, cell=0.25, start=(-4.5, -3.0), goal=(4.5, -3.0))


def scene_args(sc, **over):
    """The keyword arguments of ``clearance_grid`` / ``seeds`` from a scene dict."""
    d = {k: sc[k] for k in ("field", "cell", "polygons", "circles", "radius")}
    d.update(over)
    return d
