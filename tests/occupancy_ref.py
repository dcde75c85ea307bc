"""NumPy statement of vap_plan_occupancy and of vap_plan_seeds_occupied's free mask (include/vap.h): time-domain rows
posed as tests/footprint_ref.py poses them, the clearance of every cell centre of tests/plan_ref.py's grid against the
posed polygon by plan_ref's polygon formula, and per cell the first and last covering instant, the number of covering
rows and the smallest clearance.

``ftype`` = np.float64 does the device's IEEE operations in the device's order (sin and cos are NumPy's, which may differ
from the device's by an ulp); ``ftype`` = np.longdouble runs the same in extended precision: the difference of the two is
the reference's own rounding error.  ``gap`` is the smallest |clearance - margin| over EVERY (row, cell) pair: where it is
above 1e-9 no rounding can flip a covering decision, and first, last, count and blocked are exact."""
import numpy as np

import plan_ref as pr

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SQUARE = np.array([[-0.75, -0.75], [0.75, -0.75], [0.75, 0.75], [-0.75, 0.75]])   # footprint.rectangle(18, 18)
ROW_BLOCK = 32


def make_rows(x, y, heading, dt=0.01):
    """(n, 8) time-domain rows {time, position, velocity, acceleration, heading, angular_vel, x, y} from poses; the columns
    the occupancy does not read hold the time and zeros."""
    x, y, heading = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(heading, dtype=np.float64))
    rows = np.zeros((len(x), 8))
    rows[:, 0] = np.arange(len(x)) * dt
    rows[:, 4], rows[:, 6], rows[:, 7] = heading, x, y
    return rows


def pose(rows, footprint, ftype=np.float64):
    """(n, n_foot, 2): vertex v of the footprint at (x, y) + R(-heading) v."""
    r = np.asarray(rows, dtype=np.float64).astype(ftype)
    v = np.asarray(footprint, dtype=np.float64).astype(ftype)
    phi = -r[:, 4]
    c, s = np.cos(phi)[:, None], np.sin(phi)[:, None]
    x, y = r[:, 6][:, None], r[:, 7][:, None]
    return np.stack([x + (c * v[None, :, 0] - s * v[None, :, 1]), y + (s * v[None, :, 0] + c * v[None, :, 1])], axis=2)


def row_parts(P, px, py, ftype=np.float64):
    """(smax, d2), each (n, ny, nx): over the edges of each posed polygon P[r] the largest signed distance of the cell centres
    to an edge's line and the smallest squared point-to-segment distance (plan_ref.polygon_distance's two running values)."""
    n, m = P.shape[:2]
    px, py = px[None], py[None]
    smax = np.full((n,) + px.shape[1:], -np.inf, dtype=ftype)
    d2 = np.full(smax.shape, np.inf, dtype=ftype)
    for k in range(m):
        a, e = P[:, k], P[:, (k + 1) % m] - P[:, k]
        ax, ay, ex, ey = (t[:, None, None] for t in (a[:, 0], a[:, 1], e[:, 0], e[:, 1]))
        ll = ex * ex + ey * ey
        wx, wy = px - ax, py - ay
        smax = np.maximum(smax, (wx * ey - wy * ex) / np.sqrt(ll))
        t = np.minimum(np.maximum((wx * ex + wy * ey) * (ftype(1) / ll), ftype(0)), ftype(1))
        dx, dy = wx - t * ex, wy - t * ey
        d2 = np.minimum(d2, dx * dx + dy * dy)
    return smax, d2


def row_clearance(P, px, py, radius, ftype=np.float64):
    """(n, ny, nx): plan_ref.polygon_distance of the cell centres against each posed polygon P[r], minus radius."""
    smax, d2 = row_parts(P, px, py, ftype)
    return np.where(smax > 0, np.sqrt(d2), smax) - ftype(radius)


def taking_part(rows, footprint):
    """(n,) bool: the rows that take part.  A row with a non-finite pose covers nothing and is no part of the minimum; nor is a
    row whose pose is so large that a posed edge has a squared length of zero (or a non-finite one): the posed vertices are
    taken in fp64 as the device takes them, whatever precision the clearance then runs in."""
    r = np.asarray(rows, dtype=np.float64)
    keep = np.isfinite(r[:, [4, 6, 7]]).all(axis=1)
    with np.errstate(all="ignore"):
        V = pose(r, footprint)
        e = np.roll(V, -1, axis=1) - V
        ll = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
    return keep & ((ll > 0) & np.isfinite(ll)).all(axis=1)


def occupancy(rows, counts, footprint, field, cell, radius, margin=0.0, shift_rows=0, hold_first=False, hold_last=True,
              ftype=np.float64):
    """rows (B, capacity, 8) (or a list of (n_b, 8)), counts (B,) (None: every row).  Returns a dict: first, last, count
    (ny, nx) int64 with the header's never-covered values, min_clearance (ny, nx) ``ftype``, blocked (ny, nx) bool, gap (the
    smallest |clearance - margin| over every (row, cell) pair; +inf without rows), pairs (the number of such pairs)."""
    xs, ys = pr.centres(field, cell, ftype)
    px, py = np.meshgrid(xs, ys)
    shape = px.shape
    first = np.full(shape, INT_MAX, dtype=np.int64)
    last = np.full(shape, INT_MIN, dtype=np.int64)
    count = np.zeros(shape, dtype=np.int64)
    cmin = np.full(shape, np.inf, dtype=ftype)
    gap, pairs = np.inf, 0
    for b in range(len(rows)):
        r = np.asarray(rows[b], dtype=np.float64)
        n = len(r) if counts is None else int(min(max(int(counts[b]), 0), len(r)))
        r = r[:n]
        keep = taking_part(r, footprint)
        for k0 in range(0, n, ROW_BLOCK):
            idx = np.arange(k0, min(k0 + ROW_BLOCK, n))[keep[k0:k0 + ROW_BLOCK]]
            if not len(idx):
                continue
            c = row_clearance(pose(r[idx], footprint, ftype), px, py, radius, ftype)
            cov = c < ftype(margin)
            gap = min(gap, float(np.abs(c - ftype(margin)).min()))
            pairs += c.size
            cmin = np.minimum(cmin, c.min(axis=0))
            count += cov.sum(axis=0)
            inst = (idx + int(shift_rows))[:, None, None]
            lo = np.where(cov, inst, INT_MAX)
            hi = np.where(cov, inst, INT_MIN)
            if hold_first:
                lo = np.where(cov & (idx == 0)[:, None, None], INT_MIN, lo)
            if hold_last:
                hi = np.where(cov & (idx == n - 1)[:, None, None], INT_MAX, hi)
            first = np.minimum(first, lo.min(axis=0))
            last = np.maximum(last, hi.max(axis=0))
    return {"first": first, "last": last, "count": count, "min_clearance": cmin, "blocked": first <= last, "gap": gap, "pairs": pairs}


def window_free(free, first, last, window=None):
    """vap_plan_seeds_occupied's free mask of one problem: free in the static scene and not occupied at an instant of
    [t0, t1) — the window meets the hull [first, last] of the visits.  None: every instant."""
    t0, t1 = (INT_MIN, INT_MAX) if window is None else (int(window[0]), int(window[1]))
    occupied = (t0 < t1) & (np.asarray(first) < t1) & (np.asarray(last) >= t0)
    return np.asarray(free, dtype=bool) & ~occupied


def seeds(starts, goals, windows, field, cell, free, first, last, W=5, max_vertices=64, fields=None):
    """vap_plan_seeds_occupied for R problems on a static free mask: a list of plan_ref.plan dicts, and each problem's mask.
    ``fields``: plan_ref.plan's cache of distance fields by goal cell, for problems that all share ONE window."""
    out, masks = [], []
    for r, (s, g) in enumerate(zip(np.atleast_2d(starts), np.atleast_2d(goals))):
        m = window_free(free, first, last, None if windows is None else windows[r])
        masks.append(m)
        out.append(pr.plan(s, g, field, cell, m, W, max_vertices, fields))
    return out, masks


# The crossing scenario of the tests and of DESIGN.md section 16: on plan_ref's field of +-6 ft an 18 x 18 in partner drives north
# along x ~ 0 at 3 ft/s (10 ms rows); I go from (-4.5, -3) to (4.5, -3) as a disc of 0.75 ft wanting 0.1 ft of margin.
CROSSING = dict(field=pr.FIELD, cell=0.25, radius=0.75, margin=0.1, start=(-4.5, -3.0), goal=(4.5, -3.0), n_rows=217)


def crossing_rows(n=217):
    r = np.arange(n)
    return make_rows(np.full(n, 0.013), -5.0 + 0.007 + 0.03 * r, np.full(n, -(np.pi / 2 + 0.03)))
