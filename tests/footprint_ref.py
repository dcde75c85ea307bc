"""Brute-force NumPy reference of the footprint clearance (include/vap.h, vap_footprint_clearance), written from its
definitions: every element is tested exactly at every row (no culling), vectorised over rows.

  pose      phi = -heading; a body point v sits at (x, y) + R(phi) v
  wall      min over footprint vertices of min(p.x - xmin, xmax - p.x, p.y - ymin, ymax - p.y)
  polygon   separated: Euclidean distance (min of vertex-to-edge distances both ways); overlapping: minus the smallest
            overlap of the projections over the edge normals of both polygons
  circle    signed distance from the centre to the footprint (positive outside) minus r
Element ids: wall -1, polygons 0..P-1, circles P..P+C-1; ties go to the smallest id."""
import numpy as np


def posed(foot, heading, x, y, ftype=np.float64):
    """(N, n, 2) footprint vertices at N poses."""
    phi = -np.asarray(heading, dtype=ftype)
    c, s = np.cos(phi)[:, None], np.sin(phi)[:, None]
    foot = np.asarray(foot, dtype=ftype)
    fx, fy = foot[None, :, 0], foot[None, :, 1]
    x, y = np.asarray(x, dtype=ftype), np.asarray(y, dtype=ftype)
    return np.stack([x[:, None] + (c * fx - s * fy), y[:, None] + (s * fx + c * fy)], axis=-1)


def edge_normals(P, ftype=np.float64):
    """Outward unit normals (..., n, 2) of the edges v_i -> v_{i+1} of counter-clockwise polygons (..., n, 2)."""
    P = np.asarray(P, dtype=ftype)
    e = np.roll(P, -1, axis=-2) - P
    n = np.stack([e[..., 1], -e[..., 0]], axis=-1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def point_segment_dist(p, a, b, ftype=np.float64):
    """|p - segment(a, b)| with broadcasting over the leading axes."""
    p, a, b = np.asarray(p, dtype=ftype), np.asarray(a, dtype=ftype), np.asarray(b, dtype=ftype)
    e = b - a
    w = p - a
    t = np.clip(np.sum(w * e, axis=-1) / np.sum(e * e, axis=-1), 0.0, 1.0)
    d = w - t[..., None] * e
    return np.sqrt(np.sum(d * d, axis=-1))


def wall_clearance(P, field, ftype=np.float64):
    xmin, ymin, xmax, ymax = np.asarray(field, dtype=ftype)
    P = np.asarray(P, dtype=ftype)
    px, py = P[..., 0], P[..., 1]
    return np.min(np.minimum(np.minimum(px - xmin, xmax - px), np.minimum(py - ymin, ymax - py)), axis=-1)


def polygon_clearance(P, Q, ftype=np.float64):
    """P (N, n, 2) posed footprints, Q (m, 2) one convex polygon -> (N,)."""
    P, Q = np.asarray(P, dtype=ftype), np.asarray(Q, dtype=ftype)
    N = P.shape[0]
    QN = np.broadcast_to(Q, (N,) + Q.shape)
    axes = np.concatenate([edge_normals(P, ftype), np.broadcast_to(edge_normals(Q, ftype), (N,) + Q.shape)], axis=1)   # (N, A, 2)
    pp = np.einsum("nak,nvk->nav", axes, P)
    pq = np.einsum("nak,nvk->nav", axes, QN)
    ov = np.minimum(pp.max(-1), pq.max(-1)) - np.maximum(pp.min(-1), pq.min(-1))
    sep = ov.min(axis=1)
    # footprint vertices against polygon edges, polygon vertices against footprint edges
    d1 = point_segment_dist(P[:, :, None, :], QN[:, None, :, :], np.roll(QN, -1, axis=1)[:, None, :, :], ftype).min(axis=(1, 2))
    d2 = point_segment_dist(QN[:, :, None, :], P[:, None, :, :], np.roll(P, -1, axis=1)[:, None, :, :], ftype).min(axis=(1, 2))
    return np.where(sep > 0, -sep, np.minimum(d1, d2))


def circle_clearance(P, cx, cy, r, ftype=np.float64):
    P = np.asarray(P, dtype=ftype)
    q = np.array([cx, cy], dtype=ftype)[None, None, :]
    side = np.sum(edge_normals(P, ftype) * (q - P), axis=-1).max(axis=1)          # > 0: outside
    dist = point_segment_dist(q, P, np.roll(P, -1, axis=1), ftype).min(axis=1)
    return np.where(side > 0, dist, side) - ftype(r)


def element_clearances(rows, foot, field=None, polygons=(), circles=(), ftype=np.float64):
    """(N, 1 + P + C) clearances of N rows (columns: wall or +inf, polygons, circles) and the matching ids.  The inputs are
    float64 numbers whatever ``ftype``; the definitions are evaluated in ``ftype``.  A row with a NaN pose is NaN throughout."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    P = posed(np.asarray(foot, dtype=np.float64), rows[:, 4], rows[:, 6], rows[:, 7], ftype)
    cols = [wall_clearance(P, field, ftype) if field is not None else np.full(len(rows), np.inf, dtype=ftype)]
    cols += [polygon_clearance(P, np.asarray(q, dtype=np.float64), ftype) for q in polygons]
    cols += [circle_clearance(P, *c, ftype=ftype) for c in np.asarray(circles, dtype=np.float64).reshape(-1, 3)]
    ids = np.arange(-1, len(cols) - 1)
    E = np.stack(cols, axis=1)
    E[np.isnan(rows[:, [4, 6, 7]]).any(axis=1)] = np.nan
    return E, ids


def row_clearance(rows, foot, field=None, polygons=(), circles=(), ftype=np.float64):
    """Per row: clearance, element id (smallest on a tie), and the gap to the runner-up element.  A row with a NaN pose:
    NaN, -1, +inf."""
    E, ids = element_clearances(rows, foot, field, polygons, circles, ftype)
    bad = np.isnan(E).any(axis=1)
    k = np.argmin(np.where(bad[:, None], np.inf, E), axis=1)
    val = E[np.arange(len(E)), k]
    el = ids[k]
    if field is None:                     # no wall: its column is +inf and never wins
        el = np.where(np.isinf(val), -1, el)
    el = np.where(bad, -1, el)
    with np.errstate(invalid="ignore"):
        srt = np.sort(E, axis=1)
        gap = srt[:, 1] - srt[:, 0] if E.shape[1] > 1 else np.full(len(E), np.inf)
    gap = np.where(bad, np.inf, gap)
    return val, el, gap


def summarise(v, el, gap, margin=0.0):
    """The per-route outputs from one route's per-row clearances, elements and element gaps (row_clearance's).  A row whose
    clearance is NaN takes part in no minimum, count or first row; a route without a finite clearance gets the outputs of a
    route without rows (``n`` stays the count, ``rows`` the per-row values)."""
    out = {"n": len(v)}
    fin = ~np.isnan(v)
    if not fin.any():
        out.update(min_clearance=np.nan, min_row=-1, min_element=-1, first_row=-1, n_below=0, rows=v, elems=el, elem_gap=gap,
                   row_gap=np.inf, margin_gap=np.inf, row_gap_distinct=np.inf)
        return out
    w = np.where(fin, v, np.inf)
    r = int(np.argmin(w))
    below = np.nonzero(w < margin)[0]
    out.update(min_clearance=float(v[r]) if v.dtype == np.float64 else v[r], min_row=r, min_element=int(el[r]),
               first_row=int(below[0]) if len(below) else -1, n_below=int(len(below)), rows=v, elems=el, elem_gap=gap)
    srt = np.sort(v[fin])
    out["row_gap"] = float(srt[1] - srt[0]) if len(srt) > 1 else np.inf
    out["margin_gap"] = float(np.min(np.abs(v[fin] - margin)))
    # Rows whose clearances are equal bit for bit tie by construction (a repeated pose; the saturated value of a scene
    # element narrower than the robot, which is the extent of the element's own vertices on its own normal, the same
    # numbers at every row) and the first of them is the answer: the gap over distinct values.
    srt = np.unique(v[fin])
    out["row_gap_distinct"] = float(srt[1] - srt[0]) if len(srt) > 1 else np.inf
    return out


def route_summary(rows, count, foot, field=None, polygons=(), circles=(), margin=0.0, ftype=np.float64):
    """The per-route outputs of one route's first `count` rows, plus the per-row values and ambiguity gaps (summarise)."""
    rows = np.asarray(rows, dtype=np.float64)[:count]
    if count == 0:
        return dict(n=0, min_clearance=np.nan, min_row=-1, min_element=-1, first_row=-1, n_below=0,
                    rows=np.zeros(0), elems=np.zeros(0, int), elem_gap=np.zeros(0))
    return summarise(*row_clearance(rows, foot, field, polygons, circles, ftype), margin)
