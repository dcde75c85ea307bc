"""CPU restatements for the closest-point tests (gui/path.py:658-727): the GUI's two-pass search in NumPy, and an
independent EXACT reference (numpy.roots of (P - q) . P' per segment, Newton-polished, plus the segment endpoints)."""
import os

import numpy as np

import golden_util as gu

CLOSEST = os.path.join(gu.GOLDEN, "closest")


def cases():
    return sorted(f[:-4] for f in os.listdir(CLOSEST) if f.endswith(".npz"))


def load_case(name):
    c = np.load(os.path.join(CLOSEST, name + ".npz"))
    return c, gu.load(str(c["source"]))


class RefPath:
    """A path as the reference's segment blocks give it (golden_util.ref_segments): SM:243-275 spline mapping,
    QHS:506-541 parameter normalisation and the QHS:288-322 position basis, vectorised over parameters."""

    def __init__(self, g):
        self.seg, _, self.param_last = gu.ref_segments(g)
        ns = int(g["n_splines"])
        self.npts = np.array([int(g[f"spline{i}_n_points"]) for i in range(ns)])
        self.first = np.concatenate([[0], np.cumsum(self.npts - 1)[:-1]])
        self.W = len(g["waypoints"])

    @classmethod
    def from_arrays(cls, segments, param_last, n_points, W):
        """The same for segment blocks (W-1, 6, 2), parameters[-1] and point counts per spline given directly."""
        self = cls.__new__(cls)
        self.seg = np.asarray(segments, dtype=np.float64)
        self.param_last = np.asarray(param_last, dtype=np.float64)
        self.npts = np.asarray(n_points, dtype=np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.npts - 1)[:-1]])
        self.W = int(W)
        return self

    def spline_of(self, t):
        t = np.asarray(t, dtype=np.float64)
        ends = self.first + self.npts - 1
        si = np.full(t.shape, len(self.npts) - 1)
        for i in range(len(self.npts) - 2, -1, -1):
            si = np.where(t <= ends[i], i, si)
        return si

    def point(self, t, order=0):
        t = np.atleast_1d(np.asarray(t, dtype=np.float64))
        si = self.spline_of(t)
        lt = t - self.first[si]
        tmax = self.param_last[si]
        G = self.npts[si] - 1
        tt = np.maximum(0.0, np.minimum(lt, tmax))
        idx = tt.astype(np.int64)
        idx = np.where(idx == G, G - 1, idx)
        u = tt - idx
        u2 = u * u
        u3 = u2 * u
        u4 = u3 * u
        u5 = u4 * u
        if order == 0:
            H = [1 - 10 * u3 + 15 * u4 - 6 * u5, 10 * u3 - 15 * u4 + 6 * u5, u - 6 * u3 + 8 * u4 - 3 * u5,
                 -4 * u3 + 7 * u4 - 3 * u5, 0.5 * u2 - 1.5 * u3 + 1.5 * u4 - 0.5 * u5, 0.5 * u3 - u4 + 0.5 * u5]
        else:
            H = [-30 * u2 + 60 * u3 - 30 * u4, 30 * u2 - 60 * u3 + 30 * u4, 1 - 18 * u2 + 32 * u3 - 15 * u4,
                 -12 * u2 + 28 * u3 - 15 * u4, u - 4.5 * u2 + 6 * u3 - 2.5 * u4, 1.5 * u2 - 4 * u3 + 2.5 * u4]
        rows = self.seg[self.first[si] + idx]           # (n, 6, 2)
        out = np.zeros((len(t), 2))
        for i in range(6):
            out = out + H[i][:, None] * rows[:, i]
        return out


def gui_parameter(N, percent):
    """percent_to_parameter (SM:277-289, quirk Q6): min(max(N * percent, 0), N - 1)."""
    x = float(N) * np.asarray(percent, dtype=np.float64)
    return np.minimum(np.maximum(x, 0.0), float(N - 1))


def exact_search(path, q, seg_rows=None):
    """Independent EXACT reference: per segment the real roots in [0, 1] of g(u) = (P(u) - q) . P'(u) by numpy.roots,
    Newton-polished, and the segment endpoints; evaluated through RefPath.point.  (parameter, distance)."""
    seg = path.seg if seg_rows is None else seg_rows
    cands = [np.arange(path.W, dtype=np.float64)]
    for s in range(len(seg)):
        r = seg[s]
        cx, cy = (hermite_to_power(r[:, k]) for k in (0, 1))
        cx = cx.copy(); cy = cy.copy()
        cx[0] -= q[0]; cy[0] -= q[1]
        dx = np.arange(1, 6) * cx[1:]
        dy = np.arange(1, 6) * cy[1:]
        g = np.convolve(cx, dx) + np.convolve(cy, dy)     # ascending powers, degree 9
        if not np.any(g):
            continue
        gd = np.arange(1, 10) * g[1:]
        gr = np.trim_zeros(g[::-1], "f")
        roots = np.roots(gr) if len(gr) > 1 else np.array([])
        us = [u.real for u in roots if abs(u.imag) < 1e-6 and -1e-6 <= u.real <= 1 + 1e-6]
        for u in us:
            u = min(max(u, 0.0), 1.0)
            for _ in range(8):
                gv, gdv = np.polyval(g[::-1], u), np.polyval(gd[::-1], u)
                if gdv == 0:
                    break
                u = min(max(u - gv / gdv, 0.0), 1.0)
            cands.append(np.array([s + u]))
    t = np.concatenate(cands)
    pts = path.point(t)
    d = np.hypot(pts[:, 0] - q[0], pts[:, 1] - q[1])
    i = int(np.argmin(d))
    return float(t[i]), float(d[i])


def hermite_to_power(r):
    """Rows [p0, p1, d0, d1, dd0, dd1] of one coordinate -> monomial coefficients c0..c5 (QHS:293-298 expanded)."""
    p0, p1, d0, d1, e0, e1 = r
    d = p1 - p0
    return np.array([p0, d0, 0.5 * e0, 10 * d - 6 * d0 - 4 * d1 - 1.5 * e0 + 0.5 * e1,
                     -15 * d + 8 * d0 + 7 * d1 + 1.5 * e0 - e1, 6 * d - 3 * d0 - 3 * d1 - 0.5 * e0 + 0.5 * e1])


# ---- the wide side: the segment-row switch, query generators, tolerances (the cases: closest_cases.py) ----------------
# k_closest stages the 12 doubles of every segment in LDS while they fit 32 KB:          96 (W - 1) <= 32768
SEG_LDS_LIMIT = 32 * 1024
SEG_BYTES = {342: 32736, 343: 32832}
# launch_closest asks for spline table + staged rows.  Staged rows mean W <= 342, so at most 341 splines of 4 doubles;
# unstaged rows leave the table alone, at most one spline per segment of the widest route (1500 waypoints).
SPLINE_ROW_BYTES = 32
MAX_ROUTE_WAYPOINTS = 1500
DEFAULT_LDS = 64 * 1024
QUERIES_PER_BLOCK = 16
MAX_QUERY_BLOCKS = 65535
GAP_TIE = 1e-10             # the fixtures' rule: above it the GUI parameter must be equal
TIE_SHARE_CAP = 0.05

KIND_BOX, KIND_ON, KIND_END, KIND_RETRACED, KIND_SPLIT, KIND_LINE, KIND_EXTENSION = 0, 1, 2, 3, 4, 5, 6


def seg_bytes(W):
    return 96 * (W - 1)


def lds_request(W, n_splines):
    """Dynamic LDS bytes launch_closest asks for."""
    sg = seg_bytes(W)
    return SPLINE_ROW_BYTES * n_splines + (sg if sg <= SEG_LDS_LIMIT else 0)


def path_of_route(route, W):
    """RefPath on a drop-in route's own device-fitted rows: the fp64 segment rows the kernel reads."""
    return RefPath.from_arrays(route.segments, route.sp_param_last, route.sp_npts, W)


def split_nodes(W, rev=None, turn=None):
    """Interior nodes at which a route is cut (SM:84-158): a reverse node or a turn node."""
    s = np.zeros(W, dtype=bool)
    if rev is not None:
        s |= np.asarray(rev).astype(bool)
    if turn is not None:
        s |= np.asarray(turn, dtype=np.float64) != 0
    return [i for i in range(1, W - 1) if s[i]]


def path_of_oracle(op, rev=None, turn=None):
    """RefPath on the segments of an oracle.OraclePath (built with the same reverse / turn nodes)."""
    seg, _, pl = op.segments()
    cuts = [0] + split_nodes(op.W, rev, turn) + [op.W - 1]
    npts = np.diff(cuts) + 1
    assert len(npts) == op.n_splines == len(pl)
    return RefPath.from_arrays(seg, pl, npts, op.W)


def _gui_candidates(path, q):
    """Both passes' candidates: coarse parameters and distances, the coarse winner, fine parameters and distances."""
    N = path.W
    steps = 25 * N
    pc = np.arange(steps + 1) / steps                  # i / num_steps, correctly rounded like Python's
    tc = gui_parameter(N, pc)
    pts = path.point(tc)
    dc = np.hypot(pts[:, 0] - q[0], pts[:, 1] - q[1])
    ic = int(np.argmin(dc))                             # strict '<' in a forward scan: the first index wins
    cp = pc[ic]
    start, end = max(0.0, cp - 0.02), min(1.0, cp + 0.02)
    step = (end - start) / 500
    tf = gui_parameter(N, start + np.arange(501) * step)     # start + i * step, no fused multiply-add
    pts = path.point(tf)
    df = np.hypot(pts[:, 0] - q[0], pts[:, 1] - q[1])
    return tc, dc, ic, tf, df


def gui_search(path, q, gap=False):
    """The two passes of gui/path.py:690-722 for one query q (feet): (parameter, min_dist).  With gap=True also the
    fixtures' `gap` (tools/gen_closest_golden.py:167-171): the second-best minus the best candidate distance over both
    passes, counting only candidates at another parameter than the winner's (inf when there is none)."""
    tc, dc, ic, tf, df = _gui_candidates(path, q)
    jf = int(np.argmin(df))
    t, d = (tf[jf], df[jf]) if df[jf] < dc[ic] else (tc[ic], dc[ic])     # min_dist carries over from the coarse pass
    if not gap:
        return float(t), float(d)
    ts, ds = np.concatenate([tc, tf]), np.concatenate([dc, df])
    other = ds[ts != t]
    return float(t), float(d), (float(other.min() - ds.min()) if other.size else np.inf)


def cross_track(path, t, q):
    """(cross_track, cross, speed): +distance when q lies left of the direction of travel at t (cross > 0), else -distance."""
    p = path.point([t])[0]
    dp = path.point([t], order=1)[0]
    d = float(np.hypot(p[0] - q[0], p[1] - q[1]))
    cross = float(dp[0] * (q[1] - p[1]) - dp[1] * (q[0] - p[0]))
    return (d if cross > 0.0 else -d), cross, float(np.hypot(dp[0], dp[1]))


def brute_grid(path, per_segment=2000):
    """(t, points, resolution) of a dense grid of per_segment evaluations per segment plus the last node.  The grid point
    nearest to any parameter is within half a step of it, so the grid's best distance exceeds the true minimum by at
    most resolution = (largest speed on the grid, 5 % margin for what lies between) * half a step."""
    G = path.W - 1
    t = np.concatenate([(np.arange(G)[:, None] + np.arange(per_segment)[None] / per_segment).ravel(), [float(G)]])
    pts = np.concatenate([path.point(t[a:a + 100000]) for a in range(0, len(t), 100000)])
    sp = np.concatenate([path.point(t[a:a + 100000], order=1) for a in range(0, len(t), 100000)])
    return t, pts, float(1.05 * np.hypot(sp[:, 0], sp[:, 1]).max() * 0.5 / per_segment)


def exact_tol(waypoints, queries):
    """Bound on |EXACT distance - reference|: 1e-12 on the 12 ft field (coordinates in the binade below 8 ft), growing
    with the coordinates' ulp: 1e-12 * max(1, M / 8), M the largest magnitude among waypoints and queries."""
    M = max(float(np.max(np.abs(waypoints))), float(np.max(np.abs(queries))) if np.size(queries) else 0.0)
    return 1e-12 * max(1.0, M / 8.0)


def make_queries(path, waypoints, seed, n_box=10, n_on=10, n_end=2, retraced=()):
    """Deterministic queries for one path: (q (n, 2), kind (n,), t0 (n,)).  n_box points uniform in the waypoints'
    bounding box grown by 1 ft, n_on points on the path at parameters t0 uniform over [0, W-1], n_end points beyond each
    end along the end tangent (0.3 ft and farther, a little off the tangent line), and one point per entry of
    `retraced`: parameters whose point another parameter of the path shares exactly."""
    rng = np.random.default_rng([20343, int(seed)])
    wp = np.asarray(waypoints, dtype=np.float64)
    W = path.W
    lo, hi = wp.min(axis=0) - 1.0, wp.max(axis=0) + 1.0
    q = [rng.uniform(lo, hi, (n_box, 2))]
    kind = [np.full(n_box, KIND_BOX)]
    t0 = [np.full(n_box, np.nan)]
    ton = rng.uniform(0.0, W - 1.0, n_on)
    q.append(path.point(ton)); kind.append(np.full(n_on, KIND_ON)); t0.append(ton)
    for t_end, sign in ((0.0, -1.0), (W - 1.0, 1.0)):
        p = path.point([t_end])[0]
        d = path.point([t_end], order=1)[0]
        u = d / max(np.hypot(d[0], d[1]), 1e-12)
        for k in range(n_end):
            q.append((p + sign * (0.3 + 0.6 * k) * u + rng.normal(0.0, 0.02, 2))[None])
            kind.append(np.array([KIND_END])); t0.append(np.array([t_end]))
    for t in retraced:
        q.append(path.point([float(t)])); kind.append(np.array([KIND_RETRACED])); t0.append(np.array([float(t)]))
    return np.concatenate(q), np.concatenate(kind).astype(np.int64), np.concatenate(t0)
