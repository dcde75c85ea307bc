"""Plain NumPy fp64 reference of vap_range_readings (include/vap.h): what a single-ray distance sensor reads at every row,
its status, and the per-route summaries.  Imports nothing from the package.  The definitions are written as the header
states them (divisions and all), vectorised over the rows only: the loops over sensors, elements and edges are Python's.

Besides each reading the reference reports a decision margin: how far the reading is from any decision that would change
it — the runner-up's distance behind the best, the distance of the hit from its edge's ends, sqrt(disc) of a circle, the
window and incidence thresholds, and the same quantities for near misses that would have taken the lead.  A reading with a
margin below AMBIGUOUS, or with cos_inc < COS_EXCUSE (t carries the pose's rounding times 1 / cos_inc), is excused from a
comparison."""
import numpy as np

AMBIGUOUS = 1e-9
COS_EXCUSE = 0.1
VALID, NONE, NEAR, FAR, OBLIQUE, BLOCKED, BAD_POSE = range(7)
INF = np.inf


class _State:
    """Best candidate per reading, the runner-up's t, the best's own margin and the near misses."""

    def __init__(self, n, ftype=np.float64, ambiguous=AMBIGUOUS):
        self.t = np.full(n, INF, dtype=ftype)
        self.cos = np.full(n, np.nan, dtype=ftype)
        self.face = np.zeros(n, dtype=np.int64)
        self.el = np.full(n, -2, dtype=np.int64)
        self.second = np.full(n, INF, dtype=ftype)
        self.own = np.full(n, INF, dtype=ftype)
        self.misses = []
        self.ambiguous = ambiguous

    def offer(self, ok, t, cos, face, el, own):
        t = np.where(ok, t, INF)
        win = ok & (t < self.t)                      # a later candidate replaces the best only on a strictly smaller t
        runner = ok & ~win & (t < self.second)
        self.second = np.where(win, self.t, np.where(runner, t, self.second))
        self.t = np.where(win, t, self.t)
        self.cos = np.where(win, cos, self.cos)
        self.face = np.where(win, face, self.face)
        self.el = np.where(win, el, self.el)
        self.own = np.where(win, own, self.own)

    def miss(self, cond, t_would, viol):
        self.misses.append((cond, np.where(cond, t_would, INF), np.where(cond, viol, INF)))

    def miss_margin(self):
        m = np.full(self.t.shape, INF)
        for cond, tw, viol in self.misses:
            matters = cond & (np.maximum(tw, 0.0) <= self.t + self.ambiguous)     # it would have taken the lead (or tied)
            m = np.where(matters, np.minimum(m, viol), m)
        return m


def _edges(st, ox, oy, ux, uy, ax, ay, ex, ey, face, el):
    """Edge a -> a + e (scalars, or arrays per reading) against the rays."""
    with np.errstate(all="ignore"):
        den = ux * ey - uy * ex
        dx, dy = ax - ox, ay - oy
        t = (dx * ey - dy * ex) / den
        w = (dx * uy - dy * ux) / den
        length = np.hypot(ex, ey)
        nz = den != 0
        ok = nz & (t >= 0) & (w >= 0) & (w <= 1)
        cos = np.abs(ux * (ey / length) + uy * (-ex / length))
        own = np.minimum(np.minimum(w, 1 - w) * length, t)
        viol = np.maximum(np.maximum(-w * length, (w - 1) * length), np.maximum(-t, 0.0))
        st.offer(ok, t, cos, face, el, own)
        st.miss(nz & ~ok & np.isfinite(t) & np.isfinite(w), t, viol)


def _polygon(st, ox, oy, ux, uy, verts, el):
    m = len(verts)
    for j in range(m):
        a, b = verts[j], verts[(j + 1) % m]
        _edges(st, ox, oy, ux, uy, a[0], a[1], b[0] - a[0], b[1] - a[1], j, el)


def _circle(st, ox, oy, ux, uy, cx, cy, r, el):
    with np.errstate(all="ignore"):
        dx, dy = ox - cx, oy - cy
        b = dx * ux + dy * uy
        q = (dx * dx + dy * dy) - r * r
        disc = b * b - q
        sq = np.sqrt(np.where(disc >= 0, disc, 0.0))
        t1, t2 = -b - sq, -b + sq
        t = np.where(t1 < 0, t2, t1)
        ok = (disc >= 0) & (t >= 0)
        cos = np.abs(ux * ((ox + t * ux) - cx) + uy * ((oy + t * uy) - cy)) / r
        own = np.minimum(np.minimum(sq, np.abs(t1)), np.abs(t2))
        st.offer(ok, t, cos, 0, el, own)
        st.miss((disc < 0) & (-b >= -np.sqrt(np.abs(disc))), -b, np.sqrt(np.abs(disc)))     # the ray just passes the circle
        st.miss((disc >= 0) & (t < 0), 0.0, -t)                                               # the circle is just behind


def _wall(st, ox, oy, ux, uy, field):
    xmin, ymin, xmax, ymax = field
    with np.errstate(all="ignore"):
        inside = (ox >= xmin) & (ox <= xmax) & (oy >= ymin) & (oy <= ymax)
        tx = np.where(ux > 0, (xmax - ox) / ux, np.where(ux < 0, (xmin - ox) / ux, INF))
        ty = np.where(uy > 0, (ymax - oy) / uy, np.where(uy < 0, (ymin - oy) / uy, INF))
        fx = np.where(ux > 0, 2, 0)
        fy = np.where(uy > 0, 3, 1)
        y_side = ty < tx                                        # a tie: the x side
        t = np.where(y_side, ty, tx)
        cos = np.where(y_side, np.abs(uy), np.abs(ux))
        face = np.where(y_side, fy, fx)
        border = np.minimum(np.minimum(np.abs(ox - xmin), np.abs(xmax - ox)), np.minimum(np.abs(oy - ymin), np.abs(ymax - oy)))
        own = np.minimum(np.abs(tx - ty), border)               # the corner, and the origin on the box
        own = np.where(np.isnan(own), INF, own)
        st.offer(inside & (t < INF), t, cos, face, -1, own)
        st.miss(~inside & np.isfinite(border), 0.0, border)


def pose_polygon(foot, heading, x, y):
    """The footprint (n, 2) posed at arrays heading, x, y: vertices (N, n, 2)."""
    phi = -heading
    c, s = np.cos(phi), np.sin(phi)
    vx = x[:, None] + (c[:, None] * foot[None, :, 0] - s[:, None] * foot[None, :, 1])
    vy = y[:, None] + (s[:, None] * foot[None, :, 0] + c[:, None] * foot[None, :, 1])
    return np.stack([vx, vy], axis=2)


def cast(heading, x, y, sensor, field=None, polygons=(), circles=(), partners=(), ftype=np.float64, ambiguous=AMBIGUOUS):
    """One sensor (8,) at N poses.  partners: a list of (N, n, 2) posed footprints, or None for an absent partner.  Returns a
    dict of (N,) arrays: status, face, element, t, cos (NaN for status 1 and 6), margin, excused.  ftype: the precision of the
    whole computation (np.longdouble measures the float64 path's own rounding; the inputs are the same doubles); ambiguous: the
    margin below which a reading is excused."""
    heading, x, y = (np.asarray(v, dtype=ftype) for v in (heading, x, y))
    n = heading.shape[0]
    mx, my, bx, by, r_min, r_max, min_cos = (ftype(v) for v in sensor[:7])
    if field is not None:
        field = tuple(ftype(v) for v in field)
    phi = -heading
    with np.errstate(all="ignore"):
        c, s = np.cos(phi), np.sin(phi)
        ox, oy = x + (c * mx - s * my), y + (s * mx + c * my)
        ux, uy = c * bx - s * by, s * bx + c * by
    st = _State(n, ftype, ambiguous)
    if field is not None:
        _wall(st, ox, oy, ux, uy, field)
    polygons, circles = list(polygons), np.asarray(circles, dtype=ftype).reshape(-1, 3)
    for k, verts in enumerate(polygons):
        _polygon(st, ox, oy, ux, uy, np.asarray(verts, dtype=ftype), k)
    for k, (cx, cy, r) in enumerate(circles):
        _circle(st, ox, oy, ux, uy, cx, cy, r, len(polygons) + k)
    first_partner = len(polygons) + len(circles)
    for o, posed in enumerate(partners):
        if posed is None:
            continue
        m = posed.shape[1]
        for j in range(m):
            a, b = posed[:, j], posed[:, (j + 1) % m]
            _edges(st, ox, oy, ux, uy, a[:, 0], a[:, 1], b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], j, first_partner + o)
    bad = ~(np.isfinite(heading) & np.isfinite(x) & np.isfinite(y))
    has = st.el != -2
    with np.errstate(invalid="ignore"):
        status = np.where(bad, BAD_POSE, np.where(~has, NONE, np.where(st.el >= first_partner, BLOCKED, np.where(
            st.t < r_min, NEAR, np.where(st.t > r_max, FAR, np.where(st.cos < min_cos, OBLIQUE, VALID))))))
        margin = np.minimum(st.miss_margin(), np.where(has, np.minimum(st.second - st.t, st.own), INF))
        thresholds = np.minimum(np.minimum(np.abs(st.t - r_min), np.abs(st.t - r_max)), np.abs(st.cos - min_cos))
        margin = np.where(has & (st.el < first_partner), np.minimum(margin, thresholds), margin)
        margin = np.where(bad, INF, margin)
        excused = ~bad & ((margin < ambiguous) | (has & (st.cos < COS_EXCUSE)))
    none = bad | ~has
    return {"status": status, "face": np.where(none, 0, st.face), "element": np.where(none, -2, st.el),
            "t": np.where(none, np.nan, st.t), "cos": np.where(none, np.nan, st.cos), "margin": margin, "excused": excused}


def readings(rows, counts, sensors, field=None, polygons=(), circles=(), others=None, others_counts=None, others_foot=None,
             shift_rows=0, ftype=np.float64, ambiguous=AMBIGUOUS):
    """Every reading of a batch: rows (B, cap, 8), counts (B,), sensors (ns, 8).  Returns a dict of (B, cap, ns) arrays
    (status -1, NaN past counts; ``live`` marks the rows below the counts).  ftype, ambiguous: ``cast``'s."""
    rows = np.asarray(rows, dtype=ftype)
    B, cap = rows.shape[:2]
    sensors = np.asarray(sensors, dtype=ftype).reshape(-1, 8)
    ns = len(sensors)
    counts = np.clip(np.asarray(counts).reshape(B, -1)[:, 0], 0, cap)
    live = np.arange(cap)[None, :] < counts[:, None]
    bi, ri = np.nonzero(live)
    h, x, y = rows[bi, ri, 4], rows[bi, ri, 6], rows[bi, ri, 7]
    partners = []
    if others is not None:
        others = np.asarray(others, dtype=ftype)
        oc = np.clip(np.asarray(others_counts).reshape(len(others), -1)[:, 0], 0, others.shape[1])
        for o in range(len(others)):
            if oc[o] == 0:
                partners.append(None)
                continue
            ro = np.clip(ri - int(shift_rows), 0, oc[o] - 1)
            partners.append(pose_polygon(np.asarray(others_foot, dtype=ftype), others[o, ro, 4], others[o, ro, 6], others[o, ro, 7]))
    out = {"status": np.full((B, cap, ns), -1, dtype=np.int64), "face": np.full((B, cap, ns), -1, dtype=np.int64),
           "element": np.full((B, cap, ns), -2, dtype=np.int64), "t": np.full((B, cap, ns), np.nan, dtype=ftype),
           "cos": np.full((B, cap, ns), np.nan, dtype=ftype), "margin": np.full((B, cap, ns), INF, dtype=ftype),
           "excused": np.zeros((B, cap, ns), dtype=bool), "live": live, "counts": counts}
    for s in range(ns):
        r = cast(h, x, y, sensors[s], field, polygons, circles, partners, ftype, ambiguous)
        for k, v in r.items():
            out[k][bi, ri, s] = v
    return out


# ---- the gap record ---------------------------------------------------------------------------------------------------------
def gap_scan(ok):
    """Brute force over boolean rows: (n_ok, first_ok, last_ok, gap_rows, gap_row)."""
    ok = [bool(v) for v in ok]
    n_ok = sum(ok)
    first = ok.index(True) if n_ok else -1
    last = len(ok) - 1 - ok[::-1].index(True) if n_ok else -1
    best, start, run = 0, -1, 0
    for i, v in enumerate(ok):
        run = 0 if v else run + 1
        if run > best:
            best, start = run, i - run + 1
    return n_ok, first, last, best, start


def gap_record(ok, row0):
    """The associative record of rows row0 .. row0 + len(ok) - 1: (row0, len, n_ok, lead, trail, best, start)."""
    n = len(ok)
    if n == 0:
        return (row0, 0, 0, 0, 0, 0, -1)
    n_ok, first, last, best, start = gap_scan(ok)
    lead = first if n_ok else n
    trail = n - 1 - last if n_ok else n
    return (row0, n, n_ok, lead, trail, best, row0 + start if best else -1)


def gap_combine(a, b):
    """a, then b right behind it."""
    if a[1] == 0:
        return b
    if b[1] == 0:
        return a
    row0, la, na, lead_a, trail_a, best_a, start_a = a
    _, lb, nb, lead_b, trail_b, best_b, start_b = b
    lead = la + lead_b if lead_a == la else lead_a
    trail = lb + trail_a if trail_b == lb else trail_b
    best, start = best_a, start_a
    mid = trail_a + lead_b
    if mid > best:
        best, start = mid, row0 + la - trail_a
    if best_b > best:
        best, start = best_b, start_b
    return (row0, la + lb, na + nb, lead, trail, best, start)


def gap_finish(rec):
    """(n_ok, first_ok, last_ok, gap_rows, gap_row) of a record that starts at row 0."""
    _, n, n_ok, lead, trail, best, start = rec
    return (n_ok, lead if n_ok else -1, n - 1 - trail if n_ok else -1, best, start if best else -1)


# ---- the summaries ------------------------------------------------------------------------------------------------------------
def summaries(ref):
    """Per-route summaries of ``readings``' result: status_counts (B, ns, 8), minmax (B, ns, 2), channels (B, ns + 2, 5), and
    which of them an excused reading touches: touched (B, ns + 2) bool (channel s: sensor s's counts, min / max and channel;
    the last two: the x and y channels, which any sensor of the route touches)."""
    status, face, el, t = ref["status"], ref["face"], ref["element"], ref["t"]
    B, cap, ns = status.shape
    counts = ref["counts"]
    sc = np.zeros((B, ns, 8), dtype=np.int64)
    mm = np.full((B, ns, 2), np.nan)
    ch = np.zeros((B, ns + 2, 5), dtype=np.int64)
    touched = np.zeros((B, ns + 2), dtype=bool)
    for b in range(B):
        n = int(counts[b])
        ok = status[b, :n] == VALID                                  # (n, ns)
        wall = ok & (el[b, :n] == -1)
        xobs = (wall & ((face[b, :n] == 0) | (face[b, :n] == 2))).any(axis=1) if n else np.zeros(0, dtype=bool)
        yobs = (wall & ((face[b, :n] == 1) | (face[b, :n] == 3))).any(axis=1) if n else np.zeros(0, dtype=bool)
        for s in range(ns):
            for k in range(7):
                sc[b, s, k] = int(np.sum(status[b, :n, s] == k))
            v = t[b, :n, s][ok[:, s]]
            if len(v):
                mm[b, s] = v.min(), v.max()
            ch[b, s] = gap_scan(ok[:, s])
            touched[b, s] = ref["excused"][b, :n, s].any()
        ch[b, ns] = gap_scan(xobs)
        ch[b, ns + 1] = gap_scan(yobs)
        touched[b, ns:] = touched[b, :ns].any()
    return {"status_counts": sc, "minmax": mm, "channels": ch, "touched": touched}
