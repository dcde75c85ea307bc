"""Plain NumPy statement of vap_pursuit_rollouts (include/vap.h): a differential-drive robot with a pure-pursuit follower
rolled along the polyline of one route's time-domain rows, under one perturbation record.

``rollout`` is written for one rollout: every quantity is a scalar of ``dtype`` (or an index) and the loop is the
header's steps 1-7 in order.  Every operation in it is elementwise and the two pointer walks are masked, so handing it an
(M, 8) block of records for the SAME route walks M independent rollouts side by side and gives each exactly what a call
of its own gives.  ``dtype`` switches the arithmetic: np.float64 (what the kernel is compared against) or np.longdouble
(what the float64 run itself is compared against, to size the tolerance).  It imports nothing from the package.

Rows are {time, position, velocity, acceleration, heading, angular_vel, x, y}; the path is P_i = columns 6, 7 with the
speeds v_i = column 2; row 0's columns 4 and 5 give the start heading and body rate.  Nothing else is read.
"""
import numpy as np

PI = float(np.pi)           # the wrap's constant is the fp64 pi in every dtype
DEFAULTS = dict(track_width=1.0, lookahead=0.75, min_speed=0.1, arrive_tolerance=0.05, wheel_speed_max=6.0, tolerance=0.25,
                n_substeps=2, settle_rows=150)
NOMINAL = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0])
STATUS_NEGATIVE_SPEED, STATUS_NON_FINITE = 1, 2


def pursuit(**kw):
    f = dict(DEFAULTS)
    f.update(kw)
    return f


def wrap(a):
    """((a + pi) mod 2 pi) - pi with the floored mod."""
    return (a + PI) % (2 * PI) - PI


def sinc(x):
    """sin x / x; 1 - x^2 / 6 for |x| < 1e-4."""
    x = np.asarray(x)
    small = np.abs(x) < 1e-4
    safe = np.where(small, 1, x)
    return np.where(small, 1 - x * x / 6, np.sin(safe) / safe)


def record_valid(p):
    """The RAMSETE call's rule, and slot 7 (the rollout's lookahead; 0: the follower's) >= 0."""
    p = np.atleast_2d(np.asarray(p, dtype=np.float64))
    return np.isfinite(p).all(axis=1) & (p[:, 3] > 0) & (p[:, 4] > 0) & (p[:, 5] > 0) & (p[:, 6] >= 0) & (p[:, 7] >= 0)


def route_status(rows, n):
    """Bit 0: a row with v < 0; bit 1: a non-finite x, y or v; over rows 0 .. n - 1."""
    rows = np.asarray(rows, dtype=np.float64)
    n = min(max(int(n), 0), rows.shape[0])
    q = rows[:n][:, [6, 7, 2]]
    return (STATUS_NEGATIVE_SPEED if (q[:, 2] < 0).any() else 0) | (0 if np.isfinite(q).all() else STATUS_NON_FINITE)


def path_of(rows, n, F):
    """P (n, 2), v (n,), the segments' lengths (n - 1,), the cumulative chord length c (n,) summed strictly in index
    order, and the direction of the last segment of positive length ((1, 0) without one)."""
    P = rows[:n, 6:8].astype(F)
    v = rows[:n, 2].astype(F)
    s = P[1:] - P[:-1]
    ln = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1])
    c = np.zeros(n, dtype=F)
    for i in range(n - 1):
        c[i + 1] = c[i] + ln[i]
    u = np.array([1, 0], dtype=F)
    for i in range(n - 2, -1, -1):
        if ln[i] > 0:
            u = s[i] / ln[i]
            break
    return P, v, ln, c, u


def rollout(rows, n, f, perturb, time_step=0.01, executed=False, dtype=np.float64):
    """One route's rows (capacity, 8), its count n and perturbation record(s) (8,) or (M, 8).

    Returns a dict: status (the route's); stats (M, 6) = max e_ct, final position error, arrival time (NaN: never), the
    rollout's lookahead, 0, 0; stat_rows (M, 4) = step of max e_ct, saturated rows, arrived step (-1: never), final ic;
    e_ct, cmd_max, end_dist (M, n + settle): the cross-track error, the unsaturated command max(|c_L|, |c_R|) and the
    distance to the last point at every step; and with ``executed`` rows (M, n + settle, 8) and counts (M,).  Invalid
    records, n = 0 and a route with a status bit give NaN / -1 (counts 0)."""
    F = dtype
    rows = np.asarray(rows, dtype=np.float64)
    n = min(max(int(n), 0), rows.shape[0])
    Pr = np.atleast_2d(np.asarray(perturb, dtype=np.float64))
    M = len(Pr)
    settle, nsub = int(f["settle_rows"]), int(f["n_substeps"])
    status = route_status(rows, n)
    total = n + settle if n > 0 and status == 0 else 0
    out = {"status": status, "stats": np.full((M, 6), np.nan, dtype=F), "stat_rows": np.full((M, 4), -1, dtype=np.int64),
           "e_ct": np.full((M, total), np.nan, dtype=F), "cmd_max": np.full((M, total), np.nan, dtype=F),
           "end_dist": np.full((M, total), np.nan, dtype=F)}
    if executed:
        out["rows"] = np.full((M, total, 8), np.nan, dtype=F)
        out["counts"] = np.zeros(M, dtype=np.int64)
    ok = record_valid(Pr)
    if total == 0 or not ok.any():
        return out
    p = Pr[ok].astype(F)
    m = len(p)
    T, wmax = F(f["track_width"]), F(f["wheel_speed_max"])
    vmin, atol = F(f["min_speed"]), F(f["arrive_tolerance"])
    dt = F(time_step)
    h = dt / nsub
    gl, gr, tau = p[:, 3], p[:, 4], p[:, 6]
    tts = T * p[:, 5]
    a = np.where(tau == 0, 1, 1 - np.exp(-h / np.where(tau == 0, 1, tau)))
    L = np.where(p[:, 7] > 0, p[:, 7], F(f["lookahead"]))
    P, vp, ln, c, uend = path_of(rows, n, F)
    last = P[n - 1]
    v0, w0 = F(rows[0, 2]), F(-rows[0, 5])
    x, y, phi = P[0, 0] + p[:, 0], P[0, 1] + p[:, 1], F(-rows[0, 4]) + p[:, 2]
    wl = np.full(m, v0 - w0 * T / 2, dtype=F)
    wr = np.full(m, v0 + w0 * T / 2, dtype=F)
    ic, il = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    arrived = np.full(m, -1, dtype=np.int64)
    maxe = np.full(m, -np.inf, dtype=F)
    mrow, nsat = np.full(m, -1, dtype=np.int64), np.zeros(m, dtype=np.int64)
    dist, vprev = np.zeros(m, dtype=F), np.zeros(m, dtype=F)
    ect_rows, cmd_rows, end_rows = (np.zeros((m, total), dtype=F) for _ in range(3))
    ex_rows = np.zeros((m, total, 8), dtype=F) if executed else None
    zero, one = F(0), F(1)

    def project(i):
        """t, D of the point (x, y) on segment i (an index per rollout)."""
        sx, sy = P[i + 1, 0] - P[i, 0], P[i + 1, 1] - P[i, 1]
        ss = sx * sx + sy * sy
        t = ((x - P[i, 0]) * sx + (y - P[i, 1]) * sy) / np.where(ss == 0, 1, ss)
        t = np.where(ss == 0, zero, np.minimum(np.maximum(t, zero), one))
        ex, ey = x - (P[i, 0] + t * sx), y - (P[i, 1] + t * sy)
        return t, ex * ex + ey * ey

    for r in range(total):
        # 1. closest point
        if n >= 2:
            while True:
                nxt = np.minimum(ic + 1, n - 2)
                adv = (ic < n - 2) & (project(nxt)[1] <= project(ic)[1])
                if not adv.any():
                    break
                ic = ic + adv
            t, D = project(ic)
            ect = np.sqrt(D)
            vt = vp[ic] + t * (vp[ic + 1] - vp[ic])
            sc = c[ic] + t * ln[ic]
            at_end = (ic == n - 2) & (t == 1)
        else:
            ex, ey = x - P[0, 0], y - P[0, 1]
            ect = np.sqrt(ex * ex + ey * ey)
            vt = np.full(m, vp[0], dtype=F)
            sc = np.zeros(m, dtype=F)
            at_end = np.ones(m, dtype=bool)
        # 2. statistics
        up = ect > maxe
        maxe, mrow = np.where(up, ect, maxe), np.where(up, r, mrow)
        ect_rows[:, r] = ect
        # 3. the executed row
        if executed:
            v = (gl * wl + gr * wr) / 2
            om = (gr * wr - gl * wl) / tts
            ex_rows[:, r, 0] = r * dt
            ex_rows[:, r, 1] = dist
            ex_rows[:, r, 2] = v
            ex_rows[:, r, 3] = (v - vprev) / dt if r > 0 else 0
            ex_rows[:, r, 4] = -wrap(phi)
            ex_rows[:, r, 5] = -om
            ex_rows[:, r, 6] = x
            ex_rows[:, r, 7] = y
            vprev = v
        # 4. arrival
        ex, ey = last[0] - x, last[1] - y
        dend = np.sqrt(ex * ex + ey * ey)
        end_rows[:, r] = dend
        arrived = np.where((arrived < 0) & (at_end | (dend <= atol)), r, arrived)
        live = arrived < 0
        # 5. lookahead and command (n >= 2 here: a route of one row has arrived)
        cl, cr = np.zeros(m, dtype=F), np.zeros(m, dtype=F)
        if live.any():
            star = sc + L
            il = np.where(live, np.maximum(il, ic), il)
            while True:
                adv = live & (il < n - 2) & (c[np.minimum(il + 1, n - 1)] < star)
                if not adv.any():
                    break
                il = il + adv
            beyond = star >= c[n - 1]
            lenl = ln[il]
            fr = (star - c[il]) / np.where(lenl == 0, 1, lenl)
            fr = np.where(lenl == 0, zero, np.minimum(np.maximum(fr, zero), one))
            gx = np.where(beyond, last[0] + (star - c[n - 1]) * uend[0], P[il, 0] + fr * (P[il + 1, 0] - P[il, 0]))
            gy = np.where(beyond, last[1] + (star - c[n - 1]) * uend[1], P[il, 1] + fr * (P[il + 1, 1] - P[il, 1]))
            dx, dy = gx - x, gy - y
            ly = -np.sin(phi) * dx + np.cos(phi) * dy
            a2 = dx * dx + dy * dy
            kap = np.where(a2 == 0, zero, 2 * ly / np.where(a2 == 0, 1, a2))
            sp = np.maximum(vt, vmin)
            cl = np.where(live, sp - sp * kap * T / 2, zero)
            cr = np.where(live, sp + sp * kap * T / 2, zero)
        # 6. saturation, keeping c_L : c_R
        mx = np.maximum(np.abs(cl), np.abs(cr))
        sat = mx > wmax
        cmd_rows[:, r] = mx
        scale = np.where(sat, wmax / np.where(sat, mx, 1), 1)
        cl, cr = np.where(sat, cl * scale, cl), np.where(sat, cr * scale, cr)
        nsat = nsat + sat
        # 7. substeps: first-order wheel lag, then the exact arc
        for _ in range(nsub):
            wl = wl + (cl - wl) * a
            wr = wr + (cr - wr) * a
            v = (gl * wl + gr * wr) / 2
            om = (gr * wr - gl * wl) / tts
            u = om * h / 2
            d = v * h * sinc(u)
            x = x + d * np.cos(phi + u)
            y = y + d * np.sin(phi + u)
            phi = phi + om * h
            dist = dist + np.abs(d)
    ex, ey = last[0] - x, last[1] - y
    nan = F(np.nan)
    st = np.stack([maxe, np.sqrt(ex * ex + ey * ey), np.where(arrived >= 0, arrived * dt, nan), L, np.zeros(m, dtype=F),
                   np.zeros(m, dtype=F)], axis=1)
    out["stats"][ok] = st
    out["stat_rows"][ok] = np.stack([mrow, nsat, arrived, ic], axis=1)
    out["e_ct"][ok] = ect_rows
    out["cmd_max"][ok] = cmd_rows
    out["end_dist"][ok] = end_rows
    if executed:
        out["rows"][ok] = ex_rows
        out["counts"][ok] = total
    return out


def route_summary(stats, stat_rows, tolerance):
    """The per-route outputs from one route's (K, 6) stats and (K, 4) stat rows: worst (the smallest k on a tie), mean
    (summed in ascending k), worst_rollout, worst_row, n_exceeding, n_unfinished; NaN / -1 / 0 without a valid rollout."""
    worst, wk, wrow, total, cnt, nex, nun = -np.inf, -1, -1, stats.dtype.type(0), 0, 0, 0
    for k in range(len(stats)):
        if stat_rows[k, 0] < 0:
            continue
        e = stats[k, 0]
        if e > worst:
            worst, wk, wrow = e, k, int(stat_rows[k, 0])
        total = total + e
        cnt += 1
        nex += int(e > tolerance)
        nun += int(stat_rows[k, 2] < 0)
    if cnt == 0:
        return dict(worst=np.nan, mean=np.nan, worst_rollout=-1, worst_row=-1, n_exceeding=0, n_unfinished=0)
    return dict(worst=worst, mean=total / cnt, worst_rollout=wk, worst_row=wrow, n_exceeding=nex, n_unfinished=nun)


def golden_rows(g):
    """The reference's own time-domain rows of a golden fixture, in the time-profile layout (n, 8)."""
    c = np.asarray(g["profile_coords"], dtype=np.float64).reshape(-1, 2)
    return np.stack([g["profile_times"], g["profile_positions"], g["profile_linear_vels"], g["profile_accelerations"],
                     g["profile_headings"], g["profile_angular_vels"], c[:, 0], c[:, 1]], axis=1).astype(np.float64)
