"""Plain NumPy statement of vap_tracking_rollouts (include/vap.h): a differential-drive robot with a RAMSETE follower
rolled along the time-domain rows of one route, under one perturbation record.

``rollout`` is written for one rollout: every quantity is a scalar of ``dtype`` and the loop is the header's steps 1-7 in
order.  Every operation in it is elementwise, so handing it an (M, 8) block of records for the SAME route walks M
independent rollouts side by side and gives each exactly what a call of its own gives (the tests use that to keep the
reference fast).  ``dtype`` switches the arithmetic: np.float64 (what the kernel is compared against) or np.longdouble
(what the float64 run itself is compared against, to size the tolerance).

Rows are {time, position, velocity, acceleration, heading, angular_vel, x, y}; the reference pose at row r is
(x, y) = columns 6, 7, phi = -column 4, v = column 2, omega = -column 5.
"""
import numpy as np

PI = float(np.pi)           # the wrap's constant is the fp64 pi in every dtype
DEFAULTS = dict(track_width=1.0, b=2.0, zeta=0.7, wheel_speed_max=6.0, tolerance=0.25, n_substeps=2, settle_rows=50)
NOMINAL = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0])


def follower(**kw):
    f = dict(DEFAULTS)
    f.update(kw)
    return f


def wrap(a):
    """((a + pi) mod 2 pi) - pi with the floored mod (MPG:560-562)."""
    return (a + PI) % (2 * PI) - PI


def sinc(x):
    """sin x / x; 1 - x^2 / 6 for |x| < 1e-4."""
    x = np.asarray(x)
    small = np.abs(x) < 1e-4
    safe = np.where(small, 1, x)
    return np.where(small, 1 - x * x / 6, np.sin(safe) / safe)


def record_valid(p):
    p = np.atleast_2d(np.asarray(p, dtype=np.float64))
    return np.isfinite(p).all(axis=1) & (p[:, 3] > 0) & (p[:, 4] > 0) & (p[:, 5] > 0) & (p[:, 6] >= 0)


def rollout(rows, n, f, perturb, time_step=0.01, executed=False, dtype=np.float64):
    """One route's rows (capacity, 8), its count n and perturbation record(s) (8,) or (M, 8).

    Returns a dict: stats (M, 6) = max e_pos, max |e_y|, max |e_phi|, final position error, final |heading error|, 0;
    stat_rows (M, 2) = row of max e_pos, saturated rows; e_pos (M, n + settle) the position error at every row; cmd_max
    (M, n + settle) the unsaturated command m = max(|c_L|, |c_R|) of every row (the row is saturated when it is above the
    wheel limit); and with ``executed`` rows (M, n + settle, 8) and counts (M,).  Invalid records and n = 0 give NaN / -1 (counts 0)."""
    F = dtype
    rows = np.asarray(rows, dtype=np.float64)
    n = min(max(int(n), 0), rows.shape[0])
    P = np.atleast_2d(np.asarray(perturb, dtype=np.float64))
    M = len(P)
    settle, nsub = int(f["settle_rows"]), int(f["n_substeps"])
    total = n + settle if n > 0 else 0
    out = {"stats": np.full((M, 6), np.nan, dtype=F), "stat_rows": np.full((M, 2), -1, dtype=np.int64),
           "e_pos": np.full((M, total), np.nan, dtype=F), "cmd_max": np.full((M, total), np.nan, dtype=F)}
    if executed:
        out["rows"] = np.full((M, total, 8), np.nan, dtype=F)
        out["counts"] = np.zeros(M, dtype=np.int64)
    ok = record_valid(P)
    if n == 0 or not ok.any():
        return out
    p = P[ok].astype(F)
    m = len(p)
    R = rows.astype(F)
    T, b, zeta, wmax = F(f["track_width"]), F(f["b"]), F(f["zeta"]), F(f["wheel_speed_max"])
    dt = F(time_step)
    h = dt / nsub
    gl, gr, tau = p[:, 3], p[:, 4], p[:, 6]
    tts = T * p[:, 5]
    a = np.where(tau == 0, 1, 1 - np.exp(-h / np.where(tau == 0, 1, tau)))

    def ref(r):
        q = R[min(r, n - 1)]
        live = r < n
        return q[6], q[7], -q[4], (q[2] if live else F(0)), (-q[5] if live else F(0))

    x0, y0, ph0, v0, w0 = ref(0)
    x, y, phi = x0 + p[:, 0], y0 + p[:, 1], ph0 + p[:, 2]
    wl = np.full(m, v0 - w0 * T / 2, dtype=F)
    wr = np.full(m, v0 + w0 * T / 2, dtype=F)
    maxe, maxey, maxeph = np.full(m, -np.inf, dtype=F), np.full(m, -np.inf, dtype=F), np.full(m, -np.inf, dtype=F)
    mrow, nsat = np.full(m, -1, dtype=np.int64), np.zeros(m, dtype=np.int64)
    dist, vprev = np.zeros(m, dtype=F), np.zeros(m, dtype=F)
    epos_rows = np.zeros((m, total), dtype=F)
    cmd_rows = np.zeros((m, total), dtype=F)
    ex_rows = np.zeros((m, total, 8), dtype=F) if executed else None
    for r in range(total):
        xr, yr, phr, vr, wr_ = ref(r)
        # 1. errors in the body frame
        c, s = np.cos(phi), np.sin(phi)
        dx, dy = xr - x, yr - y
        ex, ey = c * dx + s * dy, c * dy - s * dx
        eph = wrap(phr - phi)
        epos = np.hypot(ex, ey)
        # 2. statistics
        up = epos > maxe
        maxe, mrow = np.where(up, epos, maxe), np.where(up, r, mrow)
        maxey = np.where(np.abs(ey) > maxey, np.abs(ey), maxey)
        maxeph = np.where(np.abs(eph) > maxeph, np.abs(eph), maxeph)
        epos_rows[:, r] = epos
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
        # 4. RAMSETE
        k = (2 * zeta) * np.sqrt(wr_ * wr_ + b * vr * vr)
        vc = vr * np.cos(eph) + k * ex
        wc = wr_ + k * eph + b * vr * sinc(eph) * ey
        cl, cr = vc - wc * T / 2, vc + wc * T / 2
        # 5. saturation, keeping c_L : c_R
        mx = np.maximum(np.abs(cl), np.abs(cr))
        sat = mx > wmax
        cmd_rows[:, r] = mx
        scale = np.where(sat, wmax / np.where(sat, mx, 1), 1)
        cl, cr = np.where(sat, cl * scale, cl), np.where(sat, cr * scale, cr)
        nsat = nsat + sat
        # 6. substeps: first-order wheel lag, then the exact arc
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
    # 7. final errors against row n - 1
    xl, yl, phl = R[n - 1, 6], R[n - 1, 7], -R[n - 1, 4]
    have = mrow >= 0
    nan = F(np.nan)
    st = np.stack([np.where(have, maxe, nan), np.where(have, maxey, nan), np.where(have, maxeph, nan),
                   np.where(have, np.hypot(xl - x, yl - y), nan), np.where(have, np.abs(wrap(phl - phi)), nan),
                   np.zeros(m, dtype=F)], axis=1)
    out["stats"][ok] = st
    out["stat_rows"][ok] = np.stack([mrow, np.where(have, nsat, -1)], axis=1)
    out["e_pos"][ok] = epos_rows
    out["cmd_max"][ok] = cmd_rows
    if executed:
        out["rows"][ok] = ex_rows
        out["counts"][ok] = total
    return out


def route_summary(stats, stat_rows, tolerance):
    """The per-route outputs from one route's (K, 6) stats and (K, 2) stat rows: worst (the smallest k on a tie), mean
    (summed in ascending k), worst_rollout, worst_row, n_exceeding; NaN / -1 / 0 without a valid rollout."""
    worst, wk, wrow, total, cnt, nex = -np.inf, -1, -1, stats.dtype.type(0), 0, 0
    for k in range(len(stats)):
        if stat_rows[k, 0] < 0:
            continue
        e = stats[k, 0]
        if e > worst:
            worst, wk, wrow = e, k, int(stat_rows[k, 0])
        total = total + e
        cnt += 1
        nex += int(e > tolerance)
    if cnt == 0:
        return dict(worst=np.nan, mean=np.nan, worst_rollout=-1, worst_row=-1, n_exceeding=0)
    return dict(worst=worst, mean=total / cnt, worst_rollout=wk, worst_row=wrow, n_exceeding=nex)


def golden_rows(g):
    """The reference's own time-domain rows of a golden fixture, in the time-profile layout (n, 8)."""
    c = np.asarray(g["profile_coords"], dtype=np.float64).reshape(-1, 2)
    return np.stack([g["profile_times"], g["profile_positions"], g["profile_linear_vels"], g["profile_accelerations"],
                     g["profile_headings"], g["profile_angular_vels"], c[:, 0], c[:, 1]], axis=1).astype(np.float64)
