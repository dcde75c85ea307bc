"""Plain NumPy statement of vap_odometry_rollouts (include/vap.h): the RAMSETE follower of vap_tracking_rollouts steering on
a dead-reckoned estimate that range readings reset.  Imports nothing from the package; the wrap, sinc and record checks are
tracking_ref's, the reading's rules and its decision margin are range_ref's (``cast`` states them over all candidates of a
ray at once, and test_odometry_cpu.py holds it to range_ref.cast).

``rollouts`` walks every rollout of a batch side by side: every operation is elementwise over the lanes (route b, record k),
so a lane gets exactly what a call of its own gives.  ``dtype`` switches the arithmetic: np.float64 (what the kernel is compared
against) or np.longdouble (what the float64 run is compared against, to size the tolerance).

Per rollout it reports the smallest decision margin met: range_ref's reading margin of every true reading, and for a reading
that is taken | |z - t_hat| - gate |, |cos_hat - min_cos|, the distance of the expected origin from the box and the x-against-y
wall tie of the expected ray; and tracking's saturation margin | max(|c_L|, |c_R|) - wheel_speed_max | of every row.
"""
import numpy as np

import range_ref as rr
import tracking_ref as tr

IDEAL = np.array([1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0])
INF = np.inf


def record_valid(o):
    o = np.atleast_2d(np.asarray(o, dtype=np.float64))
    return np.isfinite(o).all(axis=1) & (o[:, 0] > 0) & (o[:, 1] > 0) & (o[:, 2] > 0) & (o[:, 4] > 0)


def rule(gate, min_cos=0.0, gain=1.0, every=1):
    return dict(gate=float(gate), min_cos=float(min_cos), gain=float(gain), every=int(every))


class PackedScene:
    """field (xmin, ymin, xmax, ymax) or None, the polygons' edges in candidate order and the circles, as arrays."""

    def __init__(self, field=None, polygons=(), circles=()):
        self.field = None if field is None else tuple(float(v) for v in field)
        a, e, face, el = [], [], [], []
        for k, verts in enumerate(polygons):
            v = np.asarray(verts, dtype=np.float64)
            for j in range(len(v)):
                a.append(v[j])
                e.append(v[(j + 1) % len(v)] - v[j])
                face.append(j)
                el.append(k)
        self.a = np.array(a, dtype=np.float64).reshape(-1, 2)
        self.e = np.array(e, dtype=np.float64).reshape(-1, 2)
        self.face = np.array(face, dtype=np.int64)
        self.el = np.array(el, dtype=np.int64)
        self.n_poly = len(polygons)
        self.circles = np.asarray(circles, dtype=np.float64).reshape(-1, 3)


def wall(ox, oy, ux, uy, field):
    """Rule 1 of vap_range_readings for rays (ox, oy) + t (ux, uy): dict of ok, t, cos, face, own (the corner tie and the
    origin's distance from the box, range_ref._wall's) and miss (the distance from the box of an origin outside it, else inf)."""
    n = ox.shape[0]
    if field is None:
        return dict(ok=np.zeros(n, dtype=bool), t=np.full(n, INF), cos=np.full(n, np.nan), face=np.zeros(n, dtype=np.int64),
                    own=np.full(n, INF), miss=np.full(n, INF))
    xmin, ymin, xmax, ymax = field
    with np.errstate(all="ignore"):
        inside = (ox >= xmin) & (ox <= xmax) & (oy >= ymin) & (oy <= ymax)
        tx = np.where(ux > 0, (xmax - ox) / ux, np.where(ux < 0, (xmin - ox) / ux, INF))
        ty = np.where(uy > 0, (ymax - oy) / uy, np.where(uy < 0, (ymin - oy) / uy, INF))
        fx, fy = np.where(ux > 0, 2, 0), np.where(uy > 0, 3, 1)
        y_side = ty < tx                                        # a tie: the x side
        t = np.where(y_side, ty, tx)
        cos = np.where(y_side, np.abs(uy), np.abs(ux))
        face = np.where(y_side, fy, fx)
        border = np.minimum(np.minimum(np.abs(ox - xmin), np.abs(xmax - ox)), np.minimum(np.abs(oy - ymin), np.abs(ymax - oy)))
        own = np.minimum(np.abs(tx - ty), border)
        own = np.where(np.isnan(own), INF, own)
        ok = inside & (t < INF)
    return dict(ok=ok, t=np.where(ok, t, INF), cos=cos, face=face, own=own, miss=np.where(~inside & np.isfinite(border), border, INF))


def cast(heading, x, y, sensor, scn, dtype=np.float64):
    """One sensor (8,) at N poses against the walls, polygons and circles of a PackedScene, by vap_range_readings' rules.
    Returns dict of (N,) arrays: status, face, element, t, cos (NaN for status 1 and 6), margin (range_ref.cast's)."""
    F = dtype
    heading, x, y = (np.asarray(v, dtype=F) for v in (heading, x, y))
    n = heading.shape[0]
    mx, my, bx, by, r_min, r_max, min_cos = (F(v) for v in sensor[:7])
    with np.errstate(all="ignore"):
        phi = -heading
        c, s = np.cos(phi), np.sin(phi)
        ox, oy = x + (c * mx - s * my), y + (s * mx + c * my)
        ux, uy = c * bx - s * by, s * bx + c * by
        w = wall(ox, oy, ux, uy, scn.field)
        T, COS, OWN = [w["t"][:, None]], [w["cos"][:, None]], [w["own"][:, None]]
        FACE, EL = [w["face"][:, None]], [np.full((n, 1), -1, dtype=np.int64)]
        miss_c, miss_t, miss_v = [np.isfinite(w["miss"])[:, None]], [np.zeros((n, 1), dtype=F)], [w["miss"][:, None]]
        if len(scn.a):
            ax, ay, ex, ey = (v.astype(F)[None, :] for v in (scn.a[:, 0], scn.a[:, 1], scn.e[:, 0], scn.e[:, 1]))
            oxc, oyc, uxc, uyc = ox[:, None], oy[:, None], ux[:, None], uy[:, None]
            den = uxc * ey - uyc * ex
            dx, dy = ax - oxc, ay - oyc
            t = (dx * ey - dy * ex) / den
            ww = (dx * uyc - dy * uxc) / den
            length = np.hypot(ex, ey)
            nz = den != 0
            ok = nz & (t >= 0) & (ww >= 0) & (ww <= 1)
            T.append(np.where(ok, t, INF))
            COS.append(np.abs(uxc * (ey / length) + uyc * (-ex / length)))
            OWN.append(np.minimum(np.minimum(ww, 1 - ww) * length, t))
            FACE.append(np.broadcast_to(scn.face[None, :], t.shape))
            EL.append(np.broadcast_to(scn.el[None, :], t.shape))
            miss_c.append(nz & ~ok & np.isfinite(t) & np.isfinite(ww))
            miss_t.append(t)
            miss_v.append(np.maximum(np.maximum(-ww * length, (ww - 1) * length), np.maximum(-t, 0.0)))
        if len(scn.circles):
            cx, cy, r = (scn.circles[:, i].astype(F)[None, :] for i in range(3))
            oxc, oyc, uxc, uyc = ox[:, None], oy[:, None], ux[:, None], uy[:, None]
            dx, dy = oxc - cx, oyc - cy
            b = dx * uxc + dy * uyc
            q = (dx * dx + dy * dy) - r * r
            disc = b * b - q
            sq = np.sqrt(np.where(disc >= 0, disc, 0.0))
            t1, t2 = -b - sq, -b + sq
            t = np.where(t1 < 0, t2, t1)
            ok = (disc >= 0) & (t >= 0)
            T.append(np.where(ok, t, INF))
            COS.append(np.abs(uxc * ((oxc + t * uxc) - cx) + uyc * ((oyc + t * uyc) - cy)) / r)
            OWN.append(np.minimum(np.minimum(sq, np.abs(t1)), np.abs(t2)))
            FACE.append(np.zeros(t.shape, dtype=np.int64))
            EL.append(np.broadcast_to(scn.n_poly + np.arange(len(scn.circles))[None, :], t.shape))
            root = np.sqrt(np.abs(disc))
            miss_c += [(disc < 0) & (-b >= -root), (disc >= 0) & (t < 0)]
            miss_t += [-b, np.zeros(t.shape, dtype=F)]
            miss_v += [root, -t]
        T, COS, OWN, FACE, EL = (np.concatenate(v, axis=1) for v in (T, COS, OWN, FACE, EL))
        miss_c, miss_t, miss_v = (np.concatenate(v, axis=1) for v in (miss_c, miss_t, miss_v))
        ar = np.arange(n)
        idx = np.argmin(T, axis=1)                       # the first of equal candidates: a later one needs a strictly smaller t
        best = T[ar, idx]
        has = best < INF
        second = np.partition(T, 1, axis=1)[:, 1] if T.shape[1] > 1 else np.full(n, INF)
        cos, own, face, el = COS[ar, idx], OWN[ar, idx], FACE[ar, idx], EL[ar, idx]
        matters = miss_c & (np.maximum(miss_t, 0.0) <= best[:, None] + rr.AMBIGUOUS)
        miss_m = np.min(np.where(matters, miss_v, INF), axis=1)
        bad = ~(np.isfinite(heading) & np.isfinite(x) & np.isfinite(y))
        status = np.where(bad, rr.BAD_POSE, np.where(~has, rr.NONE, np.where(best < r_min, rr.NEAR, np.where(
            best > r_max, rr.FAR, np.where(cos < min_cos, rr.OBLIQUE, rr.VALID)))))
        margin = np.minimum(miss_m, np.where(has, np.minimum(second - best, own), INF))
        thresholds = np.minimum(np.minimum(np.abs(best - r_min), np.abs(best - r_max)), np.abs(cos - min_cos))
        margin = np.where(has, np.minimum(margin, thresholds), margin)
        margin = np.where((status == rr.VALID) & (cos < rr.COS_EXCUSE), 0.0, margin)    # t carries the pose's rounding / cos
        margin = np.where(bad, INF, margin)
    none = bad | ~has
    return {"status": status, "face": np.where(none, 0, face), "element": np.where(none, -2, el),
            "t": np.where(none, np.nan, best), "cos": np.where(none, np.nan, cos), "margin": margin.astype(np.float64)}


def rollouts(rows, counts, f, perturb, odo, sensors=None, scene=None, reset=None, time_step=0.01, executed=False,
             estimates=False, dtype=np.float64):
    """rows (B, cap, 8), counts (B,), perturbation and odometry records (B, K, 8) or (K, 8), sensors (ns, 8) or None, scene a
    PackedScene, reset a ``rule`` dict.  Returns a dict: stats (B, K, 8), stat_rows (B, K, 4), worst, mean (B,), worst_rollout,
    worst_row, n_exceeding (B,), margin (B, K), decisions (B * K, T) (bit s: sensor s accepted, bit 8 + s: rejected, bit 16: the
    row is saturated), e_pos (B * K, T), and on request rows (B * K, T, 8), counts (B * K,), est_rows (B * K, T, 4), T = cap +
    settle_rows; NaN / -1 / 0 as the header's edges."""
    F = dtype
    rows = np.asarray(rows, dtype=np.float64)
    B, cap = rows.shape[:2]
    counts = np.clip(np.asarray(counts).reshape(B, -1)[:, 0], 0, cap).astype(np.int64)
    P = np.asarray(perturb, dtype=np.float64)
    O = np.asarray(odo, dtype=np.float64)
    K = P.shape[-2]
    P = np.broadcast_to(P, (B, K, 8)).reshape(B * K, 8)
    O = np.broadcast_to(O, (B, K, 8)).reshape(B * K, 8)
    settle, nsub = int(f["settle_rows"]), int(f["n_substeps"])
    Tmax = cap + settle
    L = B * K
    lane_b = np.repeat(np.arange(B), K)
    n_l = counts[lane_b]
    ok = tr.record_valid(P) & record_valid(O) & (n_l > 0)
    out = {"stats": np.full((L, 8), np.nan, dtype=F), "stat_rows": np.full((L, 4), -1, dtype=np.int64),
           "margin": np.full(L, INF), "decisions": np.zeros((L, Tmax), dtype=np.int64), "e_pos": np.full((L, Tmax), np.nan, dtype=F)}
    if executed:
        out["rows"] = np.full((L, Tmax, 8), np.nan, dtype=F)
        out["counts"] = np.zeros(L, dtype=np.int64)
    if estimates:
        out["est_rows"] = np.full((L, Tmax, 4), np.nan, dtype=F)
    ns = 0 if sensors is None else len(sensors)
    if ok.any():
        sel = np.nonzero(ok)[0]
        p, o, lb, n = P[sel].astype(F), O[sel].astype(F), lane_b[sel], n_l[sel]
        m = len(sel)
        total = n + settle
        R = rows.astype(F)
        T_, b_, zeta, wmax = F(f["track_width"]), F(f["b"]), F(f["zeta"]), F(f["wheel_speed_max"])
        dt = F(time_step)
        h = dt / nsub
        gl, gr, tau = p[:, 3], p[:, 4], p[:, 6]
        tts = T_ * p[:, 5]
        a = np.where(tau == 0, 1, 1 - np.exp(-h / np.where(tau == 0, 1, tau)))
        encl, encr, hscale, hdrift, rscale, rbias = (o[:, i] for i in range(6))

        def ref(r):
            q = R[lb, np.minimum(r, n - 1)]
            live = r < n
            return q[:, 6], q[:, 7], -q[:, 4], np.where(live, q[:, 2], F(0)), np.where(live, -q[:, 5], F(0))

        x0, y0, ph0, v0, w0 = ref(0)
        x, y, phi = x0 + p[:, 0], y0 + p[:, 1], ph0 + p[:, 2]
        hx, hy, hphi = x0.copy(), y0.copy(), ph0.copy()
        wl, wr = v0 - w0 * T_ / 2, v0 + w0 * T_ / 2
        ninf = lambda: np.full(m, -np.inf, dtype=F)
        maxe, maxey, maxeph, maxest, maxestph = ninf(), ninf(), ninf(), ninf(), ninf()
        mrow, nsat, nacc, nrej = np.full(m, -1, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        dist, vprev = np.zeros(m, dtype=F), np.zeros(m, dtype=F)
        margin = np.full(m, INF)
        dec = np.zeros((m, Tmax), dtype=np.int64)
        epos_rows = np.full((m, Tmax), np.nan, dtype=F)
        ex_rows = np.full((m, Tmax, 8), np.nan, dtype=F) if executed else None
        es_rows = np.full((m, Tmax, 4), np.nan, dtype=F) if estimates else None
        keep = lambda act, new, old: np.where(act, new, old)
        with np.errstate(all="ignore"):
            for r in range(int(total.max())):
                act = r < total
                xr, yr, phr, vr, wr_ = ref(r)
                ch, sh = np.cos(hphi), np.sin(hphi)
                mask = np.zeros(m, dtype=np.int64)
                # 1. resets
                if ns > 0 and r % reset["every"] == 0:
                    heading = -tr.wrap(phi)
                    for s in range(ns):
                        sen = sensors[s]
                        c = cast(heading, x, y, sen, scene, F)
                        margin = np.where(act, np.minimum(margin, c["margin"]), margin)
                        read = act & (c["status"] == rr.VALID)
                        z = rscale * c["t"] + rbias
                        mx, my, bx, by = (F(v) for v in sen[:4])
                        eox, eoy = hx + (ch * mx - sh * my), hy + (sh * mx + ch * my)
                        eux, euy = ch * bx - sh * by, sh * bx + ch * by
                        w = wall(eox, eoy, eux, euy, scene.field)
                        diff = np.abs(z - w["t"])
                        accept = read & w["ok"] & (w["cos"] >= reset["min_cos"]) & (diff <= reset["gate"])
                        m_exp = np.minimum(w["miss"], np.where(w["ok"], np.minimum(np.minimum(
                            np.abs(diff - reset["gate"]), np.abs(w["cos"] - reset["min_cos"])), w["own"]), INF))
                        margin = np.where(read, np.minimum(margin, m_exp.astype(np.float64)), margin)
                        corr = F(reset["gain"]) * (w["t"] - z)
                        on_x = (w["face"] == 0) | (w["face"] == 2)
                        hx = np.where(accept & on_x, hx + corr * eux, hx)
                        hy = np.where(accept & ~on_x, hy + corr * euy, hy)
                        mask = mask | np.where(accept, 1 << s, 0) | np.where(read & ~accept, 1 << (8 + s), 0)
                        nacc = nacc + accept
                        nrej = nrej + (read & ~accept)
                # 2. errors: the true ones and the ones the follower sees
                c_, s_ = np.cos(phi), np.sin(phi)
                dx, dy = xr - x, yr - y
                ex, ey = c_ * dx + s_ * dy, c_ * dy - s_ * dx
                eph = tr.wrap(phr - phi)
                epos = np.hypot(ex, ey)
                hdx, hdy = xr - hx, yr - hy
                hex_, hey = ch * hdx + sh * hdy, ch * hdy - sh * hdx
                heph = tr.wrap(phr - hphi)
                eest = np.hypot(hx - x, hy - y)
                eestph = np.abs(tr.wrap(hphi - phi))
                # 3. statistics
                up = act & (epos > maxe)
                maxe, mrow = np.where(up, epos, maxe), np.where(up, r, mrow)
                maxey = np.where(act & (np.abs(ey) > maxey), np.abs(ey), maxey)
                maxeph = np.where(act & (np.abs(eph) > maxeph), np.abs(eph), maxeph)
                maxest = np.where(act & (eest > maxest), eest, maxest)
                maxestph = np.where(act & (eestph > maxestph), eestph, maxestph)
                epos_rows[:, r] = np.where(act, epos, np.nan)
                # 4. the executed row and the estimate row
                if executed:
                    v = (gl * wl + gr * wr) / 2
                    om = (gr * wr - gl * wl) / tts
                    row = np.stack([np.full(m, r * dt, dtype=F), dist, v, (v - vprev) / dt if r > 0 else np.zeros(m, dtype=F),
                                    -tr.wrap(phi), -om, x, y], axis=1)
                    ex_rows[:, r] = np.where(act[:, None], row, np.nan)
                    vprev = keep(act, v, vprev)
                if estimates:
                    row = np.stack([-tr.wrap(hphi), hx, hy, (mask & 255).astype(F)], axis=1)
                    es_rows[:, r] = np.where(act[:, None], row, np.nan)
                # 5. RAMSETE on the control errors
                k = (2 * zeta) * np.sqrt(wr_ * wr_ + b_ * vr * vr)
                vc = vr * np.cos(heph) + k * hex_
                wc = wr_ + k * heph + b_ * vr * tr.sinc(heph) * hey
                cl, cr = vc - wc * T_ / 2, vc + wc * T_ / 2
                # 6. saturation, keeping c_L : c_R
                mxc = np.maximum(np.abs(cl), np.abs(cr))
                sat = mxc > wmax
                margin = np.where(act, np.minimum(margin, np.abs(mxc - wmax).astype(np.float64)), margin)
                scale = np.where(sat, wmax / np.where(sat, mxc, 1), 1)
                cl, cr = np.where(sat, cl * scale, cl), np.where(sat, cr * scale, cr)
                nsat = nsat + (act & sat)
                dec[:, r] = np.where(act, mask | np.where(sat, 1 << 16, 0), 0)
                # 7. substeps: the plant's, then the estimate's
                for _ in range(nsub):
                    wl = keep(act, wl + (cl - wl) * a, wl)
                    wr = keep(act, wr + (cr - wr) * a, wr)
                    v = (gl * wl + gr * wr) / 2
                    om = (gr * wr - gl * wl) / tts
                    u = om * h / 2
                    d = v * h * tr.sinc(u)
                    x = keep(act, x + d * np.cos(phi + u), x)
                    y = keep(act, y + d * np.sin(phi + u), y)
                    phi = keep(act, phi + om * h, phi)
                    dist = keep(act, dist + np.abs(d), dist)
                    hv = (encl * (gl * wl) + encr * (gr * wr)) / 2
                    dl = (hscale * om) * h + hdrift * h
                    hu = dl / 2
                    hd = hv * h * tr.sinc(hu)
                    hx = keep(act, hx + hd * np.cos(hphi + hu), hx)
                    hy = keep(act, hy + hd * np.sin(hphi + hu), hy)
                    hphi = keep(act, hphi + dl, hphi)
            last = R[lb, n - 1]
            st = np.stack([maxe, maxey, maxeph, np.hypot(last[:, 6] - x, last[:, 7] - y), np.abs(tr.wrap(-last[:, 4] - phi)),
                           maxest, maxestph, np.hypot(hx - x, hy - y)], axis=1)
        out["stats"][sel] = st
        out["stat_rows"][sel] = np.stack([mrow, nsat, nacc, nrej], axis=1)
        out["margin"][sel] = margin
        out["decisions"][sel] = dec
        out["e_pos"][sel] = epos_rows
        if executed:
            out["rows"][sel] = ex_rows
            out["counts"][sel] = total
        if estimates:
            out["est_rows"][sel] = es_rows
    out["stats"] = out["stats"].reshape(B, K, 8)
    out["stat_rows"] = out["stat_rows"].reshape(B, K, 4)
    out["margin"] = out["margin"].reshape(B, K)
    summ = [tr.route_summary(out["stats"][b], out["stat_rows"][b], f["tolerance"]) for b in range(B)]
    for key in ("worst", "mean", "worst_rollout", "worst_row", "n_exceeding"):
        out[key] = np.array([s[key] for s in summ])
    return out
