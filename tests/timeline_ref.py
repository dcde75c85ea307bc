"""Plain Python / NumPy fp64 statement of vap_routine_timeline (include/vap.h): the legs of a routine chained into one
timeline, [turn m] [leg m] [dwell m] per slot.  Imports nothing from the package.  Every operation is one IEEE double
operation in the order the header states, so the product is compared with it bit for bit.

The turn is MPG:319-346 motion_profile_angle over ODM:4-69 generate_trapezoidal_profile, inserted the way MPG:487-507
handle_turn does: a trapezoid (or triangle) of wheel speed on an arc of |angle| track_width / 2, the heading its
rectangle-rule running sum, the angular velocity the difference of the un-wrapped headings."""
import math

import numpy as np

BAD_ROUTE = 8
TRUNCATED = 2
INT_MAX = 2147483647
MAX_LEGS = 32
TWO_PI = 2 * math.pi


def wrap_delta(d):
    """(-pi, pi]: one step either way, as the header states it."""
    if d > math.pi:
        d -= TWO_PI
    if d <= -math.pi:
        d += TWO_PI
    return d


def turn_shape(angle, max_vel, max_acc, track_width, dt):
    """(t_acc, vpeak, total_time, rows) of the trapezoid for `angle` radians."""
    arc = abs(angle) * track_width / 2
    t_acc = max_vel / max_acc
    d_acc = 0.5 * max_acc * (t_acc * t_acc)
    vpeak = max_vel
    if 2 * d_acc > arc:
        t_acc = math.sqrt(arc / max_acc)
        vpeak = max_acc * t_acc
        total = 2 * t_acc
    else:
        total = 2 * t_acc + (arc - 2 * d_acc) / vpeak
    return t_acc, vpeak, total, int(math.ceil((total + dt) / dt))


def turn_block(h_front, angle, max_vel, max_acc, track_width, dt):
    """(headings, angular velocities) of handle_turn for `angle` radians from heading `h_front`."""
    t_acc, vpeak, total, n = turn_shape(angle, max_vel, max_acc, track_width, dt)
    half_tw = track_width / 2
    sign = -1.0 if angle > 0 else 1.0
    hs, ws = np.empty(n), np.empty(n)
    accum = prev = 0.0
    for j in range(n):
        tt = float(j) * dt
        if tt <= t_acc:
            vel = max_acc * tt
        elif tt <= total - t_acc:
            vel = vpeak
        else:
            vel = vpeak - max_acc * (tt - (total - t_acc))
        hh = accum / half_tw * sign
        raw = hh
        accum += vel * dt
        ws[j] = 0.0 if j == 0 else (raw - prev) / dt
        prev = raw
        while hh + h_front > math.pi:
            hh -= TWO_PI
        while hh + h_front < -math.pi:
            hh += TWO_PI
        hs[j] = h_front + hh
    return hs, ws


def dwell_steps(w, dt):
    """int(dwell / dt); NaN or <= 0: none; saturates at INT_MAX."""
    if not w > 0.0:
        return 0
    q = w / dt
    return int(q) if q < float(INT_MAX) else INT_MAX


def _usable(h):
    return math.isfinite(h) and abs(h) <= TWO_PI


def chain(rows, counts, legs, constraints, dt=0.01, dwell=None, start_heading=None, n_legs=None,
          turn_min=math.radians(1.0), capacity_out=None, rows_fill=np.nan):
    """rows (L, cap_in, 8), counts (L,) or (L, k), legs (R, M) -> dict of rows (R, capacity_out, 8), counts (R, 2),
    map (R, M, 3), seam (R, M, 3), flags (R,), total (R,): the rows an ample capacity holds.  Rows the call does not
    write keep `rows_fill`.  capacity_out None: just enough for the longest routine."""
    rows = np.asarray(rows, dtype=np.float64)
    counts = np.asarray(counts).reshape(len(rows), -1)[:, 0].astype(np.int64)
    legs = np.asarray(legs, dtype=np.int64)
    R, M = legs.shape
    L, cap_in = rows.shape[0], rows.shape[1]
    max_vel, max_acc, track_width = float(constraints[0]), float(constraints[1]), float(constraints[5])
    built = []
    for r in range(R):
        n = M if n_legs is None else min(max(int(n_legs[r]), 0), M)
        h0 = float("nan") if start_heading is None else float(start_heading[r])
        bad = not (math.isnan(h0) or _usable(h0))
        for m in range(n):
            li = int(legs[r, m])
            if li < 0 or li >= L or counts[li] <= 0:
                bad = True
                continue
            c = min(int(counts[li]), cap_in)
            for row in (rows[li, 0], rows[li, c - 1]):
                if not (_usable(float(row[4])) and math.isfinite(row[6]) and math.isfinite(row[7])):
                    bad = True
        mp = np.full((M, 3), -1, dtype=np.int64)
        seam = np.full((M, 3), np.nan)
        blocks = []
        if bad:
            built.append((BAD_ROUTE, n, 0, mp, seam, blocks))
            continue
        o, off = 0, 0.0
        h_front, front = h0, None          # front: (position, x, y) of the output row in front
        for m in range(n):
            li = int(legs[r, m])
            c = min(int(counts[li]), cap_in)
            leg = rows[li, :c]
            first, last = leg[0], leg[c - 1]
            fpos, fx, fy = front if front is not None else (0.0, float(first[6]), float(first[7]))
            mp[m, 0] = min(o, INT_MAX)
            h_end = h_front
            if not math.isnan(h_front):
                d = wrap_delta(float(first[4]) - h_front)
                if not abs(d) < turn_min:
                    hs, ws = turn_block(h_front, -d, max_vel, max_acc, track_width, dt)
                    t = np.zeros((len(hs), 8))
                    t[:, 0] = [float(o + j) * dt for j in range(len(hs))]
                    t[:, 1], t[:, 4], t[:, 5], t[:, 6], t[:, 7] = fpos, hs, ws, fx, fy
                    blocks.append((o, t))
                    o += len(hs)
                    h_end = float(hs[-1])
                seam[m, 0] = wrap_delta(float(first[4]) - h_end)
            seam[m, 1] = float(first[6]) - fx if front is not None else 0.0
            seam[m, 2] = float(first[7]) - fy if front is not None else 0.0
            mp[m, 1] = min(o, INT_MAX)
            b = leg.copy()
            b[:, 0] = leg[:, 0] + float(o) * dt
            b[:, 1] = leg[:, 1] + off
            blocks.append((o, b))
            o += c
            mp[m, 2] = min(o, INT_MAX)
            front = (float(last[1]) + off, float(last[6]), float(last[7]))
            nd = dwell_steps(float(dwell[r][m]), dt) if dwell is not None else 0
            blocks.append((o, ("dwell", nd, front, float(last[4]))))
            o += nd
            off = off + float(last[1])
            h_front = float(last[4])
        built.append((0, n, o, mp, seam, blocks))
    cap = capacity_out if capacity_out is not None else max([b[2] for b in built] + [0])
    out = {"rows": np.full((R, cap, 8), rows_fill, dtype=np.float64), "counts": np.zeros((R, 2), dtype=np.int32),
           "map": np.zeros((R, M, 3), dtype=np.int32), "seam": np.zeros((R, M, 3)), "flags": np.zeros(R, dtype=np.uint32),
           "total": np.zeros(R, dtype=np.int64)}
    for r, (flags, n, total, mp, seam, blocks) in enumerate(built):
        for o, b in blocks:
            if isinstance(b, tuple):
                _, nd, (pos, x, y), h = b
                k = max(min(nd, cap - o), 0)
                b = np.zeros((k, 8))
                b[:, 0] = [float(o + j) * dt for j in range(k)]
                b[:, 1], b[:, 4], b[:, 6], b[:, 7] = pos, h, x, y
            k = max(min(len(b), cap - o), 0)
            out["rows"][r, o:o + k] = b[:k]
        out["counts"][r] = (min(total, cap), n)
        out["flags"][r] = flags | (TRUNCATED if total > cap else 0)
        out["map"][r], out["seam"][r], out["total"][r] = mp, seam, total
    return out


def arrival(out, dt):
    """(R, M) seconds at which each slot's site is reached (the first row of its dwell block), NaN for an unused slot."""
    m = out["map"][:, :, 2]
    return np.where(m >= 0, m.astype(np.float64) * dt, np.nan)


def duration(out, dt):
    """(R,) seconds, NaN for a bad routine."""
    return np.where(out["flags"] & BAD_ROUTE, np.nan, out["counts"][:, 0].astype(np.float64) * dt)
