"""Plain NumPy fp64 statement of vap_curve_caps and vap_drive_audit (include/vap.h): element-wise IEEE operations in the
order the header gives, one rounding each (NumPy never contracts a * b + c).  Imports nothing from the package."""
import math

import numpy as np


def _pymin(a, b):
    """Python's min(a, b) on arrays: a unless b < a."""
    return np.where(b < a, b, a)


def clamp_n(n, S):
    n = float(n)
    return 0 if not n >= 0.0 else (S if n > S else int(n))


def curvature_derivs(kappa, dd):
    """MPG:178-186 for the N samples of kappa: the two ends hold SUMS (the reference's own signs)."""
    k = np.asarray(kappa, dtype=np.float64)
    N = len(k)
    dk = np.empty(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        dk[0] = (k[1] + k[0]) / dd
        dk[N - 1] = (k[N - 1] + k[N - 2]) / dd
        dk[1:N - 1] = (k[2:] - k[:N - 2]) / (2.0 * dd)
    return dk


def caps(kappa, N, dd, max_vel, lateral=math.inf, angular=math.inf, vin=None, out_dtype=np.float64):
    """One path of vap_curve_caps.  kappa: the (S,) curvature row already widened to fp64; vin: the incoming row (S,) in its
    own type, or None (max_vel).  Returns (out (S,) of out_dtype, [n_lat, n_ang])."""
    k = np.asarray(kappa, dtype=np.float64)
    S = len(k)
    N = clamp_n(N, S)
    dd, max_vel = float(dd), float(max_vel)
    vin = np.full(S, max_vel) if vin is None else np.asarray(vin).astype(np.float64)
    out = vin.copy()
    if N == 0:
        return out.astype(out_dtype), [0, 0]
    kk, x = k[:N], vin[:N]
    ak = np.abs(kk)
    with np.errstate(divide="ignore", invalid="ignore"):
        cap_lat = np.where(ak > 0.0, np.sqrt(float(lateral) / np.where(ak > 0.0, ak, 1.0)), np.inf)
        cap_ang = np.full(N, np.inf)
        if N >= 2 and angular != math.inf:
            adk = np.abs(curvature_derivs(kk, dd))
            s = np.sqrt(float(angular) / adk)
            cap_ang = np.where(adk < 1e-9, max_vel, _pymin(s, np.full(N, max_vel)))     # MPG:45-50
        o = _pymin(_pymin(x, cap_lat), cap_ang)
        o = np.where(np.isnan(kk), np.nan, o)
        n_bound = [int(np.sum(cap_lat < x)), int(np.sum(cap_ang < x))]
    out[:N] = o
    return out.astype(out_dtype), n_bound


def wheel_rows(v, w, T, h):
    """{wL, wR, aL, aR, b, j, l, g} of rows with velocities v and angular velocities w: (n, 8)."""
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    n = len(v)
    T, h = float(T), float(h)
    with np.errstate(all="ignore"):
        half = (w * T) / 2.0
        wl, wr = v - half, v + half
        prev = lambda a: np.concatenate([[0.0], a[:-1]])
        al, ar = (wl - prev(wl)) / h, (wr - prev(wr)) / h
        b = (v - prev(v)) / h
        j = (b - prev(b)) / h
        l = v * w
        g = (w - prev(w)) / h
    return np.stack([wl, wr, al, ar, b, j, l, g], axis=1).reshape(n, 8)


def audit(v, w, n, T, h, limits):
    """One route of vap_drive_audit: v, w the (capacity,) columns 2 and 5, n the count (clamped here), limits the five in
    order.  Returns dict(peak (5,), peak_row (5,), n_over (5,), first_over (5,), status, wheel (n, 8) — (0, 8) for a route
    treated as empty)."""
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    n = max(0, min(int(n), len(v)))
    status = 0
    if n and not (np.isfinite(v[:n]).all() and np.isfinite(w[:n]).all()):
        status, n = 2, 0
    out = dict(peak=np.full(5, np.nan), peak_row=np.full(5, -1, dtype=np.int32), n_over=np.zeros(5, dtype=np.int32),
               first_over=np.full(5, -1, dtype=np.int32), status=status, wheel=np.zeros((0, 8)))
    if n == 0:
        return out
    wh = wheel_rows(v[:n], w[:n], T, h)
    out["wheel"] = wh
    a = np.abs(wh)
    pymax = lambda x, y: np.where(y > x, y, x)
    q = np.stack([pymax(a[:, 0], a[:, 1]), pymax(a[:, 2], a[:, 3]), a[:, 5], a[:, 6], a[:, 7]], axis=1)
    for i in range(5):
        col = q[:, i]
        ok = ~np.isnan(col)
        if ok.any():
            m = col[ok].max()
            out["peak"][i] = m
            out["peak_row"][i] = int(np.argmax(ok & (col == m)))
        over = col > float(limits[i])
        out["n_over"][i] = int(over.sum())
        out["first_over"][i] = int(np.argmax(over)) if over.any() else -1
    return out
