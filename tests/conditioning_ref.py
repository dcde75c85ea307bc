"""Plain fp64 statement of vap_velocity_conditioning (include/vap.h): the literal sweep of MPG:188-311 in u = v^2 — the
arithmetic of sample_limits / forward_step / backward_step of vap_device.h, operation by operation, no fused multiply-add —
run on the rows as they are and on K perturbed copies, and the deviation of the copies from the first.

The per-sample limits do not depend on the state and are formed for a whole row at once with NumPy (element-wise IEEE
operations: the same bits as one sample at a time); the recurrence itself is a Python loop over floats.  Uses search_ref's
Philox; imports nothing from the package."""
import math

import numpy as np

import search_ref

TAG = 0x434F4E44
ILLCONDITIONED = 1024


def _pymin(a, b):
    """Python's min(a, b) on arrays: a unless b < a."""
    return np.where(b < a, b, a)


def limits(cons, kabs, cur_acc, cur_dec):
    """sample_limits of vap_device.h for a row: (q, cap_u, a_acc, a_dec, straight)."""
    vmax, tw = float(cons[0]), float(cons[5])
    amax = float(cons[1])
    wmax, almax = 2.0 * vmax / tw, 2.0 * amax / tw
    kabs = np.asarray(kabs, dtype=np.float64)
    cur_acc = np.broadcast_to(np.asarray(cur_acc, dtype=np.float64), kabs.shape)
    cur_dec = np.broadcast_to(np.asarray(cur_dec, dtype=np.float64), kabs.shape)
    q = kabs * kabs
    straight = kabs < 1e-6
    vtw = np.abs(vmax / (1.0 + (tw * kabs / 2.0)))
    cap_s = _pymin(np.full_like(kabs, vmax), vtw)
    with np.errstate(divide="ignore", invalid="ignore"):
        ks = np.where(straight, 1.0, kabs)                    # (the curved branch is not taken on a straight sample)
        max_vel_ang = wmax / ks
        max_vel_kin = 2.0 * vmax / (tw * ks + 2.0)
        mts = ((2.0 * vmax / tw) * vmax) / (ks * vmax + (2.0 * vmax / tw))
        mts = _pymin(mts, np.full_like(kabs, vmax))
        vl = _pymin(_pymin(max_vel_ang, max_vel_kin), mts)
        vl = _pymin(vl, vtw)
        a_ang = almax / ks
        a_acc = _pymin(_pymin(a_ang, 2.0 * cur_acc / (tw * ks + 2.0)), cur_acc)
        a_dec = _pymin(_pymin(a_ang, 2.0 * cur_dec / (tw * ks + 2.0)), cur_dec)
    cap_u = np.where(straight, cap_s * cap_s, vl * vl)
    a_acc = np.where(straight, cur_acc, a_acc)
    a_dec = np.where(straight, cur_dec, a_dec)
    return q, cap_u, a_acc, a_dec, straight


def _div(a, b):
    """IEEE a / b for floats (Python raises on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def sweep(kappa, dth, N, dd, cons, start_vel, end_vel, vcap=None, acc_fwd=None, acc_bwd=None, dec=None):
    """U[j], j < N: the squared velocities after the backward sweep (k_velocity_seq<literal>'s row before its square root)."""
    N = int(N)
    if N < 1:
        return []
    start_u, end_u = float(start_vel) * float(start_vel), float(end_vel) * float(end_vel)
    if N < 2:
        return [end_u]
    vmax, amax, tw = float(cons[0]), float(cons[1]), float(cons[5])
    adec = amax                                               # quirk Q9: max_dec is max_acc inside the pass
    twodd = 2.0 * float(dd)
    vmax2 = vmax * vmax
    kabs = np.abs(np.asarray(kappa, dtype=np.float64)[:N])
    dt = [float(x) for x in np.asarray(dth, dtype=np.float64)[:N]]
    fabs = math.fabs
    # forward, MPG:188-249
    cur = np.full(N, amax) if acc_fwd is None else np.asarray(acc_fwd, dtype=np.float64)[:N]
    q, cap_u, a_acc, _, straight = limits(cons, kabs, cur, cur if acc_fwd is not None else adec)
    q, cap_u, a_acc, straight, cur = q.tolist(), cap_u.tolist(), a_acc.tolist(), straight.tolist(), cur.tolist()
    if vcap is not None:
        vc = np.asarray(vcap, dtype=np.float64)[:N]
        un_row = (vc * vc).tolist()
    else:
        un_row = [vmax2] * N
    un_row[N - 1] = end_u
    u, wprev = start_u, 0.0
    V = [u]
    for i in range(N - 1):
        w = u * q[i]
        if straight[i]:
            a = a_acc[i]
        else:
            x = fabs(_div(w - wprev, 2.0 * dt[i])) * tw / 2.0
            c = cur[i]
            left, right = c + x, c - x
            aw = left if fabs(left) < fabs(right) else right
            if aw < 0.0:
                aw = 0.0
            a = a_acc[i]
            if aw < a:
                a = aw
            if c < a:
                a = c
        wprev = w
        nu = u + twodd * a
        o = un_row[i + 1]
        if nu < o:
            o = nu
        if cap_u[i] < o:
            o = cap_u[i]
        u = o
        V.append(u)
    # backward, MPG:251-311
    cur = np.full(N, amax) if acc_bwd is None else np.asarray(acc_bwd, dtype=np.float64)[:N]
    cur_dec = adec if dec is None else float(dec)
    q, cap_u, _, a_dec, straight = limits(cons, kabs, cur, cur_dec)
    q, cap_u, a_dec, straight, cur = q.tolist(), cap_u.tolist(), a_dec.tolist(), straight.tolist(), cur.tolist()
    U = [0.0] * N
    u, wprev = end_u, 0.0
    U[N - 1] = u
    for i in range(N - 1, 0, -1):
        w = u * q[i]
        if straight[i]:
            a = a_dec[i]
        else:
            x = _div(w - wprev, 2.0 * dt[i - 1]) * tw / 2.0
            c = cur[i]
            left, right = c + x, c - x
            aw = left if fabs(left) < fabs(right) else right
            if aw < 0.0:
                aw = 0.0
            a = a_dec[i]
            if aw < a:
                a = aw
        wprev = w
        o = u + twodd * a
        if V[i - 1] < o:
            o = V[i - 1]
        if cap_u[i] < o:
            o = cap_u[i]
        u = o
        U[i - 1] = u
    return U


def signs(N, k, seed, path):
    """(s, s') of samples 0 .. N-1 in probe k of path `path` (first_path + b), as +-1.0 arrays."""
    x = search_ref.philox4x32_10((np.arange(N, dtype=np.uint64), np.uint64(k), np.uint64(TAG), np.uint64(path & 0xFFFFFFFF)),
                                 (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (np.where(x[0] & 1, 1.0, -1.0), np.where(x[1] & 1, 1.0, -1.0))


def probe(kappa, dth, N, dd, cons, start_vel, end_vel, K=3, delta=2.0 ** -40, seed=0, path=0, limit=math.inf, S=None, **rows):
    """One path of vap_velocity_conditioning: dict(cond, worst_sample, worst_probe, flag, sensitivity (S,), velocity (S,),
    u0 (N,)).  kappa / dth: the rows already widened to fp64; rows: vcap, acc_fwd, acc_bwd, dec."""
    kappa, dth = np.asarray(kappa, dtype=np.float64), np.asarray(dth, dtype=np.float64)
    S = len(kappa) if S is None else S
    N = max(0, min(int(N), S))
    sens, vel = np.zeros(S), np.zeros(S)
    out = dict(cond=0.0, worst_sample=-1, worst_probe=-1, flag=0, sensitivity=sens, velocity=vel, u0=np.zeros(0))
    if N < 1:
        return out
    u0 = np.array(sweep(kappa, dth, N, dd, cons, start_vel, end_vel, **rows))
    out["u0"] = u0
    vel[:N] = np.sqrt(u0)
    if N < 2:
        return out
    R = np.zeros((K, N))
    for k in range(1, K + 1):
        s, sp = signs(N, k, seed, path)
        uk = np.array(sweep(kappa[:N] * (1.0 + s * delta), dth[:N] * (1.0 + sp * delta), N, dd, cons, start_vel, end_vel, **rows))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(u0 > 0, np.abs(uk - u0) / u0, np.where(u0 == 0, np.where(uk == 0, 0.0, np.inf), np.nan))
        R[k - 1] = np.where(r > 0, r, 0.0)                    # a maximum from 0.0 under a strict >: a NaN never wins
    sens[:N] = R.max(axis=0) / (2.0 * delta)
    best = R.max()
    if best > 0:
        j = int(np.argmax(R.max(axis=0) == best))             # the smallest sample among equals,
        k = int(np.argmax(R[:, j] == best)) + 1               # then the smallest probe
        out.update(cond=float(best / (2.0 * delta)), worst_sample=j, worst_probe=k)
    out["flag"] = ILLCONDITIONED if out["cond"] > limit else 0
    return out


def dtheta(heading):
    """|heading[i + 1] - heading[i]| with a 0 behind the last sample: the row the sweeps read (MPG:208, 268)."""
    h = np.asarray(heading, dtype=np.float64)
    return np.concatenate([np.abs(h[1:] - h[:-1]), [0.0]])
