"""NumPy statement of vap_search_sample and vap_search_update (include/vap.h) and a reference search loop whose evaluation
is the CPU oracle's generate_motion_profile and tests/footprint_ref.py.  The sampler and the refit run in ``ftype`` =
np.float64 or np.longdouble: the difference of the two is the reference's own rounding error."""
import numpy as np

import footprint_ref as fr

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI = 6.283185307179586
WEIGHTS = dict(w_time=1.0, w_length=1e-3, w_violation=1e3, infeasible_base=1e6, clearance_margin=0.05, conflict_margin=0.05,
               tracking_tolerance=0.25)


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter: 4 array-likes of uint32 (broadcast against each other), key: 2 -> 4 uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*counter)]
    k = [np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [x.astype(np.uint32) for x in c]


def normals(N, W, seed, iteration, problem, ftype=np.float64):
    """(N, W, 2) standard normals of one problem's candidates (row 0 is drawn too; the sampler does not use it)."""
    n, w = np.meshgrid(np.arange(N, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
    x = philox4x32_10((n, w, np.uint64(iteration & 0xFFFFFFFF), np.uint64(problem & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = (x[0].astype(ftype) + ftype(0.5)) * ftype(2.0 ** -32)
    u2 = (x[1].astype(ftype) + ftype(0.5)) * ftype(2.0 ** -32)
    rho = np.sqrt(ftype(-2.0) * np.log(u1))
    a = ftype(TWO_PI) * u2
    return np.stack([rho * np.cos(a), rho * np.sin(a)], axis=-1)


def sample(mean, sigma, N, dt, seed=0, iteration=0, first_problem=0, best_wp=None, best_cost=None, ftype=np.float64):
    """The candidates (R, N, W, 2): in ``ftype`` before the rounding to ``dt`` when ftype is np.longdouble, else as stored
    (``dt``).  Candidate 0 and pinned coordinates are exact either way."""
    mean, sigma = np.asarray(mean, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    R, W = mean.shape[:2]
    out = np.empty((R, N, W, 2), dtype=ftype)
    for r in range(R):
        z = normals(N, W, seed, iteration, first_problem + r, ftype)
        m, s = mean[r].astype(ftype), sigma[r].astype(ftype)
        out[r] = np.where(s[None] == 0, m[None], m[None] + s[None] * z)
        if best_wp is not None and best_cost is not None and np.isfinite(best_cost[r]):
            out[r, 0] = np.asarray(best_wp[r]).astype(ftype)
        else:
            out[r, 0] = mean[r].astype(dt).astype(ftype)
    return out if ftype is np.longdouble else out.astype(dt)


def costs(weights, counts=None, time_step=0.01, length=None, flags=None, clearance=None, conflict=None, tracking=None, B=None):
    """cost, violation, duration, length per candidate, the header's operations in the header's order (fp64)."""
    w = weights
    given = [a for a in (counts, length, flags, clearance, conflict, tracking) if a is not None]
    B = len(given[0]) if given else B
    bad, nan_term = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    dur, ln, viol = np.zeros(B), np.zeros(B), np.zeros(B)
    if counts is not None:
        c = np.asarray(counts, dtype=np.int64)
        bad |= c <= 0
        dur = c.astype(np.float64) * time_step
    if length is not None:
        ln = np.asarray(length, dtype=np.float64)
        bad |= np.isnan(ln)
    if flags is not None:
        bad |= np.asarray(flags) != 0
    with np.errstate(invalid="ignore"):
        for a, sign, ref in ((clearance, -1.0, w["clearance_margin"]), (conflict, -1.0, w["conflict_margin"]),
                             (tracking, 1.0, w["tracking_tolerance"])):
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                nan_term |= np.isnan(a)
                viol = viol + np.fmax(0.0, (ref - a) if sign < 0 else (a - ref))
        viol = np.where(nan_term, np.nan, viol)
        cost = w["w_time"] * dur + w["w_length"] * ln
        cost = np.where(viol > 0, cost + (w["infeasible_base"] + w["w_violation"] * viol), cost)
        cost = np.where(bad | nan_term | np.isnan(cost), np.inf, cost)
    return cost, viol, dur, ln


def update(wp, weights, E=1, alpha=1.0, sigma_min=0.0, sigma_max=np.inf, mean=None, sigma=None, best_cost=None, best_wp=None,
           best_terms=None, ftype=np.float64, time_step=0.01, **terms):
    """vap_search_update on candidates ``wp`` (R, N, W, 2) as stored.  ``terms``: counts, length, flags, clearance, conflict,
    tracking, each (R * N,).  Returns a dict; mean, sigma, best_* are new arrays (the inputs are not changed), the refit in
    ``ftype`` with sequential sums in rank order."""
    R, N, W = wp.shape[:3]
    cost, viol, dur, ln = costs(weights, time_step=time_step, B=R * N, **terms)
    out = {"cost": cost, "violation": viol, "order": np.empty((R, N), dtype=np.int64), "n_feasible": np.empty(R, dtype=np.int64),
           "elites": []}
    if mean is not None:
        out["mean"], out["sigma"] = np.array(mean, dtype=ftype), np.array(sigma, dtype=ftype)
    if best_cost is not None:
        out["best_cost"] = np.array(best_cost, dtype=np.float64)
        out["best_wp"] = None if best_wp is None else np.array(best_wp)
        out["best_terms"] = None if best_terms is None else np.array(best_terms, dtype=np.float64)
    for r in range(R):
        c, v = cost[r * N:(r + 1) * N], viol[r * N:(r + 1) * N]
        order = np.lexsort((np.arange(N), c))                    # by (cost, index); +inf last, no NaN by construction
        out["order"][r] = order
        out["n_feasible"][r] = int(np.sum(np.isfinite(c) & (v == 0)))
        ne = min(E, int(np.isfinite(c).sum()))
        elites = order[:ne]
        out["elites"].append(elites)
        if mean is not None and ne > 0:
            a = ftype(alpha)
            for w in range(W):
                for k in range(2):
                    sg = out["sigma"][r, w, k]
                    if sg == 0:
                        continue
                    vals = wp[r, elites, w, k].astype(ftype)
                    tot = ftype(0)
                    for x in vals:
                        tot = tot + x
                    me = tot / ftype(ne)
                    sq = ftype(0)
                    for x in vals:
                        sq = sq + (x - me) * (x - me)
                    var = sq / ftype(ne)
                    out["mean"][r, w, k] = (ftype(1) - a) * out["mean"][r, w, k] + a * me
                    s = np.sqrt((ftype(1) - a) * (sg * sg) + a * var)
                    out["sigma"][r, w, k] = min(max(s, ftype(sigma_min)), ftype(sigma_max))
        if best_cost is not None:
            top = int(order[0])
            if np.isfinite(c[top]) and c[top] < out["best_cost"][r]:
                out["best_cost"][r] = c[top]
                if out["best_wp"] is not None:
                    out["best_wp"][r] = wp[r, top]
                if out["best_terms"] is not None:
                    out["best_terms"][r] = (dur[r * N + top], ln[r * N + top], v[top], float(top))
    return out


def oracle_evaluate(foot, field=None, polygons=(), circles=(), constraints=None, dt=0.01, dd=0.005):
    """evaluate(wp (B, W, 2)) -> the terms of ``update`` for every candidate, from the oracle's generate_motion_profile (the
    reference pipeline for one route) and footprint_ref's per-row clearance.  A route the oracle refuses is flagged."""
    from oracle import oracle

    def evaluate(wp):
        B = len(wp)
        t = {"counts": np.zeros(B, dtype=np.int64), "length": np.zeros(B), "flags": np.zeros(B, dtype=np.int64),
             "clearance": np.full(B, np.nan)}
        for b in range(B):
            try:
                p = oracle.OraclePath(np.asarray(wp[b], dtype=np.float64))
                rows, _, _ = p.generate_motion_profile(constraints, dt=dt, dd=dd)
                t["length"][b] = p.total_arc_length()
            except ValueError:
                t["flags"][b] = 1
                t["clearance"][b] = 0.0
                continue
            t["counts"][b] = len(rows)
            t["clearance"][b] = fr.row_clearance(rows, foot, field, polygons, circles)[0].min() if len(rows) else 0.0
        return t
    return evaluate


def search(seed_wp, sigma0, evaluate, N=64, E=8, iterations=12, alpha=0.7, sigma_min=1e-3, sigma_max=2.0, seed=0,
           weights=WEIGHTS, dt=np.float64, time_step=0.01, first_problem=0):
    """The reference loop for R problems: seed_wp, sigma0 (R, W, 2).  Returns best_wp, best_cost, best_terms, history
    (R, iterations), n_feasible (R, iterations), mean, sigma."""
    mean, sigma = np.array(seed_wp, dtype=np.float64), np.array(sigma0, dtype=np.float64)
    R, W = mean.shape[:2]
    best_cost, best_wp, best_terms = np.full(R, np.inf), np.zeros((R, W, 2), dtype=dt), np.full((R, 4), np.nan)
    hist, nfe = np.full((R, iterations), np.inf), np.zeros((R, iterations), dtype=np.int64)
    for it in range(iterations):
        wp = sample(mean, sigma, N, dt, seed, it, first_problem, best_wp, best_cost)
        u = update(wp, weights, E, alpha, sigma_min, sigma_max, mean, sigma, best_cost, best_wp, best_terms,
                   time_step=time_step, **evaluate(wp.reshape(R * N, W, 2)))
        mean, sigma, best_cost, best_wp, best_terms = u["mean"], u["sigma"], u["best_cost"], u["best_wp"], u["best_terms"]
        hist[:, it], nfe[:, it] = best_cost, u["n_feasible"]
    return {"best_wp": best_wp, "best_cost": best_cost, "best_terms": best_terms, "history": hist, "n_feasible": nfe,
            "mean": mean, "sigma": sigma}
