"""Brute-force NumPy reference of the robot-to-robot clearance (include/vap.h, vap_footprint_conflicts), written from its
definitions on top of footprint_ref.posed and footprint_ref.polygon_clearance: every row of every pair is tested exactly,
no culling.

  poses      pose_a(r) = row min(r, n_a - 1) of a; pose_o(r) = row clamp(r - shift, 0, n_o - 1) of o; r = 0 .. T - 1,
             T = max(n_a, n_o + shift, 1); a pair with n_a == 0 or n_o == 0 is invalid (NaN, -1, -1)
  clearance  the polygon clearance between the two posed footprints (phi = -heading)
``pair_rows_direct`` poses both footprints in the field frame and calls polygon_clearance row by row: the definition to the
letter.  ``pair_rows`` is the same quantity for all rows at once: polygon_clearance takes one fixed second polygon, so side
A is posed in side O's body frame (a rigid motion, which changes no distance and no projection overlap; it costs a few
ulps of the coordinates, ~1e-15 ft).  The two agree to 1e-13 (tests/test_conflict_cpu.py).

Ambiguity gaps for the index outputs: rows whose two poses repeat an earlier row's exactly (parked or waiting robots) give
the same clearance by construction and the first of them is the answer, so gaps are taken over distinct pose pairs."""
import numpy as np

import footprint_ref as fr


def horizon(n_a, n_o, shift):
    return max(int(n_a), int(n_o) + int(shift), 1)


def pose_rows(rows_a, n_a, rows_o, n_o, shift):
    """(T, 3) poses (heading, x, y) of either side at the pair's rows (float64: the inputs are float64 numbers)."""
    r = np.arange(horizon(n_a, n_o, shift))
    a = np.asarray(rows_a, dtype=np.float64)[np.minimum(r, n_a - 1)][:, [4, 6, 7]]
    o = np.asarray(rows_o, dtype=np.float64)[np.clip(r - shift, 0, n_o - 1)][:, [4, 6, 7]]
    return a, o


def pair_rows_direct(rows_a, n_a, foot_a, rows_o, n_o, foot_o, shift=0, ftype=np.float64):
    """(T,) clearances of one valid pair, each row in the field frame."""
    a, o = pose_rows(rows_a, n_a, rows_o, n_o, shift)
    PA = fr.posed(np.asarray(foot_a, dtype=np.float64), a[:, 0], a[:, 1], a[:, 2], ftype)
    PO = fr.posed(np.asarray(foot_o, dtype=np.float64), o[:, 0], o[:, 1], o[:, 2], ftype)
    return np.array([fr.polygon_clearance(PA[i:i + 1], PO[i], ftype)[0] for i in range(len(a))])


def relative_clearance(a, o, foot_a, foot_o, ftype=np.float64):
    """(N,) clearances for N pose pairs a, o (N, 3): footprint A posed in O's body frame against footprint O.  A pair with a
    NaN in either pose is NaN."""
    a, o = np.asarray(a, dtype=ftype), np.asarray(o, dtype=ftype)
    dx, dy = a[:, 1] - o[:, 1], a[:, 2] - o[:, 2]
    c, s = np.cos(o[:, 0]), np.sin(o[:, 0])          # R(-phi_o) = R(heading_o)
    P = fr.posed(np.asarray(foot_a, dtype=np.float64), a[:, 0] - o[:, 0], c * dx - s * dy, s * dx + c * dy, ftype)
    v = fr.polygon_clearance(P, np.asarray(foot_o, dtype=np.float64), ftype)
    v[np.isnan(a).any(axis=1) | np.isnan(o).any(axis=1)] = np.nan
    return v


def pair_rows(rows_a, n_a, foot_a, rows_o, n_o, foot_o, shift=0, ftype=np.float64):
    a, o = pose_rows(rows_a, n_a, rows_o, n_o, shift)
    return relative_clearance(a, o, foot_a, foot_o, ftype)


def pair_summary(v, poses, margin):
    """min, first row at it, first row below margin, and the gaps that say whether those indices are well defined.  A row
    whose clearance is NaN takes part in nothing; without a finite row: NaN, -1, -1."""
    fin = ~np.isnan(v)
    if not fin.any():
        return dict(min=np.nan, row=-1, first=-1, row_gap=np.inf, row_gap_distinct=np.inf, margin_gap=np.inf, rows=v)
    w = np.where(fin, v, np.inf)
    r = int(np.argmin(w))
    below = np.nonzero(w < margin)[0]
    _, keep = np.unique(poses[fin], axis=0, return_index=True)
    srt = np.sort(v[fin][keep])
    dst = np.unique(v[fin])        # equal bits tie by construction (footprint_ref.summarise): the gap over distinct values
    return dict(min=v[r] if v.dtype != np.float64 else float(v[r]), row=r, first=int(below[0]) if len(below) else -1,
                row_gap=float(srt[1] - srt[0]) if len(srt) > 1 else np.inf,
                row_gap_distinct=float(dst[1] - dst[0]) if len(dst) > 1 else np.inf, margin_gap=float(np.min(np.abs(v[fin] - margin))),
                rows=v)


def conflicts(rows_a, counts_a, foot_a, rows_o, counts_o, foot_o=None, margin=0.0, shift=0, matched=False, ftype=np.float64):
    """Every output of vap_footprint_conflicts, plus per pair ``row_gap`` / ``margin_gap`` / ``rows`` and per route
    ``other_gap`` (best against runner-up pair) and ``margin_gap`` (the smallest over its pairs).  A pair without a finite
    clearance counts as an invalid pair."""
    foot_o = foot_a if foot_o is None else foot_o
    rows_a, rows_o = np.asarray(rows_a, dtype=np.float64), np.asarray(rows_o, dtype=np.float64)
    Ba, Bo = len(rows_a), len(rows_o)
    assert not matched or Ba == Bo
    P = 1 if matched else Bo
    out = dict(pair_clearance=np.full((Ba, P), np.nan, dtype=ftype), pair_row=np.full((Ba, P), -1), pair_first_row=np.full((Ba, P), -1),
               pair_row_gap=np.full((Ba, P), np.inf), pair_margin_gap=np.full((Ba, P), np.inf), pair_rows={},
               pair_row_gap_distinct=np.full((Ba, P), np.inf), other_gap_distinct=np.full(Ba, np.inf),
               min_clearance=np.full(Ba, np.nan, dtype=ftype), min_other=np.full(Ba, -1), min_row=np.full(Ba, -1),
               n_conflicts=np.zeros(Ba, dtype=int), first_row=np.full(Ba, -1), other_gap=np.full(Ba, np.inf),
               margin_gap=np.full(Ba, np.inf))
    for ia in range(Ba):
        n_a = int(np.clip(counts_a[ia], 0, rows_a.shape[1]))
        others = [ia] if matched else range(Bo)
        todo = [(io, int(np.clip(counts_o[io], 0, rows_o.shape[1]))) for io in others]
        todo = [(io, n_o) for io, n_o in todo if n_a > 0 and n_o > 0]
        if not todo:
            continue
        poses = [pose_rows(rows_a[ia], n_a, rows_o[io], n_o, shift) for io, n_o in todo]
        v_all = relative_clearance(np.concatenate([p[0] for p in poses]), np.concatenate([p[1] for p in poses]), foot_a, foot_o, ftype)
        at = 0
        mins = []
        for (io, n_o), (pa, po) in zip(todo, poses):
            s = pair_summary(v_all[at:at + len(pa)], np.concatenate([pa, po], axis=1), margin)
            at += len(pa)
            p = 0 if matched else io
            out["pair_clearance"][ia, p], out["pair_row"][ia, p], out["pair_first_row"][ia, p] = s["min"], s["row"], s["first"]
            out["pair_row_gap"][ia, p], out["pair_margin_gap"][ia, p] = s["row_gap"], s["margin_gap"]
            out["pair_row_gap_distinct"][ia, p] = s["row_gap_distinct"]
            out["pair_rows"][(ia, p)] = s["rows"]
            if s["row"] >= 0:
                mins.append((s["min"], io, s["row"], s["first"]))
        if not mins:
            continue
        best = min(mins)                                  # the smallest clearance, then the smallest other
        out["min_clearance"][ia], out["min_other"][ia], out["min_row"][ia] = best[0], best[1], best[2]
        out["n_conflicts"][ia] = sum(m[0] < margin for m in mins)
        firsts = [m[3] for m in mins if m[3] >= 0]
        out["first_row"][ia] = min(firsts) if firsts else -1
        srt = np.sort([m[0] for m in mins])
        out["other_gap"][ia] = srt[1] - srt[0] if len(srt) > 1 else np.inf
        dst = np.unique([m[0] for m in mins])
        out["other_gap_distinct"][ia] = dst[1] - dst[0] if len(dst) > 1 else np.inf
        out["margin_gap"][ia] = min(out["pair_margin_gap"][ia, 0 if matched else io] for io, _ in todo)     # +inf for a NaN pair
    return out
