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


def gui_search(path, q):
    """The two passes of gui/path.py:690-722 for one query q (feet): (parameter, min_dist)."""
    N = path.W
    steps = 25 * N
    pc = np.arange(steps + 1) / steps                  # i / num_steps, correctly rounded like Python's
    tc = gui_parameter(N, pc)
    pts = path.point(tc)
    d = np.hypot(pts[:, 0] - q[0], pts[:, 1] - q[1])
    ic = int(np.argmin(d))                              # strict '<' in a forward scan: the first index wins
    cd, cp, ct = d[ic], pc[ic], tc[ic]
    start, end = max(0.0, cp - 0.02), min(1.0, cp + 0.02)
    step = (end - start) / 500
    pf = start + np.arange(501) * step                  # start + i * step, no fused multiply-add
    tf = gui_parameter(N, pf)
    pts = path.point(tf)
    d = np.hypot(pts[:, 0] - q[0], pts[:, 1] - q[1])
    jf = int(np.argmin(d))
    if d[jf] < cd:                                      # min_dist carries over from the coarse pass
        return float(tf[jf]), float(d[jf])
    return float(ct), float(cd)


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
