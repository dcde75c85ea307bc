#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — closest-point fixtures from the real reference's GUI search.

Runs only where the reference tree is present (no-op elsewhere).  PathWidget.find_closest_point_on_path
(gui/path.py:658-727) lives on a PyQt6 widget, so the unmodified function is compiled at run time from the AST of
gui/path.py and called with a stub ``self`` that carries the two attributes it reads (``spline_manager``: the
reference's QuinticHermiteSplineManager built on the fixture's waypoints and node attributes; ``nodes``) and with
small QPointF / QPainterPath stand-ins (x, y / isEmpty, length).  Only the outputs are stored:

    tests/golden/closest/<case>.npz
      source            name of the tests/golden fixture the path comes from (waypoints, node attributes, segments)
      query_px          (n, 2) the query in pixels, as the GUI passes it
      query_ft          (n, 2) the query in feet, as the function converts it (gui/path.py:688)
      kind              (n,)   0 random field point, 1 on the path at t0, 2 beyond an end, 3 between two path parts,
                               4 off the field
      t0                (n,)   the parameter of an on-path query (NaN otherwise)
      parameter         (n,)   the returned closest_parameter
      point_px          (n, 2) the returned point (pixels, gui/path.py:725)
      point_ft          (n, 2) get_point_at_parameter(parameter) of the reference
      gap               (n,)   second-best minus best candidate distance over both passes (candidates at another
                               parameter than the winner's), feet: how far the query is from a tie

    python tools/gen_closest_golden.py
"""
import ast
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_util as gu  # noqa: E402
import refimport  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "closest")
FT_PER_FIELD = 12.1090395251            # gui/path.py:688, 725
CASES = {"plain_w2": "plain_w2_s0", "plain_w5": "plain_w5_s0", "plain_w8": "plain_w8_s0", "plain_w32": "plain_w32_s0",
         "c1_w8": "c1_w8", "feat_reverse": "feat_reverse", "feat_turn": "feat_turn", "feat_tangent": "feat_tangent",
         "feat_mixed": "feat_mixed"}


class QPointF:
    def __init__(self, x=0.0, y=0.0):
        self._x, self._y = float(x), float(y)

    def x(self):
        return self._x

    def y(self):
        return self._y


class QPainterPath:
    def __init__(self, length):
        self._length = length

    def isEmpty(self):
        return False

    def length(self):
        return self._length


class _Quiet:
    def info(self, *a, **k):
        pass


def gui_function():
    """find_closest_point_on_path, compiled from the reference's own source text."""
    path = os.path.join(refimport.REFERENCE_SRC, "gui", "path.py")
    tree = ast.parse(open(path).read(), path)
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == "find_closest_point_on_path":
            mod = ast.Module(body=[node], type_ignores=[])
            ns = {"np": np, "math": math, "logger": _Quiet(), "QPointF": QPointF, "QPainterPath": QPainterPath}
            exec(compile(mod, path, "exec"), ns)
            return ns["find_closest_point_on_path"]
    raise RuntimeError("find_closest_point_on_path not found in gui/path.py")


class Recorder:
    """The reference's manager, recording every (parameter, point) the search evaluates."""

    def __init__(self, mgr):
        self.mgr = mgr
        self.seen = []

    def percent_to_parameter(self, percent):
        return self.mgr.percent_to_parameter(percent)

    def get_point_at_parameter(self, t):
        p = self.mgr.get_point_at_parameter(t)
        self.seen.append((float(t), np.array(p, dtype=float)))
        return p


def node_attrs(g):
    W = len(g["waypoints"])
    out = []
    for i in range(W):
        a = dict(is_reverse_node=bool(g["node_is_reverse_node"][i]), turn=float(g["node_turn"][i]),
                 wait_time=float(g["node_wait_time"][i]), stop=bool(g["node_stop"][i]),
                 max_velocity=float(g["node_max_velocity"][i]), max_acceleration=float(g["node_max_acceleration"][i]))
        if not np.isnan(g["node_tangent"][i][0]):
            a["tangent"] = np.asarray(g["node_tangent"][i], dtype=float)
            a["incoming_magnitude"], a["outgoing_magnitude"] = (float(v) for v in g["node_magnitudes"][i])
        out.append(refimport.Node(**a))
    return out


def queries(mgr, W, rng):
    """~96 queries in feet with their kind and (on-path) t0."""
    q, kind, t0 = [], [], []
    for _ in range(44):
        q.append(rng.uniform(-6.0, 6.0, 2)); kind.append(0); t0.append(np.nan)
    for t in rng.uniform(0.0, W - 1, 24):
        q.append(np.asarray(mgr.get_point_at_parameter(float(t)), dtype=float)); kind.append(1); t0.append(float(t))
    p0, p1 = (np.asarray(mgr.get_point_at_parameter(t), dtype=float) for t in (0.0, float(W - 1)))
    d0, d1 = (np.asarray(mgr.get_derivative_at_parameter(t), dtype=float) for t in (0.0, float(W - 1)))
    for k in range(4):
        s = 0.2 + 0.4 * k
        q.append(p0 - s * d0 / max(np.linalg.norm(d0), 1e-12) + rng.normal(0, 0.05, 2)); kind.append(2); t0.append(np.nan)
        q.append(p1 + s * d1 / max(np.linalg.norm(d1), 1e-12) + rng.normal(0, 0.05, 2)); kind.append(2); t0.append(np.nan)
    for _ in range(12):
        ta, tb = rng.uniform(0.0, W - 1, 2)
        pa, pb = (np.asarray(mgr.get_point_at_parameter(float(t)), dtype=float) for t in (ta, tb))
        q.append(0.5 * (pa + pb)); kind.append(3); t0.append(np.nan)
    for _ in range(8):
        q.append(rng.uniform(-9.0, 9.0, 2)); kind.append(4); t0.append(np.nan)
    return np.array(q), np.array(kind, dtype=np.int32), np.array(t0)


def run_case(sm_mod, fn, case, source, seed):
    g = gu.load(source)
    wp = np.asarray(g["waypoints"], dtype=float)
    W = len(wp)
    nodes = node_attrs(g)
    mgr = sm_mod.QuinticHermiteSplineManager()
    assert mgr.build_path(wp.copy(), nodes, [])
    mgr.build_lookup_table()
    rng = np.random.default_rng(seed)
    q_ft_in, kind, t0 = queries(mgr, W, rng)
    rec = Recorder(mgr)
    stub = type("PathWidgetStub", (), {})()
    stub.spline_manager = rec
    stub.nodes = nodes
    path = QPainterPath(mgr.get_total_arc_length())
    n = len(q_ft_in)
    q_px, q_ft = np.empty((n, 2)), np.empty((n, 2))
    par, pt_px, pt_ft, gap = np.empty(n), np.empty((n, 2)), np.empty((n, 2)), np.empty(n)
    for i in range(n):
        px = (q_ft_in[i] / FT_PER_FIELD + 0.5) * 2000
        q_px[i] = px
        q_ft[i] = (np.array([px[0], px[1]]) / (2000) - 0.5) * FT_PER_FIELD      # gui/path.py:687-688
        rec.seen = []
        qp, t = fn(stub, path, QPointF(px[0], px[1]))
        par[i] = t
        pt_px[i] = (qp.x(), qp.y())
        pt_ft[i] = np.asarray(mgr.get_point_at_parameter(t), dtype=float)
        d = np.array([math.hypot(p[0] - q_ft[i][0], p[1] - q_ft[i][1]) for _, p in rec.seen])
        ts = np.array([tt for tt, _ in rec.seen])
        best = d.min()
        other = d[ts != t]
        gap[i] = (other.min() - best) if other.size else np.inf
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, case + ".npz"), source=np.array(source), query_px=q_px, query_ft=q_ft, kind=kind,
                        t0=t0, parameter=par, point_px=pt_px, point_ft=pt_ft, gap=gap)
    return n, int((gap <= 1e-10).sum())


def main():
    if not refimport.available():
        print("reference tree not present: nothing to do")
        return
    sm_mod, _, _ = refimport.load()
    fn = gui_function()
    for k, (case, source) in enumerate(CASES.items()):
        n, ties = run_case(sm_mod, fn, case, source, 1000 + k)
        print(f"{case:14s} {source:14s} {n} queries, {ties} within 1e-10 ft of a tie")


if __name__ == "__main__":
    main()
