"""GPU: k_closest where no test reached it (vap_closest_points / vap_route_closest), held to the NumPy references.

A  the segment-row switch (W = 342 staged in LDS, W = 343 read from global memory), both modes, both entry points
B  the lane-strided loops of EXACT mode on their second and third trips (W = 64, 65, 129)
C  routes of many splines: the linear walk of closest_spline_of, split nodes, arc length across spline offsets
D  query blocks: Q on either side of the 16 queries of a workgroup, per-path and shared queries, B > 1
E  a zero-length path inside a batch
F  structured geometry (tests/path_families.py): ties, degenerate boxes, +-1000 ft
G  the refusal of more queries than one launch holds

Every reference runs on the fp64 segment rows the kernel reads (the drop-in route's own device-fitted rows; the fit is
tested elsewhere), once per case and process, and is handed out unchanged.  The rules:

  GUI    where the reference's gap (closest_ref.gui_search) exceeds 1e-10 the parameter is EQUAL and point, distance
         and cross-track are the reference's evaluation to 1e-11; otherwise the distance is within 1e-10.  At most 5 % of a
         case's queries may take the tie branch (the deliberate ties apart, each of which must take it).
  EXACT  |distance - exact_search| <= tol = 1e-12 max(1, M / 8) (closest_ref.exact_tol); never farther than GUI mode;
         |cross_track| == distance; a query on the path gives distance <= tol and its parameter back to 1e-9 (or the same
         spot); distance_to_time(arc_length) gives the parameter back to 1e-12.
  The sign of a cross-track is compared with the reference's cross product at the returned parameter wherever that
  product exceeds 1e-11 |P'| in magnitude — below, the 1e-11 a point may move decides the sign, not the kernel.
"""
import numpy as np
import pytest

import closest_cases as cc
import closest_ref as cr
import path_families as pf

pytestmark = pytest.mark.gpu

OUTS = ("parameter", "point", "distance", "arc_length", "cross_track")
MODES = ("gui", "exact")
_CASES = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_gen(dtype):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    return BatchedTrajectoryGenerator(0, dtype)


def host(r):
    return {k: r[k].cpu().numpy() for k in OUTS + ("flags",)}


def manager(wp, rev=None, turn=None):
    from vexautonomousplanner_amd.nodes import Node
    from vexautonomousplanner_amd.splines.spline_manager import QuinticHermiteSplineManager
    W = len(wp)
    nodes = [Node(is_reverse_node=bool(rev[i]) if rev is not None else False, turn=float(turn[i]) if turn is not None else 0.0)
             for i in range(W)]
    m = QuinticHermiteSplineManager()
    assert m.build_path(np.asarray(wp, dtype=float), nodes, [])
    return m


class Case:
    """One batch of paths with its queries and references, built once: managers (the drop-in routes), RefPaths on their
    rows, queries (q, kind, t0) per path, gui [(t, d, gap)] and exact [(t, d)] per path, tol per path."""

    def __init__(self, wp, queries_of, rev=None, turn=None):
        self.wp = np.asarray(wp, dtype=np.float64)
        self.rev, self.turn = rev, turn
        B, W, _ = self.wp.shape
        self.man = [manager(self.wp[b], None if rev is None else rev[b], None if turn is None else turn[b]) for b in range(B)]
        self.path = [cr.path_of_route(m._route, W) for m in self.man]
        self.q, self.kind, self.t0 = zip(*[queries_of(b, self.path[b], self.wp[b]) for b in range(B)])
        self._gui = {}
        self._ex = {}

    def gui(self, b, q=None):
        return self._refs(self._gui, b, q, lambda p, x: cr.gui_search(p, x, gap=True))

    def exact(self, b, q=None):
        return self._refs(self._ex, b, q, cr.exact_search)

    def _refs(self, store, b, q, fn):
        key = (b, None if q is None else q.tobytes())
        if key not in store:
            store[key] = [fn(self.path[b], x) for x in (self.q[b] if q is None else q)]
        return store[key]

    def tol(self, b, q=None):
        return cr.exact_tol(self.wp[b], self.q[b] if q is None else q)

    def profile(self, torch, gen, rows=None):
        wp = self.wp if rows is None else self.wp[rows]
        t = torch.tensor(wp, dtype=gen.tdtype, device=gen.device)
        if self.rev is None and self.turn is None:
            return gen.profile(t, samples=64)
        pick = (lambda a: a) if rows is None else (lambda a: np.asarray(a)[rows])
        return gen.profile_routes(t, node_reverse=pick(self.rev), node_turn=pick(self.turn), samples=64)


def case(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


class Worst:
    """The largest differences a test has seen, printed once at its end."""

    def __init__(self, group):
        self.group = group
        self.v = {}

    def see(self, name, x):
        self.v[name] = max(self.v.get(name, 0.0), float(x))

    def report(self, what):
        print(f"CLOSEST-WIDE {self.group} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(self.v.items())))


def sign_matters(cross, speed):
    return abs(cross) > 1e-11 * speed


def check_gui(c, b, out, q, kind, worst, ties):
    """One path's GUI outputs (a dict of arrays over its queries) under the gap rule; counts ties into `ties`."""
    path = c.path[b]
    for i, (t, d, gap) in enumerate(c.gui(b, q)):
        deliberate = kind is not None and kind[i] == cr.KIND_RETRACED
        if gap > cr.GAP_TIE:
            assert not deliberate, (b, i, gap)
            assert out["parameter"][i] == t, (b, i, out["parameter"][i], t, gap)
            p = path.point([t])[0]
            ct, cross, speed = cr.cross_track(path, t, q[i])
            e_p = np.abs(out["point"][i] - p).max()
            e_d = abs(out["distance"][i] - d)
            e_c = abs(out["cross_track"][i] - ct) if sign_matters(cross, speed) else abs(abs(out["cross_track"][i]) - d)
            worst.see("gui point", e_p); worst.see("gui distance", e_d); worst.see("gui cross-track", e_c)
            assert e_p <= 1e-11 and e_d <= 1e-11 and e_c <= 1e-11, (b, i, e_p, e_d, e_c)
        else:
            ties[1 if deliberate else 0] += 1
            e_d = abs(out["distance"][i] - d)
            worst.see("gui tie distance", e_d)
            assert e_d <= 1e-10, (b, i, out["distance"][i], d, gap)
        assert abs(out["cross_track"][i]) == out["distance"][i]
    ties[2] += len(q)


def check_tie_cap(ties, kinds):
    deliberate = sum(int((np.asarray(k) == cr.KIND_RETRACED).sum()) for k in kinds)
    assert ties[1] == deliberate, (ties, deliberate)                      # every deliberate tie took the tie branch
    assert ties[0] <= cr.TIE_SHARE_CAP * (ties[2] - deliberate), ties


def check_exact(c, b, ex, gui, q, kind, t0, worst, round_trip=True):
    """One path's EXACT outputs (dicts of arrays over its queries) against exact_search and the rules of the module."""
    path, m = c.path[b], c.man[b]
    tol = c.tol(b, q)
    np.testing.assert_array_equal(np.abs(ex["cross_track"]), ex["distance"])
    for i, (t_ref, d_ref) in enumerate(c.exact(b, q)):
        t, d = ex["parameter"][i], ex["distance"][i]
        assert d <= gui["distance"][i] * (1 + 1e-15) + 1e-15, (b, i, t, d, gui["parameter"][i], gui["distance"][i], t_ref, d_ref)
        worst.see("exact distance / tol", abs(d - d_ref) / tol)
        assert abs(d - d_ref) <= tol, (b, i, d, d_ref, tol)
        assert 0.0 <= t <= path.W - 1
        _, cross, speed = cr.cross_track(path, t, q[i])
        if sign_matters(cross, speed) and d > tol:
            assert (ex["cross_track"][i] > 0) == (cross > 0), (b, i, t, cross, ex["cross_track"][i])
        k = cr.KIND_BOX if kind is None else kind[i]
        if k in (cr.KIND_ON, cr.KIND_RETRACED, cr.KIND_LINE):
            assert d <= tol, (b, i, d, tol)
        if k == cr.KIND_ON:
            pp = path.point([t, t0[i]])
            assert abs(t - t0[i]) <= 1e-9 or np.hypot(*(pp[0] - pp[1])) <= tol, (b, i, t, t0[i])
        if k == cr.KIND_RETRACED:                                           # the smaller of the two coincident parameters
            assert t == t0[i] or abs(t - t0[i]) <= 1e-9, (b, i, t, t0[i])
        if k == cr.KIND_EXTENSION:
            assert t == t0[i] and abs(d - 2.0) <= tol, (b, i, t, d)
        if k == cr.KIND_SPLIT and abs(t - t0[i]) <= 1e-9:                   # the node itself: the earlier spline's tangent
            assert ex["cross_track"][i] > 0, (b, i, t, ex["cross_track"][i])
    if round_trip:
        m.build_lookup_table()
        for t, s in zip(ex["parameter"], ex["arc_length"]):
            e = abs(m.distance_to_time(s) - t)
            worst.see("arc-length round trip", e)
            assert e <= 1e-12, (b, t, s, e)


def check_dropin(c, b, mode, out, q):
    """The batch's row of path b equals the drop-in route's closest() bit for bit, its points vap_route_eval's."""
    rows = c.man[b]._route.closest(mode, q)
    assert np.array_equal(out["parameter"], rows[:, 0])
    assert np.array_equal(out["point"], rows[:, 1:3])
    assert np.array_equal(out["distance"], rows[:, 3])
    assert np.array_equal(out["arc_length"], rows[:, 4])
    assert np.array_equal(out["cross_track"], rows[:, 5])
    assert np.array_equal(out["point"], c.man[b].get_points_at_parameters(out["parameter"]))


def row(o, b):
    return {k: o[k][b] for k in OUTS}


def run_both_modes(torch, c, gen, group, what):
    """Batch and drop-in in both modes on the case's own queries, under every rule."""
    B = len(c.wp)
    r = c.profile(torch, gen)
    q = torch.tensor(np.stack(c.q), device=gen.device)
    o = {mode: host(gen.closest_points(r, q, mode=mode)) for mode in MODES}
    worst, ties = Worst(group), [0, 0, 0]
    for mode in MODES:
        assert np.array_equal(o[mode]["flags"], r["flags"].cpu().numpy())
        assert not (o[mode]["flags"] & 9).any()
        for b in range(B):
            check_dropin(c, b, mode, row(o[mode], b), c.q[b])
    for b in range(B):
        check_gui(c, b, row(o["gui"], b), c.q[b], c.kind[b], worst, ties)
        check_exact(c, b, row(o["exact"], b), row(o["gui"], b), c.q[b], c.kind[b], c.t0[b], worst)
    check_tie_cap(ties, c.kind)
    worst.report(what)
    return o


# -- A, B: plain wide paths ------------------------------------------------------------------------------------------
def plain_case(name):
    W, seed = cc.PLAIN_CASES[name]
    return case(name, lambda: Case(cc.plain_waypoints(name), lambda b, p, wp: cr.make_queries(p, wp, seed + b, **cc.WIDE_QUERIES)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["w342", "w343"])
def test_segment_row_switch(torch_mod, name, dtype):
    W = cc.PLAIN_CASES[name][0]
    assert (cr.seg_bytes(W) <= cr.SEG_LDS_LIMIT) == (name == "w342")
    c = plain_case(name)
    o = run_both_modes(torch_mod, c, make_gen(dtype), "A", f"{name} {dtype}")
    trips = np.concatenate([np.floor(o["exact"]["parameter"][b]) for b in range(len(c.wp))])
    assert (trips >= 256).sum() >= 4                                       # the last lane trips decide answers


@pytest.mark.parametrize("name", ["w64", "w65", "w129"])
def test_lane_stride(torch_mod, name):
    W = cc.PLAIN_CASES[name][0]
    c = plain_case(name)
    o = run_both_modes(torch_mod, c, make_gen("f64"), "B", name)
    trips = np.concatenate([np.floor(o["exact"]["parameter"][b]) for b in range(len(c.wp))])
    if W >= 65:
        assert ((trips >= 64) & (trips <= 127)).sum() >= 4
    if W >= 129:
        assert (trips >= 128).sum() >= 4


def test_exact_tie_inside_one_lane_takes_the_smaller_parameter(torch_mod):
    """Node 66 of this path is node 2 again: lane 2 of the node pass sees both (closest_cases.revisit_waypoints)."""
    c = case("revisit", lambda: Case(cc.revisit_waypoints(), lambda b, p, w: cc.revisit_queries(p, w)))
    o = run_both_modes(torch_mod, c, make_gen("f64"), "B", "revisit")
    i = int(np.flatnonzero(c.kind[0] == cr.KIND_RETRACED)[0])
    assert o["exact"]["parameter"][0, i] == float(cc.REVISIT_NODE) and o["exact"]["distance"][0, i] == 0.0


# -- C: routes with many splines -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.ROUTE_CASES))
def test_many_spline_routes(torch_mod, name):
    wp, rev, turn = cc.route_case(name)
    c = case(name, lambda: Case(wp, lambda b, p, w: cc.route_queries(p, w, rev[b], turn[b], 50 + b), rev=rev, turn=turn))
    for b, m in enumerate(c.man):
        assert m._route.n_splines == 1 + len(cr.split_nodes(wp.shape[1], rev[b], turn[b])) == cc.ROUTE_SPLINES[name][b]
    o = run_both_modes(torch_mod, c, make_gen("f64"), "C", name)
    # the split-node queries are answered at the node, where only the earlier spline's tangent gives the sign
    at_node = sum(int((np.abs(o["exact"]["parameter"][b] - c.t0[b]) <= 1e-9)[c.kind[b] == cr.KIND_SPLIT].sum()) for b in range(len(wp)))
    assert at_node >= cc.ROUTE_AT_NODE_MIN[name], at_node


# -- D: query blocks -------------------------------------------------------------------------------------------------
def block_case(Q):
    from vexautonomousplanner_amd.synth import make_waypoints
    B, W = cc.BLOCK_SHAPE
    wp = make_waypoints(B, W, cc.BLOCK_SEED).astype(np.float64)
    return case(("block", Q), lambda: Case(wp, lambda b, p, w: cc.block_queries(p, w, Q, cc.BLOCK_SEED + b)))


@pytest.mark.parametrize("Q", cc.BLOCK_QUERIES)
def test_query_blocks(torch_mod, Q):
    torch = torch_mod
    c = block_case(Q)
    B = len(c.wp)
    gen = make_gen("f64")
    shared = c.q[0]                                                        # path 0's queries, asked of every path
    r = c.profile(torch, gen)
    q_pp = torch.tensor(np.stack(c.q), device=gen.device)
    q_sh = torch.tensor(shared, device=gen.device)
    assert q_pp.shape == (B, Q, 2) and q_sh.shape == (Q, 2)
    o_pp = {m: host(gen.closest_points(r, q_pp, mode=m)) for m in MODES}
    o_sh = {m: host(gen.closest_points(r, q_sh, mode=m)) for m in MODES}
    o_ex = {m: host(gen.closest_points(r, q_sh[None].expand(B, Q, 2).contiguous(), mode=m)) for m in MODES}
    worst, ties = Worst("D"), [0, 0, 0]
    for m in MODES:
        for k in OUTS:
            assert o_sh[m][k].shape[:2] == (B, Q) and np.array_equal(o_sh[m][k], o_ex[m][k]), (m, k)
    for b in range(B):
        check_gui(c, b, row(o_pp["gui"], b), c.q[b], c.kind[b], worst, ties)
        check_exact(c, b, row(o_pp["exact"], b), row(o_pp["gui"], b), c.q[b], c.kind[b], c.t0[b], worst)
        check_gui(c, b, row(o_sh["gui"], b), shared, None, worst, ties)
        check_exact(c, b, row(o_sh["exact"], b), row(o_sh["gui"], b), shared, None, None, worst)
    assert ties[0] <= cr.TIE_SHARE_CAP * ties[2], ties
    for b in range(B):                                                     # the same path alone
        r1 = c.profile(torch, gen, rows=[b])
        for m in MODES:
            alone = host(gen.closest_points(r1, q_pp[b:b + 1].contiguous(), mode=m))
            alone_sh = host(gen.closest_points(r1, q_sh, mode=m))
            for k in OUTS:
                assert np.array_equal(alone[k][0], o_pp[m][k][b]), (m, k, b)
                assert np.array_equal(alone_sh[k][0], o_sh[m][k][b]), (m, k, b)
    worst.report(f"Q={Q}")


def test_config3_shaped_batch_against_the_references(torch_mod):
    """test_config3_batch_equals_chunks asserts that chunks agree; here four paths spread over such a batch (B = 64,
    W = 32, Q = 64, fp32 generator) are held to the references."""
    torch = torch_mod
    from vexautonomousplanner_amd.synth import make_waypoints
    B, W, Q, held = 64, 32, 64, (0, 21, 42, 63)
    wp = make_waypoints(B, W, 3).astype(np.float64)
    qs = np.random.default_rng(7).uniform(-6.05, 6.05, (B, Q, 2))
    c = case("config3", lambda: Case(wp[list(held)], lambda b, p, w: (qs[held[b]], np.full(Q, cr.KIND_BOX), np.full(Q, np.nan))))
    gen = make_gen("f32")
    r = gen.profile(torch.tensor(wp, dtype=gen.tdtype, device=gen.device), samples=64)
    o = {m: host(gen.closest_points(r, torch.tensor(qs, device=gen.device), mode=m)) for m in MODES}
    worst, ties = Worst("D"), [0, 0, 0]
    for i, b in enumerate(held):
        for m in MODES:
            check_dropin(c, i, m, row(o[m], b), qs[b])
        check_gui(c, i, row(o["gui"], b), c.q[i], c.kind[i], worst, ties)
        check_exact(c, i, row(o["exact"], b), row(o["gui"], b), c.q[i], c.kind[i], c.t0[i], worst, round_trip=False)
    assert ties[0] <= cr.TIE_SHARE_CAP * ties[2], ties
    worst.report("config-3 shape")


# -- E: a zero-length path in a batch --------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_zero_length_path_in_a_batch(torch_mod, shared):
    """profile() itself flags a path whose waypoints coincide, and closest_points starts from a copy of the result's
    flags: the bit is cleared in the result first, so that only k_closest's own atomicOr (from blockIdx.y == 0 alone;
    Q = 33 makes three query blocks) can set it again."""
    torch = torch_mod
    from vexautonomousplanner_amd import _lib
    c = block_case(33)
    gen = make_gen("f64")
    wp = c.wp.copy()
    wp[1] = wp[1, 0]                                                       # path 1: all waypoints equal
    q = c.q[0] if shared else np.stack(c.q)
    tq = torch.tensor(q, device=gen.device)
    assert (tq.shape[-2] + cr.QUERIES_PER_BLOCK - 1) // cr.QUERIES_PER_BLOCK == 3
    r = gen.profile(torch.tensor(wp, device=gen.device), samples=64)
    before = r["flags"].cpu().numpy()
    assert before[0] == 0 and before[2] == 0 and before[1] & _lib.FLAG_DEGENERATE        # profile()'s own verdict
    r["flags"].zero_()
    want = [0, _lib.FLAG_DEGENERATE, 0]
    o = {m: host(gen.closest_points(r, tq, mode=m)) for m in MODES}
    again = {m: host(gen.closest_points(r, tq, mode=m)) for m in MODES}
    assert not r["flags"].any().item()                                     # the result's own flags stay as they were
    for m in MODES:
        assert o[m]["flags"].tolist() == want and again[m]["flags"].tolist() == want, (o[m]["flags"], again[m]["flags"])
        for k in OUTS:
            assert np.isnan(o[m][k][1]).all() and np.isfinite(o[m][k][[0, 2]]).all(), (m, k)
            assert np.array_equal(again[m][k], o[m][k], equal_nan=True)
    r["flags"].copy_(torch.tensor(want, dtype=r["flags"].dtype, device=gen.device))     # a call that finds the bit set
    for m in MODES:
        assert host(gen.closest_points(r, tq, mode=m))["flags"].tolist() == want
    r2 = gen.profile(torch.tensor(wp[[0, 2]], device=gen.device), samples=64)
    tq2 = tq if shared else torch.tensor(q[[0, 2]], device=gen.device)
    for m in MODES:
        two = host(gen.closest_points(r2, tq2, mode=m))
        assert not two["flags"].any()
        for k in OUTS:
            assert np.array_equal(two[k], o[m][k][[0, 2]]), (m, k)
    # and paths 0 and 2 are right, not only equal: path 0 under its own references
    worst, ties = Worst("E"), [0, 0, 0]
    check_gui(c, 0, row(o["gui"], 0), c.q[0], c.kind[0], worst, ties)
    check_exact(c, 0, row(o["exact"], 0), row(o["gui"], 0), c.q[0], c.kind[0], c.t0[0], worst)
    worst.report(f"shared={shared}")


# -- F: structured geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", cc.FAMILY_WIDTHS)
@pytest.mark.parametrize("family", pf.FAMILIES)
def test_structured_geometry(torch_mod, family, W):
    """reversal, W = 5, member 0 is the case that found bracketed_root closing its bracket on a left end where g is
    exactly zero (the segment leaving an exact cusp): EXACT answered an on-path query 0.0175 ft off the path."""
    torch = torch_mod
    wp = cc.family_waypoints(family, W)
    c = case((family, W), lambda: Case(wp, lambda b, p, w: cc.family_queries(family, W, b, p, w)))
    B = len(wp)
    gen = make_gen("f64")
    r = c.profile(torch, gen)
    worst, ties = Worst("F"), [0, 0, 0]
    if family == "reversal":
        cusps = pf.reversal_cusps(B, W, cc.FAMILY_SEED)
        assert sum(int((k == cr.KIND_RETRACED).sum()) for k in c.kind) == sum(1 for p in cusps if p and p[1] == 1.0) == 2
    for b in range(B):                                                     # members differ in their number of queries
        q = torch.tensor(c.q[b], device=gen.device)
        o = {m: host(gen.closest_points(r, q, mode=m)) for m in MODES}
        for m in MODES:
            assert not o[m]["flags"].any()
            check_dropin(c, b, m, row(o[m], b), c.q[b])
        check_gui(c, b, row(o["gui"], b), c.q[b], c.kind[b], worst, ties)
        check_exact(c, b, row(o["exact"], b), row(o["gui"], b), c.q[b], c.kind[b], c.t0[b], worst)
        worst.see("tol", c.tol(b))
    check_tie_cap(ties, c.kind)
    worst.report(f"{family} W={W}")


# -- G: more queries than one launch ---------------------------------------------------------------------------------
def test_too_many_queries_are_refused_before_any_launch(torch_mod):
    torch = torch_mod
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd.synth import make_waypoints
    limit = cr.MAX_QUERY_BLOCKS * cr.QUERIES_PER_BLOCK
    Q = limit + 1
    gen = make_gen("f64")
    r = gen.profile(torch.tensor(make_waypoints(1, 4, 1).astype(np.float64), device=gen.device), samples=64)
    q = torch.empty((Q, 2), dtype=torch.float64, device=gen.device)       # never read: the refusal comes first
    with pytest.raises(_lib.VapError) as e:
        gen.closest_points(r, q)
    assert e.value.status == _lib.VAP_ERR_UNSUPPORTED
    assert f"Q={Q}" in str(e.value) and str(limit) in str(e.value)
    ok = gen.closest_points(r, q[:17].zero_())                            # the generator still serves the next call
    assert torch.isfinite(ok["distance"]).all().item()
