"""CPU: the closest-point C-ABI is exported and declared, and the semantics the kernel must meet are pinned against the
real reference's GUI search (tests/golden/closest, tools/gen_closest_golden.py; gui/path.py:658-727): a NumPy
restatement of the two passes — quirk Q6's clamp, min_dist carried into the fine pass, the first index winning —
gives every recorded parameter, and an independent EXACT reference is never farther than the GUI's answer."""
import functools
import os
import re

import numpy as np
import pytest

import closest_cases as cc
import closest_ref as cr
import path_families as pf
from oracle import oracle
from vexautonomousplanner_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vap_closest_points", "vap_route_closest")


def test_closest_entry_points_are_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "vap.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vap_[a-z_0-9]+)\s*\(", src))
    L = _lib.lib()
    for name in NEW:
        assert name in declared
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    assert re.search(r"#define\s+VAP_CLOSEST_GUI\s+0\b", src) and re.search(r"#define\s+VAP_CLOSEST_EXACT\s+1\b", src)
    assert _lib.closest_mode("gui") == 0 and _lib.closest_mode("EXACT") == 1
    with pytest.raises(ValueError):
        _lib.closest_mode("nearest")


def test_fixtures_cover_the_issue_cases():
    names = cr.cases()
    for want in ("plain_w2", "plain_w5", "plain_w8", "plain_w32", "c1_w8", "feat_reverse", "feat_turn", "feat_tangent",
                 "feat_mixed"):
        assert want in names
    for n in names:
        assert os.path.getsize(os.path.join(cr.CLOSEST, n + ".npz")) < 64 * 1024
        c, _ = cr.load_case(n)
        assert len(c["parameter"]) >= 90 and set(np.unique(c["kind"])) >= {0, 1, 2, 3}


@pytest.mark.parametrize("name", cr.cases())
def test_numpy_restatement_reproduces_the_gui_parameters(name):
    c, g = cr.load_case(name)
    path = cr.RefPath(g)
    # the fixture's recorded point is the reference's get_point_at_parameter: the restated evaluator agrees
    np.testing.assert_allclose(path.point(c["parameter"]), c["point_ft"], rtol=0, atol=1e-12)
    for i, q in enumerate(c["query_ft"]):
        t, d = cr.gui_search(path, q)
        if c["gap"][i] > 1e-10:
            assert t == c["parameter"][i], (i, t, c["parameter"][i])
        else:   # a tie to rounding: the same distance
            p = c["point_ft"][i]
            assert abs(d - np.hypot(p[0] - q[0], p[1] - q[1])) <= 1e-10


def test_restatement_keeps_min_dist_and_first_index():
    """A query on the first node: the coarse pass's first candidate is exact and no fine candidate is strictly closer.
    A query beyond the end: quirk Q6's clamp maps many percents to W-1 and the first of them wins."""
    c, g = cr.load_case("plain_w8")
    path = cr.RefPath(g)
    q = path.point([0.0])[0]
    t, d = cr.gui_search(path, q)
    assert t == 0.0 and d == 0.0
    p_end = path.point([float(path.W - 1)])[0]
    t, _ = cr.gui_search(path, p_end + 5 * (p_end - path.point([path.W - 1.2])[0]))
    assert t == float(path.W - 1)


@pytest.mark.parametrize("name", cr.cases())
def test_exact_reference_is_never_farther_than_the_gui(name):
    c, g = cr.load_case(name)
    path = cr.RefPath(g)
    for i, q in enumerate(c["query_ft"]):
        p = c["point_ft"][i]
        dg = float(np.hypot(p[0] - q[0], p[1] - q[1]))
        te, de = cr.exact_search(path, q)
        assert de <= dg + 1e-12, (i, de, dg)
        if c["kind"][i] == 1:    # on the path at t0
            assert de <= 1e-9


# ---- the wide side (tests/test_gpu_closest_wide.py): arithmetic, the extended references, the seeds ---------------------


def test_segment_row_switch_and_lds_arithmetic():
    """The byte counts on either side of the switch, and why launch_closest never asks for more than the 64 KB any
    launch may have: staged rows (W <= 342) leave room for at most 341 splines, unstaged rows leave the spline table of
    the widest route alone."""
    src = open(os.path.join(ROOT, "vexautonomousplanner_amd", "csrc", "vap_closest.hip")).read()
    assert re.search(r"kClosestSegLdsBytes\s*=\s*32\s*\*\s*1024\s*;", src)
    assert re.search(r"kClosestQueriesPerBlock\s*=\s*4\s*\*\s*kClosestWaves\s*;", src) and re.search(r"kClosestThreads\s*=\s*256\s*;", src)
    assert re.search(r"kClosestMaxQueryBlocks\s*=\s*65535\s*;", src)
    assert cr.QUERIES_PER_BLOCK == 4 * (256 // 64) and cr.MAX_QUERY_BLOCKS == 65535
    for W, n in cr.SEG_BYTES.items():
        assert cr.seg_bytes(W) == n == 12 * 8 * (W - 1)
    assert cr.SEG_BYTES[342] <= cr.SEG_LDS_LIMIT < cr.SEG_BYTES[343]
    dev = open(os.path.join(ROOT, "vexautonomousplanner_amd", "csrc", "vap_device.h")).read()
    m = re.search(r"kSplineStride\s*=\s*(\d+)\s*;", dev)
    assert m and 8 * int(m.group(1)) == cr.SPLINE_ROW_BYTES
    allsrc = "".join(open(os.path.join(ROOT, "vexautonomousplanner_amd", "csrc", f)).read()
                     for f in os.listdir(os.path.join(ROOT, "vexautonomousplanner_amd", "csrc")) if f.endswith((".h", ".hip")))
    m = re.search(r"kMaxRouteWaypoints\s*=\s*(\d+)\s*;", allsrc)
    assert m and int(m.group(1)) == cr.MAX_ROUTE_WAYPOINTS
    assert cr.lds_request(342, 341) == 32736 + 10912 == 43648
    assert cr.lds_request(cr.MAX_ROUTE_WAYPOINTS, cr.MAX_ROUTE_WAYPOINTS - 1) == 47968          # "at most 48 KB"
    worst = max(cr.lds_request(W, W - 1) for W in range(2, cr.MAX_ROUTE_WAYPOINTS + 1))
    assert worst == 47968 <= cr.DEFAULT_LDS


@pytest.mark.parametrize("name", cr.cases())
def test_extended_gui_search_keeps_parameters_and_gives_the_recorded_gap(name):
    c, g = cr.load_case(name)
    path = cr.RefPath(g)
    for i, q in enumerate(c["query_ft"]):
        t, d, gap = cr.gui_search(path, q, gap=True)
        assert (t, d) == cr.gui_search(path, q)
        assert gap == c["gap"][i] or abs(gap - c["gap"][i]) <= 1e-12, (i, gap, c["gap"][i])
        if c["gap"][i] > 1e-10:
            assert t == c["parameter"][i]


@functools.lru_cache(maxsize=None)
def plain_refs(name):
    """Per path of a plain wide case on the oracle's segments: (path, q, kind, t0, [gui (t, d, gap)], [exact (t, d)])."""
    W, seed = cc.PLAIN_CASES[name]
    out = []
    for b, wp in enumerate(cc.plain_waypoints(name)):
        path = cr.path_of_oracle(oracle.OraclePath(wp))
        q, kind, t0 = cr.make_queries(path, wp, seed + b, **cc.WIDE_QUERIES)
        out.append((path, q, kind, t0, [cr.gui_search(path, x, gap=True) for x in q], [cr.exact_search(path, x) for x in q]))
    return out


def _tie_share(gaps, kind):
    gaps, kind = np.asarray(gaps), np.asarray(kind)
    plain = kind != cr.KIND_RETRACED
    assert np.all(gaps[~plain] <= cr.GAP_TIE), gaps[~plain]          # every deliberate tie is one
    return int((gaps[plain] <= cr.GAP_TIE).sum()), int(plain.sum())


@pytest.mark.parametrize("name", list(cc.PLAIN_CASES))
def test_wide_references_agree_and_later_lane_trips_decide(name):
    W, _ = cc.PLAIN_CASES[name]
    ties = total = 0
    winners = []
    for path, q, kind, t0, gui, ex in plain_refs(name):
        tg, pts, res = cr.brute_grid(path)
        assert res < 2e-3
        for i, x in enumerate(q):
            d_brute = float(np.hypot(pts[:, 0] - x[0], pts[:, 1] - x[1]).min())
            assert ex[i][1] <= gui[i][1] + 1e-12, (i, ex[i], gui[i])
            assert ex[i][1] <= d_brute + 1e-12, (i, ex[i], d_brute)
            assert d_brute <= ex[i][1] + res, (i, ex[i], d_brute, res)
            if kind[i] == cr.KIND_ON:
                assert ex[i][1] <= 1e-12
        a, n = _tie_share([g[2] for g in gui], kind)
        ties, total = ties + a, total + n
        winners += [int(e[0]) for e in ex]
    assert ties <= cr.TIE_SHARE_CAP * total, (ties, total)
    winners = np.array(winners)
    if W >= 65:
        assert ((winners >= 64) & (winners <= 127)).sum() >= 4
    if W >= 129:
        assert (winners >= 128).sum() >= 4
    if W == 343:
        assert (winners >= 256).sum() >= 4


def _oracle_nodes(W, rev, turn):
    import wide_ref
    return wide_ref._plain_nodes(W, is_reverse=np.asarray(rev, dtype=float), turn=np.asarray(turn, dtype=float))


@pytest.mark.parametrize("name", list(cc.ROUTE_CASES))
def test_route_cases_meet_the_tie_cap(name):
    wp, rev, turn = cc.route_case(name)
    W = wp.shape[1]
    ties = total = at_node = 0
    for b in range(len(wp)):
        op = oracle.OraclePath(wp[b], nodes=_oracle_nodes(W, rev[b], turn[b]))
        path = cr.path_of_oracle(op, rev[b], turn[b])
        assert op.n_splines == 1 + len(cr.split_nodes(W, rev[b], turn[b])) == cc.ROUTE_SPLINES[name][b]
        q, kind, t0 = cc.route_queries(path, wp[b], rev[b], turn[b], 50 + b)
        a, n = _tie_share([cr.gui_search(path, x, gap=True)[2] for x in q], kind)
        ties, total = ties + a, total + n
        assert (kind == cr.KIND_SPLIT).sum() >= 2
        at_node += sum(abs(cr.exact_search(path, x)[0] - t) <= 1e-9 for x, t in zip(q[kind == cr.KIND_SPLIT], t0[kind == cr.KIND_SPLIT]))
    assert ties <= cr.TIE_SHARE_CAP * total, (ties, total)
    assert at_node >= cc.ROUTE_AT_NODE_MIN[name], at_node          # queries beyond a reverse node are answered at the node itself


@pytest.mark.parametrize("W", cc.FAMILY_WIDTHS)
@pytest.mark.parametrize("family", pf.FAMILIES)
def test_family_cases_meet_the_tie_cap_and_retraced_queries_tie(family, W):
    wp = cc.family_waypoints(family, W)
    ties = total = retraced = 0
    for b in range(len(wp)):
        path = cr.path_of_oracle(oracle.OraclePath(wp[b]))
        q, kind, t0 = cc.family_queries(family, W, b, path, wp[b])
        a, n = _tie_share([cr.gui_search(path, x, gap=True)[2] for x in q], kind)
        ties, total = ties + a, total + n
        retraced += int((kind == cr.KIND_RETRACED).sum())
    assert ties <= cr.TIE_SHARE_CAP * total, (family, W, ties, total)
    assert retraced == (2 if family == "reversal" else 0)            # members 0 and 3 have factor 1


@pytest.mark.parametrize("Q", cc.BLOCK_QUERIES)
def test_block_cases_meet_the_tie_cap(Q):
    from vexautonomousplanner_amd.synth import make_waypoints
    B, W = cc.BLOCK_SHAPE
    wp = make_waypoints(B, W, cc.BLOCK_SEED).astype(np.float64)
    paths = [cr.path_of_oracle(oracle.OraclePath(w)) for w in wp]
    shared = cc.block_queries(paths[0], wp[0], Q, cc.BLOCK_SEED)[0]
    ties = total = 0
    for b in range(B):
        q, kind, _ = cc.block_queries(paths[b], wp[b], Q, cc.BLOCK_SEED + b)
        for qs in (q, shared):
            ties += sum(cr.gui_search(paths[b], x, gap=True)[2] <= cr.GAP_TIE for x in qs)
            total += len(qs)
        assert len(q) == Q
    assert ties <= cr.TIE_SHARE_CAP * total, (ties, total)


def test_revisited_node_ties_exactly_and_the_reference_takes_the_smaller_parameter():
    wp = cc.revisit_waypoints()[0]
    a, b = cc.REVISIT_NODE, cc.REVISIT_NODE + 64
    assert b < cc.REVISIT_W - 1 and a % 64 == b % 64                   # one lane's two trips
    path = cr.path_of_oracle(oracle.OraclePath(wp))
    assert np.array_equal(path.point([float(a)]), path.point([float(b)]))
    q, kind, t0 = cc.revisit_queries(path, wp)
    i = int(np.flatnonzero(kind == cr.KIND_RETRACED)[0])
    assert cr.exact_search(path, q[i]) == (float(a), 0.0)
    gaps = [cr.gui_search(path, x, gap=True)[2] for x in q]
    ties, total = _tie_share(gaps, kind)
    assert ties <= cr.TIE_SHARE_CAP * total


def test_config3_shaped_case_meets_the_tie_cap():
    """The four paths test_gpu_closest_wide.py holds to the references inside its B = 64, W = 32, Q = 64 batch."""
    from vexautonomousplanner_amd.synth import make_waypoints
    wp = make_waypoints(64, 32, 3).astype(np.float64)
    qs = np.random.default_rng(7).uniform(-6.05, 6.05, (64, 64, 2))
    ties = total = 0
    for b in (0, 21, 42, 63):
        path = cr.path_of_oracle(oracle.OraclePath(wp[b]))
        ties += sum(cr.gui_search(path, x, gap=True)[2] <= cr.GAP_TIE for x in qs[b])
        total += len(qs[b])
    assert ties <= cr.TIE_SHARE_CAP * total, (ties, total)
