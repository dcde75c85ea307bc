"""No GPU: what test_gpu_wide_routes.py takes from arithmetic and from the oracle (wide_ref.py), pinned here.

The byte counts that decide the three switches of the route pipeline at their boundary shapes, the event and skip
counts of the limit cases, the multi-node steps of the coarse-step case, the integers of every wait, and that every
wide reference finishes with finite rows — so none of the GPU tests' expectations comes from a kernel."""
import numpy as np
import pytest

import time_ref
import wide_ref as wr


def test_geometry_switch_bytes():
    """96 (W - 1) bytes of segment rows against 40 KB: W = 427 is the last width staged in LDS, 428 the first that is not."""
    assert wr.GEOMETRY_LDS_LIMIT == 40960
    assert wr.GEOMETRY_BYTES == {427: 40896, 428: 40992}
    for W, nbytes in wr.GEOMETRY_BYTES.items():
        assert wr.geometry_bytes(W) == nbytes == 8 * 12 * (W - 1)
    assert wr.GEOMETRY_BYTES[427] <= wr.GEOMETRY_LDS_LIMIT < wr.GEOMETRY_BYTES[428]
    assert set(wr.GEOMETRY_WIDTHS) == set(wr.GEOMETRY_BYTES)


def test_event_list_switch_bytes():
    """24 E + 16 bytes against 48 KB with E = max(W - 2, 0) + M: E = 2047 is the last list in LDS, 2048 the first outside."""
    assert wr.EVENT_LDS_LIMIT == 49152
    assert wr.EVENT_BYTES == {2047: 49144, 2048: 49168}
    for E, nbytes in wr.EVENT_BYTES.items():
        assert wr.event_bytes(E) == nbytes == (2 * 8 + 2 * 4) * E + 16
    assert wr.EVENT_BYTES[2047] <= wr.EVENT_LDS_LIMIT < wr.EVENT_BYTES[2048]
    want = {"w2048_m1": 2047, "w2048_m2": 2048, "w6_m2044": 2048}
    assert {n: wr.event_count(W, M) for n, (W, M, _) in wr.EVENT_CASES.items()} == want
    assert wr.event_count(2, 3) == 3 and wr.event_count(1, 0) == 0


def test_wait_kernel_bytes():
    """44 W + 12 M + 16 bytes of dynamic LDS and one static word against 64 KB and against a CDNA workgroup's 160 KB."""
    assert wr.WAITS_DEFAULT_LDS == 65536 and wr.CDNA_MAX_LDS == 163840 and wr.WAITS_STATIC_BYTES == 4
    assert wr.WAITS_BYTES == {(1488, 1): 65500, (1489, 1): 65544, (1500, 1): 66028, (2048, 1): 90140, (2048, 2): 90152,
                              (428, 1): 18860, (6, 20000): 240280}
    for (W, M), nbytes in wr.WAITS_BYTES.items():
        assert wr.waits_bytes(W, M) == nbytes == 44 * W + 12 * M + 16
    need = lambda W, M: wr.WAITS_BYTES[(W, M)] + wr.WAITS_STATIC_BYTES
    assert need(1488, 1) <= wr.WAITS_DEFAULT_LDS < need(1489, 1)
    assert max(need(1500, 1), need(2048, 1), need(2048, 2)) <= wr.CDNA_MAX_LDS < need(6, 20000)
    # every wait case of the GPU file has its request in the table (M = 1 each)
    assert {(W, 1) for W, _, _, _ in wr.WAIT_CASES.values()} <= set(wr.WAITS_BYTES)


def test_wait_integers():
    """int(wait_time / dt) of every wait the wide cases use, as Python gives it."""
    for w in wr.EDGE_WAITS:
        assert time_ref.WAIT_EDGE_STEPS[(w, wr.DT)] == int(w / wr.DT)
    assert [time_ref.WAIT_EDGE_STEPS[(w, wr.DT)] for w in wr.EDGE_WAITS] == [6, 2]      # (0.35 / 0.05 = 6.999...)
    for w, n in wr.COARSE_WAIT_STEPS.items():
        assert int(w / wr.COARSE_DT) == n and w / wr.COARSE_DT == float(n)
    assert wr.COARSE_WAIT_STEPS == {0.5: 2, 0.75: 3}


@pytest.mark.parametrize("W", wr.GEOMETRY_WIDTHS)
def test_geometry_references(W):
    """Plain paths and routes on both sides of the geometry switch: the oracle finishes, the rows are finite, every node
    but the last is recorded, the routes' rows hold reversed rows and a turn."""
    refs = wr.geometry_refs(W)
    assert len(refs) == wr.GEOMETRY_PATHS
    for rows, nmap in refs:
        assert 3000 < rows.shape[0] < 4000 and np.isfinite(rows).all() and len(nmap) == W - 1
        assert (np.diff(nmap) > 0).all()
    rev, turn = wr.geometry_route_nodes(W)
    assert (rev.sum(axis=1) == 1).all() and ((turn != 0).sum(axis=1) == 1).all() and not rev[:, [0, -1]].any()
    for b, (rows, nmap) in enumerate(wr.geometry_route_refs(W)):
        assert 3000 < rows.shape[0] < 4200 and np.isfinite(rows).all() and len(nmap) == W - 1
        assert (rows[:, 2] < 0).sum() > 100                        # rows behind the reverse node
        k = int(np.flatnonzero(turn[b])[0])
        r = int(nmap[k])
        assert rows[r, 2] == 0.0 and rows[r, 1] == rows[r - 1, 1]    # the turn's first row: in place


def test_limit_walk_on_a_small_route():
    """The walk that turns the oracle's sample parameters into samples and initial velocities, on a route small enough
    to check by eye: node 1 at the first sample past parameter 1, a stop there, the second action point blocked."""
    t = np.array([0.0, 0.4, 0.8, 1.2, 1.6, 2.0])
    mv = np.array([0.0, 2.0, 0.0])
    stop = np.array([False, True, False])
    v, nk, ak = wr.limit_walk(t, 3, 4.0, 0.01, mv, stop, np.array([0.5, 0.7, 1.5]), np.array([3.0, 1.0, 0.0]), np.array([0, 0, 0]))
    assert nk.tolist() == [0, 3, wr.NEVER] and ak.tolist() == [2, wr.NEVER, wr.NEVER]
    assert v.tolist() == [4.0, 4.0, 4.0, 0.01, 2.0, 0.01]          # sample 2 still holds the old limit; 3 the stop


@pytest.mark.parametrize("name", list(wr.EVENT_CASES))
def test_event_case_counts(name):
    """What the GPU test asserts on the reference before it asks the device, and the shape of every reference row."""
    c = wr.event_case(name)
    W, M, _ = wr.EVENT_CASES[name]
    for b in range(wr.EVENT_PATHS):
        N = len(c["velocity"][b])
        assert len(c["vcap"][b]) == N and np.isfinite(c["velocity"][b]).all() and (c["velocity"][b] > 0).all()
        assert c["node_sample"][b][0] == 0 and c["node_sample"][b][-1] == wr.NEVER
        assert (c["node_sample"][b][1:-1] != wr.NEVER).all() and (np.diff(c["node_sample"][b][:-1]) > 0).all()
        assert c["actions_reached"][b] + c["actions_skipped"][b] == M
        assert not c["node_stop"][b, 0] and not c["node_stop"][b, -1]
    if W == 2048:
        assert min(c["limited_events"]) >= 1000 and c["actions_skipped"] == [0, 0]
        assert all(26000 < len(v) < 27500 for v in c["velocity"])
    else:
        assert min(c["actions_reached"]) >= 1 and min(c["actions_skipped"]) >= 2000
    pinned = {"w2048_m1": ([1149, 1065], [1, 1], [0, 0]), "w2048_m2": ([1091, 1054], [2, 2], [0, 0]),
              "w6_m2044": ([5, 4], [4, 2], [2040, 2042])}[name]
    assert (c["limited_events"], c["actions_reached"], c["actions_skipped"]) == pinned


@pytest.mark.parametrize("name", list(wr.WAIT_CASES))
def test_wait_case_references(name):
    """Every wide wait reference finishes with finite rows; its row count is the bare route's plus the pinned integers;
    the action point's wait starts one kinematic row behind its node's wait; the coarse case passes several nodes in
    one step at least ten times."""
    c = wr.wait_case(name)
    W, dt = c["W"], c["dt"]
    steps = (lambda w: time_ref.WAIT_EDGE_STEPS[(w, dt)]) if dt == wr.DT else (lambda w: wr.COARSE_WAIT_STEPS[w])
    rows, nmap, amap = c["rows"], c["nodes_map"], c["actions_map"]
    assert np.isfinite(rows).all() and len(amap) == 1
    assert c["waits"][0] > 0 and c["waits"][-1] == 0 and 0.07 * W < (c["waits"] > 0).sum() < 0.13 * W
    assert not (c["waits"][c["turns"] != 0] > 0).any() and c["turns"][0] == 0
    if dt == wr.DT:
        assert c["multi_node_steps"] == 0 and c["nodes_recorded"] == W - 1 == len(nmap)
        inserted = sum(steps(w) for w in c["waits"] if w > 0) + steps(c["ap"][1])
        turn_rows = 0
        for k in np.flatnonzero(c["turns"]):
            r, n = int(nmap[k]), 0
            while rows[r + n, 1] == rows[r - 1, 1] and rows[r + n, 2] == 0.0:
                n += 1
            assert n > 3
            turn_rows += n
        # bare_rows holds the turns' rows already
        assert rows.shape[0] == c["bare_rows"] + inserted
        assert (turn_rows > 0) == (name == "route1500")
        k = c["ap_node"]
        assert int(amap[0]) == int(nmap[k]) + steps(c["waits"][k]) + 1
    else:
        assert c["multi_node_steps"] >= wr.COARSE_MULTI_NODE_STEPS_MIN and c["nodes_recorded"] < W - 1
        assert (np.diff(nmap) > 0).all()            # never two nodes on one row: the reference records one per step at most
    pinned = {"w1488": (12951, 1487), "w1489": (13042, 1488), "w2048": (17785, 2047), "route1500": (12950, 1499),
              "coarse428": (806, 384)}[name]
    assert (rows.shape[0], len(nmap)) == pinned
