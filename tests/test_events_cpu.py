"""The CPU restatement (oracle/vap_oracle.c) on the event edge routes of the REAL reference (tests/golden/events/,
oracle/gen_golden.py --events): action points at t = 0, on a node, on each other, unsorted, at and behind the end; stops
and waits on the end nodes; int(wait / dt); reverse at node 0 and on neighbours; turns of +-180, 360 and 0.5 degrees;
limits above the robot's and tiny ones; a segment shorter than dd; dt off 0.01.  Tolerances:
oracle/fuzz_vs_reference.py's own (velocity 1e-10 relative, profile rows 1e-8 relative with a floor of 1)."""
import numpy as np
import pytest

import events_util as eu
import golden_util as gu
from oracle import oracle

NAMES = eu.names()
CASES = ("plain ap_t0 ap_negative ap_on_node3 ap_on_node3_limits ap_same_t ap_close ap_unsorted ap_last_seg ap_at_end ap_beyond "
         "ap_wait_trunc stop_first_last wait_trunc wait_dt02 turn_wait_dt60 rev_node0 rev_consecutive rev_1_and_6 rev_ap_same_t "
         "turn_180 turn_m180 turn_360 turn_small turn_wait_rev turn_consecutive vmax_above vmax_tiny limits_node0 short_seg "
         "short_seg_plain dec_ne_acc_events w2_ap w3_rev1").split()


def _path(g):
    p = oracle.OraclePath(g["waypoints"], gu.node_dict(g), gu.action_dict(g))
    p.rebuild_tables()
    return p


def _ref_rows(g):
    cols = [g["profile_" + k] for k in ("times", "positions", "linear_vels", "accelerations", "headings", "angular_vels")]
    return np.column_stack(cols + [g["profile_coords"]]) if len(cols[0]) else np.zeros((0, 8))


def test_every_case_has_its_fixture():
    assert sorted(NAMES) == sorted(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_velocity_pass_matches_reference(name):
    g = eu.load(name)
    v = _path(g).forward_backward(g["constraints"], dd=float(g["dd"]))["velocity"]
    ref = g["velocity_row"]
    assert len(v) == len(ref) == int(g["n_samples"])
    err = np.max(np.abs(v - ref) / np.abs(ref))
    print(f"{name}: velocity {err:.2e}")
    assert err <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_motion_profile_matches_reference(name):
    g = eu.load(name)
    rows, nmap, amap = _path(g).generate_motion_profile(g["constraints"], dt=float(g["profile_dt"]), dd=float(g["profile_dd"]))
    ref = _ref_rows(g)
    assert rows.shape[0] == ref.shape[0]
    assert [int(v) for v in nmap] == [int(v) for v in g["profile_nodes_map"]]
    assert [int(v) for v in amap] == [int(v) for v in g["profile_actions_map"]]
    err = np.max(np.abs(rows - ref) / np.maximum(np.abs(ref), 1.0))
    print(f"{name}: rows {err:.2e}")
    assert err <= 1e-8


@pytest.mark.parametrize("name", NAMES)
def test_grid_walk_of_the_events(name):
    """eu.walk_events (MPG:112-165 restated over a parameter row) gives the same samples on the reference's stored
    parameters and on the oracle's, every parameter agrees, and the walk is the reference's: where it places a stop the
    reference's velocity row holds 0.01 or less, and an action point it never places has left no stop behind."""
    g = eu.load(name)
    W = len(g["waypoints"])
    ap_t = g["ap_t"] if "ap_t" in g.files else np.zeros(0)
    t_or = _path(g).forward_backward(g["constraints"], dd=float(g["dd"]))["t"]
    assert len(t_or) == len(g["t_row"])
    np.testing.assert_allclose(t_or, g["t_row"], rtol=1e-12, atol=1e-13)
    nodes, acts = eu.walk_events(g["t_row"], ap_t, W)
    assert (nodes, acts) == eu.walk_events(t_or, ap_t, W)
    assert nodes[0] == 0 and nodes[-1] == (eu.INT_MAX if W > 1 else 0)
    assert all(a < b for a, b in zip(nodes[:-1], nodes[1:-1]))
    v = g["velocity_row"]
    for k in range(1, W - 1):
        if g["node_stop"][k]:
            assert v[nodes[k]] <= 0.01 * (1 + 1e-12)
    for j, k in enumerate(acts):
        if k != eu.INT_MAX and g["ap_stop"][j]:
            assert v[k] <= 0.01 * (1 + 1e-12)
    # a stop that the walk says never happens has not happened: on an unsplit route (a cusp of a split one is as slow as a
    # stop) without a placed stop the interior of the row stays above 0.01
    placed = [nodes[k] for k in range(1, W - 1) if g["node_stop"][k]] + [k for j, k in enumerate(acts) if k != eu.INT_MAX and g["ap_stop"][j]]
    low = [int(i) for i in np.nonzero(v[1:-1] <= 0.01 * (1 + 1e-12))[0] + 1]
    assert set(placed) <= set(low) and (placed or not low or int(g["n_splines"]) > 1)


# ---- the reference outputs that make a case what it is: a regenerated fixture that lost its edge fails here ----
def _maps(name):
    g = eu.load(name)
    return [int(v) for v in g["profile_nodes_map"]], [int(v) for v in g["profile_actions_map"]]


@pytest.mark.parametrize("name", ["ap_t0", "ap_negative", "ap_at_end", "ap_beyond"])
def test_record_action_points_that_never_fire(name):
    """t <= 0 (prev_t starts at 0: prev_t < ap.t never holds, MPG:144, 549) and t >= W - 1 (every parameter of the loops is
    below it): never fired, and at t <= 0 the ones after it are blocked — the rows are the plain route's."""
    g, plain = eu.load(name), eu.load("plain")
    assert _maps(name)[1] == []
    assert _maps(name)[0] == _maps("plain")[0]
    np.testing.assert_array_equal(_ref_rows(g), _ref_rows(plain))
    np.testing.assert_array_equal(g["velocity_row"], plain["velocity_row"])


def test_record_stop_and_wait_on_the_end_nodes_do_nothing():
    g, plain = eu.load("stop_first_last"), eu.load("plain")
    assert _maps("stop_first_last") == _maps("plain")
    np.testing.assert_array_equal(_ref_rows(g), _ref_rows(plain))
    np.testing.assert_array_equal(g["velocity_row"], plain["velocity_row"])


@pytest.mark.parametrize("name", ["ap_same_t", "ap_close", "ap_unsorted", "rev_ap_same_t"])
def test_record_one_action_point_fires_and_blocks_the_rest(name):
    g = eu.load(name)
    assert len(_maps(name)[1]) == 1
    _, acts = eu.walk_events(g["t_row"], g["ap_t"], len(g["waypoints"]))
    assert sum(k != eu.INT_MAX for k in acts) == 1 and acts[0] != eu.INT_MAX


def test_record_action_point_on_a_node_fires_on_the_nodes_row():
    nmap, amap = _maps("ap_on_node3")
    assert amap == [nmap[3]]
    g = eu.load("ap_on_node3")
    nodes, acts = eu.walk_events(g["t_row"], g["ap_t"], 8)
    assert acts == [nodes[3]]                        # ... and on the node's sample of the distance grid
    g = eu.load("ap_on_node3_limits")
    nodes, acts = eu.walk_events(g["t_row"], g["ap_t"], 8)
    assert acts == [nodes[3]]
    nmap, amap = _maps("ap_on_node3_limits")
    assert amap == [nmap[3]]


def test_record_waits_truncate():
    """int(wait_time / dt): 0.29 -> 28 or 29 rows by the quotient's rounding, 0.3 -> 30 (29 if the quotient lands below),
    0.07 -> 7, 0.009 -> 0; an action point with a wait below dt still enters actions_map."""
    steps = lambda w, dt: int(w / dt)
    g, plain = eu.load("wait_trunc"), eu.load("plain")
    extra = sum(steps(w, 0.01) for w in (0.29, 0.3, 0.07, 0.009))
    assert steps(0.009, 0.01) == 0 and len(g["profile_times"]) == len(plain["profile_times"]) + extra
    g = eu.load("ap_wait_trunc")
    assert len(_maps("ap_wait_trunc")[1]) == 2
    assert len(g["profile_times"]) == len(plain["profile_times"]) + steps(0.009, 0.01) + steps(0.29, 0.01)
    g = eu.load("wait_dt02")
    assert float(g["profile_dt"]) == 0.02
    assert np.sum(g["profile_linear_vels"] == 0) >= steps(0.3, 0.02) + steps(0.5, 0.02)


def test_record_short_segment_is_shorter_than_dd():
    g = eu.load("short_seg")
    assert float(g["spline0_segment_lengths"][3]) < float(g["dd"])
    np.testing.assert_array_equal(g["waypoints"], eu.load("short_seg_plain")["waypoints"])
    # one step of the distance grid passes nodes 3 AND 4, the wrap test (MPG:124) sees one node: from there on node_num
    # lags by one, the stop of node 4 lands where node 5 is passed and node 6 is never reached
    nodes, _ = eu.walk_events(g["t_row"], np.zeros(0), 8)
    t = g["t_row"]
    assert t[nodes[3] - 1] < 3.0 and t[nodes[3]] >= 4.0 and t[nodes[4] - 1] < 5.0 <= t[nodes[4]]
    assert nodes[6] == eu.INT_MAX and nodes[5] != eu.INT_MAX
    assert g["velocity_row"][nodes[4]] <= 0.01 * (1 + 1e-12)
    assert len(g["profile_nodes_map"]) == 7          # the time loop steps finer there and sees every node


def test_fixture_inputs_are_fp32_representable_and_small():
    import os
    total = 0
    for name in NAMES:
        g = eu.load(name)
        np.testing.assert_array_equal(g["waypoints"], g["waypoints"].astype(np.float32).astype(np.float64))
        assert int(g["n_samples"]) < 1000 and len(g["profile_times"]) < 900 and len(g["waypoints"]) <= 8
        size = os.path.getsize(os.path.join(eu.EVENTS, name + ".npz"))
        assert size < 128 * 1024
        total += size
    assert total < 3 * 1024 * 1024
