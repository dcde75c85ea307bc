"""GPU: every device layer on the event edge routes of the real reference (tests/golden/events/) —
the batched kernels (k_event_samples / k_event_merge / k_limit_fill, vap_time_profile_routes, vap_time_insert_events) in
f64 and f32, the one-lane vap_route_* layer behind the drop-in classes, and its batch switch.  The outputs checked are the
reference's decisions (MPG:112-165, 425-600): sample and row counts, nodes_map, actions_map, the sample at which every node
and action point takes effect — and every row.  The parametrisation is the directory listing: no case is skipped."""
import os
import sys

import numpy as np
import pytest

import events_util as eu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = eu.names()
ROW_KEYS = ("times", "positions", "linear_vels", "accelerations", "headings", "angular_vels")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def gens(torch_mod):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    return {k: BatchedTrajectoryGenerator(0, k) for k in ("f32", "f64")}


@pytest.fixture(scope="module")
def mods(torch_mod):
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    from motion_profiling_v2 import motion_profile_generator
    from splines.spline_manager import QuinticHermiteSplineManager
    from vexautonomousplanner_amd.nodes import ActionPoint, Node
    yield QuinticHermiteSplineManager, motion_profile_generator, Node, ActionPoint
    sys.path.remove(os.path.join(ROOT, "dropin"))


def cons_of(g):
    return [float(v) for v in g["constraints"]]


def expected_samples(g):
    ap_t = g["ap_t"] if "ap_t" in g.files else np.zeros(0)
    return eu.walk_events(g["t_row"], ap_t, len(g["waypoints"]))


def check_rows(g, rows, nmap, amap, tol, what):
    T = len(g["profile_times"])
    assert rows.shape[0] == T, (what, rows.shape[0], T)
    assert nmap == [int(v) for v in g["profile_nodes_map"]], what
    assert amap == [int(v) for v in g["profile_actions_map"]], what
    worst = 0.0
    for col, key in enumerate(ROW_KEYS):
        ref = g["profile_" + key]
        e = float(np.max(np.abs(rows[:, col] - ref) / np.maximum(np.abs(ref), 1.0)))
        worst = max(worst, e)
        assert e <= tol, (what, key, e)
    e_c = float(np.max(np.abs(rows[:, 6:8] - g["profile_coords"])))
    assert e_c <= tol, (what, "coords", e_c)
    return max(worst, e_c)


@pytest.mark.parametrize("dtype,tol,vtol", [("f64", 1e-8, 1e-9), ("f32", 1e-5, 1e-5)])
@pytest.mark.parametrize("name", NAMES)
def test_batched_layer_matches_reference(torch_mod, gens, name, dtype, tol, vtol):
    """profile_routes -> apply_node_limits -> time_profile -> insert_waits at the fixture's robot, dd and dt: sample count,
    the whole velocity row, the sample of every node and action point (INT_MAX where the reference never reaches it), row
    count, both maps, every row column and the coordinates."""
    g = eu.load(name)
    gen = gens[dtype]
    res, out = eu.run_chain(torch_mod, gen, [eu.route_of(g)] * 2, cons_of(g), dt=float(g["profile_dt"]), dd=float(g["profile_dd"]))
    assert not res["flags"].any().item()
    N = int(g["n_samples"])
    assert res["meta"][:, 3].tolist() == [N, N]
    v = res["velocity"][0, :N].cpu().numpy().astype(np.float64)
    e_v = float(np.max(np.abs(v - g["velocity_row"]) / g["velocity_row"]))
    nodes, acts = expected_samples(g)
    got_nodes = res["node_sample"][0].tolist()
    got_acts = res["action_sample"][0].tolist()
    rows, nmap, amap = eu.unpack(out, 0)
    print(f"EVENTS batched/{dtype} {name}: velocity {e_v:.2e} node_sample {got_nodes == nodes} action_sample {got_acts == acts} "
          f"count {rows.shape[0]}/{len(g['profile_times'])} maps {nmap == [int(x) for x in g['profile_nodes_map']]} "
          f"{amap == [int(x) for x in g['profile_actions_map']]}")
    assert got_nodes == nodes
    assert got_acts == acts
    assert e_v <= vtol, e_v
    e_r = check_rows(g, rows, nmap, amap, tol, name)
    print(f"EVENTS batched/{dtype} {name}: rows {e_r:.2e}")
    assert torch_mod.equal(out["rows"][0, :rows.shape[0]], out["rows"][1, :rows.shape[0]])
    assert torch_mod.equal(res["velocity"][0], res["velocity"][1])


def build_route(mods, g):
    Manager, _, Node, ActionPoint = mods
    nodes = []
    for i in range(len(g["waypoints"])):
        nodes.append(Node(is_reverse_node=bool(g["node_is_reverse_node"][i]), turn=float(g["node_turn"][i]),
                          wait_time=float(g["node_wait_time"][i]), stop=bool(g["node_stop"][i]),
                          max_velocity=float(g["node_max_velocity"][i]), max_acceleration=float(g["node_max_acceleration"][i])))
    aps = [ActionPoint(**a) for a in eu.action_points(eu.route_of(g))]
    m = Manager()
    assert m.build_path(g["waypoints"], nodes, aps) is True
    return m


@pytest.mark.parametrize("name", NAMES)
def test_one_lane_layer_and_its_batch_switch_match_reference(mods, name):
    """The drop-in generate_motion_profile(m, c, dt, dd) and forward_backward_pass through the one-lane vap_route_* layer
    (DeviceRoute.use_batch_kernels False) and through the batch kernels (True): each against the reference's 9-tuple and whole
    velocity row, and the two layers' counts and maps equal to each other."""
    _, mpg, _, _ = mods
    from vexautonomousplanner_amd._device_path import DeviceRoute
    g = eu.load(name)
    c = mpg.Constraints(*g["constraints"])
    dt, dd = float(g["profile_dt"]), float(g["profile_dd"])
    got = {}
    try:
        for layer in (False, True):
            DeviceRoute.use_batch_kernels = layer
            m = build_route(mods, g)
            res = mpg.generate_motion_profile(m, c, dt, dd)
            m.rebuild_tables()
            got[layer] = (res, np.array(mpg.forward_backward_pass(m, c, float(g["dd"]))))
    finally:
        DeviceRoute.use_batch_kernels = False
    T = len(g["profile_times"])
    for layer, (res, v) in got.items():
        tag = f"EVENTS {'switch' if layer else 'one-lane'} {name}"
        assert len(res) == 9
        ok = (len(res[0]) == T, res[6] == [int(x) for x in g["profile_nodes_map"]], res[7] == [int(x) for x in g["profile_actions_map"]],
              len(v) == int(g["n_samples"]))
        print(f"{tag}: count {len(res[0])}/{T} maps {ok[1]} {ok[2]} samples {len(v)}/{int(g['n_samples'])}")
        assert all(ok), (tag, ok)
        e_v = float(np.max(np.abs(v - g["velocity_row"]) / g["velocity_row"]))
        e_r = max(float(np.max(np.abs(np.array(res[k]) - g["profile_" + key]) / np.maximum(np.abs(g["profile_" + key]), 1.0)))
                  for k, key in enumerate(ROW_KEYS))
        e_c = float(np.max(np.abs(np.array(res[8]) - g["profile_coords"])))
        print(f"{tag}: velocity {e_v:.2e} rows {e_r:.2e} coords {e_c:.2e}")
        np.testing.assert_allclose(v, g["velocity_row"], rtol=1e-9, err_msg=tag)
        for k, key in enumerate(ROW_KEYS):
            np.testing.assert_allclose(res[k], g["profile_" + key], rtol=1e-8, atol=1e-8, err_msg=f"{tag} {key}")
        np.testing.assert_allclose(np.array(res[8]), g["profile_coords"], rtol=1e-10, atol=1e-10, err_msg=tag)
    (ra, _), (rb, _) = got[False], got[True]
    assert len(ra[0]) == len(rb[0]) and ra[6] == rb[6] and ra[7] == rb[7]


def default_cases():
    """The W = 8 cases that share the default robot, dd and dt: one batch."""
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, DEFAULT_DD
    out = []
    for name in NAMES:
        g = eu.load(name)
        if (len(g["waypoints"]) == 8 and cons_of(g) == [float(v) for v in DEFAULT_CONSTRAINTS] and float(g["profile_dt"]) == 0.01
                and float(g["profile_dd"]) == DEFAULT_DD):
            out.append((name, g))
    return out


def snapshot(res, out, b):
    """Everything the chain decided and computed for route b, as host arrays."""
    N = int(res["meta"][b, 3])
    rows, nmap, amap = eu.unpack(out, b)
    return {"flags": int(res["flags"][b]), "N": N, "velocity": res["velocity"][b, :N].cpu().numpy(),
            "node_sample": res["node_sample"][b].tolist(), "action_sample": res["action_sample"][b].tolist(),
            "rows": rows, "nodes_map": nmap, "actions_map": amap}


def assert_same(a, b, what, n_actions):
    assert a["flags"] == b["flags"] and a["N"] == b["N"], what
    assert a["node_sample"] == b["node_sample"], what
    # (a shorter list is padded with +inf in a batch: its padding never fires)
    assert a["action_sample"][:n_actions] == b["action_sample"][:n_actions], what
    assert all(k == eu.INT_MAX for k in a["action_sample"][n_actions:] + b["action_sample"][n_actions:]), what
    assert a["nodes_map"] == b["nodes_map"] and a["actions_map"] == b["actions_map"], what
    assert np.array_equal(a["velocity"], b["velocity"]), what
    assert a["rows"].shape == b["rows"].shape and np.array_equal(a["rows"], b["rows"]), what


@pytest.fixture(scope="module")
def alone(torch_mod, gens):
    """Every default case through the chain as a batch of one, computed once per type."""
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = {}
            for name, g in default_cases():
                res, out = eu.run_chain(torch_mod, gens[dtype], [eu.route_of(g)], list(DEFAULT_CONSTRAINTS))
                cache[dtype][name] = snapshot(res, out, 0)
        return cache[dtype]
    return get


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_together_equals_alone(torch_mod, gens, alone, dtype):
    """All default-robot W = 8 cases as ONE batch (their action-point lists padded to the longest with +inf), and again in
    reversed order: every route's rows, counts, maps, samples and velocities are bit-identical to its single-route call —
    the event lists of a batch share a kernel's LDS staging, and here differing lists at the edges sit side by side."""
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    cases = default_cases()
    assert len(cases) >= 24 and len({len(eu.action_points(eu.route_of(g))) for _, g in cases}) >= 4
    single = alone(dtype)
    for order in (cases, cases[::-1]):
        res, out = eu.run_chain(torch_mod, gens[dtype], [eu.route_of(g) for _, g in order], list(DEFAULT_CONSTRAINTS))
        for b, (name, g) in enumerate(order):
            assert_same(snapshot(res, out, b), single[name], (name, dtype, b), len(eu.action_points(eu.route_of(g))))
    print(f"EVENTS together/{dtype}: {len(cases)} routes bit-identical to their single-route calls, both orders")


def test_turn_at_node_0_is_flagged_and_its_neighbours_are_untouched(torch_mod, gens, alone):
    """include/vap.h: a turn at node 0 (IndexError in the reference, MPG:440) is VAP_FLAG_BAD_ROUTE — the flag, and the
    routes beside it in the batch bit-identical to their single-route calls."""
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    single = alone("f64")
    names = ["ap_same_t", "turn_wait_rev", "ap_on_node3_limits"]
    routes = [eu.route_of(eu.load(n)) for n in names]
    bad = dict(routes[1])
    bad["node_turn"] = bad["node_turn"].copy()
    bad["node_turn"][0] = 30.0
    res, out = eu.run_chain(torch_mod, gens["f64"], [routes[0], bad, routes[2]], list(DEFAULT_CONSTRAINTS))
    fl = res["flags"].tolist()
    assert fl[1] & _lib.FLAG_BAD_ROUTE and fl[0] == 0 and fl[2] == 0
    for b in (0, 2):
        assert_same(snapshot(res, out, b), single[names[b]], names[b], len(eu.action_points(routes[b])))
