"""Helpers of the event tests: the fixtures of tests/golden/events/ (routes of the real reference whose events sit where
the reference decides, oracle/gen_golden.py --events), the reference's distance-grid walk restated over a stored
parameter row, and the batched chain profile_routes -> apply_node_limits -> time_profile -> insert_waits."""
import glob
import os

import numpy as np

import golden_util as gu

EVENTS = os.path.join(gu.GOLDEN, "events")
INT_MAX = 0x7fffffff
AP_FIELDS = ("stop", "wait_time", "max_velocity", "max_acceleration")


def names():
    """The parametrisation of every event test: the directory listing."""
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(EVENTS, "*.npz")))


def load(name):
    z = np.load(os.path.join(EVENTS, name + ".npz"))
    return gu.Fixture((k, z[k]) for k in z.files)


def route_of(g):
    """The route of a fixture as the dict of arrays `run_chain` takes (action points in the fixture's order)."""
    return {k: g[k] for k in g.files if k.startswith(("node_", "ap_")) or k == "waypoints"}


def action_points(route):
    """A route's action points as the list of dicts the batched calls take, every field, in the order given."""
    if "ap_t" not in route or not len(route["ap_t"]):
        return []
    return [{"t": float(route["ap_t"][i]), "stop": bool(route["ap_stop"][i]), "wait_time": float(route["ap_wait_time"][i]),
             "max_velocity": float(route["ap_max_velocity"][i]), "max_acceleration": float(route["ap_max_acceleration"][i])}
            for i in range(len(route["ap_t"]))]


def walk_events(t_row, ap_t, W):
    """MPG:112-165 over the parameters of the distance grid (t_row: every sample, the appended end sample last): the
    sample at which each node and each action point takes effect, INT_MAX where the reference never reaches it.
      node:         (prev_t % 1) > (t % 1) and t < distance_to_time(total)          MPG:124
      action point: the pending one only, prev_t < ap.t and t >= ap.t              MPG:142-146, 163"""
    end = float(t_row[-1])
    node_sample = [0] + [INT_MAX] * (W - 1)
    action_sample = [INT_MAX] * len(ap_t)
    prev_t, node, act = 0.0, 0, 0
    for i, t in enumerate(t_row[:-1]):
        t = float(t)
        if (prev_t % 1) > (t % 1) and t < end:
            node += 1
            node_sample[node] = i
        if act < len(ap_t) and prev_t < ap_t[act] and t >= ap_t[act]:
            action_sample[act] = i
            act += 1
        prev_t = t
    return node_sample, action_sample


def run_chain(torch, gen, routes, cons, dt=0.01, dd=0.005, capacity=16384, capacity_rows=4096):
    """profile_routes -> apply_node_limits -> time_profile(node_reverse) -> insert_waits(node_turn, waits, action points)
    on a batch of routes of one width, each a dict of arrays; the action-point lists go in as they are (the host pads the
    shorter ones with +inf).  Returns (res, out): what apply_node_limits and insert_waits returned."""
    st = lambda key: np.stack([np.asarray(r[key]) for r in routes])
    wp = torch.tensor(st("waypoints"), dtype=gen.tdtype, device=gen.device)
    lists = [action_points(r) for r in routes]
    aps = lists if any(lists) else None
    res = gen.profile_routes(wp, node_reverse=st("node_is_reverse_node"), node_turn=st("node_turn"),
                             node_tangent=st("node_tangent"), node_magnitudes=st("node_magnitudes"),
                             constraints=cons, dd=dd, capacity=capacity)
    gen.apply_node_limits(res, cons, node_max_velocity=st("node_max_velocity"), node_stop=st("node_stop"),
                          node_max_acceleration=st("node_max_acceleration"), action_points=aps)
    tp = gen.time_profile(res, cons, dt=dt, capacity_rows=capacity_rows, node_reverse=st("node_is_reverse_node"))
    out = gen.insert_waits(res, tp, node_wait_time=st("node_wait_time"), action_points=aps, dt=dt,
                           node_turn=st("node_turn"), node_reverse=st("node_is_reverse_node"), constraints=cons)
    torch.cuda.synchronize()
    return res, out


def unpack(out, b):
    """(rows, nodes_map, actions_map) of route b of what insert_waits returned."""
    T, nn, na = (int(v) for v in out["counts"][b])
    return (out["rows"][b, :T].cpu().numpy(), [int(v) for v in out["nodes_map"][b, :nn]],
            [int(v) for v in out["actions_map"][b, :na]])


def full_profile(torch, gen, route, cons, copies=2, dt=0.01, dd=0.005):
    """The whole generate_motion_profile tuple of a route given as a dict of arrays, `copies` times in a batch."""
    res, out = run_chain(torch, gen, [route] * copies, cons, dt=dt, dd=dd)
    assert not res["flags"].any().item()
    assert torch.equal(out["rows"][0, :int(out["counts"][0, 0])], out["rows"][copies - 1, :int(out["counts"][copies - 1, 0])])
    return unpack(out, 0)
