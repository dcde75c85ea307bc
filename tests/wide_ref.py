"""What the wide-path tests (test_gpu_wide_routes.py) expect, from the oracle and from arithmetic alone.

Three kernels of the route pipeline change their code path, or their LDS budget, once a path is wide; the shapes on
either side of each switch, the bytes that decide it and the references of every case are defined here, imported by
the GPU file and pinned without a GPU by test_wide_routes_cpu.py — so no expectation of a GPU test comes from a kernel.
Every reference is computed once per process (functools.lru_cache) and handed out as it is: callers do not write to it.

It imports nothing from the library under test but the seeded waypoint generator.
"""
import functools

import numpy as np

from oracle import oracle
from vexautonomousplanner_amd.synth import make_waypoints

DEFAULT = (4.0, 8.0, 8.0, 0.8, 16.0, 12.5 / 12.0)
DT = 0.05                     # time step of the wide cases
DD = 0.05                     # their distance step: a 2048-waypoint path is ~1350 ft, 27 000 samples
NEVER = 0x7fffffff            # node_sample / action_sample of an event the reference never reaches

# ---- the three switches: bytes at their boundary shapes, as plain integers --------------------------------------------
# k_time_geometry stages 12 doubles per segment while they fit 40 KB:          96 (W - 1) <= 40960
GEOMETRY_LDS_LIMIT = 40 * 1024
GEOMETRY_BYTES = {427: 40896, 428: 40992}
# k_limit_fill keeps the merged event list (E = max(W - 2, 0) + M entries of two doubles and two ints) in LDS while
#                                                                               24 E + 16 <= 49152
EVENT_LDS_LIMIT = 48 * 1024
EVENT_BYTES = {2047: 49144, 2048: 49168}
# k_time_waits: 3 ints per possible event (2 W + M of them), the nodes_map row (W ints, padded to a pair) and two rows
# of W doubles in dynamic LDS, 44 W + 12 M + 16 bytes, beside one static word.  64 KB launches anywhere; above, the request
# has to be granted; nothing above a CDNA workgroup's 160 KB can run.
WAITS_DEFAULT_LDS = 64 * 1024
WAITS_STATIC_BYTES = 4
WAITS_BYTES = {(1488, 1): 65500, (1489, 1): 65544, (1500, 1): 66028, (2048, 1): 90140, (2048, 2): 90152, (428, 1): 18860,
               (6, 20000): 240280}
CDNA_MAX_LDS = 160 * 1024


def geometry_bytes(W):
    return 96 * (W - 1)


def event_count(W, M):
    return max(W - 2, 0) + M


def event_bytes(E):
    return 24 * E + 16


def waits_bytes(W, M):
    return 4 * (3 * (2 * W + M) + W + 2) + 16 * W + 8


# ---- waits ------------------------------------------------------------------------------------------------------------
# int(wait_time / dt) at the coarse step, as Python gives it (both quotients are exact); the entries at 0.05 s come from
# time_ref.WAIT_EDGE_STEPS.  test_wide_routes_cpu.py asserts every entry.
COARSE_DT = 0.25
COARSE_WAIT_STEPS = {0.5: 2, 0.75: 3}


def _plain_nodes(W, **over):
    n = dict(is_reverse=np.zeros(W), turn=np.zeros(W), stop=np.zeros(W), wait_time=np.zeros(W), max_velocity=np.zeros(W),
             max_acceleration=np.zeros(W), tangent=np.full((W, 2), np.nan), magnitudes=np.zeros((W, 2)))
    n.update(over)
    return n


def _actions(t, wait=None, mv=None, ma=None, stop=None):
    M = len(t)
    z = lambda a: np.zeros(M) if a is None else np.asarray(a, dtype=np.float64)
    return dict(t=np.asarray(t, dtype=np.float64), stop=z(stop), wait_time=z(wait), max_velocity=z(mv), max_acceleration=z(ma))


# ---- a. the geometry switch -------------------------------------------------------------------------------------------
GEOMETRY_WIDTHS = (427, 428)
GEOMETRY_PATHS = 3


@functools.lru_cache(maxsize=None)
def geometry_waypoints(W):
    return make_waypoints(GEOMETRY_PATHS, W, 4000 + W)         # fp32 values: both types and the oracle see the same


@functools.lru_cache(maxsize=None)
def geometry_refs(W):
    """generate_motion_profile(dt = 0.05, dd = 0.05) of the three plain paths: [(rows, nodes_map)]."""
    out = []
    for wp in geometry_waypoints(W).astype(np.float64):
        rows, nmap, _ = oracle.OraclePath(wp).generate_motion_profile(DEFAULT, dt=DT, dd=DD)
        out.append((rows, nmap))
    return out


GEOMETRY_ROUTES = 2
ROUTE_TURN_DEGREES = 35.0


def geometry_route_nodes(W):
    """One reverse node and one 35 degree turn node per route, at other places in the two routes."""
    rev = np.zeros((GEOMETRY_ROUTES, W), dtype=bool)
    turn = np.zeros((GEOMETRY_ROUTES, W))
    rev[0, W // 3], turn[0, (2 * W) // 3] = True, ROUTE_TURN_DEGREES
    rev[1, (3 * W) // 4], turn[1, W // 5] = True, ROUTE_TURN_DEGREES
    return rev, turn


@functools.lru_cache(maxsize=None)
def geometry_route_waypoints(W):
    return make_waypoints(GEOMETRY_ROUTES, W, 5000 + W)


@functools.lru_cache(maxsize=None)
def geometry_route_refs(W):
    """The two routes with their reverse and turn node: [(rows, nodes_map)] of generate_motion_profile."""
    rev, turn = geometry_route_nodes(W)
    out = []
    for b, wp in enumerate(geometry_route_waypoints(W).astype(np.float64)):
        op = oracle.OraclePath(wp, nodes=_plain_nodes(W, is_reverse=rev[b].astype(float), turn=turn[b]))
        rows, nmap, _ = op.generate_motion_profile(DEFAULT, dt=DT, dd=DD)
        out.append((rows, nmap))
    return out


# ---- b. the event-list switch -----------------------------------------------------------------------------------------
def limit_walk(t, W, max_vel, end_vel, node_mv, node_stop, ap_t, ap_mv, ap_stop):
    """The walk of forward_backward_pass over the samples' parameters `t` (MPG:100-176) as far as the initial velocities
    go: a node is passed where the parameter's fraction wraps, one action point is pending at a time and fires on the
    first sample whose parameter has reached it while the sample before had not.  Returns the `velocities` list, the
    sample of every node and of every action point (NEVER: not reached)."""
    M = len(ap_t)
    node_k = np.full(W, NEVER, dtype=np.int64)
    ap_k = np.full(M, NEVER, dtype=np.int64)
    node_k[0] = 0
    mv = node_mv[0] if node_mv[0] > 0 else max_vel
    out = []
    node, a, prev, t_end = 0, 0, 0.0, float(W - 1)
    for k, tk in enumerate(t[:-1]):
        out.append(mv)
        if (prev % 1) > (tk % 1) and tk < t_end:
            node += 1
            node_k[node] = k
            if node_stop[node]:
                out[-1] = 0.01
            mv = node_mv[node] if node_mv[node] > 0 else max_vel
        if a < M and prev < ap_t[a] and tk >= ap_t[a]:
            ap_k[a] = k
            mv = ap_mv[a] if ap_mv[a] > 0 else max_vel
            if ap_stop[a]:
                out[-1] = 0.01
            a += 1
        prev = tk
    out.append(end_vel)
    return np.array(out), node_k, ap_k


EVENT_PATHS = 2          # two paths per batch: the second one's list starts at E entries, not at 0
EVENT_CASES = {          # name: (W, M, dd)
    "w2048_m1": (2048, 1, DD),          # E = 2047: the last list that fits LDS
    "w2048_m2": (2048, 2, DD),          # E = 2048: the first one searched in global memory
    "w6_m2044": (6, 2044, 0.005),       # E = 2048 made of action points the reference skips
}


@functools.lru_cache(maxsize=None)
def event_case(name):
    """Inputs and reference of one case: a dict with waypoints (B, W, 2) fp32 values, node_max_velocity,
    node_max_acceleration, node_stop (B, W), action_points (per path: list of dicts), and per path the oracle's
    velocity row, the reference's initial velocities, node_sample, action_sample, and the counts the GPU test asserts
    before it asks the device: events reached that carry a limit, action points reached and skipped."""
    W, M, dd = EVENT_CASES[name]
    B = EVENT_PATHS
    rng = np.random.default_rng(20480 + W + M)
    wp = make_waypoints(B, W, 6000 + W)
    mv = np.where(rng.random((B, W)) < 0.3, rng.uniform(1.0, 3.5, (B, W)), 0.0)
    ma = np.where(rng.random((B, W)) < 0.3, rng.uniform(2.0, 12.0, (B, W)), 0.0)
    stop = rng.random((B, W)) < 0.05
    stop[:, 0] = stop[:, -1] = False
    aps = []
    for b in range(B):
        if M == 1:
            one = [dict(t=700.37 + 300 * b, max_velocity=2.25, max_acceleration=0.0, stop=False)]
        elif M == 2:
            one = [dict(t=512.61 + 100 * b, max_velocity=1.75, max_acceleration=0.0, stop=False),
                   dict(t=1530.23 + 100 * b, max_velocity=0.0, max_acceleration=5.5, stop=True)]
        else:
            ts = np.sort(rng.uniform(0.05, W - 1.05, size=M))
            one = [dict(t=float(t), max_velocity=float(rng.uniform(1.0, 3.0)) if rng.random() < 0.6 else 0.0,
                        max_acceleration=float(rng.uniform(2.0, 10.0)) if rng.random() < 0.5 else 0.0,
                        stop=bool(rng.random() < 0.2)) for t in ts]
        aps.append(one)
    case = dict(W=W, M=M, dd=dd, waypoints=wp, node_max_velocity=mv, node_max_acceleration=ma, node_stop=stop,
                action_points=aps, velocity=[], vcap=[], node_sample=[], action_sample=[], limited_events=[],
                actions_reached=[], actions_skipped=[])
    for b in range(B):
        at = np.array([a["t"] for a in aps[b]])
        amv = np.array([a["max_velocity"] for a in aps[b]])
        ama = np.array([a["max_acceleration"] for a in aps[b]])
        ast = np.array([float(a["stop"]) for a in aps[b]])
        op = oracle.OraclePath(wp[b].astype(np.float64),
                               nodes=_plain_nodes(W, stop=stop[b].astype(float), max_velocity=mv[b], max_acceleration=ma[b]),
                               actions=_actions(at, mv=amv, ma=ama, stop=ast))
        op.rebuild_tables()
        ref = op.forward_backward(DEFAULT, dd=dd)
        vcap, node_k, ap_k = limit_walk(ref["t"], W, DEFAULT[0], 0.01, mv[b], stop[b], at, amv, ast)
        reached_n = node_k[1:W - 1] != NEVER
        reached_a = ap_k != NEVER
        limited = int(((mv[b, 1:W - 1] > 0) | (ma[b, 1:W - 1] > 0) | stop[b, 1:W - 1])[reached_n].sum())
        limited += int(((amv > 0) | (ama > 0) | (ast > 0))[reached_a].sum())
        case["velocity"].append(ref["velocity"])
        case["vcap"].append(vcap)
        case["node_sample"].append(node_k)
        case["action_sample"].append(ap_k)
        case["limited_events"].append(limited)
        case["actions_reached"].append(int(reached_a.sum()))
        case["actions_skipped"].append(int((~reached_a).sum()))
    return case


# ---- c. the wait kernel's LDS -----------------------------------------------------------------------------------------
WAIT_CASES = {           # name: (W, turns (node: degrees), dt, seed)
    "w1488": (1488, {}, DT, 8488),            # 65 500 B: the last request below 64 KB
    "w1489": (1489, {}, DT, 8489),            # 65 544 B: the first one above
    "w2048": (2048, {}, DT, 9048),            # the widest plain path
    "route1500": (1500, {500: 90.0, 1000: -35.0}, DT, 8500),   # the widest route, two in-place turns
    "coarse428": (428, {}, COARSE_DT, 7418),  # several nodes passed in one time step (the seed: 12 such steps; of the seeds
                                              # 7400-7439 five give ten or more)
}
EDGE_WAITS = (0.35, 0.15)               # the entries of time_ref.WAIT_EDGE_STEPS at 0.05 s
COARSE_MULTI_NODE_STEPS_MIN = 10


@functools.lru_cache(maxsize=None)
def wait_case(name):
    """One route with waits on about a tenth of its nodes, one at node 0, and one action point: at 0.05 s its wait starts
    one kinematic row behind the wait of node `ap_node` (its parameter lies between those of the row at which the node
    is passed and the next one).  Returns a dict with the waypoints (W, 2) fp32 values, waits, turns (W,), the action
    point (t, wait), the oracle's rows / nodes_map / actions_map, the row count without waits (`bare_rows`), and for the
    route without waits `multi_node_steps`, the time steps that pass two or more nodes, and `nodes_recorded`, the length of
    its nodes_map.  (The reference appends to nodes_map at most once per time step, MPG:527-529, and every step appends a
    row: two nodes never share a row there — a step that passes two nodes records one of them or none, and the nodes
    behind it are taken for earlier ones.  That, not a shared row, is what a coarse step does to the maps.)"""
    W, turn_at, dt, seed = WAIT_CASES[name]
    rng = np.random.default_rng(seed)
    wp = make_waypoints(1, W, seed)[0]
    wp64 = wp.astype(np.float64)
    turns = np.zeros(W)
    for k, deg in turn_at.items():
        turns[k] = deg
    values = EDGE_WAITS if dt == DT else tuple(COARSE_WAIT_STEPS)
    waits = np.where(rng.random(W) < 0.1, rng.choice(values, size=W), 0.0)
    waits[turns != 0] = 0.0
    waits[-1] = 0.0
    waits[0] = values[0]
    ap_node = W // 4
    waits[ap_node] = values[1]
    waits[ap_node - 1] = waits[ap_node + 1] = 0.0
    bare = oracle.OraclePath(wp64, nodes=_plain_nodes(W, turn=turns))
    b_rows, b_nmap, _ = bare.generate_motion_profile(DEFAULT, dt=dt, dd=DD)
    bare.rebuild_tables()
    if dt == DT:
        r = int(b_nmap[ap_node])        # (in front of the first turn: the rows up to here are kinematic rows)
        assert 0 < r < len(b_rows) - 1
        t_r, t_next = bare.distance_to_time(b_rows[r - 1, 1]), bare.distance_to_time(b_rows[r, 1])
        assert ap_node < t_r < t_next < ap_node + 1, (t_r, t_next)
        ap = (0.5 * (t_r + t_next), values[0])
    else:
        ap = (W / 2 + 0.4, values[0])
    op = oracle.OraclePath(wp64, nodes=_plain_nodes(W, turn=turns, wait_time=waits), actions=_actions([ap[0]], wait=[ap[1]]))
    rows, nmap, amap = op.generate_motion_profile(DEFAULT, dt=dt, dd=DD)
    # steps of the bare route that pass two or more nodes: row i is integrated from the parameter of position i - 1
    t_rows = np.array([0.0] + [bare.distance_to_time(p) for p in b_rows[:-1, 1]])
    crossed = np.diff(np.floor(t_rows))
    return dict(multi_node_steps=int((crossed >= 2).sum()), nodes_recorded=len(b_nmap), W=W, dt=dt, waypoints=wp, waits=waits, turns=turns, ap=ap, ap_node=ap_node, rows=rows, nodes_map=nmap,
                actions_map=amap, bare_rows=len(b_rows))
