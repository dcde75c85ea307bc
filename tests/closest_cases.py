"""The cases of the wide closest-point tests: inputs only (seeded waypoints, node attributes, query recipes), shared by
test_closest_cpu.py, which runs the references of closest_ref.py on the oracle's segments, and test_gpu_closest_wide.py,
which runs them on the device-fitted rows of the drop-in route.  Seeds are chosen so that the reference alone meets the
tie-share cap and the lane-trip counts (test_closest_cpu.py asserts both)."""
import numpy as np

import closest_ref as cr

WIDE_PATHS = 3
WIDE_QUERIES = dict(n_box=10, n_on=10, n_end=2)          # 24 per path
PLAIN_CASES = {"w64": (64, 6400), "w65": (65, 6500), "w129": (129, 12901), "w342": (342, 34200), "w343": (343, 34300)}
ROUTE_TURN_DEGREES = 35.0
ROUTE_PATHS = 2
ROUTE_CASES = {"many129": (129, 12909), "many343": (343, 34309), "two343": (343, None)}
ROUTE_SPLINES = {"many129": (15, 15), "many343": (38, 39), "two343": (3, 3)}           # per route of the case
ROUTE_AT_NODE_MIN = {"many129": 4, "many343": 4, "two343": 1}     # split-node queries whose EXACT answer is the node itself
FAMILY_WIDTHS = (5, 13)
FAMILY_PATHS = 6
FAMILY_SEED = 77
FAMILY_QUERIES = dict(n_box=8, n_on=6, n_end=1)
BLOCK_SHAPE = (3, 8)                                       # B, W of the query-block cases
BLOCK_QUERIES = (1, 15, 16, 17, 33, 64)
BLOCK_SEED = 808


def plain_waypoints(name):
    from vexautonomousplanner_amd.synth import make_waypoints
    W, seed = PLAIN_CASES[name]
    return make_waypoints(WIDE_PATHS, W, seed).astype(np.float64)         # fp32 values: both generators see the same


def route_case(name):
    """(waypoints (B, W, 2), node_reverse (B, W) bool, node_turn (B, W) degrees) of a many-spline route case: a reverse
    node or a 35 degree turn node every ninth node, alternating, offset by the route's index; the last node stays plain."""
    from vexautonomousplanner_amd.synth import make_waypoints
    W, seed = ROUTE_CASES[name]
    if seed is None:
        import wide_ref
        rev, turn = wide_ref.geometry_route_nodes(W)
        return wide_ref.geometry_route_waypoints(W).astype(np.float64), rev, turn
    rev = np.zeros((ROUTE_PATHS, W), dtype=bool)
    turn = np.zeros((ROUTE_PATHS, W))
    for b in range(ROUTE_PATHS):
        for n, i in enumerate(range(9 - b, W - 1, 9)):
            if (n + b) % 2 == 0:
                rev[b, i] = True
            else:
                turn[b, i] = ROUTE_TURN_DEGREES
    return make_waypoints(ROUTE_PATHS, W, seed).astype(np.float64), rev, turn


def split_queries(path, splits, n=6):
    """Queries about split nodes (a split node belongs to the earlier spline): for up to n of them, spread over the
    route, the points on the path 5e-4 before and after the node's parameter (cr.KIND_ON), and a point 0.05 ft beyond the
    node along the earlier spline's end tangent, 0.01 ft to its left (cr.KIND_SPLIT; t0 is the node)."""
    if not splits:
        return np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(0)
    pick = [splits[int(round(k))] for k in np.linspace(0, len(splits) - 1, min(n, len(splits)))]
    q, kind, t0 = [], [], []
    for k in pick:
        for t in (k - 5e-4, k + 5e-4):
            q.append(path.point([t])[0]); kind.append(cr.KIND_ON); t0.append(t)
        p = path.point([float(k)])[0]
        d = path.point([float(k)], order=1)[0]
        u = d / np.hypot(d[0], d[1])
        q.append(p + 0.05 * u + 0.01 * np.array([-u[1], u[0]])); kind.append(cr.KIND_SPLIT); t0.append(float(k))
    return np.array(q), np.array(kind, dtype=np.int64), np.array(t0)


def route_queries(path, waypoints, rev, turn, seed):
    a = cr.make_queries(path, waypoints, seed, n_box=8, n_on=8, n_end=1)
    b = split_queries(path, cr.split_nodes(path.W, rev, turn))
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def family_waypoints(family, W):
    import path_families as pf
    return pf.make(family, FAMILY_PATHS, W, FAMILY_SEED)


def family_queries(family, W, b, path, waypoints):
    """The queries of member b of a family: the usual mix; for a reversal member with factor 1 the node its neighbour
    retraces (node i-1 = node i+1 exactly: the two parameters tie; t0 is the smaller); for an axis-aligned straight
    member points exactly on the line (cr.KIND_LINE) and 2 ft out on its extension beyond both ends (cr.KIND_EXTENSION)."""
    import path_families as pf
    retraced = ()
    if family == "reversal":
        plan = pf.reversal_cusps(FAMILY_PATHS, W, FAMILY_SEED)[b]
        if plan is not None and plan[1] == 1.0:
            retraced = (plan[0] - 1,)
    q, kind, t0 = cr.make_queries(path, waypoints, 1000 * W + b, retraced=retraced, **FAMILY_QUERIES)
    if family == "straight" and pf.straight_kind(b) != "random":
        wp = np.asarray(waypoints, dtype=np.float64)
        u = (wp[-1] - wp[0]) / np.hypot(*(wp[-1] - wp[0]))
        extra = [0.5 * (wp[0] + wp[1]), 0.5 * (wp[W // 2 - 1] + wp[W // 2]), 0.25 * wp[-2] + 0.75 * wp[-1],
                 wp[0] - 2.0 * u, wp[-1] + 2.0 * u]
        q = np.concatenate([q, extra])
        kind = np.concatenate([kind, [cr.KIND_LINE] * 3 + [cr.KIND_EXTENSION] * 2])
        t0 = np.concatenate([t0, [np.nan] * 3 + [0.0, W - 1.0]])
    return q, kind, t0


def block_queries(path, waypoints, Q, seed):
    n_end = 1 if Q >= 15 else 0
    n_on = Q // 3
    return cr.make_queries(path, waypoints, seed, n_box=Q - n_on - 2 * n_end, n_on=n_on, n_end=n_end)


# A path that comes back to one of its own nodes 64 nodes later: lane k of EXACT mode's node pass takes node k and node
# k + 64, so the two coincident nodes meet inside ONE lane's running best (every other exact tie of these cases is
# settled between lanes, by the wave argmin).  Any query answered at that point ties exactly; the smaller parameter wins.
REVISIT_W, REVISIT_NODE, REVISIT_SEED = 70, 2, 7000


def revisit_waypoints():
    from vexautonomousplanner_amd.synth import make_waypoints
    wp = make_waypoints(1, REVISIT_W, REVISIT_SEED)[0].astype(np.float64)
    a, b = REVISIT_NODE, REVISIT_NODE + 64
    wp[b:] += wp[a] - wp[b]
    wp = wp.astype(np.float32).astype(np.float64)
    wp[b] = wp[a]
    assert np.all(np.any(np.diff(wp, axis=0) != 0.0, axis=1))
    return wp[None]


def revisit_queries(path, waypoints):
    return cr.make_queries(path, waypoints, REVISIT_SEED, n_box=8, n_on=8, n_end=1, retraced=(REVISIT_NODE,))
