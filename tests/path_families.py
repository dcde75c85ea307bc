"""Structured path families for the parity tests (test infrastructure only: nothing in the product package or
bench.py imports this module).

`synth.make_waypoints` draws smooth random walks; the shapes here are the ones such walks never produce and on which
the kernels' special paths run: exact zeros (straight and axis-aligned runs), cusps (a path that turns back on
itself), arc-length tables with intervals orders of magnitude apart, coordinates far from or very close to the
origin, closed loops across the +-pi cut, and a sharp turn at every node.

`make(family, batch, W, seed)` returns (batch, W, 2) fp64 waypoints that are fp32-representable (rounded once
through fp32, like every other test input) and never have two adjacent waypoints equal.  The parameters of a family
are drawn per path; those that select a discrete variant (the direction of a straight path, the cusp factor, the
offset of a scaled path) cycle with the path index so that every batch of a few paths holds every variant."""
import numpy as np

from vexautonomousplanner_amd.synth import make_waypoints

FAMILIES = ("straight", "manhattan", "uneven", "reversal", "scale", "loops", "west", "zigzag")

STRAIGHT_KINDS = ("east", "north", "west", "south", "random")     # path b of a batch has kind b % 5
_AXIS = {"east": (1.0, 0.0), "north": (0.0, 1.0), "west": (-1.0, 0.0), "south": (0.0, -1.0)}
REVERSAL_FACTORS = (1.0, 0.5, 2.0)                                # path b has factor b % 3 (1: node i+1 = node i-1)
SCALE_OFFSETS = (0.0, 100.0, -1000.0)                             # path b has offset b % 3


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def table_aligned_nodes(W, per_node=1000):
    """Interior nodes whose parameter is an entry of the reference's property table (np.linspace(0, W-1, W*per_node)):
    only there does a cusp's zero first derivative land IN the table."""
    n = W * per_node
    return [i for i in range(1, W - 1) if (i * (n - 1)) % (W - 1) == 0]


def straight_kind(b):
    return STRAIGHT_KINDS[b % len(STRAIGHT_KINDS)]


def reversal_plan(b, W, rng):
    """(cusp node, factor) of path b, or None for W = 2.  Factor-1 members take a table-aligned node where W has one."""
    if W < 3:
        return None
    factor = REVERSAL_FACTORS[b % len(REVERSAL_FACTORS)]
    nodes = table_aligned_nodes(W) if factor == 1.0 else []
    nodes = nodes or list(range(1, W - 1))
    return int(nodes[int(rng.integers(len(nodes)))]), factor


def _one(family, b, W, rng):
    if family == "straight":
        kind = straight_kind(b)
        if kind == "random":
            a = rng.uniform(0.0, 2.0 * np.pi)
            s = np.concatenate([[0.0], np.cumsum(rng.uniform(0.3, 1.0, W - 1))])
            return np.outer(s, [np.cos(a), np.sin(a)]) + rng.uniform(-5.0, 5.0, 2)
        # dyadic steps and offsets: every coordinate and every difference is exact in fp32, the zero component too
        steps = np.round(rng.uniform(0.3, 1.0, W - 1) * 64.0) / 64.0
        s = np.concatenate([[0.0], np.cumsum(steps)])
        off = np.round(rng.uniform(-5.0, 5.0, 2) * 64.0) / 64.0
        return np.outer(s, _AXIS[kind]) + off
    if family == "manhattan":
        d = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=np.float64)
        k = int(rng.integers(0, 4))
        steps = []
        for _ in range(W - 1):
            k = (k + int(rng.choice([-1, 0, 1]))) % 4
            steps.append(d[k] * float(rng.choice([0.5, 1.0, 1.5])))
        return np.concatenate([[[0.0, 0.0]], np.cumsum(steps, axis=0)])
    if family == "uneven":
        wp = make_waypoints(1, W, int(rng.integers(1 << 30)))[0].astype(np.float64)
        st = np.diff(wp, axis=0) * 10.0 ** rng.uniform(-2.0, 1.0, (W - 1, 1))
        return np.concatenate([wp[:1], wp[:1] + np.cumsum(st, axis=0)])
    if family == "reversal":
        wp = make_waypoints(1, W, int(rng.integers(1 << 30)))[0].astype(np.float64)
        plan = reversal_plan(b, W, rng)
        if plan is not None:
            i, factor = plan
            wp[i + 1:] += (wp[i] - (wp[i] - wp[i - 1]) * factor) - wp[i + 1]
            wp = f32(wp)
            if factor == 1.0:
                wp[i + 1] = wp[i - 1]        # the exact cusp: the two unit chords at node i cancel bit for bit
        return wp
    if family == "scale":
        wp = make_waypoints(1, W, int(rng.integers(1 << 30)))[0].astype(np.float64)
        return wp * 10.0 ** rng.uniform(-1.0, 2.0) + SCALE_OFFSETS[b % len(SCALE_OFFSETS)]
    if family == "loops":
        th = np.cumsum(float(rng.choice([-1.0, 1.0])) * rng.uniform(0.3, 1.2, W))
        return np.stack([np.cos(th), np.sin(th)], axis=1) * rng.uniform(0.3, 2.0)
    if family == "west":
        return np.stack([-np.cumsum(rng.uniform(0.3, 1.0, W)), rng.normal(0.0, 0.05, W)], axis=1)
    if family == "zigzag":
        i = np.arange(W, dtype=np.float64)
        return np.stack([0.4 * i, 0.8 * (np.arange(W) % 2)], axis=1) + rng.uniform(-5.0, 5.0, 2)
    raise ValueError(f"unknown family {family!r}")


def _rng(family, W, seed, b):
    return np.random.default_rng([FAMILIES.index(family), int(W), int(seed), int(b)])


def make(family, batch, W, seed):
    """(batch, W, 2) fp64 waypoints of one family, fp32-representable, no two adjacent waypoints equal."""
    out = np.empty((batch, W, 2), dtype=np.float64)
    for b in range(batch):
        rng = _rng(family, W, seed, b)
        for _ in range(100):
            wp = f32(_one(family, b, W, rng))
            if np.all(np.any(np.diff(wp, axis=0) != 0.0, axis=1)):
                break
        else:
            raise RuntimeError(f"{family}: no path without adjacent duplicates")
        out[b] = wp
    return out


def reversal_cusps(batch, W, seed):
    """[(cusp node, factor) or None] of the members of make("reversal", batch, W, seed), in order."""
    return [reversal_plan(b, W, _cusp_rng(W, seed, b)) for b in range(batch)]


def _cusp_rng(W, seed, b):
    rng = _rng("reversal", W, seed, b)
    rng.integers(1 << 30)            # the draw of the base path's seed comes first
    return rng


def mixed(batch, W, seed, families=FAMILIES):
    """A batch whose consecutive paths come from different families (path b from families[b % len])."""
    per = {f: make(f, (batch + len(families) - 1) // len(families), W, seed) for f in families}
    return np.stack([per[families[b % len(families)]][b // len(families)] for b in range(batch)])


def manhattan_turns(wp):
    """(wp, turns): the angle in degrees (+90 counter-clockwise, -90 clockwise, 0 straight on) by which a Manhattan path
    turns at each interior node — what a user enters as the node's `turn` to rotate on the spot there."""
    wp = np.asarray(wp, dtype=np.float64)
    u, v = wp[1:-1] - wp[:-2], wp[2:] - wp[1:-1]
    turns = np.zeros(len(wp))
    turns[1:-1] = 90.0 * np.sign(u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0])
    return wp, turns
