"""Batches with degenerate paths in them, for tests/test_bad_paths_cpu.py and tests/test_gpu_bad_paths.py.

A CLEAN batch comes from synth.make_waypoints; its DIRTY twin has the paths at chosen positions replaced by bad ones, each
planted into a copy of the good path it replaces.  The tests compare the paths that are good in both: a path's rows do not
depend on its place in the batch (what tests/test_gpu_sample_halves.py relies on), so they must not depend on who its
neighbours are either.

Kinds (`plant`):
  dup_mid / dup_first / dup_last   two equal neighbouring waypoints: a zero-length segment (middle, first, last)
  point                            every waypoint equal: a path of zero length
  nan / pinf / ninf                one coordinate NaN, +inf, -inf
  huge                             one coordinate 1e200 (fp64 input; the squared distance overflows while the coordinate is
                                   finite) — fp32 input cannot hold it and takes +inf instead
  tiny                             the whole path scaled by 1e-170: the squared distances underflow to 0 (fp32 input: the
                                   coordinates themselves do, and the path is a point at the origin)

Placements (`PLACEMENTS`): the smallest shapes at which a kernel shares a workgroup, a wave or a quad of lanes between
paths, with the bad paths where that sharing has an edge — see the table in DESIGN.md (section "Bad paths in a batch").
"""
import functools

import numpy as np

KINDS = ("dup_mid", "dup_first", "dup_last", "point", "nan", "pinf", "ninf", "huge", "tiny")
FLAG_ASSERTED = tuple(k for k in KINDS if k != "tiny")      # tiny: the flag is reported, either answer is defensible


def plant(path, kind, f32_input=False):
    """The bad path of `kind` made from the good (W, 2) fp64 path: a copy, the input unchanged."""
    p = np.array(path, dtype=np.float64, copy=True)
    W = p.shape[0]
    m = W // 2
    if kind == "dup_mid":
        p[m] = p[m - 1]
    elif kind == "dup_first":
        p[1] = p[0]
    elif kind == "dup_last":
        p[W - 1] = p[W - 2]
    elif kind == "point":
        p[:] = p[0]
    elif kind == "nan":
        p[m, 0] = np.nan
    elif kind == "pinf" or (kind == "huge" and f32_input):
        p[m, 1] = np.inf
    elif kind == "ninf":
        p[m, 0] = -np.inf
    elif kind == "huge":
        p[m, 1] = 1e200
    elif kind == "tiny":
        p *= 1e-170
        if f32_input:
            p = p.astype(np.float32).astype(np.float64)
    else:
        raise KeyError(kind)
    return p


# name: B, W, seed, grid ("S", samples) | ("dd", dd, capacity), the positions of the bad paths, the velocity kernel option
PLACEMENTS = {
    "solo":     dict(B=5, W=8, seed=71, grids=(("S", 1021),), bad=(0, 2, 4), kernel="auto"),
    "interior": dict(B=3, W=8, seed=72, grids=(("S", 3064),), bad=(1,), kernel="auto"),
    "ragged":   dict(B=5, W=8, seed=73, grids=(("dd", 0.0046, 3072),), bad=(1, 3), kernel="auto"),
    "lanes16":  dict(B=35, W=8, seed=74, grids=(("S", 300), ("S", 1021)), bad=(0, 5, 15, 16, 34), kernel="lanes16"),
    "lanes32":  dict(B=35, W=8, seed=74, grids=(("S", 300), ("S", 1021)), bad=(0, 31, 32, 34), kernel="lanes32"),
    "lanes64":  dict(B=70, W=8, seed=75, grids=(("S", 300), ("S", 1021)), bad=(0, 63, 64, 69), kernel="lanes64"),
    "many8":    dict(B=8195, W=8, seed=76, grids=(("S", 1024),), bad=(0, 1, 7, 8, 31, 32, 8193, 8194), kernel="auto"),
    "many64":   dict(B=32773, W=8, seed=77, grids=(("S", 64),), bad=(0, 63, 64, 32772), kernel="auto"),
    "wide":     dict(B=3, W=115, seed=78, grids=(("S", 2041),), bad=(1,), kernel="auto"),
    "routes":   dict(B=5, W=8, seed=79, grids=(("S", 1021),), bad=(1, 4), kernel="auto"),
}
SMALL = ("solo", "interior", "ragged", "lanes16", "lanes32", "lanes64", "wide", "routes")
# the routes placement: a reverse node and a turn node inside every route cut it into three splines
ROUTE_REVERSE_NODE, ROUTE_TURN_NODE, ROUTE_TURN_DEG = 2, 5, 90.0
# the time-domain variant: a full group of sixteen paths of the fused kernel plus a part-filled one
TIME19 = dict(B=19, W=8, seed=80, grids=(("S", 1021),), bad=(3, 15, 16, 18), kernel="auto")


def placement(name):
    return TIME19 if name == "time19" else PLACEMENTS[name]


@functools.lru_cache(maxsize=None)
def clean_batch(name):
    """(B, W, 2) fp64, every value an fp32 value (so fp32 and fp64 inputs are the same numbers).  Read-only."""
    from vexautonomousplanner_amd.synth import make_waypoints
    p = placement(name)
    wp = make_waypoints(p["B"], p["W"], p["seed"]).astype(np.float64)
    wp.setflags(write=False)
    return wp


def calls(name):
    """The dirty twins of a placement: [(label, {position: kind})].  Call r gives position i the kind KINDS[(r + i) % 9] —
    over the nine calls every position has carried every kind, and a call with several positions carries several kinds at
    once — and a tenth call has a single bad path of kind nan at the first position."""
    pos = placement(name)["bad"]
    out = []
    for r in range(len(KINDS)):
        out.append((f"rot{r}", {b: KINDS[(r + i) % len(KINDS)] for i, b in enumerate(pos)}))
    out.append(("one_nan", {pos[0]: "nan"}))
    return out


CALL_LABELS = tuple(f"rot{r}" for r in range(len(KINDS))) + ("one_nan",)


def dirty_batch(name, label, f32_input=False):
    """(waypoints (B, W, 2) fp64, {position: kind}) of one call."""
    plan = dict(calls(name))[label]
    wp = np.array(clean_batch(name), copy=True)
    for b, kind in plan.items():
        wp[b] = plant(wp[b], kind, f32_input)
    return wp, plan


def good_mask(name, plan):
    m = np.ones(placement(name)["B"], dtype=bool)
    m[list(plan)] = False
    return m


def t_max_of(wp):
    """parameters[-1] of every path of (B, W, 2) fp64 waypoints, as the fit forms it (QHS:719-736: sequential cumsum of the
    chord lengths, then cum * G / cum)."""
    G = wp.shape[1] - 1
    with np.errstate(all="ignore"):
        d = np.diff(wp, axis=1)
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        cum = np.cumsum(dist, axis=1)[:, -1]
        return np.where(cum == 0.0, float(G), cum * G / cum)
