"""The robots, start / end speeds, shapes and paths under which every velocity kernel is held to the sequential sweep
and the sweep to the oracle: shared by test_velocity_robots_cpu.py (which proves ON THE ORACLE ALONE that the cases
reach the clauses of the recurrence they are here for) and test_gpu_velocity_robots.py (which runs the kernels on the
same inputs).  Plain NumPy and the oracle; nothing here touches a device.

Why these cases: every test that forces a velocity kernel elsewhere runs DEFAULT with start_vel = end_vel = 0.01 on
synth.make_waypoints rows, on which no sample ever reaches max_vel.  A kernel that folds a constant of DEFAULT into a
coefficient, seeds the forward sweep with something other than start_u, mishandles a start speed the backward sweep
lowers, clamps an end speed the reference keeps, or fills a ragged row's tail with the wrong end_u passes all of them."""
import functools

import numpy as np

import path_families as pf
from vexautonomousplanner_amd.synth import make_waypoints

# ---- robots: (max_vel, max_acc, max_dec, friction_coef, max_jerk, track_width) -----------------------------------------
ROBOTS = {
    "DEFAULT": (4.0, 8.0, 8.0, 0.8, 16.0, 12.5 / 12),
    "CRAWL": (1.0, 8.0, 8.0, 0.8, 16.0, 12.5 / 12),           # max_vel binds: the plateau clause
    "SLOW_NARROW": (1.5, 3.0, 3.0, 0.8, 16.0, 0.6),
    "FAST_WIDE": (7.5, 15.0, 15.0, 0.8, 16.0, 1.9),
    "ACC_GT_DEC": (4.0, 12.0, 6.0, 0.8, 16.0, 12.5 / 12),     # the velocity pass decelerates with max_acc (quirk Q9)
    "ACC_LT_DEC": (4.0, 6.0, 12.0, 0.8, 16.0, 12.5 / 12),
}
OTHER_ROBOTS = [r for r in ROBOTS if r != "DEFAULT"]
# friction_coef, max_jerk and max_dec never enter the velocity rows (velocity_consts sets cc[2] = max_acc, Q9; the other
# two are dormant in the reference): index in the constraints tuple -> the value it is changed to
IGNORED_CONSTANTS = {"max_dec": (2, 3.25), "friction_coef": (3, 0.35), "max_jerk": (4, 5.0)}

# ---- (start_vel, end_vel) -----------------------------------------------------------------------------------------------
END_SPEEDS = [
    (0.01, 0.01),    # the default
    (1.2, 0.7),      # both bind at the ends
    (2.0, 0.3),      # start above max_vel for CRAWL and SLOW_NARROW, above the backward envelope on curved paths
    (0.3, 2.0),      # end above max_vel for CRAWL and SLOW_NARROW: the reference keeps it
    (0.0, 0.0),      # bit-identity tests only: a zero velocity has no relative error
]
ORACLE_END_SPEEDS = END_SPEEDS[:4]

# ---- shapes (B, W, S): the smallest at which each kernel still takes all of its code paths ---------------------------------
# Lane-per-path kernels.  A tile holds kTileRecords / P = 1024 / P samples (vap_velocity_lanes.hip:42, :60): 64, 32 or 16.
# A pipeline step is straight-lined only when its load, put and flush tiles are all interior, which needs it >= 2,
# it + 1 < NT and, forward, a first tile before and a last one after (vap_velocity_lanes.hip:357-359): S = 449 = 7 * 64 + 1
# gives NT = 8 / 15 / 29 with forward steps 3..5 and backward steps 4..6 interior at P = 16 (more at P = 32 and 64), and
# is no multiple of any tile.  A group that is
# not full has no interior tile (nmin = -1, vap_velocity_lanes.hip:415): B = 70 = 4 * 16 + 6 = 2 * 32 + 6 = 64 + 6 has
# full groups AND a partial last group for every P.  (130, 5, 65): two tiles plus one sample at P = 16, nine groups;
# (4, 4, 2) and (3, 4, 3): rows of only the start and end sample, and of one interior sample.
LANES_SHAPES = [(70, 5, 449), (130, 5, 65), (4, 4, 2), (3, 4, 3)]
# One ragged case on the reference's own grid: every path has its own n_samples, the slots past it hold end_u inside the
# kernel and zeros in the rows.
RAGGED = dict(B=21, W=8, dd=0.005, capacity=2048)
# Register-resident relaxation (launch_velocity_relax, vap_velocity_relax.hip:1363-1380): S <= 256 takes L = 4 (the
# lanes shapes above), 256 < S <= 1024 one wavefront per path with L = 16 in fp64 (257), S <= 4096 L = 8 x 512 threads
# (1025; fp32: L = 16), above that L = 20 (fp32: L = 40) — 4097, the shape this file adds to the issue's two.
RELAX_SHAPES = [(5, 5, 257), (3, 8, 1025), (2, 8, 4097)]
# Long rows: just past velocity_relax_max_samples (vap_velocity_relax.hip:1294: 512 * 20 = 10240 samples for the fp64
# recurrence, 512 * 40 = 20480 for fp32) with a ragged last super-chunk.  Super-chunks are 64 * 16 = 1024 samples (fp64)
# and 64 * 40 = 2560 (fp32) in the look-back kernel (launch_velocity_chase, :1566-1570) and, for so few blocks, in
# relax_rounds too (launch_velocity_long, :1461-1474): 10305 = 10 * 1024 + 65, 20545 = 8 * 2560 + 65.
LONG_SHAPES = {"f32": (2, 13, 10305), "f64": (2, 13, 10305), "f32r32": (2, 13, 20545)}
# relax_wave walks a row in windows of 64 * 40 = 2560 samples (launch_velocity_windows, vap_velocity_relax.hip:1588):
# 2561 is two windows, the second of one sample.  fp32 recurrence only (vap_api.hip:128).
WAVE_SHAPE = (5, 8, 2561)
# AUTO takes the lanes kernel from kLanesMinPaths = 2048 paths on (vap_api.hip:62, :94).
AUTO_SHAPE = (2048, 4, 129)

PATH_SETS = ("walk", "straight", "manhattan")    # make_waypoints rows; the plateau at max_vel; v[0] lowered
LONG_PATH_SETS = ("walk", "straight")

# Seeds.  Every batch is drawn with SEED; path b of a batch is replaced by path b of the same batch drawn with another
# seed where it did not qualify as well conditioned (test_velocity_robots_cpu.test_oracle_bound_paths_are_well_conditioned:
# on such a path a discrete decision of the reference — a zero heading difference, a table index — flips when a waypoint
# moves by one ulp, and no bound against the oracle means anything there).  Taking path b from batch position b keeps the
# variant that cycles with the path index (the direction of a straight path).  (path set, B, W) -> {path: seed}
SEED = 7
RESEEDED = {
    ("manhattan", 70, 5): {4: 8, 6: 8, 13: 8, 16: 8, 19: 8, 21: 8, 29: 8, 30: 8, 43: 8, 48: 8, 52: 8, 57: 8, 59: 8},
    ("manhattan", 130, 5): {6: 8, 21: 8, 29: 8, 52: 8, 57: 8, 72: 8, 81: 9, 92: 8, 94: 8, 114: 8, 116: 8, 117: 8, 119: 8,
                            124: 8, 129: 8},
    ("walk", 3, 4): {0: 9},
    ("straight", 3, 4): {2: 8},
    ("manhattan", 5, 5): {4: 8},
    # (of the 2048 paths of the AUTO batch only every 97th is compared with the oracle)
    ("walk", 2048, 4): {0: 9, 194: 8, 291: 8, 776: 9, 1455: 9, 1649: 8, 1843: 9, 2037: 9},
}


def _draw(kind, B, W, seed):
    if kind == "walk":
        return pf.f32(make_waypoints(B, W, seed))
    return pf.make(kind, B, W, seed)


@functools.lru_cache(maxsize=None)
def _paths(kind, B, W):
    wp = _draw(kind, B, W, SEED)
    for seed in sorted(set(RESEEDED.get((kind, B, W), {}).values())):
        other = _draw(kind, B, W, seed)
        for b, s in RESEEDED[(kind, B, W)].items():
            if s == seed:
                wp[b] = other[b]
    wp.setflags(write=False)
    return wp


def paths(kind, B, W):
    """(B, W, 2) fp64 waypoints, fp32-representable: what an fp32 caller and an fp64 caller hand over alike."""
    return _paths(kind, B, W).copy()


@functools.lru_cache(maxsize=None)
def oracle_rows(kind, B, W, S, robot, sv, ev):
    """The oracle's five rows (and total_length) on the fixed-S grid; computed once, shared, never modified."""
    from oracle import oracle
    r = oracle.profile_batch(paths(kind, B, W), S, ROBOTS[robot], start_vel=sv, end_vel=ev, n_threads=8)
    for v in r.values():
        v.setflags(write=False)
    return r


def oracle_velocity(wp, S, cons, sv, ev):
    from oracle import oracle
    return oracle.profile_batch(wp, S, cons, start_vel=sv, end_vel=ev, n_threads=8, want=("velocity",))["velocity"]


def anchor_cases():
    """(kind, B, W, S) of every fixed-grid batch the anchor compares with the oracle."""
    return [(kind, B, W, S) for (B, W, S) in LANES_SHAPES + RELAX_SHAPES for kind in PATH_SETS]


AUTO_KIND, AUTO_ROBOT, AUTO_ENDS = "walk", "CRAWL", (2.0, 0.3)
AUTO_ORACLE_PATHS = np.arange(0, AUTO_SHAPE[0], 97)       # the paths of the AUTO batch that are compared with the oracle


def conditioning(wp, S, cons, sv, ev, ulp="f64"):
    """Per path: the largest relative change of the oracle's fp64 velocity row when every waypoint coordinate moves by
    one ulp (`ulp`: of fp64 or of fp32), four seeded sign patterns — the measure
    test_gpu_geometry.reference_curvature_noise takes for curvature."""
    ref = oracle_velocity(wp, S, cons, sv, ev)
    out = np.zeros(len(wp))
    for t in range(4):
        sign = np.random.default_rng(t).choice([-1.0, 1.0], wp.shape)
        if ulp == "f32":
            moved = np.nextafter(wp.astype(np.float32), (sign * np.inf).astype(np.float32)).astype(np.float64)
        else:
            moved = np.nextafter(wp, sign * np.inf)
        v = oracle_velocity(moved, S, cons, sv, ev)
        out = np.maximum(out, np.max(np.abs(v - ref) / np.abs(ref), axis=1))
    return out


def worst_conditioning(wp, S, ulp="f64", robots=None, ends=None):
    """conditioning() of every path, the worst over the robots and the start / end speeds the oracle is compared under."""
    out = np.zeros(len(wp))
    for robot in ROBOTS if robots is None else robots:
        for sv, ev in ORACLE_END_SPEEDS if ends is None else ends:
            out = np.maximum(out, conditioning(wp, S, ROBOTS[robot], sv, ev, ulp))
    return out


