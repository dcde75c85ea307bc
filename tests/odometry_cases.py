"""The seeded inputs of the odometry-rollout tests, shared by test_odometry_cpu.py (which holds the reference alone to the cap
on excused rollouts) and test_gpu_odometry.py (which runs the kernel on the same inputs), and the comparison's rules.  Plain
NumPy: a case is a dict of rows, counts, follower (tracking_ref's dict), P and O (perturbation and odometry records), sensors
((n, 8) C-ABI rows or None), scene (range_cases' dict) and rule (odometry_ref.rule).

The gate is 6 in.  The start offsets are drawn with sigma 0.04 ft and the odometry errors are a few per cent, so the typical
|z - t_hat| is a few hundredths of a foot, and the seeded obstacles (radii 0.3 .. 1.2 ft, away from the walls) shorten a beam by
feet: a reading is far inside or far outside the gate.

The gain is 0.25.  An accepted reset moves the estimate by gain x (t_hat - z), and between two ray casts of the same wall that
difference carries the rounding of a range of up to 12 ft, a few 1e-15 ft, afresh at every reset.  The follower turns the
estimate's position into wheel commands within the row (k = 2 zeta sqrt(omega^2 + b v^2) is 3 to 10 here, and a record with
tau = 0 passes a command to the wheels unfiltered), and the executed rows' acceleration column is a difference quotient over
dt = 0.01 s: 100 x sqrt(2) x the noise of v.  With two sensors per coordinate that is about gain x 4e-15 x 2 x 10 x 140 =
gain x 1e-11 on that column at worst, against a tolerance whose floor is 1e-12: a gain of 0.8 leaves no room (the first choice
here, and 3 of about 150 000 acceleration values of the golden routes then missed their tolerance by at most a factor of two,
all other values passing), 0.25 does.  The hand-computed cases of test_odometry_cpu.py use a gain of 1."""
import functools
import math

import numpy as np

import golden_util as gu
import odometry_ref as orf
import range_cases as rc
import tracking_ref as tr

DT = 0.01
FLOOR, FACTOR, CAP = 1e-12, 8.0, 1e-9            # test_gpu_tracking.py's tolerance: max(FLOOR, FACTOR * D), capped
AMBIGUOUS = 1e-9
EXCLUDE_RAD = 3.0
MAX_EXCUSED = 0.02
GATE_IN, INCIDENCE_DEG, GAIN = 6.0, 60.0, 0.25
GOLDEN = ("plain_w5_s0", "plain_w8_s0", "feat_turn")
LAYOUTS = ((1, 1), (3, 5), (16, 17), (64, 5), (256, 3), (300, 2))
TILE_ROWS = (63, 64, 65, 129)


def rule(gate_in, max_incidence_deg, gain, every):
    """odometry_ref.rule from inches and degrees, converted as odometry.ResetRule converts them."""
    r = orf.rule(gate_in / 12.0, min(1.0, max(0.0, math.cos(math.radians(max_incidence_deg)))), gain, every)
    r.update(gate_in=gate_in, max_incidence_deg=max_incidence_deg)
    return r


def perturbations(rng, B, K, pos=0.04, heading=0.03, gain=0.02, track=0.03, tau=0.05):
    z = rng.standard_normal((B, K, 6))
    p = np.zeros((B, K, 8))
    p[..., 0:2] = z[..., 0:2] * pos
    p[..., 2] = z[..., 2] * heading
    p[..., 3:5] = np.maximum(1.0 + z[..., 3:5] * gain, 0.5)
    p[..., 5] = np.maximum(1.0 + z[..., 5] * track, 0.5)
    p[..., 6] = tau
    p[:, 0] = tr.NOMINAL
    return p


def records(rng, B, K, enc=0.02, hscale=0.01, drift=0.01, rscale=0.005, rbias=0.02):
    z = rng.standard_normal((B, K, 6))
    o = np.zeros((B, K, 8))
    o[..., 0:2] = np.maximum(1.0 + z[..., 0:2] * enc, 0.5)
    o[..., 2] = np.maximum(1.0 + z[..., 2] * hscale, 0.5)
    o[..., 3] = z[..., 3] * drift
    o[..., 4] = np.maximum(1.0 + z[..., 4] * rscale, 0.5)
    o[..., 5] = z[..., 5] * rbias
    o[:, 0] = orf.IDEAL
    return o


def synth_rows(rng, B, cap):
    """Consistent rows of smooth random drives that stay on the field: v(t), omega(t) are sums of a few sines, integrated by
    the exact arc from a start within 1.5 ft of the centre (at most 2 s at 1.6 ft/s)."""
    rows = np.zeros((B, cap, 8))
    t = np.arange(cap) * DT
    for b in range(B):
        v = 1.0 + sum(rng.uniform(0, 0.2) * np.sin(rng.uniform(0.5, 4) * t + rng.uniform(0, 6)) for _ in range(3))
        w = sum(rng.uniform(0, 0.8) * np.sin(rng.uniform(0.5, 5) * t + rng.uniform(0, 6)) for _ in range(3))
        x, y, phi = rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-np.pi, np.pi)
        s = 0.0
        for r in range(cap):
            rows[b, r] = [t[r], s, v[r], 0.0, -tr.wrap(phi), -w[r], x, y]
            u = w[r] * DT / 2
            d = v[r] * DT * float(tr.sinc(u))
            x, y, phi, s = x + d * np.cos(phi + u), y + d * np.sin(phi + u), phi + w[r] * DT, s + abs(d)
        rows[b, 1:, 3] = np.diff(rows[b, :, 2]) / DT
    return rows


def seeded_scene(seed=5):
    """Walls + 8 polygons + 4 circles (range_cases.random_scene)."""
    return rc.random_scene(np.random.default_rng(seed))


def packed(scene):
    return None if scene is None else orf.PackedScene(scene["field"], scene["polygons"], scene["circles"])


def golden_rows_centred(name):
    """A golden route's own time-domain rows, moved so that its bounding box is centred on the field."""
    r = tr.golden_rows(gu.load(name)).copy()
    for c in (6, 7):
        r[:, c] -= (r[:, c].min() + r[:, c].max()) / 2
    return r


@functools.lru_cache(maxsize=None)
def golden_case(every):
    routes = [golden_rows_centred(n) for n in GOLDEN for _ in range(2)]
    cap = max(len(r) for r in routes)
    rows = np.zeros((len(routes), cap, 8))
    for b, r in enumerate(routes):
        rows[b, :len(r)] = r
    rng = np.random.default_rng(71)
    B, K = len(routes), 7
    return dict(rows=rows, counts=np.array([len(r) for r in routes], dtype=np.int32), follower=tr.follower(), P=perturbations(rng, B, K),
                O=records(rng, B, K), sensors=rc.SENSORS4, scene=seeded_scene(), rule=rule(GATE_IN, INCIDENCE_DEG, GAIN, every))


@functools.lru_cache(maxsize=None)
def layout_case(K, B):
    """Synthetic rows of 40 .. 200 rows, counts below the capacity, a route with n = 0, invalid perturbation and invalid
    odometry records."""
    rng = np.random.default_rng(100 * K + B)
    cap = int(rng.integers(40, 201))
    if K >= 256:
        cap = min(cap, 60)
    rows = synth_rows(rng, B, cap)
    counts = rng.integers(max(cap // 2, 2), cap + 1, B).astype(np.int32)
    counts[0] = cap
    if B >= 3:
        counts[1] = 0
    P, O = perturbations(rng, B, K), records(rng, B, K)
    if K >= 3:
        P[-1, 1, 3] = -1.0             # a gain <= 0
        O[0, 2, 0] = 0.0               # enc_left <= 0
        O[-1, K - 1, 4] = np.nan       # a non-finite range_scale
    return dict(rows=rows, counts=counts, follower=tr.follower(settle_rows=15), P=P, O=O, sensors=rc.SENSORS4, scene=seeded_scene(),
                rule=rule(GATE_IN, INCIDENCE_DEG, GAIN, 3))


@functools.lru_cache(maxsize=None)
def tile_case(every):
    """K = 64: four routes per workgroup in tiles of 64 rows; routes of 63, 64, 65 and 129 rows and 10 settle rows, so the
    last tile (rows 128 .. 138) is partial and, with every = 64, the reset rows 0, 64, 128 are the tiles' first rows."""
    rng = np.random.default_rng(64 + every)
    K, ns = 64, list(TILE_ROWS) + list(TILE_ROWS[::-1])
    rows = synth_rows(rng, len(ns), 129)
    return dict(rows=rows, counts=np.array(ns, dtype=np.int32), follower=tr.follower(settle_rows=10), P=perturbations(rng, len(ns), K),
                O=records(rng, len(ns), K), sensors=rc.SENSORS4, scene=seeded_scene(), rule=rule(GATE_IN, INCIDENCE_DEG, GAIN, every))


TRACKING_TILE_K = (64, 256, 1)


@functools.lru_cache(maxsize=None)
def tracking_tile_case(K):
    """tile_case's routes for vap_tracking_rollouts at a capacity of 160 rows: K = 64 (four routes per workgroup, tiles of 64
    rows, the last one partial), K = 256 (one route per workgroup) and K = 1 (256 routes per workgroup, tiles of 2 rows) with
    260 routes, so that a second workgroup holds 4 routes and 252 idle lanes, one of them a route without rows."""
    base = tile_case(1)
    B = 260 if K == 1 else len(base["counts"])
    pick = np.arange(B) % len(base["counts"])
    rows = np.zeros((B, 160, 8))
    rows[:, :base["rows"].shape[1]] = base["rows"][pick]
    counts = base["counts"][pick].copy()
    if K == 1:
        counts[257] = 0
    P = base["P"] if K == 64 else perturbations(np.random.default_rng(640 + K), B, K)
    return dict(rows=rows, counts=counts, follower=base["follower"], P=P)


@functools.lru_cache(maxsize=None)
def scene_size_case(over):
    """range_cases.scene_size_case's scene, under and over the LDS budget of the packed scene."""
    rng = np.random.default_rng(200 + int(over))
    B, K = 5, 7
    rows = synth_rows(rng, B, 50)
    return dict(rows=rows, counts=np.full(B, 50, dtype=np.int32), follower=tr.follower(settle_rows=5), P=perturbations(rng, B, K),
                O=records(rng, B, K), sensors=rc.SENSORS4, scene=rc.scene_size_case(over)["scene"], rule=rule(GATE_IN, INCIDENCE_DEG, GAIN, 1))


@functools.lru_cache(maxsize=None)
def sensors_case(ns):
    """0, 1 or 8 sensors: the four of range_cases and four diagonal ones."""
    rng = np.random.default_rng(300 + ns)
    B, K = 4, 5
    rows = synth_rows(rng, B, 80)
    d = np.sqrt(0.5)
    diag = np.array([[0.4, 0.4, d, d, 0.1, 9.0, 0.3, 0.0], [-0.4, 0.4, -d, d, 0.1, 9.0, 0.3, 0.0],
                     [-0.4, -0.4, -d, -d, 0.1, 9.0, 0.3, 0.0], [0.4, -0.4, d, -d, 0.1, 9.0, 0.3, 0.0]])
    sens = np.concatenate([rc.SENSORS4, diag])[:ns] if ns else None
    return dict(rows=rows, counts=np.array([80, 80, 41, 7], dtype=np.int32), follower=tr.follower(settle_rows=8), P=perturbations(rng, B, K),
                O=records(rng, B, K), sensors=sens, scene=seeded_scene() if ns else None, rule=rule(GATE_IN, 72.0, GAIN, 2) if ns else None)


def all_cases():
    """(name, case) of every case the GPU tests compare with the reference."""
    for every in (1, 5):
        yield f"golden every={every}", golden_case(every)
    for K, B in LAYOUTS:
        yield f"layout K={K} B={B}", layout_case(K, B)
    for every in (1, 64):
        yield f"tiles every={every}", tile_case(every)
    for over in (False, True):
        yield f"scene over={over}", scene_size_case(over)
    for ns in (0, 1, 8):
        yield f"sensors n={ns}", sensors_case(ns)


_REF = {}


def reference(case, rows_out=False):
    """(float64, longdouble) odometry_ref.rollouts of a case, computed once per case and kept."""
    key = (id(case), rows_out)
    if key not in _REF:
        args = (case["rows"], case["counts"], case["follower"], case["P"], case["O"], case["sensors"], packed(case["scene"]), case["rule"], DT)
        _REF[key] = tuple(orf.rollouts(*args, executed=rows_out, estimates=rows_out, dtype=F) for F in (np.float64, np.longdouble))
    return _REF[key]


def excused(r64, rld):
    """(B, K) bool: the rollouts that are checked for finiteness and the integer identities only — a decision margin below
    1e-9, different decisions in the two precisions, or max |e_phi| >= 3 rad — and (B, K) bool: the rollouts with a result."""
    B, K = r64["margin"].shape
    ok = r64["stat_rows"][..., 0] >= 0
    differ = ((r64["decisions"] != rld["decisions"]).any(axis=1) | (r64["stat_rows"].reshape(B * K, 4)[:, 1:] != rld["stat_rows"].reshape(B * K, 4)[:, 1:]).any(axis=1)).reshape(B, K)
    exc = ok & ((r64["margin"] < AMBIGUOUS) | differ | (np.nan_to_num(r64["stats"][..., 2]) >= EXCLUDE_RAD))
    return exc, ok


def tol_of(a64, ald):
    d = np.abs(a64.astype(np.longdouble) - ald).astype(np.float64)
    return np.minimum(np.maximum(FLOOR, FACTOR * d), CAP), d
