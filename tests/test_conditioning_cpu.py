"""CPU: the definition of vap_velocity_conditioning (include/vap.h) through tests/conditioning_ref.py.

(a) the replica's unperturbed sweep is the reference's velocity row on the curated fixtures (<= 1e-12; measured <= 5.2e-15);
(b) the conditioning number separates fixture big_w2048_p2 — the one path on which every implementation of the recurrence
    differs from the reference by 1e-6 — from those fixtures by a factor of 1000 at the least (measured >= 4e4);
(c) it predicts the rounding-level difference between two fp64 statements of the recurrence (the replica's u-space sweep and
    the oracle's v-space sweep, on the same rows): difference <= F * cond * 2^-53;
(d) the entry point's argument errors by value, without a device.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import conditioning_ref as cr
import golden_util as gu
from oracle import oracle
from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints

CURATED = ("c3_p0_S10000", "c1_w8", "plain_w32_s0", "plain_w32_s3", "c5_p0_S1024", "cons_other_robot_S1024")
SEEDS = (0, 1, 2)
# (c): the largest |replica - oracle| / (cond * 2^-53) measured over the 33 cases below was 1.03 (the 16 walks 0.20 .. 1.03,
# their tight variants 0.08 .. 0.93, big_w2048_p2 0.30); F is 8 times that.
MEASURED_RATIO = 1.03
F = 8 * MEASURED_RATIO


def rel_diff(v, ref):
    return float(np.max(np.abs(v - ref) / ref))


@functools.lru_cache(maxsize=None)
def curated(name, seed=0, K=1):
    g = gu.load(name)
    N = int(g["n_samples"])
    r = cr.probe(g["grid_curvature"], cr.dtheta(g["grid_heading"]), N, float(g["dd"]), g["constraints"], float(g["start_vel"]),
                 float(g["end_vel"]), K=K, seed=seed)
    return r, g["grid_velocity"]


@functools.lru_cache(maxsize=None)
def big():
    """big_w2048_p2 on the oracle's rows: the unperturbed sweep once, one probe for each of three seeds."""
    g = gu.load("big_w2048_p2")
    p = oracle.OraclePath(g["waypoints"])
    p.rebuild_tables()
    fb = p.forward_backward(g["constraints"], float(g["dd"]), float(g["start_vel"]), float(g["end_vel"]))
    N = len(fb["velocity"])
    assert N == int(g["n_samples"])
    kap, dth = fb["curvature"], cr.dtheta(fb["heading"])
    args = (N, float(g["dd"]), g["constraints"], float(g["start_vel"]), float(g["end_vel"]))
    u0 = np.array(cr.sweep(kap, dth, *args))
    conds, worst = [], []
    for seed in SEEDS:
        s, sp = cr.signs(N, 1, seed, 0)
        uk = np.array(cr.sweep(kap * (1.0 + s * 2.0 ** -40), dth * (1.0 + sp * 2.0 ** -40), *args))
        r = np.abs(uk - u0) / u0
        conds.append(float(r.max() / 2.0 ** -39))
        worst.append(int(np.argmax(r)))
    return dict(conds=conds, worst=worst, velocity=np.sqrt(u0), oracle_velocity=fb["velocity"], reference_velocity=g["velocity_full"])


@pytest.mark.parametrize("name", CURATED)
def test_unperturbed_sweep_is_the_reference_row(name):
    r, want = curated(name)
    err = rel_diff(r["velocity"][:len(want)], want)
    print(f"COND {name}: replica vs golden velocity {err:.2e}, cond {r['cond']:.3g} at sample {r['worst_sample']}")
    assert err <= 1e-12
    assert r["cond"] > 0.0 and r["worst_probe"] == 1 and 0 <= r["worst_sample"] < len(want)


def test_big_path_stands_out_by_three_orders():
    b = big()
    for seed, cb in zip(SEEDS, b["conds"]):
        top = max(curated(n, seed)[0]["cond"] for n in CURATED)
        print(f"COND seed {seed}: big_w2048_p2 {cb:.3g} (sample {b['worst'][seed]}), curated fixtures <= {top:.3g}: x{cb / top:.3g}")
        assert cb >= 1000 * top


def walks():
    """16 random 32-waypoint walks at 4000 samples, and the same walks halved under a track three times as wide."""
    wp = make_waypoints(16, 32, 7, dtype=np.float64)
    tight = tuple(DEFAULT_CONSTRAINTS[:5]) + (3 * DEFAULT_CONSTRAINTS[5],)
    return (("walk", wp, DEFAULT_CONSTRAINTS), ("tight", 0.5 * wp, tight))


def test_cond_predicts_the_rounding_level_difference():
    """|replica - oracle| <= F * cond * 2^-53 with F = 8 x the largest ratio measured: two fp64 statements of one
    recurrence on the same rows differ by rounding alone, and cond says how far that rounding grows.  Measured: the ratio
    is 0.20 .. 1.03 on the walks, 0.08 .. 0.93 on their tight variants and 0.30 on big_w2048_p2; largest 1.03, F = 8.24."""
    S = 4000
    ratios = []
    for kind, wp, cons in walks():
        ref = oracle.profile_batch(wp, S, cons)
        for b in range(len(wp)):
            dd = ref["total_length"][b] / (S - 1.5)
            r = cr.probe(ref["curvature"][b], cr.dtheta(ref["heading"][b]), S, dd, cons, 0.01, 0.01, K=3, path=b)
            diff = rel_diff(r["velocity"], ref["velocity"][b])
            ratios.append((kind, b, diff, r["cond"], diff / (r["cond"] * 2.0 ** -53)))
    bg = big()
    diff = rel_diff(bg["velocity"], bg["oracle_velocity"])
    ratios.append(("big_w2048_p2", 0, diff, max(bg["conds"]), diff / (max(bg["conds"]) * 2.0 ** -53)))
    for kind, b, diff, cond, ratio in ratios:
        print(f"COND predict {kind} {b}: difference {diff:.2e}, cond {cond:.3g}, ratio {ratio:.2f}")
    print(f"COND predict: largest ratio {max(x[4] for x in ratios):.2f}")
    for kind, b, diff, cond, ratio in ratios:
        assert diff <= F * cond * 2.0 ** -53, (kind, b, diff, cond)


def test_entry_point_checks_its_arguments_before_the_device():
    """The call's own VAP_ERR_INVALID cases, by value, with a null context.  A call whose arguments are all good gets as
    far as the context and fails there ("null context")."""
    from vexautonomousplanner_amd import _lib, conditioning
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    L = _lib.lib()
    assert "vap_velocity_conditioning" in _lib.EXPORTS and callable(conditioning.probe)
    assert callable(BatchedTrajectoryGenerator.conditioning)
    header = open(_lib.HERE + "/../include/vap.h").read()
    assert "#define VAP_FLAG_ILLCONDITIONED 1024u" in header and "VAP_OPT_CONDITIONING_SCRATCH_MB = 6" in header
    assert conditioning.FLAG_ILLCONDITIONED == _lib.FLAG_ILLCONDITIONED == cr.ILLCONDITIONED == 1024
    one = C.c_void_p(16)
    cons = _lib.make_constraints(DEFAULT_CONSTRAINTS)

    def call(B=4, S=16, K=3, delta=2.0 ** -40, limit=1e6, c=C.byref(cons), meta=one, curv=one, dth=one, vcap=None, af=None,
             ab=None, db=None, cond=one):
        st = L.vap_velocity_conditioning(None, _lib.VAP_F64, B, S, c, 0.01, 0.01, meta, curv, dth, vcap, af, ab, db, K, delta, 0, 0,
                                         limit, cond, None, None, None, None, None)
        return st, L.vap_last_error().decode()

    INV = _lib.VAP_ERR_INVALID
    assert call() == (INV, "null context")
    assert call(B=0) == (INV, "null context")                            # B = 0 is a no-op of a live context only
    for K in (0, 2, 4, 5, 8, 16, -1):
        st, msg = call(K=K)
        assert st == INV and "probes" in msg, (K, msg)
    for K in (1, 3, 7, 15):
        assert call(K=K)[1] == "null context"
    for delta in (3 * 2.0 ** -41, 1e-12, 0.0, -2.0 ** -40, 2.0 ** -49, 2.0 ** -19, math.nan, math.inf):
        st, msg = call(delta=delta)
        assert st == INV and "power of two" in msg, (delta, msg)
    for delta in (2.0 ** -48, 2.0 ** -30, 2.0 ** -20):
        assert call(delta=delta)[1] == "null context"
    for limit in (0.0, -1.0, math.nan, -math.inf):
        st, msg = call(limit=limit)
        assert st == INV and "cond_limit" in msg, (limit, msg)
    assert call(limit=math.inf)[1] == "null context"
    assert call(cond=None) == (INV, "null buffer")
    assert call(B=0, cond=None)[1] == "null context"
    # the argument errors of vap_velocity_pass_limits
    assert call(B=-1)[0] == INV and "batch" in call(B=-1)[1]
    assert call(S=1)[0] == INV and "sample capacity" in call(S=1)[1]
    assert call(c=None) == (INV, "null buffer") and call(meta=None) == (INV, "null buffer")
    st, msg = call(af=one)
    assert st == INV and "come as a set" in msg
    st, msg = call(af=one, ab=one, db=one)                               # ... together with d_vcap
    assert st == INV and "come as a set" in msg
    assert call(af=one, ab=one, db=one, vcap=one)[1] == "null context"
