"""Odometry rollouts without a device: the export, the declaration and the binding; the Python layer's conversions and
refusals; the C-ABI's host validation (it runs before the context is touched); tests/odometry_ref.py on cases worked by hand;
and the cap on excused rollouts, held on the reference alone on the inputs test_gpu_odometry.py runs."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import odometry_cases as oc
import odometry_ref as orf
import range_cases as rc
import range_ref as rr
import tracking_ref as tr
from vexautonomousplanner_amd import _lib, odometry, sensors, tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.01
HALF = rc.HALF
WALLS = orf.PackedScene(rc.FIELD)
FRONT = np.array([[0.6, 0.0, 1.0, 0.0, 0.0, 20.0, 0.0, 0.0]])
LEFT = np.array([[0.0, 0.6, 0.0, 1.0, 0.0, 20.0, 0.0, 0.0]])


def straight(n=200, x0=-3.0, v=1.0):
    """n rows along +x at heading 0 from (x0, 0) at v ft/s."""
    rows = np.zeros((1, n, 8))
    rows[0, :, 0] = np.arange(n) * DT
    rows[0, :, 1] = rows[0, :, 0] * v
    rows[0, :, 2] = v
    rows[0, :, 6] = x0 + rows[0, :, 1]
    return rows


def roll(rows, O, sens=None, scene=None, reset=None, P=tr.NOMINAL, f=None):
    f = f or tr.follower(settle_rows=20)
    return orf.rollouts(rows, [rows.shape[1]], f, np.atleast_2d(P), np.atleast_2d(O), sens, scene, reset, DT, executed=True, estimates=True)


# ---- the export, the declaration, the binding, the package ---------------------------------------------------------------------
def test_entry_point_is_exported_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "vap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+vap_odometry_rollouts\s*\(([^;]*)\)\s*;", code)
    assert m, "vap_odometry_rollouts is not declared in include/vap.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert len(args) == 33 and args[0] == "vap_ctx *ctx" and args[15] == "const vap_reset_rule *rule" and args[-1] == "double *d_est_rows"
    assert len(_lib.lib().vap_odometry_rollouts.argtypes) == 33
    assert "vap_odometry_rollouts" in _lib.EXPORTS and hasattr(_lib.lib(), "vap_odometry_rollouts")
    fields = re.search(r"typedef struct \{([^}]*)\}\s*vap_reset_rule;", code).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", fields) == [n for n, _ in _lib.ResetRuleStruct._fields_]
    import vexautonomousplanner_amd as pkg
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    assert "odometry" in pkg.__all__ and pkg.odometry is odometry
    assert callable(BatchedTrajectoryGenerator.odometry_rollouts)


def test_reset_rule_converts_inches_and_degrees():
    r = odometry.ResetRule(6.0, 60.0, 0.5, 3)
    s = r.as_struct()
    assert (s.gate, s.min_cos, s.gain, s.every) == (0.5, min(1.0, math.cos(math.radians(60.0))), 0.5, 3)
    assert odometry.ResetRule(1.0, 90.0).min_cos == 0.0 and odometry.ResetRule(1.0, 0.0).min_cos == 1.0
    c = oc.rule(6.0, 60.0, 0.5, 3)
    assert (c["gate"], c["min_cos"]) == (s.gate, s.min_cos)
    for kw in (dict(gate_in=-1.0), dict(gate_in=float("inf")), dict(gate_in=float("nan")), dict(max_incidence_deg=91.0),
               dict(max_incidence_deg=-1.0), dict(gain=1.5), dict(gain=-0.1), dict(gain=float("nan")), dict(every=0), dict(every=10001),
               dict(every=2.5)):
        with pytest.raises(ValueError):
            odometry.ResetRule(**kw)


def test_sample_records():
    a, b = odometry.sample_records(3, 5, seed=4), odometry.sample_records(3, 5, seed=4)
    assert a.shape == (3, 5, 8) and (a == b).all() and (a != odometry.sample_records(3, 5, seed=5)).any()
    assert (a[:, 0] == np.array(odometry.IDEAL)).all() and (a[..., 6:] == 0).all() and orf.record_valid(a.reshape(-1, 8)).all()
    assert (odometry.sample_records(2, 4, 0, 0, 0, 0, 0) == np.array(odometry.IDEAL)).all()
    assert "measured" in odometry.sample_records.__doc__ and "measured" in odometry.ResetRule.__doc__
    for kw in (dict(K=0), dict(K=4097), dict(B=-1), dict(enc_sigma=-1.0), dict(drift_sigma=float("nan"))):
        with pytest.raises(ValueError):
            odometry.sample_records(**dict(dict(B=1, K=2), **kw))


def test_python_refusals_come_before_the_device():
    rows, P, O = np.zeros((4, 8)), np.zeros((2, 8)), np.zeros((2, 8))
    f, rule, scene = tracking.Follower(), odometry.ResetRule(), None
    from vexautonomousplanner_amd import footprint as fp
    scene = fp.Scene(field=rc.FIELD)
    with pytest.raises(TypeError):
        odometry.rollouts(rows, None, tracking.Pursuit(), P, O)
    with pytest.raises(TypeError):
        odometry.rollouts(rows, None, object(), P, O)
    with pytest.raises(TypeError):
        odometry.rollouts(rows, None, f, P, O, sensors=rc.SENSORS4, scene=None, rule=rule)
    with pytest.raises(TypeError):
        odometry.rollouts(rows, None, f, P, O, sensors=rc.SENSORS4, scene=scene, rule=None)
    bad = rc.SENSORS4.copy()
    bad[0, 2] = 0.5
    for kw in (dict(follower=tracking.Follower(n_substeps=0)), dict(follower=tracking.Follower(track_width=0.0)), dict(time_step=0.0),
               dict(time_step=float("nan")), dict(sensors=bad, scene=scene, rule=rule), dict(sensors=np.zeros((9, 8)), scene=scene, rule=rule),
               dict(records=np.zeros((3, 8))), dict(records=np.zeros((2, 7))), dict(perturbations=np.zeros((2, 2, 2, 8)))):
        args = dict(follower=f, perturbations=P, records=O)
        args.update(kw)
        with pytest.raises(ValueError):
            odometry.rollouts(rows, None, args.pop("follower"), args.pop("perturbations"), args.pop("records"), **args)


def test_abi_checks_its_arguments_before_the_context():
    """With a null context a bad argument is reported as that argument, a good call as the null context."""
    L = _lib.lib()
    one = (C.c_double * 8)(*tr.NOMINAL)
    odo = (C.c_double * 8)(*orf.IDEAL)
    cnt = (C.c_int * 2)(4, 0)
    rows = (C.c_double * 32)()
    sens = np.ascontiguousarray(rc.SENSORS4)
    field = np.array(rc.FIELD)
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.dp)
    buf = np.zeros(4 * 54 * 4 + 2)

    def call(n_sens=4, sensors=sens, rule=(0.5, 0.5, 1.0, 1), odo=odo, est=None, cap_exec=54, K=1, fld=field, n_circle=0, circles=None, **kw):
        fs = tracking.Follower(**kw).as_struct()
        rs = None if rule is None else _lib.ResetRuleStruct(*rule)
        st = L.vap_odometry_rollouts(None, 1, 4, rows, cnt, 2, 0.01, C.byref(fs), K, 0, one, 0, odo, n_sens, dp(sensors),
                                     None if rs is None else C.byref(rs), dp(fld), 0, None, None, n_circle, dp(circles), None, None, None,
                                     None, None, None, None, cap_exec, None, None, est)
        return st, L.vap_last_error().decode()

    for kw in (dict(), dict(n_sens=0, sensors=None, rule=None, fld=None), dict(n_sens=0), dict(est=C.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16))):
        st, msg = call(**kw)
        assert st == _lib.VAP_ERR_INVALID and "null context" in msg, (kw, msg)
    bad = sens.copy()
    bad[1, 6] = 1.5
    for kw, word in ((dict(n_sens=-1), "sensors"), (dict(n_sens=9), "sensors"), (dict(rule=(-0.1, 0.5, 1.0, 1)), "gate"),
                     (dict(rule=(float("inf"), 0.5, 1.0, 1)), "gate"), (dict(rule=(float("nan"), 0.5, 1.0, 1)), "gate"),
                     (dict(rule=(0.5, 1.1, 1.0, 1)), "min_cos"), (dict(rule=(0.5, -0.1, 1.0, 1)), "min_cos"), (dict(rule=(0.5, float("nan"), 1.0, 1)), "min_cos"),
                     (dict(rule=(0.5, 0.5, 1.1, 1)), "gain"), (dict(rule=(0.5, 0.5, -0.1, 1)), "gain"), (dict(rule=(0.5, 0.5, 1.0, 0)), "every"),
                     (dict(rule=(0.5, 0.5, 1.0, 10001)), "every"), (dict(rule=None), "null reset rule"), (dict(sensors=None), "null sensors"),
                     (dict(odo=None), "null odometry"), (dict(odo=C.c_void_p(C.addressof(odo) + 8)), "aligned"),
                     (dict(est=C.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16 + 8)), "aligned"),
                     (dict(est=C.c_void_p(buf.ctypes.data + (-buf.ctypes.data) % 16), cap_exec=53), "cap_exec"), (dict(sensors=bad), "min_cos"),
                     (dict(n_substeps=0), "n_substeps"), (dict(K=0), "K ="), (dict(fld=np.array([1.0, 0.0, 0.0, 1.0])), "field"),
                     (dict(n_circle=1, circles=np.array([0.0, 0.0, -1.0])), "circle")):
        st, msg = call(**kw)
        assert st == _lib.VAP_ERR_INVALID and word in msg and "null context" not in msg, (kw, msg)
    st, msg = call(n_circle=257, circles=np.ones(257 * 3))
    assert st == _lib.VAP_ERR_UNSUPPORTED and "null context" not in msg, msg


# ---- the reference's cast is range_ref's ----------------------------------------------------------------------------------------
def test_cast_equals_range_ref():
    rng = np.random.default_rng(3)
    sc = oc.seeded_scene()
    pk = oc.packed(sc)
    n = 400
    h, x, y = rng.uniform(-np.pi, np.pi, n), rng.uniform(-HALF - 0.3, HALF + 0.3, n), rng.uniform(-HALF - 0.3, HALF + 0.3, n)
    h[5], x[6] = np.nan, np.inf
    for scene, args in ((pk, (sc["field"], sc["polygons"], sc["circles"])), (orf.PackedScene(None, sc["polygons"], sc["circles"]), (None, sc["polygons"], sc["circles"])),
                        (WALLS, (rc.FIELD,))):
        for s in rc.SENSORS4:
            a, b = orf.cast(h, x, y, s, scene), rr.cast(h, x, y, s, *args)
            for k in ("status", "face", "element"):
                assert (a[k] == b[k]).all(), k
            for k in ("t", "cos"):
                assert (a[k].view(np.int64) == b[k].view(np.int64)).all(), k
            taken = b["status"] == rr.VALID
            assert taken.any() and (a["margin"][taken] == np.where(b["cos"][taken] < rr.COS_EXCUSE, 0.0, b["margin"][taken])).all()
            assert (a["margin"] == b["margin"])[~taken].all()


# ---- hand-computed cases ------------------------------------------------------------------------------------------------------
def test_ideal_record_without_sensors_is_tracking_ref_bit_for_bit():
    rng = np.random.default_rng(8)
    rows = oc.synth_rows(rng, 1, 90)
    P = oc.perturbations(rng, 1, 6)
    P[..., 0:3] = 0.0
    f = tr.follower(settle_rows=12)
    for F in (np.float64, np.longdouble):
        a = orf.rollouts(rows, [77], f, P, orf.IDEAL[None], None, None, None, DT, True, True, F)
        b = tr.rollout(rows[0], 77, f, P[0], DT, executed=True, dtype=F)
        assert (a["stats"][0][:, :5] == b["stats"][:, :5]).all() and (a["stats"][0][:, 5:] == 0).all()
        assert (a["stat_rows"][0][:, :2] == b["stat_rows"]).all() and (a["stat_rows"][0][:, 2:] == 0).all()
        assert (a["e_pos"][:, :89] == b["e_pos"]).all() and (a["rows"][:, :89] == b["rows"]).all() and (a["counts"] == b["counts"]).all()
        assert (a["est_rows"][:, :89, :3] == a["rows"][:, :89][:, :, [4, 6, 7]]).all()
        s = tr.route_summary(b["stats"], b["stat_rows"], f["tolerance"])
        assert (a["worst"][0], a["mean"][0], a["worst_rollout"][0], a["worst_row"][0], a["n_exceeding"][0]) == \
            (s["worst"], s["mean"], s["worst_rollout"], s["worst_row"], s["n_exceeding"])
    # a start offset is the true pose's alone: the estimate starts on row 0
    P2 = oc.perturbations(rng, 1, 3)
    c = orf.rollouts(rows, [77], f, P2, orf.IDEAL[None], None, None, None, DT, True, True)
    assert (c["est_rows"][:, 0, 1:3] == rows[0, 0, 6:8]).all() and (c["rows"][1:, 0, 6:8] != rows[0, 0, 6:8]).any()
    assert np.allclose(c["stats"][0, 1:, 5], np.hypot(P2[0, 1:, 0], P2[0, 1:, 1]), atol=0.05) and (c["stats"][0, 1:, 5] > 0).all()


def test_encoder_error_grows_with_the_distance():
    O = orf.IDEAL.copy()
    O[0:2] = 1.02
    r = roll(straight(), O)
    dist, eest = r["rows"][0, :, 1], np.hypot(r["est_rows"][0, :, 1] - r["rows"][0, :, 6], r["est_rows"][0, :, 2] - r["rows"][0, :, 7])
    assert dist[-1] > 1.5 and np.max(np.abs(eest - 0.02 * dist)) <= 1e-12
    assert abs(r["stats"][0, 0, 7] - 0.02 * dist[-1]) <= 1e-3 and r["stats"][0, 0, 5] >= eest.max()
    assert (r["stat_rows"][0, 0, 2:] == 0).all()


def test_front_sensor_with_gain_one_sets_x():
    O = orf.IDEAL.copy()
    O[0:2] = 1.02
    r = roll(straight(), O, FRONT, WALLS, orf.rule(10.0, 0.0, 1.0, 5))
    mask = r["est_rows"][0, :, 3]
    reset = np.nonzero(mask)[0]
    assert (reset == np.arange(0, 220, 5)).all() and r["stat_rows"][0, 0, 2] == 44 and r["stat_rows"][0, 0, 3] == 0
    # the estimate row is written before the reset of its own row is driven on: the reset shows in the row itself
    assert np.max(np.abs(r["est_rows"][0, reset, 1] - r["rows"][0, reset, 6])) <= 1e-12
    between = np.setdiff1d(np.arange(220), reset)
    assert np.max(np.abs(r["est_rows"][0, between, 1] - r["rows"][0, between, 6])) > 1e-5
    assert r["stats"][0, 0, 5] < 0.02 * 0.05 + 1e-9                   # never further off than 2 % of five rows' travel


def test_heading_drift_and_a_side_sensor_on_a_y_wall():
    O = orf.IDEAL.copy()
    O[3] = 0.05
    free = roll(straight(), O)
    r = roll(straight(), O, LEFT, WALLS, orf.rule(10.0, 0.0, 1.0, 1))
    assert r["stat_rows"][0, 0, 2] == 220 and (r["est_rows"][0, :, 3] == 1).all()
    ey_free = np.abs(free["est_rows"][0, :, 2] - free["rows"][0, :, 7])
    ey = np.abs(r["est_rows"][0, :, 2] - r["rows"][0, :, 7])
    print(f"heading drift 0.05 rad/s: final |y_hat - y| {ey_free[-1]:.4f} ft without the sensor, {ey[-1]:.6f} ft with it")
    assert ey_free[-1] > 0.05 and ey.max() < 0.1 * ey_free[-1]
    # the heading estimate is untouched: it is off by the drift alone, with and without the resets
    for q in (free, r):
        dphi = -q["est_rows"][0, :, 0] - (-q["rows"][0, :, 4])
        assert np.max(np.abs(dphi - 0.05 * np.arange(220) * DT)) <= 1e-12
    assert abs(r["stats"][0, 0, 6] - 0.05 * 219 * DT) <= 1e-12


def test_a_post_outside_the_gate_is_rejected_and_counted():
    post = orf.PackedScene(rc.FIELD, (), [(2.0, 0.0, 0.2)])
    O = orf.IDEAL.copy()
    O[0:2] = 1.02
    r = roll(straight(100), O, FRONT, post, orf.rule(0.5, 0.0, 1.0, 1))
    free = roll(straight(100), O)
    assert (r["stat_rows"][0, 0, 2:] == (0, 120)).all() and (r["est_rows"][0, :, 3] == 0).all()
    assert (r["rows"] == free["rows"]).all() and (r["est_rows"][..., :3] == free["est_rows"][..., :3]).all()
    assert (r["decisions"][0] == 1 << 8).all()


def test_a_post_inside_the_gate_gives_a_wrong_reset_of_known_size():
    post = orf.PackedScene(rc.FIELD, (), [(HALF - 0.15, 0.0, 0.1)])           # its face is 0.25 ft in front of the wall
    r = roll(straight(100), orf.IDEAL.copy(), FRONT, post, orf.rule(0.5, 0.0, 1.0, 1))
    assert (r["stat_rows"][0, 0, 2:] == (120, 0)).all()
    off = r["est_rows"][0, :, 1] - r["rows"][0, :, 6]
    assert np.max(np.abs(off - (HALF - (HALF - 0.15 - 0.1)))) <= 1e-12
    assert abs(r["stats"][0, 0, 7] - 0.25) <= 1e-12 and abs(r["stats"][0, 0, 5] - 0.25) <= 1e-12


def test_range_bias_moves_the_estimate_by_gain_times_bias():
    O = orf.IDEAL.copy()
    O[5] = 0.1
    gain = 0.5
    r = roll(straight(100), O, FRONT, WALLS, orf.rule(1.0, 0.0, gain, 10))
    off = r["est_rows"][0, :, 1] - r["rows"][0, :, 6]
    k = np.arange(120) // 10 + 1                                              # resets taken up to and including row r
    assert r["stat_rows"][0, 0, 2] == 12 and abs(off[0] + gain * 0.1 * 1.0) <= 1e-15
    assert np.max(np.abs(off + 0.1 * (1 - (1 - gain) ** k))) <= 1e-12


def test_without_a_field_every_valid_reading_is_rejected():
    post = orf.PackedScene(None, (), [(4.0, 0.0, 0.3)])
    r = roll(straight(100), orf.IDEAL.copy(), FRONT, post, orf.rule(10.0, 0.0, 1.0, 1))
    assert (r["stat_rows"][0, 0, 2:] == (0, 120)).all()
    none = roll(straight(100), orf.IDEAL.copy(), LEFT, post, orf.rule(10.0, 0.0, 1.0, 1))     # nothing in the beam: no reading, no count
    assert (none["stat_rows"][0, 0, 2:] == (0, 0)).all()


def test_invalid_records_and_empty_routes():
    rows = np.concatenate([straight(30), straight(30)])
    O = np.stack([orf.IDEAL, orf.IDEAL, orf.IDEAL, orf.IDEAL, orf.IDEAL])
    O[1, 0], O[2, 2], O[3, 4], O[4, 7] = 0.0, -1.0, 0.0, np.nan
    r = orf.rollouts(rows, [30, 0], tr.follower(settle_rows=3), np.broadcast_to(tr.NOMINAL, (5, 8)), O, None, None, None, DT, True, True)
    assert (r["stat_rows"][0, 0] >= 0).all() and (r["stat_rows"][0, 1:] == -1).all() and (r["stat_rows"][1] == -1).all()
    assert np.isnan(r["stats"][0, 1:]).all() and np.isnan(r["stats"][1]).all() and (r["counts"] == [33, 0, 0, 0, 0, 0, 0, 0, 0, 0]).all()
    assert r["worst_rollout"][0] == 0 and r["worst_rollout"][1] == -1 and np.isnan(r["worst"][1]) and r["n_exceeding"][1] == 0


# ---- the excuse cap, on the inputs the GPU tests run ------------------------------------------------------------------------------
def test_excused_rollouts_stay_under_the_cap():
    for name, case in oc.all_cases():
        r64, rld = oc.reference(case, True)
        exc, ok = oc.excused(r64, rld)
        n_ok, n_exc = int(ok.sum()), int(exc.sum())
        sr = r64["stat_rows"][ok]
        print(f"{name}: {n_exc} of {n_ok} rollouts excused ({n_exc / max(n_ok, 1):.2%}); resets accepted {int(sr[:, 2].sum())}, "
              f"rejected {int(sr[:, 3].sum())}; smallest margin {r64['margin'][ok].min():.2e}")
        assert n_ok > 0 and n_exc <= oc.MAX_EXCUSED * n_ok, name
        if case["sensors"] is not None:
            assert sr[:, 2].sum() > 0 and sr[:, 3].sum() > 0, name
