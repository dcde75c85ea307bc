"""CPU: the pure-pursuit rollout definitions (include/vap.h, vap_pursuit_rollouts) through the NumPy reference of
tests/pursuit_ref.py — analytic cases, degenerate routes, the reference's own rows of the golden fixtures — and the host
side of vexautonomousplanner_amd.tracking: Pursuit, lookahead_sweep, the dispatch of ``rollouts`` on the follower's type,
the C-ABI's argument checks (they run before the context is touched, so they need no device) and the declaration."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import golden_util as gu
import pursuit_ref as pr
from vexautonomousplanner_amd import _lib, tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.01

# Undisturbed rollout at the default lookahead (0.75 ft, 2 substeps, 150 settle rows) on the reference's own rows: this
# reference gives 0.1014 (c1_w8), 0.0956 (feat_limits), 0.0952 (feat_stop), 0.0952 ft (feat_wait) on the plain fixtures,
# where pure pursuit cuts the corners by about L^2 kappa / 8, and 0.3535 ft on feat_turn, where the plan turns on the spot
# and this follower swings round instead.  The plain bound is 1.5 x the largest plain value.
PLAIN_BOUND = 1.5 * 0.1014
TURN_BOUND = 0.25


def line_rows(n, v=2.0):
    """A straight line along x at constant speed in the time-profile layout."""
    rows = np.zeros((n, 8))
    t = np.arange(n) * DT
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 6] = t, v * t, v, v * t
    return rows


def circle_rows(n, radius=3.0, v=2.0):
    """A circle through the origin, tangent to x there, counter-clockwise, at constant speed."""
    th = v * np.arange(n) * DT / radius
    rows = np.zeros((n, 8))
    rows[:, 0], rows[:, 1], rows[:, 2] = np.arange(n) * DT, radius * th, v
    rows[:, 4], rows[:, 5] = -th, -v / radius
    rows[:, 6], rows[:, 7] = radius * np.sin(th), radius * (1 - np.cos(th))
    return rows


@pytest.mark.parametrize("L", [0.5, 1.0])
def test_lateral_offset_on_a_straight_line_overshoots_by_exp_minus_pi(L):
    """Linearised about a straight line at speed v, pure pursuit with lookahead L is y'' + (2 v / L) y' + (2 v^2 / L^2) y
    = 0: damping 1 / sqrt(2) for every L, so the first overshoot is exp(-pi) = 4.3214 % of a small offset, and the error
    then dies out."""
    off = 0.02
    rec = np.array(pr.NOMINAL)
    rec[1] = off
    out = pr.rollout(line_rows(900), 900, pr.pursuit(lookahead=L, settle_rows=0), rec, DT, executed=True)
    y = out["rows"][0][:, 7]
    assert y[0] == off and out["stat_rows"][0, 0] == 0 and out["stats"][0, 0] == pytest.approx(off, abs=1e-15)
    cross = int(np.argmax(y < 0))
    assert cross > 0 and (np.diff(y[:cross]) <= 0).all()
    over = -y.min() / off
    print(f"L = {L}: first overshoot {100 * over:.4f} % of the offset (exp(-pi) = {100 * math.exp(-math.pi):.4f} %)")
    assert over == pytest.approx(math.exp(-math.pi), rel=0.01)
    # decayed below 1e-6 of the offset before the prolonged tangent takes over (the last L of the line)
    keep = 900 - int(L / (2.0 * DT)) - 5
    assert np.abs(y[keep - 100:keep]).max() < 1e-6 * off
    assert out["stat_rows"][0, 1] == 0


def test_circle_is_its_own_pursuit_arc():
    """On a circle, tangent to it, the pursuit arc through a goal on the circle is the circle: away from the last L of
    arc (where the goal leaves along the prolonged tangent) e_ct stays at the polyline's level.  This reference gives
    1.74e-5 ft (the sagitta of a 0.02 ft chord on a 3 ft circle is 1.7e-5 ft); the bound is twice that."""
    n = 700
    rows = circle_rows(n)
    out = pr.rollout(rows, n, pr.pursuit(settle_rows=0), pr.NOMINAL, DT)
    e = out["e_ct"][0]
    keep = n - int(0.75 / (2.0 * DT)) - 5
    print(f"circle: max e_ct {e[:keep].max():.3e} ft away from the last lookahead, {e.max():.3e} ft overall")
    assert e[:keep].max() < 2 * 1.74e-5 < 1e-3
    assert out["stat_rows"][0, 1] == 0 and out["stat_rows"][0, 2] >= keep


def test_records_side_by_side_equal_records_one_at_a_time():
    rows = pr.golden_rows(gu.load("feat_wait"))
    P = tracking.sample_perturbations(1, 6, seed=4)[0]
    P[3, 3] = -1.0                                         # invalid: a gain <= 0
    P[4, 7] = -0.5                                         # invalid: slot 7 < 0
    P[5, 7] = 1.2
    both = pr.rollout(rows, len(rows), pr.pursuit(), P, DT, executed=True)
    for k in range(len(P)):
        one = pr.rollout(rows, len(rows), pr.pursuit(), P[k], DT, executed=True)
        for key in ("stats", "stat_rows", "rows", "counts"):
            np.testing.assert_array_equal(both[key][k], one[key][0], err_msg=f"{key} {k}")
    for k in (3, 4):
        assert np.isnan(both["stats"][k]).all() and both["stat_rows"][k].tolist() == [-1] * 4 and both["counts"][k] == 0
    assert not pr.record_valid(P)[3] and not pr.record_valid(P)[4] and pr.record_valid(P)[[0, 1, 2, 5]].all()
    s = pr.route_summary(both["stats"], both["stat_rows"], 0.25)
    valid = [0, 1, 2, 5]
    assert s["worst"] == both["stats"][valid, 0].max() and s["worst_rollout"] in valid and s["n_unfinished"] == 0
    assert pr.record_valid(tracking.NOMINAL).all() and pr.record_valid(tracking.sample_perturbations(2, 5).reshape(-1, 8)).all()


def test_degenerate_routes():
    rows = line_rows(40)
    f = pr.pursuit(settle_rows=10)
    none = pr.rollout(rows, 0, f, pr.NOMINAL, DT, executed=True)
    assert np.isnan(none["stats"]).all() and (none["stat_rows"] == -1).all() and none["counts"][0] == 0 and none["status"] == 0
    assert pr.route_summary(none["stats"], none["stat_rows"], 0.25) == dict(
        worst=pytest.approx(np.nan, nan_ok=True), mean=pytest.approx(np.nan, nan_ok=True), worst_rollout=-1, worst_row=-1,
        n_exceeding=0, n_unfinished=0)
    # n = 1 arrives at step 0 and stays: the start offset is the cross-track and the final error
    rec = np.array(pr.NOMINAL)
    rec[0], rec[1] = 0.3, -0.4
    one = pr.rollout(rows[5:], 1, pr.pursuit(settle_rows=10, min_speed=0.0), rec, DT, executed=True)
    assert one["stat_rows"][0].tolist() == [0, 0, 0, 0] and one["counts"][0] == 11
    assert one["stats"][0, 0] == pytest.approx(0.5, abs=1e-15) and one["stats"][0, 2] == 0.0
    # arrived at step 0: the command is 0 from the start and, with tau = 0, so are the wheels: the robot stays
    assert (one["cmd_max"][0] == 0).all() and one["stats"][0, 1] == pytest.approx(0.5, abs=1e-12)
    # a negative speed row: bit 0; a non-finite x: bit 1; both give what n = 0 gives
    neg = rows.copy()
    neg[17, 2] = -0.5
    o = pr.rollout(neg, 40, f, pr.NOMINAL, DT, executed=True)
    assert o["status"] == 1 and np.isnan(o["stats"]).all() and (o["stat_rows"] == -1).all() and o["counts"][0] == 0
    assert pr.rollout(neg, 17, f, pr.NOMINAL, DT)["status"] == 0          # the row is past the count
    bad = rows.copy()
    bad[3, 6] = np.inf
    o = pr.rollout(bad, 40, f, pr.NOMINAL, DT)
    assert o["status"] == 2 and np.isnan(o["stats"]).all()
    bad[9, 2] = -1.0
    assert pr.route_status(bad, 40) == 3
    bad[:, 4] = np.nan                                                    # columns 1, 3, 4, 5 do not count (4, 5: row 0's do start the pose)
    assert pr.route_status(bad, 40) == 3 and pr.route_status(rows, 40) == 0


def test_a_wait_in_the_middle_is_passed_over():
    """120 rows that stay on one point (v = 0) in the middle of a line: the segments without length are skipped, the
    robot does not dwell, and it arrives about 120 rows earlier than the plan's n."""
    base = line_rows(300)
    rows = np.concatenate([base[:150], np.repeat(base[150:151], 120, axis=0), base[150:]])
    rows[150:270, 2] = 0.0
    rows[:, 0] = np.arange(len(rows)) * DT
    n = len(rows)
    assert n == 420
    out = pr.rollout(rows, n, pr.pursuit(), pr.NOMINAL, DT)
    plain = pr.rollout(base, 300, pr.pursuit(), pr.NOMINAL, DT)
    arr, arr0 = int(out["stat_rows"][0, 2]), int(plain["stat_rows"][0, 2])
    print(f"wait route: {n} rows, arrived at step {arr}; without the wait {arr0} of 300")
    assert 0 <= arr0 <= 300 and abs(arr - arr0) <= 3 and abs((n - arr) - 120) <= 10
    assert out["stats"][0, 0] < 1e-12 and out["stat_rows"][0, 3] >= 270            # ic went past the wait rows


def test_slot_7_overrides_the_followers_lookahead():
    rows = pr.golden_rows(gu.load("c1_w8"))
    P = np.repeat(pr.NOMINAL[None], 3, axis=0)
    P[1, 7], P[2, 7] = 1.25, 0.75
    out = pr.rollout(rows, len(rows), pr.pursuit(lookahead=0.75), P, DT)
    other = pr.rollout(rows, len(rows), pr.pursuit(lookahead=1.25), pr.NOMINAL, DT)
    np.testing.assert_array_equal(out["stats"][:, 3], [0.75, 1.25, 0.75])
    np.testing.assert_array_equal(out["stats"][1], other["stats"][0])          # slot 7 = 1.25 is a follower with 1.25
    np.testing.assert_array_equal(out["stats"][0], out["stats"][2])            # 0 is the follower's own
    assert out["stats"][1, 0] > out["stats"][0, 0] + 0.01


def test_lookahead_sweep():
    P = tracking.sample_perturbations(2, 3, seed=1)
    la = [0.5, 0.0, 1.5, 1.0]
    S = tracking.lookahead_sweep(P, la)
    assert S.shape == (2, 12, 8) and S.dtype == np.float64
    for k in range(3):
        for m in range(4):
            np.testing.assert_array_equal(S[:, k * 4 + m, :7], P[:, k, :7])
            assert (S[:, k * 4 + m, 7] == la[m]).all()
    S1 = tracking.lookahead_sweep(P[0], la)
    np.testing.assert_array_equal(S1, S[0])
    assert (P[..., 7] == 0).all(), "the input is left as it was"
    assert pr.record_valid(S.reshape(-1, 8)).all()
    for bad in ([-0.1], [np.nan], []):
        with pytest.raises(ValueError):
            tracking.lookahead_sweep(P, bad)
    with pytest.raises(ValueError):
        tracking.lookahead_sweep(np.zeros((3, 7)), la)
    with pytest.raises(ValueError):
        tracking.lookahead_sweep(np.zeros((2048, 8)), [0.5, 1.0, 1.5])


@pytest.mark.parametrize("name", ["c1_w8", "feat_limits", "feat_stop", "feat_wait"])
def test_plain_goldens_arrive_and_stay_close(name):
    rows = pr.golden_rows(gu.load(name))
    f = pr.pursuit()
    out = pr.rollout(rows, len(rows), f, pr.NOMINAL, DT)
    st, sr = out["stats"][0], out["stat_rows"][0]
    print(f"{name}: {len(rows)} rows, undisturbed max e_ct {st[0]:.4f} ft at step {sr[0]}, arrived at step {sr[2]}, final {st[1]:.4f} ft")
    assert 0 <= sr[2] < len(rows) + f["settle_rows"] and st[2] == sr[2] * DT
    assert st[0] < PLAIN_BOUND
    assert st[1] <= 2 * f["arrive_tolerance"]
    P = tracking.sample_perturbations(1, 8, seed=3)[0]
    many = pr.rollout(rows, len(rows), f, P, DT)
    assert (many["stat_rows"][:, 2] >= 0).all(), "every disturbed rollout arrives within the settle rows"
    assert pr.route_summary(many["stats"], many["stat_rows"], f["tolerance"])["n_unfinished"] == 0


def test_the_in_place_turn_is_swung_round():
    rows = pr.golden_rows(gu.load("feat_turn"))
    out = pr.rollout(rows, len(rows), pr.pursuit(), pr.NOMINAL, DT)
    print(f"feat_turn: {len(rows)} rows, undisturbed max e_ct {out['stats'][0, 0]:.4f} ft at step {out['stat_rows'][0, 0]}")
    assert out["status"] == 0 and out["stats"][0, 0] > TURN_BOUND


def test_pursuit_defaults_and_validation():
    f = tracking.Pursuit()
    assert {k: getattr(f, k) for k in pr.DEFAULTS} == pr.DEFAULTS
    s = f.validate().as_struct()
    assert (s.track_width, s.lookahead, s.min_speed, s.arrive_tolerance, s.wheel_speed_max, s.tolerance, s.n_substeps, s.settle_rows) == \
        (1.0, 0.75, 0.1, 0.05, 6.0, 0.25, 2, 150)
    for kw in (dict(track_width=0), dict(lookahead=0), dict(lookahead=float("inf")), dict(wheel_speed_max=-1), dict(min_speed=-0.1),
               dict(arrive_tolerance=float("nan")), dict(tolerance=float("nan")), dict(n_substeps=0), dict(n_substeps=17),
               dict(n_substeps=1.5), dict(settle_rows=-1), dict(settle_rows=10001)):
        with pytest.raises(ValueError):
            tracking.Pursuit(**kw).validate()
    tracking.Pursuit(min_speed=0, arrive_tolerance=0, tolerance=float("inf")).validate()
    with pytest.raises(ValueError):
        tracking.rollouts(np.zeros((4, 8)), None, tracking.Pursuit(lookahead=0), np.zeros((1, 8)))
    with pytest.raises(TypeError):
        tracking.rollouts(np.zeros((4, 8)), None, dict(pr.DEFAULTS), np.zeros((1, 8)))


def test_abi_checks_its_arguments_before_the_context():
    """The C-ABI's host validation runs before the context is touched: with a null context a bad argument is reported
    as that argument, a good call as the null context."""
    L = _lib.lib()
    one = (C.c_double * 8)(*pr.NOMINAL)
    cnt = (C.c_int * 2)(4, 0)
    rows = (C.c_double * 40)()
    base = C.addressof(rows)
    aligned = C.c_void_p(base + (-base) % 16)
    off8 = C.c_void_p(aligned.value + 8)

    def call(B=1, cap=4, rows=aligned, counts=cnt, stride=2, dt=0.01, K=1, pert=one, f=None, cap_exec=0, exec_rows=None, stats=None, **kw):
        fs = tracking.Pursuit(**kw).as_struct() if f is None else f
        st = L.vap_pursuit_rollouts(None, B, cap, rows, counts, stride, dt, C.byref(fs) if fs else None, K, 0, pert,
                                    stats, None, None, None, None, None, None, None, None, cap_exec, exec_rows, None)
        return st, L.vap_last_error().decode()

    st, msg = call()
    assert st == _lib.VAP_ERR_INVALID and "null context" in msg
    st, msg = call(B=0)
    assert st == _lib.VAP_ERR_INVALID and "null context" in msg
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(track_width=0.0), "track_width"), (dict(track_width=inf), "track_width"), (dict(lookahead=0.0), "lookahead"),
                     (dict(lookahead=-1.0), "lookahead"), (dict(lookahead=nan), "lookahead"), (dict(wheel_speed_max=0.0), "wheel_speed_max"),
                     (dict(min_speed=-0.1), "min_speed"), (dict(min_speed=inf), "min_speed"), (dict(arrive_tolerance=-1e-9), "arrive_tolerance"),
                     (dict(arrive_tolerance=nan), "arrive_tolerance"), (dict(tolerance=nan), "tolerance is NaN"),
                     (dict(dt=0.0), "time_step"), (dict(dt=-0.01), "time_step"), (dict(dt=inf), "time_step"),
                     (dict(n_substeps=0), "n_substeps"), (dict(n_substeps=17), "n_substeps"), (dict(settle_rows=-1), "settle_rows"),
                     (dict(settle_rows=10001), "settle_rows"), (dict(K=0), "K ="), (dict(K=4097), "K ="), (dict(rows=None), "null rows"),
                     (dict(counts=None), "null rows"), (dict(pert=None), "perturbation"), (dict(stride=0), "counts_stride"),
                     (dict(B=-1), "bad shape"), (dict(cap=-1), "bad shape"), (dict(cap_exec=153, exec_rows=aligned), "cap_exec"),
                     (dict(rows=off8), "16-byte aligned"), (dict(stats=off8), "16-byte aligned"),
                     (dict(cap_exec=154, exec_rows=off8), "16-byte aligned")):
        st, msg = call(**kw)
        assert st == _lib.VAP_ERR_INVALID and word in msg and "null context" not in msg, (kw, msg)
    st, msg = call(cap_exec=154, exec_rows=aligned)               # capacity 4 + 150 settle rows fits: on to the context
    assert "null context" in msg
    st, msg = call(min_speed=0.0, arrive_tolerance=0.0, tolerance=inf)
    assert "null context" in msg
    st, msg = call(f=False)
    assert st == _lib.VAP_ERR_INVALID and "follower" in msg
    st, msg = call(cap=2**31 - 100, rows=aligned)
    assert st == _lib.VAP_ERR_UNSUPPORTED and "settle rows" in msg


def test_entry_point_is_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "vap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+vap_pursuit_rollouts\s*\(([^;]*)\)\s*;", code)
    assert m, "vap_pursuit_rollouts is not declared in include/vap.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert len(args) == 23 and args[0] == "vap_ctx *ctx" and args[7] == "const vap_pursuit *f"
    assert args[18:20] == ["int *d_n_unfinished", "int *d_route_status"]
    assert len(_lib.lib().vap_pursuit_rollouts.argtypes) == 23
    assert "vap_pursuit_rollouts" in _lib.EXPORTS and hasattr(_lib.lib(), "vap_pursuit_rollouts")
    fields = re.search(r"typedef struct \{([^}]*)\}\s*vap_pursuit;", code).group(1)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", fields)
    assert names == [n for n, _ in _lib.PursuitStruct._fields_]
    assert "reverse legs" in src and "in-place turns" in src


class _Called(Exception):
    pass


@pytest.mark.parametrize("follower,symbol", [(tracking.Follower(), "vap_tracking_rollouts"), (tracking.Pursuit(), "vap_pursuit_rollouts")])
def test_rollouts_dispatches_on_the_followers_type(monkeypatch, follower, symbol):
    """``rollouts`` reaches vap_tracking_rollouts with a Follower, as before, and vap_pursuit_rollouts with a Pursuit:
    everything between the type check and the C call is stubbed, and the ctypes symbols record which one was called."""
    import torch
    calls = []

    class FakeLib:
        def vap_tracking_rollouts(self, *a):
            calls.append(("vap_tracking_rollouts", len(a)))
            raise _Called()

        def vap_pursuit_rollouts(self, *a):
            calls.append(("vap_pursuit_rollouts", len(a)))
            raise _Called()

    class FakeCtx:
        _L, handle = FakeLib(), None

    cpu = torch.device("cpu")
    monkeypatch.setattr(tracking, "time_rows", lambda rows, counts, _, device: (
        torch.as_tensor(rows)[None], torch.tensor([[rows.shape[0], 0]], dtype=torch.int32), True, cpu))
    monkeypatch.setattr(tracking, "device_array", lambda a, dev, dtype: torch.as_tensor(a, dtype=dtype))
    monkeypatch.setattr(tracking, "buffers", lambda out, shapes, dev: {k: torch.zeros(s, dtype=d) for k, (s, d) in shapes.items()})
    monkeypatch.setattr(tracking, "context_for", lambda dev, ctx: FakeCtx())
    with pytest.raises(_Called):
        tracking.rollouts(np.zeros((4, 8)), None, follower, np.array([tracking.NOMINAL]))
    assert calls == [(symbol, 21 if symbol == "vap_tracking_rollouts" else 23)]
