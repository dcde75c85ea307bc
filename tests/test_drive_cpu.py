"""CPU: the references of the drive caps and the drive audit (tests/drive_ref.py), and the Python layer without a device.

Caps: drive_ref.caps goes into conditioning_ref.sweep(vcap=) — the replica test_gpu_conditioning.py holds the literal
velocity kernel to — on golden paths.  With A = 3 and A = 6 ft/s^2 the lateral cap binds and holds:
max(U |k|) over samples 1 .. N - 1 <= A (1 + 4 * 2^-52) — U is the squared velocity; the cap's own square is within 2 ulp of
A / |k| (a division, a square root and a square, each rounded once) and the product with |k| adds one more.  With A = 25.7
(mu = 0.8) it binds nowhere and changes no bit: the wheel-speed limit holds the goldens at 7.6 - 7.7 ft/s^2.
Audit: wL / wR are get_wheel_trajectory of the drop-in on the goldens' time-domain columns, aL / aR are MPG:612-616."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import conditioning_ref as cr
import drive_ref as dr
import golden_util as gu

GOLDENS = ("plain_w8_s0", "plain_w8_s1", "plain_w32_s0", "c3_p1_S1024")
BOUND = 1.0 + 4 * 2.0 ** -52


@functools.lru_cache(maxsize=None)
def path(name):
    g = gu.load(name)
    kap = np.asarray(g["grid_curvature"], dtype=np.float64)
    N = len(kap)
    L = float(g["total_length"])
    dd = float(g["dd"]) if float(g["dd"]) > 0 else L / (N - 1.5)
    cons = tuple(float(x) for x in g["constraints"])
    return dict(kap=kap, dth=cr.dtheta(g["grid_heading"]), N=N, dd=dd, cons=cons, sv=float(g["start_vel"]), ev=float(g["end_vel"]),
                golden=np.asarray(g["grid_velocity"], dtype=np.float64))


@functools.lru_cache(maxsize=None)
def swept(name, lateral=math.inf, angular=math.inf):
    """(U, n_bound, cap row) of the replica's sweep under the caps; no caps: the plain sweep."""
    p = path(name)
    vcap, nb = None, [0, 0]
    if lateral != math.inf or angular != math.inf:
        vcap, nb = dr.caps(p["kap"], p["N"], p["dd"], p["cons"][0], lateral, angular)
    U = np.array(cr.sweep(p["kap"], p["dth"], p["N"], p["dd"], p["cons"], p["sv"], p["ev"], vcap=vcap))
    return U, nb, vcap


def duration(name, U):
    p = path(name)
    return float(np.sum(p["dd"] / np.sqrt(U)))


@pytest.mark.parametrize("name", GOLDENS)
def test_plain_sweep_is_the_golden_row(name):
    U, _, _ = swept(name)
    err = float(np.max(np.abs(np.sqrt(U) - path(name)["golden"]) / path(name)["golden"]))
    print(f"DRIVE {name}: plain sweep vs golden {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("A", [3.0, 6.0])
def test_lateral_cap_binds_and_holds(name, A):
    p = path(name)
    U0, _, _ = swept(name)
    U, nb, vcap = swept(name, lateral=A)
    lat = float(np.max(U[1:] * np.abs(p["kap"][1:])))
    below = int(np.sum(vcap[1:p["N"] - 1] ** 2 < U0[1:p["N"] - 1]))
    print(f"DRIVE {name} A={A}: max v^2|k| = A * (1 + {lat / A - 1:.2e}), cap below the plain velocity on {below} of {p['N']} samples, "
          f"n_bound {nb}, sum dd/v {duration(name, U0):.3f} -> {duration(name, U):.3f} s")
    assert lat <= A * BOUND
    assert nb[0] > 0 and nb[1] == 0 and below > 0
    assert not np.array_equal(U, U0)
    assert duration(name, U) > duration(name, U0)


@pytest.mark.parametrize("name", GOLDENS)
def test_cap_of_mu_08_binds_nowhere_and_changes_no_bit(name):
    U0, _, _ = swept(name)
    U, nb, vcap = swept(name, lateral=25.7)
    p = path(name)
    print(f"DRIVE {name}: plain max v^2|k| = {float(np.max(U0[1:] * np.abs(p['kap'][1:]))):.2f} ft/s^2; n_bound at 25.7: {nb}")
    assert np.array_equal(U.view(np.int64), U0.view(np.int64))


@pytest.mark.parametrize("name", GOLDENS)
def test_curvature_rate_cap_binds(name):
    p = path(name)
    alpha = 2.0 * 8.0 / p["cons"][5]
    U0, _, _ = swept(name)
    U, nb, vcap = swept(name, angular=alpha)
    below = int(np.sum(vcap[1:p["N"] - 1] ** 2 < U0[1:p["N"] - 1]))
    print(f"DRIVE {name} alpha={alpha:.2f}: n_bound {nb}, below the plain velocity on {below} samples, sum dd/v "
          f"{duration(name, U0):.3f} -> {duration(name, U):.3f} s")
    assert nb[1] > 0 and nb[0] == 0
    assert not np.array_equal(U, U0)


def test_curvature_rate_end_quirk():
    """Three samples by hand: the two ends take the SUM of neighbouring curvatures over dd (MPG:180, 182), the middle the
    central difference."""
    k = np.array([0.5, 1.5, 4.0])
    dk = dr.curvature_derivs(k, 0.25)
    assert dk.tolist() == [(1.5 + 0.5) / 0.25, (4.0 - 0.5) / 0.5, (4.0 + 1.5) / 0.25] == [8.0, 7.0, 22.0]
    out, nb = dr.caps(k, 3, 0.25, 4.0, angular=32.0)
    assert out.tolist() == [math.sqrt(32.0 / 8.0), math.sqrt(32.0 / 7.0), math.sqrt(32.0 / 22.0)] and nb == [0, 3]
    # |dk| < 1e-9: max_vel (MPG:45-46); an incoming row below the cap stays; samples at and above N keep the incoming row
    out, nb = dr.caps(np.array([0.0, 0.0, 0.0, 9.0]), 3, 0.25, 4.0, lateral=1.0, angular=32.0, vin=np.array([5.0, 3.0, 4.0, 7.0]))
    assert out.tolist() == [4.0, 3.0, 4.0, 7.0] and nb == [0, 1]
    # the lateral cap: sqrt(A / |k|), off on a straight sample; a NaN curvature gives NaN; N < 2: no rate cap
    out, nb = dr.caps(np.array([4.0, 0.0, -1.0, math.nan]), 4, 0.25, 4.0, lateral=1.0)
    assert out[:3].tolist() == [0.5, 4.0, 1.0] and math.isnan(out[3]) and nb == [2, 0]
    out, nb = dr.caps(np.array([4.0, 1.0]), 1, 0.25, 4.0, angular=1e-6)
    assert out.tolist() == [4.0, 4.0] and nb == [0, 0]
    out, _ = dr.caps(np.array([4.0, 1.0]), 2, 0.25, 4.0, lateral=1.0, out_dtype=np.float32)
    assert out.dtype == np.float32 and out.tolist() == [0.5, 1.0]


@pytest.mark.parametrize("name", ("plain_w5_s0", "plain_w8_s0", "feat_turn", "feat_reverse"))
def test_audit_wheels_are_the_references(name):
    from vexautonomousplanner_amd.motion_profiling_v2.motion_profile_generator import get_wheel_trajectory
    g = gu.load(name)
    v, w = g["profile_linear_vels"], g["profile_angular_vels"]
    T, h = float(g["constraints"][5]), 0.01              # MPG:389: the reference's dt
    wh = dr.wheel_rows(v, w, T, h)
    left, right = get_wheel_trajectory(list(v), list(w), T)
    assert wh[:, 0].tolist() == [float(x) for x in left] and wh[:, 1].tolist() == [float(x) for x in right]
    # MPG:612-616, literally, for r >= 1 (at i = 0 the reference wraps to the last row; the audit starts from rest)
    la = [(left[i] - left[i - 1]) / h for i in range(len(left))]
    ra = [(right[i] - right[i - 1]) / h for i in range(len(right))]
    assert wh[1:, 2].tolist() == [float(x) for x in la[1:]] and wh[1:, 3].tolist() == [float(x) for x in ra[1:]]
    assert wh[0, 2] == left[0] / h and wh[0, 3] == right[0] / h
    a = dr.audit(v, w, len(v), T, h, [math.inf] * 5)
    print(f"DRIVE {name}: peaks {a['peak']} at rows {a['peak_row']}")
    assert a["status"] == 0 and a["peak"][0] == np.max(np.maximum(np.abs(left), np.abs(right)))


def test_synthetic_audit_rows():
    """Constant rows: every peak sits on the first row attaining it; a limit equal to the peak is not exceeded."""
    n, T, h = 40, 1.0, 0.5
    v, w = np.full(n, 2.0), np.full(n, 0.5)
    a = dr.audit(v, w, n, T, h, [2.25, 4.5, 9.0, 1.0, 1.0])
    # wL = 1.75, wR = 2.25; row 0 starts from rest: aR = 4.5, b = 4, j = 8 at row 0 and -8 at row 1; l = 1; g = 1 at row 0
    assert a["peak"].tolist() == [2.25, 4.5, 8.0, 1.0, 1.0]
    assert a["peak_row"].tolist() == [0, 0, 0, 0, 0]
    assert a["n_over"].tolist() == [0, 0, 0, 0, 0] and a["first_over"].tolist() == [-1] * 5
    below = [math.nextafter(x, 0.0) for x in (2.25, 4.5, 8.0, 1.0, 1.0)]
    a = dr.audit(v, w, n, T, h, below)
    assert a["n_over"].tolist() == [n, 1, 2, n, 1] and a["first_over"].tolist() == [0] * 5
    # a later, larger value moves the peak; an equal one does not
    v2 = v.copy()
    v2[10], v2[20] = 3.0, 3.0
    a = dr.audit(v2, w, n, T, h, [math.inf] * 5)
    assert a["peak"][0] == 3.25 and a["peak_row"][0] == 10
    # empty and non-finite routes
    a = dr.audit(v, w, 0, T, h, [0.0] * 5)
    assert np.isnan(a["peak"]).all() and a["peak_row"].tolist() == [-1] * 5 and a["n_over"].tolist() == [0] * 5 and a["status"] == 0
    w2 = w.copy()
    w2[7] = math.nan
    a = dr.audit(v, w2, n, T, h, [0.0] * 5)
    assert a["status"] == 2 and np.isnan(a["peak"]).all() and a["first_over"].tolist() == [-1] * 5 and len(a["wheel"]) == 0
    assert dr.audit(v, w2, 7, T, h, [0.0] * 5)["status"] == 0           # the NaN lies behind the route's rows
    # an in-place turn: v = 0, the wheels run against each other
    a = dr.audit(np.zeros(5), np.full(5, 2.0), 5, 1.5, h, [math.inf] * 5)
    assert a["peak"].tolist() == [1.5, 3.0, 0.0, 0.0, 4.0] and a["wheel"][0].tolist() == [-1.5, 1.5, -3.0, 3.0, 0.0, 0.0, 0.0, 4.0]


def test_python_layer_without_a_device():
    import vexautonomousplanner_amd as pkg
    from vexautonomousplanner_amd import _lib, drive
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    assert "drive" in pkg.__all__ and pkg.drive is drive
    assert callable(BatchedTrajectoryGenerator.apply_curve_caps) and callable(BatchedTrajectoryGenerator.drive_audit)
    c = _lib.make_constraints(DEFAULT_CONSTRAINTS)
    caps = drive.CurveCaps.from_constraints(DEFAULT_CONSTRAINTS)
    assert caps.lateral_acc_max == c.friction_coef * 32.174 and caps.angular_acc_max == math.inf
    caps = drive.CurveCaps.from_constraints(DEFAULT_CONSTRAINTS, g=9.81, lateral=False, angular=True)
    assert caps.lateral_acc_max == math.inf and caps.angular_acc_max == 2.0 * c.max_acc / c.track_width
    assert drive.CurveCaps().validate().lateral_acc_max == math.inf
    for bad in (math.nan, -1.0, 0.0):
        with pytest.raises(ValueError):
            drive.CurveCaps(lateral_acc_max=bad).validate()
        with pytest.raises(ValueError):
            drive.CurveCaps(angular_acc_max=bad).as_struct()
    lim = drive.Limits.from_constraints(DEFAULT_CONSTRAINTS)
    assert (lim.track_width, lim.wheel_speed_max, lim.wheel_acc_max, lim.jerk_max, lim.lateral_acc_max, lim.angular_acc_max) == \
        (c.track_width, c.max_vel, c.max_acc, c.max_jerk, c.friction_coef * 32.174, 2.0 * c.max_acc / c.track_width)
    assert drive.Limits(1.0, jerk_max=0.0).validate().jerk_max == 0.0
    for kw in (dict(track_width=0.0), dict(track_width=-1.0), dict(track_width=math.nan), dict(track_width=math.inf),
               dict(track_width=1.0, wheel_speed_max=math.nan), dict(track_width=1.0, jerk_max=-1.0)):
        with pytest.raises(ValueError):
            drive.Limits(**kw).validate()
    with pytest.raises(TypeError):
        drive.audit(np.zeros((3, 8)), None, (1.0,) * 6)
    # the structs' field order is the header's
    assert [f for f, _ in _lib.CurveLimitsStruct._fields_] == ["lateral_acc_max", "angular_acc_max"]
    assert [f for f, _ in _lib.DriveLimitsStruct._fields_] == ["track_width", "wheel_speed_max", "wheel_acc_max", "jerk_max",
                                                              "lateral_acc_max", "angular_acc_max"]
    s = drive.Limits(1.0, 2.0, 3.0, 4.0, 5.0, 6.0).as_struct()
    assert (C.sizeof(s), s.track_width, s.angular_acc_max) == (48, 1.0, 6.0) and C.sizeof(drive.CurveCaps(1.0, 2.0).as_struct()) == 16
    header = open(_lib.HERE + "/../include/vap.h").read()
    assert "double track_width, wheel_speed_max, wheel_acc_max, jerk_max, lateral_acc_max, angular_acc_max;" in header
    L = _lib.lib()
    for name in ("vap_curve_caps", "vap_drive_audit"):
        assert name in _lib.EXPORTS and hasattr(L, name)


def test_entry_points_check_their_arguments_before_the_device():
    """The calls' own VAP_ERR_INVALID cases with a null context; a call whose arguments are all good fails at the context."""
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    L = _lib.lib()
    INV = _lib.VAP_ERR_INVALID
    one = C.c_void_p(16)
    cons = _lib.make_constraints(DEFAULT_CONSTRAINTS)

    def caps(B=4, S=16, c=cons, lim=(3.0, math.inf), meta=one, out=one):
        ls = _lib.CurveLimitsStruct(*lim) if lim is not None else None
        st = L.vap_curve_caps(None, _lib.VAP_F64, B, S, C.byref(c) if c is not None else None, C.byref(ls) if ls is not None else None,
                              meta, one, None, out, None)
        return st, L.vap_last_error().decode()

    assert caps() == (INV, "null context") and caps(B=0) == (INV, "null context")
    for lim in ((math.nan, 1.0), (0.0, 1.0), (-1.0, 1.0), (1.0, math.nan), (1.0, 0.0), (math.inf, -math.inf)):
        st, msg = caps(lim=lim)
        assert st == INV and "positive" in msg, (lim, msg)
    assert caps(lim=(math.inf, math.inf))[1] == "null context"
    for field in ("max_vel", "track_width"):
        for bad in (math.nan, math.inf):
            c = _lib.make_constraints(DEFAULT_CONSTRAINTS)
            setattr(c, field, bad)
            st, msg = caps(c=c)
            assert st == INV and "finite" in msg, (field, bad, msg)
    for kw in (dict(meta=None), dict(lim=None), dict(out=None), dict(c=None)):
        st, msg = caps(**kw)
        assert st == INV and "null" in msg and msg != "null context", (kw, msg)
    assert caps(B=-1)[0] == INV and "batch" in caps(B=-1)[1]

    def audit(B=2, cap=8, rows=one, counts=one, stride=2, h=0.01, lim=(1.0, 1.0, 1.0, 1.0, 1.0, math.inf), wheel=None):
        ls = _lib.DriveLimitsStruct(*lim) if lim is not None else None
        st = L.vap_drive_audit(None, B, cap, rows, counts, stride, h, C.byref(ls) if ls is not None else None, None, None, None, None,
                               None, wheel)
        return st, L.vap_last_error().decode()

    assert audit() == (INV, "null context") and audit(B=0, rows=None, counts=None) == (INV, "null context")
    for h in (0.0, -0.01, math.nan, math.inf):
        st, msg = audit(h=h)
        assert st == INV and "time_step" in msg, (h, msg)
    for tw in (0.0, -1.0, math.nan, math.inf):
        st, msg = audit(lim=(tw, 1.0, 1.0, 1.0, 1.0, 1.0))
        assert st == INV and "track_width" in msg, (tw, msg)
    for q in range(1, 6):
        for bad in (math.nan, -1.0):
            lim = [1.0] * 6
            lim[q] = bad
            st, msg = audit(lim=tuple(lim))
            assert st == INV and "limit" in msg, (q, bad, msg)
    assert audit(lim=(1.0, 0.0, 0.0, 0.0, 0.0, 0.0))[1] == "null context"
    for kw in (dict(rows=None), dict(counts=None), dict(lim=None)):
        st, msg = audit(**kw)
        assert st == INV and "null rows" in msg, (kw, msg)
    for kw in (dict(rows=C.c_void_p(24)), dict(wheel=C.c_void_p(40))):
        st, msg = audit(**kw)
        assert st == INV and "aligned" in msg, (kw, msg)
    assert audit(B=-1)[0] == INV and audit(cap=-1)[0] == INV and audit(stride=0)[0] == INV
