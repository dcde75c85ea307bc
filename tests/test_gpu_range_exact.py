"""GPU: the ray cast of vap_range_readings and vap_odometry_rollouts ON its decisions.  The inputs of tests/range_exact_cases.py
(heading 0, cardinal beams, dyadic coordinates: every product and sum of the header's formulas is exact) against the NumPy
reference with nothing excused: status, face and element equal, range and cos_incidence the same bits, every route's summaries
equal (test_gpu_range.compare_exact).  test_range_exact_cpu.py holds that reference to the header in exact rational
arithmetic on the same inputs, and shows that each family notices its rule switched."""
import functools
import math

import numpy as np
import pytest

import range_cases as rc
import range_exact_cases as xc
import range_ref as rr
import test_gpu_range as tgr
import tracking_ref as tr
import odometry_ref as orf

pytestmark = pytest.mark.gpu
ALL = tgr.SUMMARY_KEYS + tgr.ROW_KEYS


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def reference(fam, name):
    return rc.reference(rr, xc.family(fam)[name])


def readings_of(res):
    """A call's per-reading outputs in the reference's layout."""
    st, fa, el = tgr.sn().unpack(res["code"].cpu().numpy())
    return {"status": st, "face": fa, "element": el, "t": res["range"].cpu().numpy(), "cos": res["cos_incidence"].cpu().numpy()}


# ---- 1. the families --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["lattice", "ties", "vertices", "origins", "tangent", "thresholds"])
def test_family_bit_for_bit(torch_mod, fam):
    n = 0
    for name, case in xc.family(fam).items():
        ref = reference(fam, name)
        res = tgr.run(case)
        tgr.compare_exact(res, ref, name)
        # culling off, summaries only, host input, a second call: the same bits
        assert tgr.same_bits(res, tgr.run(case, cull=False), ALL), name
        assert tgr.same_bits(res, tgr.run(case, per_row=False), tgr.SUMMARY_KEYS), name
        tgr.compare_exact(tgr.run(case, per_row=False, cull=False, stride=3), ref, name + " summaries")
        assert tgr.same_bits(res, tgr.run(case, device_input=False), ALL), name
        assert tgr.same_bits(res, tgr.run(case), ALL), name
        n += int(ref["live"].sum()) * ref["status"].shape[2]
    print(f"RANGE EXACT {fam}: {n} readings bit for bit, nothing excused")


def test_wide_four_step_tile_and_both_scene_paths(torch_mod):
    """1024 routes of capacity 300 take the four-step tile with obstacles present; the padded copy reads the scene from global
    memory.  Both equal the reference, and each other: range and cosine bit for bit, status and face equal, and the elements
    once the circles' indices are moved back over the padding."""
    plain, padded = xc.family("wide")["wide"], xc.family("wide")["wide padded"]
    assert xc.packed_doubles(plain["scene"]) <= tgr.lds_budget() < xc.packed_doubles(padded["scene"])
    B, cap = plain["rows"].shape[:2]
    assert B * ((cap + 1023) // 1024) >= 1024
    a, b = tgr.run(plain), tgr.run(padded)
    tgr.compare_exact(a, reference("wide", "wide"), "wide")
    tgr.compare_exact(b, reference("wide", "wide padded"), "wide padded")
    ra, rb = readings_of(a), readings_of(b)
    rb["element"] = np.where(rb["element"] >= len(padded["scene"]["polygons"]), rb["element"] - xc.PAD_POLYGONS, rb["element"])
    assert xc.same_readings(ra, rb) is None, xc.same_readings(ra, rb)
    assert tgr.same_bits(a, b, tgr.SUMMARY_KEYS)
    for case, res in ((plain, a), (padded, b)):
        assert tgr.same_bits(res, tgr.run(case, cull=False), ALL)
        assert tgr.same_bits(res, tgr.run(case, per_row=False), tgr.SUMMARY_KEYS)


def test_moved_translation_and_scaling_are_identities(torch_mod):
    """Every moved case against the reference, and against the device's own readings of its base: a translation by 2^10, 2^17
    or 2^23 ft reproduces range, cosine and code bit for bit, a scaling by 2^-10 or 2^10 the codes and cosines and the ranges
    times the power of two (range_exact_cases.check_moved; a circle's cosine is taken at a hit point in the frame's own
    coordinates and moves with the frame where that point rounds)."""
    bases = xc.moved_bases()
    base_res = {name: readings_of(tgr.run(xc.family("moved")[f"moved {name} base"])) for name in bases}
    for name in bases:
        tgr.compare_exact(tgr.run(xc.family("moved")[f"moved {name} base"]), reference("moved", f"moved {name} base"), name)
    n_loose = 0
    for name, kind, amount, _ in xc.moved_variants():
        key = f"moved {name} {kind} {amount:g}"
        case = xc.family("moved")[key]
        res = tgr.run(case)
        tgr.compare_exact(res, reference("moved", key), key)
        n_loose += xc.check_moved(bases[name], base_res[name], kind, amount, readings_of(res), key)
        assert tgr.same_bits(res, tgr.run(case, cull=False), ALL), key
    print(f"RANGE EXACT moved: {n_loose} circle cosines taken at a rounded hit point")


# ---- 2. a partner with a NaN pose ---------------------------------------------------------------------------------------------
def test_nan_partner_takes_part_in_nothing(torch_mod):
    """'NaN candidates take part in nothing': on the rows where partner 0's pose is not finite the readings are those of the call
    without that partner (its count 0: absent, the other partner keeps its element), on every other row those of the call with
    it."""
    case = xc.family("ties")["ties partner"]
    with_it = tgr.run(case)
    without = dict(case, others_counts=np.array([0, case["others_counts"][1]], dtype=np.int32))
    without_it = tgr.run(without)
    tgr.compare_exact(without_it, rc.reference(rr, without), "without the partner")
    bad = dict(case, others=case["others"].copy())
    nan_rows = {1: (6, math.nan), 5: (7, math.nan), 6: (4, math.nan), 9: (6, math.inf), 10: (4, -math.inf)}
    for r, (col, v) in nan_rows.items():
        bad["others"][0, r, col] = v
    for cull in (True, False):
        got = tgr.bits(tgr.run(bad, cull=cull), tgr.ROW_KEYS)
        a, b = tgr.bits(with_it, tgr.ROW_KEYS), tgr.bits(without_it, tgr.ROW_KEYS)
        for k in tgr.ROW_KEYS:
            for r in range(case["rows"].shape[1]):
                want = b if r in nan_rows else a
                assert np.array_equal(got[k][:, r], want[k][:, r]), (k, r, cull)
    # the partner did change those rows while its pose was finite
    assert any(not np.array_equal(tgr.bits(with_it, ("code",))["code"][:, r], tgr.bits(without_it, ("code",))["code"][:, r]) for r in nan_rows)


# ---- 3. odometry: the same cast with rollout lanes in place of row lanes --------------------------------------------------------
ODO_ROWS, ODO_SETTLE, ODO_K = 5, 2, 3


def odometry_case(which):
    """Stationary routes (v = omega = 0 on every row) at lattice points of a scene: with the ideal odometry record and no
    perturbation the executed pose stays the lattice point exactly, so every executed row repeats the route's one reading."""
    if which == "ties":
        base = xc.ties_scene_case()
        pts = np.concatenate([base["rows"][b, :n, 6:8] for b, n in enumerate(base["counts"])])
        scene, sensors = base["scene"], xc.cardinal_sensors(r_min=0.5, r_max=5.0, min_cos=0.5)      # 0.5: some readings sit on r_min
    else:
        pts = xc.lattice_poses(np.random.default_rng(106), 80)
        scene, sensors = xc.lattice_scene(), xc.LATTICE_SENSORS
    rows = np.zeros((len(pts), ODO_ROWS, 8))
    rows[:, :, 0] = np.arange(ODO_ROWS) * 0.01
    rows[:, :, 6:8] = pts[:, None, :]
    return dict(rows=rows, counts=np.full(len(pts), ODO_ROWS, dtype=np.int32), scene=scene, sensors=sensors, pts=pts)


@pytest.mark.parametrize("which", ["ties", "lattice"])
def test_odometry_resets_are_the_valid_readings_nothing_excused(torch_mod, which):
    from vexautonomousplanner_amd import footprint, odometry, sensors, tracking
    case = odometry_case(which)
    B, K, total = len(case["pts"]), ODO_K, ODO_ROWS + ODO_SETTLE
    P = np.broadcast_to(tr.NOMINAL, (B, K, 8)).copy()
    O = np.broadcast_to(orf.IDEAL, (B, K, 8)).copy()
    sc = case["scene"]
    scene = footprint.Scene(field=sc["field"], polygons=sc["polygons"], circles=sc["circles"])
    res = odometry.rollouts(case["rows"], case["counts"], tracking.Follower(**tr.follower(settle_rows=ODO_SETTLE)), P, O,
                            sensors=case["sensors"], scene=scene, rule=odometry.ResetRule(6.0, 60.0, 0.0, 1), time_step=0.01,
                            executed=True, estimates=True)
    torch_mod.cuda.synchronize()
    ex_rows, ex_counts = res["rows"].cpu().numpy(), res["counts"].cpu().numpy()
    assert (ex_counts[:, 0] == total).all()
    # the executed pose is the lattice point, exactly, on every row of every rollout
    pts = np.repeat(case["pts"], K, axis=0)
    assert (ex_rows[:, :total, 6:8] == pts[:, None, :]).all() and (ex_rows[:, :total, 4] == 0.0).all()
    # the valid readings of those rows: from the reference with nothing excused, and from vap_range_readings on the executed rows
    ref_rows = np.zeros((B * K, total, 8))
    ref_rows[:, :, 6:8] = pts[:, None, :]
    ref = rr.readings(ref_rows, np.full(B * K, total), case["sensors"], sc["field"], sc["polygons"], sc["circles"])
    want = (ref["status"] == rr.VALID).sum(axis=(1, 2))
    rd = sensors.readings(res["rows"], res["counts"], case["sensors"], scene, per_row=True)
    torch_mod.cuda.synchronize()
    st, _, _ = sensors.unpack(rd["code"].cpu().numpy())
    assert np.array_equal((st == 0).sum(axis=(1, 2)), want)
    assert int((ref["margin"][ref["live"]] == 0.0).sum()) > 0 and 0 < want.sum() < B * K * total * len(case["sensors"])
    stat_rows = res["stat_rows"].cpu().numpy()
    tried = (stat_rows[..., 2] + stat_rows[..., 3]).reshape(-1)
    assert np.array_equal(tried, want), (which, np.argwhere(tried != want)[:5], tried[tried != want][:5], want[tried != want][:5])
    # the three rollouts of a route are equal
    stats = res["stats"].cpu().numpy().view(np.int64)
    assert (stats == stats[:, :1]).all() and (stat_rows == stat_rows[:, :1]).all()
    er = ex_rows.reshape(B, K, *ex_rows.shape[1:])[:, :, :total].view(np.int64)
    assert (er == er[:, :1]).all()
