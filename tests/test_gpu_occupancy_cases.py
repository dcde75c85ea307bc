"""GPU: vap_plan_occupancy and the window mask of vap_plan_seeds_occupied / vap_plan_travel ON their decisions.  The inputs of
tests/occupancy_cases.py (heading 0, dyadic coordinates, clearances exactly on the margin) against the NumPy reference of
tests/occupancy_ref.py with nothing excused: first, last, count and blocked equal, min_clearance the same bits (but for the sign
of a clearance that is zero, which nothing defines: occupancy_cases.same), with and without the minimum, with culling on and
off.  test_occupancy_cases_cpu.py shows on the reference alone that each family holds
what it is named for and that nothing before the final sqrt and subtraction depends on the precision, which licenses the bits.

Measured on the MI355X (the figures are in DESIGN.md section 16): every comparison below exact; the collapsed poses covered the
whole grid with min_clearance -inf before the rule "a collapsed pose takes part in nothing" went into the kernel."""
import numpy as np
import pytest

import occupancy_cases as xc
import occupancy_ref as oc
import order_ref as orf
import test_gpu_plan as tgp
import test_gpu_routine as tgr

pytestmark = pytest.mark.gpu
P, host = tgp.P, tgp.host
LEAN = xc.KEYS + ("blocked",)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def field_scene(field):
    from vexautonomousplanner_amd import footprint as fp
    return fp.Scene(field=field)


def device(case, rows=None, min_clearance=True, cull=True, raw=False):
    out = P().occupancy(case["rows"] if rows is None else rows, case["counts"], case["foot"], field_scene(case["field"]), case["cell"],
                        case["radius"], margin=case["margin"], shift_rows=case["shift_rows"], hold_first=case["hold_first"],
                        hold_last=case["hold_last"], min_clearance=min_clearance, cull=cull)
    return out if raw else {k: host(v) for k, v in out.items()}


def hold(name, got, ref):
    """A device dict to the reference: the integers equal, the minimum the same bits."""
    keys = xc.ALL_KEYS if "min_clearance" in got else LEAN
    for k in xc.KEYS:
        assert got[k].dtype == np.int32, (name, k)
    bad = xc.same(got, ref, keys, zero_sign=False)                   # a zero's sign: occupancy_cases.same
    if bad is not None:
        where = np.argwhere(np.asarray(got[bad]) != np.asarray(ref[bad]))
        j, i = where[0] if len(where) else (0, 0)
        raise AssertionError((name, bad, len(where), (int(j), int(i)), got[bad][j, i], ref[bad][j, i]))


def every_way(name, case, ref, rows=None):
    """With and without the minimum, with culling on and off: the reference, four times."""
    for min_clearance in (True, False):
        for cull in (True, False):
            hold(f"{name} (minimum {min_clearance}, cull {cull})", device(case, rows, min_clearance, cull), ref)


# ---- 1. ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(xc.FEET) + ["on the edge", "deep inside"])
def test_ties_decide_as_the_reference(torch_mod, which):
    n = 0
    for name, case in xc.family("ties").items():
        if f" {which}" not in name:
            continue
        ref = xc.cached_reference("ties", name)
        every_way(name, case, ref)
        n += 1
    assert n >= 2
    print(f"OCCUPANCY CASES ties {which}: {n} cases, four ways each, bit for bit")


# ---- 2. chunks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold_", xc.HOLDS, ids=lambda h: f"{int(h[0])}{int(h[1])}")
def test_chunk_boundaries_counts_and_holds(torch_mod, hold_):
    tag = f"hold {int(hold_[0])}{int(hold_[1])}"
    cases = xc.family("chunks")
    singles = []
    for n in xc.CHUNK_COUNTS:
        name = f"chunks n={n} {tag}"
        got = device(cases[name])
        hold(name, got, xc.cached_reference("chunks", name))
        hold(name + " lean, no cull", device(cases[name], min_clearance=False, cull=False), xc.cached_reference("chunks", name))
        singles.append(got)
    name = f"chunks all {tag}"
    every_way(name, cases[name], xc.cached_reference("chunks", name))
    assert xc.same(device(cases[name]), xc.merged(singles)) is None


# ---- 3. instants --------------------------------------------------------------------------------------------------------------
def test_instants_beside_the_hold_values(torch_mod):
    from vexautonomousplanner_amd import _lib
    for name, case in xc.family("instants").items():
        every_way(name, case, xc.cached_reference("instants", name))
    base = xc.family("instants")["instants low hold 11"]
    for shift in xc.SHIFT_REFUSED:
        with pytest.raises(_lib.VapError) as e:
            device(dict(base, shift_rows=shift))
        assert e.value.status == _lib.VAP_ERR_UNSUPPORTED, shift


# ---- 4. non-finite and collapsed poses --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", list(xc.BAD_VALUES))
def test_non_finite_poses_take_part_in_nothing(torch_mod, value):
    n = 0
    for name, case in xc.family("nonfinite").items():
        if name != "bad base" and f" {value} " not in name:
            continue
        every_way(name, case, xc.cached_reference("nonfinite", name))
        n += 1
    assert n == 13


def test_collapsed_poses_take_part_in_nothing(torch_mod):
    for name, case in xc.family("collapsed").items():
        ref = xc.cached_reference("collapsed", name)
        every_way(name, case, ref)
        on, off = device(case), device(case, cull=False)
        for k in xc.ALL_KEYS:
            assert np.array_equal(on[k].view(np.uint8), off[k].view(np.uint8)), (name, k)
        assert np.isfinite(on["min_clearance"]).all() and not on["blocked"].all(), name


# ---- 5. far -------------------------------------------------------------------------------------------------------------------
def test_far_from_the_origin_the_same_arrays(torch_mod):
    base = {name: device(xc.far_base(name)) for name in ("at", "above")}
    for name, case in xc.family("far").items():
        every_way(name, case, xc.cached_reference("far", name))
        assert xc.same(device(case), base[name.split()[-1]]) is None, name


# ---- 6. many ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["many ones", "many pairs"])
def test_more_work_items_than_workgroups(torch_mod, which):
    torch = torch_mod
    case = xc.family("many")[which]
    rows = torch.as_tensor(case["distinct"], device="cuda")[torch.as_tensor(case["index"], device="cuda")].contiguous()
    assert rows.shape[0] * ((rows.shape[1] + 63) // 64) > xc.MAX_BLOCKS
    want = xc.many_expected(case)
    every_way(which, case, want, rows=rows)


# ---- 7. minimum ---------------------------------------------------------------------------------------------------------------
def test_minimum_over_forty_chunks(torch_mod):
    case = xc.family("minimum")["minimum"]
    ref = xc.cached_reference("minimum", "minimum")
    every_way("minimum", case, ref)
    a, b, off = device(case), device(case), device(case, cull=False)
    for k in xc.ALL_KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), off[k].view(np.uint8)), k


# ---- 8. windows ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window_occupancies(torch_mod):
    w = xc.windows()
    out = {}
    for which in ("plain", "held"):
        occ = device(w[which], min_clearance=False, raw=True)
        hold("windows " + which, {k: host(v) for k, v in occ.items()}, xc.reference(w[which]))
        out[which] = occ
    return w, out


def test_windows_on_a_cells_first_and_last_instant(torch_mod, window_occupancies):
    w, occ = window_occupancies
    sc, W = xc.WINDOW_SCENE, xc.WINDOW_W
    free = xc.static_free()
    for which in ("plain", "held"):
        probs = [p for p in w["problems"] if p["occ"] == which]
        starts, goals = np.array([p["start"] for p in probs]), np.array([p["goal"] for p in probs])
        windows = [p["window"] for p in probs]
        ref_occ = xc.reference(w[which])
        ref, _ = oc.seeds(starts, goals, windows, sc["field"], sc["cell"], free, ref_occ["first"], ref_occ["last"], W=W)
        out = P().seeds(starts, goals, tgp.scene_of(sc), W, sc["radius"], cell=sc["cell"], margin=sc["margin"], vertices=True,
                        distance=True, occupancy=occ[which], windows=np.array(windows, dtype=np.int64))
        out = {k: host(v) for k, v in out.items()}
        for r, p in enumerate(probs):
            tgp.check_problem(f"window {p['name']} {p['window']}", out, r, ref[r], starts[r], goals[r], W)
    print(f"OCCUPANCY CASES windows: {len(w['problems'])} problems bit for bit in flags, vertices and distance field")


def test_edge_windows_through_travel(torch_mod, window_occupancies):
    w, occ = window_occupancies
    sc, W = xc.WINDOW_SCENE, xc.WINDOW_W
    free = xc.static_free()
    ref_occ = xc.reference(w["plain"])
    points = np.array([t["points"] for t in w["travel"]])
    windows = np.array([t["window"] for t in w["travel"]], dtype=np.int64)
    tr = tgr.device_travel(sc, points, W, occupancy=occ["plain"], windows=windows)
    tgr.check_against_seeds("edge windows", sc, points, tr, W, occupancy=occ["plain"], windows=windows)
    for r, t in enumerate(w["travel"]):
        mask = oc.window_free(free, ref_occ["first"], ref_occ["last"], t["window"])
        tgr.check_against_reference(f"travel {t['window']}", tr, r, orf.travel(points[r], sc["field"], sc["cell"], mask, W))
