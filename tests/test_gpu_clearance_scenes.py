"""GPU: the two exact clearance geometries on the deterministic families of tests/scene_cases.py — the footprint against a
static scene (footprint.clearance; vap_footprint.h) and two moving footprints (footprint.conflicts, footprint.shifts;
vap_conflict.h), and row_clearance_capped through the rollout kernels — against the NumPy references, with what
tests/test_scene_cases_cpu.py proves of the families on the references alone.

Values: within tol(X) = max(1e-12, 16 eps X) of the float64 reference, X the largest coordinate in the case; `cull=False`
gives the same bits in every output.  Indices: exact in the exact, tie, plateau, twin and NaN families; in the random-pose
families under the neighbours' AMBIGUOUS rule (threshold sc.ambiguous(X), gaps over distinct values: equal bits tie by construction,
footprint_ref.summarise), at most 5 % skipped per kind over the families of one test.

Measured on the MI355X, largest |device - reference| (ft) and, from the CPU test, the largest D = |float64 - long double|
of the reference:

  family                          X        |device - reference|   D         tol(X)
  exact, ties, pair_exact,
    pair_plateau                  <= 192   0 (every row exact)    <= 1e-16  1e-12
  containment                     61       6.2e-15                3.5e-15   1e-12
  shapes (16, triangle, sliver,
    pentagon)                     <= 10    1.3e-15                1.1e-15   1e-12
  shapes (1e3 ft square)          1002     4.4e-16                3.4e-16   3.6e-12
  full                            65       1.4e-14                7.1e-15   1e-12
  nan_rows (static, pairs)        6        8.9e-16                6.5e-16   1e-12
  far(2^10)                       1e3      4.6e-13                3.8e-13   3.6e-12
  far(2^17)                       1.3e5    5.8e-11                4.1e-11   4.7e-10
  far(2^23)                       8.4e6    3.7e-09                2.8e-09   3.0e-08
  pair_shapes, pair_others        <= 20    3.6e-15                6.1e-15   1e-12
  pair_far(2^10)                  1e3      1.6e-13                4.6e-15   3.6e-12
  pair_far(2^17)                  1.3e5    2.3e-11                4.6e-15   4.7e-10
  pair_far(2^23)                  8.4e6    1.6e-09                4.6e-15   3.0e-08
The device at X against the device at 0 (far): at most 2.5e-09 ft at X = 2^23.  The pair kernel's error at large X is the
rounding of the posed bounding-circle centre where the footprint's centre is off its origin (the triangle); everything after
that is relative.  The static kernel projects world coordinates and holds tol(X) with a factor of 8 to spare at 2^23.
Skipped as ambiguous: 1 of 49 rows (containment's robot inside the 16-gon, whose plateau comes from the robot's own posed
vertices and differs by rounding from row to row), 2 of 88 per far(X); none of the pair indices.
"""
import numpy as np
import pytest

import scene_cases as sc
import test_gpu_conflict as tgc
import test_gpu_footprint as tgf
import test_gpu_rollout_clearance as trc
import rollout_clearance_ref as rc

pytestmark = pytest.mark.gpu

AMBIGUOUS = tgf.AMBIGUOUS
STATIC_KEYS = tgf.KEYS
Tally = tgc.Tally


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def fpm():
    from vexautonomousplanner_amd import footprint
    return footprint


def scene_of(case):
    return fpm().Scene(field=case["field"], polygons=case["polygons"], circles=case["circles"])


# ---- static -----------------------------------------------------------------------------------------------------------
def run_static(torch, case, cull=True):
    rows, counts = tgc.side(torch, case["rows"], case["counts"], 2)
    res = fpm().clearance(rows, counts, case["foot"], scene_of(case), margin=case["margin"], per_row=True, cull=cull)
    torch.cuda.synchronize()
    return res


def check_static(res, case, tally=None):
    """Every output against sc.static_reference within tol(X); indices exactly (tally None) or under the AMBIGUOUS rule.
    Returns the largest clearance difference seen."""
    tol, amb = sc.tol(case["X"]), sc.ambiguous(case["X"])
    got = {k: res[k].cpu().numpy() for k in STATIC_KEYS}
    rcl = res["row_clearance"].cpu().numpy()
    worst = 0.0
    for b, s in enumerate(sc.static_reference(case)):
        n = s["n"]
        assert np.isnan(rcl[b, n:]).all(), b
        if n:
            assert np.array_equal(np.isnan(rcl[b, :n]), np.isnan(s["rows"])), (b, "NaN rows")
            d = float(np.nanmax(np.abs(rcl[b, :n] - s["rows"]), initial=0.0))
            worst = max(worst, d)
            assert d <= tol, (case["name"], b, d, tol)
        g = tuple(got[k][b] for k in STATIC_KEYS)
        if s["min_row"] < 0:
            assert np.isnan(g[0]) and g[1:] == (-1, -1, -1, 0), (b, g)
            continue
        worst = max(worst, abs(g[0] - s["min_clearance"]))
        assert abs(g[0] - s["min_clearance"]) <= tol, (case["name"], b, g[0], s["min_clearance"])
        r = int(g[1])
        assert 0 <= r < n and abs(s["rows"][r] - s["min_clearance"]) <= amb, (b, g)
        assert g[0] == rcl[b, r], (b, "the minimum is the per-row value at min_row")
        want = (s["min_row"], s["min_element"], s["first_row"], s["n_below"])
        if tally is None:
            assert g[1:] == want, (case["name"], b, g, want)
            continue
        if tally.case("row", s["row_gap_distinct"] > amb):
            assert r == s["min_row"], (case["name"], b, g, want)
        if tally.case("other", s["elem_gap"][r] > amb):
            assert g[2] == s["elems"][r], (case["name"], b, g, s["elems"][r])
        if tally.case("margin", s["margin_gap"] > amb):
            assert g[3:] == want[2:], (case["name"], b, g, want)
    if tally is not None:
        tally.worst = max(tally.worst, worst)
    return worst


def static_both(torch, case, tally=None):
    """The case with culling on, checked, and the same bits with culling off."""
    res = run_static(torch, case)
    worst = check_static(res, case, tally)
    a, b = tgf.bits(res), tgf.bits(run_static(torch, case, cull=False))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{case['name']}: {k}, cull off")
    print(f"{case['name']}: X = {case['X']:.4g}, max |device - reference| {worst:.2e} ft (tol {sc.tol(case['X']):.1e})")
    return res


def test_exact(torch_mod):
    case = sc.exact()
    res = static_both(torch_mod, case)
    v = res["row_clearance"][0].cpu().numpy()
    want = np.array([c for c, _ in case["expect"]])
    assert np.abs(v - want).max() <= 1e-15, v - want
    assert not np.signbit(v[want == 0.0]).any()                      # touching is not contact: +0.0, the distance branch
    # one row at a time: each row's element
    rows = np.ascontiguousarray(np.swapaxes(case["rows"], 0, 1))
    one = fpm().clearance(rows, np.ones(len(rows), dtype=np.int32), case["foot"], scene_of(case), margin=case["margin"])
    torch_mod.cuda.synchronize()
    assert one["min_element"].tolist() == [e for _, e in case["expect"]]
    assert np.abs(one["min_clearance"].cpu().numpy() - want).max() <= 1e-15


@pytest.mark.parametrize("variant", range(4))
def test_ties(torch_mod, variant):
    case = sc.ties()[variant]
    res = static_both(torch_mod, case)
    e = case["expect"]
    r0 = list(sc.TIE_R0)
    assert res["min_row"].tolist() == r0 and res["first_row"].tolist() == r0
    assert res["n_below"].tolist() == [sc.TIE_ROWS - r for r in r0]
    assert res["min_element"].tolist() == [e["element"]] * len(r0)
    assert res["min_clearance"].tolist() == [e["plateau"]] * len(r0)


def test_containment_shapes_and_full(torch_mod):
    tally = Tally()
    for case in [sc.containment()] + sc.shapes() + [sc.full()]:
        static_both(torch_mod, case, tally)
    res = run_static(torch_mod, sc.full())
    assert tuple(res["min_element"][2:].tolist()) == sc.full()["expect"] == (255, 511, -1)
    tally.close("containment, shapes, full")


@pytest.mark.parametrize("X", sc.FAR)
def test_far(torch_mod, X):
    tally = Tally()
    for there, here in sc.far(X):
        a, b = static_both(torch_mod, there, tally), static_both(torch_mod, here, tally)
        va, vb = a["row_clearance"].cpu().numpy(), b["row_clearance"].cpu().numpy()
        d = float(np.nanmax(np.abs(va - vb)))
        print(f"{there['name']}: max |device at X - device at 0| {d:.2e} ft")
        assert d <= sc.tol(there["X"]) + sc.tol(here["X"]), (there["name"], d)
    tally.close(f"far, X = {X:g}")


# ---- pairs ------------------------------------------------------------------------------------------------------------
def run_pairs(torch, case, shift=0, matched=False, cull=True, margin=None):
    n = min(len(case["rows_a"]), len(case["rows_o"])) if matched else None
    a, ca = tgc.side(torch, case["rows_a"][:n], case["counts_a"][:n], 2)
    o, co = tgc.side(torch, case["rows_o"][:n], case["counts_o"][:n], 3)
    res = fpm().conflicts(a, ca, case["foot_a"], o, co, case["foot_o"], margin=case["margin"] if margin is None else margin, shift_rows=shift,
                          pairing="matched" if matched else "all", pairs=True, cull=cull)
    torch.cuda.synchronize()
    return res


def check_pairs(res, ref, tol, tally=None, matched=False, name="", amb=AMBIGUOUS):
    """tgc.check with a tolerance (and an ambiguity threshold) of its own; tally None: every index exactly."""
    got = {k: res[k].cpu().numpy() for k in tgc.ROUTE_KEYS + tgc.PAIR_KEYS}
    Ba, P = ref["pair_clearance"].shape
    assert got["pair_clearance"].shape == (Ba, P)
    worst = 0.0
    for ia in range(Ba):
        for p in range(P):
            want = ref["pair_clearance"][ia, p]
            g = (got["pair_clearance"][ia, p], got["pair_row"][ia, p], got["pair_first_row"][ia, p])
            if np.isnan(want):
                assert np.isnan(g[0]) and g[1:] == (-1, -1), (name, ia, p, g)
                continue
            worst = max(worst, abs(g[0] - want))
            assert abs(g[0] - want) <= tol, (name, ia, p, g[0], want)
            rows = ref["pair_rows"][(ia, p)]
            assert 0 <= g[1] < len(rows) and abs(rows[g[1]] - want) <= amb, (name, ia, p, g)
            if tally is None:
                assert g[1:] == (ref["pair_row"][ia, p], ref["pair_first_row"][ia, p]), (name, ia, p, g, ref["pair_row"][ia, p], ref["pair_first_row"][ia, p])
                continue
            if tally.case("row", ref["pair_row_gap_distinct"][ia, p] > amb):
                assert g[1] == ref["pair_row"][ia, p], (name, ia, p, g, ref["pair_row"][ia, p])
            if tally.case("margin", ref["pair_margin_gap"][ia, p] > amb):
                assert g[2] == ref["pair_first_row"][ia, p], (name, ia, p, g, ref["pair_first_row"][ia, p])
    for ia in range(Ba):
        g = tuple(got[k][ia] for k in tgc.ROUTE_KEYS)
        if ref["min_other"][ia] < 0:
            assert np.isnan(g[0]) and g[1:] == (-1, -1, 0, -1), (name, ia, g)
            continue
        want = ref["min_clearance"][ia]
        worst = max(worst, abs(g[0] - want))
        assert abs(g[0] - want) <= tol, (name, ia, g[0], want)
        p = 0 if matched else g[1]
        assert (g[1] == ia if matched else 0 <= g[1] < P) and abs(ref["pair_clearance"][ia, p] - want) <= amb, (name, ia, g)
        assert g[2] == got["pair_row"][ia, p] and g[0] == got["pair_clearance"][ia, p], (name, ia, g)
        full = (ref["min_other"][ia], ref["min_row"][ia], ref["n_conflicts"][ia], ref["first_row"][ia])
        if tally is None:
            assert g[1:] == full, (name, ia, g, full)
            continue
        if tally.case("other", ref["other_gap_distinct"][ia] > amb):
            assert g[1] == full[0], (name, ia, g, full)
            if tally.case("row", ref["pair_row_gap_distinct"][ia, p] > amb):
                assert g[2] == full[1], (name, ia, g, full)
        if tally.case("margin", ref["margin_gap"][ia] > amb):
            assert g[3:] == full[2:], (name, ia, g, full)
    if tally is not None:
        tally.worst = max(tally.worst, worst)
    return worst


def shifts_match(torch, case, results):
    """footprint.shifts with hold = 14 at sc.SHIFTS returns conflicts' pair_clearance, the same number."""
    a, ca = tgc.side(torch, case["rows_a"], case["counts_a"], 2)
    o, co = tgc.side(torch, case["rows_o"], case["counts_o"], 3)
    lo, step = min(sc.SHIFTS), max(sc.SHIFTS)                           # -5, 0, 5
    for cull in (True, False):
        t = fpm().shifts(a, ca, case["foot_a"], o, co, case["foot_o"], margin=case["margin"], shift_lo=lo, n_shifts=3, shift_step=step, hold=14,
                         pairs=True, cull=cull)["pair_table"]
        torch.cuda.synchronize()
        t = t.cpu().numpy()
        for k, shift in enumerate((lo, lo + step, lo + 2 * step)):
            pc = results[shift]["pair_clearance"].cpu().numpy()
            assert np.array_equal(np.isnan(t[:, :, k]), np.isnan(pc)), (case["name"], shift)
            np.testing.assert_array_equal(np.nan_to_num(t[:, :, k]).view(np.int64), np.nan_to_num(pc).view(np.int64),
                                          err_msg=f"{case['name']}: shift {shift}, cull {cull}")


def pairs_every_way(torch, case, tally=None, pairings=(False, True)):
    """Shifts 0, 5, -5, both pairings, culling on and off with the same bits; then the shift table.  Returns the largest
    difference from the reference."""
    worst = 0.0
    tol = sc.tol(case["X"])
    all_pairs = {}
    for shift in sc.SHIFTS:
        for matched in pairings:
            res = run_pairs(torch, case, shift, matched)
            worst = max(worst, check_pairs(res, sc.pair_reference(case, shift, matched), tol, tally, matched, f"{case['name']} shift {shift}",
                                           sc.ambiguous(case["X"])))
            tgc.same_bits(res, run_pairs(torch, case, shift, matched, cull=False))
            if not matched:
                all_pairs[shift] = res
    if all_pairs:
        shifts_match(torch, case, all_pairs)
    print(f"{case['name']}: X = {case['X']:.4g}, max |device - reference| {worst:.2e} ft (tol {tol:.1e})")
    return worst


def test_pair_exact(torch_mod):
    torch = torch_mod
    case = sc.pair_exact()
    pairs_every_way(torch, case)
    for shift in sc.SHIFTS:
        for matched in (False, True):
            res = run_pairs(torch, case, shift, matched)
            for ia, (v, row, first) in enumerate(case["expect"]["pair"]):
                assert (res["pair_clearance"][ia] - v).abs().max().item() <= 1e-15
                assert (res["pair_row"][ia] == row).all() and (res["pair_first_row"][ia] == first).all()
                # touching (projections that meet, `!(ov > 0.0)`) is the distance branch: +0.0, not minus an overlap of 0
                assert v != 0.0 or not np.signbit(res["pair_clearance"][ia].cpu().numpy()).any()
    # O is parked: the same polygon as a scene polygon under the static check
    a, ca = tgc.side(torch, case["rows_a"], case["counts_a"], 2)
    s = fpm().clearance(a, ca, case["foot_a"], fpm().Scene(field=None, polygons=[case["foot_o"]]), margin=case["margin"])
    res = run_pairs(torch, case, 0, True)
    torch.cuda.synchronize()
    assert (s["min_clearance"] - res["pair_clearance"][:, 0]).abs().max().item() <= 1e-15
    assert torch.equal(s["min_row"], res["pair_row"][:, 0]) and torch.equal(s["first_row"], res["pair_first_row"][:, 0])


def test_pair_plateau(torch_mod):
    torch = torch_mod
    stand, parallel = sc.pair_plateau()
    pairs_every_way(torch, stand)
    e = stand["expect"]
    for shift in sc.SHIFTS:
        for matched in (False, True):
            for cull in (True, False):
                res = run_pairs(torch, stand, shift, matched, cull)
                for ia in range(len(sc.PLATEAU_R0)):
                    assert (res["pair_clearance"][ia] == e["clearance"]).all()
                    assert (res["pair_row"][ia] == e["row"][ia]).all(), (shift, matched, cull, ia, res["pair_row"][ia].tolist())
                    assert (res["pair_first_row"][ia] == e["first"][ia]).all()
    pairs_every_way(torch, parallel, pairings=(True,))
    for shift in sc.SHIFTS:
        for cull in (True, False):
            at = run_pairs(torch, parallel, shift, True, cull, margin=1.0)                       # the comparison is a strict <
            above = run_pairs(torch, parallel, shift, True, cull, margin=1.0 + 2.0 ** -40)
            for res, first, ncon in ((at, -1, 0), (above, 0, 1)):
                assert res["pair_clearance"][:, 0].tolist() == [1.0, 1.0] and res["pair_row"][:, 0].tolist() == [0, 0]
                assert res["pair_first_row"][:, 0].tolist() == [first] * 2 and res["n_conflicts"].tolist() == [ncon] * 2
                check_pairs(res, sc.pair_reference(parallel, shift, True, margin=1.0 if first < 0 else 1.0 + 2.0 ** -40), 1e-15, None, True)


def test_pair_others(torch_mod):
    case = sc.pair_others()
    pairs_every_way(torch_mod, case, pairings=(False,))
    for shift in sc.SHIFTS:
        res = run_pairs(torch_mod, case, shift)
        assert res["min_other"].tolist() == case["expect"]["min_other"] == [3, 2]
        assert res["n_conflicts"].tolist() == case["expect"]["n_conflicts"]
        pc = res["pair_clearance"]
        assert pc[0, 3].item() == pc[0, 9].item() and pc[1, 2].item() == pc[1, 20].item()


def test_pair_shapes(torch_mod):
    tally = Tally()
    for case in sc.pair_shapes():
        pairs_every_way(torch_mod, case, tally)
    tally.close("pair_shapes")


@pytest.mark.parametrize("X", sc.FAR)
def test_pair_far(torch_mod, X):
    tally = Tally()
    for there, here in sc.pair_far(X):
        pairs_every_way(torch_mod, there, tally)
        pairs_every_way(torch_mod, here, tally)
        a = run_pairs(torch_mod, there)["pair_clearance"].cpu().numpy()
        b = run_pairs(torch_mod, here)["pair_clearance"].cpu().numpy()
        assert np.nanmax(np.abs(a - b)) <= sc.tol(there["X"]) + sc.tol(here["X"]), there["name"]
    tally.close(f"pair_far, X = {X:g}")


# ---- NaN poses --------------------------------------------------------------------------------------------------------
def test_nan_rows(torch_mod):
    static, pair = sc.nan_rows()
    res = static_both(torch_mod, static)                                     # per-row NaN exactly at the NaN rows; no other output sees them
    assert torch_mod.isnan(res["row_clearance"][3]).all() and torch_mod.isnan(res["min_clearance"][3])
    assert [int(res[k][3]) for k in ("min_row", "min_element", "first_row", "n_below")] == [-1, -1, -1, 0]
    pairs_every_way(torch_mod, pair, pairings=(False, True))
    res = run_pairs(torch_mod, pair)
    assert torch_mod.isnan(res["pair_clearance"][3]).all() and (res["pair_row"][3] == -1).all() and (res["pair_first_row"][3] == -1).all()
    assert torch_mod.isnan(res["min_clearance"][3])
    assert [int(res[k][3]) for k in ("min_other", "min_row", "n_conflicts", "first_row")] == [-1, -1, 0, -1]


# ---- row_clearance_capped against row_clearance ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
@pytest.mark.parametrize("family", ["containment", "full"])
def test_rollout_clearance_on_the_families(torch_mod, kind, family):
    """The fused rollout clearance (row_clearance_capped) against the two-call pipeline (row_clearance), bit for bit, with
    the family's scene laid along the rollouts' rows: plateaus and deep contact, and 512 elements."""
    torch = torch_mod
    tk, fp = trc.trk(), fpm()
    K, B = 3, 4
    rows, counts, P = rc.layout_case(kind, K, B)
    if family == "containment":
        case = sc.containment()
        centres = [(0.0, 0.0), (20.0, 0.0), (40.0, 0.0), (60.0, 0.0)]
        spots = [rows[b, r, 6:8] for b, r in ((0, 30), (1, 15), (3, 40), (3, 90))]            # routes 0, 1 and 3 have rows
        polygons = [p + (spots[i] - centres[i]) for i, p in enumerate(case["polygons"])]
        circles = [(*(spots[2 + i] + (c[:2] - centres[2 + i])), c[2]) for i, c in enumerate(case["circles"])]
        scene, foot = fp.Scene(field=rc.FIELD, polygons=polygons, circles=circles), case["foot"]
    else:
        case = sc.full()
        off = rows[0, 40, 6:8] - np.array([30.0, 30.0])                                        # on circle 119, mid-lattice: every route lies inside it
        f = case["field"]
        scene = fp.Scene(field=(f[0] + off[0], f[1] + off[1], f[2] + off[0], f[3] + off[1]), polygons=[p + off for p in case["polygons"]],
                         circles=case["circles"] + [off[0], off[1], 0.0])
        foot = case["foot"]
    follower = trc.make_follower(kind, settle_rows=20, n_substeps=3, tolerance=0.1)
    d_rows, d_counts = torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0")
    outs = []
    for cull in (True, False):
        fused = tk.rollout_clearance(d_rows, d_counts, follower, P, foot, scene, margin=case["margin"], time_step=trc.DT, cull=cull)
        torch.cuda.synchronize()
        trc.check_against_pipeline(torch, kind, fused, d_rows, d_counts, follower, P, foot, scene, case["margin"])
        outs.append(fused)
    trc.assert_same_bits(outs[0], outs[1], trc.FOLLOWER_KEYS[kind] + trc.CLEAR_KEYS, "cull off")
    c = outs[0]["clearance"].cpu().numpy()
    el = outs[0]["clear_rows"][..., 1].cpu().numpy()
    print(f"{kind} on {family}: clearances {np.round(c[~np.isnan(c)], 4).tolist()}, elements {sorted(set(el[el >= -1].tolist()))}")
    assert (c[~np.isnan(c)] < 0).any()
