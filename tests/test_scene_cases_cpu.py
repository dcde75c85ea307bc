"""CPU: the families of tests/scene_cases.py proven on the NumPy references alone (tests/footprint_ref.py,
tests/conflict_ref.py): the closed forms, the classes each family is named for, the rounding D = |float64 - long double|
of the reference against a quarter of tol(X), and how many index outputs the AMBIGUOUS rule leaves out.

The saturated plateau is the global minimum of a route that reaches it.  Where the narrower of the two shapes is a scene
element (or side O, in whose frame the pair reference works), its value is that shape's own extent on its own normal: the
same numbers at every row, in the reference and in the kernels, so the rows tie bit for bit and the first is the answer.
The index gaps of these tests are therefore taken over distinct values (``row_gap_distinct``, ``other_gap_distinct``), and
the families put the narrower shape on that side.  What stays ambiguous is the robot inside the 16-gon of ``containment``,
whose plateau comes from the robot's own posed vertices and differs by rounding from row to row.  The cap on skipped cases
(5 %, test_gpu_conflict.MAX_SKIPPED) is taken per kind of index over the random-pose families of one geometry together;
the threshold is scene_cases.ambiguous(X)."""
import numpy as np
import pytest

import scene_cases as sc
from test_gpu_conflict import AMBIGUOUS, MAX_SKIPPED, Tally


def tally_static(case, tally):
    """What test_gpu_clearance_scenes.check_static will compare for this case, on the reference alone."""
    amb = sc.ambiguous(case["X"])
    for s in sc.static_reference(case):
        if s["min_row"] < 0:
            continue
        tally.case("row", s["row_gap_distinct"] > amb)
        tally.case("other", s["elem_gap"][s["min_row"]] > amb)
        tally.case("margin", s["margin_gap"] > amb)


def tally_pairs(case, shift, tally):
    ref = sc.pair_reference(case, shift)
    amb = sc.ambiguous(case["X"])
    Ba, P = ref["pair_clearance"].shape
    for ia in range(Ba):
        for p in range(P):
            if ref["pair_row"][ia, p] >= 0:
                tally.case("row", ref["pair_row_gap_distinct"][ia, p] > amb)
                tally.case("margin", ref["pair_margin_gap"][ia, p] > amb)
        if ref["min_other"][ia] >= 0:
            tally.case("other", ref["other_gap_distinct"][ia] > amb)
            tally.case("margin", ref["margin_gap"][ia] > amb)


def classes(v):
    """(contact, touching or near, separated) row counts of per-row clearances."""
    v = v[~np.isnan(v)]
    return int((v < 0).sum()), int((np.abs(v) <= 0.05).sum()), int((v > 0).sum())


# ---- closed forms -----------------------------------------------------------------------------------------------------
def test_exact_reproduces_its_closed_forms():
    case = sc.exact()
    s = sc.static_reference(case)[0]
    want = np.array([v for v, _ in case["expect"]])
    assert np.abs(s["rows"] - want).max() <= 1e-15
    assert not np.signbit(s["rows"][want == 0.0]).any()
    assert s["elems"].tolist() == [e for _, e in case["expect"]]
    assert (s["elem_gap"] > 1.0).all()
    assert (s["min_clearance"], s["min_row"], s["min_element"]) == (-0.75, 10, 8)
    assert (s["first_row"], s["n_below"]) == (0, int((want < case["margin"]).sum())) and s["margin_gap"] >= 2.0 ** -4
    # coordinates are multiples of 2^-10
    for a in [case["rows"][0][:, 6:8], case["circles"]] + case["polygons"]:
        assert np.array_equal(a * 1024, np.round(a * 1024))


def test_pair_exact_reproduces_its_closed_forms():
    case = sc.pair_exact()
    for shift in sc.SHIFTS:
        for matched in (True, False):
            ref = sc.pair_reference(case, shift, matched)
            for ia, (v, row, first) in enumerate(case["expect"]["pair"]):
                for p in range(ref["pair_clearance"].shape[1]):
                    assert abs(ref["pair_clearance"][ia, p] - v) <= 1e-15 and (v != 0.0 or not np.signbit(ref["pair_clearance"][ia, p]))
                    assert (ref["pair_row"][ia, p], ref["pair_first_row"][ia, p]) == (row, first)
                    n = len(case["expect"]["per_row"][ia])
                    assert np.abs(ref["pair_rows"][(ia, p)][:n] - case["expect"]["per_row"][ia]).max() <= 1e-15


# ---- the tie families: exact by construction, nothing skipped -------------------------------------------------------
def test_ties_hold_their_plateau():
    for case in sc.ties():
        e = case["expect"]
        for s, r0 in zip(sc.static_reference(case), sc.TIE_R0):
            v = s["rows"]
            assert (v[r0:] == e["plateau"]).all() and (v[:r0] > case["margin"]).all() and e["plateau"] < case["margin"], case["name"]
            assert (s["min_clearance"], s["min_row"], s["first_row"], s["n_below"]) == (e["plateau"], r0, r0, sc.TIE_ROWS - r0)
            assert s["min_element"] == e["element"] and (s["elems"][r0:] == e["element"]).all()
            # the tie: the twins, both circles and (one variant) the wall give the plateau exactly
            assert (s["elem_gap"][r0:] == 0.0).all()
    assert [c["expect"]["element"] for c in sc.ties()] == [3, 3, -1, 201]
    assert [c["expect"]["plateau"] < 0 for c in sc.ties()] == [False, True, False, True]


def test_pair_plateau_holds_its_plateau():
    stand, parallel = sc.pair_plateau()
    for shift in sc.SHIFTS:
        for matched in (True, False):
            ref = sc.pair_reference(stand, shift, matched)
            e = stand["expect"]
            for ia, r0 in enumerate(sc.PLATEAU_R0):
                for p in range(ref["pair_clearance"].shape[1]):
                    v = ref["pair_rows"][(ia, p)]
                    assert (v[r0:] == e["clearance"]).all() and (v[:r0] > e["clearance"]).all()
                    assert (ref["pair_clearance"][ia, p], ref["pair_row"][ia, p], ref["pair_first_row"][ia, p]) == (-1.5, r0, e["first"][ia])
                    assert ref["pair_margin_gap"][ia, p] >= 2.0 ** -8
        for margin, first, ncon in ((1.0, -1, 0), (1.0 + 2.0 ** -40, 0, 1)):
            ref = sc.pair_reference(parallel, shift, True, margin=margin)
            for ia in range(2):
                assert (ref["pair_rows"][(ia, 0)] == 1.0).all()
                assert (ref["pair_clearance"][ia, 0], ref["pair_row"][ia, 0], ref["pair_first_row"][ia, 0]) == (1.0, 0, first)
                assert ref["n_conflicts"][ia] == ncon


def test_pair_others_twins():
    case = sc.pair_others()
    assert np.array_equal(case["rows_o"][3], case["rows_o"][9]) and np.array_equal(case["rows_o"][2], case["rows_o"][20])
    for shift in sc.SHIFTS:
        ref = sc.pair_reference(case, shift)
        assert ref["min_other"].tolist() == case["expect"]["min_other"] and ref["n_conflicts"].tolist() == case["expect"]["n_conflicts"]
        for ia, (lo, hi) in enumerate(((3, 9), (2, 20))):
            assert ref["pair_clearance"][ia, lo] == ref["pair_clearance"][ia, hi] == ref["min_clearance"][ia]
            assert ref["pair_row"][ia, lo] == ref["pair_row"][ia, hi] == ref["min_row"][ia]
            # apart from the twin, nothing is close: the indices are exact without the AMBIGUOUS rule
            rest = np.delete(ref["pair_clearance"][ia], [lo, hi])
            assert rest.min() - ref["min_clearance"][ia] > 0.5 and ref["margin_gap"][ia] > 1e-3
            assert ref["pair_row_gap"][ia, lo] > 1e-6


# ---- the classes each family names ------------------------------------------------------------------------------------
def test_containment_has_contained_rows():
    case = sc.containment()
    refs = sc.static_reference(case)
    alt = 0.25 * np.sqrt(3.0) / 2.0                       # the triangle's altitude: its narrowest extent
    v = [s["rows"] for s in refs]
    contained = [np.abs(v[0] + 1.5) <= 1e-12, np.abs(v[1] + alt) <= 1e-12, v[2] < -5.0, v[3] < -0.1]
    for b in range(4):
        n_con, _, n_sep = classes(v[b])
        assert contained[b].sum() >= 10 and n_sep >= 10 and n_con > contained[b].sum(), (b, int(contained[b].sum()), n_con, n_sep)
    assert [s["min_element"] for s in refs] == [0, 1, 2, 3]
    # the circle centre inside the robot: deeper than the radius, with the deepest row where the walk crosses the centre
    assert refs[2]["min_row"] in (110, 111) and refs[3]["min_row"] in (110, 111)
    assert abs(refs[2]["min_clearance"] + 5.75) < 0.02 and abs(refs[3]["min_clearance"] + 0.85) < 0.01


def test_shapes_have_contact_and_separated_rows():
    for case in sc.shapes():
        v = np.concatenate([s["rows"] for s in sc.static_reference(case)])
        n_con, n_near, n_sep = classes(v)
        assert n_con >= 30 and n_near >= 30 and n_sep >= 30, (case["name"], n_con, n_near, n_sep)
    big = sc.shapes()[-1]
    assert big["X"] > 1000.0 and sc.tol(big["X"]) > 1e-12
    assert len(sc.shapes()[0]["foot"]) == 16 and all(len(p) == 16 for p in sc.shapes()[0]["polygons"])


def test_full_reaches_the_limits_and_its_three_winners():
    case = sc.full()
    assert len(case["polygons"]) == 256 and sum(len(p) for p in case["polygons"]) == 4096 and len(case["circles"]) == 256
    assert len(case["foot"]) == 16
    refs = sc.static_reference(case)
    for s in refs[:2]:
        for e in case["expect"]:
            assert (s["elems"] == e).sum() >= 10, e
    assert tuple(s["min_element"] for s in refs[2:]) == case["expect"]
    assert refs[0]["min_element"] == -1 and refs[0]["min_clearance"] < 0


def test_pair_shapes_have_their_classes():
    cases = sc.pair_shapes()
    for case in cases:
        ref = sc.pair_reference(case)
        v = np.concatenate(list(ref["pair_rows"].values()))
        n_con, _, n_sep = classes(v)
        assert n_con >= 30 and n_sep >= 30, (case["name"], n_con, n_sep)
    ref = sc.pair_reference(cases[2])
    v = np.concatenate(list(ref["pair_rows"].values()))
    saturated = np.abs(v + 0.01) <= 1e-12                 # the small robot's extent: contained in the large one's projection
    assert saturated.sum() >= 30 and ((v < 0) & ~saturated).sum() >= 30 and (v > 0).sum() >= 30, (saturated.sum(), ((v < 0) & ~saturated).sum())
    assert (np.abs(ref["pair_clearance"] + 0.01) <= 1e-12).any() and (ref["pair_clearance"] > 0).any()


def test_nan_rows_family():
    static, pair = sc.nan_rows()
    refs = sc.static_reference(static)
    lo, hi = sc.NAN_BLOCK
    for b, s in enumerate(refs[:3]):
        bad = np.isnan(static["rows"][b][:, [4, 6, 7]]).any(axis=1)
        assert np.array_equal(np.isnan(s["rows"]), bad) and bad.sum() == (67, 67, 1)[b]
        assert not bad[s["min_row"]] and (s["first_row"] < 0 or not bad[s["first_row"]])
        assert s["n_below"] == int((s["rows"][~bad] < static["margin"]).sum()) > 0
        # nothing is close: the GPU test compares these indices exactly
        assert min(s["row_gap_distinct"], s["margin_gap"], s["elem_gap"][s["min_row"]]) > AMBIGUOUS
    assert refs[0]["min_row"] < lo and refs[1]["min_row"] >= hi
    assert refs[2]["min_row"] != static["masked_min_row"] and abs(refs[2]["min_row"] - static["masked_min_row"]) == 1
    s = refs[3]
    assert np.isnan(s["rows"]).all() and np.isnan(s["min_clearance"])
    assert (s["min_row"], s["min_element"], s["first_row"], s["n_below"]) == (-1, -1, -1, 0)
    for shift in sc.SHIFTS:
        ref = sc.pair_reference(pair, shift)
        assert np.isnan(ref["pair_clearance"][3]).all() and (ref["pair_row"][3] == -1).all() and (ref["pair_first_row"][3] == -1).all()
        assert np.isnan(ref["min_clearance"][3])
        assert (ref["min_other"][3], ref["min_row"][3], ref["n_conflicts"][3], ref["first_row"][3]) == (-1, -1, 0, -1)
        assert np.isfinite(ref["pair_clearance"][:3]).all()
        assert min(ref["pair_row_gap_distinct"][:3].min(), ref["pair_margin_gap"][:3].min(), ref["other_gap_distinct"][:3].min()) > AMBIGUOUS
        for (ia, p), v in ref["pair_rows"].items():
            if ia < 3:
                assert 0 < np.isnan(v).sum() < len(v) and not np.isnan(v[ref["pair_row"][ia, p]])


# ---- the reference earns the tolerance --------------------------------------------------------------------------------
def static_families():
    return [sc.exact()] + sc.ties() + [sc.containment()] + sc.shapes() + [sc.nan_rows()[0]]


def pair_families():
    return [sc.pair_exact(), *sc.pair_plateau()] + sc.pair_shapes() + [sc.pair_others(), sc.nan_rows()[1]]


def test_reference_rounding_is_a_quarter_of_the_tolerance_static():
    worst = {}
    for case in static_families() + [c for X in sc.FAR for c, _ in sc.far(X)]:
        d = sc.static_D(case)
        worst[case["name"]] = d
        assert d <= sc.tol(case["X"]) / 4, (case["name"], d, case["X"])
    print("D static:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_reference_rounding_is_a_quarter_of_the_tolerance_full():
    case = sc.full()
    d = sc.static_D(case)
    print(f"D full: {d:.1e}")
    assert d <= sc.tol(case["X"]) / 4


def test_reference_rounding_is_a_quarter_of_the_tolerance_pairs():
    worst = {}
    for case in pair_families() + [c for X in sc.FAR for c, _ in sc.pair_far(X)]:
        d = max(sc.pair_D(case, shift) for shift in (0, 5))
        worst[case["name"]] = d
        assert d <= sc.tol(case["X"]) / 4, (case["name"], d, case["X"])
    print("D pairs:", {k: f"{v:.1e}" for k, v in worst.items()})


# ---- far: the translation is exact --------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", sc.FAR)
def test_far_is_the_same_geometry(X):
    for there, here in sc.far(X):
        assert there["X"] >= X - 16 and np.array_equal(there["rows"][:, :, 6] - X, here["rows"][:, :, 6], equal_nan=True)
        assert all(np.array_equal(p - [X, -X], q) for p, q in zip(there["polygons"], here["polygons"]))
        d = max(np.abs(a["rows"] - b["rows"]).max() for a, b in zip(sc.static_reference(there), sc.static_reference(here)))
        assert d <= sc.tol(X) / 4 + sc.tol(0) / 4, (there["name"], d)
    for there, here in sc.pair_far(X):
        assert there["X"] >= X - 16 and np.array_equal(there["rows_a"][:, :, 7] + X, here["rows_a"][:, :, 7], equal_nan=True)
        a, b = sc.pair_reference(there), sc.pair_reference(here)
        assert np.abs(a["pair_clearance"] - b["pair_clearance"]).max() <= sc.tol(X) / 4 + sc.tol(0) / 4


# ---- how much the AMBIGUOUS rule leaves out ---------------------------------------------------------------------------
def test_ambiguous_indices_stay_under_the_cap():
    tally = Tally()
    for case in [sc.containment(), sc.full()] + sc.shapes() + [c for X in sc.FAR for pair in sc.far(X) for c in pair]:
        tally_static(case, tally)
    tally.close("static random-pose families", MAX_SKIPPED)
    tally = Tally()
    for case in sc.pair_shapes() + [c for X in sc.FAR for pair in sc.pair_far(X) for c in pair]:
        for shift in sc.SHIFTS:
            tally_pairs(case, shift, tally)
    tally.close("pair random-pose families", MAX_SKIPPED)
