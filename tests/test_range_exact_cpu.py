"""CPU: the exact families of tests/range_exact_cases.py bite, shown on the NumPy reference alone.

range_ref.readings equals the exact checker (the header's rules in fractions.Fraction) on every reading of every family: range
and cosine bit for bit, status, face and element equal, nothing excused.  (The sign of a zero range is the one thing left out
here: the header's quotient 0 / den has none, the reference's float quotient has; test_gpu_range_exact.py holds the kernel to
the reference's.)  Each family holds the decisions it is named for, counted; the moved cases reproduce their bases on the
reference itself; and switching one rule of the checker to its neighbour changes a reading of the family built for it."""
import functools

import numpy as np
import pytest

import range_cases as rc
import range_exact_cases as xc
import range_ref as rr

FAMILY_NAMES = tuple(xc.FAMILIES)


@functools.lru_cache(maxsize=None)
def checked(fam):
    """{case name: (reference, checker)} of a family, computed once."""
    return {name: (rc.reference(rr, case), xc.exact_readings(case)) for name, case in xc.family(fam).items()}


def flags_of(fam):
    total = {}
    for _, (_, ex) in checked(fam).items():
        for k, v in ex["flags"].items():
            total[k] = total.get(k, 0) + v
    return total


def margin_zero(fam):
    return sum(int((ref["margin"][ref["live"]] == 0.0).sum()) for ref, _ in checked(fam).values())


def statuses(fam):
    out = np.zeros(7, dtype=np.int64)
    for ref, _ in checked(fam).values():
        out += np.bincount(ref["status"][ref["live"]].ravel(), minlength=7)
    return out


# ---- 1. the reference is the header, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_reference_equals_the_exact_checker(fam):
    n = 0
    for name, (ref, ex) in checked(fam).items():
        live = ref["live"]
        assert xc.same_readings(ex, ref, zero_sign=False) is None, (name, xc.same_readings(ex, ref, zero_sign=False))
        assert not ((ref["status"] == rr.BAD_POSE) & live[:, :, None]).any(), name
        n += int(live.sum()) * ref["status"].shape[2]
    print(f"RANGE EXACT {fam}: {n} readings equal the checker, {margin_zero(fam)} with margin exactly 0, statuses {statuses(fam).tolist()}, "
          f"decisions {flags_of(fam)}")
    assert n > 0


# ---- 2. each family holds its decisions -----------------------------------------------------------------------------------------
# (family, decision, at least this many readings): the decisions each family was built for
MINIMA = (
    ("lattice", "margin 0", 1000), ("lattice", "hit on a vertex", 100), ("lattice", "beam along an edge's line", 100),
    ("lattice", "tie polygon edges", 50), ("lattice", "t == r_min", 5), ("lattice", "t == r_max", 5), ("lattice", "cos == min_cos", 100),
    ("lattice", "tangent circle", 10),
    ("ties", "margin 0", 60), ("ties", "tie polygon > polygon", 10), ("ties", "tie polygon > circle", 3), ("ties", "tie wall > circle", 4),
    ("ties", "tie wall > polygon", 6), ("ties", "tie polygon > partner", 20), ("ties", "tie partner > partner", 5),
    ("vertices", "margin 0", 100), ("vertices", "hit on a vertex", 100), ("vertices", "tie polygon edges", 60),
    ("vertices", "beam along an edge's line", 60),
    ("origins", "margin 0", 200), ("origins", "origin on the box", 60), ("origins", "origin on an edge", 30), ("origins", "origin on a circle", 30),
    ("origins", "tie wall corner", 40),
    ("tangent", "margin 0", 60), ("tangent", "tangent circle", 60),
    ("thresholds", "margin 0", 30), ("thresholds", "t == r_min", 9), ("thresholds", "t == r_max", 9), ("thresholds", "cos == min_cos", 12),
    ("wide", "margin 0", 10000),
    ("moved", "margin 0", 3000), ("moved", "tie polygon > partner", 100),
)


@pytest.mark.parametrize("fam,what,least", MINIMA)
def test_family_holds_its_decisions(fam, what, least):
    got = margin_zero(fam) if what == "margin 0" else flags_of(fam).get(what, 0)
    assert got >= least, (fam, what, got)


def test_every_status_is_met():
    """0 valid, 2 near, 3 far, 4 oblique on the lattice; 1 none from origins outside the field; 5 blocked by the partners."""
    assert (statuses("lattice")[[0, 2, 3, 4]] >= 100).all(), statuses("lattice")
    assert statuses("origins")[1] >= 20 and statuses("ties")[5] >= 20
    total = sum(statuses(f) for f in FAMILY_NAMES)
    assert (total[:6] > 0).all() and total[6] == 0


def test_threshold_sides_by_hand():
    """around(): r_min = t, t+, t-; r_max = t, t+, t-; r_min = r_max = t; min_cos = cos.  Equality is valid on every threshold; one
    ulp above t as r_min is NEAR, one ulp below t as r_max is FAR, one ulp above the cosine as min_cos is OBLIQUE."""
    for name in ("thresholds wall", "thresholds edge", "thresholds third"):
        ref, _ = checked("thresholds")[name]
        assert ref["status"][0, 0].tolist() == [0, 2, 0, 0, 0, 3, 0, 0], (name, ref["status"][0, 0])
        assert ref["status"][0, 2].tolist() == ref["status"][0, 0].tolist()
    ref, _ = checked("thresholds")["thresholds cos"]
    assert ref["status"][0, 0].tolist() == [0, 0, 0, 4, 0, 0, 4, 0], ref["status"][0, 0]
    # the pose half a foot on: the wall reading is 5.5, below every r_min of 6 and one ulp around it
    ref, _ = checked("thresholds")["thresholds wall"]
    assert ref["status"][0, 1].tolist() == [2, 2, 2, 0, 0, 0, 2, 0] and (ref["t"][0, 1] == 5.5).all()


def test_wide_takes_the_four_step_tile_and_both_scene_paths():
    plain, padded = xc.family("wide")["wide"], xc.family("wide")["wide padded"]
    B, cap = plain["rows"].shape[:2]
    assert B * ((cap + 1023) // 1024) >= 1024
    assert xc.packed_doubles(plain["scene"]) <= 2048 < xc.packed_doubles(padded["scene"])
    counts = plain["counts"]
    assert (counts <= 12).mean() > 0.9 and {255, 256, 257, 300} <= set(counts.tolist())
    a, b = checked("wide")["wide"][0], checked("wide")["wide padded"][0]
    el = np.where(b["element"] >= len(padded["scene"]["polygons"]), b["element"] - xc.PAD_POLYGONS, b["element"])
    assert xc.same_readings(a, dict(b, element=el)) is None


# ---- 3. moved: translation and scaling are identities, on the reference itself --------------------------------------------------
def test_moved_holds_on_the_reference():
    bases = xc.moved_bases()
    got = checked("moved")
    n_loose = n = 0
    for name, kind, amount, _ in xc.moved_variants():
        base, moved = got[f"moved {name} base"][0], got[f"moved {name} {kind} {amount:g}"][0]
        n_loose += xc.check_moved(bases[name], base, kind, amount, moved, (name, kind, amount))
        n += int(base["live"].sum()) * base["status"].shape[2]
    print(f"RANGE EXACT moved: {n} readings, {n_loose} circle cosines taken at a rounded hit point")
    assert n_loose < 0.1 * n


# ---- 4. a switched rule changes a reading ---------------------------------------------------------------------------------------
SWITCHES = (("w_inclusive", "vertices", "vertices"), ("t_inclusive", "origins", "origins"), ("box_inclusive", "origins", "origins"),
            ("first_wins_edges", "ties", "ties scene"), ("first_wins_edges", "vertices", "vertices"),
            ("first_wins_edges", "ties", "ties 16 partners"), ("first_wins_edges", "ties", "ties partner"),
            ("first_wins_circles", "ties", "ties scene"), ("wall_tie_x", "origins", "origins corner"),
            ("disc_inclusive", "tangent", "tangent"), ("near_strict", "thresholds", "thresholds edge"),
            ("far_strict", "thresholds", "thresholds third"), ("oblique_strict", "thresholds", "thresholds cos"),
            ("near_strict", "thresholds", "thresholds wall"), ("far_strict", "thresholds", "thresholds edge"),
            ("oblique_strict", "lattice", "lattice"))


@pytest.mark.parametrize("rule,fam,name", SWITCHES)
def test_a_switched_rule_changes_a_reading(rule, fam, name):
    case = xc.family(fam)[name]
    _, ex = checked(fam)[name]
    flipped = xc.exact_readings(case, check_exact=False, **{rule: False})
    diff = xc.same_readings(ex, flipped, zero_sign=False)
    assert diff is not None, (rule, name)
    # and only where the reference says a decision sits: a reading the switch changes has margin exactly 0
    ref, _ = checked(fam)[name]
    changed = np.zeros(ref["status"].shape, dtype=bool)
    for k in ("status", "face", "element"):
        changed |= ex[k] != flipped[k]
    assert changed.any() and (ref["margin"][changed] == 0.0).all(), (rule, name)
