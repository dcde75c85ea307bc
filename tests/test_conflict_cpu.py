"""CPU: the robot-to-robot clearance definitions (include/vap.h, vap_footprint_conflicts) on hand-computed cases through
the NumPy reference of tests/conflict_ref.py, the reference's symmetry and its two evaluation orders against each other,
the C-ABI's declaration, export and binding, and the host-side footprint validation of footprint.conflicts."""
import math
import os
import re

import numpy as np
import pytest

import conflict_ref as cr
from vexautonomousplanner_amd import _lib
from vexautonomousplanner_amd import footprint as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])       # 1 ft square, counter-clockwise
NARROW = np.array([[-0.6, -0.625], [0.6, -0.625], [0.6, 0.625], [-0.6, 0.625]])


def rows_of(poses):
    """(n, 8) rows from (heading, x, y) triples, 10 ms apart."""
    r = np.zeros((len(poses), 8))
    r[:, [4, 6, 7]] = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    r[:, 0] = 0.01 * np.arange(len(poses))
    return r


def one(pa, po, foot_a=UNIT, foot_o=UNIT):
    return float(cr.pair_rows(rows_of([pa]), 1, foot_a, rows_of([po]), 1, foot_o)[0])


def random_walk(rng, n):
    r = np.zeros((n, 8))
    r[:, 6:8] = rng.uniform(-3, 3, 2) + np.cumsum(rng.normal(0, 0.05, (n, 2)), axis=0)
    r[:, 4] = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.normal(0, 0.05, n))
    return r


def test_two_squares_apart_overlapping_touching():
    assert one((0, 0, 0), (0, 1.5, 0)) == pytest.approx(0.5, abs=1e-15)
    assert one((0, 0, 0), (0, 0.8, 0)) == pytest.approx(-0.2, abs=1e-15)
    assert one((0, 0, 0), (0, 0, -1.5)) == pytest.approx(0.5, abs=1e-15)
    assert one((0, 0, 0), (0, 1.0, 0)) == pytest.approx(0.0, abs=1e-15)
    # diagonal: corner to corner
    assert one((0, 0, 0), (0, 2.0, 2.0)) == pytest.approx(math.sqrt(2), abs=1e-15)
    # the pose convention: a heading of h turns the body by -h; an offset rectangle shows the sign
    front = np.array([[0.0, -0.5], [2.0, -0.5], [2.0, 0.5], [0.0, 0.5]])                # reaches 2 ft ahead of the point
    assert one((math.pi / 2, 0, 0), (0, 0, -4.0), foot_a=front) == pytest.approx(1.5, abs=1e-14)   # phi = -90 deg: ahead is -y
    assert one((math.pi / 2, 0, 0), (0, 0, 4.0), foot_a=front) == pytest.approx(3.5, abs=1e-14)    # behind: nothing of it


def test_square_turned_by_45_degrees():
    # the other's corner points at us: 2 - 0.5 - sqrt(2)/2
    assert one((0, 0, 0), (math.pi / 4, 2.0, 0)) == pytest.approx(1.5 - math.sqrt(0.5), abs=1e-15)
    # overlapping: the smallest overlap is along our own x axis, 0.5 + sqrt(2)/2 - 1
    assert one((0, 0, 0), (-math.pi / 4, 1.0, 0)) == pytest.approx(0.5 - math.sqrt(0.5), abs=1e-15)
    # both turned: two parallel faces again
    assert one((math.pi / 4, 0, 0), (math.pi / 4, 1.0, 1.0)) == pytest.approx(math.sqrt(2) - 1.0, abs=1e-15)


def test_saturation_at_the_narrower_extent():
    # one on top of the other: minus the narrower footprint's extent, however the two sit
    assert one((0, 0, 0), (0, 0.01, 0.02), foot_a=np.array(UNIT) * 1.5, foot_o=NARROW) == pytest.approx(-1.2, abs=1e-15)
    assert one((0, 0, 0), (0, 0.03, -0.01), foot_a=np.array(UNIT) * 1.5, foot_o=NARROW) == pytest.approx(-1.2, abs=1e-15)


def test_parked_robot_passed_by_a_moving_one():
    # both squares turned by 45 degrees, corner towards corner: o sits at (0, 2); a drives along y = 0 from x = -2 in
    # 0.25 ft steps.  The corners are hypot(x, 2 - sqrt(2)) apart: closest at x = 0, row 8
    q = math.pi / 4
    a = rows_of([(q, -2 + 0.25 * i, 0) for i in range(17)])
    o = rows_of([(q, 0, 2.0)])
    ref = cr.conflicts(a[None], [17], UNIT, o[None], [1], margin=0.65)
    h = 2.0 - math.sqrt(2.0)
    assert ref["pair_clearance"][0, 0] == pytest.approx(h, abs=1e-15) and ref["pair_row"][0, 0] == 8
    v = ref["pair_rows"][(0, 0)]
    assert len(v) == 17
    np.testing.assert_allclose(v[6:11], [math.hypot(x, h) for x in (-0.5, -0.25, 0.0, 0.25, 0.5)], atol=1e-15)
    # below the margin while hypot(x, 0.586) < 0.65, |x| < 0.28: rows 7, 8, 9
    assert ref["pair_first_row"][0, 0] == 7 and int(np.sum(v < 0.65)) == 3
    assert (ref["min_clearance"][0], ref["min_other"][0], ref["min_row"][0], ref["n_conflicts"][0], ref["first_row"][0]) == \
        (ref["pair_clearance"][0, 0], 0, 8, 1, 7)
    assert ref["pair_row_gap"][0, 0] == pytest.approx(math.hypot(0.25, h) - h, abs=1e-15)
    # the other way round: the moving one is the "other"
    swapped = cr.conflicts(o[None], [1], UNIT, a[None], [17], margin=0.65)
    assert swapped["pair_row"][0, 0] == 8 and swapped["pair_first_row"][0, 0] == 7


def test_shift_of_either_sign_and_the_horizon():
    # two robots driving the same line towards each other's start, 1 ft per row
    a = rows_of([(0, float(i), 0) for i in range(6)])            # x = 0 .. 5
    o = rows_of([(0, 5.0 - i, 3.0) for i in range(4)])           # x = 5 .. 2, 3 ft to the side
    gap = lambda xa, xo: math.hypot(max(abs(xa - xo) - 1.0, 0.0), 2.0)
    for shift in (0, 2, 4, -1, -3, -10, 9):
        assert cr.horizon(6, 4, shift) == max(6, 4 + shift, 1)
        v = cr.pair_rows(a, 6, UNIT, o, 4, UNIT, shift)
        assert len(v) == max(6, 4 + shift)
        want = [gap(min(r, 5), 5.0 - min(max(r - shift, 0), 3)) for r in range(len(v))]
        np.testing.assert_allclose(v, want, atol=1e-15)
    # a later start moves the meeting: shift 0 -> they pass between rows 2 and 3; shift 4 -> o still parked at x = 5
    assert int(np.argmin(cr.pair_rows(a, 6, UNIT, o, 4, UNIT, 0))) == 2
    assert int(np.argmin(cr.pair_rows(a, 6, UNIT, o, 4, UNIT, 4))) == 4
    # counts shorter than the arrays; a horizon of one row
    assert len(cr.pair_rows(a, 1, UNIT, o, 1, UNIT, -5)) == 1
    assert len(cr.pair_rows(a, 2, UNIT, o, 3, UNIT, 0)) == 3


def test_empty_sides():
    a = rows_of([(0, 0, 0), (0, 1, 0)])
    o = rows_of([(0, 0, 3), (0, 1, 3)])
    ref = cr.conflicts(np.stack([a, a]), [2, 0], UNIT, np.stack([o, o, o]), [0, 2, 0], margin=5.0)
    assert np.isnan(ref["pair_clearance"][0, [0, 2]]).all() and np.isnan(ref["pair_clearance"][1]).all()
    assert ref["pair_row"][0].tolist() == [-1, 0, -1] and ref["pair_first_row"][0].tolist() == [-1, 0, -1]
    assert (ref["min_clearance"][0], ref["min_other"][0], ref["min_row"][0], ref["n_conflicts"][0], ref["first_row"][0]) == (2.0, 1, 0, 1, 0)
    assert math.isnan(ref["min_clearance"][1])
    assert (ref["min_other"][1], ref["min_row"][1], ref["n_conflicts"][1], ref["first_row"][1]) == (-1, -1, 0, -1)
    none = cr.conflicts(np.zeros((2, 0, 8)), [0, 0], UNIT, np.stack([o]), [2])
    assert np.isnan(none["min_clearance"]).all() and (none["n_conflicts"] == 0).all()


def test_matched_pairing_is_the_diagonal():
    rng = np.random.default_rng(3)
    a = np.stack([random_walk(rng, 40) for _ in range(4)])
    o = np.stack([random_walk(rng, 30) for _ in range(4)])
    ca, co = [40, 7, 0, 22], [30, 30, 5, 1]
    full = cr.conflicts(a, ca, UNIT * 1.5, o, co, NARROW, margin=0.25, shift=3)
    diag = cr.conflicts(a, ca, UNIT * 1.5, o, co, NARROW, margin=0.25, shift=3, matched=True)
    for k in ("pair_clearance", "pair_row", "pair_first_row"):
        np.testing.assert_array_equal(np.diagonal(full[k]), diag[k][:, 0])
    np.testing.assert_array_equal(diag["min_other"], [0, 1, -1, 3])


def test_reference_is_symmetric_and_its_two_forms_agree():
    rng = np.random.default_rng(11)
    tri = np.array([[-0.4, -0.5], [0.9, 0.0], [-0.4, 0.6]])
    worst, signs = 0.0, set()
    for shift in (0, 13, -6):
        a, o = random_walk(rng, 50), random_walk(rng, 35)
        o[:, 6:8] += a[0, 6:8] - o[0, 6:8] + rng.normal(0, 0.5, 2)          # near each other: both branches are taken
        # The horizon starts at side A's row 0, so a swap with a nonzero shift moves the time origin and drops the rows
        # before the new side A's start.  Robots that wait at their first pose for at least |shift| rows lose only
        # repeats of a pose pair that is still examined: then the swap changes nothing but the row numbers.
        a[:14], o[:14] = a[13], o[13]
        v = cr.pair_rows(a, 50, UNIT * 1.5, o, 35, tri, shift)
        signs |= set(np.sign(v))
        direct = cr.pair_rows_direct(a, 50, UNIT * 1.5, o, 35, tri, shift)
        worst = max(worst, float(np.max(np.abs(v - direct))))
        w = cr.pair_rows(o, 35, tri, a, 50, UNIT * 1.5, -shift)
        lo = max(shift, 0)
        np.testing.assert_allclose(v[lo:lo + 30], w[lo - shift:lo - shift + 30], atol=1e-13)
        assert abs(v.min() - w.min()) <= 1e-13
    assert worst <= 1e-13, worst
    assert {-1.0, 1.0} <= signs          # overlapping and separated rows were both compared


def header_prototype(name):
    src = open(os.path.join(ROOT, "include", "vap.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/vap.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_abi_declared_exported_and_bound():
    args = header_prototype("vap_footprint_conflicts")
    assert len(args) == 26 and args[0] == "vap_ctx *ctx" and args[1:4] == ["int pairing", "int shift_rows", "double margin"]
    assert "vap_footprint_conflicts" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "vap_footprint_conflicts"), "libvap.so does not export vap_footprint_conflicts"
    assert len(L.vap_footprint_conflicts.argtypes) == len(args)
    src = open(os.path.join(ROOT, "include", "vap.h")).read()
    assert re.search(r"VAP_CONFLICT_ALL_PAIRS\s*=\s*0", src) and re.search(r"VAP_CONFLICT_MATCHED\s*=\s*1", src)
    assert (_lib.CONFLICT_ALL_PAIRS, _lib.CONFLICT_MATCHED) == (0, 1)
    assert callable(fp.conflicts)
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    assert callable(BatchedTrajectoryGenerator.footprint_conflicts)


def test_bad_footprints_raise_before_any_device_work():
    rows, counts = np.zeros((2, 4, 8)), [4, 4]
    seventeen = [[math.cos(t), math.sin(t)] for t in np.linspace(0, 2 * math.pi, 18)[:-1]]
    dent = [[0, 0], [2, 0], [1, 0.5], [2, 2], [0, 2]]
    for bad in (UNIT[::-1], dent, seventeen, UNIT[:2], [[0, 0], [1, 0], [2, 0], [1, 1]]):
        with pytest.raises(ValueError):
            fp.conflicts(rows, counts, bad, rows, counts)
        with pytest.raises(ValueError):
            fp.conflicts(rows, counts, UNIT, rows, counts, footprint_o=bad)
    with pytest.raises(ValueError):
        fp.conflicts(rows, counts, UNIT, rows, counts, pairing="some")
