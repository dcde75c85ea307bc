"""CPU: the definitions of the clearance over a window of start shifts (include/vap.h, vap_conflict_shifts) through the
reference of tests/shift_ref.py: its two statements of the definition against each other for all 16 hold masks, hold 14
against the existing call's reference, the scan rules on hand-written masks, the analytic crossing, and the C-ABI's
declaration, export and binding."""
import math
import os
import re

import numpy as np
import pytest

import conflict_ref as cr
import shift_ref as sr
from vexautonomousplanner_amd import _lib
from vexautonomousplanner_amd import footprint as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])
NARROW = np.array([[-0.6, -0.625], [0.6, -0.625], [0.6, 0.625], [-0.6, 0.625]])


def random_walk(rng, n):
    r = np.zeros((n, 8))
    r[:, 6:8] = rng.uniform(-2, 2, 2) + np.cumsum(rng.normal(0, 0.08, (n, 2)), axis=0)
    r[:, 4] = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.normal(0, 0.05, n))
    r[:, 0] = 0.01 * np.arange(n)
    return r


PAIRS = [(1, 1), (1, 9), (7, 1), (12, 5), (6, 17), (23, 23)]


@pytest.fixture(scope="module")
def small_pairs():
    rng = np.random.default_rng(11)
    out = []
    for n_a, n_o in PAIRS:
        a, o = random_walk(rng, n_a), random_walk(rng, n_o)
        if n_a == 12:
            a[3, 6] = np.nan                                   # a NaN pose: its clearances take part in nothing
        out.append((a, o, sr.clearance_matrix(a, n_a, UNIT, o, n_o, NARROW)))
    return out


def test_the_two_statements_agree_for_every_hold_mask(small_pairs):
    cases = 0
    for a, o, M in small_pairs:
        n_a, n_o = M.shape
        shifts = np.arange(-n_o - 5, n_a + 6)
        for hold in range(16):
            fast = sr.table_fast(M, shifts, hold)
            direct = np.array([sr.table_direct(M, int(s), hold) for s in shifts])
            np.testing.assert_array_equal(fast, direct, err_msg=f"{M.shape} hold {hold}")
            cases += len(shifts)
    assert cases == 16 * sum(n_a + n_o + 11 for n_a, n_o in PAIRS)


def test_hold_bits_drop_what_they_say(small_pairs):
    a, o, M = small_pairs[4]                                   # 6 x 17
    n_a, n_o = M.shape
    assert sr.examined(n_a, n_o, 0, 0) == [(t, t) for t in range(6)]
    assert sr.examined(n_a, n_o, 3, 0) == [(t, t - 3) for t in range(3, 6)]
    assert sr.examined(n_a, n_o, 3, sr.O_FIRST)[:3] == [(0, 0), (1, 0), (2, 0)]
    assert sr.examined(n_a, n_o, -2, sr.A_FIRST)[:2] == [(0, 0), (0, 1)]
    assert sr.examined(n_a, n_o, 0, sr.A_LAST)[-1] == (5, 16) and len(sr.examined(n_a, n_o, 0, sr.A_LAST)) == 17
    assert sr.examined(n_a, n_o, -15, sr.O_LAST) == [(0, 15), (1, 16)] + [(t, 16) for t in range(2, 6)]
    assert sr.examined(n_a, n_o, 9, 0) == [] and math.isnan(sr.table_direct(M, 9, 0))
    # past both ends with every bit: the far corner pairs
    assert sr.examined(n_a, n_o, 8, 15)[6:8] == [(5, 0), (5, 0)] and sr.examined(n_a, n_o, -19, 15)[17:19] == [(0, 16), (0, 16)]


def test_hold_14_is_the_existing_call(small_pairs):
    for a, o, M in small_pairs:
        n_a, n_o = M.shape
        shifts = np.arange(-n_o - 5, n_a + 6)
        tab = sr.table_fast(M, shifts, 14)
        for s, got in zip(shifts, tab):
            v = cr.pair_rows(a, n_a, UNIT, o, n_o, NARROW, int(s))
            v = v[~np.isnan(v)]
            assert got == v.min(), (M.shape, s)


def test_scan_rules_on_hand_written_masks():
    m = [1, 0, 0, 1, 0, 0, 0, 1, 0]
    assert sr.scan(m, 1, +1) == (1, 6) and sr.scan(m, 1, -1) == (8, 6)
    assert sr.scan(m, 3, +1) == (4, 6) and sr.scan(m, 3, -1) == (6, 6)
    assert sr.scan(m, 2, +1) == (1, 6) and sr.scan(m, 2, -1) == (6, 6)
    assert sr.scan(m, 4, +1) == (-1, 6) and sr.scan(m, 4, -1) == (-1, 6)
    free = [0] * 5
    assert sr.scan(free, 5, +1) == (0, 5) and sr.scan(free, 5, -1) == (4, 5)
    assert sr.scan(free, 6, +1) == (-1, 5) and sr.scan(free, 6, -1) == (-1, 5)        # a run longer than the window
    assert sr.scan([1, 1], 1, +1) == (-1, 0)


def test_invalid_pairs_and_routes_without_a_valid_pair():
    rng = np.random.default_rng(3)
    rows_a = np.stack([random_walk(rng, 8) for _ in range(3)])
    rows_o = np.stack([random_walk(rng, 8) for _ in range(2)])
    kw = dict(margin=10.0, shift_lo=-2, n_shifts=5, hold=14)
    r = sr.sweep(rows_a, [8, 0, 5], UNIT, rows_o, [0, 6], **kw)
    assert np.isnan(r["pair_table"][:, 0]).all() and np.isnan(r["pair_table"][1]).all()
    assert r["pair_first"].tolist() == [[-1, -1], [-1, -1], [-1, -1]] and r["pair_safe"].tolist() == [[0, 0], [0, 0], [0, 0]]
    assert r["route_first"].tolist() == [-1, -1, -1] and r["route_safe"].tolist() == [0, 0, 0]       # margin 10 ft blocks all
    assert np.isnan(r["route_table"][1]).all() and not np.isnan(r["route_table"][[0, 2]]).any()
    # no valid pair: a route with rows is blocked nowhere, a route without rows gets -1 / 0
    for direction, first in ((+1, 0), (-1, 4)):
        r = sr.sweep(rows_a, [8, 0, 5], UNIT, rows_o, [0, 0], direction=direction, **kw)
        assert r["route_first"].tolist() == [first, -1, first] and r["route_safe"].tolist() == [5, 0, 5]
        assert np.isnan(r["route_table"]).all() and (r["pair_first"] == -1).all() and (r["pair_safe"] == 0).all()
    r = sr.sweep(rows_a, [8, 0, 5], UNIT, rows_o, [0, 0], min_run=6, **kw)
    assert r["route_first"].tolist() == [-1, -1, -1] and r["route_safe"].tolist() == [5, 0, 5]
    # a per-route base moves the window
    base = [3, 0, -4]
    r = sr.sweep(rows_a, [8, 0, 5], UNIT, rows_o, [7, 6], base=base, **kw)
    for ia in (0, 2):
        moved = sr.sweep(rows_a, [8, 0, 5], UNIT, rows_o, [7, 6], **dict(kw, shift_lo=-2 + base[ia]))
        np.testing.assert_array_equal(r["pair_table"][ia], moved["pair_table"][ia])


def test_binding_and_header():
    header = open(os.path.join(ROOT, "include", "vap.h")).read()
    m = re.search(r"\bint vap_conflict_shifts\(([^;]*)\);", header)
    assert m, "include/vap.h does not declare vap_conflict_shifts"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert "vap_conflict_shifts" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "vap_conflict_shifts") and len(L.vap_conflict_shifts.argtypes) == len(args) == 30
    assert [a.split()[-1].lstrip("*") for a in args[:10]] == ["ctx", "pairing", "hold", "margin", "shift_lo", "shift_step", "n_shifts",
                                                             "d_shift_base", "min_run", "scan"]
    assert [a.split()[-1].lstrip("*") for a in args[-6:]] == ["d_table", "d_pair_first", "d_pair_safe", "d_route_table", "d_route_first",
                                                             "d_route_safe"]
    assert (_lib.HOLD_A_FIRST, _lib.HOLD_A_LAST, _lib.HOLD_O_FIRST, _lib.HOLD_O_LAST) == (1, 2, 4, 8)
    assert "VAP_HOLD_A_FIRST = 1, VAP_HOLD_A_LAST = 2, VAP_HOLD_O_FIRST = 4, VAP_HOLD_O_LAST = 8" in header
    assert f"#define VAP_CONFLICT_SHIFTS_MAX {_lib.CONFLICT_SHIFTS_MAX}" in header and _lib.CONFLICT_SHIFTS_MAX >= 4096
    assert fp.HOLD_CONFLICTS == 14 and fp.HOLD_ALL == 15
    for f in (fp.shifts, fp.earliest_start):
        assert callable(f)
    from vexautonomousplanner_amd import timeline
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    assert callable(timeline.dwell_to_clear)
    assert callable(BatchedTrajectoryGenerator.conflict_shifts) and callable(BatchedTrajectoryGenerator.earliest_start)
    # the wrappers validate on the host before anything touches a device
    a, o, unit = sr.crossing()
    with pytest.raises(ValueError):
        fp.shifts(a, None, unit, o, None, scan="sideways")
    with pytest.raises(ValueError):
        fp.shifts(a, None, unit[::-1], o, None)
    with pytest.raises(ValueError):
        fp.earliest_start(a, None, unit, o, None, who="both")


def delay(tab, margin, who, max_delay, min_run=1):
    """earliest_start's rule on a reference table over shifts -max_delay .. max_delay."""
    b = tab < margin
    mid = len(tab) // 2
    if who == "o":
        first, _ = sr.scan(b[mid:mid + max_delay + 1], min_run, +1)
        return first
    first, _ = sr.scan(b[mid - max_delay:mid + 1], min_run, -1)
    return -1 if first < 0 else max_delay - first


def test_analytic_crossing():
    a, o, unit = sr.crossing()
    M = sr.clearance_matrix(a, 161, unit, o, 161, unit)
    shifts = np.arange(-64, 65)
    tab = sr.table_fast(M, shifts, 15)
    np.testing.assert_array_equal(tab, sr.table_fast(M, shifts, 14))
    at = lambda s: tab[s + 64]
    assert at(0) == -1.0 and at(30) == at(-30) == -0.0625 and at(31) == at(-31) == at(32) == at(-32) == 0.0
    assert at(33) == at(-33) == 0.0625 and at(40) == at(-40) == pytest.approx(0.35355339059327373, abs=1e-15)
    np.testing.assert_array_equal(tab < 0.0, np.abs(shifts) <= 30)
    np.testing.assert_array_equal(tab < 0.25, np.abs(shifts) <= 37)
    assert int((tab < 0.0).sum()) == 61 and int((tab < 0.25).sum()) == 75
    for who in ("a", "o"):
        assert delay(tab, 0.0, who, 64) == 31 and delay(tab, 0.25, who, 64) == 38
        assert delay(tab, 0.0, who, 20) == -1 and delay(tab, 0.25, who, 20) == -1
