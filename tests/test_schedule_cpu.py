"""CPU: the reference of the wait schedule (tests/schedule_ref.py) against itself, so that the GPU tests' cases bite.

solve (the recurrence) equals brute (every delay vector, the tie-break as a sort key); tables (instant by instant) equals
the composition of shift_ref.table_fast it is documented as; the known case has its stated numbers; the seeded family
holds routines without a schedule, with a free one and with a real wait."""
import numpy as np
import pytest

import schedule_cases as sc
import schedule_ref as ref
import shift_ref as sr


def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and (a[2] == b[2] or (a[2] != a[2] and b[2] != b[2]))


def test_solve_equals_brute_on_random_tables():
    cases = sc.random_tables(7, 2400)
    seen = {"none": 0, "zero": 0, "positive": 0}
    waited_late = 0
    for move, wait, S in cases:
        for q in (1, 3):
            got, want = ref.solve(move, wait, S, 0.0, q), ref.brute(move, wait, S, 0.0, q)
            assert same(got, want), (move, wait, S, q, got, want)
        if S:
            seen[sc.classify(got[1])] += 1
            waited_late += got[1] > 0 and got[0][0] < got[1]
    assert min(seen.values()) >= 200 and waited_late >= 50, (seen, waited_late)


def test_solve_edge_tables():
    nan = float("nan")
    # S = 0 and an empty window: no schedule, -1 in every slot
    assert ref.solve(np.full((3, 4), 0.5), np.full((3, 4), 0.5), 0, 0.0) == ([-1, -1, -1], -1, pytest.approx(nan, nan_ok=True))
    # NaN never blocks; unused slots get 0
    d, total, c = ref.solve(np.full((3, 4), nan), np.full((3, 4), nan), 2, 0.0)
    assert d == [0, 0, 0] and total == 0 and c != c
    # the tie-break: both slots may take the wait; the earlier one gets it
    move = np.array([[0.5, 0.5, 0.5], [-1.0, -1.0, 0.5]])
    wait = np.full((2, 3), 0.5)
    assert ref.solve(move, wait, 2, 0.0, 5)[:2] == ([10, 0], 10)
    # ... unless standing at the start is blocked: then it leaves at once and waits in front of slot 1
    wait[0, 1] = -1.0
    assert ref.solve(move, wait, 2, 0.0, 5)[:2] == ([5, 5], 10)
    wait[0, 0] = -1.0
    assert ref.solve(move, wait, 2, 0.0, 5) == ([0, 10], 10, 0.5)
    # an entry exactly at the margin is unblocked
    assert ref.solve(np.array([[0.25]]), np.array([[0.0]]), 1, 0.25) == ([0], 0, 0.25)


def composed(rows_a, n, seg, foot_a, rows_o, counts_o, foot_o, C, q, mats, key):
    ms = [mats[(key, p)] for p in range(len(rows_o)) if (key, p) in mats]

    def table_of(lo, hi, shifts, hold):
        out = np.full(len(shifts), np.nan)
        for Mx in ms:
            out = np.fmin(out, sr.table_fast(Mx[lo:hi], shifts, hold))
        return out
    return ref.composed_tables(table_of, n, seg, C, q)


_FAMILY = {}


def family_reference(seed):
    """The family's rows and, per routine, (move, wait, S, bad, solve); computed once per seed."""
    if seed not in _FAMILY:
        rows_a, counts_a, seg, rows_o, counts_o = case = sc.family(seed)
        mats, per = {}, []
        for r in range(sc.R):
            mv, wt, S, bad = ref.tables(rows_a[r], counts_a[r], seg[r], sc.FOOT, rows_o, counts_o, sc.FOOT, sc.FAMILY_C, sc.FAMILY_Q,
                                        matrices=mats, key=r)
            per.append((mv, wt, S, bad, ref.solve(mv, wt, S, sc.FAMILY_MARGIN, sc.FAMILY_Q)))
        _FAMILY[seed] = (case, per, mats)
    return _FAMILY[seed]


@pytest.mark.parametrize("seed", [0, 3])
def test_tables_equal_the_shift_table_composition(seed):
    (rows_a, counts_a, seg, rows_o, counts_o), per, mats = family_reference(seed)
    for r in range(sc.R):
        mv, wt, S, _ = composed(rows_a[r], int(counts_a[r]), seg[r], sc.FOOT, rows_o, counts_o, sc.FOOT, sc.FAMILY_C, sc.FAMILY_Q, mats, r)
        np.testing.assert_array_equal(mv, per[r][0])
        np.testing.assert_array_equal(wt, per[r][1])
        assert S == per[r][2] >= 1


def test_known_case():
    a, seg, o, co = sc.known()
    for q in (1, 2, 4):
        C = sc.KNOWN_WINDOW // q
        for sel, want in (([0], sc.KNOWN_ONE), ([0, 1], sc.KNOWN_BOTH)):
            mv, wt, S, bad = ref.tables(a[0], 161, seg[0], sc.UNIT, o[sel], co[sel], sc.UNIT, C, q)
            assert S == 2 and not bad
            d, total, c = ref.solve(mv, wt, S, sc.KNOWN_MARGIN, q)
            assert d == want[q] and total == sum(want[q]), (q, sel, d)
            if len(sel) == 2:
                assert c == sc.KNOWN_BOTH_CLEARANCE
            # nothing is near a decision
            assert min(np.nanmin(np.abs(mv - sc.KNOWN_MARGIN)), np.nanmin(np.abs(wt - sc.KNOWN_MARGIN))) >= 1.0 / 32.0
            if C <= 12:
                assert same(ref.brute(mv, wt, S, sc.KNOWN_MARGIN, q), (d, total, c))


def test_family_holds_every_class():
    seen = {"none": 0, "zero": 0, "positive": 0}
    near = 0
    for seed in sc.FAMILY_SEEDS:
        _, per, _ = family_reference(seed)
        for mv, wt, S, bad, (d, total, c) in per:
            assert S >= 1 and not bad
            seen[sc.classify(total)] += 1
            with np.errstate(invalid="ignore"):
                near += int((np.abs(mv - sc.FAMILY_MARGIN) <= 1e-9).sum() + (np.abs(wt - sc.FAMILY_MARGIN) <= 1e-9).sum())
    assert min(seen.values()) >= 4, seen
    assert near == 0


def test_segment_lists():
    assert ref.segments([0, 5, -1], 10) == (2, [0, 5, 10], False)
    assert ref.segments([-1, -1], 10) == (0, [], False) and ref.segments([0, 5], 0) == (0, [], False)
    for seg in ([1, 5], [0, 5, 5], [0, 7, 5], [0, 10], [0, -1, 5], [-1, 0]):
        assert ref.segments(seg, 10) == (0, [], True), seg
