"""CPU: the exact families of tests/rollout_exact_cases.py bite, shown on the NumPy references alone.

tracking_ref, pursuit_ref, odometry_ref and rollout_clearance_ref's composition equal the exact checker (the header's steps in
fractions.Fraction) on every output of every case: floats bit for bit, integers equal, nothing excused.  (The sign of a zero is
the one thing left out here: a rational has none; test_gpu_rollout_exact.py holds the kernels to the references'.)  The numbers
the families were built for are asserted by hand, and switching one rule of the checker to its neighbour changes an output of
every family."""
import functools
import math

import numpy as np
import pytest

import rollout_exact_cases as xc

FAMILY_NAMES = tuple(xc.FAMILIES)
PI = math.pi


@functools.lru_cache(maxsize=None)
def checked(fam):
    """{case name: (reference, checker)} of a family, computed once."""
    return {name: (xc.reference(case), xc.exact(case)) for name, case in xc.family(fam).items()}


def ref_of(fam, name):
    return checked(fam)[name][0]


# ---- 1. the references are the header, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_reference_equals_the_exact_checker(fam):
    n = 0
    for name, (ref, ex) in checked(fam).items():
        case = xc.family(fam)[name]
        d = xc.same(ex, ref, xc.keys_of(case), zero_sign=False)
        assert d is None, (name, d)
        n += ref["stats"].shape[0] * ref["stats"].shape[1]
    print(f"ROLLOUT EXACT {fam}: {len(checked(fam))} cases, {n} rollouts equal the checker in every bit and every integer")
    assert n > 0


# ---- 2. the numbers the families were built for, by hand ------------------------------------------------------------------------
def test_wrap_by_hand():
    for kind in ("ramsete", "odometry", "pursuit"):
        ref = ref_of("wrap", f"wrap {kind}")
        head = ref["rows"][:, :8, 4]
        assert (np.abs(head) <= PI).all() and (head == head[:, :1]).all(), kind
        h = dict(zip(xc.WRAP_DPHI, head[:, 0]))
        # wrap(pi) = wrap(-pi) = -pi: the heading column is +pi for both; 2 pi and 0 give 0; 3 pi lands on the double beside pi
        assert h[PI] == PI and h[-PI] == PI and h[2 * PI] == 0.0 and h[0.0] == 0.0, kind
        assert abs(abs(h[3 * PI]) - PI) < 1e-15 and abs(abs(h[-3 * PI]) - PI) < 1e-15
        assert abs(h[5.5] - (2 * PI - 5.5)) < 1e-15 and abs(h[-7.25] - (7.25 - 2 * PI)) < 1e-15
        assert abs(h[1e6] + math.remainder(1e6, 2 * PI)) < 1e-9 and abs(h[-1e6] - math.remainder(1e6, 2 * PI)) < 1e-9
        if kind != "pursuit":
            # e_phi = wrap(0 - dphi) and the heading -wrap(dphi) round apart, and both sit at pi for dphi = +-pi
            assert (np.abs(ref["stats"][0, :, 2] - np.abs(head[:, 0])) < 1e-9).all() and (ref["stats"][0, :, 4] == ref["stats"][0, :, 2]).all()
            assert (ref["stats"][0, :, [0, 1, 3]] == 0.0).all()
    a, b = ref_of("wrap", "wrap ramsete"), ref_of("wrap", "wrap odometry")
    assert xc.same(a, dict(b, stats=b["stats"][..., :6] * [1, 1, 1, 1, 1, 0], stat_rows=b["stat_rows"][..., :2]),
                   ("stats", "stat_rows", "rows", "counts") + xc.SUMMARY) is None
    assert (b["stats"][0, :, 6] == b["stats"][0, :, 2]).all()                   # the estimate's heading stays the plan's


def test_first_stays_by_hand():
    for kind in ("ramsete", "odometry", "pursuit"):
        ref = ref_of("first", f"first K5 {kind}")
        assert (ref["stat_rows"][..., 0] == 0).all() and (ref["stats"][0, :, 0] == [0.25, 0.5, 0.5, 0.25, 0.5]).all(), kind
        assert (ref["worst"][0], ref["worst_rollout"][0], ref["worst_row"][0], ref["n_exceeding"][0]) == (0.5, 1, 0, 3), kind
        assert ref["mean"][0] == (((0.25 + 0.5) + 0.5) + 0.25 + 0.5) / 5
        assert ref_of("first", f"first K5 below {kind}")["n_exceeding"][0] == 5
        wide = ref_of("first", f"first K3 B87 {kind}")
        assert (wide["worst_rollout"] == np.arange(87) % 2).all() and (wide["stat_rows"][..., 0] == 0).all()
        assert (wide["n_exceeding"] == 2 * (np.arange(87) % 2)).all()
        assert ref_of("first", f"first K256 {kind}")["worst_rollout"].tolist() == [0, 200]
        assert ref_of("first", f"first K257 {kind}")["worst_rollout"].tolist() == [255]
        assert ref_of("first", f"first K300 {kind}")["worst_rollout"].tolist() == [255, 256]
    assert (ref_of("first", "first K5 pursuit")["n_unfinished"] == 5).all()


def test_the_means_are_ascending_sums_by_hand():
    """max e_pos = (1, 2^-53 four times, 0 elsewhere): 1 + 2^-53 is a tie and rounds to 1 every time, so the ascending sum is 1
    and the mean 1 / K; descending, pairwise or by blocks of 256 the four small terms meet first and the sum is above 1."""
    for kind in ("ramsete", "odometry", "pursuit"):
        for K, small in xc.MEAN_SMALL.items():
            ref = ref_of("first", f"first mean K{K} {kind}")
            e = ref["stats"][0, :, 0]
            assert e[0] == 1.0 and (e[list(small)] == xc.EPS).all() and np.count_nonzero(e) == 5
            assert ref["mean"][0] == 1.0 / K and (4 * xc.EPS + 1.0) / K != 1.0 / K, (kind, K)
            assert (ref["worst_rollout"][0], ref["n_exceeding"][0]) == (0, 1)
    for kind in ("ramsete", "pursuit"):
        for K in (5, 300):
            ref = ref_of("clear", f"clear mean K{K} {kind}")
            c = ref["clearance"][0]
            assert c[0] == 1.0 and (c[1:] == xc.EPS).all()
            assert ref["mean_clearance"][0] == 1.0 / K and ((K - 1) * xc.EPS + 1.0) / K != 1.0 / K
            assert (ref["worst_clearance"][0], ref["worst_clear_rollout"][0], ref["n_colliding"][0]) == (xc.EPS, 1, K - 1)


def test_drive_thresholds_by_hand():
    for kind in ("ramsete", "odometry"):
        assert ref_of("drive", f"drive at {kind}")["stat_rows"][0, 0, 1] == 0
        assert ref_of("drive", f"drive below {kind}")["stat_rows"][0, 0, 1] == 2          # both live rows, no settle row
        half = ref_of("drive", f"drive half {kind}")
        assert half["stat_rows"][0, 0, 1] == 1 and half["rows"][0, 1, 2] == 1.0 and half["rows"][0, 1, 6] == 0.0625   # scale 1/2
    at, below, half = (ref_of("drive", f"drive {n} pursuit") for n in ("at", "below", "half"))
    # at the limit the robot is 1/8 ft from the end at step 4 and has arrived; at the double below it is short of that by 2^-54
    assert at["stat_rows"][0, 0].tolist() == [0, 0, 4, 4] and below["stat_rows"][0, 0, 1:3].tolist() == [5, 5]
    assert (below["rows"][0, 1:6, 2] == xc.dn(2.0)).all()
    assert half["stat_rows"][0, 0, 1:3].tolist() == [8, 8] and (half["rows"][0, 1:9, 2] == 1.0).all()
    assert ref_of("drive", "drive min_speed pursuit")["stat_rows"][0, 0].tolist() == [0, 0, 4, 4]


def test_contraction_by_hand():
    """RAMSETE halves an offset every live row: e_pos at row r is |offset| 2^-r while x still holds it (40 rows here)."""
    for settle in (0, 10):
        case = xc.family("contraction")[f"contraction settle {settle} ramsete"]
        ref = ref_of("contraction", f"contraction settle {settle} ramsete")
        K = case["P"].shape[1]
        assert (ref["stat_rows"][..., 0] == 0).all() and (ref["stats"][..., 0] == np.abs(case["P"][..., 0])).all()
        for b, n in enumerate(xc.TILE_ROWS):
            live = min(n, 40)
            e = np.abs(case["rows"][b, :live, 6][None, :] - ref["rows"][b * K:(b + 1) * K, :live, 6])
            assert (e == np.abs(case["P"][b, :, :1]) * 0.5 ** np.arange(live)[None, :]).all(), (settle, n)
            assert (ref["counts"][b * K:(b + 1) * K] == n + settle).all()
        if settle == 0:                          # one row: the robot drives 1/8 ft on and half its offset back, the plan stands still
            assert (ref["stats"][0, :, 3] == np.abs(case["P"][0, :, 0] / 2 + 0.125)).all()
        # under odometry the follower sees the estimate, which has no offset: the true offset stays what it was.  The plan stops
        # on its last row and the robot one step (1/8 ft) later: a robot ahead of the plan is furthest off on the first settle row
        odo = ref_of("contraction", f"contraction settle {settle} odometry")
        ahead = (case["P"][..., 0] > 0) & (settle > 0)
        assert (odo["stat_rows"][..., 0] == np.where(ahead, np.array(xc.TILE_ROWS)[:, None], 0)).all()
        assert (odo["stats"][..., 7] == np.abs(case["P"][..., 0])).all()
        assert (odo["stats"][..., 0] == np.abs(case["P"][..., 0] + np.where(ahead, 0.125, 0.0))).all()


def test_validity_by_hand():
    case = xc.family("validity")["validity ramsete"]
    P = case["P"][0]
    fin = np.isfinite(P).all(axis=1)
    want = fin & (P[:, 3] > 0) & (P[:, 4] > 0) & (P[:, 5] > 0) & (P[:, 6] >= 0)
    for kind, ok in (("ramsete", want), ("odometry", want), ("pursuit", want & (P[:, 7] >= 0))):
        ref = ref_of("validity", f"validity {kind}")
        assert ((ref["stat_rows"][0, :, 0] >= 0) == ok).all() and (ref["counts"] == np.where(ok, 7, 0)).all(), kind
        assert np.isnan(ref["stats"][0, ~ok]).all() and (ref["stat_rows"][0, ~ok] == -1).all()
        # a valid record that is the base record in all but a tiny or signed-zero slot gives the base record's outputs
        base = int(np.nonzero((P == xc.NOMINAL).all(axis=1))[0][0])
        like = ok & (P[:, :3] == 0).all(axis=1)
        cols = [0, 1, 2] if kind == "pursuit" else [0, 1, 2, 3, 4]
        assert like.sum() >= 40 and (ref["stats"][0, like][:, cols] == ref["stats"][0, base, cols]).all(), kind
        assert ref["worst_rollout"][0] == len(P) - 1 and ref["worst"][0] == 0.5          # the last record: dx = 1/2
    # 5e-324 is positive, -0.0 and 0.0 are not; tau = -0.0 and 5e-324 are valid, -5e-324 is not; slot 7 = -1 only bothers pure pursuit
    tiny = (P == xc.TINY).any(axis=1)
    assert tiny.sum() == 5 and want[tiny].all() and not want[(P[:, 3:6] == 0).any(axis=1)].any()
    assert not want[P[:, 6] == -xc.TINY].any() and want[(P[:, 6] == 0) & np.signbit(P[:, 6]) & fin & (P[:, 3:6] > 0).all(axis=1)].all()
    O = xc.family("validity")["validity odometry records"]["O"][0]
    ok = np.isfinite(O).all(axis=1) & (O[:, [0, 1, 2, 4]] > 0).all(axis=1)
    ref = ref_of("validity", "validity odometry records")
    assert ((ref["stat_rows"][0, :, 0] >= 0) == ok).all() and 20 < ok.sum() < len(O) - 20
    assert (ref["stats"][0, ok, 0] == 0.25).all() and ref["worst_rollout"][0] == int(np.argmax(ok))


def test_pointers_by_hand():
    """Records start the robot on vertex 0, 1, 2 and one step before vertex 0; it moves one vertex a step.  stat_rows = {step of
    max e_ct, saturated, arrived step, final ic}: arrival 1/8 ft (one vertex) before the end, ic the segment that starts there."""
    r = lambda name: ref_of("pointers", f"pointers {name}")["stat_rows"][0].tolist()
    assert r("vertices") == [[0, 0, 7, 7], [0, 0, 6, 7], [0, 0, 5, 7], [0, 0, 8, 7]]
    assert r("arrive below") == [[0, 0, 8, 7], [0, 0, 7, 7], [0, 0, 6, 7], [0, 0, 9, 7]]          # on the last vertex: at_end
    assert r("repeats mid") == [[0, 0, 7, 10], [0, 0, 6, 10], [0, 0, 5, 10], [0, 0, 8, 10]]
    assert r("repeats end") == [[0, 0, 7, 7], [0, 0, 6, 7], [0, 0, 5, 7], [0, 0, 8, 7]]
    assert r("n1") == [[0, 0, 0, 0]] * 4                                           # one point: at_end at once, ic stays 0
    assert r("n2") == [[0, 0, 0, 0]] * 3 + [[0, 0, 1, 0]]
    assert ref_of("pointers", "pointers vertices")["stats"][0, :, 1].tolist() == [0.125] * 4          # it stops where it arrived
    assert ref_of("pointers", "pointers arrive below")["stats"][0, :, 1].tolist() == [0.0] * 4


def test_gate_by_hand():
    """Offsets 1/4, -1/2, 0, -1/4 against a gate of 1/4 ft; 12 rows.  stat_rows columns 2, 3 = resets accepted, rejected."""
    ar = lambda name: ref_of("gate", f"gate {name}")["stat_rows"][0, :, 2:].tolist()
    assert ar("at") == [[12, 0], [0, 12], [12, 0], [12, 0]]
    assert ar("below") == [[0, 12], [0, 12], [12, 0], [0, 12]]
    assert ar("half gain") == [[12, 0], [0, 12], [12, 0], [12, 0]]
    assert ar("every 5") == [[3, 0], [0, 3], [3, 0], [3, 0]]                      # rows 0, 5 and 10: the last two are settle rows
    assert ar("half gain every 5") == [[3, 0]] * 4
    assert ar("window") == [[12, 0], [0, 0], [0, 0], [0, 0]]                      # only dx = 1/4 reads 3.75
    est = ref_of("gate", "gate every 5")["est_rows"]
    assert (est[0, :12, 3] == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]).all() and (est[1, :12, 3] == 0).all()
    assert (est[0, :12, 1] == 2.25).all() and (est[1, :12, 1] == 2.0).all()      # gain 1: the estimate is on the truth at once
    half = ref_of("gate", "gate half gain")["est_rows"]
    assert (half[0, :6, 1] == 2.25 - 0.25 * 0.5 ** np.arange(1, 7)).all()
    slow = ref_of("gate", "gate half gain every 5")["est_rows"]
    assert (slow[1, :12, 1] == [1.75] * 5 + [1.625] * 5 + [1.5625] * 2).all()


def test_clearance_fold_by_hand():
    for kind in ("ramsete", "pursuit"):
        at, above = ref_of("clear", f"clear small at {kind}"), ref_of("clear", f"clear small above {kind}")
        # route 0's records: 1/4 (a tie of both walls: element 0), 1/4, 1/8 at the left wall (element 1), 1/8 at the right
        assert at["clearance"][0].tolist() == [0.25, 0.25, 0.125, 0.125] and at["clear_rows"][0].tolist() == \
            [[0, 0, -1, 0], [0, 0, -1, 0], [0, 1, 0, 8], [0, 0, 0, 8]], kind
        assert above["clear_rows"][0].tolist() == [[0, 0, 0, 8], [0, 0, 0, 8], [0, 1, 0, 8], [0, 0, 0, 8]]
        assert (at["worst_clearance"] == 0.125).all() and at["worst_clear_rollout"].tolist() == [2, 0, 0]        # the records roll by b
        assert at["worst_clear_element"].tolist() == [1, 0, 1] and (at["worst_clear_row"] == 0).all()
        assert (at["n_colliding"] == 2).all() and (above["n_colliding"] == 4).all() and (at["n_clear_valid"] == 4).all()
        assert (at["mean_clearance"] == 0.1875).all()
        for name, K in (("K300", 300), ("lanes", 256)):
            big = ref_of("clear", f"clear {name} at {kind}")
            B = len(big["worst_clearance"])
            assert big["worst_clear_rollout"].tolist() == [[2, 0, 0][b % 3] for b in range(B)] and (big["n_colliding"] == K // 2).all()
            assert (big["n_clear_valid"] == K).all() and (big["clear_rows"][..., 0] == 0).all()


# ---- 3. a switched rule changes an output ------------------------------------------------------------------------------------------
SWITCHES = (("wrap_low", "wrap", "wrap ramsete"), ("wrap_low", "wrap", "wrap odometry"), ("wrap_low", "wrap", "wrap pursuit"),
            ("max_first", "first", "first K5 ramsete"), ("max_first", "first", "first K5 odometry"), ("max_first", "first", "first K5 pursuit"),
            ("worst_first", "first", "first K5 ramsete"), ("worst_first", "first", "first K3 B87 pursuit"),
            ("worst_first", "first", "first K256 odometry"), ("worst_first", "first", "first K257 ramsete"),
            ("worst_first", "first", "first K300 pursuit"), ("exceed_strict", "first", "first K5 ramsete"),
            ("exceed_strict", "first", "first K3 B87 odometry"),
            ("mean_ascending", "first", "first mean K5 ramsete"), ("mean_ascending", "first", "first mean K256 odometry"),
            ("mean_ascending", "first", "first mean K300 pursuit"), ("mean_ascending", "first", "first mean K300 ramsete"),
            ("mean_ascending", "clear", "clear mean K5 ramsete"), ("mean_ascending", "clear", "clear mean K300 pursuit"),
            ("below_strict", "clear", "clear K300 at ramsete"), ("below_strict", "clear", "clear lanes at pursuit"),
            ("sat_strict", "drive", "drive at ramsete"), ("sat_strict", "drive", "drive at odometry"), ("sat_strict", "drive", "drive at pursuit"),
            ("max_first", "contraction", "contraction settle 10 odometry"), ("max_first", "contraction", "contraction settle 10 pursuit"),
            ("worst_first", "contraction", "contraction settle 0 ramsete"),
            ("gain_strict", "validity", "validity ramsete"), ("tau_inclusive", "validity", "validity pursuit"),
            ("slot7_inclusive", "validity", "validity pursuit"), ("gain_strict", "validity", "validity odometry records"),
            ("closest_tie", "pointers", "pointers vertices"), ("closest_tie", "pointers", "pointers repeats mid"),
            ("arrive_inclusive", "pointers", "pointers vertices"), ("arrive_inclusive", "pointers", "pointers repeats end"),
            ("gate_inclusive", "gate", "gate at"), ("min_cos_inclusive", "gate", "gate at"), ("near_strict", "gate", "gate window"),
            ("far_strict", "gate", "gate window"), ("gate_inclusive", "gate", "gate every 5"),
            ("clear_first", "clear", "clear small at ramsete"), ("below_strict", "clear", "clear small at pursuit"),
            ("clear_worst_first", "clear", "clear small at ramsete"), ("element_first", "clear", "clear small at pursuit"),
            ("clear_worst_first", "clear", "clear K300 at ramsete"), ("clear_first", "clear", "clear lanes at pursuit"))


@pytest.mark.parametrize("rule,fam,name", SWITCHES)
def test_a_switched_rule_changes_an_output(rule, fam, name):
    case = xc.family(fam)[name]
    _, ex = checked(fam)[name]
    flipped = xc.exact(case, **{rule: False})
    assert xc.same(ex, flipped, xc.keys_of(case), zero_sign=False) is not None, (rule, name)


def test_every_family_and_every_rule_is_switched():
    assert {fam for _, fam, _ in SWITCHES} == set(FAMILY_NAMES)
    assert {rule for rule, _, _ in SWITCHES} == set(xc.RULES)
    for _, fam, name in SWITCHES:
        assert name in xc.family(fam)
