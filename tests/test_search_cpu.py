"""CPU: the NumPy reference of the route search (tests/search_ref.py) against known answers and the definitions of
include/vap.h, and two search scenarios through the reference loop (the CPU oracle's generate_motion_profile and
tests/footprint_ref.py as the evaluation).  Also that the product exposes the two entry points and the Python surface.

Scenarios (an 18 x 18 in robot, a field of +-6 ft, default constraints, W = 5, pinned ends, sigma0 = 0.5 ft, N = 64, E = 8,
alpha = 0.7, 12 iterations):
  A  no obstacle, a zigzag seed.  The straight line has zero curvature and the shortest length, so its cost through the
     same pipeline is the lower bound: the search must close >= 90 % of the gap between the seed's cost and it
     (measured: 4.2705 s -> 2.4880 s against 2.4780 s, 99.4 %).
  B  a straight seed through a circle of radius 0.5 ft at the origin, margin 0.1 ft: the best route must be feasible
     (measured: feasible from the third iteration, 2.7885 s after 12).
Both need a non-increasing history."""
import numpy as np
import pytest

import search_ref as sr

FIELD = (-6.0, -6.0, 6.0, 6.0)
SEED_A = np.array([[-4, 0], [-2, 1], [0, -1], [2, 1], [4, 0]], dtype=np.float64)
LINE = np.array([[-4, 0], [-2, 0], [0, 0], [2, 0], [4, 0]], dtype=np.float64)
CIRCLE_B = (0.0, 0.0, 0.5)
MARGIN_B = 0.1


def sigma0(R=1, W=5, s=0.5):
    sg = np.full((R, W, 2), s)
    sg[:, 0] = sg[:, -1] = 0.0
    return sg


def foot():
    from vexautonomousplanner_amd import footprint as fp
    return fp.rectangle(18, 18)


def constraints():
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    return DEFAULT_CONSTRAINTS


def hexes(c):
    return " ".join("%08x" % int(np.asarray(v).reshape(-1)[0]) for v in c)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert hexes(sr.philox4x32_10(counter, key)) == want


def test_product_declares_the_search_calls():
    from vexautonomousplanner_amd import _lib, search
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    L = _lib.lib()
    assert "vap_search_sample" in _lib.EXPORTS and "vap_search_update" in _lib.EXPORTS
    assert hasattr(L, "vap_search_sample") and hasattr(L, "vap_search_update")
    assert callable(search.refine) and callable(search.rank) and callable(BatchedTrajectoryGenerator.refine)
    w = search.Weights()
    assert (w.w_time, w.w_length, w.w_violation, w.infeasible_base, w.clearance_margin, w.conflict_margin,
            w.tracking_tolerance) == (1.0, 1e-3, 1e3, 1e6, 0.05, 0.05, 0.25)
    assert {k: getattr(w, k) for k in sr.WEIGHTS} == sr.WEIGHTS
    with pytest.raises(ValueError):
        search.SearchConfig(candidates=4097).validate()
    with pytest.raises(ValueError):
        search.SearchConfig(candidates=8, elites=9).validate()


def test_entry_points_check_their_arguments_before_the_device():
    """N outside 1..4096, W outside 2..2048 and a bad weight are refused by value, without a device."""
    import ctypes as C
    from vexautonomousplanner_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)
    sample = lambda N, W: L.vap_search_sample(None, _lib.VAP_F64, 1, N, W, one, one, None, None, 0, 0, 0, one)
    assert sample(0, 5) == _lib.VAP_ERR_INVALID and sample(4097, 5) == _lib.VAP_ERR_INVALID
    assert sample(8, 1) == _lib.VAP_ERR_INVALID and sample(8, 2049) == _lib.VAP_ERR_UNSUPPORTED
    ws = _lib.SearchWeights(1.0, 1e-3, 1e3, 1e6, 0.05, 0.05, 0.25)
    upd = lambda N, E, w: L.vap_search_update(None, _lib.VAP_F64, 1, N, 5, one, None, 1, 0.01, None, None, None, None, None,
                                              C.byref(w), E, 0.7, 0.0, 1.0, one, one, None, None, None, None, None, None, None,
                                              None, 0, 0)
    assert upd(4097, 1, ws) == _lib.VAP_ERR_INVALID and upd(8, 9, ws) == _lib.VAP_ERR_INVALID and upd(8, 0, ws) == _lib.VAP_ERR_INVALID
    assert upd(8, 4, _lib.SearchWeights(-1.0, 0, 0, 0, 0, 0, 0)) == _lib.VAP_ERR_INVALID


def test_sampler_elitism_and_pins():
    rng = np.random.default_rng(1)
    R, N, W = 3, 16, 6
    mean = rng.uniform(-5, 5, (R, W, 2))
    sigma = rng.uniform(0.1, 1.0, (R, W, 2))
    sigma[:, 0] = sigma[:, -1] = 0.0
    sigma[1, 2, 1] = 0.0
    best = rng.uniform(-5, 5, (R, W, 2)).astype(np.float32)
    best_cost = np.array([3.5, np.inf, np.nan])
    for dt in (np.float32, np.float64):
        wp = sr.sample(mean, sigma, N, dt, seed=7, iteration=2, best_wp=best.astype(dt), best_cost=best_cost)
        assert wp.dtype == dt and wp.shape == (R, N, W, 2)
        assert np.array_equal(wp[0, 0], best[0].astype(dt))                         # the best so far
        assert np.array_equal(wp[1, 0], mean[1].astype(dt)) and np.array_equal(wp[2, 0], mean[2].astype(dt))
        pinned = np.broadcast_to(sigma[:, None] == 0, wp.shape)
        assert np.array_equal(wp[:, 1:][pinned[:, 1:]], np.broadcast_to(mean[:, None].astype(dt), wp.shape)[:, 1:][pinned[:, 1:]])
        assert (wp[:, 1:][~pinned[:, 1:]] != np.broadcast_to(mean[:, None].astype(dt), wp.shape)[:, 1:][~pinned[:, 1:]]).all()
    # a candidate depends on (seed, iteration, problem, n, w) only
    a = sr.sample(mean, sigma, 8, np.float64, seed=7, iteration=2)
    b = sr.sample(mean, sigma, N, np.float64, seed=7, iteration=2)
    assert np.array_equal(a, b[:, :8])
    c = sr.sample(mean[2:], sigma[2:], N, np.float64, seed=7, iteration=2, first_problem=2)
    assert np.array_equal(c[0], b[2])
    assert not np.array_equal(sr.sample(mean, sigma, N, np.float64, seed=8, iteration=2)[:, 1:], b[:, 1:])
    assert not np.array_equal(sr.sample(mean, sigma, N, np.float64, seed=7, iteration=3)[:, 1:], b[:, 1:])
    # the normals are standard normal
    z = sr.normals(4096, 32, 11, 0, 0)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and np.isfinite(z).all()


def planted_terms(N):
    """Terms with exact ties, NaN, inf and flagged candidates planted."""
    rng = np.random.default_rng(5)
    t = {"counts": rng.integers(200, 400, N), "length": rng.uniform(5, 12, N), "flags": np.zeros(N, dtype=np.int64),
         "clearance": rng.uniform(-0.2, 1.0, N)}
    t["counts"][[3, 9, 20]] = 250
    t["length"][[3, 9, 20]] = 8.0
    t["clearance"][[3, 9, 20]] = 0.5          # an exact three-way tie among feasible candidates
    t["clearance"][[4, 11]] = -0.125
    t["counts"][[4, 11]] = 300
    t["length"][[4, 11]] = 9.0                # an exact tie among infeasible ones
    t["clearance"][5] = np.nan
    t["length"][6] = np.nan
    t["length"][7] = np.inf
    t["flags"][8] = 2
    t["counts"][10] = 0
    t["clearance"][12] = np.inf
    t["clearance"][13] = -np.inf
    return t


def test_order_ties_and_infinite_costs():
    N = 32
    t = planted_terms(N)
    wp = np.random.default_rng(2).uniform(-5, 5, (1, N, 4, 2))
    u = sr.update(wp, sr.WEIGHTS, **t)
    c, v, order = u["cost"], u["violation"], u["order"][0]
    assert np.isinf(c[[5, 6, 7, 8, 10, 13]]).all() and np.isnan(v[5]) and np.isfinite(c[12]) and v[12] == 0
    assert c[3] == c[9] == c[20] and c[4] == c[11]
    pos = {int(i): k for k, i in enumerate(order)}
    assert pos[3] + 1 == pos[9] and pos[9] + 1 == pos[20] and pos[4] + 1 == pos[11]      # ties by index
    assert sorted(order[-6:].tolist()) == [5, 6, 7, 8, 10, 13] and order[-6:].tolist() == [5, 6, 7, 8, 10, 13]
    assert (np.diff(c[order[:-6]]) >= 0).all() and np.isfinite(c[order[:-6]]).all()
    feas = np.isfinite(c) & (v == 0)
    assert u["n_feasible"][0] == feas.sum()
    # any feasible candidate beats any infeasible one; among infeasible ones the smaller violation wins
    k = int(feas.sum())
    assert feas[order[:k]].all() and not feas[order[k:]].any()
    inf_fin = [i for i in order[k:] if np.isfinite(c[i])]
    assert (np.diff(v[inf_fin]) >= 0).all()


def test_best_so_far_is_replaced_only_by_a_strictly_lower_cost():
    N, W = 8, 3
    wp = np.random.default_rng(3).uniform(-5, 5, (1, N, W, 2))
    t = {"counts": np.full(N, 300), "length": np.full(N, 8.0)}
    t["counts"][5] = 250
    c_top = sr.costs(sr.WEIGHTS, **t)[0][5]
    prev_wp, prev_terms = np.zeros((1, W, 2)), np.full((1, 4), -1.0)
    for prev, replaced in ((np.inf, True), (c_top + 1e-9, True), (c_top, False), (c_top - 1e-9, False), (np.nan, False)):
        u = sr.update(wp, sr.WEIGHTS, best_cost=np.array([prev]), best_wp=prev_wp, best_terms=prev_terms, **t)
        if replaced:
            assert u["best_cost"][0] == c_top and np.array_equal(u["best_wp"][0], wp[0, 5])
            assert u["best_terms"][0].tolist() == [2.5, 8.0, 0.0, 5.0]
        else:
            assert np.array_equal(u["best_cost"], np.array([prev]), equal_nan=True)
            assert np.array_equal(u["best_wp"], prev_wp) and np.array_equal(u["best_terms"], prev_terms)
    # nothing finite: nothing replaced
    u = sr.update(wp, sr.WEIGHTS, best_cost=np.array([np.inf]), best_wp=prev_wp, best_terms=prev_terms, counts=np.zeros(N, dtype=int))
    assert np.isinf(u["best_cost"][0]) and np.array_equal(u["best_wp"], prev_wp)


def test_refit_keeps_its_bits_without_a_finite_candidate_and_clamps_sigma():
    rng = np.random.default_rng(4)
    N, W = 16, 4
    wp = rng.uniform(-5, 5, (1, N, W, 2))
    mean, sigma = rng.uniform(-5, 5, (1, W, 2)), rng.uniform(0.1, 1, (1, W, 2))
    sigma[0, 0] = 0.0
    u = sr.update(wp, sr.WEIGHTS, 4, 0.7, 1e-3, 2.0, mean, sigma, flags=np.ones(N, dtype=int))
    assert np.array_equal(u["mean"].view(np.int64), mean.view(np.int64)) and np.array_equal(u["sigma"].view(np.int64), sigma.view(np.int64))
    assert len(u["elites"][0]) == 0
    t = {"counts": rng.integers(200, 400, N)}
    # fewer finite candidates than E: the elites are those
    fl = np.ones(N, dtype=int)
    fl[[2, 7]] = 0
    u = sr.update(wp, sr.WEIGHTS, 4, 0.7, 1e-3, 2.0, mean, sigma, flags=fl, **t)
    assert sorted(u["elites"][0].tolist()) == [2, 7]
    # the clamp, both ways; a pinned coordinate keeps mean and sigma
    wide = sr.update(wp, sr.WEIGHTS, 4, 1.0, 1e-3, 0.25, mean, sigma, **t)
    assert (wide["sigma"][0, 1:] == 0.25).all()
    same = np.repeat(wp[:, :1], N, axis=1)
    tight = sr.update(same, sr.WEIGHTS, 4, 1.0, 1e-3, 2.0, mean, sigma, **t)
    assert (tight["sigma"][0, 1:] == 1e-3).all() and np.array_equal(tight["mean"][0, 1:], same[0, 0, 1:])
    for u in (wide, tight):
        assert (u["sigma"][0, 0] == 0).all() and np.array_equal(u["mean"][0, 0], mean[0, 0])
    # the refit itself: alpha-blend of the elites' mean and population variance
    u = sr.update(wp, sr.WEIGHTS, 4, 0.7, 0.0, np.inf, mean, sigma, **t)
    el = wp[0, u["elites"][0]]
    assert np.allclose(u["mean"][0, 1:], 0.3 * mean[0, 1:] + 0.7 * el.mean(axis=0)[1:], rtol=1e-14)
    assert np.allclose(u["sigma"][0, 1:], np.sqrt(0.3 * sigma[0, 1:] ** 2 + 0.7 * el.var(axis=0)[1:]), rtol=1e-14)
    ld = sr.update(wp, sr.WEIGHTS, 4, 0.7, 0.0, np.inf, mean, sigma, ftype=np.longdouble, **t)
    assert np.abs(ld["mean"] - u["mean"]).max() < 1e-14


@pytest.fixture(scope="module")
def scenario_a():
    ev = sr.oracle_evaluate(foot(), FIELD, constraints=constraints())
    ends = sr.costs(sr.WEIGHTS, **ev(np.stack([SEED_A, LINE])))[0]
    return sr.search(SEED_A[None], sigma0(), ev), ends


def test_scenario_a_closes_the_gap_to_the_straight_line(scenario_a):
    res, (c_seed, c_line) = scenario_a
    h = res["history"][0]
    share = (c_seed - res["best_cost"][0]) / (c_seed - c_line)
    print(f"scenario A: seed {c_seed:.4f} s -> {res['best_cost'][0]:.4f} s, straight line {c_line:.4f} s, share {share:.4f}")
    assert c_line < c_seed and h[0] <= c_seed
    assert (np.diff(h) <= 0).all()
    assert res["best_cost"][0] >= c_line - 1e-9
    assert share >= 0.9
    assert np.array_equal(res["best_wp"][0, [0, -1]], SEED_A[[0, -1]])


def test_scenario_b_leaves_the_collision():
    w = dict(sr.WEIGHTS, clearance_margin=MARGIN_B)
    ev = sr.oracle_evaluate(foot(), FIELD, circles=[CIRCLE_B], constraints=constraints())
    c_seed, v_seed = sr.costs(w, **ev(LINE[None]))[:2]
    assert v_seed[0] > 0 and c_seed[0] > 1e6                      # the seed collides
    res = sr.search(LINE[None], sigma0(), ev, weights=w)
    h = res["history"][0]
    first = int(np.argmax(h < 1e6))
    print(f"scenario B: seed {c_seed[0]:.1f} -> {res['best_cost'][0]:.4f} s, feasible from iteration {first}")
    assert (np.diff(h) <= 0).all()
    assert np.isfinite(res["best_cost"][0]) and res["best_terms"][0, 2] == 0.0
    # independently: the best route's own rows clear the circle by the margin
    again = ev(res["best_wp"])
    assert again["clearance"][0] >= MARGIN_B and again["flags"][0] == 0
    assert sr.costs(w, **again)[0][0] == res["best_cost"][0]
