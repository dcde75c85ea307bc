"""GPU: the route search (vap_search_sample, vap_search_update, search.refine, BatchedTrajectoryGenerator.refine) against
the NumPy reference of tests/search_ref.py and, end to end, against the conditions of tests/test_search_cpu.py.

Tolerances.  Candidate 0 and pinned coordinates are copies: bit for bit.  A sampled fp64 coordinate must lie within
max(1e-13, 8 D) of the float64 reference, D = |float64 - longdouble| of the reference (the convention of
tests/test_gpu_tracking.py: the device's log / sincos are within an ulp or two of NumPy's); an fp32 coordinate within one
fp32 ulp (the fp64 value is rounded once).  The cost is a handful of IEEE operations in the header's order: 4 ulp.  Order,
elites, n_feasible and the best candidate are exact; the refitted mean and sigma within max(1e-13, 8 D).

End to end, scenarios A and B of test_search_cpu.py run on the device (dd = 0.005 ft, dt = 0.01 s, the oracle's grid) with
N = 64 and N = 4096 under the same conditions: A closes >= 90 % of the gap between the seed's cost and the straight line's,
both through the same device pipeline; B ends feasible; both histories are non-increasing."""
import os
import sys

import numpy as np
import pytest

import footprint_ref as fr
import search_ref as sr

pytestmark = pytest.mark.gpu

FLOOR, FACTOR = 1e-13, 8.0
FIELD = (-6.0, -6.0, 6.0, 6.0)
SEED_A = np.array([[-4, 0], [-2, 1], [0, -1], [2, 1], [4, 0]], dtype=np.float64)
LINE = np.array([[-4, 0], [-2, 0], [0, 0], [2, 0], [4, 0]], dtype=np.float64)
CIRCLE_B = (0.0, 0.0, 0.5)
MARGIN_B = 0.1
DD, DT, CAP_S, CAP_ROWS = 0.005, 0.01, 4096, 1024


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def S():
    from vexautonomousplanner_amd import search
    return search


def FP():
    from vexautonomousplanner_amd import footprint
    return footprint


_gens = {}


def generator(dtype="f32"):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    if dtype not in _gens:
        _gens[dtype] = BatchedTrajectoryGenerator(0, dtype)
    return _gens[dtype]


def np_dt(torch, tdt):
    return np.float32 if tdt == torch.float32 else np.float64


def bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view({4: np.int32, 8: np.int64, 1: np.int8}[a.dtype.itemsize]) if a.dtype != np.bool_ else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- sampler

def sampler_case(torch, dt):
    rng = np.random.default_rng(1)
    R, N, W = 3, 300, 7                      # 6300 threads: 25 workgroups, the last one partly idle
    mean = rng.uniform(-5, 5, (R, W, 2))
    sigma = rng.uniform(0.05, 1.0, (R, W, 2))
    sigma[:, 0] = sigma[:, -1] = 0.0
    sigma[1, 3, 1] = 0.0
    best = rng.uniform(-5, 5, (R, W, 2)).astype(dt)
    best_cost = np.array([3.5, np.inf, np.nan])
    return R, N, W, mean, sigma, best, best_cost


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sampler_matches_reference(torch_mod, dtype):
    torch = torch_mod
    tdt = torch.float64 if dtype == "f64" else torch.float32
    dt = np_dt(torch, tdt)
    R, N, W, mean, sigma, best, best_cost = sampler_case(torch, dt)
    dev = torch.device("cuda", 0)
    got = S().sample(torch.tensor(mean, device=dev), torch.tensor(sigma, device=dev), N, dtype=tdt, seed=0x123456789ABCDEF,
                     iteration=3, first_problem=5, best_waypoints=torch.tensor(best, device=dev),
                     best_cost=torch.tensor(best_cost, device=dev))
    assert got.dtype == tdt and tuple(got.shape) == (R * N, W, 2)
    g = got.cpu().numpy().reshape(R, N, W, 2)
    kw = dict(seed=0x123456789ABCDEF, iteration=3, first_problem=5, best_wp=best, best_cost=best_cost)
    r64 = sr.sample(mean, sigma, N, np.float64, **kw)
    rld = sr.sample(mean, sigma, N, dt, ftype=np.longdouble, **kw)
    ref = r64.astype(dt)
    # candidate 0: the best so far where its cost is finite, else the mean; pinned coordinates: the mean
    assert np.array_equal(g[0, 0].view(np.uint8), best[0].view(np.uint8))
    assert np.array_equal(g[1:, 0].view(np.uint8), mean[1:].astype(dt).view(np.uint8))
    pinned = np.broadcast_to(sigma[:, None] == 0, g.shape)[:, 1:]
    want_pin = np.broadcast_to(mean[:, None].astype(dt), g.shape)[:, 1:]
    assert np.array_equal(g[:, 1:][pinned], want_pin[pinned])
    free_g, free_r = g[:, 1:][~pinned].astype(np.float64), ref[:, 1:][~pinned].astype(np.float64)
    D = np.abs(r64[:, 1:][~pinned].astype(np.longdouble) - rld[:, 1:][~pinned]).astype(np.float64)
    diff = np.abs(free_g - free_r)
    if dtype == "f64":
        tol = np.maximum(FLOOR, FACTOR * D)
    else:
        tol = np.spacing(np.abs(ref[:, 1:][~pinned])).astype(np.float64)
    print(f"sampler {dtype}: max |kernel - reference| {diff.max():.3e}, max D {D.max():.3e}, {int((diff > 0).sum())} of {diff.size} differ")
    bad = np.argmax(diff - tol)
    assert (diff <= tol).all(), (free_g[bad], free_r[bad], D[bad])
    assert (g[:, 1:][~pinned] != want_pin[~pinned]).all()


def test_sampler_does_not_depend_on_the_launch_shape(torch_mod):
    torch = torch_mod
    dev = torch.device("cuda", 0)
    R, _, W, mean, sigma, _, _ = sampler_case(torch, np.float64)
    rng = np.random.default_rng(2)
    mean, sigma = np.concatenate([mean, rng.uniform(-5, 5, (1, W, 2))]), np.concatenate([sigma, rng.uniform(0.1, 1, (1, W, 2))])
    m, s = torch.tensor(mean, device=dev), torch.tensor(sigma, device=dev)
    for tdt in (torch.float64, torch.float32):
        a = S().sample(m, s, 128, dtype=tdt, seed=9, iteration=1).view(4, 128, W, 2)
        b = S().sample(m, s, 64, dtype=tdt, seed=9, iteration=1).view(4, 64, W, 2)
        assert same_bits(a[:, :64], b)
        for r in range(4):
            one = S().sample(m[r:r + 1].contiguous(), s[r:r + 1].contiguous(), 128, dtype=tdt, seed=9, iteration=1, first_problem=r)
            assert same_bits(one.view(128, W, 2), a[r])
        assert not same_bits(S().sample(m, s, 128, dtype=tdt, seed=10, iteration=1).view(4, 128, W, 2)[:, 1:], a[:, 1:])
        assert not same_bits(S().sample(m, s, 128, dtype=tdt, seed=9, iteration=2).view(4, 128, W, 2)[:, 1:], a[:, 1:])
        assert not same_bits(a[0, 1:], a[1, 1:])


# ---------------------------------------------------------------- update

def update_case(R, N, W, dt, seed):
    """Random terms with planted exact ties, NaN, inf and flagged candidates; problem R - 1 has no finite candidate, problem
    R - 2 fewer finite ones than elites."""
    rng = np.random.default_rng(seed)
    B = R * N
    wp = rng.uniform(-5, 5, (R, N, W, 2)).astype(dt)
    t = {"counts": rng.integers(200, 400, B), "length": rng.uniform(5, 12, B), "flags": np.zeros(B, dtype=np.int64),
         "clearance": rng.uniform(-0.1, 1.0, B), "conflict": rng.uniform(-0.05, 1.0, B), "tracking": rng.uniform(0.0, 0.3, B)}
    for r in range(R):
        o = r * N
        tie = o + np.array([3, 9, N - 1])
        t["counts"][tie], t["length"][tie], t["clearance"][tie], t["conflict"][tie], t["tracking"][tie] = 201, 5.0, 0.5, 0.5, 0.1
        tie2 = o + np.array([4, 11])
        t["counts"][tie2], t["length"][tie2], t["clearance"][tie2], t["conflict"][tie2], t["tracking"][tie2] = 300, 9.0, -0.125, 0.5, 0.1
        t["clearance"][o + 5] = np.nan
        t["length"][o + 6] = np.nan
        t["length"][o + 7] = np.inf
        t["flags"][o + 8] = 2
        t["counts"][o + 10] = 0
        t["clearance"][o + 12] = np.inf
        t["conflict"][o + 13] = -np.inf
        t["tracking"][o + 14] = np.nan
    if R >= 2:
        t["flags"][(R - 1) * N:] = 1
        t["flags"][(R - 2) * N:(R - 1) * N] = 4
        t["flags"][(R - 2) * N + np.array([2, 17])] = 0
    mean, sigma = rng.uniform(-5, 5, (R, W, 2)), rng.uniform(0.05, 1.0, (R, W, 2))
    sigma[:, 0] = sigma[:, -1] = 0.0
    best_cost = np.full(R, np.inf)
    best_cost[0] = 1.0                                  # below every cost here: problem 0 keeps its best
    best_wp = rng.uniform(-5, 5, (R, W, 2)).astype(dt)
    best_terms = rng.uniform(0, 1, (R, 4))
    return wp, t, mean, sigma, best_cost, best_wp, best_terms


@pytest.mark.parametrize("dtype,N,E", [("f64", 100, 16), ("f32", 100, 100), ("f64", 2500, 300), ("f32", 4096, 64)])
def test_update_matches_reference(torch_mod, dtype, N, E):
    torch = torch_mod
    dev = torch.device("cuda", 0)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    dt = np_dt(torch, tdt)
    R, W = 4, 6
    alpha, smin, smax, iteration = 0.7, 0.08, 1.5, 2
    wp, t, mean, sigma, best_cost, best_wp, best_terms = update_case(R, N, W, dt, 10 + N)
    B = R * N
    r64 = sr.update(wp, sr.WEIGHTS, E, alpha, smin, smax, mean, sigma, best_cost, best_wp, best_terms, **t)
    rld = sr.update(wp, sr.WEIGHTS, E, alpha, smin, smax, mean, sigma, best_cost, best_wp, best_terms, ftype=np.longdouble, **t)
    counts = np.stack([t["counts"], np.full(B, 7)], axis=1).astype(np.int32)             # stride 2
    meta = np.stack([np.zeros(B), t["length"], np.zeros(B), np.zeros(B)], axis=1)

    def call():
        d = lambda a: torch.tensor(a, device=dev)
        st = dict(mean=d(mean), sigma=d(sigma), best_cost=d(best_cost), best_waypoints=d(best_wp), best_terms=d(best_terms),
                  history=torch.full((R, 5), -1.0, dtype=torch.float64, device=dev))
        res = S().update(d(wp.reshape(B, W, 2)), R, counts=d(counts), time_step=0.01, meta=d(meta), flags=d(t["flags"].astype(np.int32)),
                         clearance=d(t["clearance"]), conflict_clearance=d(t["conflict"]), tracking_worst=d(t["tracking"]),
                         elites=E, alpha=alpha, sigma_min=smin, sigma_max=smax, iteration=iteration, **st)
        return {**res, **st}
    a, b = call(), call()
    for k in a:
        assert same_bits(a[k], b[k]), f"{k}: two calls differ"
    g = {k: v.cpu().numpy() for k, v in a.items()}
    # cost: 4 ulp; inf where the reference's is; violation NaN where the reference's is
    c, cr = g["cost"], r64["cost"]
    assert np.array_equal(np.isinf(c), np.isinf(cr)) and not np.isnan(c).any()
    fin = np.isfinite(cr)
    assert (np.abs(c[fin] - cr[fin]) <= 4 * np.spacing(cr[fin])).all()
    assert np.array_equal(np.isnan(g["violation"]), np.isnan(r64["violation"]))
    vf = ~np.isnan(r64["violation"])
    assert np.array_equal(g["violation"][vf], r64["violation"][vf])
    print(f"update {dtype} N={N}: max cost difference {np.abs(c[fin] - cr[fin]).max():.3e}")
    assert np.array_equal(g["order"], r64["order"])
    assert np.array_equal(g["n_feasible"], r64["n_feasible"])
    for r in range(R):
        ne = len(r64["elites"][r])
        assert np.array_equal(g["order"][r, :ne], r64["elites"][r]) and np.isfinite(c[r * N + g["order"][r, :ne]]).all()
        assert ne == N or np.isinf(c[r * N + g["order"][r, ne]]) or ne == E
    assert len(r64["elites"][R - 1]) == 0 and (N == 1 or len(r64["elites"][R - 2]) == min(2, E))
    # best so far: index exact, waypoints bit for bit, cost and terms
    assert np.array_equal(g["best_terms"][:, 3], r64["best_terms"][:, 3])
    assert np.array_equal(g["best_waypoints"].view(np.uint8), r64["best_wp"].view(np.uint8))
    assert np.array_equal(g["best_cost"], r64["best_cost"]) or \
        (np.abs(g["best_cost"] - r64["best_cost"])[np.isfinite(r64["best_cost"])] <= 4 * np.spacing(r64["best_cost"][np.isfinite(r64["best_cost"])])).all()
    assert np.allclose(g["best_terms"], r64["best_terms"], rtol=1e-15, atol=0)
    assert g["best_cost"][0] == 1.0 and np.array_equal(g["best_waypoints"][0], best_wp[0])          # not replaced
    assert np.isinf(g["best_cost"][R - 1]) and np.array_equal(g["best_waypoints"][R - 1], best_wp[R - 1])
    assert np.array_equal(g["history"][:, iteration], g["best_cost"]) and (np.delete(g["history"], iteration, axis=1) == -1.0).all()
    # refit: max(1e-13, 8 D); untouched where nothing is finite and where sigma is 0
    for k in ("mean", "sigma"):
        D = np.abs(r64[k].astype(np.longdouble) - rld[k]).astype(np.float64)
        diff = np.abs(g[k] - r64[k])
        print(f"  {k}: max |kernel - reference| {diff.max():.3e}, max D {D.max():.3e}")
        assert (diff <= np.maximum(FLOOR, FACTOR * D)).all(), k
    assert np.array_equal(g["mean"][R - 1].view(np.int64), mean[R - 1].view(np.int64))
    assert np.array_equal(g["sigma"][R - 1].view(np.int64), sigma[R - 1].view(np.int64))
    assert np.array_equal(g["mean"][:, [0, -1]].view(np.int64), mean[:, [0, -1]].view(np.int64)) and (g["sigma"][:, [0, -1]] == 0).all()
    free = g["sigma"][:R - 1, 1:-1]
    assert (free >= smin).all() and (free <= smax).all()
    # rank(): the same scores and order with no mean and no best
    d = lambda x: torch.tensor(x, device=dev)
    rk = S().rank(d(wp.reshape(B, W, 2)), R, counts=d(counts), time_step=0.01, meta=d(meta), flags=d(t["flags"].astype(np.int32)),
                  clearance=d(t["clearance"]), conflict_clearance=d(t["conflict"]), tracking_worst=d(t["tracking"]))
    for k in ("cost", "violation", "order", "n_feasible"):
        assert same_bits(rk[k], a[k]), k


def test_update_with_single_terms(torch_mod):
    """Every term alone (the others NULL) against the reference: a missing term takes no part in the cost."""
    torch = torch_mod
    dev = torch.device("cuda", 0)
    R, N, W = 2, 70, 4
    wp, t, *_ = update_case(R, N, W, np.float64, 3)
    B = R * N
    d = lambda x: torch.tensor(x, device=dev)
    names = {"counts": "counts", "length": "meta", "flags": "flags", "clearance": "clearance", "conflict": "conflict_clearance",
             "tracking": "tracking_worst"}
    for k, arg in names.items():
        v = t[k]
        if k == "length":
            v = np.stack([np.zeros(B), v, np.zeros(B), np.zeros(B)], axis=1)
        elif k in ("counts", "flags"):
            v = v.astype(np.int32)
        got = S().rank(d(wp.reshape(B, W, 2)), R, **{arg: d(v)})
        ref = sr.update(wp, sr.WEIGHTS, **{k: t[k]})
        assert np.array_equal(got["order"].cpu().numpy(), ref["order"]), k
        assert np.array_equal(got["cost"].cpu().numpy(), ref["cost"]), k
        assert np.array_equal(got["n_feasible"].cpu().numpy(), ref["n_feasible"]), k


def test_update_with_one_candidate(torch_mod):
    """N = 1: nothing to sort; the candidate is the elite and the best."""
    torch = torch_mod
    dev = torch.device("cuda", 0)
    wp = np.random.default_rng(8).uniform(-5, 5, (2, 1, 3, 2))
    mean, sigma = np.zeros((2, 3, 2)), np.full((2, 3, 2), 0.5)
    counts = np.array([250, 0], dtype=np.int32)
    d = lambda x: torch.tensor(x, device=dev)
    st = dict(mean=d(mean), sigma=d(sigma), best_cost=d(np.full(2, np.inf)), best_waypoints=d(np.zeros((2, 3, 2))),
              best_terms=d(np.zeros((2, 4))))
    res = S().update(d(wp.reshape(2, 3, 2)), 2, counts=d(counts), elites=1, alpha=1.0, sigma_min=0.01, sigma_max=1.0, **st)
    assert res["order"].cpu().numpy().tolist() == [[0], [0]] and res["n_feasible"].cpu().numpy().tolist() == [1, 0]
    assert res["cost"].cpu().numpy().tolist() == [2.5, np.inf]
    assert np.array_equal(st["mean"].cpu().numpy()[0], wp[0, 0]) and (st["sigma"].cpu().numpy()[0] == 0.01).all()
    assert np.array_equal(st["mean"].cpu().numpy()[1], mean[1]) and np.array_equal(st["sigma"].cpu().numpy()[1], sigma[1])
    assert st["best_cost"].cpu().numpy().tolist() == [2.5, np.inf]
    assert np.array_equal(st["best_waypoints"].cpu().numpy()[0], wp[0, 0]) and (st["best_waypoints"].cpu().numpy()[1] == 0).all()
    assert st["best_terms"].cpu().numpy()[0].tolist() == [2.5, 0.0, 0.0, 0.0]


# ---------------------------------------------------------------- end to end

def scene_a():
    return FP().Scene(field=FIELD)


def scene_b():
    return FP().Scene(field=FIELD, circles=[CIRCLE_B])


def config(N, E=None, margin=0.05, **kw):
    s = S()
    return s.SearchConfig(candidates=N, elites=E if E is not None else max(8, N // 8), iterations=12, alpha=0.7,
                          weights=s.Weights(clearance_margin=margin), **kw)


def run(gen, seeds, scene, cfg, sigma0=0.5, **kw):
    return gen.refine(seeds, sigma0, FP().rectangle(18, 18), scene, dd=DD, dt=DT, capacity=CAP_S, capacity_rows=CAP_ROWS, config=cfg, **kw)


def pipeline_cost(torch, gen, routes, scene, weights, others=None):
    """The cost of ``routes`` (B, W, 2) through profile -> time_profile -> clearance [-> conflicts] -> rank, and the pieces."""
    wp = torch.tensor(np.asarray(routes), dtype=gen.tdtype, device=gen.device)
    res = gen.profile(wp, dd=DD, capacity=CAP_S)
    tp = gen.time_profile(res, dt=DT, capacity_rows=CAP_ROWS)
    foot = FP().rectangle(18, 18)
    clr = gen.footprint_clearance(tp, foot, scene, margin=weights.clearance_margin)
    terms = dict(counts=tp["counts"], time_step=DT, meta=res["meta"], flags=res["flags"], clearance=clr["min_clearance"])
    if others is not None:
        terms["conflict_clearance"] = gen.footprint_conflicts(tp, foot, others, margin=weights.conflict_margin)["min_clearance"]
    rk = S().rank(wp, len(routes), weights=weights, **terms)
    return rk["cost"].cpu().numpy(), rk["violation"].cpu().numpy(), res, tp, clr


def check_history(out, iterations=12):
    h = out["history"].cpu().numpy()
    assert h.shape[1] == iterations and not np.isnan(h).any() and (np.diff(h, axis=1) <= 0).all()
    assert np.array_equal(h[:, -1], out["best_cost"].cpu().numpy())
    return h


@pytest.mark.parametrize("N", [64, 4096])
def test_scenario_a_closes_the_gap_to_the_straight_line(torch_mod, N):
    torch = torch_mod
    gen = generator("f32")
    cfg = config(N, E=8 if N == 64 else None)
    c_seed, c_line = pipeline_cost(torch, gen, np.stack([SEED_A, LINE]), scene_a(), cfg.weights)[0]
    out = run(gen, SEED_A, scene_a(), cfg)
    h = check_history(out)
    best = float(out["best_cost"].item())
    share = (c_seed - best) / (c_seed - c_line)
    print(f"scenario A, N = {N}: seed {c_seed:.4f} s -> {best:.4f} s, straight line {c_line:.4f} s, share {share:.4f}")
    assert c_line < c_seed and h[0, 0] <= c_seed
    assert share >= 0.9
    assert bool(out["feasible"].item())
    bw = out["best_waypoints"].cpu().numpy()
    assert np.array_equal(bw[0, [0, -1]], SEED_A[[0, -1]].astype(bw.dtype))


@pytest.fixture(scope="module")
def scenario_b(torch_mod):
    """Scenario B at N = 64 and N = 4096 on the fp32 generator, run once and shared."""
    gen = generator("f32")
    return {N: run(gen, LINE, scene_b(), config(N, E=8 if N == 64 else None, margin=MARGIN_B)) for N in (64, 4096)}


@pytest.mark.parametrize("N", [64, 4096])
def test_scenario_b_leaves_the_collision(torch_mod, scenario_b, N):
    torch = torch_mod
    gen = generator("f32")
    out = scenario_b[N]
    w = S().Weights(clearance_margin=MARGIN_B)
    h = check_history(out)
    c_seed, v_seed = pipeline_cost(torch, gen, LINE[None], scene_b(), w)[:2]
    assert v_seed[0] > 0 and c_seed[0] > 1e6                        # the seed collides
    best, terms = float(out["best_cost"].item()), out["best_terms"].cpu().numpy()[0]
    print(f"scenario B, N = {N}: seed {c_seed[0]:.1f} -> {best:.4f} s, feasible from iteration {int(np.argmax(h[0] < 1e6))}, "
          f"n_feasible {out['n_feasible'].cpu().numpy()[0].tolist()}")
    assert bool(out["feasible"].item()) and np.isfinite(best) and terms[2] == 0.0 and best < 1e6
    # independently: the best route profiled alone, its rows against the footprint reference
    bw = out["best_waypoints"].cpu().numpy()
    cost1, viol1, res, tp, _ = pipeline_cost(torch, gen, bw, scene_b(), w)
    n = int(tp["counts"][0, 0].item())
    rows = tp["rows"][0, :n].cpu().numpy()
    clearance = fr.row_clearance(rows, FP().rectangle(18, 18), FIELD, (), [CIRCLE_B])[0].min()
    assert int(res["flags"][0].item()) == 0 and clearance >= MARGIN_B, clearance
    # best_terms reproduced: the batch size may pick another velocity kernel (1e-5 relative on the velocities), so the
    # count may move by a row and the fp32 pipeline's length by 1e-6 relative
    length = float(res["meta"][0, 1].item())
    print(f"  alone: {n} rows, length {length:.6f} ft, clearance {clearance:.4f} ft; best_terms {terms.tolist()}")
    assert abs(terms[0] - n * DT) <= DT * 1.000001 and abs(terms[1] - length) <= 1e-6 * length and viol1[0] == 0.0
    assert abs(cost1[0] - best) <= DT * 1.000001 + 1e-3 * 1e-6 * length
    assert 0 <= terms[3] < N and terms[3] == int(terms[3])


def test_refine_twice_gives_the_same_bits(torch_mod, scenario_b):
    gen = generator("f32")
    again = run(gen, LINE, scene_b(), config(64, E=8, margin=MARGIN_B))
    for k, v in scenario_b[64].items():
        assert same_bits(v, again[k]), k


def test_four_problems_equal_four_single_runs(torch_mod):
    """R = 4 copies of scenario B in one call against four R = 1 calls with first_problem = r: every output bit for bit."""
    torch = torch_mod
    gen = generator("f64")
    cfg = config(64, E=8, margin=MARGIN_B, seed=3)
    four = run(gen, np.repeat(LINE[None], 4, axis=0), scene_b(), cfg)
    assert tuple(four["history"].shape) == (4, 12) and tuple(four["n_feasible"].shape) == (4, 12)
    assert tuple(four["cost"].shape) == (4, 64) and tuple(four["order"].shape) == (4, 64)
    hist = four["history"].cpu().numpy()
    assert len({hist[r].tobytes() for r in range(4)}) > 1                     # the problems draw different candidates
    for r in range(4):
        one = run(gen, LINE, scene_b(), cfg, first_problem=r)
        for k, v in one.items():
            assert same_bits(v[0], four[k][r]), (k, r)
    assert bool(four["feasible"].all().item())


def test_a_parked_partner_on_the_best_route_is_avoided(torch_mod, scenario_b):
    """A partner parked on B's best route makes it infeasible; the search, seeded with that route, finds another feasible
    one.  Settings: the detour has to move the route's middle by the partner's width plus the margin, 1.55 ft, and the
    overlap measure is flat while one footprint's projection contains the other's (include/vap.h), so sigma0 is 1 ft, the
    size of the obstacle, not scenario B's 0.5 ft; N = 256, E = 32, 12 iterations."""
    torch = torch_mod
    gen = generator("f32")
    w = S().Weights(clearance_margin=MARGIN_B, conflict_margin=0.05)
    bw = scenario_b[64]["best_waypoints"].cpu().numpy()
    _, _, _, tp, _ = pipeline_cost(torch, gen, bw, scene_b(), w)
    n = int(tp["counts"][0, 0].item())
    mid = tp["rows"][0, n // 2].cpu().numpy()
    # the partner: one row, parked for good at the middle of B's best route, heading 0
    prow = np.zeros((1, 1, 8))
    prow[0, 0, 6:8] = mid[6:8]
    others = {"rows": torch.tensor(prow, device=gen.device), "counts": torch.tensor([[1, 0]], dtype=torch.int32, device=gen.device)}
    cost, viol = pipeline_cost(torch, gen, bw, scene_b(), w, others=others)[:2]
    assert viol[0] > 0 and cost[0] > 1e6                              # B's best route now collides
    cfg = S().SearchConfig(candidates=256, elites=32, iterations=12, alpha=0.7, weights=w)
    out = run(gen, bw[0], scene_b(), cfg, sigma0=1.0, others=others)
    h = check_history(out)
    print(f"partner at {mid[6:8].tolist()}: {cost[0]:.1f} -> {float(out['best_cost'].item()):.4f} s, history {h[0].tolist()}")
    assert bool(out["feasible"].item())
    new = out["best_waypoints"].cpu().numpy()
    assert not np.array_equal(new, bw)
    cost2, viol2, _, tp2, clr2 = pipeline_cost(torch, gen, new, scene_b(), w, others=others)
    assert viol2[0] == 0.0 and float(clr2["min_clearance"][0].item()) >= MARGIN_B
    # the partner's square as a fixed polygon of the footprint reference
    n2 = int(tp2["counts"][0, 0].item())
    square = FP().rectangle(18, 18) + mid[6:8]
    gap = fr.row_clearance(tp2["rows"][0, :n2].cpu().numpy(), FP().rectangle(18, 18), None, [square], ())[0].min()
    assert gap >= 0.05 - 1e-9, gap


def test_config_3_shape_runs(torch_mod):
    """R = 1, N = 4096, W = 32, S = 10^4, 5 iterations on the field scene of tools/footprint_bench.py."""
    torch = torch_mod
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from footprint_bench import field_scene
    from vexautonomousplanner_amd.synth import make_waypoints
    gen = generator("f32")
    seed = make_waypoints(1, 32, 3)[0].astype(np.float64)
    cfg = S().SearchConfig(candidates=4096, elites=256, iterations=5)
    out = gen.refine(seed, 0.3, FP().rectangle(18, 18), field_scene(), samples=10000, capacity_rows=2048, config=cfg)
    torch.cuda.synchronize()
    check_history(out, 5)
    for k in ("best_waypoints", "best_cost", "best_terms", "history", "mean", "sigma"):
        assert bool(torch.isfinite(out[k]).all().item()), k
    assert tuple(out["best_waypoints"].shape) == (1, 32, 2) and tuple(out["cost"].shape) == (1, 4096)
    order = out["order"].cpu().numpy()[0]
    assert sorted(order.tolist()) == list(range(4096))
    c = out["cost"].cpu().numpy()[0]
    nfin = int(np.isfinite(c).sum())
    assert np.isfinite(c[order[:nfin]]).all() and (np.diff(c[order[:nfin]]) >= 0).all()
    h = out["history"].cpu().numpy()[0]
    print(f"config 3 shape: history {h.tolist()}, n_feasible {out['n_feasible'].cpu().numpy()[0].tolist()}")
