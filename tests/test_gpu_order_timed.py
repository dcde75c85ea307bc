"""GPU: vap_plan_order_timed (plan.order_timed, plan.timed_routine, BatchedTrajectoryGenerator.plan_timed_routine) against
tests/order_timed_ref.py and, for the rows of the chosen order, against the device's own timeline.chain.

Every comparison is exact: the order, the counts and the arrival rows are integers, value_total is an fp64 sum formed in
ascending site order, and duration / arrival are one fp64 product each.  No tolerance.  Every output buffer of a device call
is prefilled with a sentinel, so an entry the call does not write shows."""
import contextlib
import math

import numpy as np
import pytest

import order_timed_ref as otr
import plan_ref as pr
import test_order_timed_cpu as tcpu
import test_timeline_cpu as tc

pytestmark = pytest.mark.gpu

CONS, SLOW = tcpu.CONS, tcpu.SLOW
SENTINEL = -77
INTS = ("order", "n_visited", "rows_total", "arrival_rows", "flags")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def P():
    from vexautonomousplanner_amd import plan
    return plan


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def sentinel_out(torch, R, M):
    mk = lambda shape, dtype, v: torch.full(shape, v, dtype=dtype, device="cuda:0")
    return {"order": mk((R, M), torch.int32, SENTINEL), "n_visited": mk((R,), torch.int32, SENTINEL),
            "rows_total": mk((R,), torch.int32, SENTINEL), "arrival_rows": mk((R, M), torch.int32, SENTINEL),
            "value_total": mk((R,), torch.float64, float(SENTINEL)), "flags": mk((R,), torch.int32, SENTINEL)}


def device_solve(torch, pb, constraints=CONS, dt=0.01, budget=None, end=None, out=None, **over):
    """plan.order_timed on the problem dict of test_order_timed_cpu.random_problems, into sentinel-filled buffers; returns
    host arrays.  ``budget`` is in seconds."""
    R, M = pb["leg"].shape[0], pb["leg"].shape[1] - 1
    out = sentinel_out(torch, R, M) if out is None else out
    kept = {k: out[k].data_ptr() for k in INTS + ("value_total",)}
    kw = dict(dwell=pb["dwell"], start_heading=pb["start_heading"], value=pb["value"], before=pb["before"],
              leg_flags=pb["leg_flags"])
    kw.update(over)
    res = P().order_timed(pb["rows"], pb["counts"], pb["leg"], budget=budget, end=end, constraints=constraints, dt=dt, out=out, **kw)
    torch.cuda.synchronize()
    assert all(res[k].data_ptr() == p for k, p in kept.items())         # the caller's buffers were filled
    return {k: host(v) for k, v in res.items()}


def ref_solve(pb, method, constraints=CONS, dt=0.01, budget=None, end=None, **over):
    rows = None if budget is None else [otr.budget_rows(b, dt) for b in np.broadcast_to(budget, (pb["leg"].shape[0],))]
    return tcpu.solve(pb, method, constraints, dt, budget_rows=rows, end=end, **over)


def check(got, ref, dt):
    """Device against reference, every output; duration and arrival are rows * dt."""
    assert tcpu.same(got, ref)
    assert got["feasible"].tolist() == (ref["flags"] == 0).tolist()
    want_d = np.where(ref["rows_total"] >= 0, ref["rows_total"].astype(np.float64) * dt, np.nan)
    want_a = np.where(ref["arrival_rows"] >= 0, ref["arrival_rows"].astype(np.float64) * dt, np.nan)
    for g, w in ((got["duration"], want_d), (got["arrival"], want_a)):
        assert bool(((bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))).all()), (g, w)
    return True


def seconds(rows, dt):
    """A budget in seconds that int(budget / dt) turns into exactly ``rows`` rows."""
    return (np.asarray(rows, dtype=np.float64) + 0.5) * dt


# ---------------------------------------------------------------- 1: caller-written legs

def written_legs(dt):
    """The 9 legs of P = 4 in a capacity of 80, counts from {1, 63, 64, 65, 80}, headings exact: arriving at site 1 with
    3.0 and leaving with -3.0 crosses the wrap the short way; -0.0 -> -pi is a reversal; 0.9 degrees either way stay below
    turn_min, 1.1 degrees do not."""
    deg = math.radians
    spec = {  # (a, b): (count, first heading, last heading)
        (0, 1): (63, 0.5, 3.0), (0, 2): (64, 0.5 + deg(0.9), -0.0), (0, 3): (65, 0.5 - deg(0.9), 1.0),
        (1, 2): (80, -3.0, -0.0), (1, 3): (1, 3.0 + deg(1.1), 3.0 + deg(1.1)), (2, 1): (64, -math.pi, 1.0 + deg(0.9)),
        (2, 3): (63, -math.pi, 1.0), (3, 1): (65, 1.0 + deg(0.9), 3.0), (3, 2): (80, 1.0 - deg(1.1), math.pi)}
    legs, mat = [], np.full((4, 4), -1, dtype=np.int32)
    for (a, b), (n, hf, hl) in spec.items():
        l = tc.straight_leg(n, (float(a), float(b)), hf, 0.01 * n, dt)
        l[-1, 4] = hl if n > 1 else hf
        mat[a, b] = len(legs)
        legs.append(l)
    rows, counts = tc.pack(legs, cap=80)
    return rows, np.stack([counts, counts + 5], axis=1).astype(np.int32), mat


@pytest.mark.parametrize("dt", [0.01, 0.02])
@pytest.mark.parametrize("constraints", [CONS, SLOW], ids=["triangle", "trapezoid"])
def test_written_legs_against_the_brute_force(torch_mod, constraints, dt):
    rows, counts, mat = written_legs(dt)
    starts = [np.nan, 0.5, 0.5 + math.radians(0.9), -2.6, math.pi, -0.0, 3.0, 0.5 - math.radians(1.1)]
    R = len(starts)
    rng = np.random.default_rng(5)
    pb = dict(rows=rows, counts=counts, leg=np.broadcast_to(mat, (R, 4, 4)).copy(), leg_flags=np.zeros(9, dtype=np.uint32),
              dwell=rng.choice([0.0, 0.05, 0.019, 0.1], size=(R, 4)), start_heading=np.array(starts),
              value=rng.choice([1.0, 2.0, 0.5], size=(R, 4)), before=np.zeros((R, 4), dtype=np.uint32))
    full = ref_solve(pb, "brute", constraints, dt)
    assert (full["flags"] == 0).all()
    assert check(device_solve(torch_mod, pb, constraints, dt), full, dt)
    for end in (None, 2):
        for budget in (seconds(full["rows_total"] - 1, dt), seconds(full["rows_total"], dt), seconds(rng.integers(0, 200, R), dt),
                       seconds(rng.integers(100, 400, R), dt)):
            ref = ref_solve(pb, "brute", constraints, dt, budget=budget, end=end)
            assert check(device_solve(torch_mod, pb, constraints, dt, budget=budget, end=end), ref, dt)
    # the chosen order's rows are the timeline's, on the device
    from vexautonomousplanner_amd import timeline
    got = device_solve(torch_mod, pb, constraints, dt)
    stops = np.concatenate([np.zeros((R, 1), dtype=np.int64), got["order"]], axis=1)
    legs = mat[stops[:, :-1], stops[:, 1:]]
    slot_dwell = np.take_along_axis(pb["dwell"], got["order"].astype(np.int64), axis=1)
    tl = timeline.chain(rows, counts, legs, dwell=slot_dwell, start_heading=pb["start_heading"], constraints=constraints, dt=dt,
                        capacity_rows=1024)
    torch_mod.cuda.synchronize()
    assert host(tl["flags"]).tolist() == [0] * R and np.array_equal(host(tl["counts"])[:, 0], got["rows_total"])
    assert np.array_equal(host(tl["map"])[:, :, 2], got["arrival_rows"])


# ---------------------------------------------------------------- 2, 8: the largest table

@pytest.fixture(scope="module")
def eight_sites():
    """R = 64 random problems of M = 8 over 40 shared legs with the special cases in front, and the reference's answers,
    computed once."""
    rng = np.random.default_rng(88)
    R, M = 64, 8
    pb = tcpu.random_problems(rng, R, M, L=40, spoilt=10, bad_index=0.08)
    pb["leg"][0] = -1                                                   # everything forbidden
    pb["start_heading"][1] = 7.0                                        # outside +-2 pi
    pb["start_heading"][2] = np.nan
    pb["before"][3] = 0
    pb["before"][3, 1], pb["before"][3, 2] = 2, 1                       # a cycle: 2 before 1, 1 before 2
    pb["before"][4] = 0
    for k in range(2, 6):
        pb["before"][4, k] = 1 << (k - 2)                               # a chain 1 < 2 < 3 < 4 < 5
    pb["before"][5, 3] |= 0xFFFFFF00                                    # bits >= M are ignored
    budget = seconds(rng.integers(0, 260, R), 0.01)
    cases = {"full": dict(), "full_end": dict(end=5), "budget": dict(budget=budget), "budget_end": dict(budget=budget, end=3)}
    refs = {k: ref_solve(pb, "dp", CONS, 0.01, **kw) for k, kw in cases.items()}
    return pb, cases, refs


@pytest.mark.parametrize("case", ["full", "full_end", "budget", "budget_end"])
def test_eight_sites_against_the_reference(torch_mod, eight_sites, case):
    pb, cases, refs = eight_sites
    ref = refs[case]
    if case == "full":
        assert ref["flags"][[0, 1, 3]].tolist() == [otr.INFEASIBLE] * 3 and ref["flags"][[2, 4]].tolist() == [0, 0]
        assert (ref["flags"] == 0).sum() >= 48
        o = ref["order"][4].tolist()
        assert [o.index(k) for k in (1, 2, 3, 4, 5)] == sorted(o.index(k) for k in (1, 2, 3, 4, 5))
    if case == "budget":
        assert len(set(ref["n_visited"].tolist())) >= 5 and ref["flags"][0] == 0 and ref["n_visited"][0] == 0
    assert check(device_solve(torch_mod, pb, CONS, 0.01, **cases[case]), ref, 0.01)


def test_two_calls_give_the_same_bytes(torch_mod, eight_sites):
    torch = torch_mod
    pb, cases, refs = eight_sites
    out = sentinel_out(torch, 64, 8)
    first = device_solve(torch, pb, CONS, 0.01, out=out, **cases["budget"])
    again = device_solve(torch, pb, CONS, 0.01, out=out, **cases["budget"])
    for k in INTS + ("value_total", "duration", "arrival"):
        assert np.array_equal(np.ascontiguousarray(first[k]).view(np.uint8), np.ascontiguousarray(again[k]).view(np.uint8)), k


# ---------------------------------------------------------------- 3: small and persistent cases

@pytest.mark.parametrize("M", [1, 2])
def test_one_and_two_sites(torch_mod, M):
    rng = np.random.default_rng(20 + M)
    pb = tcpu.random_problems(rng, 24, M, L=8, spoilt=2, bad_index=0.1)
    for kw in (dict(), dict(end=M), dict(budget=seconds(rng.integers(0, 40, 24), 0.02))):
        ref = ref_solve(pb, "brute", SLOW, 0.02, **kw)
        assert check(device_solve(torch_mod, pb, SLOW, 0.02, **kw), ref, 0.02)
    assert len(set(ref_solve(pb, "brute", SLOW, 0.02)["flags"].tolist())) == 2      # feasible and infeasible ones


def test_more_problems_than_workgroups_and_none(torch_mod):
    torch = torch_mod
    rng = np.random.default_rng(31)
    R = 1100                                                            # the persistent grid has 1024 workgroups
    pb = tcpu.random_problems(rng, R, 2, L=12, spoilt=2, bad_index=0.05)
    budget = seconds(rng.integers(0, 60, R), 0.01)
    for kw in (dict(), dict(budget=budget)):
        assert check(device_solve(torch, pb, CONS, 0.01, **kw), ref_solve(pb, "dp", CONS, 0.01, **kw), 0.01)
    # R = 0: nothing is touched
    rows = torch.zeros((3, 4, 8), dtype=torch.float64, device="cuda:0")
    none = P().order_timed(rows, torch.ones((3, 1), dtype=torch.int32, device="cuda:0"),
                           torch.zeros((0, 3, 3), dtype=torch.int32, device="cuda:0"))
    torch.cuda.synchronize()
    assert tuple(none["order"].shape) == (0, 2) and tuple(none["duration"].shape) == (0,)
    with pytest.raises(ValueError):
        P().order_timed(rows, torch.ones((3, 1), dtype=torch.int32, device="cuda:0"),
                        torch.zeros((1, 10, 10), dtype=torch.int32, device="cuda:0"))


# ---------------------------------------------------------------- 4: the budget's rules

def test_budget_rules(torch_mod):
    """The hand cases of test_order_timed_cpu.test_budget_rules_by_hand, one problem each, on the device."""
    torch = torch_mod
    dt = 0.01
    leg_rows = [tc.straight_leg(10, (0, 0), 0.5, 1.0, dt) for _ in range(4)]
    rows, counts = tc.pack(leg_rows)
    mat = np.array([[-1, 0, 1], [-1, -1, 2], [-1, 3, -1]], dtype=np.int32)
    ones = np.array([0.0, 1.0, 1.0])
    problems = [  # (budget rows, value, before, end), expected (order, rows, value, flags)
        ((0, ones, 0, None), ([-1, -1], 0, 0.0, 0)),
        ((9, ones, 0, None), ([-1, -1], 0, 0.0, 0)),                    # one row below the shortest sequence
        ((10, ones, 0, None), ([1, -1], 10, 1.0, 0)),                   # exactly at it; equal value and rows: the lowest S
        ((19, ones, 0, None), ([1, -1], 10, 1.0, 0)),
        ((20, ones, 0, None), ([2, 1], 20, 2.0, 0)),                    # 1, 2 ties with 2, 1: the lowest last site
        ((-4, ones, 0, None), ([-1, -1], 0, 0.0, 0)),                   # negative counts as 0
        ((10, np.array([0.0, 1.0, 1.5]), 0, None), ([2, -1], 10, 1.5, 0)),
        ((100, np.array([0.0, np.nan, -2.0]), 0, None), ([-1, -1], 0, 0.0, 0)),   # worth nothing: the fewest rows win
        ((100, np.array([0.0, np.inf, 0.25]), 0, None), ([2, -1], 10, 0.25, 0)),
        ((100, np.array([0.0, 1.0, 0.0]), 2, None), ([2, 1], 20, 1.0, 0)),        # site 1 waits for the worthless site 2
        ((9, ones, 0, 1), ([-1, -1], -1, np.nan, otr.INFEASIBLE)),                # must end at 1 and nothing fits
        ((10, ones, 0, 2), ([2, -1], 10, 1.0, 0)),
    ]
    for n, ((b, value, before1, end), (order, total, val, flags)) in enumerate(problems):
        pb = dict(rows=rows, counts=counts.reshape(-1, 1), leg=mat[None].copy(), leg_flags=None, dwell=None, start_heading=None,
                  value=value[None], before=np.array([[0, before1, 0]], dtype=np.uint32))
        ref = ref_solve(pb, "brute", CONS, dt, budget=[float(seconds(b, dt))], end=end)
        assert ref["order"].tolist() == [order] and ref["rows_total"].tolist() == [total] and ref["flags"].tolist() == [flags], n
        assert bits(ref["value_total"]).tolist() == bits([val]).tolist() or (np.isnan(val) and np.isnan(ref["value_total"][0])), n
        assert check(device_solve(torch, pb, CONS, dt, budget=float(seconds(b, dt)), end=end), ref, dt), n
    # an ample budget with positive values gives full mode's bytes
    rng = np.random.default_rng(41)
    pb = tcpu.random_problems(rng, 32, 5, L=20, bad_index=0.0)
    pb["value"] = rng.choice([1.0, 2.0, 0.25], size=pb["value"].shape)
    full = device_solve(torch, pb, CONS, dt)
    ample = device_solve(torch, pb, CONS, dt, budget=1e7)
    assert check(full, ref_solve(pb, "dp", CONS, dt), dt) and (full["flags"] == 0).sum() >= 16
    ok = full["flags"] == 0
    for k in INTS + ("value_total", "duration", "arrival"):
        assert np.array_equal(np.ascontiguousarray(full[k][ok]).view(np.uint8), np.ascontiguousarray(ample[k][ok]).view(np.uint8)), k


# ---------------------------------------------------------------- 5: real legs

def profiled_pairs(torch, gen, points, dt, W=5, wobble=0.0, seed=0):
    """profile -> time_profile of the (P - 1)^2 ordered pairs that can be legs: W waypoints on the segment, the inner ones
    moved by ``wobble`` feet.  Returns tp, the (P, P) leg matrix and the profile's flags."""
    rng = np.random.default_rng(seed)
    Pn = len(points)
    pairs = [(a, b) for a in range(Pn) for b in range(1, Pn) if a != b]
    mat = np.full((Pn, Pn), -1, dtype=np.int32)
    wp = np.zeros((len(pairs), W, 2))
    for k, (a, b) in enumerate(pairs):
        mat[a, b] = k
        wp[k] = np.linspace(points[a], points[b], W)
        wp[k, 1:-1] += rng.normal(0, wobble, (W - 2, 2)) if wobble else 0.0
    res = gen.profile(torch.tensor(wp, dtype=gen.tdtype, device=gen.device), CONS, dd=0.005, capacity=4096)
    tp = gen.time_profile(res, CONS, dt=dt, capacity_rows=1024)
    return tp, mat, res["flags"]


@pytest.mark.parametrize("dt", [0.01, 0.02])
def test_real_legs_chain_to_the_same_rows(torch_mod, dt):
    torch = torch_mod
    from vexautonomousplanner_amd import timeline
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    gen = BatchedTrajectoryGenerator(0, "f32")
    points = np.array([[0.0, 0.0], [2.5, 0.4], [-1.0, 2.2], [1.2, -2.0]])
    tp, mat, flags = profiled_pairs(torch, gen, points, dt, wobble=0.15, seed=3)
    R, M = 3, 3
    dwell = np.array([[0.0, 0.3, 0.0, 0.11], [0.0, 0.0, 0.25, 0.019], [0.0, 1.0, 0.0, 0.0]])
    start = np.array([2.0, np.nan, -1.0])
    out = sentinel_out(torch, R, M)
    od = P().order_timed(tp["rows"], tp["counts"], np.broadcast_to(mat, (R, 4, 4)).copy(), dwell=dwell, start_heading=start,
                         leg_flags=flags, end=None, constraints=CONS, dt=dt, out=out, ctx=gen.ctx)
    # gathered on the device, as plan.timed_routine does
    o = od["order"].to(torch.int64)
    frm = torch.cat([torch.zeros_like(o[:, :1]), o[:, :-1]], dim=1)
    legs = torch.tensor(mat, device=gen.device)[frm, o]
    slot_dwell = torch.gather(torch.tensor(dwell, device=gen.device), 1, o)
    tl = gen.routine_timeline(tp, legs, dwell=slot_dwell, start_heading=start, n_legs=od["n_visited"], constraints=CONS, dt=dt,
                              capacity_rows=4096)
    torch.cuda.synchronize()
    rows, counts = host(tp["rows"]), host(tp["counts"])
    assert host(flags).tolist() == [0] * 9 and (counts[:, 0] > 40).all() and (counts[:, 0] < 1024).all()
    got = {k: host(v) for k, v in od.items()}
    pb = dict(rows=rows, counts=counts, leg=np.broadcast_to(mat, (R, 4, 4)), leg_flags=host(flags), dwell=dwell,
              start_heading=start, value=None, before=None)
    assert check(got, ref_solve(pb, "brute", CONS, dt), dt)
    assert host(tl["flags"]).tolist() == [0] * R
    assert np.array_equal(host(tl["counts"])[:, 0], got["rows_total"]) and np.array_equal(host(tl["counts"])[:, 1], got["n_visited"])
    assert np.array_equal(host(tl["map"])[:, :, 2], got["arrival_rows"]) and got["n_visited"].tolist() == [M] * R
    assert np.array_equal(bits(host(tl["duration"])), bits(got["duration"])) and np.array_equal(bits(host(tl["arrival"])), bits(got["arrival"]))


# ---------------------------------------------------------------- 6: the worked case

def test_the_length_order_is_the_slower_one_on_the_device(torch_mod):
    torch = torch_mod
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    gen = BatchedTrajectoryGenerator(0, "f32")
    points = np.array([tcpu.AB_POINTS[k] for k in (0, 1, 2)])
    tp, mat, flags = profiled_pairs(torch, gen, points, 0.01, W=3)
    od = P().order_timed(tp["rows"], tp["counts"], mat, start_heading=math.pi, leg_flags=flags, ctx=gen.ctx)
    both = np.array([[mat[0, 1], mat[1, 2]], [mat[0, 2], mat[2, 1]]])    # A then B; B then A
    tl = gen.routine_timeline(tp, both, start_heading=[math.pi, math.pi], capacity_rows=1024)
    torch.cuda.synchronize()
    rows, counts = host(tp["rows"]), host(tp["counts"])
    p = otr.Problem(rows, counts[:, 0], mat, CONS, 0.01, math.radians(1.0), None, math.pi, None, None, None, None, None)
    ab, ba = p.sequence((1, 2)), p.sequence((2, 1))
    assert host(od["order"]).tolist() == [2, 1] and int(od["rows_total"]) == ba[0] and host(od["arrival_rows"]).tolist() == ba[1]
    assert host(tl["counts"])[:, 0].tolist() == [ab[0], ba[0]] and host(tl["flags"]).tolist() == [0, 0]
    d = host(tl["duration"])
    assert bits(d[1]) == bits(host(od["duration"])) and d[1] < d[0]
    assert ab[0] - ba[0] == int(host(tl["counts"])[0, 0]) - int(od["rows_total"]) > 80       # 87 rows on the oracle's legs


# ---------------------------------------------------------------- 7: end to end

@contextlib.contextmanager
def no_host_reads(torch, monkeypatch):
    """Inside, reading a device tensor on the host or waiting for the device raises."""
    def refuse(name, orig):
        def f(self, *a, **kw):
            if isinstance(self, torch.Tensor) and self.is_cuda:
                raise AssertionError(f"host read of a device tensor: {name}")
            return orig(self, *a, **kw)
        return f
    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__"):
            m.setattr(torch.Tensor, name, refuse(name, getattr(torch.Tensor, name)))
        m.setattr(torch.cuda, "synchronize", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("torch.cuda.synchronize")))
        yield


def test_timed_routine_end_to_end(torch_mod, monkeypatch):
    """Scene C's routine (the start and four sites) through plan_timed_routine: the order of the profiled seed legs by the
    clock, chained; against the reference on the same legs, against plan.routine's length order chained over the same
    legs, and under a budget that leaves one site out."""
    torch = torch_mod
    import test_gpu_routine as tgr
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    sc, W, M, dt = pr.SCENE_C, 9, 4, 0.01
    gen = BatchedTrajectoryGenerator(0, "f32")
    scene = tgr.scene_of(sc)
    dwell = np.array([0.0, 0.3, 0.0, 0.2, 0.1])
    kw = dict(cell=sc["cell"], margin=sc["margin"], before=tgr.BEFORE, dwell=dwell, start_heading=0.5, constraints=CONS, dt=dt,
              leg_capacity_rows=1024)
    torch.cuda.synchronize()
    with no_host_reads(torch, monkeypatch):
        res = gen.plan_timed_routine(tgr.ROUTINE, scene, W, sc["radius"], **kw)
    torch.cuda.synchronize()
    assert tuple(res["legs"].shape) == (M, W, 2) and tuple(res["order"].shape) == (M,) and tuple(res["leg_matrix"].shape) == (5, 5)
    rows, counts, flags, mat = host(res["leg_rows"]), host(res["leg_counts"]), host(res["leg_flags"]), host(res["leg_matrix"])
    assert rows.shape[0] == M * M and flags.tolist() == [0] * (M * M)
    masks = P().before_masks(tgr.BEFORE, 1, 5)
    pb = dict(rows=rows, counts=counts, leg=mat[None], leg_flags=flags, dwell=dwell[None], start_heading=np.array([0.5]),
              value=None, before=masks)
    ref = ref_solve(pb, "dp", CONS, dt)
    got = {k: host(res[k])[None] for k in INTS + ("value_total", "feasible", "duration", "arrival")}
    assert check(got, ref, dt) and ref["flags"].tolist() == [0]
    tl = {k: host(v) for k, v in res["timeline"].items()}
    assert tl["flags"].tolist() == [0] and tl["counts"].tolist() == [[int(ref["rows_total"][0]), M]]
    assert tl["map"][0, :, 2].tolist() == ref["arrival_rows"][0].tolist()
    order = ref["order"][0].tolist()
    stops = [0] + order
    assert host(res["leg_index"]).tolist() == [int(mat[a, b]) for a, b in zip(stops[:-1], stops[1:])]
    wp = host(res["waypoints"])
    assert np.array_equal(bits(host(res["legs"])), bits(np.stack([wp[a, b] for a, b in zip(stops[:-1], stops[1:])])))
    # plan.routine's order (by length) chained over the same legs takes at least as many rows: the timed order is the
    # fewest rows over every admissible order
    by_length = host(gen.plan_routine(tgr.ROUTINE, scene, W, sc["radius"], cell=sc["cell"], margin=sc["margin"],
                                      before=tgr.BEFORE)["order"]).tolist()
    ls = [0] + by_length
    chained = gen.routine_timeline({"rows": res["leg_rows"], "counts": res["leg_counts"]},
                                   np.array([[mat[a, b] for a, b in zip(ls[:-1], ls[1:])]]),
                                   dwell=np.array([[dwell[s] for s in by_length]]), start_heading=[0.5], constraints=CONS, dt=dt)
    torch.cuda.synchronize()
    n_length = int(host(chained["counts"])[0, 0])
    print(f"timed order {order}: {int(ref['rows_total'][0])} rows; length order {by_length}: {n_length} rows")
    assert host(chained["flags"]).tolist() == [0] and int(ref["rows_total"][0]) <= n_length
    # a budget one row short of the whole routine leaves one site out
    budget = float(seconds(int(ref["rows_total"][0]) - 1, dt))
    short = gen.plan_timed_routine(tgr.ROUTINE, scene, W, sc["radius"], budget=budget, capacity_rows=8192, **kw)
    torch.cuda.synchronize()
    ref_short = ref_solve(pb, "dp", CONS, dt, budget=[budget])
    got = {k: host(short[k])[None] for k in INTS + ("value_total", "feasible", "duration", "arrival")}
    assert check(got, ref_short, dt)
    assert int(short["n_visited"]) == 3 and float(short["duration"]) <= budget
    stl = {k: host(v) for k, v in short["timeline"].items()}
    assert stl["counts"].tolist() == [[int(ref_short["rows_total"][0]), 3]] and stl["flags"].tolist() == [0]
    assert stl["map"][0, :, 2].tolist() == ref_short["arrival_rows"][0].tolist() and np.isnan(host(short["legs"])[3]).all()
