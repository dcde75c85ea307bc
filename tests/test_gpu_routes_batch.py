"""GPU: batches of routes with reverse / turn nodes (several splines per route) through the batched kernels
(vap_profile_routes: k_fit_routes, per-spline k_lut + offsets, k_sample_routes, the plain velocity pass; then
vap_route_limits / vap_velocity_pass_limits for node and action-point limits) — against the real reference's golden
routes (feat_reverse, feat_turn, feat_mixed, feat_split2, and the plain / tangent ones as the one-spline case) and
against the oracle on random routes.  SM:42-172, 243-275, 436-464; MPG:70-316."""
import numpy as np
import pytest

import golden_util as gu
from events_util import full_profile

pytestmark = pytest.mark.gpu

ROUTES = ["feat_reverse", "feat_turn", "feat_mixed", "feat_split2", "feat_tangent", "feat_stop", "feat_limits", "feat_action",
          "plain_w8_s0", "plain_w2_s1"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_gen(dtype):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    return BatchedTrajectoryGenerator(0, dtype)


def run_route(torch, gen, g, copies=3):
    """The golden route `copies` times in one batch (so that the batch axis is exercised), limits applied."""
    wp = np.repeat(g["waypoints"][None], copies, axis=0)
    W = wp.shape[1]
    N = int(g["n_samples"])
    rep = lambda a: np.repeat(np.asarray(a)[None], copies, axis=0)
    t = torch.tensor(wp, dtype=gen.tdtype, device=gen.device)
    r = gen.profile_routes(t, node_reverse=rep(g["node_is_reverse_node"]), node_turn=rep(g["node_turn"]),
                           node_tangent=rep(g["node_tangent"]), node_magnitudes=rep(g["node_magnitudes"]),
                           constraints=g["constraints"], dd=float(g["dd"]), capacity=N + 9)
    aps = None
    if "ap_t" in g.files:
        one = [{"t": float(t_), "max_velocity": float(mv), "max_acceleration": float(ma), "stop": bool(st)}
               for t_, mv, ma, st in zip(g["ap_t"], g["ap_max_velocity"], g["ap_max_acceleration"], g["ap_stop"])]
        aps = [one for _ in range(copies)]
    if aps or g["node_stop"].any() or g["node_max_velocity"].any() or g["node_max_acceleration"].any():
        gen.apply_node_limits(r, g["constraints"], node_max_velocity=rep(g["node_max_velocity"]), node_stop=rep(g["node_stop"]),
                              node_max_acceleration=rep(g["node_max_acceleration"]), action_points=aps)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("dtype,tol", [("f32", 1e-5), ("f64", 1e-9)])
@pytest.mark.parametrize("name", ROUTES)
def test_batched_route_matches_reference_golden(torch_mod, name, dtype, tol):
    g = gu.load(name)
    gen = make_gen(dtype)
    r = run_route(torch_mod, gen, g)
    N = int(g["n_samples"])
    assert not r["flags"].any().item()
    assert r["spline_counts"].tolist() == [int(g["n_splines"])] * 3
    assert (r["meta"][:, 3] == N).all().item()
    np.testing.assert_allclose(r["meta"][:, 1].cpu().numpy(), float(g["total_length"]), rtol=1e-14)
    gi = g["grid_idx"]
    for b in (0, 2):
        got = {k: r[k][b, :N].cpu().numpy().astype(np.float64)[gi] for k in ("x", "y", "heading", "curvature", "velocity")}
        e_v = np.max(np.abs(got["velocity"] - g["grid_velocity"]) / g["grid_velocity"])
        e_k = np.max(np.abs(got["curvature"] - g["grid_curvature"]) / np.maximum(np.abs(g["grid_curvature"]), 1e-2))
        e_h = np.max(np.abs(got["heading"] - g["grid_heading"])) / np.pi
        e_x = np.max(np.abs(got["x"] - g["grid_x"]) / np.maximum(np.abs(g["grid_x"]), 1.0))
        e_y = np.max(np.abs(got["y"] - g["grid_y"]) / np.maximum(np.abs(g["grid_y"]), 1.0))
        print(f"{name}/{dtype}: v {e_v:.2e} k {e_k:.2e} h {e_h:.2e} x {e_x:.2e} y {e_y:.2e}")
        assert max(e_v, e_k, e_h, e_x, e_y) <= tol, (e_v, e_k, e_h, e_x, e_y)
    assert torch_mod.equal(r["velocity"][0], r["velocity"][2])


@pytest.mark.parametrize("name", ["feat_reverse", "feat_turn", "feat_mixed", "feat_split2"])
def test_batched_route_fit_and_tables_match_reference(torch_mod, name):
    """The segment rows and the concatenated arc-length table the batched kernels leave on the context, read back
    through the staged pointers: equal to the reference's (the table bit for bit, like the plain one)."""
    import ctypes as C
    torch = torch_mod
    g = gu.load(name)
    gen = make_gen("f64")
    r = run_route(torch, gen, g, copies=2)
    # the context's scratch is not public API; the public check is through the rows above — here: total length,
    # parameters[-1] of the table and the spline count, which depend on every spline's fit and table
    assert r["spline_counts"].tolist() == [int(g["n_splines"])] * 2
    assert float(r["meta"][0, 1]) == float(g["total_length"])
    assert float(r["meta"][0, 0]) == pytest.approx(float(g["lut_parameters"][-1]), rel=1e-15)


@pytest.mark.parametrize("dtype,tol", [("f32", 1e-5), ("f64", 1e-8)])
def test_batched_random_routes_match_oracle(torch_mod, dtype, tol):
    """Random routes — reverse / turn nodes anywhere in 1..W-2 (also adjacent ones: 2-node splines), tangent overrides,
    stops, per-node limits — against the oracle's forward_backward on the reference's grid and on the fixed-S grid."""
    from oracle import oracle
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    torch = torch_mod
    rng = np.random.default_rng(99)
    gen = make_gen(dtype)
    for W, B, use_dd in ((8, 12, True), (5, 9, False), (3, 6, True), (12, 7, False)):
        wp = make_waypoints(B, W, 300 + W).astype(np.float32).astype(np.float64)
        rev = rng.random((B, W)) < 0.25
        turn = np.where(rng.random((B, W)) < 0.25, rng.choice([-135.0, -60.0, 45.0, 90.0, 170.0], size=(B, W)), 0.0)
        rev[:, -1] = False
        turn[:, -1] = 0.0
        tan = np.full((B, W, 2), np.nan)
        mag = np.zeros((B, W, 2))
        for b in range(B):
            for k in range(W):
                if rng.random() < 0.2:
                    a = rng.uniform(0, 2 * np.pi)
                    tan[b, k] = (np.cos(a), np.sin(a))
                    mag[b, k] = rng.uniform(0.3, 1.0, size=2)
        stop = rng.random((B, W)) < 0.15
        stop[:, 0] = stop[:, -1] = False
        mv = np.where(rng.random((B, W)) < 0.3, rng.uniform(1.0, 3.5, (B, W)), 0.0)
        S = 1500
        refs = []
        for b in range(B):
            nodes = dict(is_reverse=rev[b].astype(float), turn=turn[b], stop=stop[b].astype(float), wait_time=np.zeros(W),
                         max_velocity=mv[b], max_acceleration=np.zeros(W), tangent=tan[b], magnitudes=mag[b])
            op = oracle.OraclePath(wp[b], nodes=nodes)
            op.rebuild_tables()
            dd = 0.005 if use_dd else op.dd_for_samples(S)
            refs.append(op.forward_backward(DEFAULT_CONSTRAINTS, dd=dd))
        t = torch.tensor(wp, dtype=gen.tdtype, device=gen.device)
        kw = dict(dd=0.005, capacity=max(len(r["velocity"]) for r in refs) + 4) if use_dd else dict(samples=S)
        r = gen.profile_routes(t, node_reverse=rev, node_turn=turn, node_tangent=tan, node_magnitudes=mag, **kw)
        gen.apply_node_limits(r, DEFAULT_CONSTRAINTS, node_max_velocity=mv, node_stop=stop)
        torch.cuda.synchronize()
        assert not r["flags"].any().item()
        for b in range(B):
            N = len(refs[b]["velocity"])
            assert int(r["meta"][b, 3]) == N, (W, b)
            for k, floor in (("velocity", 0.0), ("curvature", 1e-2), ("x", 1.0), ("y", 1.0)):
                got = r[k][b, :N].cpu().numpy().astype(np.float64)
                err = np.max(np.abs(got - refs[b][k]) / np.maximum(np.abs(refs[b][k]), floor))
                assert err <= (1e-5 if dtype == "f32" else (tol if k == "velocity" else 1e-9)), (W, b, k, err)
            eh = np.max(np.abs(r["heading"][b, :N].cpu().numpy().astype(np.float64) - refs[b]["heading"])) / np.pi
            assert eh <= (1e-5 if dtype == "f32" else 1e-9), (W, b, eh)


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-8), ("f32", 1e-5)])
@pytest.mark.parametrize("name", ["feat_reverse", "feat_turn", "feat_mixed", "feat_split2", "feat_wait", "feat_action", "feat_tangent"])
def test_batched_route_full_motion_profile_matches_reference_golden(torch_mod, name, dtype, tol):
    """generate_motion_profile of the real reference — rows, nodes_map, actions_map — for routes with reverse nodes
    (reversed rows), in-place turns (inserted heading profiles), waits, limits and action points, through the batched
    path.  MPG:389-628."""
    g = gu.load(name)
    gen = make_gen(dtype)
    route = {k: g[k] for k in g.files if k.startswith(("node_", "ap_")) or k == "waypoints"}
    rows, nmap, amap = full_profile(torch_mod, gen, route, [float(v) for v in g["constraints"]])
    T = len(g["profile_times"])
    assert rows.shape[0] == T
    assert nmap == [int(v) for v in g["profile_nodes_map"]]
    assert amap == [int(v) for v in g["profile_actions_map"]]
    for col, key in ((0, "times"), (1, "positions"), (2, "linear_vels"), (3, "accelerations"), (4, "headings"), (5, "angular_vels")):
        ref = g["profile_" + key]
        e = np.abs(rows[:, col] - ref) / np.maximum(np.abs(ref), 1.0)
        assert e.max() <= tol, (key, e.max())
    assert np.max(np.abs(rows[:, 6:8] - g["profile_coords"])) <= tol


def test_batched_random_routes_full_motion_profile_matches_oracle(torch_mod):
    """Random routes with reverse / turn nodes, waits, limits and action points against the oracle's
    generate_motion_profile (row counts, both maps, every row)."""
    from oracle import oracle
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    torch = torch_mod
    rng = np.random.default_rng(808)
    gen = make_gen("f64")
    W = 8
    for it in range(8):
        wp = make_waypoints(1, W, 900 + it)[0].astype(np.float64)
        rev = rng.random(W) < 0.3
        turn = np.where(rng.random(W) < 0.3, rng.choice([-120.0, -45.0, 30.0, 90.0, 175.0], size=W), 0.0)
        rev[-1] = False
        turn[-1] = turn[0] = 0.0
        stop = (rng.random(W) < 0.2).astype(float)
        stop[0] = stop[-1] = 0
        wait = np.where(rng.random(W) < 0.3, rng.uniform(0.05, 0.4, W), 0.0)
        mv = np.where(rng.random(W) < 0.3, rng.uniform(1.0, 3.5, W), 0.0)
        ts = np.sort(rng.uniform(0.3, W - 1.3, size=int(rng.integers(0, 3))))
        route = dict(waypoints=wp, node_is_reverse_node=rev.astype(float), node_turn=turn, node_stop=stop, node_wait_time=wait,
                     node_max_velocity=mv, node_max_acceleration=np.zeros(W), node_tangent=np.full((W, 2), np.nan),
                     node_magnitudes=np.zeros((W, 2)), ap_t=ts, ap_stop=np.zeros(len(ts)), ap_wait_time=rng.uniform(0.0, 0.3, len(ts)),
                     ap_max_velocity=np.zeros(len(ts)), ap_max_acceleration=np.zeros(len(ts)))
        nodes = dict(is_reverse=route["node_is_reverse_node"], turn=turn, stop=stop, wait_time=wait, max_velocity=mv,
                     max_acceleration=np.zeros(W), tangent=route["node_tangent"], magnitudes=route["node_magnitudes"])
        actions = dict(t=ts, stop=route["ap_stop"], wait_time=route["ap_wait_time"], max_velocity=route["ap_max_velocity"],
                       max_acceleration=route["ap_max_acceleration"]) if len(ts) else None
        op = oracle.OraclePath(wp, nodes=nodes, actions=actions)
        ref_rows, ref_nmap, ref_amap = op.generate_motion_profile(DEFAULT_CONSTRAINTS)
        rows, nmap, amap = full_profile(torch, gen, route, list(DEFAULT_CONSTRAINTS))
        assert rows.shape[0] == len(ref_rows), (it, rows.shape[0], len(ref_rows))
        assert nmap == [int(v) for v in ref_nmap] and amap == [int(v) for v in ref_amap], it
        err = np.max(np.abs(rows - ref_rows) / np.maximum(np.abs(ref_rows), 1.0))
        assert err <= 1e-7, (it, err)


def test_bad_routes_are_flagged(torch_mod):
    """A reverse / turn attribute on the LAST node indexes points[W] in the reference (IndexError, SM:97): flagged;
    a turn at node 0 raises there too (quirk Q4): flagged by the time-domain event pass."""
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    torch = torch_mod
    gen = make_gen("f32")
    wp = torch.tensor(make_waypoints(3, 6, 5), dtype=gen.tdtype, device=gen.device)
    rev = np.zeros((3, 6), dtype=bool)
    rev[1, 5] = True
    rev[2, 2] = True
    r = gen.profile_routes(wp, node_reverse=rev, samples=400)
    torch.cuda.synchronize()
    fl = r["flags"].cpu().numpy()
    assert fl[1] & _lib.FLAG_BAD_ROUTE and fl[0] == 0 and fl[2] == 0
    assert r["spline_counts"].tolist() == [1, 1, 2]
    turn = np.zeros((3, 6))
    turn[0, 0] = 30.0
    r = gen.profile_routes(wp, node_turn=turn, dd=0.01, capacity=4000)
    tp = gen.time_profile(r, DEFAULT_CONSTRAINTS)
    gen.insert_waits(r, tp, node_turn=turn)
    torch.cuda.synchronize()
    fl = r["flags"].cpu().numpy()
    assert fl[0] & _lib.FLAG_BAD_ROUTE and fl[1] == 0 and fl[2] == 0
    # the staged entry points that take caller tables know nothing of splines: refused on a batch of routes
    import ctypes as C
    rows = torch.zeros((3, 512, 8), dtype=torch.float64, device=gen.device)
    counts = torch.zeros((3, 2), dtype=torch.int32, device=gen.device)
    nmap = torch.zeros((3, 6), dtype=torch.int32, device=gen.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    c = _lib.make_constraints(DEFAULT_CONSTRAINTS)
    st = gen._L.vap_time_profile(gen.ctx.handle, gen.vdtype, 3, 6, 4000, None, None, p(r["meta"]), p(r["velocity"]), C.byref(c), 0.01, 512,
                                 p(rows), p(counts), p(nmap), p(r["flags"]))
    assert st == _lib.VAP_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_routes_without_splits_equal_the_plain_path_bit_for_bit(torch_mod, dtype):
    """profile_routes on a batch in which no node splits (max_splines == 1) goes through the plain path's kernels:
    the rows equal BatchedTrajectoryGenerator.profile's bit for bit, and node limits / the time domain work on it."""
    torch = torch_mod
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    gen = make_gen(dtype)
    B, W, S = 37, 8, 2000
    wp = torch.tensor(make_waypoints(B, W, 77), dtype=gen.tdtype, device=gen.device)
    plain = {k: v.clone() for k, v in gen.profile(wp, DEFAULT_CONSTRAINTS, samples=S).items()}
    none = np.zeros((B, W), dtype=bool)
    r = gen.profile_routes(wp, node_reverse=none, node_turn=np.zeros((B, W)), constraints=DEFAULT_CONSTRAINTS, samples=S)
    torch.cuda.synchronize()
    assert int(r["spline_counts"].max()) == 1
    for k in ("x", "y", "heading", "curvature", "velocity", "meta", "flags"):
        assert torch.equal(r[k], plain[k]), k
    mv = np.zeros((B, W))
    mv[:, 3] = 2.0
    gen.apply_node_limits(r, DEFAULT_CONSTRAINTS, node_max_velocity=mv)
    tp = gen.time_profile(r, DEFAULT_CONSTRAINTS, dt=0.01, capacity_rows=4096, node_reverse=none)
    torch.cuda.synchronize()
    assert int(tp["counts"][:, 0].min()) > 50 and not r["flags"].any().item()


@pytest.mark.parametrize("dtype,tol", [("f32", 1e-5), ("f64", 1e-8)])
def test_large_batch_of_split_routes_matches_oracle_on_a_sample(torch_mod, dtype, tol):
    """A config-3-shaped batch of routes (1024 x 32 nodes x 6000 samples, ~10 % reverse / turn nodes: 4 splines per route on
    average, up to 10): flags clean, every velocity finite and positive, and 12 random routes against the oracle."""
    from oracle import oracle
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    torch = torch_mod
    rng = np.random.default_rng(2024)
    gen = make_gen(dtype)
    B, W, S = 1024, 32, 6000
    wp = make_waypoints(B, W, 31).astype(np.float32).astype(np.float64)
    rev = rng.random((B, W)) < 0.05
    turn = np.where(rng.random((B, W)) < 0.05, rng.choice([-120.0, -45.0, 60.0, 90.0], size=(B, W)), 0.0)
    rev[:, -1] = False
    turn[:, -1] = turn[:, 0] = 0.0
    r = gen.profile_routes(torch.tensor(wp, dtype=gen.tdtype, device=gen.device), node_reverse=rev, node_turn=turn,
                           constraints=DEFAULT_CONSTRAINTS, samples=S)
    torch.cuda.synchronize()
    assert not r["flags"].any().item()
    assert int(r["spline_counts"].max()) >= 6 and int(r["spline_counts"].min()) >= 1
    v = r["velocity"]
    # (no 0.01 floor here: the cusp at a reverse / turn node has a huge curvature and the reference's cap goes down with it)
    assert torch.isfinite(v).all().item() and float(v.min()) > 0.0 and float(v.max()) <= DEFAULT_CONSTRAINTS[0] * (1 + 1e-6)
    for b in rng.choice(B, size=12, replace=False):
        nodes = dict(is_reverse=rev[b].astype(float), turn=turn[b], stop=np.zeros(W), wait_time=np.zeros(W), max_velocity=np.zeros(W),
                     max_acceleration=np.zeros(W), tangent=np.full((W, 2), np.nan), magnitudes=np.zeros((W, 2)))
        op = oracle.OraclePath(wp[b], nodes=nodes)
        op.rebuild_tables()
        ref = op.forward_backward(DEFAULT_CONSTRAINTS, dd=op.dd_for_samples(S))
        assert len(ref["velocity"]) == S and int(r["meta"][b, 3]) == S
        for k, floor in (("velocity", 0.0), ("curvature", 1e-2), ("x", 1.0), ("y", 1.0)):
            got = r[k][b].cpu().numpy().astype(np.float64)
            err = np.max(np.abs(got - ref[k]) / np.maximum(np.abs(ref[k]), floor))
            assert err <= (tol if k == "velocity" or dtype == "f32" else 1e-9), (int(b), k, err)


def test_widest_route_and_refusals(torch_mod):
    """The route fit keeps 13 doubles and an int per node in LDS: routes of up to 1500 nodes run (held to the oracle on
    a 1500-node route with a reverse and a turn node), wider ones are refused with VAP_ERR_UNSUPPORTED instead of a raw
    launch failure; node_tangent without node_magnitudes and a non-finite node_turn are refused on the host."""
    from oracle import oracle
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    torch = torch_mod
    gen = make_gen("f64")
    W = 1500
    wp = make_waypoints(1, W, 4242).astype(np.float64)
    rev = np.zeros((1, W), dtype=bool)
    turn = np.zeros((1, W))
    rev[0, 700] = True
    turn[0, 1200] = 35.0
    r = gen.profile_routes(torch.tensor(wp, dtype=gen.tdtype, device=gen.device), node_reverse=rev, node_turn=turn,
                           constraints=DEFAULT_CONSTRAINTS, samples=20000)
    torch.cuda.synchronize()
    assert int(r["flags"].abs().max().item()) == 0 and int(r["spline_counts"][0].item()) == 3
    nodes = dict(is_reverse=rev[0].astype(float), turn=turn[0], stop=np.zeros(W), wait_time=np.zeros(W), max_velocity=np.zeros(W),
                 max_acceleration=np.zeros(W), tangent=np.full((W, 2), np.nan), magnitudes=np.zeros((W, 2)))
    op = oracle.OraclePath(wp[0], nodes=nodes)
    op.rebuild_tables()
    assert abs(float(r["meta"][0, 1].item()) - op.total_arc_length()) <= 1e-9 * op.total_arc_length()
    wide = torch.tensor(make_waypoints(1, 1501, 7).astype(np.float64), dtype=gen.tdtype, device=gen.device)
    with pytest.raises(_lib.VapError) as ei:
        gen.profile_routes(wide, constraints=DEFAULT_CONSTRAINTS, samples=4000)
    assert ei.value.status == _lib.VAP_ERR_UNSUPPORTED
    small = torch.tensor(make_waypoints(2, 6, 8).astype(np.float64), dtype=gen.tdtype, device=gen.device)
    with pytest.raises(ValueError):
        gen.profile_routes(small, node_tangent=np.full((2, 6, 2), np.nan), samples=500)
    bad_turn = np.zeros((2, 6))
    bad_turn[1, 2] = np.nan
    with pytest.raises(ValueError):
        gen.profile_routes(small, node_turn=bad_turn, samples=500)


def test_follow_up_calls_refuse_a_superseded_result(torch_mod):
    """apply_node_limits / time_profile read rows the context kept from the profile call that made `result`: a result
    that a later profile call of the same shape has superseded is refused instead of silently mixing two batches."""
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    torch = torch_mod
    gen = make_gen("f32")
    a = torch.tensor(make_waypoints(3, 6, 1).astype(np.float32), device=gen.device)
    b = torch.tensor(make_waypoints(3, 6, 2).astype(np.float32), device=gen.device)
    ra = gen.profile(a, DEFAULT_CONSTRAINTS, samples=600)
    rb = gen.profile(b, DEFAULT_CONSTRAINTS, samples=600)
    with pytest.raises(ValueError):
        gen.apply_node_limits(ra, DEFAULT_CONSTRAINTS, node_max_velocity=np.full((3, 6), 2.0))
    with pytest.raises(ValueError):
        gen.time_profile(ra, DEFAULT_CONSTRAINTS)
    gen.apply_node_limits(rb, DEFAULT_CONSTRAINTS, node_max_velocity=np.full((3, 6), 2.0))
    gen.time_profile(rb, DEFAULT_CONSTRAINTS)
    torch.cuda.synchronize()
