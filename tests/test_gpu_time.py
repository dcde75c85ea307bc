"""The time-domain kernels (vap_time.hip) off the reference's 0.01 s step, and bit for bit.

  a, b  k_time_integrate / k_time_integrate_quad / k_time_fused against the host replica of MPG:566-584 (time_ref.py,
        pinned on the oracle by test_time_cpu.py): equal row counts and equal BYTES of time, position, velocity and
        acceleration.  The kernels' fast loops replace three divisions by reciprocal + correction; the replica divides.
  c     the fp32 rows with the fp64 residual behind them: every kernel the same bits, off 0.01.
  d, e  the whole chain against the oracle's generate_motion_profile off 0.01, inserted rows at the values of
        wait_time / dt that round just below an integer, in-place turns on both branches of the trapezoid.
  f     vap_time_insert_events with a capacity that cuts inside the inserted rows.
Bounds of d and e: 1e-7 (fp64) and 1e-5 (the default fp32 mode) relative to max(|ref|, 1), the project's own; the
acceleration column at steps below 0.01 gets the bound times 0.01 / dt — it is a velocity difference divided by dt, so
the same error of the velocity row weighs 1 / dt.
"""
import ctypes as C

import numpy as np
import pytest

import time_ref

pytestmark = pytest.mark.gpu

DEFAULT = (4.0, 8.0, 8.0, 0.8, 16.0, 12.5 / 12.0)
ROBOTS = [DEFAULT, (4.0, 12.0, 6.0, 0.8, 16.0, 12.5 / 12), (4.0, 6.0, 12.0, 0.8, 16.0, 12.5 / 12)]
SLOW = (1.0, 8.0, 8.0, 0.8, 16.0, 12.5 / 12.0)        # max_vel^2 / max_acc = 0.125 ft: a 90 degree turn is a trapezoid
STEPS = [0.01, 0.02, 0.005, 1 / 60, 0.0125, 0.003, 0.05]
KERNELS = ("lane", "quad", "fused", "auto")
TRUNCATED = 2
CAP_ROWS = 2100


def _id(v):
    return f"{v:.5g}" if isinstance(v, float) else None


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def gens(torch_mod):
    """f64; f32 on the plain fp32 row (the replica can be fed that row); f32res: the default fp32 mode."""
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator as G
    return {"f64": G(0, "f64"), "f32": G(0, "f32", time_domain_residual=False), "f32res": G(0, "f32")}


def _time_profile(torch, gen, res, cons, dt, cap, kernel, flags0):
    """time_profile with the given kernel into buffers that hold NaN / -1 beforehand (memory a former call filled proves
    nothing), the flags as the profile call left them; returns numpy rows, counts, nodes_map, flags."""
    B = res["velocity"].shape[0]
    W = gen._last_shape[1]
    out = {"rows": torch.full((B, cap, 8), float("nan"), dtype=torch.float64, device=gen.device),
           "counts": torch.full((B, 2), -1, dtype=torch.int32, device=gen.device),
           "nodes_map": torch.full((B, W), -1, dtype=torch.int32, device=gen.device)}
    res["flags"].copy_(flags0)
    gen.set_time_kernel(kernel)
    try:
        tp = gen.time_profile(res, cons, dt=dt, capacity_rows=cap, out=out)
        torch.cuda.synchronize()
    finally:
        gen.set_time_kernel("auto")
    return tp["rows"].cpu().numpy(), tp["counts"].cpu().numpy(), tp["nodes_map"].cpu().numpy(), res["flags"].cpu().numpy()


def _replicas(res, cons, dt, cap):
    """time_ref.integrate of every path of the batch, fed the velocity rows and meta as they are on the device."""
    vel = res["velocity"].cpu().numpy()
    meta = res["meta"].cpu().numpy()
    out = []
    for b in range(vel.shape[0]):
        n = int(meta[b, 3]) if np.isfinite(meta[b, 3]) else 0
        out.append(time_ref.integrate(vel[b, :n], meta[b, 1], meta[b, 2], dt, cons[1], cons[2], cap))
    return out


def _assert_bits(torch, gen, res, cons, dt, cap, reps, what):
    flags0 = res["flags"].clone()
    for k in KERNELS:
        rows, counts, _, flags = _time_profile(torch, gen, res, cons, dt, cap, k, flags0)
        for b, (ref, count, truncated) in enumerate(reps):
            assert int(counts[b, 0]) == count, (what, k, b, int(counts[b, 0]), count)
            assert np.ascontiguousarray(rows[b, :count, :4]).tobytes() == np.ascontiguousarray(ref[:, :4]).tobytes(), (what, k, b)
            assert bool(flags[b] & TRUNCATED) == truncated, (what, k, b)


def _batch_19(torch, gen):
    """19 paths of 6 waypoints: one full wavefront of quads and a partly filled one; path 3 has zero length."""
    from vexautonomousplanner_amd.synth import make_waypoints
    wp = make_waypoints(19, 6, 96)
    wp[3] = wp[3, :1]
    return torch.tensor(wp, device=gen.device, dtype=gen.tdtype)


# ---- a. the recurrence bit for bit against the replica ----------------------------------------------------------------
@pytest.mark.parametrize("grid", ["dd", "fixed"])
@pytest.mark.parametrize("dt", STEPS, ids=_id)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_recurrence_equals_the_replica_bit_for_bit(torch_mod, gens, dtype, dt, grid):
    """lane, quad, fused and auto against MPG:566-584 restated with true divisions: equal counts and equal bytes of
    columns 0-3, on the reference's grid (dd = 0.005) and on a fixed grid whose dd_b = L / (S - 1.5) is no round number;
    then with a capacity of 37 rows: the replica's first 37 rows, counts of 37 and the flag."""
    gen = gens[dtype]
    wp = _batch_19(torch_mod, gen)
    res = gen.profile(wp, DEFAULT, dd=0.005, capacity=2048) if grid == "dd" else gen.profile(wp, DEFAULT, samples=700)
    torch_mod.cuda.synchronize()
    assert not (res["flags"].cpu().numpy() & TRUNCATED).any()
    reps = _replicas(res, DEFAULT, dt, CAP_ROWS)
    counts = [r[1] for r in reps]
    assert counts[3] == 0 and min(c for b, c in enumerate(counts) if b != 3) >= 25 and not any(r[2] for r in reps), counts
    _assert_bits(torch_mod, gen, res, DEFAULT, dt, CAP_ROWS, reps, (dtype, dt, grid))
    cut = _replicas(res, DEFAULT, dt, 37)
    assert [r[1] for r in cut] == [min(c, 37) for c in counts] and [r[2] for r in cut] == [c > 37 for c in counts]
    assert sum(r[2] for r in cut) >= 6          # (at 0.05 s the shortest paths have fewer than 37 rows)
    _assert_bits(torch_mod, gen, res, DEFAULT, dt, 37, cut, (dtype, dt, grid, "capacity 37"))


@pytest.mark.parametrize("dt", [0.02, 1 / 60], ids=_id)
@pytest.mark.parametrize("cons", ROBOTS, ids=["default", "acc12_dec6", "acc6_dec12"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_recurrence_equals_the_replica_other_robots(torch_mod, gens, dtype, cons, dt):
    """max_dec != max_acc (the time loop is where max_dec acts, MPG:573-575), at two steps off 0.01."""
    gen = gens[dtype]
    res = gen.profile(_batch_19(torch_mod, gen), cons, dd=0.005, capacity=2048)
    torch_mod.cuda.synchronize()
    reps = _replicas(res, cons, dt, CAP_ROWS)
    assert not any(r[2] for r in reps)
    _assert_bits(torch_mod, gen, res, cons, dt, CAP_ROWS, reps, (dtype, cons, dt))


# ---- b. rows the velocity pass never produces -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0.05, 0.02], ids=_id)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_recurrence_on_rows_the_velocity_pass_never_produces(torch_mod, gens, dtype, dt):
    """The API integrates the row as the caller left it: rows written in place into the result before the call, which
    take the branches a forward-backward row never does, against the replica bit for bit on all four kernels.
      0  constant 0.05: every step takes the `current_vel <= 0.1` branch (MPG:581-582)
      1  all zeros: the target velocity sits at the 0.001 floor, the position creeps at 0.1 * dt
      2  0.5 / 4.0 on alternate samples (the mean of the two lerps one sample apart is then the same everywhere)
      3  0.5 / 4.0 in blocks of eight samples: with max_dec != max_acc both acceleration clips act
      4  a single spike
      5  the velocity pass's own row"""
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens[dtype]
    cons = ROBOTS[1]                                    # max_acc 12, max_dec 6
    wp = torch.tensor(make_waypoints(6, 3, 55), device=gen.device, dtype=gen.tdtype)
    res = gen.profile(wp, cons, dd=0.005, capacity=512)
    torch.cuda.synchronize()
    meta = res["meta"].cpu().numpy()
    vel = res["velocity"].cpu().numpy().copy()
    n = meta[:, 3].astype(int)
    assert (n >= 100).all() and (n <= 512).all()
    i = np.arange(512)
    vel[0, :] = 0.05
    vel[1, :] = 0.0
    vel[2, :] = np.where(i % 2 == 0, 0.5, 4.0)
    vel[3, :] = np.where((i // 8) % 2 == 0, 0.5, 4.0)
    vel[4, :] = 0.5
    vel[4, n[4] // 2] = 4.0
    res["velocity"].copy_(torch.tensor(vel, device=gen.device, dtype=gen.tdtype))     # in place: the same rows, edited
    reps = _replicas(res, cons, dt, CAP_ROWS)
    assert not any(r[2] for r in reps), [r[1] for r in reps]
    assert (reps[0][0][:, 2] <= 0.1).all() and reps[0][1] > 20
    assert (reps[1][0][:, 4] == 0.001).all() and reps[1][1] > 100
    acc = reps[3][0][:, 3]
    n_up, n_down = int((acc == cons[1]).sum()), int((acc == -cons[2]).sum())
    assert n_up >= 1 and n_down >= 1 and n_up + n_down > len(acc) / 2, (n_up, n_down, len(acc))
    _assert_bits(torch, gen, res, cons, dt, CAP_ROWS, reps, (dtype, dt))


# ---- c. the fp32 residual path off 0.01 -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,W,S,caps", [(1, 4, 900, (CAP_ROWS,)), (17, 6, 1500, (CAP_ROWS,)), (67, 5, 700, (CAP_ROWS, 60))])
@pytest.mark.parametrize("dt", [0.02, 1 / 60, 0.003], ids=_id)
def test_residual_mode_kernels_agree_off_the_default_step(torch_mod, gens, dt, B, W, S, caps):
    """The default fp32 mode (fp32 rows + the fp64 recurrence's residual on the context): lane, quad, fused and auto
    give the same counts, maps, flags and row bytes — all eight columns — at steps off 0.01, for batches that leave quads
    and wavefronts partly empty, a path of zero length and a capacity that truncates."""
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens["f32res"]
    wp_np = make_waypoints(B, W, 77 + B)
    if B == 17:
        wp_np[3] = wp_np[3, :1]
    res = gen.profile(torch.tensor(wp_np, device=gen.device, dtype=gen.tdtype), DEFAULT, samples=S)
    flags0 = res["flags"].clone()
    for cap in caps:
        got = {k: _time_profile(torch, gen, res, DEFAULT, dt, cap, k, flags0) for k in KERNELS}
        rows_a, counts_a, nm_a, flags_a = got["lane"]
        live = np.delete(counts_a, 3, axis=0) if B == 17 else counts_a
        if B == 17:
            assert counts_a[3, 0] == 0 and counts_a[3, 1] == 1
        if cap == 60:
            assert (counts_a[:, 0] == 60).all() and (flags_a & TRUNCATED).all()
        else:
            assert live[:, 0].min() >= 60 and not (flags_a & TRUNCATED).any()
        for k in KERNELS[1:]:
            rows_b, counts_b, nm_b, flags_b = got[k]
            assert np.array_equal(counts_a, counts_b) and np.array_equal(flags_a, flags_b), (k, cap)
            for b in range(B):
                assert rows_a[b, :counts_a[b, 0]].tobytes() == rows_b[b, :counts_a[b, 0]].tobytes(), (k, cap, b)
                assert np.array_equal(nm_a[b, :counts_a[b, 1]], nm_b[b, :counts_a[b, 1]]), (k, cap, b)


# ---- d. the whole chain against the oracle off 0.01 -------------------------------------------------------------------
def _bounds(tol, dt):
    b = np.full(8, tol)
    if dt < 0.01:
        b[3] = tol * (0.01 / dt)
    return b


def _assert_rows(got, ref, tol, dt, what):
    assert got.shape[0] == ref.shape[0], (what, got.shape[0], ref.shape[0])
    err = (np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max(axis=0) if ref.shape[0] else np.zeros(8)
    print(what, "max error per column", " ".join(f"{e:.2e}" for e in err))
    assert (err <= _bounds(tol, dt)).all(), (what, err)


@pytest.mark.parametrize("dt", [0.02, 0.005, 1 / 60, 0.003], ids=_id)
@pytest.mark.parametrize("W", [5, 8, 32])
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-7), ("f32res", 1e-5)])
def test_chain_matches_the_oracle_off_the_default_step(torch_mod, gens, dtype, tol, W, dt):
    """profile(dd = 0.005) -> time_profile(dt) for six random paths against generate_motion_profile(dt): row count,
    nodes_map and all eight columns.  (The 32-waypoint paths need up to 4453 rows at 0.003.)"""
    from oracle import oracle
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens[dtype]
    wp = make_waypoints(6, W, 400 + W)                 # fp32 values: the same waypoints for both types and the oracle
    res = gen.profile(torch.tensor(wp, device=gen.device, dtype=gen.tdtype), DEFAULT, dd=0.005, capacity=16384)
    rows, counts, nmap, flags = _time_profile(torch, gen, res, DEFAULT, dt, CAP_ROWS if W < 32 else 4608, "auto", res["flags"].clone())
    assert not flags.any()
    for b in range(6):
        ref, ref_n, _ = oracle.OraclePath(wp[b].astype(np.float64)).generate_motion_profile(DEFAULT, dt=dt, dd=0.005)
        assert int(counts[b, 0]) == ref.shape[0], (b, int(counts[b, 0]), ref.shape[0])
        assert [int(v) for v in nmap[b, :counts[b, 1]]] == [int(v) for v in ref_n], b
        _assert_rows(rows[b, :counts[b, 0]], ref, tol, dt, (dtype, W, dt, b))


@pytest.mark.parametrize("dt", [0.01, 0.02], ids=_id)
def test_fp32_sweep_of_64_paths_matches_the_oracle(torch_mod, gens, dt):
    """The default fp32 mode on 64 paths of 8 waypoints: every path's row count, nodes_map and rows to 1e-5."""
    from oracle import oracle
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens["f32res"]
    wp = make_waypoints(64, 8, 914)
    res = gen.profile(torch.tensor(wp, device=gen.device, dtype=gen.tdtype), DEFAULT, dd=0.005, capacity=16384)
    rows, counts, nmap, flags = _time_profile(torch, gen, res, DEFAULT, dt, CAP_ROWS, "auto", res["flags"].clone())
    assert not flags.any()
    for b in range(64):
        ref, ref_n, _ = oracle.OraclePath(wp[b].astype(np.float64)).generate_motion_profile(DEFAULT, dt=dt, dd=0.005)
        assert [int(v) for v in nmap[b, :counts[b, 1]]] == [int(v) for v in ref_n], b
        _assert_rows(rows[b, :counts[b, 0]], ref, 1e-5, dt, ("f32 sweep", dt, b))


# ---- e. inserted rows at rounding edges and off 0.01 ------------------------------------------------------------------
def _oracle_route(wp, wait, turn, aps, cons, dt):
    from oracle import oracle
    W = len(wp)
    nodes = dict(is_reverse=np.zeros(W), turn=turn, stop=np.zeros(W), wait_time=wait, max_velocity=np.zeros(W),
                 max_acceleration=np.zeros(W), tangent=np.full((W, 2), np.nan), magnitudes=np.zeros((W, 2)))
    actions = None
    if aps:
        M = len(aps)
        actions = dict(t=np.array([a[0] for a in aps]), stop=np.zeros(M), wait_time=np.array([a[1] for a in aps]),
                       max_velocity=np.zeros(M), max_acceleration=np.zeros(M))
    return oracle.OraclePath(wp, nodes=nodes, actions=actions).generate_motion_profile(cons, dt=dt, dd=0.005)


def _gpu_routes(torch, gen, wps, waits, turns, aps, cons, dt):
    """profile_routes -> apply_node_limits -> time_profile -> insert_waits for a batch of routes; returns the result of
    profile_routes, the kinematic rows' dict and the dict of insert_waits."""
    wp = torch.tensor(np.asarray(wps), device=gen.device, dtype=gen.tdtype)
    ap_dicts = [[{"t": float(t), "wait_time": float(w)} for t, w in al] for al in aps]
    res = gen.profile_routes(wp, node_turn=np.asarray(turns), constraints=cons, dd=0.005, capacity=4096)
    gen.apply_node_limits(res, cons, action_points=ap_dicts)
    tp = gen.time_profile(res, cons, dt=dt, capacity_rows=CAP_ROWS)
    out = gen.insert_waits(res, tp, node_wait_time=np.asarray(waits), action_points=ap_dicts, dt=dt,
                           node_turn=np.asarray(turns), constraints=cons)
    torch.cuda.synchronize()
    return res, tp, out


def _route_of(out, b):
    T, nn, na = (int(v) for v in out["counts"][b])
    return (out["rows"][b, :T].cpu().numpy(), [int(v) for v in out["nodes_map"][b, :nn]],
            [int(v) for v in out["actions_map"][b, :na]])


def _wait_run(rows, start):
    """Rows of a wait from `start` on: position, velocity and acceleration exactly 0 (MPG:511-513; a kinematic row's
    position is above 0, a turn's rows keep the last position)."""
    n = 0
    while start + n < len(rows) and rows[start + n, 1] == 0.0 and rows[start + n, 2] == 0.0 and rows[start + n, 3] == 0.0:
        n += 1
    return n


def _turn_run(rows, start):
    """Rows of an in-place turn from `start` on: zero velocity at the position of the row before (MPG:499-501)."""
    n = 0
    while start + n < len(rows) and rows[start + n, 1] == rows[start - 1, 1] and rows[start + n, 2] == 0.0:
        n += 1
    return n


@pytest.mark.parametrize("dt", [0.01, 0.05, 0.1, 0.02], ids=_id)
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-7), ("f32res", 1e-5)])
def test_waits_at_rounding_edges_match_the_oracle(torch_mod, gens, dtype, tol, dt):
    """Node and action-point waits whose wait_time / dt rounds just below an integer (0.29 / 0.01 = 28.999..., the
    reference's int() drops a row) or is exact, at four steps: a wait at node 0, an action point one row behind a
    node's wait, waits further on.  Row count, both maps and the rows against the oracle; each wait's inserted rows
    against the integer Python gives (pinned in test_time_cpu.py)."""
    from oracle import oracle
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens[dtype]
    ws = [w for (w, d) in time_ref.WAIT_EDGE_STEPS if d == dt]
    steps = lambda w: time_ref.WAIT_EDGE_STEPS[(w, dt)]
    pick = lambda i: ws[i % len(ws)]
    W = 6
    wps = make_waypoints(2, W, 620).astype(np.float64)
    # the action point behind node 3 of route 0: between the parameters of the row at which the node is passed and the next
    plain = oracle.OraclePath(wps[0])
    p_rows, p_nmap, _ = plain.generate_motion_profile(DEFAULT, dt=dt, dd=0.005)
    plain.rebuild_tables()
    r = int(p_nmap[3])
    assert 0 < r < len(p_rows) - 1
    t_r, t_next = plain.distance_to_time(p_rows[r - 1, 1]), plain.distance_to_time(p_rows[r, 1])
    assert 3.0 < t_r < t_next < 4.0
    waits = np.zeros((2, W))
    waits[0, 0], waits[0, 2], waits[0, 3] = pick(0), pick(1), pick(2)
    waits[1, 1], waits[1, 4] = pick(1), pick(3)
    aps = [[(1.4, pick(3)), (0.5 * (t_r + t_next), pick(0))], [(0.6, pick(2))]]
    turns = np.zeros((2, W))
    res, tp, out = _gpu_routes(torch, gen, wps, waits, turns, aps, DEFAULT, dt)
    assert not res["flags"].any().item()
    for b in range(2):
        ref, ref_n, ref_a = _oracle_route(wps[b], waits[b], turns[b], aps[b], DEFAULT, dt)
        rows, nmap, amap = _route_of(out, b)
        assert rows.shape[0] == ref.shape[0], (b, rows.shape[0], ref.shape[0])
        assert nmap == [int(v) for v in ref_n] and amap == [int(v) for v in ref_a], (b, nmap, amap)
        assert len(nmap) >= W - 1 and len(amap) == len(aps[b])     # (at coarse steps the reference records the last node too)
        for k in range(W - 1):
            if waits[b, k] > 0:
                assert _wait_run(rows, nmap[k]) == steps(waits[b, k]), (b, k, waits[b, k])
        for j, (_, w) in enumerate(aps[b]):
            assert _wait_run(rows, amap[j]) == steps(w), (b, j, w)
        inserted = sum(steps(w) for w in waits[b] if w > 0) + sum(steps(w) for _, w in aps[b])
        assert rows.shape[0] == int(tp["counts"][b, 0]) + inserted
        _assert_rows(rows, ref, tol, dt, (dtype, dt, b))
    # route 0: the node's wait, ONE kinematic row, the action point's wait
    _, nmap, amap = _route_of(out, 0)
    assert amap[1] == nmap[3] + steps(waits[0, 3]) + 1


@pytest.mark.parametrize("dt", [0.01, 0.02, 0.005, 0.0125], ids=_id)
@pytest.mark.parametrize("cons", [DEFAULT, SLOW], ids=["default", "max_vel_1"])
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-7), ("f32res", 1e-5)])
def test_turns_match_the_oracle_off_the_default_step(torch_mod, gens, dtype, tol, cons, dt):
    """In-place turns of 17, +-90, 180 and 270 degrees (one with a wait on the same node, one route with a wait at node 0):
    the rows of np.arange(0, total_time + dt, dt) as an integer, the maps and the rows against the oracle.  The default
    robot's turns below ~220 degrees are triangular profiles; with max_vel = 1 a 90 degree turn is a trapezoid."""
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens[dtype]
    arc, two_d_acc = np.radians(90.0) * cons[5] / 2, cons[0] ** 2 / cons[1]
    assert (two_d_acc > arc) == (cons is DEFAULT)                      # ODM:16: which branch a 90 degree turn takes
    W = 5
    wps = make_waypoints(2, W, 733).astype(np.float64)
    turns = np.array([[0.0, 17.0, 90.0, -90.0, 0.0], [0.0, 180.0, 270.0, 0.0, 0.0]])
    waits = np.zeros((2, W))
    waits[0, 2] = 0.13                                                 # a turn and a wait on the same node
    waits[1, 0] = 0.07                                                 # a wait at node 0
    aps = [[], [(2.5, 0.06)]]
    res, tp, out = _gpu_routes(torch, gen, wps, waits, turns, aps, cons, dt)
    assert not res["flags"].any().item()
    for b in range(2):
        ref, ref_n, ref_a = _oracle_route(wps[b], waits[b], turns[b], aps[b], cons, dt)
        rows, nmap, amap = _route_of(out, b)
        assert rows.shape[0] == ref.shape[0], (b, rows.shape[0], ref.shape[0])
        assert nmap == [int(v) for v in ref_n] and amap == [int(v) for v in ref_a], (b, nmap, amap)
        for k in range(1, W - 1):
            if turns[b, k] != 0:
                n_ref = _turn_run(ref, int(ref_n[k]))
                assert n_ref > 3 and _turn_run(rows, nmap[k]) == n_ref, (b, k, _turn_run(rows, nmap[k]), n_ref)
                if waits[b, k] > 0:
                    assert _wait_run(rows, nmap[k] + n_ref) == int(waits[b, k] / dt) == _wait_run(ref, int(ref_n[k]) + n_ref)
        _assert_rows(rows, ref, tol, dt, (dtype, cons[0], dt, b))


# ---- f. truncated inserts ---------------------------------------------------------------------------------------------
def test_truncated_inserts_keep_the_rows_below_the_capacity(torch_mod, gens):
    """vap_time_insert_events with a capacity_out below what the waits and turns need, cutting inside a wait, inside a
    turn, in kinematic rows behind an event and exactly at an event's first row: the rows below the capacity are those
    of a call with ample capacity bit for bit, counts are min(count, capacity), VAP_FLAG_TRUNCATED is set on the routes
    that were cut and on no other, and both maps are those of the ample call (they may then hold rows at or above the
    capacity: include/vap.h).  Through the C-ABI with a caller-owned buffer, nothing behind a route's rows is written."""
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens["f64"]
    dt, B, W = 0.01, 3, 5
    wps = make_waypoints(B, W, 871).astype(np.float64)
    wps[2] = wps[2, :1] + 0.6 * (wps[2] - wps[2, :1])                  # a shorter route
    turns = np.zeros((B, W))
    turns[:, 2] = 90.0
    waits = np.zeros((B, W))
    waits[:, 1], waits[:, 3] = 0.13, 0.21
    aps = [[(0.5, 0.05)] for _ in range(B)]
    res, tp, ample = _gpu_routes(torch, gen, wps, waits, turns, aps, DEFAULT, dt)
    assert not res["flags"].any().item()
    flags0 = res["flags"].clone()
    a_rows, a_counts = ample["rows"].cpu().numpy(), ample["counts"].cpu().numpy()
    a_nmap, a_amap = ample["nodes_map"].cpu().numpy(), ample["actions_map"].cpu().numpy()
    full = a_counts[:, 0]
    assert len(set(full.tolist())) == 3 and (a_counts[:, 1] == W - 1).all() and (a_counts[:, 2] == 1).all()
    nm = a_nmap[0]
    r0 = a_rows[0, :full[0]]
    n_wait, n_turn = _wait_run(r0, nm[1]), _turn_run(r0, nm[2])
    assert n_wait == 13 and n_turn > 20 and nm[3] - 3 > nm[2] + n_turn
    caps = {"inside a wait": int(nm[1]) + 5, "at an event's first row": int(nm[2]), "inside a turn": int(nm[2]) + 7,
            "kinematic rows behind an event": int(nm[3]) - 3, "the shortest route's count": int(full.min())}
    ap_dicts = [[{"t": t, "wait_time": w} for t, w in al] for al in aps]

    def check(cap, rows, counts, nmap, amap, flags, what):
        want = np.minimum(full, cap)
        assert np.array_equal(counts[:, 0], want), (what, counts[:, 0], want)
        assert np.array_equal(counts[:, 1:], a_counts[:, 1:]), what
        assert np.array_equal((flags & TRUNCATED) != 0, full > cap), (what, flags, full)
        assert np.array_equal(nmap, a_nmap) and np.array_equal(amap, a_amap), what
        for b in range(B):
            assert rows[b, :want[b]].tobytes() == a_rows[b, :want[b]].tobytes(), (what, b)

    for what, cap in caps.items():
        res["flags"].copy_(flags0)
        out = gen.insert_waits(res, tp, node_wait_time=waits, action_points=ap_dicts, dt=dt, capacity_rows=cap,
                               node_turn=turns, constraints=DEFAULT)
        torch.cuda.synchronize()
        assert (full > cap).any() and out["rows"].shape[1] == cap
        check(cap, out["rows"].cpu().numpy(), out["counts"].cpu().numpy(), out["nodes_map"].cpu().numpy(),
              out["actions_map"].cpu().numpy(), res["flags"].cpu().numpy(), what)

    # the C-ABI, caller-owned buffers: B routes of `cap` rows and one route's worth of rows behind them
    cap = caps["inside a turn"]
    sentinel = -7.25e300
    dev = gen.device
    rows_out = torch.full((B + 1, cap, 8), sentinel, dtype=torch.float64, device=dev)
    counts_out = torch.full((B, 3), -1, dtype=torch.int32, device=dev)
    nmap_out = torch.zeros((B, W), dtype=torch.int32, device=dev)
    amap_out = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    d_wait, d_turn = torch.tensor(waits, device=dev), torch.tensor(turns, device=dev)
    d_apt = torch.tensor([[al[0][0]] for al in aps], dtype=torch.float64, device=dev)
    d_apw = torch.tensor([[al[0][1]] for al in aps], dtype=torch.float64, device=dev)
    res["flags"].copy_(flags0)
    p = lambda t: C.c_void_p(t.data_ptr())
    c = _lib.make_constraints(DEFAULT)
    gen.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib().vap_time_insert_events(gen.ctx.handle, B, W, 1, tp["rows"].shape[1], cap, dt, C.byref(c), p(res["meta"]),
                                                 p(tp["rows"]), p(tp["counts"]), p(tp["nodes_map"]), p(d_wait), p(d_turn), None,
                                                 p(d_apt), p(d_apw), p(rows_out), p(counts_out), p(nmap_out), p(amap_out),
                                                 p(res["flags"])), "vap_time_insert_events")
    torch.cuda.synchronize()
    got = rows_out.cpu().numpy()
    assert (got[B] == sentinel).all(), "rows behind the last route's capacity were written"
    counts = counts_out.cpu().numpy()
    check(cap, got[:B], counts, nmap_out.cpu().numpy(), amap_out.cpu().numpy(), res["flags"].cpu().numpy(), "C-ABI")
    for b in range(B):
        assert (got[b, counts[b, 0]:] == sentinel).all(), b          # nor any row behind a route's count
