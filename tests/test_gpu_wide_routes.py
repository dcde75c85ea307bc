"""The route pipeline (apply_node_limits -> time_profile -> insert_waits) on paths wide enough to cross its three switches.

  a  k_time_geometry<SEG_LDS, ROUTES> stages the segment rows in LDS up to W = 427 and reads them from global memory from
     428 on: plain paths and routes of both widths, every time kernel, against the host replica (columns 0-3, bit for
     bit) and the oracle (row counts, nodes_map, columns 4-7).
  b  k_limit_fill<R, EV_LDS> keeps the merged event list in LDS up to E = 2047 events: W = 2048 with one and with two
     action points, and W = 6 with 2044 action points the reference skips (k_event_merge's blocked chain).
  c  k_time_waits' dynamic LDS, 44 W + 12 M + 16 bytes: 65 500 B at W = 1488, 65 544 B at 1489, 90 140 B at 2048, the widest
     route (1500 nodes), a coarse step that passes several nodes at once, and a request no workgroup can hold.
  d  caller pointers that are not 16-byte aligned: refused for the rows of 8 doubles, scalar stores for per-sample rows.
Shapes, byte counts, references and the counts asserted before the device is asked come from wide_ref.py, pinned
without a GPU in test_wide_routes_cpu.py.  Bounds: those of test_gpu_time.py (1e-7 fp64, 1e-5 fp32 with the residual,
relative to max(|ref|, 1)) and of test_gpu_routes_batch.py for velocity rows (1e-8 fp64, 1e-5 fp32); nothing new."""
import ctypes as C

import numpy as np
import pytest

import time_ref
import wide_ref as wr
from test_gpu_time import (KERNELS, TRUNCATED, _assert_rows, _replicas, _route_of, _time_profile, _turn_run,  # noqa: F401
                           _wait_run, gens, torch_mod)

pytestmark = pytest.mark.gpu

DEFAULT = wr.DEFAULT
SENTINEL = -7.25                      # exact in fp32 and fp64; no kernel here writes a negative limit, position or count
SAMPLE_CAP = 8192                     # samples of a 428-waypoint path at dd = 0.05: ~5700


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- a. the geometry switch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", wr.GEOMETRY_WIDTHS)
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-7), ("f32", None), ("f32res", 1e-5)])
def test_geometry_switch_on_plain_paths(torch_mod, gens, dtype, tol, W):
    """Three plain paths of 427 (segment rows in LDS) and of 428 waypoints (in global memory) through lane, quad, fused and
    auto at dt = 0.05: rows and nodes_map byte-identical across the four; columns 0-3 and the count bit-equal to
    time_ref.integrate of the device's own velocity row ("f64" and "f32": the replica cannot be fed the residual the
    default fp32 mode keeps on the context, so "f32res" is held to its own four kernels and to the oracle); count,
    nodes_map and all eight columns against the oracle ("f64" at 1e-7, "f32res" at 1e-5).  lane and quad reach
    k_time_geometry<true, false> at 427 and <false, false> at 428."""
    torch = torch_mod
    gen = gens[dtype]
    assert (wr.GEOMETRY_BYTES[W] <= wr.GEOMETRY_LDS_LIMIT) == (W == 427)
    refs = wr.geometry_refs(W)
    wp = torch.tensor(wr.geometry_waypoints(W), device=gen.device, dtype=gen.tdtype)
    res = gen.profile(wp, DEFAULT, dd=wr.DD, capacity=SAMPLE_CAP)
    torch.cuda.synchronize()
    assert not res["flags"].any().item()
    cap = 4096
    flags0 = res["flags"].clone()
    got = {k: _time_profile(torch, gen, res, DEFAULT, wr.DT, cap, k, flags0) for k in KERNELS}
    rows_a, counts_a, nmap_a, flags_a = got["lane"]
    assert not flags_a.any()
    for k in KERNELS[1:]:
        rows_b, counts_b, nmap_b, flags_b = got[k]
        assert np.array_equal(counts_a, counts_b) and np.array_equal(flags_a, flags_b), k
        for b in range(wr.GEOMETRY_PATHS):
            assert rows_a[b, :counts_a[b, 0]].tobytes() == rows_b[b, :counts_a[b, 0]].tobytes(), (k, b)
            assert np.array_equal(nmap_a[b, :counts_a[b, 1]], nmap_b[b, :counts_a[b, 1]]), (k, b)
    if dtype != "f32res":
        for b, (rep, count, truncated) in enumerate(_replicas(res, DEFAULT, wr.DT, cap)):
            assert int(counts_a[b, 0]) == count and not truncated, (b, int(counts_a[b, 0]), count)
            assert np.ascontiguousarray(rows_a[b, :count, :4]).tobytes() == np.ascontiguousarray(rep[:, :4]).tobytes(), b
    if tol is not None:
        for b, (ref, ref_n) in enumerate(refs):
            assert int(counts_a[b, 0]) == ref.shape[0], (b, int(counts_a[b, 0]), ref.shape[0])
            assert [int(v) for v in nmap_a[b, :counts_a[b, 1]]] == [int(v) for v in ref_n], b
            _assert_rows(rows_a[b, :counts_a[b, 0]], ref, tol, wr.DT, ("geometry plain", dtype, W, b))


@pytest.mark.parametrize("W", wr.GEOMETRY_WIDTHS)
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-7), ("f32res", 1e-5)])
def test_geometry_switch_on_routes(torch_mod, gens, dtype, tol, W):
    """Two routes of 427 and of 428 nodes, each with one reverse node and one 35 degree turn node (three splines), through
    profile_routes -> time_profile(node_reverse) with every time kernel setting (k_time_geometry<true, true> at 427,
    <false, true> at 428): rows and nodes_map byte-identical across the settings; then insert_waits(node_turn) against
    the oracle's generate_motion_profile of the same routes: row count, nodes_map, all eight columns."""
    torch = torch_mod
    gen = gens[dtype]
    B = wr.GEOMETRY_ROUTES
    rev, turn = wr.geometry_route_nodes(W)
    refs = wr.geometry_route_refs(W)
    wp = torch.tensor(wr.geometry_route_waypoints(W), device=gen.device, dtype=gen.tdtype)
    res = gen.profile_routes(wp, node_reverse=rev, node_turn=turn, constraints=DEFAULT, dd=wr.DD, capacity=SAMPLE_CAP)
    torch.cuda.synchronize()
    assert not res["flags"].any().item() and res["spline_counts"].tolist() == [3] * B
    cap = 4096
    flags0 = res["flags"].clone()
    got = {}
    for k in KERNELS:
        out = {"rows": torch.full((B, cap, 8), float("nan"), dtype=torch.float64, device=gen.device),
               "counts": torch.full((B, 2), -1, dtype=torch.int32, device=gen.device),
               "nodes_map": torch.full((B, W), -1, dtype=torch.int32, device=gen.device)}
        res["flags"].copy_(flags0)
        gen.set_time_kernel(k)
        try:
            tp = gen.time_profile(res, DEFAULT, dt=wr.DT, capacity_rows=cap, out=out, node_reverse=rev)
            torch.cuda.synchronize()
        finally:
            gen.set_time_kernel("auto")
        got[k] = (tp["rows"].cpu().numpy(), tp["counts"].cpu().numpy(), tp["nodes_map"].cpu().numpy())
        assert not res["flags"].any().item(), k
    rows_a, counts_a, nmap_a = got["lane"]
    for k in KERNELS[1:]:
        rows_b, counts_b, nmap_b = got[k]
        assert np.array_equal(counts_a, counts_b), k
        for b in range(B):
            assert rows_a[b, :counts_a[b, 0]].tobytes() == rows_b[b, :counts_a[b, 0]].tobytes(), (k, b)
            assert np.array_equal(nmap_a[b, :counts_a[b, 1]], nmap_b[b, :counts_a[b, 1]]), (k, b)
    full = gen.insert_waits(res, tp, dt=wr.DT, node_turn=turn, node_reverse=rev, constraints=DEFAULT)
    torch.cuda.synchronize()
    assert not res["flags"].any().item()
    for b, (ref, ref_n) in enumerate(refs):
        rows, nmap, amap = _route_of(full, b)
        assert rows.shape[0] == ref.shape[0], (b, rows.shape[0], ref.shape[0])
        assert nmap == [int(v) for v in ref_n] and amap == [], b
        k = int(np.flatnonzero(turn[b])[0])
        n_ref = _turn_run(ref, int(ref_n[k]))
        assert n_ref > 3 and _turn_run(rows, nmap[k]) == n_ref and rows.shape[0] == int(counts_a[b, 0]) + n_ref
        assert (rows[:, 2] < 0).sum() == (ref[:, 2] < 0).sum() > 100          # the rows behind the reverse node
        _assert_rows(rows, ref, tol, wr.DT, ("geometry routes", dtype, W, b))


# ---- b. the event-list switch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wr.EVENT_CASES))
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-8), ("f32res", 1e-5)])
def test_event_list_switch(torch_mod, gens, dtype, tol, name):
    """apply_node_limits on two paths whose merged event list has E = 2047 entries (the last size k_limit_fill keeps in
    LDS: 49 144 B) and E = 2048 (searched in global memory): 2048 waypoints with max_velocity on ~30 %, max_acceleration
    on ~30 % and a stop on ~5 % of the nodes and one / two action points; and 6 waypoints with 2044 sorted action points,
    nearly all of which the reference never reaches (one pending action point per sample).  node_sample and
    action_sample equal the reference's samples as integers, vcap its initial velocities as fp64 values, the velocity row
    the oracle's forward_backward within 1e-8 (fp64) / 1e-5 (the default fp32 mode)."""
    torch = torch_mod
    c = wr.event_case(name)
    W, M, dd = wr.EVENT_CASES[name]
    E = wr.event_count(W, M)
    assert (wr.event_bytes(E) <= wr.EVENT_LDS_LIMIT) == (name == "w2048_m1")
    # on the reference, before the device is asked
    if W == 2048:
        assert min(c["limited_events"]) >= 1000
    else:
        assert min(c["actions_reached"]) >= 1 and min(c["actions_skipped"]) >= 2000
    gen = gens[dtype]
    B = wr.EVENT_PATHS
    N = [len(v) for v in c["velocity"]]
    wp = torch.tensor(c["waypoints"], device=gen.device, dtype=gen.tdtype)
    res = gen.profile(wp, DEFAULT, dd=dd, capacity=max(N) + 5)
    gen.apply_node_limits(res, DEFAULT, node_max_velocity=c["node_max_velocity"], node_stop=c["node_stop"],
                          node_max_acceleration=c["node_max_acceleration"], action_points=c["action_points"])
    torch.cuda.synchronize()
    assert not res["flags"].any().item()
    assert res["vcap"].dtype == torch.float64
    node_k, ap_k = res["node_sample"].cpu().numpy(), res["action_sample"].cpu().numpy()
    vcap, vel = res["vcap"].cpu().numpy(), res["velocity"].cpu().numpy().astype(np.float64)
    meta = res["meta"].cpu().numpy()
    for b in range(B):
        assert int(meta[b, 3]) == N[b], (b, int(meta[b, 3]), N[b])
        assert np.array_equal(node_k[b].astype(np.int64), c["node_sample"][b]), (b, np.flatnonzero(node_k[b] != c["node_sample"][b])[:8])
        assert np.array_equal(ap_k[b].astype(np.int64), c["action_sample"][b]), (b, np.flatnonzero(ap_k[b] != c["action_sample"][b])[:8])
        bad = np.flatnonzero(vcap[b, :N[b]] != c["vcap"][b])
        assert bad.size == 0, (b, bad[:8], vcap[b, bad[:8]], c["vcap"][b][bad[:8]])
        err = np.max(np.abs(vel[b, :N[b]] - c["velocity"][b]) / c["velocity"][b])
        print(("event list", name, dtype, b), f"velocity max rel err {err:.2e}")
        assert err <= tol, (b, err)


# ---- c. the wait kernel's LDS -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wr.WAIT_CASES))
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-7), ("f32res", 1e-5)])
def test_waits_on_wide_routes(torch_mod, gens, dtype, tol, name):
    """insert_waits where k_time_waits' LDS request crosses 64 KB (W = 1488: 65 500 B, 1489: 65 544 B), at the widest plain
    path (2048: 90 140 B) and the widest route (1500 nodes, two in-place turns), and at a step of 0.25 s that passes two
    nodes at once a dozen times (the reference then records one of them or none: its nodes_map is short and its waits
    move to other nodes — never two nodes on one row).  Waits on about a tenth of the nodes at the values whose
    wait_time / dt rounds just below an integer, one at node 0, an action point's wait one kinematic row behind a node's.
    Row count, both maps and the rows against the oracle; every wait's rows against the pinned integer; the count is
    time_profile's plus the inserted rows."""
    torch = torch_mod
    c = wr.wait_case(name)
    W, dt = c["W"], c["dt"]
    assert wr.WAITS_BYTES[(W, 1)] + wr.WAITS_STATIC_BYTES <= wr.CDNA_MAX_LDS
    coarse = dt != wr.DT
    if coarse:
        assert c["multi_node_steps"] >= wr.COARSE_MULTI_NODE_STEPS_MIN and len(c["nodes_map"]) < W - 1
    steps = (lambda w: wr.COARSE_WAIT_STEPS[w]) if coarse else (lambda w: time_ref.WAIT_EDGE_STEPS[(w, dt)])
    gen = gens[dtype]
    ref, ref_n, ref_a = c["rows"], c["nodes_map"], c["actions_map"]
    wp = torch.tensor(c["waypoints"][None], device=gen.device, dtype=gen.tdtype)
    waits, turns = c["waits"][None], c["turns"][None]
    routed = bool(c["turns"].any())
    aps = [[{"t": float(c["ap"][0]), "wait_time": float(c["ap"][1])}]]
    if routed:
        res = gen.profile_routes(wp, node_turn=turns, constraints=DEFAULT, dd=wr.DD, capacity=30000)
    else:
        res = gen.profile(wp, DEFAULT, dd=wr.DD, capacity=30000)
    gen.apply_node_limits(res, DEFAULT, action_points=aps)
    tp = gen.time_profile(res, DEFAULT, dt=dt, capacity_rows=c["bare_rows"] + 64)
    out = gen.insert_waits(res, tp, node_wait_time=waits, action_points=aps, dt=dt, node_turn=turns if routed else None,
                           constraints=DEFAULT)
    torch.cuda.synchronize()
    assert not res["flags"].any().item()
    rows, nmap, amap = _route_of(out, 0)
    assert rows.shape[0] == ref.shape[0], (rows.shape[0], ref.shape[0])
    assert nmap == [int(v) for v in ref_n], [(i, a, int(b)) for i, (a, b) in enumerate(zip(nmap, ref_n)) if a != int(b)][:8]
    assert amap == [int(v) for v in ref_a], (amap, ref_a)
    turn_rows = 0
    for k in np.flatnonzero(c["turns"]):
        n_ref = _turn_run(ref, int(ref_n[k]))
        assert n_ref > 3 and _turn_run(rows, nmap[k]) == n_ref, (k, n_ref)
        turn_rows += n_ref
    waited = [k for k in range(len(nmap)) if c["waits"][k] > 0]
    assert len(waited) >= 30 and waited[0] == 0
    for k in waited:
        run = _wait_run(rows, nmap[k])
        assert run == _wait_run(ref, int(ref_n[k])), k
        # (at the coarse step an action point's wait may follow a node's on the same row: one run of both)
        assert run == steps(c["waits"][k]) or (coarse and run == steps(c["waits"][k]) + steps(c["ap"][1])), (k, run)
    assert _wait_run(rows, amap[0]) == steps(c["ap"][1])
    inserted = sum(steps(c["waits"][k]) for k in waited) + steps(c["ap"][1]) + turn_rows
    assert rows.shape[0] == int(tp["counts"][0, 0]) + inserted
    if not coarse:      # the node's wait, ONE kinematic row, the action point's wait
        k = c["ap_node"]
        assert amap[0] == nmap[k] + steps(c["waits"][k]) + 1
    _assert_rows(rows, ref, tol, dt, ("waits", name, dtype))


def _small_time_profile(torch, gen, B, W, dt):
    from vexautonomousplanner_amd.synth import make_waypoints
    wp = torch.tensor(make_waypoints(B, W, 620), device=gen.device, dtype=gen.tdtype)
    res = gen.profile(wp, DEFAULT, dd=0.005, capacity=2048)
    tp = gen.time_profile(res, DEFAULT, dt=dt, capacity_rows=512)
    torch.cuda.synchronize()
    assert not res["flags"].any().item() and int(tp["counts"][:, 0].min()) > 20
    return res, tp


def test_waits_refuse_what_no_workgroup_holds(torch_mod, gens):
    """W = 6 with M = 20000 action points asks for 240 280 bytes of dynamic LDS, above any CDNA workgroup's 160 KB: both
    entry points return VAP_ERR_UNSUPPORTED from host code, before any launch (not a raw HIP launch error), the message
    names W, M and the bytes, and nothing is written: the output counts, maps and rows keep their sentinels."""
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    gen = gens["f64"]
    B, W, M, dt = 2, 6, 20000, 0.05
    need = wr.WAITS_BYTES[(W, M)] + wr.WAITS_STATIC_BYTES
    assert need == 240284 > wr.CDNA_MAX_LDS
    res, tp = _small_time_profile(torch, gen, B, W, dt)
    dev = gen.device
    cap_in, cap_out = tp["rows"].shape[1], tp["rows"].shape[1] + 8
    rows_out = torch.full((B, cap_out, 8), SENTINEL, dtype=torch.float64, device=dev)
    counts_out = torch.full((B, 3), -77, dtype=torch.int32, device=dev)
    nmap_out = torch.full((B, W), -77, dtype=torch.int32, device=dev)
    amap_out = torch.full((B, M), -77, dtype=torch.int32, device=dev)
    d_apt = torch.full((B, M), float("inf"), dtype=torch.float64, device=dev)
    d_apw = torch.zeros((B, M), dtype=torch.float64, device=dev)
    flags0 = res["flags"].clone()
    c = _lib.make_constraints(DEFAULT)
    L = _lib.lib()
    gen.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    calls = {
        "vap_time_insert_events": lambda: L.vap_time_insert_events(
            gen.ctx.handle, B, W, M, cap_in, cap_out, dt, C.byref(c), _p(res["meta"]), _p(tp["rows"]), _p(tp["counts"]),
            _p(tp["nodes_map"]), None, None, None, _p(d_apt), _p(d_apw), _p(rows_out), _p(counts_out), _p(nmap_out),
            _p(amap_out), _p(res["flags"])),
        "vap_time_insert_waits": lambda: L.vap_time_insert_waits(
            gen.ctx.handle, B, W, M, cap_in, cap_out, dt, None, None, _p(res["meta"]), _p(tp["rows"]), _p(tp["counts"]),
            _p(tp["nodes_map"]), None, _p(d_apt), _p(d_apw), _p(rows_out), _p(counts_out), _p(nmap_out), _p(amap_out),
            _p(res["flags"])),
    }
    for what, call in calls.items():
        with pytest.raises(_lib.VapError) as ei:
            _lib.check(call(), what)
        assert ei.value.status == _lib.VAP_ERR_UNSUPPORTED, (what, str(ei.value))
        msg = str(ei.value)
        print(what, "->", msg)
        assert "W=6" in msg and "M=20000" in msg and str(need) in msg, msg
    torch.cuda.synchronize()
    assert (counts_out == -77).all().item() and (nmap_out == -77).all().item() and (amap_out == -77).all().item()
    assert (rows_out == SENTINEL).all().item() and torch.equal(res["flags"], flags0)
    # and through the Python layer (padding action points: t = +inf)
    with pytest.raises(_lib.VapError) as ei:
        gen.insert_waits(res, tp, action_points=[[{"t": float("inf")}] * M] * B, dt=dt)
    assert ei.value.status == _lib.VAP_ERR_UNSUPPORTED
    # the context is as usable as before
    ok = gen.insert_waits(res, tp, action_points=[[{"t": 1.5, "wait_time": 0.15}]] * B, dt=dt)
    torch.cuda.synchronize()
    assert ok["counts"][:, 0].tolist() == (tp["counts"][:, 0] + 2).tolist() and ok["counts"][:, 2].tolist() == [1] * B


# ---- d. caller pointers that are not 16-byte aligned ------------------------------------------------------------------
def test_misaligned_row_pointers_are_refused(torch_mod, gens):
    """The rows of 8 doubles move 16 bytes at a time: d_rows_in or d_rows_out at data_ptr() + 8 is refused with
    VAP_ERR_INVALID by vap_time_insert_events and vap_time_insert_waits before any launch — the outputs keep their
    sentinels — and the same call with aligned pointers runs."""
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    gen = gens["f64"]
    B, W, M, dt = 2, 6, 1, 0.05
    res, tp = _small_time_profile(torch, gen, B, W, dt)
    dev = gen.device
    cap_in = tp["rows"].shape[1]
    cap_out = cap_in + 8
    n_in, n_out = B * cap_in * 8, B * cap_out * 8
    buf_in = torch.zeros((n_in + 2,), dtype=torch.float64, device=dev)
    buf_in[1:n_in + 1] = tp["rows"].reshape(-1)
    buf_out = torch.full((n_out + 2,), SENTINEL, dtype=torch.float64, device=dev)
    assert buf_in.data_ptr() % 16 == 0 and buf_out.data_ptr() % 16 == 0 and tp["rows"].data_ptr() % 16 == 0
    counts_out = torch.full((B, 3), -77, dtype=torch.int32, device=dev)
    nmap_out = torch.full((B, W), -77, dtype=torch.int32, device=dev)
    amap_out = torch.full((B, M), -77, dtype=torch.int32, device=dev)
    d_apt = torch.full((B, M), 1.5, dtype=torch.float64, device=dev)
    d_apw = torch.full((B, M), 0.15, dtype=torch.float64, device=dev)
    flags0 = res["flags"].clone()
    c = _lib.make_constraints(DEFAULT)
    L = _lib.lib()
    gen.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def events(rows_in, rows_out):
        return L.vap_time_insert_events(gen.ctx.handle, B, W, M, cap_in, cap_out, dt, C.byref(c), _p(res["meta"]), C.c_void_p(rows_in),
                                        _p(tp["counts"]), _p(tp["nodes_map"]), None, None, None, _p(d_apt), _p(d_apw),
                                        C.c_void_p(rows_out), _p(counts_out), _p(nmap_out), _p(amap_out), _p(res["flags"]))

    def waits(rows_in, rows_out):
        return L.vap_time_insert_waits(gen.ctx.handle, B, W, M, cap_in, cap_out, dt, None, None, _p(res["meta"]), C.c_void_p(rows_in),
                                       _p(tp["counts"]), _p(tp["nodes_map"]), None, _p(d_apt), _p(d_apw), C.c_void_p(rows_out),
                                       _p(counts_out), _p(nmap_out), _p(amap_out), _p(res["flags"]))

    for entry in (events, waits):
        for rows_in, rows_out in ((tp["rows"].data_ptr(), buf_out.data_ptr() + 8), (buf_in.data_ptr() + 8, buf_out.data_ptr())):
            st = entry(rows_in, rows_out)
            assert st == _lib.VAP_ERR_INVALID, (entry.__name__, st)
            assert b"misaligned row pointer" in L.vap_last_error()
    torch.cuda.synchronize()
    assert (buf_out == SENTINEL).all().item() and (counts_out == -77).all().item() and (nmap_out == -77).all().item()
    assert (amap_out == -77).all().item() and torch.equal(res["flags"], flags0)
    _lib.check(events(tp["rows"].data_ptr(), buf_out.data_ptr()), "vap_time_insert_events")
    torch.cuda.synchronize()
    assert counts_out[:, 0].tolist() == (tp["counts"][:, 0] + 2).tolist() and (buf_out[n_out:] == SENTINEL).all().item()


def _offset_rows(torch, names, n, dtype, shift, dev):
    """One buffer per name: 16 bytes of guard, `shift` bytes, n elements, 32 bytes of guard, all holding the sentinel.
    Returns the buffers and, per name, the element at which the n elements start."""
    item = torch.empty((), dtype=dtype).element_size()
    guard, off = 16 // item, shift // item
    bufs = {k: torch.full((guard + off + n + 2 * guard,), SENTINEL, dtype=dtype, device=dev) for k in names}
    for t in bufs.values():
        assert t.data_ptr() % 16 == 0
    return bufs, guard + off, guard


def _rows_and_guards(bufs, start, guard, n):
    out = {}
    for k, t in bufs.items():
        h = t.cpu().numpy()
        assert (h[start - guard:start] == SENTINEL).all(), (k, "the 16 bytes in front of the rows were written")
        assert (h[start + n:start + n + guard] == SENTINEL).all(), (k, "the 16 bytes behind the rows were written")
        out[k] = h[start:start + n].tobytes()
    return out


@pytest.mark.parametrize("dtype,shift", [("f32r32", 4), ("f64", 8)])
def test_limit_rows_at_a_base_that_is_not_16_byte_aligned(torch_mod, gens, dtype, shift):
    """vap_route_limits promises no alignment of d_vcap and the acceleration rows: B = 3 rows of S = 1027 samples (odd, so
    every row has another phase) in a sub-buffer 4 bytes (fp32 rows) / 8 bytes (fp64 rows) behind a 16-byte boundary hold
    the same bytes as in an aligned buffer, and the 16 bytes on either side keep their sentinel.
    What this test cannot show: on this hardware an unaligned 16-byte global store is most likely carried out all the
    same, so the code before the address entered the store predicate might pass as well.  The test holds the contract —
    rows complete, equal, nothing outside them touched; it is no evidence that the earlier code faulted."""
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens["f64"] if dtype == "f64" else BatchedTrajectoryGenerator(0, "f32", recurrence="f32")
    dev = gen.device
    B, W, M, S = 3, 8, 2, 1027
    L = _lib.lib()
    ldt = torch.float64 if L.vap_limit_rows_dtype(gen.ctx.handle, gen.vdtype) == _lib.VAP_F64 else torch.float32
    assert torch.empty((), dtype=ldt).element_size() == shift
    rng = np.random.default_rng(1027)
    res = gen.profile(torch.tensor(make_waypoints(B, W, 1027), device=dev, dtype=gen.tdtype), DEFAULT, samples=S)
    mv = np.where(rng.random((B, W)) < 0.5, rng.uniform(1.0, 3.5, (B, W)), 0.0)
    ma = np.where(rng.random((B, W)) < 0.5, rng.uniform(2.0, 12.0, (B, W)), 0.0)
    stop = (rng.random((B, W)) < 0.3).astype(np.int32)
    stop[:, 0] = stop[:, -1] = 0
    stop[:, 3] = 1
    d = {"mv": torch.tensor(mv, device=dev), "ma": torch.tensor(ma, device=dev), "stop": torch.tensor(stop, device=dev),
         "apt": torch.tensor(np.tile([1.3, 5.6], (B, 1)), device=dev), "apmv": torch.tensor(np.tile([1.5, 0.0], (B, 1)), device=dev),
         "apma": torch.tensor(np.tile([0.0, 6.0], (B, 1)), device=dev),
         "apstop": torch.tensor(np.tile([0, 1], (B, 1)).astype(np.int32), device=dev)}
    dec = torch.zeros((B,), dtype=ldt, device=dev)
    node_k = torch.zeros((B, W), dtype=torch.int32, device=dev)
    ap_k = torch.zeros((B, M), dtype=torch.int32, device=dev)
    c = _lib.make_constraints(DEFAULT)
    gen.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    got = {}
    for sh in (0, shift):
        bufs, start, guard = _offset_rows(torch, ("vcap", "acc_forward", "acc_backward"), B * S, ldt, sh, dev)
        at = lambda k: C.c_void_p(bufs[k].data_ptr() + start * shift)
        assert at("vcap").value % 16 == sh
        _lib.check(L.vap_route_limits(gen.ctx.handle, gen.vdtype, B, W, M, S, None, _p(res["meta"]), _p(d["mv"]), _p(d["ma"]), _p(d["stop"]),
                                      _p(d["apt"]), _p(d["apmv"]), _p(d["apma"]), _p(d["apstop"]), C.byref(c), 0.01, at("vcap"),
                                      at("acc_forward"), at("acc_backward"), _p(dec), _p(node_k), _p(ap_k)), "vap_route_limits")
        torch.cuda.synchronize()
        got[sh] = _rows_and_guards(bufs, start, guard, B * S)
    for k in got[0]:
        assert got[0][k] == got[shift][k], k
    vcap = np.frombuffer(got[shift]["vcap"], dtype=np.float64 if shift == 8 else np.float32).reshape(B, S)
    assert (vcap > 0).all() and (vcap == vcap.dtype.type(0.01)).sum() >= 2 * B and len(np.unique(vcap)) >= 6


@pytest.mark.parametrize("dtype,shift", [("f32res", 4), ("f64", 8)])
def test_route_sampler_rows_at_a_base_that_is_not_16_byte_aligned(torch_mod, gens, dtype, shift):
    """vap_profile_routes promises no alignment of x / y / heading / curvature / velocity: three routes of three splines
    (k_sample_routes), S = 1027, rows 4 bytes (fp32) / 8 bytes (fp64) behind a 16-byte boundary — the same bytes as in
    aligned buffers, sentinels on either side intact.  The limit of this test is that of the one above: an unaligned
    vector store is most likely tolerated by the hardware, so it holds the contract and proves no earlier fault."""
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd.batch import END_VEL, START_VEL
    from vexautonomousplanner_amd.synth import make_waypoints
    torch = torch_mod
    gen = gens[dtype]
    dev = gen.device
    B, W, S = 3, 8, 1027
    assert torch.empty((), dtype=gen.tdtype).element_size() == shift
    wp = torch.tensor(make_waypoints(B, W, 2054), device=dev, dtype=gen.tdtype)
    rev = np.zeros((B, W), dtype=np.int32)
    turn = np.zeros((B, W))
    rev[:, 3], turn[:, 5] = 1, 60.0
    d_rev, d_turn = torch.tensor(rev, device=dev), torch.tensor(turn, device=dev)
    c = _lib.make_constraints(DEFAULT)
    L = _lib.lib()
    gen.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    names = ("x", "y", "heading", "curvature", "velocity")
    got = {}
    for sh in (0, shift):
        bufs, start, guard = _offset_rows(torch, names, B * S, gen.tdtype, sh, dev)
        at = lambda k: C.c_void_p(bufs[k].data_ptr() + start * shift)
        assert at("x").value % 16 == sh
        meta = torch.zeros((B, 4), dtype=torch.float64, device=dev)
        flags = torch.zeros((B,), dtype=torch.int32, device=dev)
        nspl = torch.zeros((B,), dtype=torch.int32, device=dev)
        _lib.check(L.vap_profile_routes(gen.ctx.handle, gen.vdtype, B, W, S, 0.0, 3, _p(wp), _p(d_rev), _p(d_turn), None, None, C.byref(c),
                                        float(START_VEL), float(END_VEL), at("x"), at("y"), at("heading"), at("curvature"),
                                        at("velocity"), _p(meta), _p(flags), _p(nspl)), "vap_profile_routes")
        torch.cuda.synchronize()
        assert not flags.any().item() and nspl.tolist() == [3] * B and (meta[:, 3] == S).all().item()
        got[sh] = _rows_and_guards(bufs, start, guard, B * S)
    for k in names:
        assert got[0][k] == got[shift][k], k
    vel = np.frombuffer(got[shift]["velocity"], dtype=np.float64 if shift == 8 else np.float32)
    assert np.isfinite(vel).all() and (vel > 0).all() and vel.max() > 1.0
