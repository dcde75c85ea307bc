"""GPU: scene clearance of the disturbed rollouts (vap_rollout_clearance, tracking.rollout_clearance,
BatchedTrajectoryGenerator.rollout_clearance, search.refine(robust_clearance=True)).

The contract is a composition, and the tests hold it bit for bit: per rollout the five clearance numbers are those of
``tracking.rollouts(executed=True)`` followed by ``footprint.clearance`` on its executed rows; the per-route outputs are
the ascending-k fold of the call's own per-rollout outputs; the follower's outputs are those of plain ``rollouts``.  Against
the NumPy composition of tests/rollout_clearance_ref.py the golden routes are held to the rule test_gpu_tracking.py uses
for the clearance of executed rows: 1e-9 ft, the row may be any row within 1e-9 of the minimum, counts are compared where
no row is within 1e-9 of the margin; a RAMSETE rollout whose reference max |e_phi| >= 3.0 rad sits at the wrap's
discontinuity and is left out of that comparison, at most 2 % of a test's rollouts."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import pursuit_ref as pr
import rollout_clearance_ref as rc
import tracking_ref as tr

pytestmark = pytest.mark.gpu

DT = 0.01
AMBIGUOUS = 1e-9
EXCLUDE_RAD = 3.0
FOLLOWER_KEYS = {"ramsete": ("stats", "stat_rows", "worst", "mean", "worst_rollout", "worst_row", "n_exceeding"),
                 "pursuit": ("stats", "stat_rows", "worst", "mean", "worst_rollout", "worst_row", "n_exceeding", "n_unfinished",
                             "route_status")}
ROUTE_KEYS = ("worst_clearance", "worst_clear_rollout", "worst_clear_row", "worst_clear_element", "mean_clearance", "n_colliding",
              "n_clear_valid")
CLEAR_KEYS = ("clearance", "clear_rows") + ROUTE_KEYS


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def trk():
    from vexautonomousplanner_amd import tracking
    return tracking


def FP():
    from vexautonomousplanner_amd import footprint
    return footprint


def make_follower(kind, **kw):
    return (trk().Follower if kind == "ramsete" else trk().Pursuit)(**kw)


def bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def assert_same_bits(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=f"{what}: {k}")


def check_against_pipeline(torch, kind, fused, rows, counts, follower, P, foot, scene, margin, ctx=None):
    """The fused call's outputs against the two-call pipeline's and plain rollouts', bit for bit, and its per-route outputs
    against the fold of its own per-rollout ones.  Returns the pipeline's clearance dict."""
    tk, fp = trk(), FP()
    ex = tk.rollouts(rows, counts, follower, P, time_step=DT, executed=True, ctx=ctx)
    cl = fp.clearance(ex["rows"], ex["counts"], foot, scene, margin=margin, ctx=ctx)
    plain = tk.rollouts(rows, counts, follower, P, time_step=DT, ctx=ctx)
    torch.cuda.synchronize()
    B, K = fused["clearance"].shape
    assert fused["clear_rows"].shape == (B, K, 4) and ex["rows"].shape[0] == B * K
    np.testing.assert_array_equal(bits(fused["clearance"]), bits(cl["min_clearance"].view(B, K)), err_msg="clearance")
    want = torch.stack([cl["min_row"], cl["min_element"], cl["first_row"], cl["n_below"]], dim=1).view(B, K, 4)
    np.testing.assert_array_equal(bits(fused["clear_rows"]), bits(want), err_msg="clear_rows")
    for i, name in enumerate(tk.CLEAR_ROW_COLUMNS):
        assert torch.equal(fused[name], fused["clear_rows"][..., i])
    assert_same_bits(fused, plain, FOLLOWER_KEYS[kind], "follower outputs against plain rollouts")
    assert_same_bits(fused, ex, FOLLOWER_KEYS[kind], "follower outputs against rollouts(executed=True)")
    c, r = fused["clearance"].cpu().numpy(), fused["clear_rows"].cpu().numpy()
    got = {k: fused[k].cpu().numpy() for k in ROUTE_KEYS}
    for b in range(B):
        s = rc.fold(c[b], r[b], margin)
        for k in ROUTE_KEYS:
            np.testing.assert_array_equal(got[k][b], s[k], err_msg=f"route {b}: {k}")       # NaN equals NaN, else exact
    return cl


# ---- 1. bit for bit against the two-call pipeline: layouts, edge cases -------------------------------------------------
@pytest.mark.parametrize("kind,K,B,seed", rc.LAYOUTS)
def test_bits_against_the_two_call_pipeline(torch_mod, kind, K, B, seed):
    torch = torch_mod
    tk, fp = trk(), FP()
    rows, counts, P = rc.layout_case(kind, K, B)
    field, polygons, circles = rc.layout_scene(rows, counts, seed)
    scene = fp.Scene(field=field, polygons=polygons, circles=circles)
    foot = fp.rectangle(18, 18)
    follower = make_follower(kind, settle_rows=20, n_substeps=3, tolerance=0.1)
    d_rows, d_counts = torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0")
    fused = tk.rollout_clearance(d_rows, d_counts, follower, P, foot, scene, margin=rc.MARGIN, time_step=DT)
    again = tk.rollout_clearance(d_rows, d_counts, follower, torch.tensor(P, device="cuda:0"), foot, scene, margin=rc.MARGIN, time_step=DT)
    nocull = tk.rollout_clearance(d_rows, d_counts, follower, P, foot, scene, margin=rc.MARGIN, time_step=DT, cull=False)
    torch.cuda.synchronize()
    check_against_pipeline(torch, kind, fused, d_rows, d_counts, follower, P, foot, scene, rc.MARGIN)
    assert_same_bits(fused, again, FOLLOWER_KEYS[kind] + CLEAR_KEYS, "two calls")
    assert_same_bits(fused, nocull, FOLLOWER_KEYS[kind] + CLEAR_KEYS, "cull off")
    # shared records: (K, 8) for every route equals the same records repeated per route
    Ps = P[B - 1].copy()
    shared = tk.rollout_clearance(d_rows, d_counts, follower, Ps, foot, scene, margin=rc.MARGIN, time_step=DT)
    repeated = tk.rollout_clearance(d_rows, d_counts, follower, np.repeat(Ps[None], B, axis=0), foot, scene, margin=rc.MARGIN, time_step=DT)
    torch.cuda.synchronize()
    assert_same_bits(shared, repeated, FOLLOWER_KEYS[kind] + CLEAR_KEYS, "shared records")
    # the edge outputs are the header's (that the scene is neither empty nor all-colliding is held on the reference, on the CPU)
    c = fused["clearance"].cpu().numpy()
    ncol, nval = fused["n_colliding"].cpu().numpy(), fused["n_clear_valid"].cpu().numpy()
    e = B // 2                                                                      # a route without rows
    assert torch.isnan(fused["clearance"][e]).all() and (fused["clear_rows"][e, :, :3] == -1).all() and (fused["clear_rows"][e, :, 3] == 0).all()
    assert torch.isnan(fused["worst_clearance"][e]) and torch.isnan(fused["mean_clearance"][e])
    assert [int(fused[k][e]) for k in ("worst_clear_rollout", "worst_clear_row", "worst_clear_element", "n_colliding", "n_clear_valid")] == [-1, -1, -1, 0, 0]
    if K >= 3:
        assert torch.isnan(fused["clearance"][:, K // 2]).all() and (fused["clear_rows"][:, K // 2, 0] == -1).all()
        assert (fused["worst_clear_rollout"] != K // 2).all()
    else:
        assert torch.isnan(fused["worst_clearance"][3]) and int(fused["n_clear_valid"][3]) == 0
    if kind == "pursuit":
        assert int(fused["route_status"][2]) == 1 and torch.isnan(fused["clearance"][2]).all() and int(fused["n_clear_valid"][2]) == 0
    print(f"{kind} K = {K}, B = {B}: {int((c < 0).sum())} rollouts in contact, {int(((ncol > 0) & (ncol < nval)).sum())} mixed routes")


# ---- 2. the golden routes' full rows (stride-3 counts) ---------------------------------------------------------------
def full_rows(torch, name, copies=2):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    g = gu.load(name)
    gen = BatchedTrajectoryGenerator(0, "f64")
    cons = [float(v) for v in g["constraints"]]
    rep = lambda a: np.repeat(np.asarray(a)[None], copies, axis=0)
    wp = torch.tensor(rep(g["waypoints"]), dtype=torch.float64, device=gen.device)
    res = gen.profile_routes(wp, node_reverse=rep(g["node_is_reverse_node"]), node_turn=rep(g["node_turn"]),
                             node_tangent=rep(g["node_tangent"]), node_magnitudes=rep(g["node_magnitudes"]),
                             constraints=cons, dd=0.005, capacity=16384)
    gen.apply_node_limits(res, cons, node_max_velocity=rep(g["node_max_velocity"]), node_stop=rep(g["node_stop"]),
                          node_max_acceleration=rep(g["node_max_acceleration"]))
    tp = gen.time_profile(res, cons, dt=DT, capacity_rows=4096, node_reverse=rep(g["node_is_reverse_node"]))
    out = gen.insert_waits(res, tp, node_wait_time=rep(g["node_wait_time"]), dt=DT, node_turn=rep(g["node_turn"]),
                           node_reverse=rep(g["node_is_reverse_node"]), constraints=cons)
    torch.cuda.synchronize()
    assert not res["flags"].any().item()
    return gen, g, out


@pytest.mark.parametrize("kind,name", [("ramsete", "c1_w8"), ("ramsete", "feat_turn"), ("ramsete", "feat_wait"), ("ramsete", "feat_reverse"),
                                       ("pursuit", "c1_w8"), ("pursuit", "feat_turn"), ("pursuit", "feat_wait")])
def test_golden_routes_full_rows(torch_mod, kind, name):
    torch = torch_mod
    tk, fp = trk(), FP()
    gen, g, out = full_rows(torch, name)
    rows, counts = out["rows"].cpu().numpy(), out["counts"][:, 0].cpu().numpy()
    assert out["counts"].shape[1] == 3                      # the event-insertion counts: stride 3
    n = int(counts[0])
    K = 16
    follower = make_follower(kind)
    P = tk.sample_perturbations(2, K, seed=11)
    foot = fp.rectangle(18, 18, 2)
    rng = np.random.default_rng(n)
    pts = rows[0, rng.integers(0, n, 4), 6:8]
    lo, hi = rows[0, :n, 6:8].min(axis=0), rows[0, :n, 6:8].max(axis=0)
    scene = fp.Scene(field=(lo[0] - 1.0, lo[1] - 1.6, hi[0] + 1.5, hi[1] + 1.2),
                     circles=[(*(p + rng.normal(0, 0.8, 2)), rng.uniform(0.1, 0.5)) for p in pts])
    margin = 0.1
    fused = gen.rollout_clearance(out, follower, P, foot, scene, margin=margin, time_step=DT)
    torch.cuda.synchronize()
    check_against_pipeline(torch, kind, fused, out["rows"], out["counts"], follower, P, foot, scene, margin, ctx=gen.ctx)
    # against the NumPy composition
    c, r = fused["clearance"].cpu().numpy(), fused["clear_rows"].cpu().numpy()
    f = (tr.follower if kind == "ramsete" else pr.pursuit)(**{k: getattr(follower, k) for k in (tr.DEFAULTS if kind == "ramsete" else pr.DEFAULTS)})
    n_cmp = n_exc = 0
    worst = 0.0
    for b in range(2):
        ref = rc.route(rows[b], counts[b], kind, f, P[b], foot, field=scene.field, circles=scene.circles, margin=margin)
        for k in range(K):
            s = ref["per"][k]
            if kind == "ramsete" and np.nan_to_num(ref["rollout"]["stats"][k, 2]) >= EXCLUDE_RAD:
                n_exc += 1
                assert np.isfinite(c[b, k])
                continue
            n_cmp += 1
            assert s["n"] > 0 and r[b, k, 0] >= 0, (b, k)
            d = abs(c[b, k] - s["min_clearance"])
            worst = max(worst, d)
            assert d <= 1e-9, (b, k, c[b, k], s["min_clearance"])
            assert abs(s["rows"][int(r[b, k, 0])] - s["min_clearance"]) <= AMBIGUOUS, (b, k, "min row")
            if s["margin_gap"] > AMBIGUOUS:
                assert r[b, k, 3] == s["n_below"] and r[b, k, 2] == s["first_row"], (b, k, "rows below the margin")
            if s["elem_gap"][int(r[b, k, 0])] > AMBIGUOUS:
                assert r[b, k, 1] == s["elems"][int(r[b, k, 0])], (b, k, "element")
    assert n_exc <= 0.02 * (n_cmp + n_exc), f"{n_exc} of {n_cmp + n_exc} rollouts at the wrap's discontinuity"
    print(f"{kind} {name}: {n} rows, {n_cmp} rollouts against the NumPy composition ({n_exc} left out), max diff {worst:.2e} ft; worst "
          f"clearance {fused['worst_clearance'][0].item():.4f} ft, {int(fused['n_colliding'][0])} of {int(fused['n_clear_valid'][0])} rollouts below {margin}")


# ---- 3. the known answer ---------------------------------------------------------------------------------------------
def test_known_answer_on_the_device(torch_mod):
    """rollout_clearance_ref.known_case: clearance D -+ dy - 0.75 - r at the start row.  The start pose has phi = 0 exactly,
    so the start row's clearance is a handful of exact-or-once-rounded operations: 1e-15."""
    torch = torch_mod
    tk, fp = trk(), FP()
    rows, P, circles, expect, n_col = rc.known_case()
    scene = fp.Scene(field=None, circles=circles)
    res = tk.rollout_clearance(rows, None, tk.Follower(settle_rows=rc.KNOWN_SETTLE), P, fp.rectangle(18, 18), scene, margin=rc.KNOWN_MARGIN)
    torch.cuda.synchronize()
    c = res["clearance"].cpu().numpy()
    print("known answer on the device:", c, res["clear_rows"].cpu().numpy().tolist())
    assert c.shape == (3,) and np.abs(c - expect).max() <= 1e-15
    assert res["clear_min_row"].tolist() == [0, 0, 0] and res["clear_min_element"].tolist() == [0, 0, 0]
    assert res["clear_first_row"].tolist() == [-1, 0, -1]
    assert (int(res["n_colliding"]), int(res["n_clear_valid"])) == (n_col, 3)
    assert (int(res["worst_clear_rollout"]), int(res["worst_clear_row"]), int(res["worst_clear_element"])) == (1, 0, 0)
    assert res["worst_clearance"].item() == c[1]


def test_known_answer_pure_pursuit_on_the_device(torch_mod):
    """The same case under pure pursuit: the reference's rows 0, 1, 0, and the nearer record 1.0147e-4 ft below the start row's
    value at row 1 (rollout_clearance_ref.KNOWN_PURSUIT_DIP, known to 1e-11; the device's one step of sincos adds 1e-15)."""
    torch = torch_mod
    tk, fp = trk(), FP()
    rows, P, circles, expect, n_col = rc.known_case()
    res = tk.rollout_clearance(rows, None, tk.Pursuit(settle_rows=rc.KNOWN_SETTLE), P, fp.rectangle(18, 18), fp.Scene(field=None, circles=circles),
                               margin=rc.KNOWN_MARGIN)
    torch.cuda.synchronize()
    c = res["clearance"].cpu().numpy()
    want = expect - np.array([0.0, rc.KNOWN_PURSUIT_DIP, 0.0])
    print("known answer under pure pursuit on the device:", c, res["clear_rows"].cpu().numpy().tolist())
    assert np.abs(c - want).max() <= 1e-10
    assert tuple(res["clear_min_row"].tolist()) == rc.KNOWN_PURSUIT_ROWS and res["clear_min_element"].tolist() == [0, 0, 0]
    assert (int(res["n_colliding"]), int(res["n_clear_valid"]), int(res["worst_clear_rollout"]), int(res["worst_clear_row"])) == (n_col, 3, 1, 1)


# ---- both kernels: more workgroups than the device has CUs -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
def test_more_workgroups_than_cus(torch_mod, kind):
    """The layouts above are a few workgroups, which run the kernel with the clearance split off the rollout lanes; a launch
    with more workgroups than the device has CUs (here 600 routes x 128 rollouts: 300 workgroups) takes the clearance in the
    rollout lanes.  Both hold the same contract: the two-call pipeline's bits."""
    torch = torch_mod
    tk, fp = trk(), FP()
    assert torch.cuda.get_device_properties(0).multi_processor_count < 300
    K, B, cap = 128, 600, 60
    rng = np.random.default_rng(9)
    rows = rc.synth_rows(rng, B, cap)
    counts = rng.integers(30, cap + 1, B).astype(np.int32)
    field, polygons, circles = rc.layout_scene(rows, counts, 2)
    scene = fp.Scene(field=field, polygons=polygons, circles=circles)
    follower = make_follower(kind, settle_rows=10)
    P = tk.sample_perturbations(1, K, seed=4)[0]
    d_rows, d_counts = torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0")
    fused = tk.rollout_clearance(d_rows, d_counts, follower, P, fp.rectangle(18, 18), scene, margin=rc.MARGIN, time_step=DT)
    torch.cuda.synchronize()
    check_against_pipeline(torch, kind, fused, d_rows, d_counts, follower, P, fp.rectangle(18, 18), scene, rc.MARGIN)
    assert (fused["n_clear_valid"] == K).all()


# ---- 4. the C-ABI: NULL outputs, refusals, B = 0; host arrays, a single trajectory, out= -------------------------------
@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
def test_null_outputs_and_abi_checks(torch_mod, kind):
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    tk, fp = trk(), FP()
    L = _lib.lib()
    ctx = _lib.Context(0)
    rng = np.random.default_rng(5)
    pursuit = kind == "pursuit"
    foot = np.ascontiguousarray(fp.rectangle(18, 18))
    INV, UNS = _lib.VAP_ERR_INVALID, _lib.VAP_ERR_UNSUPPORTED
    for K, B in ((5, 9), (260, 2)):
        cap, settle = 90, 10
        h_rows = rc.synth_rows(rng, B, cap)
        pad = torch.zeros(B * cap * 8 + 2, dtype=torch.float64, device="cuda:0")
        rows = pad[:B * cap * 8].view(B, cap, 8)
        rows.copy_(torch.tensor(h_rows))
        counts = torch.tensor(np.stack([rng.integers(20, cap + 1, B), np.zeros(B)], axis=1).astype(np.int32), device="cuda:0")
        P = torch.tensor(tk.sample_perturbations(B, K, seed=K), device="cuda:0")
        fs = make_follower(kind, settle_rows=settle).as_struct()
        circles = np.array([[h_rows[0, 40, 6] + 0.9, h_rows[0, 40, 7], 0.2], [h_rows[B - 1, 30, 6], h_rows[B - 1, 30, 7] - 1.0, 0.25]])
        field = np.array(rc.FIELD)
        i32, f64 = torch.int32, torch.float64
        spec = [((B, K, 6), f64), ((B, K, 4 if pursuit else 2), i32), ((B,), f64), ((B,), f64), ((B,), i32), ((B,), i32), ((B,), i32)]
        spec += [((B,), i32), ((B,), i32)] if pursuit else []
        spec += [((B, K), f64), ((B, K, 4), i32), ((B,), f64), ((B,), i32), ((B,), i32), ((B,), i32), ((B,), f64), ((B,), i32), ((B,), i32)]

        def fresh():
            return [torch.full(s, -7, dtype=d, device="cuda:0") for s, d in spec]

        def call(outs, skip=None, K=K, foot=foot, circles=circles, rows_ptr=None, unfinished=None, B=B):
            p = [C.c_void_p(t.data_ptr()) if i != skip else None for i, t in enumerate(outs)]
            if not pursuit:
                p[7:7] = [unfinished, None]
            st = L.vap_rollout_clearance(ctx.handle, 1 if pursuit else 0, C.cast(C.pointer(fs), C.c_void_p), B, cap,
                                         C.c_void_p(rows.data_ptr() if rows_ptr is None else rows_ptr), C.c_void_p(counts.data_ptr()), 2, DT,
                                         K, 0, C.c_void_p(P.data_ptr()), 4, foot.ctypes.data_as(_lib.dp), field.ctypes.data_as(_lib.dp), 0,
                                         None, None, len(circles), circles.ctypes.data_as(_lib.dp), 0.1, *p)
            ctx.synchronize()
            return st

        full = fresh()
        assert call(full) == _lib.VAP_OK
        assert not any((t == -7).all() for t in full)
        for skip in range(len(spec)):
            outs = fresh()
            assert call(outs, skip=skip) == _lib.VAP_OK, skip
            for i, (a, b) in enumerate(zip(outs, full)):
                if i == skip:
                    assert (a == -7).all(), (skip, "a skipped output was written")
                else:
                    assert torch.equal(a.view(i32), b.view(i32)), (skip, i)
        p_none = [None] * 18                                        # every output NULL
        assert L.vap_rollout_clearance(ctx.handle, 1 if pursuit else 0, C.cast(C.pointer(fs), C.c_void_p), B, cap, C.c_void_p(rows.data_ptr()),
                                       C.c_void_p(counts.data_ptr()), 2, DT, K, 0, C.c_void_p(P.data_ptr()), 4, foot.ctypes.data_as(_lib.dp),
                                       field.ctypes.data_as(_lib.dp), 0, None, None, len(circles), circles.ctypes.data_as(_lib.dp), 0.1,
                                       *p_none) == _lib.VAP_OK
        ctx.synchronize()
        # refusals, each with a message
        if not pursuit:
            assert call(fresh(), unfinished=C.c_void_p(counts.data_ptr())) == INV and b"d_n_unfinished" in L.vap_last_error()
        assert call(fresh(), foot=np.ascontiguousarray(foot[::-1])) == INV and b"clockwise" in L.vap_last_error()
        many = np.tile(circles[:1], (257, 1))
        assert call(fresh(), circles=many) == UNS and b"circles" in L.vap_last_error()
        assert call(fresh(), rows_ptr=pad.data_ptr() + 8) == INV and b"aligned" in L.vap_last_error()
        assert call(fresh(), K=0) == INV and L.vap_last_error() and call(fresh(), K=4097) == INV and L.vap_last_error()
        assert call(fresh(), B=0) == _lib.VAP_OK                    # B = 0 is a no-op
    ctx.close()


@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
def test_host_input_single_trajectory_and_out(torch_mod, kind):
    torch = torch_mod
    tk, fp = trk(), FP()
    rng = np.random.default_rng(8)
    rows = rc.synth_rows(rng, 3, 100)
    counts = np.array([100, 60, 80], dtype=np.int32)
    follower = make_follower(kind, settle_rows=5)
    P = tk.sample_perturbations(3, 4, seed=2)
    foot = fp.rectangle(18, 18)
    scene = fp.Scene(field=rc.FIELD, circles=[(rows[1, 30, 6] + 1.0, rows[1, 30, 7], 0.2)])
    keys = FOLLOWER_KEYS[kind] + CLEAR_KEYS
    dev = tk.rollout_clearance(torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0"), follower, P, foot, scene, margin=0.1)
    bufs = {}
    host = tk.rollout_clearance(rows, counts, follower, P, foot, scene, margin=0.1, out=bufs)
    torch.cuda.synchronize()
    assert_same_bits(dev, host, keys, "host arrays")
    assert set(bufs) == set(keys)
    ptrs = {k: t.data_ptr() for k, t in bufs.items()}
    tk.rollout_clearance(rows, counts, follower, P, foot, scene, margin=0.1, out=bufs)
    assert {k: t.data_ptr() for k, t in bufs.items()} == ptrs
    # a single trajectory: (K, ...) and 0-d tensors; out= keeps the batch-shaped buffers and a second call reuses them
    sb = {}
    one = tk.rollout_clearance(rows[1, :60], None, follower, P[1], foot, scene, margin=0.1, out=sb)
    torch.cuda.synchronize()
    assert one["clearance"].shape == (4,) and one["clear_rows"].shape == (4, 4) and one["clear_min_row"].shape == (4,)
    assert one["worst_clearance"].dim() == 0 and one["n_colliding"].dim() == 0 and one["stats"].shape == (4, 6)
    assert set(sb) == set(keys) and sb["clearance"].shape == (1, 4) and sb["worst_clearance"].shape == (1,)
    for k in keys:
        np.testing.assert_array_equal(bits(one[k]), bits(dev[k][1]), err_msg=k)
    ptrs = {k: t.data_ptr() for k, t in sb.items()}
    two = tk.rollout_clearance(rows[1, :60], None, follower, P[1], foot, scene, margin=0.1, out=sb)
    torch.cuda.synchronize()
    assert {k: t.data_ptr() for k, t in sb.items()} == ptrs and two["clearance"].data_ptr() == ptrs["clearance"]
    assert_same_bits(one, two, keys, "out= reuse")


# ---- 5. refine ---------------------------------------------------------------------------------------------------------
FIELD_B = (-6.0, -6.0, 6.0, 6.0)
LINE = np.array([[-4, 0], [-2, 0], [0, 0], [2, 0], [4, 0]], dtype=np.float64)
CIRCLE_B = (0.0, 0.0, 0.5)
MARGIN_B = 0.1
REFINE_KW = dict(dd=0.005, dt=DT, capacity=4096, capacity_rows=1024)


def test_refine_with_robust_clearance(torch_mod):
    """Scenario B of DESIGN.md section 14 (a straight seed through a post) with a RAMSETE follower, 8 records of
    sample_perturbations' default sigmas shared by every candidate, N = 256, E = 32, 12 iterations.

    What follows from the cost: the best route is a candidate of some iteration whose violation was 0, and with the option
    its clearance term was min(planned min_clearance, worst_clearance of its 8 rollouts), so both were >= clearance_margin
    for the rows that iteration scored.  Those rows are reproduced here by evaluating the best waypoints in a batch of the
    search's own size (N copies): the profile picks its velocity kernel by the batch size, and a batch of one may move a
    velocity by 1e-5 relative (tests/test_gpu_search.py), which is enough to cross a margin the search has shaved."""
    from vexautonomousplanner_amd import search
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    torch = torch_mod
    tk, fp = trk(), FP()
    gen = BatchedTrajectoryGenerator(0, "f32")
    N = 256
    cfg = search.SearchConfig(candidates=N, elites=32, iterations=12, alpha=0.7, weights=search.Weights(clearance_margin=MARGIN_B))
    foot, scene = fp.rectangle(18, 18), fp.Scene(field=FIELD_B, circles=[CIRCLE_B])
    follower = tk.Follower()
    P = tk.sample_perturbations(1, 8, seed=5)[0]
    out = gen.refine(LINE, 0.5, foot, scene, config=cfg, follower=follower, perturbations=P, robust_clearance=True, **REFINE_KW)
    torch.cuda.synchronize()
    assert bool(out["feasible"].item()) and out["best_terms"][0, 2].item() == 0.0
    assert tuple(out["n_colliding"].shape) == (1, N) and out["n_colliding"].dtype == torch.int32

    def evaluate(wp1):
        wp = wp1.expand(N, -1, -1).contiguous()
        prof = gen.profile(wp, dd=0.005, capacity=4096)
        tp = gen.time_profile(prof, dt=DT, capacity_rows=1024)
        planned = gen.footprint_clearance(tp, foot, scene, margin=MARGIN_B)
        r = gen.rollout_clearance(tp, follower, P, foot, scene, margin=MARGIN_B, time_step=DT)
        torch.cuda.synchronize()
        return planned["min_clearance"][0].item(), r["worst_clearance"][0].item(), int(r["n_colliding"][0]), r["worst"][0].item()

    planned, worst_c, n_col, worst_e = evaluate(out["best_waypoints"])
    print(f"refine, robust: best cost {out['best_cost'].item():.4f} s, planned clearance {planned:.4f} ft, worst clearance of 8 rollouts "
          f"{worst_c:.4f} ft, {n_col} colliding, worst tracking error {worst_e:.4f} ft")
    assert worst_c >= MARGIN_B and n_col == 0 and planned >= MARGIN_B

    # without the option: today's sequence, call for call, written out here
    plain = gen.refine(LINE, 0.5, foot, scene, config=cfg, follower=follower, perturbations=P, **REFINE_KW)
    torch.cuda.synchronize()
    assert "n_colliding" not in plain
    W = LINE.shape[0]
    wts = cfg.weights
    mean = torch.tensor(LINE[None], device=gen.device)
    sigma = torch.full((1, W, 2), 0.5, dtype=torch.float64, device=gen.device)
    sigma[:, 0] = 0.0
    sigma[:, -1] = 0.0
    wp = torch.empty((N, W, 2), dtype=gen.tdtype, device=gen.device)
    best_wp = torch.zeros((1, W, 2), dtype=gen.tdtype, device=gen.device)
    best_cost = torch.full((1,), float("inf"), dtype=torch.float64, device=gen.device)
    best_terms = torch.full((1, 4), float("nan"), dtype=torch.float64, device=gen.device)
    history = torch.full((1, 12), float("inf"), dtype=torch.float64, device=gen.device)
    Pd = torch.tensor(P, device=gen.device)
    prof, tp, clr, trkb, upd = None, {}, {}, {}, {}
    for it in range(12):
        search.sample(mean, sigma, N, seed=cfg.seed, iteration=it, best_waypoints=best_wp, best_cost=best_cost, out=wp, ctx=gen.ctx)
        prof = gen.profile(wp, out=prof, dd=0.005, capacity=4096)
        gen.time_profile(prof, dt=DT, capacity_rows=1024, out=tp)
        fp.clearance(tp["rows"], tp["counts"], foot, scene, margin=wts.clearance_margin, out=clr, ctx=gen.ctx)
        tk.rollouts(tp["rows"], tp["counts"], follower, Pd, time_step=DT, out=trkb, ctx=gen.ctx)
        search.update(wp, 1, weights=wts, counts=tp["counts"], time_step=DT, meta=prof["meta"], flags=prof["flags"], mean=mean, sigma=sigma,
                      elites=cfg.elites, alpha=cfg.alpha, sigma_min=cfg.sigma_min, sigma_max=cfg.sigma_max, best_cost=best_cost,
                      best_waypoints=best_wp, best_terms=best_terms, history=history, iteration=it, out=upd, ctx=gen.ctx,
                      clearance=clr["min_clearance"], tracking_worst=trkb["worst"])
    torch.cuda.synchronize()
    for k, v in (("best_waypoints", best_wp), ("best_cost", best_cost), ("best_terms", best_terms), ("history", history), ("mean", mean),
                 ("sigma", sigma)):
        np.testing.assert_array_equal(bits(plain[k]), bits(v), err_msg=k)
    np.testing.assert_array_equal(bits(plain["cost"]), bits(upd["cost"].view(1, N)))
    p2, w2, n2, e2 = evaluate(plain["best_waypoints"])
    print(f"refine, not robust: best cost {plain['best_cost'].item():.4f} s, planned clearance {p2:.4f} ft, worst clearance of 8 rollouts "
          f"{w2:.4f} ft, {n2} colliding, worst tracking error {e2:.4f} ft")
