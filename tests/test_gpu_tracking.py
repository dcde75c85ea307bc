"""GPU: closed-loop tracking rollouts (vap_tracking_rollouts, tracking.rollouts, BatchedTrajectoryGenerator.
tracking_rollouts) against the NumPy reference of tests/tracking_ref.py: the golden routes' full time-domain rows (plain,
reversed, in-place turn and wait rows), a config-3-shaped batch, K from 1 to 300 (several routes per workgroup and
several workgroups per route), shared against per-route records, counts below capacity, routes without rows, invalid
records, every output pointer NULL in turn, two calls bit for bit, the executed rows, and the clearance of the executed
rows against the footprint reference on the reference's executed rows.

Tolerance.  Per case the reference runs in float64 and in np.longdouble; D = |float64 - longdouble| per output value is
the reference's own rounding error.  The kernel must lie within max(1e-12, 8 D), capped at 1e-9 (ft or rad), of the
float64 reference: the loop is contractive, so rounding does not amplify, and the factor 8 covers the device's 1-ulp
sincos against NumPy's over about 1e4 trigonometric calls per rollout.  The row of the maximum may be any row whose
reference e_pos is within 1e-9 of the maximum (AMBIGUOUS, as in the footprint tests).  A rollout whose reference
max |e_phi| >= 3.0 rad sits at the wrap's discontinuity: it is checked for finiteness only, and at most 2 % of a test's
rollouts may be such.  The saturated-row count equals the reference's unless some row of that rollout has its command
m = max(|c_L|, |c_R|) within 1e-9 of the wheel limit (then that many rows may count on either side).  The executed
heading column is compared like every other column and must lie in [-pi, pi]; only a row whose reference heading is
within 1e-9 of +-pi, where a rounding error lands on either side of the wrap, is compared modulo 2 pi."""
import ctypes as C

import numpy as np
import pytest

import footprint_ref as fr
import golden_util as gu
import odometry_cases as oc
import tracking_ref as tr

pytestmark = pytest.mark.gpu

FLOOR, FACTOR, CAP = 1e-12, 8.0, 1e-9
AMBIGUOUS = 1e-9
EXCLUDE_RAD = 3.0
DT = 0.01
STAT_NAMES = ("max e_pos", "max |e_y|", "max |e_phi|", "final e_pos", "final |e_phi|")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def trk():
    from vexautonomousplanner_amd import tracking
    return tracking


def ref_dict(f):
    return tr.follower(**{k: getattr(f, k) for k in tr.DEFAULTS})


def tol_of(a64, ald):
    d = np.abs(a64.astype(np.longdouble) - ald).astype(np.float64)
    return np.minimum(np.maximum(FLOOR, FACTOR * d), CAP), d


class Worst:
    """The largest reference rounding error D and kernel difference seen, for the report."""

    def __init__(self):
        self.d, self.k = 0.0, 0.0

    def take(self, d, k):
        if np.size(d):
            self.d, self.k = max(self.d, float(np.nanmax(d))), max(self.k, float(np.nanmax(k)))


def compare(res, rows, counts, follower, P, executed=False, worst=None):
    """Every output of a kernel call against the reference, route by route.  P: (B, K, 8).  Returns (rollouts compared,
    rollouts excluded, the reference's float64 outputs per route)."""
    f = ref_dict(follower)
    worst = worst if worst is not None else Worst()
    stats, srows = res["stats"].cpu().numpy(), res["stat_rows"].cpu().numpy()
    summ = {k: res[k].cpu().numpy() for k in ("worst", "mean", "worst_rollout", "worst_row", "n_exceeding")}
    B, K = P.shape[:2]
    assert stats.shape == (B, K, 6) and srows.shape == (B, K, 2)
    if executed:
        erows, ecounts = res["rows"].cpu().numpy(), res["counts"].cpu().numpy()
        assert erows.shape[0] == B * K and ecounts.shape == (B * K, 2)
    n_cmp = n_exc = 0
    refs = []
    for b in range(B):
        n = min(max(int(counts[b]), 0), rows.shape[1])
        r64 = tr.rollout(rows[b], n, f, P[b], DT, executed=executed)
        rld = tr.rollout(rows[b], n, f, P[b], DT, executed=executed, dtype=np.longdouble)
        refs.append(r64)
        ok = r64["stat_rows"][:, 0] >= 0
        excl = ok & (np.nan_to_num(r64["stats"][:, 2]) >= EXCLUDE_RAD)
        cmp_ = ok & ~excl
        n_cmp, n_exc = n_cmp + int(cmp_.sum()), n_exc + int(excl.sum())
        # rollouts without a result: NaN / -1, no executed rows
        assert np.isnan(stats[b, ~ok]).all() and (srows[b, ~ok] == -1).all(), b
        assert np.isfinite(stats[b, ok]).all() and (srows[b, ok] >= 0).all(), b
        if executed:
            assert (ecounts[b * K:(b + 1) * K, 0] == r64["counts"]).all() and (ecounts[b * K:(b + 1) * K, 1] == 0).all(), b
        t, d = tol_of(r64["stats"], rld["stats"])
        diff = np.abs(stats[b] - r64["stats"])
        for k in np.nonzero(cmp_)[0]:
            for c in range(5):
                assert diff[k, c] <= t[k, c], (b, k, STAT_NAMES[c], stats[b, k, c], r64["stats"][k, c], d[k, c])
            assert stats[b, k, 5] == 0.0
            e = r64["e_pos"][k]
            row = int(srows[b, k, 0])
            assert 0 <= row < len(e) and abs(e[row] - r64["stats"][k, 0]) <= AMBIGUOUS, (b, k, row)
            # saturated rows: the reference's count; only rows whose command is within AMBIGUOUS of the limit may count on either side
            near = int((np.abs(r64["cmd_max"][k] - f["wheel_speed_max"]) <= AMBIGUOUS).sum())
            assert abs(int(srows[b, k, 1]) - int(r64["stat_rows"][k, 1])) <= near, (b, k, "saturated rows", srows[b, k, 1], r64["stat_rows"][k, 1], near)
            if executed:
                m = int(r64["counts"][k])
                got, want = erows[b * K + k, :m], r64["rows"][k]
                te, de = tol_of(want, rld["rows"][k])
                dd = np.abs(got - want)
                assert (np.abs(got[:, 4]) <= np.pi).all(), (b, k, "executed heading outside [-pi, pi]")
                at_pi = np.abs(np.abs(want[:, 4]) - np.pi) <= AMBIGUOUS      # either side of the wrap
                dd[at_pi, 4] = np.abs(tr.wrap(got[at_pi, 4] - want[at_pi, 4]))
                bad = np.argwhere(dd > te)
                assert not len(bad), (b, k, "executed", bad[0], got[tuple(bad[0])], want[tuple(bad[0])], de[tuple(bad[0])])
                worst.take(de, dd)
        worst.take(d[cmp_, :5], diff[cmp_, :5])
        # the route's summary (only where no rollout was excluded: an excluded one may be the worst)
        s64 = tr.route_summary(r64["stats"], r64["stat_rows"], f["tolerance"])
        sld = tr.route_summary(rld["stats"], rld["stat_rows"], f["tolerance"])
        if not ok.any():
            assert np.isnan(summ["worst"][b]) and np.isnan(summ["mean"][b]), b
            assert (summ["worst_rollout"][b], summ["worst_row"][b], summ["n_exceeding"][b]) == (-1, -1, 0), b
        elif not excl.any():
            for key in ("worst", "mean"):
                t1, _ = tol_of(np.float64(s64[key]), np.longdouble(sld[key]))
                assert abs(summ[key][b] - s64[key]) <= t1, (b, key, summ[key][b], s64[key])
            wk = int(summ["worst_rollout"][b])
            assert ok[wk] and abs(r64["stats"][wk, 0] - s64["worst"]) <= AMBIGUOUS, (b, wk)
            assert summ["worst_row"][b] == srows[b, wk, 0], b
            e = r64["stats"][ok, 0]
            if np.min(np.abs(e - f["tolerance"])) > AMBIGUOUS:
                assert summ["n_exceeding"][b] == s64["n_exceeding"], b
            # the kernel's own summary is exactly the fixed-order reduction of its own per-rollout outputs
            own = tr.route_summary(stats[b], srows[b], f["tolerance"])
            assert (summ["worst"][b], summ["mean"][b], wk, summ["n_exceeding"][b]) == \
                (own["worst"], own["mean"], own["worst_rollout"], own["n_exceeding"]), b
        else:
            assert np.isfinite(summ["worst"][b]) and np.isfinite(summ["mean"][b]), b
    assert n_exc <= 0.02 * max(n_cmp + n_exc, 1), f"{n_exc} of {n_cmp + n_exc} rollouts at the wrap's discontinuity"
    return n_cmp, n_exc, refs


def bits(res, keys=("stats", "stat_rows", "worst", "mean", "worst_rollout", "worst_row", "n_exceeding")):
    return {k: res[k].cpu().numpy().view(np.int64 if res[k].dtype.itemsize == 8 else np.int32).copy() for k in keys if k in res}


def synth_rows(rng, B, cap):
    """Consistent rows of smooth random drives: v(t), omega(t) are sums of a few sines, integrated by the exact arc."""
    rows = np.zeros((B, cap, 8))
    t = np.arange(cap) * DT
    for b in range(B):
        v = 2.0 + sum(rng.uniform(0, 0.8) * np.sin(rng.uniform(0.5, 4) * t + rng.uniform(0, 6)) for _ in range(3))
        w = sum(rng.uniform(0, 1.2) * np.sin(rng.uniform(0.5, 5) * t + rng.uniform(0, 6)) for _ in range(3))
        x, y, phi = rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(-np.pi, np.pi)
        s = 0.0
        for r in range(cap):
            rows[b, r] = [t[r], s, v[r], 0.0, -tr.wrap(phi), -w[r], x, y]
            u = w[r] * DT / 2
            d = v[r] * DT * float(tr.sinc(u))
            x, y, phi, s = x + d * np.cos(phi + u), y + d * np.sin(phi + u), phi + w[r] * DT, s + abs(d)
        rows[b, 1:, 3] = np.diff(rows[b, :, 2]) / DT
    return rows


# ---- 1, 8, 9. the golden routes' full rows: values, executed rows, clearance of the executed rows ---------------------
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


@pytest.mark.parametrize("name", ["c1_w8", "feat_limits", "feat_stop", "feat_wait", "feat_turn", "feat_reverse", "feat_mixed"])
def test_golden_routes_full_rows(torch_mod, name):
    from vexautonomousplanner_amd import footprint as fp
    torch = torch_mod
    tk = trk()
    gen, g, out = full_rows(torch, name)
    rows, counts = out["rows"].cpu().numpy(), out["counts"][:, 0].cpu().numpy()
    assert out["counts"].shape[1] == 3                      # the event-insertion counts: stride 3
    n = int(counts[0])
    if name in ("feat_turn", "feat_reverse", "feat_mixed"):
        v = rows[0, :n, 2]
        assert (v < 0).any() or ((v == 0) & (np.abs(rows[0, :n, 5]) > 0)).any(), name
    if name == "feat_wait":
        assert ((rows[0, 1:n - 1, 2] == 0) & (rows[0, 1:n - 1, 5] == 0)).any(), "wait rows"
    K = 16
    follower = tk.Follower()
    P = tk.sample_perturbations(2, K, seed=11)
    res = gen.tracking_rollouts(out, follower, P, time_step=DT, executed=True)
    torch.cuda.synchronize()
    worst = Worst()
    n_cmp, n_exc, refs = compare(res, rows, counts, follower, P, executed=True, worst=worst)
    nominal = res["max_error"][0, 0].item()
    print(f"{name}: {n} rows, {n_cmp} rollouts compared, {n_exc} excluded, worst D {worst.d:.2e}, worst |kernel - reference| "
          f"{worst.k:.2e}; undisturbed max e_pos {nominal:.4f} ft, worst of {K} {res['worst'][0].item():.4f} ft "
          f"(rollout {int(res['worst_rollout'][0])}, row {int(res['worst_row'][0])}), max |e_phi| {res['max_heading_error'].max().item():.2f} rad")
    assert res["rows"].shape == (2 * K, rows.shape[1] + follower.settle_rows, 8) and res["counts"].shape == (2 * K, 2)
    # composition: the executed rows go to the clearance call as they are
    foot = fp.rectangle(18, 18, 2)
    rng = np.random.default_rng(n)
    pts = rows[0, rng.integers(0, n, 4), 6:8]
    lo, hi = rows[0, :n, 6:8].min(axis=0), rows[0, :n, 6:8].max(axis=0)
    scene = fp.Scene(field=(lo[0] - 1.0, lo[1] - 1.6, hi[0] + 1.5, hi[1] + 1.2),
                     circles=[(*(p + rng.normal(0, 0.8, 2)), rng.uniform(0.1, 0.5)) for p in pts])
    cl = gen.footprint_clearance(res, foot, scene, margin=0.1, per_row=True)
    torch.cuda.synchronize()
    got = {k: cl[k].cpu().numpy() for k in ("min_clearance", "min_row", "n_below", "first_row", "row_clearance")}
    wc = 0.0
    for b in range(2):
        for k in range(0, K, 3):
            m = int(refs[b]["counts"][k])
            s = fr.route_summary(refs[b]["rows"][k].astype(np.float64), m, foot, field=scene.field, circles=scene.circles, margin=0.1)
            i = b * K + k
            d = max(abs(got["min_clearance"][i] - s["min_clearance"]), float(np.max(np.abs(got["row_clearance"][i, :m] - s["rows"]))))
            wc = max(wc, d)
            assert d <= 1e-9, (b, k, d)
            assert abs(s["rows"][int(got["min_row"][i])] - s["min_clearance"]) <= AMBIGUOUS
            if s["margin_gap"] > AMBIGUOUS:
                assert got["n_below"][i] == s["n_below"] and got["first_row"][i] == s["first_row"], (b, k)
            assert np.isnan(got["row_clearance"][i, m:]).all()
    print(f"{name}: clearance of the executed rows against the reference's: max diff {wc:.2e} ft")


# ---- 2. config 3's batch ---------------------------------------------------------------------------------------------
def test_config3_batch_sample(torch_mod):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    torch = torch_mod
    tk = trk()
    gen = BatchedTrajectoryGenerator(0, "f32")
    wp = torch.tensor(make_waypoints(4096, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    K = 16
    follower = tk.Follower()
    P = tk.sample_perturbations(4096, K, seed=3)
    r = gen.tracking_rollouts(tp, follower, P, time_step=DT)
    torch.cuda.synchronize()
    counts = tp["counts"][:, 0].cpu().numpy()
    assert counts.sum() > 4_000_000
    pick = np.sort(np.random.default_rng(4).choice(4096, 64, replace=False))
    sel = torch.tensor(pick, device=gen.device)
    rows = tp["rows"][sel].cpu().numpy()
    sub = {k: r[k][sel] for k in ("stats", "stat_rows", "worst", "mean", "worst_rollout", "worst_row", "n_exceeding")}
    worst = Worst()
    n_cmp, n_exc, _ = compare(sub, rows, counts[pick], follower, P[pick], worst=worst)
    print(f"config 3: {int(counts.sum())} rows x {K} rollouts, sample of 64 routes: {n_cmp} compared, {n_exc} excluded, worst D "
          f"{worst.d:.2e}, worst |kernel - reference| {worst.k:.2e}; batch worst {r['worst'].max().item():.4f} ft, "
          f"{int((r['n_exceeding'] > 0).sum())} of 4096 routes with a rollout above {follower.tolerance} ft")


# ---- 3, 4, 5, 7. K sweep: layouts, shared records, short counts, empty routes, invalid records, two calls -------------
@pytest.mark.parametrize("K,B", [(1, 300), (3, 100), (16, 20), (64, 6), (300, 3), (256, 2), (257, 2), (256, 3), (257, 3)])
def test_rollout_counts_and_layouts(torch_mod, K, B):
    torch = torch_mod
    tk = trk()
    rng = np.random.default_rng(100 + K)
    cap = 120
    rows = synth_rows(rng, B, cap)
    counts = rng.integers(30, cap + 1, B).astype(np.int32)
    if B > 2:
        counts[B // 2] = 0                                      # a route without rows (two routes: both have rows)
    counts[0], counts[B - 1] = cap + 500, cap                   # clamped to capacity
    if B > 4:
        counts[1] = -3                                          # clamped to 0
    for b in range(B):                                          # rows past counts are never read
        rows[b, max(min(int(counts[b]), cap), 0):] = np.nan
    follower = tk.Follower(settle_rows=20, n_substeps=3, tolerance=0.1)
    P = tk.sample_perturbations(B, K, seed=K, tau=0.03)
    if K >= 3:
        P[:, K // 2, 3] = 0.0                                   # invalid: gain_left <= 0
        P[0, K - 1, 0] = np.nan                                 # invalid: non-finite
        P[B - 1, 1, 6] = -0.01                                  # invalid: tau < 0
        P[B - 1, 2, 5] = -1.0                                   # invalid: track_scale <= 0
    else:
        P[3, 0, 4] = -1.0                                       # a route whose only rollout is invalid
    d_rows, d_counts = torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0")
    res = tk.rollouts(d_rows, d_counts, follower, P, time_step=DT, executed=True)
    again = tk.rollouts(d_rows, d_counts, follower, torch.tensor(P, device="cuda:0"), time_step=DT, executed=True)
    torch.cuda.synchronize()
    worst = Worst()
    n_cmp, n_exc, _ = compare(res, rows, counts, follower, P, executed=True, worst=worst)
    print(f"K = {K}, B = {B}: {n_cmp} rollouts compared, {n_exc} excluded, worst D {worst.d:.2e}, worst |kernel - reference| {worst.k:.2e}")
    # two calls: the same bits (executed rows over the rows that exist)
    a, b2 = bits(res), bits(again)
    for k in a:
        np.testing.assert_array_equal(a[k], b2[k], err_msg=k)
    ec = res["counts"][:, 0].cpu().numpy()
    np.testing.assert_array_equal(ec, again["counts"][:, 0].cpu().numpy())
    ra, rb = res["rows"].cpu().numpy(), again["rows"].cpu().numpy()
    for i in np.nonzero(ec)[0][:40]:
        np.testing.assert_array_equal(ra[i, :ec[i]].view(np.int64), rb[i, :ec[i]].view(np.int64))
    # shared records: (K, 8) for every route equals the same records repeated per route
    Ps = P[B - 1].copy()
    shared = tk.rollouts(d_rows, d_counts, follower, Ps, time_step=DT)
    repeated = tk.rollouts(d_rows, d_counts, follower, np.repeat(Ps[None], B, axis=0), time_step=DT)
    torch.cuda.synchronize()
    a, b2 = bits(shared), bits(repeated)
    for k in a:
        np.testing.assert_array_equal(a[k], b2[k], err_msg=k)
    np.testing.assert_array_equal(bits(shared)["stats"][B - 1], bits(res)["stats"][B - 1])
    # explicit edge outputs
    e = B // 2
    if B > 2:
        assert torch.isnan(res["stats"][e]).all() and (res["stat_rows"][e] == -1).all() and (res["counts"][e * K:(e + 1) * K] == 0).all()
        assert torch.isnan(res["worst"][e]) and torch.isnan(res["mean"][e])
        assert (int(res["worst_rollout"][e]), int(res["worst_row"][e]), int(res["n_exceeding"][e])) == (-1, -1, 0)
    if K >= 3:
        assert torch.isnan(res["stats"][:, K // 2]).all() and (res["stat_rows"][:, K // 2] == -1).all()
        assert (res["counts"].reshape(B, K, 2)[:, K // 2, 0] == 0).all()
        assert (res["worst_rollout"] != K // 2).all()
    else:
        assert torch.isnan(res["worst"][3]) and int(res["worst_rollout"][3]) == -1 and int(res["n_exceeding"][3]) == 0


# ---- the edges of the staged tiles --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", oc.TRACKING_TILE_K)
def test_tile_edges(torch_mod, K):
    """Routes of 63, 64, 65 and 129 rows with 10 settle rows at a capacity of 160, executed rows on (odometry_cases.
    tracking_tile_case): K = 64 stages four routes in tiles of 64 rows, the last one partial; K = 256 one route; K = 1 stages
    256 routes in tiles of 2 rows, and its second workgroup holds 4 routes, one of them without rows, and 252 idle lanes.
    test_tracking_cpu.py holds, on the reference alone, that no rollout of these inputs is excused.  At K = 64 the same call
    through odometry.rollouts with the ideal record, no start offset and no sensors gives the same bits."""
    torch = torch_mod
    tk = trk()
    case = oc.tracking_tile_case(K)
    rows, counts, P = case["rows"], case["counts"], case["P"]
    follower = tk.Follower(**case["follower"])
    d_rows, d_counts = torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0")
    res = tk.rollouts(d_rows, d_counts, follower, P, time_step=DT, executed=True)
    torch.cuda.synchronize()
    worst = Worst()
    n_cmp, n_exc, _ = compare(res, rows, counts, follower, P, executed=True, worst=worst)
    print(f"tile edges K = {K}: {n_cmp} rollouts compared, {n_exc} excluded, worst D {worst.d:.2e}, worst |kernel - reference| {worst.k:.2e}")
    assert n_exc == 0 and n_cmp == K * int((counts > 0).sum())
    assert (res["counts"][:, 0].cpu().numpy() == np.repeat(np.where(counts > 0, counts + 10, 0), K)).all()
    if K != 64:
        return
    from vexautonomousplanner_amd import odometry
    P0 = P.copy()
    P0[..., 0:3] = 0.0                                          # the estimate starts on row 0: no start offset
    ref = tk.rollouts(d_rows, d_counts, follower, P0, time_step=DT, executed=True)
    got = odometry.rollouts(d_rows, d_counts, follower, P0, np.broadcast_to(oc.orf.IDEAL, P0.shape).copy(), time_step=DT, executed=True)
    torch.cuda.synchronize()
    a, b = bits(ref, ("worst", "mean", "worst_rollout", "worst_row", "n_exceeding", "counts")), \
        bits(got, ("worst", "mean", "worst_rollout", "worst_row", "n_exceeding", "counts"))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(bits(ref, ("stats",))["stats"][..., :5], bits(got, ("stats",))["stats"][..., :5])
    np.testing.assert_array_equal(ref["stat_rows"].cpu().numpy(), got["stat_rows"][..., :2].cpu().numpy())
    ec = ref["counts"][:, 0].cpu().numpy()
    live = np.arange(ref["rows"].shape[1])[None, :] < ec[:, None]
    np.testing.assert_array_equal(ref["rows"].cpu().numpy()[live].view(np.int64), got["rows"].cpu().numpy()[live].view(np.int64))


# ---- a large, known saturated-row count ------------------------------------------------------------------------------
def test_saturated_rows_known_count(torch_mod):
    """Straight routes along x at 8 and 7 ft/s against a 6 ft/s wheel limit.  The undisturbed rollout starts on the path
    with phi = 0, so e_y = e_phi = 0 exactly and c_L = c_R = v_r + k e_x with e_x >= 0 (the robot is the slower one):
    every one of the n live rows is saturated, row 0 included, and no settle row is (there v_r = omega_r = 0, so k = 0 and
    the command is 0).  The count of the undisturbed rollout is therefore n; the disturbed ones equal the reference's."""
    torch = torch_mod
    tk = trk()
    cap, K = 160, 16
    counts = np.array([150, 97], dtype=np.int32)
    rows = np.zeros((2, cap, 8))
    t = np.arange(cap) * DT
    for b, v in enumerate((8.0, 7.0)):
        rows[b, :, 0], rows[b, :, 1], rows[b, :, 2], rows[b, :, 6], rows[b, :, 7] = t, v * t, v, 1.0 + v * t, -2.0
    follower = tk.Follower(settle_rows=20)
    P = tk.sample_perturbations(2, K, seed=21)
    res = tk.rollouts(torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0"), follower, P, time_step=DT, executed=True)
    torch.cuda.synchronize()
    n_cmp, n_exc, refs = compare(res, rows, counts, follower, P, executed=True)
    sat = res["saturated_rows"].cpu().numpy()
    print(f"saturated rows: undisturbed {sat[:, 0]}, over the {K} rollouts {sat.min(axis=1)}..{sat.max(axis=1)}")
    assert n_cmp == 2 * K and n_exc == 0
    for b in range(2):
        assert refs[b]["stat_rows"][0, 1] == counts[b] and sat[b, 0] == counts[b], (b, sat[b, 0])


# ---- 6. every output pointer NULL in turn; the C-ABI's own checks ------------------------------------------------------
def test_null_outputs_and_abi_checks(torch_mod):
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    tk = trk()
    L = _lib.lib()
    ctx = _lib.Context(0)
    rng = np.random.default_rng(5)
    for K, B in ((5, 9), (260, 2)):
        cap, settle = 90, 10
        rows = torch.tensor(synth_rows(rng, B, cap), device="cuda:0")
        counts = torch.tensor(np.stack([rng.integers(20, cap + 1, B), np.zeros(B)], axis=1).astype(np.int32), device="cuda:0")
        P = torch.tensor(tk.sample_perturbations(B, K, seed=K), device="cuda:0")
        fs = tk.Follower(settle_rows=settle).as_struct()
        cap_exec = cap + settle

        def fresh():
            return [torch.full((B, K, 6), -7.0, dtype=torch.float64, device="cuda:0"), torch.full((B, K, 2), -7, dtype=torch.int32, device="cuda:0"),
                    torch.full((B,), -7.0, dtype=torch.float64, device="cuda:0"), torch.full((B,), -7.0, dtype=torch.float64, device="cuda:0"),
                    torch.full((B,), -7, dtype=torch.int32, device="cuda:0"), torch.full((B,), -7, dtype=torch.int32, device="cuda:0"),
                    torch.full((B,), -7, dtype=torch.int32, device="cuda:0"),
                    torch.full((B * K, cap_exec, 8), -7.0, dtype=torch.float64, device="cuda:0"),
                    torch.full((B * K, 2), -7, dtype=torch.int32, device="cuda:0")]

        def call(outs, skip=None, cap_exec=cap_exec, K=K, fs=fs, dt=DT):
            p = [C.c_void_p(t.data_ptr()) if i != skip else None for i, t in enumerate(outs)]
            st = L.vap_tracking_rollouts(ctx.handle, B, cap, C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), 2, dt,
                                         C.byref(fs), K, 0, C.c_void_p(P.data_ptr()), *p[:7], cap_exec, p[7], p[8])
            ctx.synchronize()
            return st

        full = fresh()
        assert call(full) == _lib.VAP_OK
        assert not (full[0][..., :5] == -7.0).any() and not (full[6] == -7).any() and not (full[8] == -7).any()
        for skip in range(9):
            outs = fresh()
            assert call(outs, skip=skip) == _lib.VAP_OK, skip
            for i, (a, b) in enumerate(zip(outs, full)):
                if i == skip:
                    assert (a == -7).all(), (skip, "a skipped output was written")
                else:
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (skip, i)
        none = fresh()
        assert L.vap_tracking_rollouts(ctx.handle, B, cap, C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), 2, DT, C.byref(fs), K, 0,
                                       C.c_void_p(P.data_ptr()), *[None] * 7, 0, None, None) == _lib.VAP_OK
        ctx.synchronize()
        # rows past a rollout's count are left as they were
        ec = full[8][:, 0].cpu().numpy()
        ex = full[7].cpu().numpy()
        assert all((ex[i, ec[i]:] == -7.0).all() for i in range(0, B * K, 7))
        INV = _lib.VAP_ERR_INVALID
        assert call(fresh(), cap_exec=cap + settle - 1) == INV and b"cap_exec" in L.vap_last_error()
        assert call(fresh(), K=0) == INV and call(fresh(), K=4097) == INV
        assert call(fresh(), dt=0.0) == INV
        assert call(fresh(), fs=tk.Follower(settle_rows=settle, n_substeps=2).as_struct()) == _lib.VAP_OK
        bad = tk.Follower(settle_rows=settle).as_struct()
        bad.n_substeps = 17
        assert call(fresh(), fs=bad) == INV
        bad.n_substeps, bad.zeta = 2, 0.0
        assert call(fresh(), fs=bad) == INV
    # B = 0 is a no-op
    assert L.vap_tracking_rollouts(ctx.handle, 0, 0, None, None, 2, DT, C.byref(fs), 4, 0, None, *[None] * 7, 0, None, None) == _lib.VAP_OK
    e = tk.rollouts(torch.zeros((0, 16, 8), dtype=torch.float64, device="cuda:0"), torch.zeros((0, 2), dtype=torch.int32, device="cuda:0"),
                    tk.Follower(), tk.sample_perturbations(0, 4))
    assert e["stats"].shape == (0, 4, 6) and e["worst"].shape == (0,)
    ctx.close()


# ---- host input, a single trajectory, out= reuse ---------------------------------------------------------------------
def test_host_input_single_trajectory_and_out(torch_mod):
    torch = torch_mod
    tk = trk()
    rng = np.random.default_rng(8)
    rows = synth_rows(rng, 3, 100)
    counts = np.array([100, 60, 80], dtype=np.int32)
    follower = tk.Follower(settle_rows=5)
    P = tk.sample_perturbations(3, 4, seed=2)
    dev = tk.rollouts(torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0"), follower, P)
    bufs = {}
    host = tk.rollouts(rows, counts, follower, P, out=bufs)
    torch.cuda.synchronize()
    a, b = bits(dev), bits(host)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    keep = bufs["stats"].data_ptr()
    tk.rollouts(rows, counts, follower, P, out=bufs)
    assert bufs["stats"].data_ptr() == keep
    one = tk.rollouts(rows[1, :60], None, follower, P[1], executed=True)
    torch.cuda.synchronize()
    assert one["stats"].shape == (4, 6) and one["worst"].dim() == 0 and one["rows"].shape == (4, 65, 8)
    np.testing.assert_array_equal(bits(one, ("stats",))["stats"], a["stats"][1])
    assert one["worst"].item() == dev["worst"][1].item() and one["max_error"].shape == (4,)
    assert (one["counts"][:, 0] == 65).all()
    # out= with a single trajectory: the dict keeps the batch-shaped buffers and only those, and a second call reuses them
    sb = {}
    o1 = tk.rollouts(rows[1, :60], None, follower, P[1], executed=True, out=sb)
    assert set(sb) == {"stats", "stat_rows", "worst", "mean", "worst_rollout", "worst_row", "n_exceeding", "rows", "counts"}
    assert sb["stats"].shape == (1, 4, 6) and sb["worst"].shape == (1,) and o1["stats"].shape == (4, 6)
    ptrs = {k: t.data_ptr() for k, t in sb.items()}
    o2 = tk.rollouts(rows[1, :60], None, follower, P[1], executed=True, out=sb)
    torch.cuda.synchronize()
    assert {k: t.data_ptr() for k, t in sb.items()} == ptrs
    assert o2["stats"].data_ptr() == ptrs["stats"] and o2["rows"].data_ptr() == ptrs["rows"] and o2["worst"].dim() == 0
    np.testing.assert_array_equal(bits(o2, ("stats",))["stats"], a["stats"][1])
