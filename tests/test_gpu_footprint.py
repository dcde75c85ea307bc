"""GPU: robot-footprint clearance (vap_footprint_clearance, footprint.clearance, BatchedTrajectoryGenerator.
footprint_clearance) against the brute-force NumPy reference of tests/footprint_ref.py: analytic cases, random poses and
scenes, the golden routes' full time-domain rows (reversed and in-place turn rows), rows past counts, culling on / off,
per-row values, host / device input, the C-ABI's scene validation and a config-3-sized batch."""
import ctypes as C
import math

import numpy as np
import pytest

import footprint_ref as fr
import golden_util as gu

pytestmark = pytest.mark.gpu

TOL = 1e-12          # ft, kernel against the reference
AMBIGUOUS = 1e-9     # best and runner-up closer than this: either index is right
KEYS = ("min_clearance", "min_row", "min_element", "first_row", "n_below")
SQUARE = np.array([[-0.75, -0.75], [0.75, -0.75], [0.75, 0.75], [-0.75, 0.75]])


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def fpm():
    from vexautonomousplanner_amd import footprint
    return footprint


def random_convex(rng, n, cx, cy, radius):
    """A strictly convex n-gon: sorted angles on a rotated ellipse, counter-clockwise."""
    while True:
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        if np.min(np.diff(np.concatenate([a, a[:1] + 2 * np.pi]))) > 0.5 / n:
            break
    rx, ry, rot = radius, radius * rng.uniform(0.4, 1.0), rng.uniform(0, np.pi)
    p = np.stack([rx * np.cos(a), ry * np.sin(a)], axis=1)
    R = np.array([[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]])
    return p @ R.T + [cx, cy]


def random_scene(rng, n_poly=8, n_circle=4):
    fp = fpm()
    h = fp.FIELD_FT / 2
    polys = [random_convex(rng, int(rng.integers(3, 9)), *rng.uniform(-h + 1, h - 1, 2), rng.uniform(0.3, 1.2))
             for _ in range(n_poly)]
    circles = [(*rng.uniform(-h + 1, h - 1, 2), rng.uniform(0.1, 0.6)) for _ in range(n_circle)]
    return fp.Scene(polygons=polys, circles=circles)


def random_rows(rng, B, cap):
    """Random poses, each route a short random walk (rows of a route stay close, like real rows)."""
    h = 12.1090395251 / 2
    rows = np.zeros((B, cap, 8))
    for b in range(B):
        p = rng.uniform(-h, h, 2)
        steps = np.cumsum(rng.normal(0, 0.05, (cap, 2)), axis=0)
        rows[b, :, 6:8] = p + steps
        rows[b, :, 4] = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.normal(0, 0.05, cap))
        rows[b, :, 0] = np.arange(cap) * 0.01
    return rows


def scene_kw(scene):
    return dict(field=scene.field, polygons=scene.polygons, circles=scene.circles)


def reference(rows, counts, foot, scene, margin):
    return [fr.route_summary(rows[b], int(counts[b]), foot, margin=margin, **scene_kw(scene)) for b in range(len(rows))]


def check(res, refs, tol=TOL):
    """Kernel outputs against the reference summaries; returns the largest clearance difference seen."""
    got = {k: res[k].cpu().numpy() for k in KEYS}
    rc = res["row_clearance"].cpu().numpy() if "row_clearance" in res else None
    worst = 0.0
    for b, s in enumerate(refs):
        if s["n"] == 0:
            assert math.isnan(got["min_clearance"][b]), b
            assert (got["min_row"][b], got["min_element"][b], got["first_row"][b], got["n_below"][b]) == (-1, -1, -1, 0), b
            continue
        e = abs(got["min_clearance"][b] - s["min_clearance"])
        worst = max(worst, e)
        assert e <= tol, (b, got["min_clearance"][b], s["min_clearance"])
        r = int(got["min_row"][b])
        assert 0 <= r < s["n"] and abs(s["rows"][r] - s["min_clearance"]) <= AMBIGUOUS, b
        if s["row_gap"] > AMBIGUOUS:
            assert r == s["min_row"], (b, r, s["min_row"])
        if s["elem_gap"][r] > AMBIGUOUS:
            assert got["min_element"][b] == s["elems"][r], (b, got["min_element"][b], s["elems"][r])
        if s["margin_gap"] > AMBIGUOUS:
            assert got["first_row"][b] == s["first_row"], (b, got["first_row"][b], s["first_row"])
            assert got["n_below"][b] == s["n_below"], (b, got["n_below"][b], s["n_below"])
        if rc is not None:
            d = np.max(np.abs(rc[b, :s["n"]] - s["rows"]))
            worst = max(worst, d)
            assert d <= tol, (b, d)
            assert np.isnan(rc[b, s["n"]:]).all(), b
    return worst


def bits(res):
    return {k: res[k].cpu().numpy().view(np.int64 if res[k].dtype.itemsize == 8 else np.int32).copy()
            for k in KEYS + ("row_clearance",) if k in res}


# ---- 1. analytic cases ------------------------------------------------------------------------------------------------
def test_analytic_cases(torch_mod):
    fp = fpm()
    torch = torch_mod

    def run(headings, xs, scene):
        rows = np.zeros((len(headings), 2, 8))
        rows[:, 0, 4], rows[:, 0, 6] = headings, xs
        rows[:, 1] = np.nan                                      # past counts
        counts = np.ones(len(headings), dtype=np.int32)
        r = fp.clearance(torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0"), SQUARE, scene,
                         per_row=True)
        torch.cuda.synchronize()
        return r["min_clearance"].cpu().numpy(), r["min_element"].cpu().numpy(), r

    v, el, r = run([0.0, -math.pi / 4, math.pi / 4], [0.0, 0.0, 1.0], fp.Scene(field=(-10.0, -10.0, 1.25, 10.0)))
    np.testing.assert_allclose(v, [0.5, 1.25 - 0.75 * math.sqrt(2), 0.25 - 0.75 * math.sqrt(2)], rtol=0, atol=1e-14)
    assert el.tolist() == [-1, -1, -1]
    assert r["feasible"].tolist() == [True, True, False] and r["first_row"].tolist() == [-1, -1, 0]
    v, el, _ = run([0.0], [0.0], fp.Scene(field=None, polygons=[[[0.55, -1.0], [2.0, -1.0], [2.0, 1.0], [0.55, 1.0]]]))
    assert abs(v[0] + 0.2) <= 1e-14 and el[0] == 0
    v, el, _ = run([0.0], [0.0], fp.Scene(field=None, polygons=[[[5, 5], [6, 5], [6, 6]]], circles=[(2.0, 0.0, 1.25)]))
    assert abs(v[0]) <= 1e-14 and el[0] == 1
    # ties: the wall and a polygon both 0.5 away -> the wall; two equal polygons -> the first
    box = [[1.25, -1.0], [2.0, -1.0], [2.0, 1.0], [1.25, 1.0]]
    v, el, _ = run([0.0], [0.0], fp.Scene(field=(-10.0, -10.0, 1.25, 10.0), polygons=[box]))
    assert abs(v[0] - 0.5) <= 1e-14 and el[0] == -1
    v, el, _ = run([0.0], [-1.0], fp.Scene(field=None, polygons=[box, box]))
    assert abs(v[0] - 1.5) <= 1e-14 and el[0] == 0


# ---- 2, 5, 6. random poses, footprints and scenes -----------------------------------------------------------------------
def random_case(seed):
    fp = fpm()
    rng = np.random.default_rng(seed)
    B, cap = 12, 400
    counts = rng.integers(1, cap + 1, B).astype(np.int32)
    counts[3] = 0
    rows = random_rows(rng, B, cap)
    foot = fp.rectangle(*rng.uniform(12, 24, 2), rng.uniform(-3, 3)) if seed % 2 else random_convex(rng, int(rng.integers(3, 17)), 0.1, 0, 0.9)
    return rows, counts, foot, random_scene(rng), float(rng.uniform(0.0, 0.5))


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_against_reference(torch_mod, seed):
    fp = fpm()
    torch = torch_mod
    rows, counts, foot, scene, margin = random_case(seed)
    d_rows, d_counts = torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0")
    res = fp.clearance(d_rows, d_counts, foot, scene, margin=margin, per_row=True)
    off = fp.clearance(d_rows, d_counts, foot, scene, margin=margin, per_row=True, cull=False)
    torch.cuda.synchronize()
    worst = check(res, reference(rows, counts, foot, scene, margin))
    print(f"seed {seed}: {int(counts.sum())} rows, max |kernel - reference| {worst:.2e} ft")
    a, b = bits(res), bits(off)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # 6. the reductions equal a torch reduction of the per-row values
    rc = res["row_clearance"]
    valid = torch.arange(rc.shape[1], device=rc.device)[None, :] < d_counts[:, None]
    filled = torch.where(valid, rc, torch.full_like(rc, float("inf")))
    have = d_counts > 0
    mn = filled.min(dim=1).values
    assert torch.equal(mn[have], res["min_clearance"][have])
    assert torch.equal(filled.argmin(dim=1)[have].int(), res["min_row"][have])
    below = valid & (rc < margin)
    assert torch.equal(below.sum(dim=1).int(), res["n_below"])
    first = torch.where(below.any(dim=1), below.int().argmax(dim=1), torch.full_like(d_counts.long(), -1))
    assert torch.equal(first.int(), res["first_row"])
    t = torch.tensor(rows[np.arange(len(rows)), np.maximum(res["min_row"].cpu().numpy(), 0), 0], device=rc.device)
    assert torch.equal(res["min_time"][have], t[have])


# ---- 4. rows past counts; a route without rows ------------------------------------------------------------------------
def test_rows_past_counts_are_ignored(torch_mod):
    fp = fpm()
    torch = torch_mod
    rows, counts, foot, scene, margin = random_case(5)
    junk = rows.copy()
    rng = np.random.default_rng(9)
    for b in range(len(rows)):
        tail = junk[b, counts[b]:]
        tail[:] = rng.choice([np.nan, np.inf, -np.inf, 1e300, -3.0, 0.0], size=tail.shape)
    runs = [fp.clearance(torch.tensor(r, device="cuda:0"), torch.tensor(counts, device="cuda:0"), foot, scene, margin=margin,
                         per_row=True) for r in (rows, junk)]
    torch.cuda.synchronize()
    a, b = bits(runs[0]), bits(runs[1])
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    r = runs[1]
    assert math.isnan(r["min_clearance"][3].item()) and math.isnan(r["min_time"][3].item())
    assert [int(r[k][3]) for k in ("min_row", "min_element", "first_row", "n_below")] == [-1, -1, -1, 0]
    assert bool(r["feasible"][3]) and torch.isnan(r["row_clearance"][3]).all()
    # counts outside [0, capacity] are clamped
    cl = counts.copy()
    cl[0], cl[1] = -5, rows.shape[1] + 1000
    c = fp.clearance(torch.tensor(rows, device="cuda:0"), torch.tensor(cl, device="cuda:0"), foot, scene, margin=margin)
    torch.cuda.synchronize()
    assert int(c["min_row"][0]) == -1 and int(c["n_below"][0]) == 0
    check({k: c[k][1:2] for k in KEYS}, reference(rows[1:2], [rows.shape[1]], foot, scene, margin))


# ---- 7. host input, single trajectory --------------------------------------------------------------------------------
def test_host_input_and_single_trajectory(torch_mod):
    fp = fpm()
    torch = torch_mod
    rows, counts, foot, scene, margin = random_case(6)
    dev = fp.clearance(torch.tensor(rows, device="cuda:0"), torch.tensor(counts, device="cuda:0"), foot, scene, margin=margin)
    host = fp.clearance(rows, counts, foot, scene, margin=margin)
    torch.cuda.synchronize()
    a, b = bits(dev), bits(host)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    n = int(counts[0])
    one = fp.clearance(rows[0, :n], None, foot, scene, margin=margin, per_row=True)
    torch.cuda.synchronize()
    assert one["min_clearance"].dim() == 0 and one["row_clearance"].shape == (n,)
    for k in KEYS:
        assert one[k].item() == dev[k][0].item(), k
    # a clockwise footprint is reordered in Python
    cw = fp.clearance(rows, counts, foot[::-1], scene, margin=margin)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cw["min_clearance"].cpu().numpy(), host["min_clearance"].cpu().numpy())


# ---- 3. real trajectories: reversed rows and in-place turn rows --------------------------------------------------------
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
    tp = gen.time_profile(res, cons, dt=0.01, capacity_rows=4096, node_reverse=rep(g["node_is_reverse_node"]))
    out = gen.insert_waits(res, tp, node_wait_time=rep(g["node_wait_time"]), dt=0.01, node_turn=rep(g["node_turn"]),
                           node_reverse=rep(g["node_is_reverse_node"]), constraints=cons)
    torch.cuda.synchronize()
    assert not res["flags"].any().item()
    return gen, g, tp, out


def route_scene(rows, n):
    """Obstacles placed along the route so that some rows touch them and some do not."""
    fp = fpm()
    rng = np.random.default_rng(n)
    pts = rows[rng.integers(0, n, 6), 6:8]
    polys = [random_convex(rng, int(rng.integers(3, 9)), *(p + rng.normal(0, 0.8, 2)), rng.uniform(0.2, 0.8)) for p in pts[:4]]
    circles = [(*(p + rng.normal(0, 0.8, 2)), rng.uniform(0.1, 0.5)) for p in pts[4:]]
    lo, hi = rows[:n, 6:8].min(axis=0), rows[:n, 6:8].max(axis=0)
    return fp.Scene(field=(lo[0] - 1.0, lo[1] - 1.6, hi[0] + 1.5, hi[1] + 1.2), polygons=polys, circles=circles)


@pytest.mark.parametrize("name", ["feat_reverse", "feat_turn", "feat_mixed"])
def test_golden_routes_full_rows(torch_mod, name):
    fp = fpm()
    torch = torch_mod
    gen, g, tp, out = full_rows(torch, name)
    foot = fp.rectangle(18, 18, 2)
    for d, stride in ((out, 3), (tp, 2)):
        rows, counts = d["rows"].cpu().numpy(), d["counts"][:, 0].cpu().numpy()
        assert d["counts"].shape[1] == stride
        n = int(counts[0])
        if d is out:
            # reversed rows (negative velocity) or in-place turn rows (zero velocity, changing heading) are present
            v = rows[0, :n, 2]
            assert (v < 0).any() or ((v == 0) & (np.abs(rows[0, :n, 5]) > 0)).any(), name
        scene = route_scene(rows[0], n)
        res = gen.footprint_clearance(d, foot, scene, margin=0.1, per_row=True)
        off = gen.footprint_clearance(d, foot, scene, margin=0.1, per_row=True, cull=False)
        torch.cuda.synchronize()
        worst = check(res, reference(rows, counts, foot, scene, 0.1))
        print(f"{name} stride {stride}: {n} rows, max |kernel - reference| {worst:.2e} ft, min {res['min_clearance'][0].item():.4f} "
              f"at row {int(res['min_row'][0])} ({scene.element_name(int(res['min_element'][0]))}), {int(res['n_below'][0])} below")
        a, b = bits(res), bits(off)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- 8. the C-ABI validates the scene ---------------------------------------------------------------------------------
def test_abi_rejects_bad_scenes(torch_mod):
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    L = _lib.lib()
    ctx = _lib.Context(0)
    rows = torch.zeros((1, 4, 8), dtype=torch.float64, device="cuda:0")
    counts = torch.full((1, 2), 4, dtype=torch.int32, device="cuda:0")
    outs = [torch.empty(1, dtype=torch.float64, device="cuda:0")] + [torch.empty(1, dtype=torch.int32, device="cuda:0") for _ in range(4)]
    arr = lambda a, t=C.c_double: (t * len(a))(*a)
    flat = lambda v: arr([float(x) for p in v for x in p])
    sq = [[-0.75, -0.75], [0.75, -0.75], [0.75, 0.75], [-0.75, 0.75]]
    tri = [[3.0, 3.0], [4.0, 3.0], [3.0, 4.0]]

    def call(foot=sq, field=(-6.0, -6.0, 6.0, 6.0), polys=(tri,), circles=((0.0, 4.0, 0.5),), starts=None):
        starts = starts if starts is not None else np.cumsum([0] + [len(p) for p in polys]).tolist()
        pxy = [x for p in polys for x in p]
        return L.vap_footprint_clearance(ctx.handle, 1, 4, C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), 2,
                                         len(foot), flat(foot), arr(field) if field is not None else None, len(polys),
                                         arr(starts, C.c_int), flat(pxy) if pxy else None, len(circles),
                                         flat(circles) if circles else None, 0.0, None,
                                         *[C.c_void_p(t.data_ptr()) for t in outs])

    assert call() == _lib.VAP_OK
    torch.cuda.synchronize()
    # the square at the origin: wall 5.25, triangle 2.25 * sqrt(2), circle (id 1) 4 - 0.75 - 0.5
    assert abs(outs[0].item() - 2.75) <= 1e-14 and outs[2].item() == 1
    assert call(field=None, polys=(), circles=()) == _lib.VAP_OK
    INV, UNS = _lib.VAP_ERR_INVALID, _lib.VAP_ERR_UNSUPPORTED
    assert call(foot=sq[::-1]) == INV                                           # clockwise footprint
    assert call(polys=(tri[::-1],)) == INV                                      # clockwise polygon
    assert b"clockwise" in L.vap_last_error()
    assert call(polys=([[0, 0], [1, 0], [2, 0], [1, 1]],)) == INV               # collinear
    assert call(polys=([[0, 0], [1, 0], [1, 0], [1, 1]],)) == INV               # duplicate
    assert call(polys=([[0, 0], [2, 0], [1, 0.5], [2, 2], [0, 2]],)) == INV     # non-convex
    assert call(circles=((0.0, 0.0, 0.0),)) == INV                              # zero radius
    assert call(field=(1.0, 0.0, 0.0, 1.0)) == INV                              # empty box
    assert call(foot=sq[:2]) == INV
    assert call(polys=(tri,), starts=[1, 4]) == INV
    assert call(polys=(tri,) * 257) == UNS
    assert call(circles=((0.0, 4.0, 0.5),) * 257) == UNS
    ctx.close()


# ---- 9. config 3's batch --------------------------------------------------------------------------------------------
def test_config3_batch_sample(torch_mod):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    fp = fpm()
    torch = torch_mod
    gen = BatchedTrajectoryGenerator(0, "f32")
    wp = torch.tensor(make_waypoints(4096, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    scene = random_scene(np.random.default_rng(33))
    foot = fp.rectangle(18, 18)
    r = gen.footprint_clearance(tp, foot, scene, margin=0.04)
    torch.cuda.synchronize()
    counts = tp["counts"][:, 0].cpu().numpy()
    assert counts.sum() > 4_000_000
    pick = np.random.default_rng(4).choice(4096, 64, replace=False)
    rows = tp["rows"][torch.tensor(pick, device=gen.device)].cpu().numpy()
    worst = check({k: r[k][torch.tensor(pick, device=gen.device)] for k in KEYS}, reference(rows, counts[pick], foot, scene, 0.04))
    print(f"config 3: {int(counts.sum())} rows, {int(r['feasible'].sum())} of 4096 routes feasible, sample max diff {worst:.2e} ft")
