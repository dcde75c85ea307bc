"""vap_odometry_rollouts on the device against tests/odometry_ref.py (the header's words in NumPy) on the inputs of
tests/odometry_cases.py, and against the calls it must agree with: vap_tracking_rollouts (bit for bit with the ideal record) and
vap_range_readings (the resets it counts are that call's valid readings of its own executed rows).

Tolerance: test_gpu_tracking.py's, per value: max(1e-12, 8 D) capped at 1e-9, D = |float64 - longdouble| of the reference.  The
row of a maximum may be any row within 1e-9 of it.  A rollout is excused — checked for finiteness and the integer identities
only — when its decision margin is below 1e-9, its two reference precisions took different decisions or its max |e_phi| is
3 rad or more; at most 2 % of a test's rollouts, which test_odometry_cpu.py holds on the reference alone."""
import ctypes as C

import numpy as np
import pytest

import odometry_cases as oc
import tracking_ref as tr

pytestmark = pytest.mark.gpu
DT = oc.DT
SUMMARY = ("worst", "mean", "worst_rollout", "worst_row", "n_exceeding")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def mods():
    from vexautonomousplanner_amd import footprint, odometry, sensors, tracking
    return footprint, odometry, sensors, tracking


def follower_of(f):
    from vexautonomousplanner_amd import tracking
    return tracking.Follower(**f)


def scene_of(sc):
    from vexautonomousplanner_amd import footprint as fp
    return fp.Scene(field=sc["field"], polygons=[np.asarray(p) for p in sc["polygons"]], circles=[tuple(c) for c in sc["circles"]])


def rule_of(r):
    from vexautonomousplanner_amd import odometry
    ru = odometry.ResetRule(r["gate_in"], r["max_incidence_deg"], r["gain"], r["every"])
    assert (ru.gate, ru.min_cos) == (r["gate"], r["min_cos"])
    return ru


def run(case, executed=False, estimates=False, cull=True, shared_p=False, shared_o=False, **kw):
    _, od, _, _ = mods()
    has = case["sensors"] is not None
    P = case["P"][0] if shared_p else case["P"]
    O = case["O"][0] if shared_o else case["O"]
    return od.rollouts(case["rows"], case["counts"], follower_of(case["follower"]), P, O, sensors=case["sensors"] if has else None,
                       scene=scene_of(case["scene"]) if has else None, rule=rule_of(case["rule"]) if has else None, time_step=DT,
                       executed=executed, estimates=estimates, cull=cull, **kw)


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def bits(res, keys):
    return {k: res[k].view(np.int64 if res[k].dtype.itemsize == 8 else np.int32).copy() for k in keys if k in res}


def compare(got, case, rows_out, name=""):
    """Every output of a call against the reference.  Returns (rollouts with a result, excused)."""
    r64, rld = oc.reference(case, rows_out)
    exc, ok = oc.excused(r64, rld)
    B, K = ok.shape
    f = case["follower"]
    stats, srows = got["stats"], got["stat_rows"]
    assert stats.shape == (B, K, 8) and srows.shape == (B, K, 4)
    assert np.isnan(stats[~ok]).all() and (srows[~ok] == -1).all()
    assert np.isfinite(stats[ok]).all() and (srows[ok] >= 0).all()
    n = np.clip(case["counts"], 0, case["rows"].shape[1])
    total = np.where(ok, (n + f["settle_rows"])[:, None], 0)
    assert (srows[ok][:, 0] < total[ok]).all() and (srows[ok][:, 1] <= total[ok]).all()
    if rows_out:
        assert (got["counts"][:, 0] == total.ravel()).all() and (got["counts"][:, 1] == 0).all()
    cmp_ = ok & ~exc
    t, d = oc.tol_of(r64["stats"], rld["stats"])
    diff = np.abs(stats - r64["stats"])
    worst_d = worst_k = 0.0
    if cmp_.any():
        bad = np.argwhere(cmp_[..., None] & (diff > t))
        assert not len(bad), (name, bad[0], stats[tuple(bad[0])], r64["stats"][tuple(bad[0])], d[tuple(bad[0])])
        worst_d, worst_k = float(d[cmp_].max()), float(diff[cmp_].max())
        assert (srows[cmp_][:, 1:] == r64["stat_rows"][cmp_][:, 1:]).all(), name
    for b, k in np.argwhere(cmp_):
        i = b * K + k
        e = r64["e_pos"][i]
        row = int(srows[b, k, 0])
        assert abs(e[row] - r64["stats"][b, k, 0]) <= oc.AMBIGUOUS, (name, b, k, row)
        if rows_out:
            m = int(total[b, k])
            for key, rkey, hcol in (("rows", "rows", 4), ("estimate_rows", "est_rows", 0)):
                g, want = got[key][i, :m], r64[rkey][i, :m]
                te, de = oc.tol_of(want, rld[rkey][i, :m])
                dd = np.abs(g - want)
                at_pi = np.abs(np.abs(want[:, hcol]) - np.pi) <= oc.AMBIGUOUS      # either side of the wrap
                dd[at_pi, hcol] = np.abs(tr.wrap(g[at_pi, hcol] - want[at_pi, hcol]))
                badr = np.argwhere(dd > te)
                if len(badr):
                    j = tuple(badr[0])
                    print(f"{name} {key} rollout ({b}, {k}) row {j[0]} column {j[1]}: kernel {g[j]!r} reference {want[j]!r} "
                          f"|diff| {dd[j]:.3e} D {de[j]:.3e}; {len(badr)} values of {dd.size} above their tolerance, largest |diff| {dd.max():.3e}")
                assert not len(badr), (name, key, b, k, badr[0])
                worst_d, worst_k = max(worst_d, float(de.max())), max(worst_k, float(dd.max()))
            assert (got["estimate_rows"][i, :m, 3] == (r64["decisions"][i, :m] & 255)).all(), (name, b, k)
    # the route summaries: the fixed-order reduction of the call's own per-rollout outputs, and the reference's where nobody is excused
    for b in range(B):
        own = tr.route_summary(stats[b], srows[b], f["tolerance"])
        if not ok[b].any():
            assert np.isnan(got["worst"][b]) and np.isnan(got["mean"][b])
            assert (got["worst_rollout"][b], got["worst_row"][b], got["n_exceeding"][b]) == (-1, -1, 0)
            continue
        assert (got["worst"][b], got["mean"][b], got["worst_rollout"][b], got["worst_row"][b], got["n_exceeding"][b]) == \
            (own["worst"], own["mean"], own["worst_rollout"], own["worst_row"], own["n_exceeding"]), (name, b)
        if not exc[b].any():
            for key in ("worst", "mean"):
                t1, _ = oc.tol_of(np.float64(r64[key][b]), np.longdouble(rld[key][b]))
                assert abs(got[key][b] - r64[key][b]) <= t1, (name, b, key)
    n_ok, n_exc = int(ok.sum()), int(exc.sum())
    assert n_exc <= oc.MAX_EXCUSED * max(n_ok, 1), (name, n_exc, n_ok)
    print(f"{name}: {n_ok} rollouts, {n_exc} excused, worst D {worst_d:.2e}, worst |kernel - reference| {worst_k:.2e}, "
          f"resets accepted {int(srows[ok][:, 2].sum())} rejected {int(srows[ok][:, 3].sum())}")
    return n_ok, n_exc


# ---- 1. the golden routes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 5])
def test_golden_routes(torch_mod, every):
    case = oc.golden_case(every)
    got = host(run(case, executed=True, estimates=True))
    compare(got, case, True, f"golden every={every}")


# ---- 2. layouts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,B", oc.LAYOUTS)
def test_layouts(torch_mod, K, B):
    case = oc.layout_case(K, B)
    got = host(run(case, executed=True, estimates=True))
    n_ok, _ = compare(got, case, True, f"layout K={K} B={B}")
    if K >= 3:
        assert n_ok < K * B                                   # invalid records and the route without rows took no part
    # shared against per-route, for each of the two record arrays independently
    keys = ("stats", "stat_rows") + SUMMARY
    for sp, so in ((True, False), (False, True)):
        c2 = dict(case)
        if sp:
            c2["P"] = np.broadcast_to(case["P"][0], case["P"].shape).copy()
        if so:
            c2["O"] = np.broadcast_to(case["O"][0], case["O"].shape).copy()
        a, b = bits(host(run(c2)), keys), bits(host(run(c2, shared_p=sp, shared_o=so)), keys)
        assert all((a[k] == b[k]).all() for k in keys), (sp, so)


# ---- 3. tile edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 64])
def test_tile_edges(torch_mod, every):
    case = oc.tile_case(every)
    got = host(run(case, executed=True, estimates=True))
    compare(got, case, True, f"tiles every={every}")
    mask = got["estimate_rows"][:, :, 3]
    tot = got["counts"][:, 0]
    live = np.arange(mask.shape[1])[None, :] < tot[:, None]
    assert (mask[live & (np.arange(mask.shape[1])[None, :] % every != 0)] == 0).all()
    for r in (0, 63, 64, 128):
        if r % every == 0:
            assert (mask[:, r][tot > r] > 0).any(), r       # resets on the tiles' first and last rows


# ---- 4. the scene on both sides of the LDS budget, culling on and off ----------------------------------------------------------
@pytest.mark.parametrize("over", [False, True])
def test_scene_size_and_culling(torch_mod, over):
    case = oc.scene_size_case(over)
    n_dbl = sum(4 + 8 * len(p) for p in case["scene"]["polygons"]) + 4 * len(case["scene"]["circles"])
    assert (n_dbl > 2048) == over
    on = host(run(case, executed=True, estimates=True, cull=True))
    off = host(run(case, executed=True, estimates=True, cull=False))
    compare(on, case, True, f"scene over={over}")
    keys = ("stats", "stat_rows", "counts") + SUMMARY
    a, b = bits(on, keys), bits(off, keys)
    assert all((a[k] == b[k]).all() for k in keys)
    live = np.arange(on["rows"].shape[1])[None, :] < on["counts"][:, :1]
    for k in ("rows", "estimate_rows"):
        assert (on[k][live].view(np.int64) == off[k][live].view(np.int64)).all(), k


# ---- 5. the number of sensors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [0, 1, 8])
def test_number_of_sensors(torch_mod, ns):
    case = oc.sensors_case(ns)
    got = host(run(case, executed=True, estimates=True))
    compare(got, case, True, f"sensors n={ns}")
    ok = got["stat_rows"][..., 0] >= 0
    if ns == 0:
        assert (got["stat_rows"][ok][:, 2:] == 0).all()
    else:
        assert got["stat_rows"][ok][:, 2].sum() > 0
        live = np.arange(got["rows"].shape[1])[None, :] < got["counts"][:, :1]
        assert (got["estimate_rows"][:, :, 3][live] < (1 << ns)).all()


# ---- 6. equal to vap_tracking_rollouts, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sensors", [False, True])
def test_equals_tracking_rollouts(torch_mod, with_sensors):
    _, _, _, tk = mods()
    base = oc.layout_case(16, 17)
    case = dict(base)
    case["P"] = base["P"].copy()
    case["P"][..., 0:3] = 0.0                                  # no start offset
    case["O"] = np.broadcast_to(oc.orf.IDEAL, base["O"].shape).copy()
    if with_sensors:
        case["rule"] = oc.rule(oc.GATE_IN, oc.INCIDENCE_DEG, 0.0, 1)       # gain 0: a reset changes nothing
    else:
        case["sensors"] = case["scene"] = case["rule"] = None
    got = host(run(case, executed=True, estimates=True))
    ref = host(tk.rollouts(case["rows"], case["counts"], follower_of(case["follower"]), case["P"], time_step=DT, executed=True))
    assert (got["stats"][..., :5].view(np.int64) == ref["stats"][..., :5].view(np.int64)).all()
    ok = ref["stat_rows"][..., 0] >= 0
    assert ok.any() and (got["stats"][ok][:, 5:] == 0.0).all() and np.isnan(got["stats"][~ok][:, 5:]).all()
    assert (got["stat_rows"][..., :2] == ref["stat_rows"]).all()
    for k in SUMMARY:
        assert (got[k].view(np.int64 if got[k].dtype.itemsize == 8 else np.int32) == ref[k].view(np.int64 if ref[k].dtype.itemsize == 8 else np.int32)).all(), k
    assert (got["counts"] == ref["counts"]).all()
    live = np.arange(got["rows"].shape[1])[None, :] < got["counts"][:, :1]
    assert live.any() and (got["rows"][live].view(np.int64) == ref["rows"][live].view(np.int64)).all()
    assert (got["estimate_rows"][live][:, :3] == got["rows"][live][:, [4, 6, 7]]).all()      # the estimate is the true pose
    if with_sensors:
        assert got["stat_rows"][ok][:, 2].sum() > 0


# ---- 7. equal to vap_range_readings ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 5])
def test_resets_are_the_valid_readings_of_the_executed_rows(torch_mod, every):
    _, _, sn, _ = mods()
    case = oc.golden_case(every)
    res = run(case, executed=True, estimates=True)
    rd = sn.readings(res["rows"], res["counts"], case["sensors"], scene_of(case["scene"]), per_row=True)
    status = (rd["code"].cpu().numpy() & 15)
    code = rd["code"].cpu().numpy()
    got = host(res)
    B, K = got["stat_rows"].shape[:2]
    tot = got["counts"][:, 0]
    r = np.arange(code.shape[1])[None, :, None]
    valid = (code >= 0) & (status == 0) & (r < tot[:, None, None]) & (r % every == 0)
    tried = got["stat_rows"][..., 2].reshape(-1) + got["stat_rows"][..., 3].reshape(-1)
    assert tot.min() > 0 and (tried == valid.sum(axis=(1, 2))).all()
    # and the accepted ones sit where the mask says
    mask = got["estimate_rows"][:, :, 3]
    live = np.arange(mask.shape[1])[None, :] < tot[:, None]
    mask = np.where(live, mask, 0.0).astype(np.int64)               # rows past a rollout's count are not written
    acc = sum(((mask >> s) & 1) for s in range(4))
    assert (acc.sum(axis=1) == got["stat_rows"][..., 2].reshape(-1)).all()


# ---- 8. output plumbing --------------------------------------------------------------------------------------------------------
def test_null_outputs_same_bits_out_and_single(torch_mod):
    torch = torch_mod
    _, od, _, _ = mods()
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd._call import dptr, ptr
    case = oc.sensors_case(1)
    keys = ("stats", "stat_rows") + SUMMARY + ("rows", "counts", "estimate_rows")
    out = {}
    a = run(case, executed=True, estimates=True, out=out)
    torch.cuda.synchronize()
    ha = host(a)
    ptrs = {k: out[k].data_ptr() for k in keys}
    b = run(case, executed=True, estimates=True, out=out)
    torch.cuda.synchronize()
    assert all(out[k].data_ptr() == ptrs[k] for k in keys)                  # out= is reused
    hb = host(b)
    live = np.arange(ha["rows"].shape[1])[None, :] < ha["counts"][:, :1]
    for k in keys:
        x, y = (ha[k][live], hb[k][live]) if k in ("rows", "estimate_rows") else (ha[k], hb[k])
        assert (x.view(np.int64 if x.dtype.itemsize == 8 else np.int32) == y.view(np.int64 if y.dtype.itemsize == 8 else np.int32)).all(), k
    # a single trajectory
    n0 = int(case["counts"][0])
    s = od.rollouts(case["rows"][0, :n0], None, follower_of(case["follower"]), case["P"][0], case["O"][0], sensors=case["sensors"],
                    scene=scene_of(case["scene"]), rule=rule_of(case["rule"]), time_step=DT, estimates=True)
    assert s["stats"].shape == (5, 8) and s["worst"].dim() == 0 and s["estimate_rows"].shape[0] == 5
    assert (s["stats"].cpu().numpy().view(np.int64) == ha["stats"][0].view(np.int64)).all()

    # every output pointer NULL in turn, and the refusals, through the C-ABI
    dev = torch.device("cuda", 0)
    rows = torch.as_tensor(case["rows"], device=dev)
    counts = torch.as_tensor(case["counts"], device=dev)
    P, O = torch.as_tensor(case["P"], device=dev), torch.as_tensor(case["O"], device=dev)
    B, cap = rows.shape[:2]
    K = P.shape[1]
    f = follower_of(case["follower"])
    cap_exec = cap + f.settle_rows
    sc = scene_of(case["scene"])
    sens = np.ascontiguousarray(case["sensors"])
    ctx = _lib.default_context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    names = ("stats", "stat_rows", "worst", "mean", "worst_rollout", "worst_row", "n_exceeding", "rows", "counts", "estimate_rows")
    SENT = 7

    def fresh():
        d = {k: out[k].clone() for k in names}
        for v in d.values():
            v.fill_(SENT)
        return d

    def call(o, skip=None, fs=None, rule=case["rule"], n_sens=1, sensors=sens, odo=O, cap_exec=cap_exec, K=K, off=None):
        fs = fs or f.as_struct()
        rs = None if rule is None else _lib.ResetRuleStruct(rule["gate"], rule["min_cos"], rule["gain"], rule["every"])
        p = {k: (None if k == skip else ptr(o[k])) for k in names}
        if off:
            p[off] = C.c_void_p(o[off].data_ptr() + 8)
        return ctx._L.vap_odometry_rollouts(
            ctx.handle, B, cap, ptr(rows), ptr(counts), 1, DT, C.byref(fs), K, 0, ptr(P), 0,
            None if odo is None else (C.c_void_p(O.data_ptr() + 8) if odo is Ellipsis else ptr(odo)), n_sens,
            None if sensors is None else dptr(sensors), None if rs is None else C.byref(rs), dptr(sc.field), sc.n_polygons,
            sc.poly_start.ctypes.data_as(_lib.ip), dptr(sc.poly_xy), sc.n_circles, dptr(sc.circles), p["stats"], p["stat_rows"], p["worst"],
            p["mean"], p["worst_rollout"], p["worst_row"], p["n_exceeding"], cap_exec, p["rows"], p["counts"], p["estimate_rows"])

    for skip in names:
        o = fresh()
        assert call(o, skip=skip) == _lib.VAP_OK
        torch.cuda.synchronize()
        assert (o[skip] == SENT).all(), skip
        for k in names:
            if k != skip and k not in ("rows", "estimate_rows"):
                g = o[k].cpu().numpy()
                assert (g.view(np.int64 if g.dtype.itemsize == 8 else np.int32) == ha[k].view(np.int64 if g.dtype.itemsize == 8 else np.int32)).all(), (skip, k)

    def rule_with(**kw):
        r = dict(case["rule"])
        r.update(kw)
        return r

    bad_sens = sens.copy()
    bad_sens[0, 2] = 0.5
    refusals = {
        "n_sens -1": dict(n_sens=-1), "n_sens 9": dict(n_sens=9), "gate < 0": dict(rule=rule_with(gate=-0.1)),
        "gate inf": dict(rule=rule_with(gate=np.inf)), "gate nan": dict(rule=rule_with(gate=np.nan)),
        "min_cos > 1": dict(rule=rule_with(min_cos=1.5)), "min_cos < 0": dict(rule=rule_with(min_cos=-0.1)),
        "gain > 1": dict(rule=rule_with(gain=1.01)), "gain < 0": dict(rule=rule_with(gain=-1.0)), "every 0": dict(rule=rule_with(every=0)),
        "every 10001": dict(rule=rule_with(every=10001)), "null rule": dict(rule=None), "null sensors": dict(sensors=None),
        "null odometry": dict(odo=None), "misaligned odometry": dict(odo=Ellipsis), "misaligned estimate rows": dict(off="estimate_rows"),
        "a beam that is no unit vector": dict(sensors=bad_sens), "cap_exec too small": dict(cap_exec=cap_exec - 1),
        "K 0": dict(K=0), "n_substeps 0": dict(fs=_lib.FollowerStruct(1.0, 2.0, 0.7, 6.0, 0.25, 0, 10)),
    }
    for what, kw in refusals.items():
        o = fresh()
        assert call(o, **kw) == _lib.VAP_ERR_INVALID, what
        torch.cuda.synchronize()
        assert all((o[k] == SENT).all() for k in names), what
