"""GPU: the follower rollouts ON their decisions.  The inputs of tests/rollout_exact_cases.py (stationary routes and on-axis
routes whose every product is exact, so an FMA contraction cannot change a bit) through tracking.rollouts, odometry.rollouts and
tracking.rollout_clearance against the float64 NumPy references with nothing excused: every float output the same bits, the
sign of a zero and the place of every NaN included, every integer output equal, no AMBIGUOUS window, 0 % of the rollouts
excluded.  Each case runs twice for the same bits, and the follower calls once more without executed rows.  test_rollout_exact_cpu.py holds those
references to the header in exact rational arithmetic on the same inputs, and shows that each family notices its rule switched.

The executed rows and the estimate rows are written into buffers filled with NaN: rows past a rollout's count stay NaN."""
import functools

import numpy as np
import pytest

import rollout_exact_cases as xc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def reference(fam, name):
    return xc.reference(xc.family(fam)[name])


def follower_of(case):
    from vexautonomousplanner_amd import tracking
    return (tracking.Pursuit if case["kind"] == "pursuit" else tracking.Follower)(**case["f"])


def scene_of(field, polygons=()):
    from vexautonomousplanner_amd import footprint
    return footprint.Scene(field=field, polygons=[np.asarray(p) for p in polygons], circles=[])


def run(torch, case, executed=True, clear=True):
    """One call of the case: vap_rollout_clearance where the case has a scene (clear False: the follower's own call with
    executed rows), else the follower's call.  Returns the outputs in the reference's layout."""
    from vexautonomousplanner_amd import odometry, tracking
    kind, fol = case["kind"], follower_of(case)
    B, cap = case["rows"].shape[:2]
    K, T = case["P"].shape[1], cap + int(case["f"]["settle_rows"])
    dev = torch.device("cuda", 0)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    out = {"rows": nan(B * K, T, 8), "estimate_rows": nan(B * K, T, 4)} if executed else None
    keys = [k for k in xc.keys_of(case) if executed or k not in ("rows", "counts", "est_rows")]
    if case["clear"] and clear:
        c = case["clear"]
        res = tracking.rollout_clearance(case["rows"], case["counts"], fol, case["P"], c["foot"], scene_of(c["field"], c["polygons"]),
                                         margin=c["margin"], time_step=case["dt"])
        keys = [k for k in keys if k not in ("rows", "counts")]
    elif kind == "odometry":
        has = case["sensors"] is not None
        r = case["rule"]
        res = odometry.rollouts(case["rows"], case["counts"], fol, case["P"], case["O"], sensors=case["sensors"] if has else None,
                                scene=scene_of(case["field"]) if has else None,
                                rule=odometry.ResetRule(r["gate_in"], r["max_incidence_deg"], r["gain"], r["every"]) if has else None,
                                time_step=case["dt"], executed=executed, estimates=executed, out=out)
        if has:
            assert (odometry.ResetRule(r["gate_in"], r["max_incidence_deg"], r["gain"], r["every"]).gate, r["min_cos"]) == (r["gate"], 1.0)
    else:
        res = tracking.rollouts(case["rows"], case["counts"], fol, case["P"], time_step=case["dt"], executed=executed, out=out)
        keys = [k for k in keys if not k.startswith("clear") and k not in xc.CLEAR_SUMMARY]
    torch.cuda.synchronize()
    got = {}
    for k in keys:
        a = res[{"est_rows": "estimate_rows"}.get(k, k)]
        if executed and k in ("rows", "est_rows"):
            assert a.data_ptr() == out[{"est_rows": "estimate_rows"}.get(k, k)].data_ptr()
        a = a.cpu().numpy()
        if k == "counts":
            assert (a[:, 1] == 0).all()
            a = a[:, 0]
        got[k] = a
    return got


def check(torch, fam, name):
    case, ref = xc.family(fam)[name], reference(fam, name)
    got = run(torch, case)
    d = xc.same(got, ref, list(got))
    assert d is None, (name, d)
    again = run(torch, case)
    assert xc.same(got, again, list(got)) is None, (name, "a second call")
    if not case["clear"]:                      # vap_rollout_clearance writes no executed rows: there is no second form of it
        plain = run(torch, case, executed=False)
        assert xc.same(plain, ref, list(plain)) is None, (name, "without executed rows", xc.same(plain, ref, list(plain)))
    return got, ref["stats"].shape[0] * ref["stats"].shape[1]


@pytest.mark.parametrize("fam", ["wrap", "first", "drive", "contraction", "validity", "pointers", "gate"])
def test_family_bit_for_bit(torch_mod, fam):
    n = 0
    for name in xc.family(fam):
        n += check(torch_mod, fam, name)[1]
    print(f"ROLLOUT EXACT {fam}: {len(xc.family(fam))} cases, {n} rollouts bit for bit, nothing excused")


def test_odometry_with_the_ideal_record_is_ramsete(torch_mod):
    """'With the ideal record and a zero start offset the call equals vap_tracking_rollouts': here the start has a heading
    offset only, and the estimate's heading error is the true one."""
    a = run(torch_mod, xc.family("wrap")["wrap ramsete"])
    b = run(torch_mod, xc.family("wrap")["wrap odometry"])
    assert xc.same(dict(a, stats=a["stats"][..., :5]), dict(b, stats=b["stats"][..., :5], stat_rows=b["stat_rows"][..., :2]),
                   ("stats", "stat_rows", "rows", "counts") + xc.SUMMARY) is None
    assert (b["stats"][..., 6].view(np.int64) == b["stats"][..., 2].view(np.int64)).all() and (b["stat_rows"][..., 2:] == 0).all()


@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
def test_clearance_fold_in_three_layouts(torch_mod, kind):
    """ClearAcc::fold and ClearSummary on ties: the split kernel (a workgroup a CU), the lane kernel (more workgroups than CUs),
    K > 256 (the reduce kernel) and the two-call form, executed rows then footprint.clearance, agree bit for bit."""
    from vexautonomousplanner_amd import footprint
    torch = torch_mod
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 0
    per_record = {}
    for name, case in xc.family("clear").items():
        if not name.endswith(kind):
            continue
        got, m = check(torch, "clear", name)
        n += m
        B, K = case["P"].shape[:2]
        grid = (B + 256 // K - 1) // (256 // K) if K <= 256 else B * ((K + 255) // 256)
        assert (grid > cus) == ("lanes" in name), (name, grid, cus)
        # the two-call form: the follower's executed rows, then vap_footprint_clearance with counts_stride 2
        ex = run(torch, case, clear=False)
        assert xc.same(ex, reference("clear", name), list(ex)) is None, name
        c = case["clear"]
        two = footprint.clearance(torch.as_tensor(ex["rows"], device="cuda"), torch.as_tensor(ex["counts"].astype(np.int32), device="cuda"),
                                  c["foot"], scene_of(c["field"], c["polygons"]), margin=c["margin"])
        torch.cuda.synchronize()
        rows4 = np.stack([two[k].cpu().numpy() for k in ("min_row", "min_element", "first_row", "n_below")], axis=1).reshape(B, K, 4)
        assert xc.same({"clearance": two["min_clearance"].cpu().numpy().reshape(B, K), "clear_rows": rows4}, got, ("clearance", "clear_rows")) is None, name
        if c["margin"] == 0.25 and "mean" not in name:      # the same records under every layout: the same bits, row and element per record
            for k in range(4):                # (the rows below the margin count the route's rows, 8 or 9)
                key = case["P"][0, k].tobytes()
                mine = (got["clearance"][0, k].tobytes(), got["clear_rows"][0, k, :3].tolist())
                assert per_record.setdefault(key, mine) == mine, (name, k)
    print(f"ROLLOUT EXACT clear {kind}: {n} rollouts bit for bit in the split, lane and reduce layouts and the two-call form ({cus} CUs)")
