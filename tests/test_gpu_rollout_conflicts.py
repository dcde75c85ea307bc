"""GPU: clearance of the disturbed rollouts to the partner's routines (vap_rollout_conflicts, tracking.rollout_conflicts,
BatchedTrajectoryGenerator.rollout_conflicts, search.refine(robust_conflicts=True)).

The contract is a composition, and the tests hold it bit for bit, on integers: per rollout the pair and route outputs are
those of ``tracking.rollouts(executed=True)`` followed by ``footprint.conflicts`` on that executed route at the rollout's own
shift (one conflicts call per distinct shift, on the executed routes that carry it); the per-route outputs are the
ascending-k fold of the call's own per-rollout outputs; the follower's outputs are those of plain ``rollouts``.  Against the
NumPy composition of tests/rollout_conflicts_ref.py the golden routes are held to the rule of test_gpu_rollout_clearance.py:
1e-9 ft, the row may be any row within 1e-9 of the minimum, counts are compared where no pair is within 1e-9 of the margin;
a RAMSETE rollout whose reference max |e_phi| >= 3.0 rad sits at the wrap's discontinuity and is left out of that
comparison, at most 2 % of a test's rollouts."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import pursuit_ref as pr
import rollout_clearance_ref as rc
import rollout_conflicts_ref as xr
import tracking_ref as tr

pytestmark = pytest.mark.gpu

DT = 0.01
AMBIGUOUS = 1e-9
EXCLUDE_RAD = 3.0
FOLLOWER_KEYS = {"ramsete": ("stats", "stat_rows", "worst", "mean", "worst_rollout", "worst_row", "n_exceeding"),
                 "pursuit": ("stats", "stat_rows", "worst", "mean", "worst_rollout", "worst_row", "n_exceeding", "n_unfinished",
                             "route_status")}
ROUTE_KEYS = xr.ROUTE_KEYS
CONFLICT_KEYS = ("conflict", "conflict_rows") + ROUTE_KEYS
PAIR_KEYS = ("pair_clearance", "pair_rows")


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


class Pair:
    """The pair of calls, its rollouts run once: ``rollouts(executed=True)`` and plain ``rollouts`` of one batch."""

    def __init__(self, torch, kind, rows, counts, follower, P, ctx=None):
        tk = trk()
        self.torch, self.kind, self.ctx = torch, kind, ctx
        self.ex = tk.rollouts(rows, counts, follower, P, time_step=DT, executed=True, ctx=ctx)
        self.plain = tk.rollouts(rows, counts, follower, P, time_step=DT, ctx=ctx)
        torch.cuda.synchronize()

    def check(self, fused, foot, rows_o, counts_o, foot_o, margin, sums, what=""):
        """The fused call's outputs (pairs=True) against ``footprint.conflicts`` per distinct shift of ``sums`` (B, K) on the
        executed routes that carry it, the follower's outputs against plain rollouts, and the per-route outputs against the fold
        of the call's own per-rollout ones."""
        torch, fp = self.torch, FP()
        B, K = fused["conflict"].shape
        Bo = fused["pair_clearance"].shape[2]
        assert fused["conflict_rows"].shape == (B, K, 4) and fused["pair_rows"].shape == (B, K, Bo, 2) and self.ex["rows"].shape[0] == B * K
        flat = np.asarray(sums, dtype=np.int64).reshape(-1)
        distinct = np.unique(flat)
        assert len(distinct) <= 8
        pc, prw = fused["pair_clearance"].reshape(B * K, Bo), fused["pair_rows"].reshape(B * K, Bo, 2)
        cf, cr4 = fused["conflict"].reshape(B * K), fused["conflict_rows"].reshape(B * K, 4)
        for s in distinct:
            idx = torch.tensor(np.nonzero(flat == s)[0], device=pc.device)
            two = fp.conflicts(self.ex["rows"][idx].contiguous(), self.ex["counts"][idx].contiguous(), foot, rows_o, counts_o, foot_o,
                               margin=margin, shift_rows=int(s), pairs=True, ctx=self.ctx)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(bits(pc[idx]), bits(two["pair_clearance"]), err_msg=f"{what} shift {s}: pair_clearance")
            np.testing.assert_array_equal(bits(prw[idx]), bits(torch.stack([two["pair_row"], two["pair_first_row"]], dim=2)),
                                          err_msg=f"{what} shift {s}: pair_rows")
            np.testing.assert_array_equal(bits(cf[idx]), bits(two["min_clearance"]), err_msg=f"{what} shift {s}: conflict")
            want = torch.stack([two["min_other"], two["min_row"], two["n_conflicts"], two["first_row"]], dim=1)
            np.testing.assert_array_equal(bits(cr4[idx]), bits(want), err_msg=f"{what} shift {s}: conflict_rows")
        for i, name in enumerate(trk().CONFLICT_ROW_COLUMNS):
            assert torch.equal(fused[name], fused["conflict_rows"][..., i])
        assert_same_bits(fused, self.plain, FOLLOWER_KEYS[self.kind], f"{what} follower outputs against plain rollouts")
        assert_same_bits(fused, self.ex, FOLLOWER_KEYS[self.kind], f"{what} follower outputs against rollouts(executed=True)")
        check_fold(fused, margin, what)


def check_fold(fused, margin, what=""):
    c, r = fused["conflict"].cpu().numpy(), fused["conflict_rows"].cpu().numpy()
    got = {k: fused[k].cpu().numpy() for k in ROUTE_KEYS}
    for b in range(c.shape[0]):
        s = xr.fold(c[b], r[b], margin)
        for k in ROUTE_KEYS:
            np.testing.assert_array_equal(got[k][b], s[k], err_msg=f"{what} route {b}: {k}")       # NaN equals NaN, else exact


# ---- 1., 4., 5. bit for bit against the pair of calls: layouts, partner counts, the ways a shift arrives ----------------
@pytest.mark.parametrize("Bo", xr.OTHERS)
@pytest.mark.parametrize("kind,K,B,_", rc.LAYOUTS)
def test_bits_against_the_pair_of_calls(torch_mod, kind, K, B, _, Bo):
    torch = torch_mod
    tk, fp = trk(), FP()
    rows, counts, P = rc.layout_case(kind, K, B)
    rows_o, counts_o, b_ref = xr.partners(rows, counts, xr.PARTNER_SEEDS[(kind, K, B)], Bo)
    assert rows_o.shape == (Bo, xr.CAP_O, 8) and counts_o.shape == (Bo, 2)
    foot = fp.rectangle(18, 18)
    follower = make_follower(kind, settle_rows=xr.SETTLE, n_substeps=3, tolerance=0.1)
    dev = "cuda:0"
    d_rows, d_counts = torch.tensor(rows, device=dev), torch.tensor(counts, device=dev)
    d_rows_o, d_counts_o = torch.tensor(rows_o, device=dev), torch.tensor(counts_o, device=dev)
    pair = Pair(torch, kind, d_rows, d_counts, follower, P)

    def fused_call(mode, P=P, **kw):
        h, rs, ks = xr.layout_shifts(kind, K, B, b_ref, counts, mode)
        kw = {"pairs": True, **kw}
        res = tk.rollout_conflicts(d_rows, d_counts, follower, P, foot, d_rows_o, d_counts_o, margin=xr.MARGIN, shift_rows=h, route_shift=rs,
                                   rollout_shift=ks, time_step=DT, **kw)
        torch.cuda.synchronize()
        return res, xr.sums(h, rs, ks, B, K)

    results = {}
    for mode in ("route", "rollout", "host", "all"):
        results[mode], s = fused_call(mode)
        pair.check(results[mode], foot, d_rows_o, d_counts_o, None, xr.MARGIN, s, what=mode)
    assert_same_bits(results["route"], results["all"], FOLLOWER_KEYS[kind] + CONFLICT_KEYS + PAIR_KEYS, "the same sums, delivered in three parts")
    mode = xr.primary_mode(K)
    fused = results[mode]
    again, _s = fused_call(mode, P=torch.tensor(P, device=dev))
    nocull, _s = fused_call(mode, cull=False)
    nopairs, _s = fused_call(mode, pairs=False)
    assert_same_bits(fused, again, FOLLOWER_KEYS[kind] + CONFLICT_KEYS + PAIR_KEYS, "two calls")
    assert_same_bits(fused, nocull, FOLLOWER_KEYS[kind] + CONFLICT_KEYS + PAIR_KEYS, "cull off")
    assert_same_bits(fused, nopairs, FOLLOWER_KEYS[kind] + CONFLICT_KEYS, "pairs=False")
    assert "pair_clearance" not in nopairs and "pair_rows" not in nopairs
    # shared records: (K, 8) for every route equals the same records repeated per route
    Ps = P[B - 1].copy()
    shared, _s = fused_call(mode, P=Ps)
    repeated, _s = fused_call(mode, P=np.repeat(Ps[None], B, axis=0))
    assert_same_bits(shared, repeated, FOLLOWER_KEYS[kind] + CONFLICT_KEYS + PAIR_KEYS, "shared records")
    # the edge outputs are the header's (that the partners bite is held on the reference, on the CPU)
    e = B // 2                                                                      # a route without rows
    assert torch.isnan(fused["conflict"][e]).all() and (fused["conflict_rows"][e, :, [0, 1, 3]] == -1).all() and (fused["conflict_rows"][e, :, 2] == 0).all()
    assert torch.isnan(fused["pair_clearance"][e]).all() and (fused["pair_rows"][e] == -1).all()
    assert torch.isnan(fused["worst_conflict"][e]) and torch.isnan(fused["mean_conflict"][e])
    assert [int(fused[k][e]) for k in ROUTE_KEYS if k not in ("worst_conflict", "mean_conflict")] == [-1, -1, -1, 0, 0]
    if K >= 3:
        assert torch.isnan(fused["conflict"][:, K // 2]).all() and (fused["conflict_rows"][:, K // 2, 1] == -1).all()
        assert (fused["worst_conflict_rollout"] != K // 2).all()
    else:
        assert torch.isnan(fused["worst_conflict"][3]) and int(fused["n_conflict_valid"][3]) == 0
    if kind == "pursuit":
        assert int(fused["route_status"][2]) == 1 and torch.isnan(fused["conflict"][2]).all() and int(fused["n_conflict_valid"][2]) == 0
    if Bo >= 3:                                                                     # partner 1 has no rows: an invalid pair never wins
        assert torch.isnan(fused["pair_clearance"][:, :, 1]).all() and (fused["pair_rows"][:, :, 1] == -1).all()
        assert (fused["conflict_other"] != 1).all()
    if Bo == 16:
        assert torch.isnan(fused["pair_clearance"][:, :, 4]).all() and (fused["conflict_other"] != 4).all()      # count -3
    c = fused["conflict"].cpu().numpy()
    ncon, nval = fused["n_conflicting"].cpu().numpy(), fused["n_conflict_valid"].cpu().numpy()
    print(f"{kind} K = {K}, B = {B}, Bo = {Bo}: {int((c < 0).sum())} rollouts in contact, {int(((ncon > 0) & (ncon < nval)).sum())} mixed routes")


# ---- 2. side O's edge cases under count strides 3 and 1 ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
@pytest.mark.parametrize("stride", [3, 1])
def test_side_o_edge_cases_and_count_strides(torch_mod, kind, stride):
    """Partners 0 .. 5 of the layout's set: a full drive, count 0, count 1, count cap_o + 500, count -3, a NaN heading in one
    row; the counts in column 0 of (Bo, 3) or as (Bo,)."""
    torch = torch_mod
    tk, fp = trk(), FP()
    K, B, Bo = 16, 20, 6
    rows, counts, P = rc.layout_case(kind, K, B)
    rows_o, counts_o, b_ref = xr.partners(rows, counts, xr.PARTNER_SEEDS[(kind, K, B)], Bo)
    assert counts_o[:, 0].tolist()[1:5] == [0, 1, xr.CAP_O + 500, -3] and np.isnan(rows_o[5, :counts_o[5, 0], 4]).sum() == 1
    c_o = counts_o[:, 0].copy() if stride == 1 else np.concatenate([counts_o, np.full((Bo, 1), 77, dtype=np.int32)], axis=1)
    foot = fp.rectangle(18, 18)
    follower = make_follower(kind, settle_rows=xr.SETTLE, n_substeps=3, tolerance=0.1)
    dev = "cuda:0"
    d_rows, d_counts = torch.tensor(rows, device=dev), torch.tensor(counts, device=dev)
    d_rows_o, d_counts_o = torch.tensor(rows_o, device=dev), torch.tensor(np.ascontiguousarray(c_o), device=dev)
    h, rs, ks = xr.layout_shifts(kind, K, B, b_ref, counts, "rollout")
    fused = tk.rollout_conflicts(d_rows, d_counts, follower, P, foot, d_rows_o, d_counts_o, margin=xr.MARGIN, rollout_shift=ks, pairs=True,
                                 time_step=DT)
    torch.cuda.synchronize()
    Pair(torch, kind, d_rows, d_counts, follower, P).check(fused, foot, d_rows_o, d_counts_o, None, xr.MARGIN, xr.sums(h, rs, ks, B, K))
    for o in (1, 4):
        assert torch.isnan(fused["pair_clearance"][:, :, o]).all() and (fused["pair_rows"][:, :, o] == -1).all() and (fused["conflict_other"] != o).all()
    live = fused["conflict_row"] >= 0
    assert live.any() and torch.isfinite(fused["pair_clearance"][..., 5][live]).all()      # the NaN row takes part in nothing; the others do


# ---- 3. deep overlap: saturated ties over many rows and across partners ------------------------------------------------
@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
def test_deep_overlap_keeps_the_first_row_and_the_smallest_other(torch_mod, kind):
    """Three partners parked ON the route (the same pose, twice, and one further along): the clearance saturates at minus the
    footprint's extent over many rows and ties exactly between partners 0 and 1, so partner 1 never wins (partner 2 saturates
    at the same extent to the last bits, and may)."""
    torch = torch_mod
    tk, fp = trk(), FP()
    rng = np.random.default_rng(3)
    rows = rc.synth_rows(rng, 4, 100)
    counts = np.array([100, 80, 100, 60], dtype=np.int32)
    rows_o = np.zeros((3, 4, 8))
    rows_o[0, :] = rows_o[1, :] = rows[0, 40]
    rows_o[2, :] = rows[0, 70]
    counts_o = np.array([4, 4, 1], dtype=np.int32)
    K = 8
    P = tk.sample_perturbations(4, K, seed=2, pos_sigma=0.02, heading_sigma=0.01)
    foot = fp.rectangle(18, 18)
    follower = make_follower(kind, settle_rows=10)
    dev = "cuda:0"
    d_rows, d_counts = torch.tensor(rows, device=dev), torch.tensor(counts, device=dev)
    d_rows_o, d_counts_o = torch.tensor(rows_o, device=dev), torch.tensor(counts_o, device=dev)
    ks = np.array([0, 0, 5, 5, -5, -5, 200, 200], dtype=np.int32)
    fused = tk.rollout_conflicts(d_rows, d_counts, follower, P, foot, d_rows_o, d_counts_o, margin=0.05, rollout_shift=ks, pairs=True, time_step=DT)
    torch.cuda.synchronize()
    Pair(torch, kind, d_rows, d_counts, follower, P).check(fused, foot, d_rows_o, d_counts_o, None, 0.05, xr.sums(0, None, ks, 4, K))
    assert (fused["conflict"][0] < -0.5).all() and (fused["conflict_other"][0] != 1).all()          # deep, and the smaller o on the tie
    assert (fused["pair_rows"][0, :, 1, 0] == fused["pair_rows"][0, :, 0, 0]).all()
    np.testing.assert_array_equal(bits(fused["pair_clearance"][0, :, 0]), bits(fused["pair_clearance"][0, :, 1]))
    assert (fused["conflict_n"][0] >= 2).all()


# ---- 4. the C-ABI: every output NULL in turn, refusals, B = 0 ---------------------------------------------------------
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
        cap, settle, Bo, cap_o = 90, 10, 3, 150
        h_rows = rc.synth_rows(rng, B, cap)
        pad = torch.zeros(B * cap * 8 + 2, dtype=torch.float64, device="cuda:0")
        rows = pad[:B * cap * 8].view(B, cap, 8)
        rows.copy_(torch.tensor(h_rows))
        counts = torch.tensor(np.stack([rng.integers(20, cap + 1, B), np.zeros(B)], axis=1).astype(np.int32), device="cuda:0")
        P = torch.tensor(tk.sample_perturbations(B, K, seed=K), device="cuda:0")
        h_o = rc.synth_rows(rng, Bo, cap_o)
        h_o[0, :, 6:8] += h_rows[0, 40, 6:8] - h_o[0, 40, 6:8] + 0.8
        rows_o = torch.tensor(h_o, device="cuda:0")
        counts_o = torch.tensor(np.array([[cap_o, 0], [60, 0], [100, 0]], dtype=np.int32), device="cuda:0")
        ks = torch.tensor((np.arange(K) % 3 * 40 - 30).astype(np.int32), device="cuda:0")
        rs = torch.tensor((np.arange(B) % 2 * 7).astype(np.int32), device="cuda:0")
        fs = make_follower(kind, settle_rows=settle).as_struct()
        i32, f64 = torch.int32, torch.float64
        spec = [((B, K, 6), f64), ((B, K, 4 if pursuit else 2), i32), ((B,), f64), ((B,), f64), ((B,), i32), ((B,), i32), ((B,), i32)]
        spec += [((B,), i32), ((B,), i32)] if pursuit else []
        spec += [((B, K, Bo), f64), ((B, K, Bo, 2), i32), ((B, K), f64), ((B, K, 4), i32), ((B,), f64), ((B,), i32), ((B,), i32), ((B,), i32),
                 ((B,), f64), ((B,), i32), ((B,), i32)]

        def fresh():
            return [torch.full(s, -7, dtype=d, device="cuda:0") for s, d in spec]

        def call(outs, skip=None, K=K, foot_o=foot, rows_ptr=None, unfinished=None, B=B, Bo=Bo, shift=3, margin=0.1):
            p = [C.c_void_p(t.data_ptr()) if i != skip else None for i, t in enumerate(outs)]
            if not pursuit:
                p[7:7] = [unfinished, None]
            st = L.vap_rollout_conflicts(ctx.handle, 1 if pursuit else 0, C.cast(C.pointer(fs), C.c_void_p), B, cap,
                                         C.c_void_p(rows.data_ptr() if rows_ptr is None else rows_ptr), C.c_void_p(counts.data_ptr()), 2, DT,
                                         K, 0, C.c_void_p(P.data_ptr()), 4, foot.ctypes.data_as(_lib.dp), Bo, cap_o, C.c_void_p(rows_o.data_ptr()),
                                         C.c_void_p(counts_o.data_ptr()), 2, 4, foot_o.ctypes.data_as(_lib.dp), margin, shift,
                                         C.c_void_p(rs.data_ptr()), C.c_void_p(ks.data_ptr()), *p)
            ctx.synchronize()
            return st

        full = fresh()
        assert call(full) == _lib.VAP_OK, L.vap_last_error()
        assert not any((t == -7).all() for t in full)
        for skip in range(len(spec)):
            outs = fresh()
            assert call(outs, skip=skip) == _lib.VAP_OK, skip
            for i, (a, b) in enumerate(zip(outs, full)):
                if i == skip:
                    assert (a == -7).all(), (skip, "a skipped output was written")
                else:
                    assert torch.equal(a.view(i32), b.view(i32)), (skip, i)
        p_none = [None] * 20                                        # every output NULL at once
        assert L.vap_rollout_conflicts(ctx.handle, 1 if pursuit else 0, C.cast(C.pointer(fs), C.c_void_p), B, cap, C.c_void_p(rows.data_ptr()),
                                       C.c_void_p(counts.data_ptr()), 2, DT, K, 0, C.c_void_p(P.data_ptr()), 4, foot.ctypes.data_as(_lib.dp), Bo,
                                       cap_o, C.c_void_p(rows_o.data_ptr()), C.c_void_p(counts_o.data_ptr()), 2, 4, foot.ctypes.data_as(_lib.dp),
                                       0.1, 3, None, None, *p_none) == _lib.VAP_OK
        ctx.synchronize()
        # refusals, each with a message
        if not pursuit:
            assert call(fresh(), unfinished=C.c_void_p(counts.data_ptr())) == INV and b"d_n_unfinished" in L.vap_last_error()
        assert call(fresh(), foot_o=np.ascontiguousarray(foot[::-1])) == INV and b"clockwise" in L.vap_last_error()
        assert call(fresh(), Bo=0) == INV and b"Bo" in L.vap_last_error()
        assert call(fresh(), Bo=17) == UNS and b"Bo" in L.vap_last_error()
        assert call(fresh(), shift=(1 << 24) + 1) == INV and b"shift_rows" in L.vap_last_error()
        assert call(fresh(), margin=float("nan")) == INV and b"margin" in L.vap_last_error()
        assert call(fresh(), rows_ptr=pad.data_ptr() + 8) == INV and b"aligned" in L.vap_last_error()
        assert call(fresh(), K=0) == INV and L.vap_last_error() and call(fresh(), K=4097) == INV and L.vap_last_error()
        assert call(fresh(), B=0) == _lib.VAP_OK                    # B = 0 is a no-op
    ctx.close()


@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
def test_host_input_single_trajectory_generator_and_out(torch_mod, kind):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    torch = torch_mod
    tk, fp = trk(), FP()
    rng = np.random.default_rng(8)
    rows = rc.synth_rows(rng, 3, 100)
    counts = np.array([100, 60, 80], dtype=np.int32)
    rows_o = rc.synth_rows(rng, 2, 150)
    rows_o[0, :, 6:8] += rows[1, 30, 6:8] - rows_o[0, 30, 6:8] + 1.0
    counts_o = np.array([150, 90], dtype=np.int32)
    follower = make_follower(kind, settle_rows=5)
    P = tk.sample_perturbations(3, 4, seed=2)
    foot = fp.rectangle(18, 18)
    keys = FOLLOWER_KEYS[kind] + CONFLICT_KEYS
    kw = dict(margin=0.1, shift_rows=-4, rollout_shift=[0, 9, -9, 30])
    d = lambda a: torch.tensor(a, device="cuda:0")
    dev = tk.rollout_conflicts(d(rows), d(counts), follower, P, foot, d(rows_o), d(counts_o), **kw)
    bufs = {}
    host = tk.rollout_conflicts(rows, counts, follower, P, foot, rows_o, counts_o, out=bufs, **kw)
    gen = BatchedTrajectoryGenerator(0, "f64")
    via = gen.rollout_conflicts({"rows": d(rows), "counts": d(counts)}, follower, P, foot, {"rows": d(rows_o), "counts": d(counts_o)}, **kw)
    torch.cuda.synchronize()
    assert_same_bits(dev, host, keys, "host arrays")
    assert_same_bits(dev, via, keys, "the generator's method")
    assert set(bufs) == set(keys)
    ptrs = {k: t.data_ptr() for k, t in bufs.items()}
    tk.rollout_conflicts(rows, counts, follower, P, foot, rows_o, counts_o, out=bufs, **kw)
    assert {k: t.data_ptr() for k, t in bufs.items()} == ptrs
    # a single trajectory on either side: (K, ...) and 0-d tensors; out= keeps the batch-shaped buffers
    sb = {}
    one = tk.rollout_conflicts(rows[1, :60], None, follower, P[1], foot, rows_o, counts_o, out=sb, pairs=True, **kw)
    torch.cuda.synchronize()
    assert one["conflict"].shape == (4,) and one["conflict_rows"].shape == (4, 4) and one["conflict_other"].shape == (4,)
    assert one["pair_clearance"].shape == (4, 2) and one["pair_rows"].shape == (4, 2, 2)
    assert one["worst_conflict"].dim() == 0 and one["n_conflicting"].dim() == 0 and one["stats"].shape == (4, 6)
    assert sb["conflict"].shape == (1, 4) and sb["worst_conflict"].shape == (1,)
    for k in keys:
        np.testing.assert_array_equal(bits(one[k]), bits(dev[k][1]), err_msg=k)
    lone = tk.rollout_conflicts(rows[1, :60], None, follower, P[1], foot, rows_o[0, :150], None, pairs=True, **kw)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(lone["pair_clearance"][:, 0]), bits(one["pair_clearance"][:, 0]))


# ---- 6. the golden routes' full rows (stride-3 counts), the partner the same route mirrored ---------------------------
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


@pytest.mark.parametrize("kind,name", [("ramsete", "feat_turn"), ("ramsete", "feat_reverse"), ("ramsete", "feat_wait"),
                                       ("pursuit", "feat_turn"), ("pursuit", "feat_wait")])
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
    rows_o, counts_o = xr.mirrored(rows[:1], counts[:1])
    others = {"rows": torch.tensor(rows_o, device=gen.device), "counts": torch.tensor(counts_o, device=gen.device)}
    margin = 0.1
    ks = xr.GOLDEN_JITTER
    fused = gen.rollout_conflicts(out, follower, P, foot, others, margin=margin, rollout_shift=ks, pairs=True, time_step=DT)
    torch.cuda.synchronize()
    Pair(torch, kind, out["rows"], out["counts"], follower, P, ctx=gen.ctx).check(fused, foot, others["rows"], others["counts"], None, margin,
                                                                                  xr.sums(0, None, ks, 2, K))
    # against the NumPy composition
    c, r = fused["conflict"].cpu().numpy(), fused["conflict_rows"].cpu().numpy()
    f = (tr.follower if kind == "ramsete" else pr.pursuit)(**{k: getattr(follower, k) for k in (tr.DEFAULTS if kind == "ramsete" else pr.DEFAULTS)})
    n_cmp = n_exc = 0
    worst = 0.0
    for b in range(2):
        ref = xr.route(rows[b], counts[b], kind, f, P[b], foot, rows_o, counts_o, margin=margin, shifts=ks)
        for k in range(K):
            s = ref["per"][k]
            if kind == "ramsete" and np.nan_to_num(ref["rollout"]["stats"][k, 2]) >= EXCLUDE_RAD:
                n_exc += 1
                assert np.isfinite(c[b, k])
                continue
            n_cmp += 1
            assert r[b, k, 1] >= 0 and s["min_row"][0] >= 0, (b, k)
            d = abs(c[b, k] - s["min_clearance"][0])
            worst = max(worst, d)
            assert d <= 1e-9, (b, k, c[b, k], s["min_clearance"][0])
            assert abs(s["pair_rows"][(0, 0)][int(r[b, k, 1])] - s["min_clearance"][0]) <= AMBIGUOUS, (b, k, "min row")
            if s["margin_gap"][0] > AMBIGUOUS:
                assert r[b, k, 2] == s["n_conflicts"][0] and r[b, k, 3] == s["first_row"][0], (b, k, "pairs below the margin")
    assert n_exc <= 0.02 * (n_cmp + n_exc), f"{n_exc} of {n_cmp + n_exc} rollouts at the wrap's discontinuity"
    print(f"{kind} {name}: {n} rows, {n_cmp} rollouts against the NumPy composition ({n_exc} left out), max diff {worst:.2e} ft; worst "
          f"conflict {fused['worst_conflict'][0].item():.4f} ft, {int(fused['n_conflicting'][0])} of {int(fused['n_conflict_valid'][0])} rollouts below {margin}")


# ---- the known answers on the device ------------------------------------------------------------------------------------
def test_known_answers_on_the_device(torch_mod):
    torch = torch_mod
    tk, fp = trk(), FP()
    rows, P, partner, cnt, expect = xr.known_case()
    res = tk.rollout_conflicts(rows, None, tk.Follower(settle_rows=xr.KNOWN_SETTLE), P, fp.rectangle(18, 18), partner, cnt, margin=xr.KNOWN_MARGIN)
    torch.cuda.synchronize()
    c = res["conflict"].cpu().numpy()
    print("known answer on the device:", c, res["conflict_rows"].cpu().numpy().tolist())
    assert c.shape == (3,) and np.abs(c - expect).max() <= 1e-12
    assert res["conflict_row"].tolist() == [0, 0, 0] and res["conflict_other"].tolist() == [0, 0, 0] and res["conflict_first_row"].tolist() == [-1, 0, -1]
    assert (int(res["n_conflicting"]), int(res["n_conflict_valid"]), int(res["worst_conflict_rollout"])) == (1, 3, 1)
    rows, P, partner, cnt = xr.crossing_case()
    res = tk.rollout_conflicts(rows, None, tk.Follower(settle_rows=xr.KNOWN_SETTLE), np.repeat(P, 2, axis=0), fp.rectangle(18, 18), partner, cnt,
                               rollout_shift=[0, xr.KNOWN_CROSS_JITTER])
    torch.cuda.synchronize()
    assert res["conflict"][0].item() > 0 and res["conflict"][1].item() < -1.0 and res["conflict_row"][1].item() == 20


# ---- 8. refine ---------------------------------------------------------------------------------------------------------
FIELD_B = (-6.0, -6.0, 6.0, 6.0)
LINE = np.array([[-4, 0], [-2, 0], [0, 0], [2, 0], [4, 0]], dtype=np.float64)
REFINE_KW = dict(dd=0.005, dt=DT, capacity=4096, capacity_rows=1024)


def test_refine_with_robust_conflicts(torch_mod):
    """One iteration with the option against search.rank of terms composed by hand from footprint.conflicts and
    tracking.rollout_conflicts: cost and order equal.  With the option False (and the two shift arguments at their
    defaults) the result has the bits of a call that does not name the new arguments."""
    from vexautonomousplanner_amd import search
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    torch = torch_mod
    tk, fp = trk(), FP()
    gen = BatchedTrajectoryGenerator(0, "f32")
    N = 128
    wts = search.Weights(conflict_margin=0.1)
    foot, scene = fp.rectangle(18, 18), fp.Scene(field=FIELD_B)
    follower = tk.Follower()
    P = tk.sample_perturbations(1, 8, seed=5)[0]
    jitter = np.array([0, 10, -10, 25, -25, 40, -40, 5], dtype=np.int32)
    # the partner drives up the line x = 0 across the seed, through the origin at its row 150
    m = 300
    o_rows = np.zeros((1, m, 8))
    t = np.arange(m) * DT
    o_rows[0, :, 0], o_rows[0, :, 1], o_rows[0, :, 2], o_rows[0, :, 4] = t, 2.0 * t, 2.0, -np.pi / 2
    o_rows[0, :, 7] = 2.0 * (np.arange(m) - 150) * DT
    others = {"rows": torch.tensor(o_rows, device=gen.device), "counts": torch.tensor(np.array([[m]], dtype=np.int32), device=gen.device)}
    cfg1 = search.SearchConfig(candidates=N, elites=16, iterations=1, weights=wts)
    out = gen.refine(LINE, 0.5, foot, scene, config=cfg1, others=others, follower=follower, perturbations=P, robust_conflicts=True,
                     others_shift_rows=20, others_start_jitter=jitter, **REFINE_KW)
    torch.cuda.synchronize()
    assert tuple(out["n_conflicting"].shape) == (1, N) and out["n_conflicting"].dtype == torch.int32
    # the same iteration by hand
    W = LINE.shape[0]
    mean = torch.tensor(LINE[None], device=gen.device)
    sigma = torch.full((1, W, 2), 0.5, dtype=torch.float64, device=gen.device)
    sigma[:, 0] = 0.0
    sigma[:, -1] = 0.0
    wp = search.sample(mean, sigma, N, seed=cfg1.seed, iteration=0, dtype=gen.tdtype, ctx=gen.ctx,
                       best_waypoints=torch.zeros((1, W, 2), dtype=gen.tdtype, device=gen.device),
                       best_cost=torch.full((1,), float("inf"), dtype=torch.float64, device=gen.device))
    prof = gen.profile(wp, dd=0.005, capacity=4096)
    tp = gen.time_profile(prof, dt=DT, capacity_rows=1024)
    clr = fp.clearance(tp["rows"], tp["counts"], foot, scene, margin=wts.clearance_margin, ctx=gen.ctx)
    planned = fp.conflicts(tp["rows"], tp["counts"], foot, others["rows"], others["counts"], margin=wts.conflict_margin, shift_rows=20, ctx=gen.ctx)
    rcf = tk.rollout_conflicts(tp["rows"], tp["counts"], follower, P, foot, others["rows"], others["counts"], margin=wts.conflict_margin,
                               shift_rows=20, rollout_shift=jitter, time_step=DT, ctx=gen.ctx)
    wc = rcf["worst_conflict"]
    term = torch.where(torch.isnan(wc), planned["min_clearance"], torch.minimum(planned["min_clearance"], wc))
    ranked = search.rank(wp, 1, weights=wts, counts=tp["counts"], time_step=DT, meta=prof["meta"], flags=prof["flags"],
                         clearance=clr["min_clearance"], conflict_clearance=term, tracking_worst=rcf["worst"], ctx=gen.ctx)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(out["cost"]), bits(ranked["cost"].view(1, N)))
    np.testing.assert_array_equal(bits(out["order"]), bits(ranked["order"]))
    np.testing.assert_array_equal(bits(out["n_conflicting"]), bits(rcf["n_conflicting"].view(1, N)))
    assert (term < planned["min_clearance"]).any(), "some candidate is closer to the partner disturbed than planned"
    print(f"refine, one robust iteration: {int((rcf['n_conflicting'] > 0).sum())} of {N} candidates have a conflicting rollout, "
          f"{int((planned['min_clearance'] < wts.conflict_margin).sum())} conflict as planned")
    # the option off: the bits of a call that does not name the new arguments
    cfg = search.SearchConfig(candidates=N, elites=16, iterations=3, weights=wts)
    base = gen.refine(LINE, 0.5, foot, scene, config=cfg, others=others, follower=follower, perturbations=P, **REFINE_KW)
    named = gen.refine(LINE, 0.5, foot, scene, config=cfg, others=others, follower=follower, perturbations=P, robust_conflicts=False,
                       others_shift_rows=0, others_start_jitter=None, **REFINE_KW)
    torch.cuda.synchronize()
    assert "n_conflicting" not in named
    for k in ("best_waypoints", "history", "cost", "best_cost"):
        np.testing.assert_array_equal(bits(base[k]), bits(named[k]), err_msg=k)
