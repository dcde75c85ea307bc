"""GPU: a routine's waits against its partners (vap_schedule_tables, vap_schedule_solve, timeline.schedule,
BatchedTrajectoryGenerator.routine_schedule).

The tables are compared with the composition of footprint.shifts they are documented as, on gathered segments, for equal
numbers (NaN matching NaN, no tolerance): the same packed rows go through the same arithmetic.  Against
tests/schedule_ref.py the tables agree within tests/test_gpu_footprint.py's TOL, and "blocked" is compared where the
reference's |entry - margin| exceeds AMBIGUOUS; at most 5 % of the entries may be skipped so (asserted; the reference's
own cases have none).  The schedule is integers: vap_schedule_solve equals schedule_ref.solve on the same tables exactly,
nothing excused."""
import ctypes as C
import math

import numpy as np
import pytest

import schedule_cases as sc
import schedule_ref as ref
import test_gpu_footprint as tgf
import test_schedule_cpu as tsc

pytestmark = pytest.mark.gpu

TOL = tgf.TOL
AMBIGUOUS = tgf.AMBIGUOUS
MAX_SKIPPED = 0.05
OUT_KEYS = ("delay_rows", "total_rows", "clearance", "n_seg", "flags", "move", "wait")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def mods():
    from vexautonomousplanner_amd import footprint, timeline
    return footprint, timeline


def side(torch, rows, counts, stride):
    c = np.full((len(counts), stride), -7, dtype=np.int32)
    c[:, 0] = counts
    return torch.tensor(np.asarray(rows, dtype=np.float64), device="cuda:0"), torch.tensor(c, device="cuda:0")


def same_numbers(torch, a, b):
    """Equal as numbers: NaN matches NaN, +0 equals -0."""
    return ((a == b) | (torch.isnan(a) & torch.isnan(b))).all()


def same_bytes(a, b, keys=OUT_KEYS):
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        view = np.int64 if x.dtype.itemsize == 8 else np.int32
        np.testing.assert_array_equal(x.view(view), y.view(view), err_msg=k)


def check_solution(res, r, want, label=""):
    d, total, c = want
    assert res["delay_rows"][r].tolist() == d, (label, r, res["delay_rows"][r].tolist(), d)
    assert int(res["total_rows"][r]) == total, (label, r)
    got = float(res["clearance"][r])
    assert got == c or (got != got and c != c), (label, r, got, c)


def solve_on_host(res, margin, q):
    """schedule_ref.solve on the tables the device returned: what the device's schedule must equal exactly."""
    mv, wt, ns = res["move"].cpu().numpy(), res["wait"].cpu().numpy(), res["n_seg"].cpu().numpy()
    return [ref.solve(mv[r], wt[r], int(ns[r]), margin, q) for r in range(len(ns))]


class Tally:
    def __init__(self):
        self.skipped = self.total = 0
        self.worst = 0.0

    def add(self, got, want, margin):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        d = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
        self.worst = max(self.worst, float(d.max()))
        assert d.max() <= TOL, d.max()
        with np.errstate(invalid="ignore"):
            clear = ~(np.abs(want - margin) <= AMBIGUOUS)              # NaN entries are never ambiguous
            np.testing.assert_array_equal((got < margin)[clear], (want < margin)[clear])
        self.total += clear.size
        self.skipped += int((~clear).sum())
        return bool(clear.all())

    def close(self, label):
        print(f"{label}: max |kernel - reference| {self.worst:.2e} ft; ambiguous {self.skipped}/{self.total} entries")
        assert self.total > 0 and self.skipped <= MAX_SKIPPED * self.total, (label, self.skipped, self.total)


def composition(torch, fp, da, ca, seg, foot_a, do, co, foot_o, n_delays, q):
    """move and wait from footprint.shifts on gathered segments, all on the device.  ``seg``: the host slot map."""
    R, M = seg.shape
    nan = float("nan")
    move = torch.full((R, M, n_delays), nan, dtype=torch.float64, device="cuda:0")
    wait = torch.full((R, M, n_delays), nan, dtype=torch.float64, device="cuda:0")
    counts = ca[:, 0].cpu().numpy()
    for r in range(R):
        n = int(np.clip(counts[r], 0, da.shape[1]))
        S, b, bad = ref.segments(seg[r], n)
        for m in range(S):
            rows = da[r, b[m]:b[m + 1]].contiguous()
            t = fp.shifts(rows, None, foot_a, do, co, foot_o, shift_lo=-(b[m] + (n_delays - 1) * q), n_shifts=n_delays, shift_step=q,
                          hold=14 if m == S - 1 else 12, table=True)["route_table"]
            move[r, m] = t.flip(0)
            h = max(b[m] - 1, 0)
            t = fp.shifts(da[r, h:h + 1].contiguous(), None, foot_a, do, co, foot_o, shift_lo=-(b[m] + n_delays * q - 1),
                          n_shifts=n_delays * q, hold=12, table=True)["route_table"].flip(0).reshape(n_delays, q)
            low = torch.where(torch.isnan(t), torch.full_like(t, float("inf")), t).min(dim=1).values
            wait[r, m] = torch.where(torch.isinf(low), torch.full_like(low, nan), low)
    return move, wait


# ---- the tables: the existing call's numbers, and the reference's ---------------------------------------------------------
@pytest.mark.parametrize("seed", list(sc.FAMILY_SEEDS))
def test_family_tables_and_schedules(torch_mod, seed):
    torch = torch_mod
    fp, timeline = mods()
    (rows_a, counts_a, seg, rows_o, counts_o), per, _ = tsc.family_reference(seed)
    da, ca = side(torch, rows_a, counts_a, 2)
    do, co = side(torch, rows_o, counts_o, 3)
    res = timeline.schedule((da, ca, seg), sc.FOOT, do, co, margin=sc.FAMILY_MARGIN, n_delays=sc.FAMILY_C, delay_step=sc.FAMILY_Q,
                            tables=True)
    assert res["move"].shape == res["wait"].shape == (sc.R, sc.M, sc.FAMILY_C) and res["delay_rows"].shape == (sc.R, sc.M)
    move, wait = composition(torch, fp, da, ca, seg, sc.FOOT, do, co, sc.FOOT, sc.FAMILY_C, sc.FAMILY_Q)
    assert bool(same_numbers(torch, res["move"], move)) and bool(same_numbers(torch, res["wait"], wait))
    tally = Tally()
    host = solve_on_host(res, sc.FAMILY_MARGIN, sc.FAMILY_Q)
    mv, wt = res["move"].cpu().numpy(), res["wait"].cpu().numpy()
    assert res["flags"].tolist() == [0] * sc.R
    for r in range(sc.R):
        ref_mv, ref_wt, S, bad, want = per[r]
        assert int(res["n_seg"][r]) == S
        clear = tally.add(mv[r], ref_mv, sc.FAMILY_MARGIN) & tally.add(wt[r], ref_wt, sc.FAMILY_MARGIN)
        check_solution(res, r, host[r], "fused against solve on its own tables")
        if clear:
            assert host[r][:2] == want[:2], (r, host[r], want)
            assert abs(host[r][2] - want[2]) <= TOL or (host[r][2] != host[r][2] and want[2] != want[2])
    tally.close(f"family seed {seed}")
    # vap_schedule_solve alone, on the tables the fused call returned: the same bytes
    from vexautonomousplanner_amd import _lib
    ctx = _lib.Context(0)
    alone = raw_solve(torch, _lib.lib(), ctx, mv, wt, res["n_seg"].cpu().numpy(), sc.FAMILY_MARGIN, sc.FAMILY_Q)
    same_bytes(alone, res, ("delay_rows", "total_rows", "clearance"))
    ctx.close()
    d = res["delay_rows"]
    assert bool((res["start_delay_rows"] == d[:, 0]).all())
    add = res["dwell_add"].cpu().numpy()
    dn = d.cpu().numpy()
    want_add = np.zeros((sc.R, sc.M))
    want_add[:, :-1] = np.where(dn[:, 1:] > 0, (dn[:, 1:] + 0.5) * 0.01, 0.0)
    np.testing.assert_allclose(add, want_add, rtol=0, atol=1e-12)


# ---- vap_schedule_solve on tables no geometry would produce -----------------------------------------------------------------
def raw_solve(torch, L, ctx, move, wait, n_seg, margin, q, outputs=(True, True, True)):
    R, M, Cn = move.shape
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)    # behind the uploads and fills below, in front of the reads
    dm, dw = torch.tensor(move, device="cuda:0"), torch.tensor(wait, device="cuda:0")
    dn = torch.tensor(np.asarray(n_seg, dtype=np.int32), device="cuda:0")
    out = {"delay_rows": torch.full((R, M), 77, dtype=torch.int32, device="cuda:0"),
           "total_rows": torch.full((R,), 77, dtype=torch.int32, device="cuda:0"),
           "clearance": torch.full((R,), 77.0, dtype=torch.float64, device="cuda:0")}
    keys = ("delay_rows", "total_rows", "clearance")
    st = L.vap_schedule_solve(ctx.handle, R, M, Cn, q, float(margin), p(dm), p(dw), p(dn),
                              *[p(out[k]) if on else None for k, on in zip(keys, outputs)])
    assert st == 0, L.vap_last_error()
    return out


def test_solve_equals_the_reference_on_random_tables(torch_mod):
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    L, ctx = _lib.lib(), _lib.Context(0)
    groups = {}
    for move, wait, S in sc.random_tables(7, 2400):
        groups.setdefault(move.shape, []).append((move, wait, S))
    n = 0
    for shape, cases in sorted(groups.items()):
        move, wait = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
        ns = [c[2] for c in cases]
        for q in (1, 3):
            out = raw_solve(torch, L, ctx, move, wait, ns, 0.0, q)
            for r in range(len(cases)):
                check_solution(out, r, ref.solve(move[r], wait[r], ns[r], 0.0, q), f"{shape} q={q}")
        n += len(cases)
    assert n >= 2000
    ctx.close()


@pytest.mark.parametrize("M", [1, 4, 32])
def test_solve_window_sizes(torch_mod, M):
    """C around the 64-bit word, and the largest window: sparse blocks so that schedules reach deep into the window."""
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    L, ctx = _lib.lib(), _lib.Context(0)
    rng = np.random.default_rng(40 + M)
    seen = {"none": 0, "zero": 0, "positive": 0}
    for Cn in (1, 63, 64, 65, 130, 4096):
        R = 3 if Cn == 4096 else 8
        move = rng.choice([0.5, -0.5, np.nan], size=(R, M, Cn), p=[0.5, 0.4, 0.1])
        wait = rng.choice([0.5, -0.5, np.nan], size=(R, M, Cn), p=[0.9, 0.02, 0.08])
        # long clear waits with a move that opens late, an early blocked wait, everything blocked, nothing blocked
        move[0, :, :Cn - 1] = -0.5
        move[0, :, Cn - 1] = 0.25
        wait[0] = 0.5
        wait[1, :, min(Cn - 1, 70)] = -1.0
        move[2] = -0.5
        if R > 3:
            move[3], wait[3] = np.nan, np.nan
            wait[4] = 0.5
            move[4] = -0.5
            for m in range(M):
                move[4, m, min(Cn - 1, (m * Cn) // M):] = 0.5 + m
        ns = rng.integers(1, M + 1, R)
        ns[0] = M
        if R > 5:
            ns[5], ns[6] = 0, M + 9                           # clamped to 0 .. M
        for q in (1, 5):
            out = raw_solve(torch, L, ctx, move, wait, ns, 0.0, q)
            for r in range(R):
                want = ref.solve(move[r], wait[r], ns[r], 0.0, q)
                check_solution(out, r, want, f"C={Cn} M={M} q={q}")
                seen[sc.classify(want[1])] += 1
    assert min(seen.values()) >= 3, seen
    ctx.close()


def test_solve_optional_outputs(torch_mod):
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    L, ctx = _lib.lib(), _lib.Context(0)
    cases = sc.random_tables(11, 40, m=3)
    cases = [c for c in cases if c[0].shape[1] == 5]
    move, wait, ns = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), [c[2] for c in cases]
    full = raw_solve(torch, L, ctx, move, wait, ns, 0.0, 2)
    for i, k in enumerate(("delay_rows", "total_rows", "clearance")):
        on = [True] * 3
        on[i] = False
        part = raw_solve(torch, L, ctx, move, wait, ns, 0.0, 2, on)
        same_bytes(part, full, [x for x in ("delay_rows", "total_rows", "clearance") if x != k])
        assert bool((part[k] == 77).all())
    ctx.close()


# ---- shapes -----------------------------------------------------------------------------------------------------------------
_SHAPES = {}


def shapes_case():
    """Five routines (capacity 160): slots at rows 1, 63, 64, 65, 128 and n - 1; counts 0, -3 and capacity + 500; one-row
    segments throughout.  Four partners (capacity 130) with counts 130, 0, 1 and 97.  Junk behind the counts."""
    if not _SHAPES:
        rng = np.random.default_rng(77)
        cap_a, cap_o, M = 160, 130, 8
        counts_a = np.array([150, 0, -3, cap_a + 500, 70], dtype=np.int32)
        n_a = np.clip(counts_a, 0, cap_a)
        counts_o = np.array([130, 0, 1, 97], dtype=np.int32)
        rows_a = np.stack([sc._drive(rng, cap_a, max(int(n), 1), 0.05) for n in n_a])
        rows_o = np.stack([sc._drive(rng, cap_o, max(int(n), 1), 0.06) for n in counts_o])
        rows_o[2, :, 6:8] += 2.5                                  # the one-row partner parks beside the crossing, not on it
        seg = np.full((5, M), -1, dtype=np.int32)
        seg[0, :7] = [0, 1, 63, 64, 65, 128, 149]
        seg[1, :2] = [0, 5]
        seg[2, :2] = [0, 5]
        seg[3, :2] = [0, 159]
        seg[4] = np.arange(8)
        for rows, counts in ((rows_a, n_a), (rows_o, counts_o)):
            for b in range(len(rows)):
                rows[b, counts[b]:, 1:] = rng.choice([np.nan, np.inf, 1e300, -3.0], size=rows[b, counts[b]:, 1:].shape)
        _SHAPES["case"] = (rows_a, counts_a, seg, rows_o, counts_o)
        _SHAPES["mats"] = {}
    return _SHAPES["case"], _SHAPES["mats"]


@pytest.mark.parametrize("q,Cn", [(1, 130), (2, 40), (7, 40), (20, 70)])
def test_shapes_against_reference(torch_mod, q, Cn):
    """q = 1 with 130 delays: three bands of lanes, the last of two; q = 20: the staged partner rows of 64 delays no longer
    fit, so the bands are 32 delays wide."""
    torch = torch_mod
    fp, timeline = mods()
    (rows_a, counts_a, seg, rows_o, counts_o), mats = shapes_case()
    margin = 0.1
    da, ca = side(torch, rows_a, counts_a, 3)
    do, co = side(torch, rows_o, counts_o, 2)
    res = timeline.schedule((da, ca, seg), sc.FOOT, do, co, margin=margin, n_delays=Cn, delay_step=q, tables=True)
    host = solve_on_host(res, margin, q)
    mv, wt = res["move"].cpu().numpy(), res["wait"].cpu().numpy()
    tally = Tally()
    assert res["flags"].tolist() == [0] * 5 and res["n_seg"].tolist() == [7, 0, 0, 2, 8]
    for r in range(5):
        ref_mv, ref_wt, S, bad = ref.tables(rows_a[r], counts_a[r], seg[r], sc.FOOT, rows_o, counts_o, sc.FOOT, Cn, q, matrices=mats, key=r)
        clear = tally.add(mv[r], ref_mv, margin) & tally.add(wt[r], ref_wt, margin)
        check_solution(res, r, host[r], f"q={q}")
        if clear:
            assert host[r][:2] == ref.solve(ref_mv, ref_wt, S, margin, q)[:2]
    for r in (1, 2):
        assert res["delay_rows"][r].tolist() == [-1] * 8 and int(res["total_rows"][r]) == -1 and np.isnan(mv[r]).all()
    assert not np.isnan(mv[0, :7]).any() and np.isnan(mv[0, 7]).all() and np.isnan(wt[0, 7]).all()
    tally.close(f"shapes q={q}")
    if q == 2:
        move, wait = composition(torch, fp, da, ca, seg, sc.FOOT, do, co, sc.FOOT, Cn, q)
        assert bool(same_numbers(torch, res["move"], move)) and bool(same_numbers(torch, res["wait"], wait))


def test_no_partners_many_routines_and_one(torch_mod):
    torch = torch_mod
    fp, timeline = mods()
    (rows_a, counts_a, seg, rows_o, counts_o), _ = shapes_case()
    da, ca = side(torch, rows_a, counts_a, 1)
    do, co = side(torch, rows_o, counts_o, 1)
    kw = dict(margin=0.1, n_delays=70, delay_step=2, tables=True)
    # Bo = 0, and partners that all have no rows: NaN tables, an all-zero schedule for a routine with rows
    for o_rows, o_counts in ((do[:0], co[:0]), (do, torch.zeros_like(co))):
        res = timeline.schedule((da, ca, seg), sc.FOOT, o_rows, o_counts, **kw)
        assert bool(torch.isnan(res["move"]).all()) and bool(torch.isnan(res["wait"]).all())
        assert res["n_seg"].tolist() == [7, 0, 0, 2, 8] and res["total_rows"].tolist() == [0, -1, -1, 0, 0]
        assert res["delay_rows"].tolist() == [[0] * 8, [-1] * 8, [-1] * 8, [0] * 8, [0] * 8]
        assert bool(torch.isnan(res["clearance"]).all())
    # R = 1, and R = 300 (more workgroups than CUs): every routine's answer is its own
    base = timeline.schedule((da, ca, seg), sc.FOOT, do, co, **kw)
    one = timeline.schedule((da[3:4], ca[3:4], seg[3:4]), sc.FOOT, do, co, **kw)
    same_bytes(one, {k: base[k][3:4] for k in OUT_KEYS})
    idx = torch.arange(300, device="cuda:0") % 5
    many = timeline.schedule((da[idx], ca[idx], torch.tensor(seg, device="cuda:0")[idx]), sc.FOOT, do, co, **kw)
    same_bytes(many, {k: base[k][idx] for k in OUT_KEYS})
    # no routines at all
    none = timeline.schedule((da[:0], ca[:0], seg[:0]), sc.FOOT, do, co, **kw)
    assert none["delay_rows"].shape == (0, 8) and none["move"].shape == (0, 8, 70)


def test_bad_segment_lists_flag_their_routine_only(torch_mod):
    torch = torch_mod
    fp, timeline = mods()
    from vexautonomousplanner_amd import _lib
    (rows_a, counts_a, seg, rows_o, counts_o), _ = shapes_case()
    n = 150
    lists = [[0, 60], [1, 60], [0, 60, 60], [0, 90, 60], [0, n], [0, -1, 60], [-1, 0], [0, 60]]
    segs = np.full((len(lists), 3), -1, dtype=np.int32)
    for i, l in enumerate(lists):
        segs[i, :len(l)] = l
    da, ca = side(torch, np.repeat(rows_a[:1], len(lists), axis=0), np.full(len(lists), n), 1)
    do, co = side(torch, rows_o, counts_o, 1)
    res = timeline.schedule((da, ca, segs), sc.FOOT, do, co, margin=0.1, n_delays=33, tables=True)
    bad = [0, 1, 1, 1, 1, 1, 1, 0]
    assert res["flags"].tolist() == [_lib.FLAG_BAD_ROUTE * b for b in bad]
    assert timeline.FLAGS["bad_route"] == _lib.FLAG_BAD_ROUTE
    assert res["n_seg"].tolist() == [2 * (1 - b) for b in bad]
    good = timeline.schedule((da[:1], ca[:1], segs[:1]), sc.FOOT, do, co, margin=0.1, n_delays=33, tables=True)
    for r, b in enumerate(bad):
        if b:
            assert bool(torch.isnan(res["move"][r]).all()) and bool(torch.isnan(res["wait"][r]).all())
            assert res["delay_rows"][r].tolist() == [-1] * 3 and int(res["total_rows"][r]) == -1 and math.isnan(float(res["clearance"][r]))
        else:
            same_bytes({k: res[k][r:r + 1] for k in OUT_KEYS}, good)
    assert not bool(torch.isnan(good["move"][0, :2]).any())


def test_cull_two_calls_out_reuse_and_wrapper(torch_mod):
    torch = torch_mod
    fp, timeline = mods()
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    rows_a, counts_a, seg, rows_o, counts_o = sc.family(2)
    da, ca = side(torch, rows_a, counts_a, 2)
    do, co = side(torch, rows_o, counts_o, 3)
    kw = dict(margin=sc.FAMILY_MARGIN, n_delays=sc.FAMILY_C, delay_step=sc.FAMILY_Q, tables=True)
    on = timeline.schedule((da, ca, seg), sc.FOOT, do, co, **kw)
    off = timeline.schedule((da, ca, seg), sc.FOOT, do, co, cull=False, **kw)
    same_bytes(on, off)
    again = timeline.schedule((da, ca, seg), sc.FOOT, do, co, **kw)
    same_bytes(on, again)
    # out= is filled in place and reused; a buffer of another shape is replaced
    bufs = {"move": torch.zeros(1, device="cuda:0")}
    first = timeline.schedule((da, ca, seg), sc.FOOT, do, co, out=bufs, **kw)
    assert first is bufs
    ptrs = {k: bufs[k].data_ptr() for k in OUT_KEYS}
    second = timeline.schedule((da, ca, seg), sc.FOOT, do, co, out=bufs, **kw)
    assert second is bufs and ptrs == {k: bufs[k].data_ptr() for k in OUT_KEYS}
    same_bytes(second, on)
    # host inputs, another footprint for the partners, without the tables
    host = timeline.schedule((rows_a, counts_a, seg), sc.FOOT, rows_o, counts_o, sc.FOOT, margin=sc.FAMILY_MARGIN, n_delays=sc.FAMILY_C,
                             delay_step=sc.FAMILY_Q)
    assert "move" not in host and "wait" not in host
    same_bytes(host, on, ("delay_rows", "total_rows", "clearance", "n_seg", "flags"))
    # the generator's wrapper: its own context, the dict chain returns
    gen = BatchedTrajectoryGenerator(0, "f64")
    tl = {"rows": da, "counts": ca, "map": torch.tensor(seg, device="cuda:0")[:, :, None].expand(sc.R, sc.M, 3)}
    wrapped = gen.routine_schedule(tl, sc.FOOT, {"rows": do, "counts": co}, **kw)
    same_bytes(wrapped, on)
    # arguments are refused before any device work, in the siblings' style
    for bad in (dict(n_delays=0), dict(n_delays=4097), dict(delay_step=0), dict(margin=float("nan"))):
        with pytest.raises(ValueError):
            timeline.schedule((da, ca, seg), sc.FOOT, do, co, **{**kw, **bad})
    with pytest.raises(ValueError):
        timeline.schedule((da, ca, seg[:, :0]), sc.FOOT, do, co, **kw)
    with pytest.raises(ValueError):
        timeline.schedule((da, ca, seg[:3]), sc.FOOT, do, co, **kw)
    with pytest.raises(ValueError):
        timeline.schedule((da, ca, seg), sc.FOOT[::-1], do, co, **kw)
    with pytest.raises(ValueError):
        timeline.schedule((da[0], None, seg), sc.FOOT, do, co, **kw)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_input_and_optional_outputs(torch_mod):
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    L = _lib.lib()
    ctx = _lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)    # one stream for torch's fills and the calls
    rows = torch.zeros((2, 4, 8), dtype=torch.float64, device="cuda:0")
    rows[:, :, 6] = torch.tensor([[0.0], [3.0]], device="cuda:0")
    counts = torch.full((2, 2), 4, dtype=torch.int32, device="cuda:0")
    seg = torch.tensor([[0, 2], [0, -1]], dtype=torch.int32, device="cuda:0")
    new = lambda: {"move": torch.full((2, 2, 3), 7.0, dtype=torch.float64, device="cuda:0"),
                   "wait": torch.full((2, 2, 3), 7.0, dtype=torch.float64, device="cuda:0"),
                   "n_seg": torch.full((2,), 7, dtype=torch.int32, device="cuda:0"),
                   "flags": torch.zeros((2,), dtype=torch.int32, device="cuda:0")}
    out = new()
    flat = lambda v: (C.c_double * (2 * len(v)))(*[float(x) for p in v for x in p])
    sq = [[-0.75, -0.75], [0.75, -0.75], [0.75, 0.75], [-0.75, 0.75]]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    keys = ("move", "wait", "n_seg", "flags")

    def call(n_delays=3, step=1, R=2, cap_a=4, rows_a=rows, counts_a=counts, foot_a=sq, M=2, seg_start=seg, Bo=2, cap_o=4, rows_o=rows,
             counts_o=counts, foot_o=sq, stride=2, handle=ctx.handle, o=None, skip=None):
        o = out if o is None else o
        return L.vap_schedule_tables(handle, n_delays, step, R, cap_a, p(rows_a), p(counts_a), stride, len(foot_a), flat(foot_a),
                                     M, p(seg_start), Bo, cap_o, p(rows_o), p(counts_o), 2, len(foot_o), flat(foot_o),
                                     *[None if k == skip else p(o[k]) for k in keys])

    INV, UNS = _lib.VAP_ERR_INVALID, _lib.VAP_ERR_UNSUPPORTED
    assert call() == _lib.VAP_OK
    torch.cuda.synchronize()
    # two 1.5 ft squares 3 ft apart, parked: each routine meets itself (-1.5) before the other (1.5), at every delay
    want = np.full((2, 2, 3), -1.5)
    want[1, 1] = np.nan
    np.testing.assert_allclose(out["move"].cpu().numpy(), want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(out["wait"].cpu().numpy(), want, rtol=0, atol=1e-14)
    assert out["n_seg"].tolist() == [2, 1] and out["flags"].tolist() == [0, 0]
    # every output is optional: the others do not change
    for k in keys:
        part = new()
        assert call(o=part, skip=k) == _lib.VAP_OK
        torch.cuda.synchronize()
        same_bytes(part, out, [x for x in keys if x != k])
        assert bool((part[k] == (0 if k == "flags" else 7)).all())
    assert call(n_delays=0) == INV and call(step=0) == INV and call(M=0) == INV
    assert call(rows_a=None) == INV and call(rows_o=None) == INV and call(counts_a=None) == INV and call(counts_o=None) == INV
    assert call(seg_start=None) == INV
    assert call(cap_a=-1) == INV and call(cap_o=-1) == INV and call(R=-1) == INV and call(Bo=-1) == INV and call(stride=0) == INV
    assert call(cap_a=2 ** 31) == UNS and call(cap_o=2 ** 31) == UNS
    assert _lib.SCHEDULE_MAX_DELAYS == 4096 and call(n_delays=_lib.SCHEDULE_MAX_DELAYS + 1) == UNS
    assert call(M=_lib.TIMELINE_MAX_LEGS + 1) == UNS and call(n_delays=3, step=2 ** 29) == _lib.VAP_OK and call(n_delays=4, step=2 ** 30) == UNS
    dent = [[0, 0], [2, 0], [1, 0.5], [2, 2], [0, 2]]
    for bad in (sq[::-1], dent, sq[:2]):
        assert call(foot_a=bad) == INV and call(foot_o=bad) == INV
    # arguments are checked before the context is touched: a null context with bad arguments is still "invalid"
    assert call(n_delays=0, handle=None) == INV and call(M=33, handle=None) == UNS
    # R = 0 is a no-op: nothing is written
    torch.cuda.synchronize()
    fresh = new()
    assert call(R=0, o=fresh) == _lib.VAP_OK and call(R=0, rows_a=None, counts_a=None, seg_start=None, o=fresh) == _lib.VAP_OK
    assert call(R=0, foot_a=sq[::-1], o=fresh) == INV
    torch.cuda.synchronize()
    assert bool((fresh["move"] == 7.0).all()) and bool((fresh["n_seg"] == 7).all())
    # Bo = 0 needs no partner pointers
    assert call(Bo=0, rows_o=None, counts_o=None, o=fresh) == _lib.VAP_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(fresh["move"]).all()) and fresh["n_seg"].tolist() == [2, 1]

    def solve(R=2, M=2, n_delays=3, step=1, margin=0.0, move=out["move"], wait=out["wait"], n_seg=out["n_seg"], handle=ctx.handle):
        return L.vap_schedule_solve(handle, R, M, n_delays, step, margin, p(move), p(wait), p(n_seg), p(delays), p(total), None)

    delays = torch.full((2, 2), 7, dtype=torch.int32, device="cuda:0")
    total = torch.full((2,), 7, dtype=torch.int32, device="cuda:0")
    assert solve(margin=-2.0) == _lib.VAP_OK
    torch.cuda.synchronize()
    assert delays.tolist() == [[0, 0], [0, 0]] and total.tolist() == [0, 0]
    assert solve() == _lib.VAP_OK
    torch.cuda.synchronize()
    assert delays.tolist() == [[-1, -1], [-1, -1]] and total.tolist() == [-1, -1]
    assert solve(M=0) == INV and solve(n_delays=0) == INV and solve(step=0) == INV and solve(R=-1) == INV
    assert solve(margin=float("nan")) == INV and solve(margin=float("inf")) == INV
    assert solve(move=None) == INV and solve(wait=None) == INV and solve(n_seg=None) == INV
    assert solve(M=33) == UNS and solve(n_delays=4097) == UNS and solve(n_delays=4, step=2 ** 30) == UNS
    assert solve(step=0, handle=None) == INV
    delays.fill_(7)
    assert solve(R=0) == _lib.VAP_OK and solve(R=0, move=None, wait=None, n_seg=None) == _lib.VAP_OK
    torch.cuda.synchronize()
    assert bool((delays == 7).all())
    ctx.close()


# ---- the known case -----------------------------------------------------------------------------------------------------------
def test_known_case(torch_mod):
    torch = torch_mod
    fp, timeline = mods()
    a, seg, o, co = sc.known()
    for q in (1, 2, 4):
        for sel, want in (([0], sc.KNOWN_ONE), ([0, 1], sc.KNOWN_BOTH)):
            res = timeline.schedule((a, [161], seg), sc.UNIT, o[sel], co[sel], margin=sc.KNOWN_MARGIN, n_delays=sc.KNOWN_WINDOW // q,
                                    delay_step=q)
            assert res["delay_rows"].tolist() == [want[q]] and res["total_rows"].tolist() == [sum(want[q])], (q, sel)
            assert res["start_delay_rows"].tolist() == [want[q][0]]
            if len(sel) == 2:
                assert res["clearance"].item() == sc.KNOWN_BOTH_CLEARANCE
    # what the existing calls give instead: a start delay alone must outwait partner 2 for good, which never happens
    both = fp.earliest_start(a, [161], sc.UNIT, o, co, margin=sc.KNOWN_MARGIN, max_delay_rows=47, who="a")
    assert both["delay_rows"].tolist() == [-1]


# ---- end to end: schedule, chain again, check with the existing call ---------------------------------------------------------
def test_routine_end_to_end(torch_mod):
    torch = torch_mod
    fp, timeline = mods()
    rows, counts, partners, pc = sc.routine_scene()
    DT, margin, Cn, q, foot = sc.ROUTINE_DT, sc.ROUTINE_MARGIN, sc.ROUTINE_C, sc.ROUTINE_Q, sc.ROUTINE_FOOT
    legs = np.array([[0, 1, 2]], dtype=np.int32)
    tl = timeline.chain(rows, counts, legs, dt=DT)
    dp = torch.tensor(partners, device="cuda:0")
    assert not bool(fp.conflicts(tl["rows"], tl["counts"], foot, dp, pc, margin=margin)["compatible"][0])
    res = timeline.schedule(tl, foot, dp, pc, margin=margin, n_delays=Cn, delay_step=q, tables=True)
    d = res["delay_rows"][0].tolist()
    total = int(res["total_rows"][0])
    assert int(res["n_seg"][0]) == 3 and total == sum(d) > 0 and all(x % q == 0 for x in d)
    # it leaves the start before partner 1 parks on it and waits out partner 0's crossing at site 0: two waits
    assert d[0] > 0 and d[1] > 0 and res["clearance"].item() >= margin
    old_map, old_n = tl["map"][0].cpu().numpy(), int(tl["counts"][0, 0])
    cap = int(tl["rows"].shape[1]) + Cn * q
    again = timeline.chain(rows, counts, legs, dwell=res["dwell_add"], dt=DT, capacity_rows=cap)
    cum = np.concatenate([[0], np.cumsum(d[1:])])               # rows inserted in front of slot m, the start shift aside
    new_map = again["map"][0].cpu().numpy()
    np.testing.assert_array_equal(new_map[:, 0], old_map[:, 0] + cum)
    assert int(again["counts"][0, 0]) == old_n + cum[-1]
    # the re-chained poses are the rows the schedule gathered: every old row moved by its slot's cumulative wait, the hold
    # pose in between
    src = np.zeros(old_n + cum[-1], dtype=np.int64)
    for m in range(3):
        lo, hi = old_map[m, 0], old_map[m + 1, 0] if m < 2 else old_n
        if m > 0:
            src[lo + cum[m - 1]:lo + cum[m]] = lo - 1
        src[lo + cum[m]:hi + cum[m]] = np.arange(lo, hi)
    old_rows, new_rows = tl["rows"][0].cpu().numpy(), again["rows"][0].cpu().numpy()
    np.testing.assert_array_equal(new_rows[:len(src)][:, [4, 6, 7]], old_rows[src][:, [4, 6, 7]])
    ok = fp.conflicts(again["rows"], again["counts"], foot, dp, pc, margin=margin, shift_rows=-d[0])
    assert bool(ok["compatible"][0]) and ok["min_clearance"].item() >= margin
    # one step less in the window and the reference finds nothing
    n = old_n
    mv, wt, S, bad = ref.tables(old_rows, n, old_map[:, 0], foot, partners, pc, foot, total // q, q)
    assert S == 3 and ref.solve(mv, wt, S, margin, q)[1] == -1
    got_mv = res["move"][0, :, :total // q].cpu().numpy()
    assert np.abs(got_mv - mv).max() <= TOL
