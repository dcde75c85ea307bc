"""GPU: clearance over a window of start shifts (vap_conflict_shifts, footprint.shifts / earliest_start,
BatchedTrajectoryGenerator.conflict_shifts, timeline.dwell_to_clear).

With hold = 14 the table is the existing call's pair_clearance at every shift of the window: the same packed rows through
the same arithmetic, so the comparison is for equal numbers (NaN matching NaN, +-0 equal), no tolerance, and "blocked" is
compared with that call's pair_first_row >= 0 exactly.  The other hold masks go against tests/shift_ref.py within
tests/test_gpu_footprint.py's TOL; blocked, first and safe are compared where the reference's |table - margin| exceeds
AMBIGUOUS, and at most 5 % of the (pair, shift) cases of a test may be skipped as ambiguous (asserted).  The rows are
tests/test_gpu_conflict.py's random_case construction: capacities 160 and 130 (two and a half 64-row blocks), counts 0, 1
and full, junk beyond the counts."""
import ctypes as C
import math

import numpy as np
import pytest

import shift_ref as sr
import test_gpu_footprint as tgf
import test_timeline_cpu as tc

pytestmark = pytest.mark.gpu

TOL = tgf.TOL
AMBIGUOUS = tgf.AMBIGUOUS
MAX_SKIPPED = 0.05
SQUARE = tgf.SQUARE
RECT = np.array([[-0.6, -0.625], [0.6, -0.625], [0.6, 0.625], [-0.6, 0.625]])
SMALL = np.array([[-0.3, -0.25], [0.3, -0.25], [0.3, 0.25], [-0.3, 0.25]])
OUT_KEYS = ("first", "n_safe", "route_table", "pair_table", "pair_first", "pair_safe")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def fpm():
    from vexautonomousplanner_amd import footprint
    return footprint


def random_case(seed, Ba=9, Bo=7, cap_a=160, cap_o=130):
    fp = fpm()
    rng = np.random.default_rng(seed)
    rows_a, rows_o = tgf.random_rows(rng, Ba, cap_a), tgf.random_rows(rng, Bo, cap_o)
    counts_a, counts_o = rng.integers(1, cap_a + 1, Ba), rng.integers(1, cap_o + 1, Bo)
    if Ba >= 4:
        counts_a[[1, 2, 3]] = 0, 1, cap_a
    if Bo >= 4:
        counts_o[[0, 2, 3]] = cap_o, 1, 0
    kind = seed % 3
    if kind == 0:
        foot_a, foot_o = SQUARE, RECT
    elif kind == 1:
        foot_a, foot_o = fp.rectangle(15, 18, 3), tgf.random_convex(rng, int(rng.integers(3, 9)), 0.0, 0.1, 0.7)
    else:
        foot_a = tgf.random_convex(rng, int(rng.integers(3, 9)), 0.1, 0.0, 0.8)
        foot_o = tgf.random_convex(rng, int(rng.integers(3, 9)), 0.0, 0.0, 0.6)
    for rows, counts in ((rows_a, counts_a), (rows_o, counts_o)):
        for b in range(len(rows)):
            rows[b, counts[b]:, 1:] = rng.choice([np.nan, np.inf, 1e300, -3.0], size=rows[b, counts[b]:, 1:].shape)
    return rows_a, counts_a.astype(np.int32), foot_a, rows_o, counts_o.astype(np.int32), foot_o


def side(torch, rows, counts, stride):
    c = np.full((len(counts), stride), -7, dtype=np.int32)
    c[:, 0] = counts
    return torch.tensor(rows, device="cuda:0"), torch.tensor(c, device="cuda:0")


def same_numbers(torch, a, b):
    """Equal as numbers: NaN matches NaN, +0 equals -0."""
    return ((a == b) | (torch.isnan(a) & torch.isnan(b))).all()


def same_bytes(a, b, keys):
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        view = np.int64 if x.dtype.itemsize == 8 else np.int32
        np.testing.assert_array_equal(x.view(view), y.view(view), err_msg=k)


def looped_equals(torch, fp, sh, da, ca, foot_a, do, co, foot_o, margin, shifts, pairing="all"):
    """The sweep's pair table against one existing call per shift, compared on the device; one synchronisation."""
    ok = torch.ones((), dtype=torch.bool, device="cuda:0")
    bufs = {}
    for k, s in enumerate(shifts):
        c = fp.conflicts(da, ca, foot_a, do, co, foot_o, margin=margin, shift_rows=int(s), pairing=pairing, pairs=True, out=bufs)
        col = sh["pair_table"][:, :, k]
        ok &= same_numbers(torch, col, c["pair_clearance"])
        ok &= ((col < margin) == (c["pair_first_row"] >= 0)).all()
    return bool(ok.item())


# ---- the analytic crossing --------------------------------------------------------------------------------------------
def test_analytic_crossing(torch_mod):
    torch = torch_mod
    fp = fpm()
    a, o, unit = sr.crossing()
    r = fp.shifts(a, None, unit, o, None, margin=0.0, shift_lo=-64, n_shifts=129, hold=15, table=True, pairs=True)
    torch.cuda.synchronize()
    assert r["first"].dim() == 0 and r["route_table"].shape == (129,) and r["pair_table"].shape == (1, 129)
    tab = r["route_table"].cpu().numpy()
    np.testing.assert_array_equal(tab, r["pair_table"][0].cpu().numpy())
    at = lambda s: tab[s + 64]
    assert at(0) == -1.0 and at(30) == at(-30) == -0.0625 and at(31) == at(-31) == at(32) == at(-32) == 0.0
    assert at(33) == at(-33) == 0.0625 and abs(at(40) - 0.35355339059327373) <= TOL and abs(at(-40) - 0.35355339059327373) <= TOL
    np.testing.assert_array_equal(tab < 0.0, np.abs(np.arange(-64, 65)) <= 30)
    np.testing.assert_array_equal(tab < 0.25, np.abs(np.arange(-64, 65)) <= 37)
    assert r["n_safe"].item() == 129 - 61 and r["first"].item() == 0 and r["first_shift"].item() == -64
    assert abs(r["first_time"].item() + 0.64) <= 1e-12
    assert fp.shifts(a, None, unit, o, None, margin=0.25, shift_lo=-64, n_shifts=129, hold=15)["n_safe"].item() == 129 - 75
    for who in ("a", "o"):
        for margin, max_delay, want in ((0.0, 64, 31), (0.25, 64, 38), (0.0, 20, -1), (0.25, 20, -1)):
            e = fp.earliest_start(a, None, unit, o, None, margin=margin, max_delay_rows=max_delay, who=who)
            assert e["delay_rows"].item() == want, (who, margin, max_delay)
            t = e["delay_time"].item()
            assert math.isnan(t) if want < 0 else abs(t - 0.01 * want) <= 1e-12
    # a run of three clear shifts starts at the same delay here (everything later is clear too) unless the window ends first
    assert fp.earliest_start(a, None, unit, o, None, max_delay_rows=64, who="o", min_run=3)["delay_rows"].item() == 31
    assert fp.earliest_start(a, None, unit, o, None, max_delay_rows=32, who="a", min_run=3)["delay_rows"].item() == -1


# ---- hold 14: equality with the existing call -------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_hold_14_equals_the_existing_call(torch_mod, seed):
    torch = torch_mod
    fp = fpm()
    margin, lo, n = 0.25, -135, 300
    rows_a, counts_a, foot_a, rows_o, counts_o, foot_o = random_case(seed)
    da, ca = side(torch, rows_a, counts_a, 2)
    do, co = side(torch, rows_o, counts_o, 3)
    sh = fp.shifts(da, ca, foot_a, do, co, foot_o, margin=margin, shift_lo=lo, n_shifts=n, hold=14, pairs=True)
    assert sh["pair_table"].shape == (9, 7, n)
    assert looped_equals(torch, fp, sh, da, ca, foot_a, do, co, foot_o, margin, range(lo, lo + n))
    m = min(len(rows_a), len(rows_o))
    shm = fp.shifts(da[:m], ca[:m], foot_a, do[:m], co[:m], foot_o, margin=margin, shift_lo=lo, n_shifts=n, hold=14, pairs=True,
                    pairing="matched")
    assert shm["pair_table"].shape == (m, 1, n)
    assert looped_equals(torch, fp, shm, da[:m], ca[:m], foot_a, do[:m], co[:m], foot_o, margin, range(lo, lo + n), "matched")
    idx = torch.arange(m, device="cuda:0")
    assert bool(same_numbers(torch, shm["pair_table"][:, 0], sh["pair_table"][idx, idx]))
    # both outcomes occur, and invalid pairs are NaN / -1 / 0
    pt = sh["pair_table"].cpu().numpy()
    assert (pt < margin).any() and (pt >= margin).any()
    assert np.isnan(pt[1]).all() and np.isnan(pt[:, 3]).all()
    assert (sh["pair_first"][1] == -1).all() and (sh["pair_safe"][:, 3] == 0).all() and sh["first"][1].item() == -1


# ---- the other hold masks against the reference -----------------------------------------------------------------------
_REF = {}


def reference(seed):
    """The case and its clearance matrices, computed once and shared by every hold mask."""
    if seed not in _REF:
        _REF[seed] = (random_case(seed), {})
    return _REF[seed]


class Tally:
    def __init__(self):
        self.skipped = self.total = 0
        self.worst = 0.0

    def close(self, label):
        print(f"{label}: max |kernel - reference| {self.worst:.2e} ft; ambiguous {self.skipped}/{self.total} (pair, shift) cases")
        assert self.total > 0 and self.skipped <= MAX_SKIPPED * self.total, (label, self.skipped, self.total)


def check_against_reference(got, ref, margin, tally):
    """Tables within TOL; blocked per shift, and first / safe of a window, where no entry of it is ambiguous."""
    for tab_k, first_k, safe_k in (("pair_table", "pair_first", "pair_safe"), ("route_table", "first", "n_safe")):
        g, w = got[tab_k].cpu().numpy(), ref[tab_k if tab_k != "route_table" else "route_table"]
        w = w.reshape(g.shape)
        gf = got[first_k].cpu().numpy().reshape(g.shape[:-1])
        gs = got[safe_k].cpu().numpy().reshape(g.shape[:-1])
        wf = ref["pair_first" if first_k == "pair_first" else "route_first"].reshape(gf.shape)
        ws = ref["pair_safe" if safe_k == "pair_safe" else "route_safe"].reshape(gs.shape)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=tab_k)
        d = np.abs(np.nan_to_num(g) - np.nan_to_num(w))
        tally.worst = max(tally.worst, float(d.max()))
        assert d.max() <= TOL, (tab_k, d.max())
        with np.errstate(invalid="ignore"):
            clear = ~(np.abs(w - margin) <= AMBIGUOUS)             # NaN entries are never ambiguous
            np.testing.assert_array_equal((g < margin)[clear], (w < margin)[clear], err_msg=tab_k)
        if tab_k == "pair_table":
            tally.total += clear.size
            tally.skipped += int((~clear).sum())
        whole = clear.all(axis=-1)
        np.testing.assert_array_equal(gf[whole], wf[whole], err_msg=first_k)
        np.testing.assert_array_equal(gs[whole], ws[whole], err_msg=safe_k)


@pytest.mark.parametrize("hold", [0, 1, 5, 10, 15])
def test_hold_masks_against_reference(torch_mod, hold):
    torch = torch_mod
    fp = fpm()
    tally = Tally()
    safe = []
    for seed in range(3):
        (rows_a, counts_a, foot_a, rows_o, counts_o, foot_o), matrices = reference(seed)
        da, ca = side(torch, rows_a, counts_a, 2)
        do, co = side(torch, rows_o, counts_o, 3)
        for margin, scan, min_run in ((0.25, "up", 1), (1.0, "down", 3)):
            kw = dict(margin=margin, shift_lo=-70, n_shifts=160, hold=hold, min_run=min_run)
            got = fp.shifts(da, ca, foot_a, do, co, foot_o, scan=scan, table=True, pairs=True, **kw)
            torch.cuda.synchronize()
            ref = sr.sweep(rows_a, counts_a, foot_a, rows_o, counts_o, foot_o, direction=1 if scan == "up" else -1, matrices=matrices, **kw)
            check_against_reference(got, ref, margin, tally)
            valid = ref["pair_safe"][~np.isnan(ref["pair_table"]).all(axis=2)]
            safe.append(valid.sum() / (160.0 * max(len(valid), 1)))
    print(f"hold {hold}: safe fraction of the valid pairs' shifts {min(safe):.2f} .. {max(safe):.2f}")
    tally.close(f"hold {hold}")


# ---- shapes -----------------------------------------------------------------------------------------------------------
def reduce_pairs(torch, res, counts_a, margin, min_run, direction):
    """The per-route outputs from the call's own pair table: torch reductions, then the scan rule on the host."""
    pt = res["pair_table"]
    inf = torch.full_like(pt, float("inf"))
    mn = torch.where(torch.isnan(pt), inf, pt).min(dim=1).values
    route_table = torch.where(torch.isinf(mn) & (mn > 0), torch.full_like(mn, float("nan")), mn)
    blocked = (pt < margin).any(dim=1).cpu().numpy()
    first, safe = [], []
    for ia in range(pt.shape[0]):
        f, s = sr.scan(blocked[ia], min_run, direction) if counts_a[ia] > 0 else (-1, 0)
        first.append(f)
        safe.append(s)
    return route_table, np.array(first), np.array(safe)


@pytest.mark.parametrize("Ba", [1, 17, 33])
def test_shapes(torch_mod, Ba):
    torch = torch_mod
    fp = fpm()
    Bo, cap_a, cap_o, margin = 5, 150, 97, 0.25
    rng = np.random.default_rng(2000 + Ba)
    rows_a, rows_o = tgf.random_rows(rng, Ba, cap_a), tgf.random_rows(rng, Bo, cap_o)
    counts_a, counts_o = rng.integers(1, cap_a + 1, Ba).astype(np.int32), rng.integers(1, cap_o + 1, Bo).astype(np.int32)
    counts_a[0] = cap_a
    if Ba > 4:
        counts_a[4] = 0
    da, ca = side(torch, rows_a, counts_a, 2)
    do, co = side(torch, rows_o, counts_o, 3)
    for step in (1, 3, 70):
        for n in (1, 63, 64, 65, 257):
            lo = -(n // 2) * step
            kw = dict(margin=margin, shift_lo=lo, n_shifts=n, shift_step=step, min_run=2, table=True, pairs=True)
            on = fp.shifts(da, ca, SMALL, do, co, SMALL * 1.5, **kw)
            on = {k: v.clone() for k, v in on.items()}
            again = fp.shifts(da, ca, SMALL, do, co, SMALL * 1.5, **kw)
            off = fp.shifts(da, ca, SMALL, do, co, SMALL * 1.5, cull=False, **kw)
            torch.cuda.synchronize()
            assert on["pair_table"].shape == (Ba, Bo, n) and on["route_table"].shape == (Ba, n)
            same_bytes(on, again, OUT_KEYS)
            for k in OUT_KEYS:
                assert bool(same_numbers(torch, on[k].double(), off[k].double())), (step, n, k)
            if step == 1 or n <= 65:
                assert looped_equals(torch, fp, on, da, ca, SMALL, do, co, SMALL * 1.5, margin, [lo + k * step for k in range(n)]), (step, n)
            route_table, first, safe = reduce_pairs(torch, on, counts_a, margin, 2, +1)
            assert bool(same_numbers(torch, on["route_table"], route_table)), (step, n)
            np.testing.assert_array_equal(on["first"].cpu().numpy(), first, err_msg=f"step {step} n {n}")
            np.testing.assert_array_equal(on["n_safe"].cpu().numpy(), safe, err_msg=f"step {step} n {n}")
            s = lo + on["first"].cpu().numpy().astype(np.int64) * step
            np.testing.assert_array_equal(on["first_shift"].cpu().numpy(), np.where(first >= 0, s, 0))


def test_base_out_host_input_and_wrapper(torch_mod):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    torch = torch_mod
    fp = fpm()
    rows_a, counts_a, foot_a, rows_o, counts_o, foot_o = random_case(31)
    da, ca = side(torch, rows_a, counts_a, 2)
    do, co = side(torch, rows_o, counts_o, 3)
    kw = dict(margin=0.25, shift_lo=-20, n_shifts=70, shift_step=2, scan="down", min_run=2, table=True, pairs=True)
    # a per-route base of mixed signs equals separate calls with shift_lo moved
    base = np.array([0, 5, -3, 40, -77, 1, 2, -1, 130], dtype=np.int32)
    based = fp.shifts(da, ca, foot_a, do, co, foot_o, base=base, **kw)
    based_dev = fp.shifts(da, ca, foot_a, do, co, foot_o, base=torch.tensor(base, device="cuda:0"), **kw)
    same_bytes(based, based_dev, OUT_KEYS)
    for ia in range(len(base)):
        moved = fp.shifts(da, ca, foot_a, do, co, foot_o, **dict(kw, shift_lo=-20 + int(base[ia])))
        for k in OUT_KEYS:
            assert bool(same_numbers(torch, based[k][ia].double(), moved[k][ia].double())), (ia, k)
        assert based["first_shift"][ia].item() == moved["first_shift"][ia].item()
    # out= reuses the buffers; host arrays are accepted; the generator's wrapper runs on its own context
    dev = fp.shifts(da, ca, foot_a, do, co, foot_o, **kw)
    host = fp.shifts(rows_a, counts_a, foot_a, rows_o, counts_o, foot_o, **kw)
    bufs = {}
    first = fp.shifts(da, ca, foot_a, do, co, foot_o, out=bufs, **kw)
    ptrs = {k: bufs[k].data_ptr() for k in OUT_KEYS}
    second = fp.shifts(da, ca, foot_a, do, co, foot_o, out=bufs, **kw)
    gen = BatchedTrajectoryGenerator(0, "f64")
    wrapped = gen.conflict_shifts({"rows": da, "counts": ca}, foot_a, {"rows": do, "counts": co}, foot_o, **kw)
    torch.cuda.synchronize()
    assert first is bufs and second is bufs and {k: bufs[k].data_ptr() for k in ptrs} == ptrs
    for other in (host, second, wrapped):
        same_bytes(dev, other, OUT_KEYS)
    lean = fp.shifts(da, ca, foot_a, do, co, foot_o, **dict(kw, table=False, pairs=False))
    assert "pair_table" not in lean and "route_table" not in lean
    same_bytes(dev, lean, ("first", "n_safe"))
    e = gen.earliest_start({"rows": da, "counts": ca}, foot_a, {"rows": do, "counts": co}, foot_o, margin=0.25, max_delay_rows=40, who="o")
    s = fp.shifts(da, ca, foot_a, do, co, foot_o, margin=0.25, shift_lo=0, n_shifts=41, hold=15)
    assert torch.equal(e["delay_rows"], s["first"])
    # nothing on side O: a route with rows is blocked nowhere
    none = fp.shifts(da, ca, foot_a, np.zeros((0, 4, 8)), np.zeros((0,), dtype=np.int32), n_shifts=5, scan="down", table=True)
    assert none["first"].tolist() == [4 if n > 0 else -1 for n in counts_a] and none["n_safe"].tolist() == [5 if n > 0 else 0 for n in counts_a]
    assert torch.isnan(none["route_table"]).all()
    with pytest.raises(ValueError):
        fp.shifts(da, ca, foot_a, do, co, foot_o, pairing="matched")


# ---- the C-ABI's input checks -----------------------------------------------------------------------------------------
def test_abi_rejects_bad_input(torch_mod):
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    L = _lib.lib()
    ctx = _lib.Context(0)
    rows = torch.zeros((2, 4, 8), dtype=torch.float64, device="cuda:0")
    rows[:, :, 6] = torch.tensor([[0.0], [3.0]], device="cuda:0")
    counts = torch.full((2, 2), 4, dtype=torch.int32, device="cuda:0")
    table = torch.full((2, 2, 3), 7.0, dtype=torch.float64, device="cuda:0")
    first = torch.full((2,), 7, dtype=torch.int32, device="cuda:0")
    flat = lambda v: (C.c_double * (2 * len(v)))(*[float(x) for p in v for x in p])
    sq = [[-0.75, -0.75], [0.75, -0.75], [0.75, 0.75], [-0.75, 0.75]]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(pairing=0, hold=14, n_shifts=3, step=1, min_run=1, scan=1, Ba=2, cap_a=4, rows_a=rows, counts_a=counts, foot_a=sq, Bo=2,
             cap_o=4, rows_o=rows, counts_o=counts, foot_o=sq, stride=2, handle=ctx.handle):
        return L.vap_conflict_shifts(handle, pairing, hold, 0.0, -1, step, n_shifts, None, min_run, scan,
                                     Ba, cap_a, p(rows_a), p(counts_a), stride, len(foot_a), flat(foot_a),
                                     Bo, cap_o, p(rows_o), p(counts_o), 2, len(foot_o), flat(foot_o),
                                     p(table), None, None, None, p(first), None)

    INV, UNS = _lib.VAP_ERR_INVALID, _lib.VAP_ERR_UNSUPPORTED
    assert call() == _lib.VAP_OK
    torch.cuda.synchronize()
    # two 1.5 ft squares 3 ft apart, parked: 1.5 ft between them, -1.5 against themselves, at every shift
    np.testing.assert_allclose(table.cpu().numpy(), np.broadcast_to(np.array([[-1.5, 1.5], [1.5, -1.5]])[:, :, None], (2, 2, 3)), rtol=0, atol=1e-14)
    assert first.tolist() == [-1, -1]
    assert call(pairing=1) == _lib.VAP_OK and call(hold=0) == _lib.VAP_OK and call(hold=15) == _lib.VAP_OK and call(scan=-1) == _lib.VAP_OK
    assert call(n_shifts=0) == INV and call(step=0) == INV and call(min_run=0) == INV
    assert call(scan=0) == INV and call(scan=2) == INV and call(hold=-1) == INV and call(hold=16) == INV
    assert call(pairing=1, Bo=1) == INV and b"matched" in L.vap_last_error()
    assert call(pairing=2) == INV
    assert call(rows_a=None) == INV and call(rows_o=None) == INV and call(counts_a=None) == INV and call(counts_o=None) == INV
    assert call(cap_a=-1) == INV and call(cap_o=-1) == INV and call(Ba=-1) == INV and call(stride=0) == INV
    assert call(cap_a=2 ** 31) == UNS and call(cap_o=2 ** 31) == UNS
    assert _lib.CONFLICT_SHIFTS_MAX >= 4096 and call(n_shifts=_lib.CONFLICT_SHIFTS_MAX + 1) == UNS
    dent = [[0, 0], [2, 0], [1, 0.5], [2, 2], [0, 2]]
    for bad in (sq[::-1], dent, sq[:2]):
        assert call(foot_a=bad) == INV and call(foot_o=bad) == INV
    # arguments are checked before the context is touched: a null context with bad arguments is still "invalid"
    assert call(n_shifts=0, handle=None) == INV
    # an empty side is a no-op: nothing is written
    torch.cuda.synchronize()
    table.fill_(7.0)
    assert call(Ba=0) == _lib.VAP_OK and call(Bo=0) == _lib.VAP_OK and call(Bo=0, rows_o=None, counts_o=None) == _lib.VAP_OK
    assert call(Ba=0, foot_a=sq[::-1]) == INV
    torch.cuda.synchronize()
    assert bool((table == 7.0).all())
    # the largest window, far steps and shifts far past both ends: every entry is the parked pair's
    big = torch.full((2, 2, _lib.CONFLICT_SHIFTS_MAX), 7.0, dtype=torch.float64, device="cuda:0")
    assert L.vap_conflict_shifts(ctx.handle, 0, 15, 0.0, -2 ** 31, 2 ** 20, _lib.CONFLICT_SHIFTS_MAX, None, 1, 1,
                                 2, 4, p(rows), p(counts), 2, 4, flat(sq), 2, 4, p(rows), p(counts), 2, 4, flat(sq),
                                 p(big), None, None, None, None, None) == _lib.VAP_OK
    torch.cuda.synchronize()
    assert float((big[0, 1] - 1.5).abs().max()) <= 1e-14 and float((big[1, 1] + 1.5).abs().max()) <= 1e-14
    ctx.close()


# ---- end to end: the dwell that lets the rest of a routine clear the partner ------------------------------------------------
def test_dwell_to_clear_end_to_end(torch_mod):
    torch = torch_mod
    from vexautonomousplanner_amd import timeline
    fp = fpm()
    DT = 0.02
    # tests/test_gpu_timeline.py's partner scene: leg 0 arrives along +x at the origin, leg 1 leaves along -y; the partner
    # crosses leg 1's path at y = -2 along +x and meets only the timeline
    a = tc.straight_leg(60, (-2.0, 0.0), 0.0, 2.0, DT)
    b = tc.straight_leg(150, (0.0, 0.0), math.pi / 2, 5.0, DT)
    rows, counts = tc.pack([a, b])
    partner = tc.straight_leg(306, (-8.0, -2.0), 0.0, 16.0, DT)[None]
    margin = 0.085
    legs = np.array([[0, 1]], dtype=np.int32)
    d = timeline.chain(rows, counts, legs, dt=DT)
    assert not bool(fp.conflicts(d["rows"], d["counts"], SQUARE, partner, [306], margin=margin)["compatible"][0])
    dwell = timeline.dwell_to_clear(d, 1, SQUARE, partner, [306], margin=margin)
    torch.cuda.synchronize()
    assert dwell.shape == (1,) and math.isfinite(dwell.item())
    n = int(round(dwell.item() / DT - 0.5))
    assert 1 <= n <= 256 and abs(dwell.item() - (n + 0.5) * DT) <= 1e-9
    cap = int(d["rows"].shape[1]) + 256
    waited = timeline.chain(rows, counts, legs, dwell=np.array([[dwell.item(), 0.0]]), dt=DT, capacity_rows=cap)
    assert int(waited["counts"][0, 0]) == int(d["counts"][0, 0]) + n
    assert bool(fp.conflicts(waited["rows"], waited["counts"], SQUARE, partner, [306], margin=margin)["compatible"][0])
    short = timeline.chain(rows, counts, legs, dwell=np.array([[dwell.item() - DT, 0.0]]), dt=DT, capacity_rows=cap)
    assert int(short["counts"][0, 0]) == int(d["counts"][0, 0]) + n - 1
    assert not bool(fp.conflicts(short["rows"], short["counts"], SQUARE, partner, [306], margin=margin)["compatible"][0])
    # a partner parked on leg 1 for good: no dwell helps; a slot the routine does not use: NaN as well
    parked = tc.straight_leg(1, (0.0, -2.0), 0.0, 0.0, DT)[None]
    assert math.isnan(timeline.dwell_to_clear(d, 1, SQUARE, parked, [1], margin=margin).item())
    one = timeline.chain(rows, counts, legs, n_legs=np.array([1], dtype=np.int32), dt=DT)
    assert math.isnan(timeline.dwell_to_clear(one, 1, SQUARE, partner, [306], margin=margin).item())
    # slot 0: the routine's start is delayed; leg 0 never comes near the partner, so only the later legs decide
    assert math.isfinite(timeline.dwell_to_clear(d, 0, SQUARE, partner, [306], margin=margin).item())


# ---- config 3's batch ---------------------------------------------------------------------------------------------------
def test_config3_batch_sample(torch_mod):
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    torch = torch_mod
    fp = fpm()
    gen = BatchedTrajectoryGenerator(0, "f32")
    wp = torch.tensor(make_waypoints(4096, 32, 3), device=gen.device)
    res = gen.profile(wp, DEFAULT_CONSTRAINTS, samples=10000)
    tp = gen.time_profile(res, DEFAULT_CONSTRAINTS, capacity_rows=2048)
    foot_a, foot_o = fp.rectangle(18, 18), fp.rectangle(15, 16, 1)
    # tools/conflict_bench.py's partner: the same rows turned by 180 degrees about the field centre; its first 8 routines
    others = {"rows": tp["rows"][:8].clone(), "counts": tp["counts"][:8]}
    others["rows"][:, :, 6:8] *= -1.0
    others["rows"][:, :, 4] -= math.pi
    pick = torch.tensor(np.random.default_rng(4).choice(4096, 64, replace=False), device=gen.device)
    sample = {"rows": tp["rows"][pick].contiguous(), "counts": tp["counts"][pick].contiguous()}
    margin, lo, n = 0.04, -32, 64
    sh = gen.conflict_shifts(sample, foot_a, others, foot_o, margin=margin, shift_lo=lo, n_shifts=n, hold=14, table=True, pairs=True)
    assert looped_equals(torch, fp, sh, sample["rows"], sample["counts"], foot_a, others["rows"], others["counts"], foot_o, margin,
                         range(lo, lo + n))
    pt = sh["pair_table"]
    assert int((pt < margin).sum()) > 0 and int((pt >= margin).sum()) > 0
    print(f"config 3 sample, 64 x 8 pairs x 64 shifts: {int((pt < margin).sum())} of {pt.numel()} blocked; "
          f"{int((sh['first'] >= 0).sum())} of 64 routes have a clear shift")
