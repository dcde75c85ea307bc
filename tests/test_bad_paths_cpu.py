"""The cases of tests/bad_path_cases.py bite, and the sampler's index chain stays in range on them — no GPU.

1. The oracle on the paths: the clean batches profile without a non-finite value, and every kind of bad path (but `tiny`)
   gives a zero segment length or a non-finite value in the reference's own arithmetic.
2. The `many64` placement has paths of both table classes (parameters[-1] == G and != G) beside every bad path.
3. A NumPy replica of the fit and of the arc-length table (fit_path / lut_path of vap_tables.hip, their expressions in
   their order; equal to the oracle's table bit for bit on the clean paths) makes the tables a bad path leaves behind, and
   a replica of k_sample's index chain
       table search / walk -> slope -> t = fma(slope, s - d0, t0) -> table_index_fast -> tp -> normalize_inside -> segment
   with the device's float -> int conversion (NaN -> 0, saturating) walks every sample of every thread over them:
       1 <= idx <= 999 (sD[idx - 1] and sD[idx] are table entries), 0 <= jj < tab_n, 0 <= sg < G.
   The chain as it was before the lower clamps (fixed=False) leaves the range on the interior tile — the finding.
4. The same for k_sample_routes' entry of the concatenated table and its predecessor: a length of NaN answers entry 0 of
   spline 0, whose predecessor was read from spline -1.
"""
import math

import numpy as np
import pytest

import bad_path_cases as bc

LUT_N = 1000
SPN = 1000            # property-table entries per node
CHUNK, TILE, THREADS, SPT = 1024, 1020, 256, 4
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def dev_int(x):
    """(int)x on the device (v_cvt_i32_f64): NaN -> 0, out of range saturates."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return I32_MAX
    if x <= -2147483648.0:
        return I32_MIN
    return int(x)


def dev_div_inrange(a, b):
    """div_inrange of vap_device.h: a reciprocal estimate refined by fma — the quotient for operands in range, NaN where the
    reciprocal is 0 or inf (b = inf, 0, denormal, NaN: the refinement multiplies 0 by inf)."""
    if b != b or a != a or b == 0.0 or math.isinf(b) or abs(b) < 2.0 ** -1022:
        return math.nan
    q = a / b
    return math.nan if math.isinf(q) else q


# ---- vap_tables.hip: fit_path and lut_path ---------------------------------------------------------------------------------------
def fit(path):
    """(segments (G, 12), t_max, degenerate) of one (W, 2) fp64 path, fit_path's expressions."""
    with np.errstate(all="ignore"):
        p = np.asarray(path, dtype=np.float64)
        W = len(p)
        G = W - 1
        d = p[1:] - p[:-1]
        dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        degenerate = bool(np.any(~(dist > 0.0) | ~np.isfinite(dist)))
        cum = np.cumsum(dist)[-1]
        t_max = float(G) if cum == 0.0 else cum * G / cum
        fd = np.empty((W, 2))
        fd[0] = d[0] / dist[0]
        fd[W - 1] = d[G - 1] / dist[G - 1]
        for i in range(1, W - 1):
            fd[i] = (d[i - 1] / dist[i - 1] + d[i] / dist[i]) / 2
        sd = np.zeros((W, 2))
        for i in range(1, W - 1):
            avg = (dist[i - 1] + dist[i]) / 2
            sd[i] = (fd[i + 1] - fd[i - 1]) / (avg * 0.5)
        seg = np.empty((G, 6, 2))
        for i in range(G):
            L = dist[i]
            seg[i, 0], seg[i, 1] = p[i], p[i + 1]
            if L > 0:
                seg[i, 2], seg[i, 3] = fd[i] * L, fd[i + 1] * L
                seg[i, 4], seg[i, 5] = sd[i] * (L * L), sd[i + 1] * (L * L)
            else:
                seg[i, 2], seg[i, 3], seg[i, 4], seg[i, 5] = fd[i], fd[i + 1], sd[i], sd[i + 1]
        return seg.reshape(G, 12), t_max, degenerate


def lut(seg, t_max):
    """The 1000 cumulative distances of lut_path (SM:443-454) and whether the path's length is usable."""
    with np.errstate(all="ignore"):
        G = len(seg)
        step = t_max / (LUT_N - 1)
        mag = np.empty(LUT_N)
        for j in range(LUT_N):
            t = t_max if j == LUT_N - 1 else j * step
            tt = t if t < t_max else t_max          # normalize_parameter, the device's selects
            tt = 0.0 if 0.0 > tt else tt
            i = dev_int(tt)
            if i == G:
                i = G - 1
            assert 0 <= i < G, (j, i)               # the table kernel's own segment index
            lt = tt - i
            t2 = lt * lt
            t3 = t2 * lt
            t4 = t3 * lt
            H = (-30 * t2 + 60 * t3 - 30 * t4, 30 * t2 - 60 * t3 + 30 * t4, 1 - 18 * t2 + 32 * t3 - 15 * t4,
                 -12 * t2 + 28 * t3 - 15 * t4, lt - 4.5 * t2 + 6 * t3 - 2.5 * t4, 1.5 * t2 - 4 * t3 + 2.5 * t4)
            ax = ay = 0.0
            for k in range(6):
                ax += H[k] * seg[i, 2 * k]
                ay += H[k] * seg[i, 2 * k + 1]
            mag[j] = math.sqrt(ax * ax + ay * ay) if ax * ax + ay * ay >= 0 else math.nan
        dt = 1.0 * step - 0.0 * step
        inc = np.zeros(LUT_N)
        inc[1:] = (mag[:-1] + mag[1:]) * 0.5 * dt
        D = np.cumsum(inc)
        total = float(D[-1])
        return D, total, total > 0.0 and math.isfinite(total)


# ---- vap_sample.hip: the index chain of k_sample -----------------------------------------------------------------------------------
def search_left_fixed(D, s):
    lo = 0
    step = 512
    while step > 0:
        j = lo + step
        r = j - 1 if step >= 32 else (j if j < LUT_N else LUT_N) - 1
        if D[r] < s:
            lo = j
        step >>= 1
    return lo if lo < LUT_N else LUT_N


def table_index(t, tab_n, end_param):
    """table_search + table_index of vap_device.h (the reference's own rounding)."""
    def lin(j):
        return end_param if j == tab_n - 1 else j * (end_param / (tab_n - 1))
    step = end_param / (tab_n - 1)
    x = math.ceil(t / step) if math.isfinite(t / step) else t / step
    j = 0 if x != x else int(max(min(x, 2.0 ** 62), -2.0 ** 62))
    j = min(max(j, 0), tab_n - 1)
    while j > 0 and lin(j - 1) >= t:
        j -= 1
    while j < tab_n - 1 and lin(j) < t:
        j += 1
    if j == 0:
        return 0
    frac = t - math.floor(t) if math.isfinite(t) else math.nan
    return j - 1 if frac > 0.5 else j


def chain(path, grid, fixed=True, garbage=0.0):
    """Every sample of every thread of k_sample on the tables the path leaves behind.  `fixed`: with the lower clamps of
    table_index_fast / normalize_inside and the interior tile denied to a path without a usable length; False: the chain as
    it was.  `garbage`: what sD[-1] reads (the unfixed interior body only).  Returns the extremes met."""
    seg, t_max, _ = fit(path)
    D, total, usable = lut(seg, t_max)
    W = len(path)
    G = W - 1
    tab_n = W * SPN
    end_param = float(G)
    lstep = t_max / (LUT_N - 1)
    tstep = G / (tab_n - 1)
    inv_tstep = 1.0 / tstep
    with np.errstate(all="ignore"):
        if grid[0] == "S":
            S = grid[1]
            dd = np.float64(total) / (S - 1.5)
            N = S
        else:
            dd, S = np.float64(grid[1]), grid[2]
            N = 2
        if usable and dd > 0.0:
            sgrid = np.concatenate([[0.0], np.cumsum(np.full(S + 1, dd))])      # s_k = fl(s_(k-1) + dd), MPG:112-122
            if grid[0] == "dd":
                N = min(int(np.count_nonzero(sgrid[:S + 1] < total)) + 1, S)
        else:
            sgrid = np.zeros(S + 2)                                              # one run that never moves
    dd = float(dd)
    tile = CHUNK if S <= CHUNK else TILE
    aligned = S % 4 == 0 and S % 2 == 0
    ext = dict(idx=[LUT_N, 0], jj=[I32_MAX, I32_MIN], sg=[I32_MAX, I32_MIN], interior_tiles=0, samples=0)

    def see(key, v):
        ext[key][0] = min(ext[key][0], v)
        ext[key][1] = max(ext[key][1], v)

    def sD(i):
        return garbage if i < 0 else float(D[i])

    def slope(idx):
        if idx == 0:
            return 0.0
        t0 = (idx - 1) * lstep
        t1 = t_max if idx == LUT_N - 1 else idx * lstep
        return dev_div_inrange(t1 - t0, sD(idx) - sD(idx - 1))

    for k0 in range(0, S, tile):
        if k0 >= N:
            continue
        interior = k0 > 0 and k0 + THREADS * SPT < N - 1 and aligned and k0 + THREADS * SPT <= S
        if fixed:
            interior = interior and usable
        ext["interior_tiles"] += int(interior)
        for tid in range(THREADS):
            kbase = k0 + tid * SPT
            sk = float(sgrid[min(kbase, N - 1)])
            idx = 0
            for g in range(SPT):
                k = kbase + g if interior else min(kbase + g, N - 1)
                if g > 0:
                    sk = sk + dd
                s = sk if interior else (total if k == N - 1 else sk)
                if g == 0:
                    idx = search_left_fixed(D, s)
                    if not interior:
                        idx = max(idx, 1)
                else:
                    while idx < LUT_N - 1 and sD(idx) < s:
                        idx += 1
                see("idx", idx)
                d0 = sD(idx - 1)
                t0 = (idx - 1) * lstep
                w = slope(idx)
                prod = w * (s - d0)
                t = prod + t0                       # (fma: one rounding less; the ranges asserted do not turn on it)
                exact = False if interior else (s <= 0.0 or s >= total)
                if not interior and s >= total:
                    t = end_param
                # table_index_fast
                x = t * inv_tstep
                cx = math.ceil(x) if math.isfinite(x) else x
                j = dev_int(cx)
                j = min(j, tab_n - 1)
                if fixed:
                    j = max(j, 0)
                dxi = cx - x if math.isfinite(x) else math.nan
                frac = t - math.floor(t) if math.isfinite(t) else math.nan
                fh = abs(frac - 0.5)
                near = dxi < 1e-8 or dxi > 1.0 - 1e-8 or fh < 1e-11 or fh > 0.5 - 1e-11
                jj = j - 1 if (j > 0 and frac > 0.5) else j
                if near and not exact:
                    t1 = t_max if idx == LUT_N - 1 else idx * lstep
                    with np.errstate(all="ignore"):
                        t = float(t0 + (t1 - t0) * np.float64(s - d0) / np.float64(sD(idx) - d0))
                    jj = table_index(t, tab_n, end_param)
                see("jj", jj)
                tp = end_param if jj == tab_n - 1 else jj * tstep
                for par in (tp, t):                 # normalize_inside, twice per sample
                    i = dev_int(par)
                    i = min(i, G - 1)
                    if fixed:
                        i = max(i, 0)
                    see("sg", i)
                ext["samples"] += 1
    ext["usable"], ext["N"], ext["S"] = usable, N, S
    return ext


# ---- 1. the oracle on the paths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.SMALL + ("time19",))
def test_clean_batches_profile_without_a_non_finite_value(name):
    from oracle import oracle
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    wp = bc.clean_batch(name)
    for grid in bc.placement(name)["grids"]:
        if name == "routes":
            # as routes: the reverse node and the turn node of the GPU placement cut every one into three splines
            W = wp.shape[1]
            rev, turn = np.zeros(W), np.zeros(W)
            rev[bc.ROUTE_REVERSE_NODE], turn[bc.ROUTE_TURN_NODE] = 1.0, bc.ROUTE_TURN_DEG
            nodes = dict(is_reverse=rev, turn=turn, stop=np.zeros(W), wait_time=np.zeros(W), max_velocity=np.zeros(W),
                         max_acceleration=np.zeros(W), tangent=np.full((W, 2), np.nan), magnitudes=np.zeros((W, 2)))
            for b in range(len(wp)):
                op = oracle.OraclePath(wp[b], nodes=nodes)
                assert op.n_splines == 3
                op.rebuild_tables()
                fb = op.forward_backward(DEFAULT_CONSTRAINTS, dd=op.dd_for_samples(grid[1]))
                assert len(fb["velocity"]) == grid[1] and math.isfinite(op.total_arc_length()) and op.total_arc_length() > 0
                assert all(np.all(np.isfinite(v)) for v in fb.values()) and np.all(fb["velocity"] > 0)
        elif grid[0] == "S":
            ref = oracle.profile_batch(wp, grid[1], DEFAULT_CONSTRAINTS)
            for k in ("x", "y", "heading", "curvature", "velocity", "total_length"):
                assert np.all(np.isfinite(ref[k])), (name, k)
            assert np.all(ref["velocity"] > 0)
        else:
            for b in range(len(wp)):
                op = oracle.OraclePath(wp[b])
                op.rebuild_tables()                      # (forward_backward reads the tables)
                fb = op.forward_backward(DEFAULT_CONSTRAINTS, grid[1])
                assert 2 < len(fb["velocity"]) <= grid[2]
                assert all(np.all(np.isfinite(v)) for v in fb.values())


@pytest.mark.parametrize("f32_input", [False, True])
@pytest.mark.parametrize("kind", bc.KINDS)
def test_each_kind_is_what_it_claims_in_the_reference_arithmetic(kind, f32_input):
    """Segment lengths and parameters[-1] (QHS:160, 719-736) and, where parameters[-1] is a number, the arc-length table
    (SM:443-454) of the oracle: a zero segment, a non-finite length or a non-finite table for every kind but tiny — and the
    replica of the device's fit says `degenerate` for every kind, tiny included (its squared distances underflow)."""
    from oracle import oracle
    good = bc.clean_batch("solo")[0]
    bad = bc.plant(good, kind, f32_input)
    assert not np.array_equal(bad, good, equal_nan=True) and np.array_equal(good, bc.clean_batch("solo")[0])
    _, t_max_dev, degenerate = fit(bad)
    assert degenerate, kind
    o = oracle.OraclePath(bad)
    _, seglen, plast = o.segments()
    if kind in ("nan", "pinf", "ninf", "huge"):
        # a non-finite segment length and parameters[-1] = NaN in the oracle's own fit (huge with fp64 input: finite
        # coordinates, an infinite length); the reference builds no table from there — its normalisation raises on NaN —
        # and the oracle's table routine is not called
        assert np.any(~np.isfinite(seglen)) and not np.any(np.isfinite(plast)), (kind, seglen, plast)
        assert np.any(np.isnan(seglen)) if kind == "nan" else np.any(np.isinf(seglen)), (kind, seglen)
        assert np.all(np.isfinite(bad)) == (kind == "huge" and not f32_input)
        assert not math.isfinite(t_max_dev)       # the replica of the device's fit agrees
        return
    assert np.all(np.isfinite(bad)) and np.all(np.isfinite(plast)) and t_max_dev == plast[0], (kind, plast)
    o.rebuild_tables()
    d, _, total = o.lut()
    assert np.any(seglen == 0.0), kind
    if kind != "tiny":
        assert not np.all(np.isfinite(d)) and not math.isfinite(total), kind
    print(kind, "zero segments", int(np.sum(seglen == 0.0)), "non-finite table entries", int(np.sum(~np.isfinite(d))), "total", total)


def test_good_paths_are_not_flagged_by_the_replica_and_its_table_is_the_oracles():
    from oracle import oracle
    for name in ("solo", "wide"):
        wp = bc.clean_batch(name)
        for b in range(len(wp)):
            seg, t_max, degenerate = fit(wp[b])
            D, total, usable = lut(seg, t_max)
            o = oracle.OraclePath(wp[b])
            oseg, _, plast = o.segments()
            o.rebuild_tables()
            d, _, ototal = o.lut()
            assert not degenerate and usable
            assert t_max == plast[0] and np.array_equal(seg, oseg.reshape(-1, 12))
            assert np.array_equal(D, d) and total == ototal, (name, b)


# ---- 2. the many64 class condition ---------------------------------------------------------------------------------------------------
def test_many64_has_both_table_classes_beside_every_bad_path():
    """k_lut_many<64> lets the paths with parameters[-1] == G share one basis evaluation (s_std): every workgroup of 64 paths
    that holds a bad path must hold good paths of both classes — and the bad paths themselves are of neither (NaN) or of the
    shared class (the zero-length kinds), depending on their kind."""
    p = bc.placement("many64")
    wp = bc.clean_batch("many64")
    G = p["W"] - 1
    std = bc.t_max_of(wp) == float(G)
    for b in p["bad"]:
        b0 = b // 64 * 64
        good = [q for q in range(b0, min(b0 + 64, p["B"])) if q not in p["bad"]]
        assert std[good].any() and (~std[good]).any(), (b, int(std[good].sum()), len(good))
    classes = set()
    for kind in bc.KINDS:
        tm = bc.t_max_of(bc.plant(wp[0], kind)[None])[0]
        classes.add("nan" if tm != tm else ("std" if tm == G else "off"))
    assert {"nan", "std"} <= classes


# ---- 3. the index chain --------------------------------------------------------------------------------------------------------------
CHAIN_KINDS = tuple((k, False) for k in bc.KINDS) + (("tiny", True), ("huge", True))


def _shapes():
    seen = {}
    for name in tuple(bc.PLACEMENTS) + ("time19",):
        p = bc.placement(name)
        for grid in p["grids"]:
            seen.setdefault((p["W"], grid), name)
    return [(name, grid) for (_, grid), name in seen.items()]


SHAPES = _shapes()


def test_every_placement_is_covered_by_a_chain_shape():
    covered = {(bc.placement(n)["W"], g) for n, g in SHAPES}
    for name in tuple(bc.PLACEMENTS) + ("time19",):
        p = bc.placement(name)
        assert all((p["W"], g) in covered for g in p["grids"]), name


@pytest.mark.parametrize("name,grid", SHAPES, ids=[f"{n}-{'x'.join(str(v) for v in g)}" for n, g in SHAPES])
def test_index_chain_stays_in_range_on_every_kind(name, grid):
    """Every sample of every thread, every tile (the interior body included), every kind, no kind excused — and the good
    path the kinds are planted into, which takes the interior tile where the shape has one."""
    p = bc.placement(name)
    W = p["W"]
    G, tab_n = W - 1, W * SPN
    good = bc.clean_batch(name)[p["bad"][0]]
    e = chain(good, grid)
    assert e["usable"] and 1 <= e["idx"][0] and e["idx"][1] <= LUT_N - 1
    assert 0 <= e["jj"][0] and e["jj"][1] == tab_n - 1 and 0 <= e["sg"][0] and e["sg"][1] == G - 1
    if name == "interior":
        assert e["interior_tiles"] == 1
    for kind, f32_input in CHAIN_KINDS:
        e = chain(bc.plant(good, kind, f32_input), grid)
        what = (name, grid, kind, f32_input, e)
        assert not e["usable"], what
        assert e["interior_tiles"] == 0, what                 # a path without a usable length never takes the interior body
        assert 1 <= e["idx"][0] and e["idx"][1] <= LUT_N - 1, what
        assert 0 <= e["jj"][0] and e["jj"][1] < tab_n, what
        assert 0 <= e["sg"][0] and e["sg"][1] < G, what
        assert 0 <= e["N"] <= e["S"] and e["samples"] > 0, what


@pytest.mark.parametrize("garbage", [0.0, 1.0, math.nan, math.inf, -math.inf])
def test_the_chain_without_the_lower_clamps_left_the_range_on_the_interior_tile(garbage):
    """The finding.  A path with a zero-length segment has a table that is NaN from some entry on, a length of NaN and still
    N = S samples on the fixed grid: it took the interior tile, whose search answers entry 0 for the distance 0 its run table
    gives — sD[-1] is read (whatever lies before the table in LDS: `garbage`), t = -lut_step, and table_index_fast, clamped
    from above only, returned a negative entry.  (The segment index stayed 0 here: -lut_step > -1 up to W = 1000.  From W =
    1001 on, (int)t <= -2 and the coefficient block is read before the path's own.)"""
    grid = bc.placement("interior")["grids"][0]
    good = bc.clean_batch("interior")[1]
    worst = 0
    for kind in ("dup_mid", "dup_first", "dup_last", "point"):
        e = chain(bc.plant(good, kind), grid, fixed=False, garbage=garbage)
        assert e["interior_tiles"] == 1 and e["idx"][0] == 0, (kind, e)
        worst = min(worst, e["jj"][0])
        assert 0 <= chain(bc.plant(good, kind), grid, fixed=True, garbage=garbage)["jj"][0]
    if math.isfinite(garbage):
        assert worst < 0, worst


# ---- 4. k_sample_routes: the entry of the concatenated table and its predecessor -----------------------------------------------------
def route_entry(D, off, s, state=None):
    """locate() / the walk of k_sample_routes (vap_routes_batch.hip) for one distance s that passed the early returns (not
    s <= 0, not s >= total): D (n_spl, 1000) partial distances, off (n_spl,) their offsets; state = (si, j) of the thread's
    previous sample or None.  Returns (si, j): the first entry with distance >= s."""
    n_spl = len(D)

    def dist_at(si, e):
        return D[si][e] + off[si]
    if state is None:
        si = 0
        while si < n_spl - 1 and dist_at(si, LUT_N - 1) < s:
            si += 1
        lo, hi = 0, LUT_N - 1
        while lo < hi:
            mid = (lo + hi) >> 1
            if dist_at(si, mid) < s:
                lo = mid + 1
            else:
                hi = mid
        return si, lo
    si, j = state
    while dist_at(si, j) < s:
        if j < LUT_N - 1:
            j += 1
        else:
            si, j = si + 1, 0
    return si, j


def route_predecessor(si, j, fixed=True):
    """(spline, entry) whose distance and parameter the interpolation reads as d0 / t0."""
    if fixed:
        return (si if (j > 0 or si == 0) else si - 1), (j - 1 if j > 0 else (0 if si == 0 else LUT_N - 1))
    return (si if j > 0 else si - 1), (j - 1 if j > 0 else LUT_N - 1)


def test_route_sampler_reads_its_own_tables_for_a_length_of_nan():
    """A route whose length is NaN has the run table that never moves: its samples are s = 0 (early return) and, for the last
    one, s = total = NaN, which passes both early returns.  Every comparison with NaN is false, so the search — and the walk
    from any earlier position — answers entry 0 of spline 0, whatever the tables hold; its predecessor was taken from spline
    -1 (the finding: a read before the route's tables and before the spline table in LDS) and is now entry 0 itself.  On good
    tables entry 0 is never the answer (s > 0 = distances[0]), so the change cannot reach a good route."""
    good = bc.clean_batch("routes")[0]
    tables = []
    for kind in ("dup_mid", "point", "nan"):
        seg, t_max, _ = fit(bc.plant(good, kind))
        tables.append(lut(seg, t_max)[0])
    D_bad = np.stack(tables)
    off_bad = np.array([0.0, float(D_bad[0][-1]), math.nan])
    for state in (None, (0, 0), (0, 1)):
        si, j = route_entry(D_bad, off_bad, math.nan, state)
        assert (si, j) == (state or (0, 0))
        ps, pj = route_predecessor(si, j)
        assert 0 <= ps < len(D_bad) and 0 <= pj < LUT_N and 0 <= si < len(D_bad) and 0 <= j < LUT_N
    assert route_predecessor(0, 0, fixed=False) == (-1, LUT_N - 1)        # as it was
    # good tables: three splines made of one good path's table, every grid distance strictly inside (0, total)
    seg, t_max, _ = fit(good)
    D1, total1, usable = lut(seg, t_max)
    assert usable
    D, off = np.stack([D1, D1, D1]), np.array([0.0, total1, total1 + total1])
    total = off[2] + total1
    state = None
    for s in np.linspace(0.0, total, 1021)[1:-1]:
        state = route_entry(D, off, float(s), state)
        si, j = state
        assert (si, j) != (0, 0) and (si, j) == route_entry(D, off, float(s))       # the walk is the search
        assert route_predecessor(si, j) == route_predecessor(si, j, fixed=False)
        ps, pj = route_predecessor(si, j)
        assert 0 <= ps <= si < 3 and 0 <= pj < LUT_N and D[ps][pj] + off[ps] < s <= D[si][j] + off[si]
