"""A degenerate path never disturbs its batch neighbours.

Every placement of tests/bad_path_cases.py — the smallest shapes at which a kernel shares a workgroup, a wave or a quad of
lanes between paths — runs as a clean batch and as its dirty twins through the same generator, mode and kernel option:

  good paths   x, y, heading, curvature, velocity and the meta row are byte-identical between the two runs, flag 0 in both
  bad paths    VAP_FLAG_DEGENERATE (kind `tiny`: reported, not asserted), meta[3] an integer in [0, S], the call returns;
               any further bit is printed ("extra bits"), no value of their rows is asserted
  one anchor   the clean `solo` batch against the oracle, test_gpu_parity.check_fields at that file's tolerances — the one
               tolerance of this file; bit-equality to a wrong clean run would prove nothing

and the same through the staged calls, the time domain (lane / quad / fused kernels, waits), the consumers of the rows
(node limits, curve caps, conditioning, closest points) and the ranking of vap_search_update.  The clean run of a
(placement, grid, mode, kernel) is computed once and shared, read-only.
"""
import functools

import numpy as np
import pytest

import bad_path_cases as bc
from test_gpu_parity import DTYPES_TOL, check_fields, make_gen, torch_mod  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROWS = ("x", "y", "heading", "curvature", "velocity")
SENTINEL = -7.25e77


@functools.lru_cache(maxsize=None)
def gen_for(mode, kernel="auto"):
    return make_gen(mode, velocity_kernel=kernel)


def _grid_kw(grid):
    return dict(samples=grid[1]) if grid[0] == "S" else dict(dd=grid[1], capacity=grid[2])


def _capacity(grid):
    return grid[1] if grid[0] == "S" else grid[2]


def _route_nodes(B, W):
    rev = np.zeros((B, W), dtype=bool)
    turn = np.zeros((B, W))
    rev[:, bc.ROUTE_REVERSE_NODE] = True
    turn[:, bc.ROUTE_TURN_NODE] = bc.ROUTE_TURN_DEG
    return rev, turn


def profile(torch, name, wp64, grid, mode, kernel):
    """One fused call (vap_profile_batch; vap_profile_routes for the routes placement); tensors stay on the device."""
    gen = gen_for(mode, kernel)
    wp = torch.tensor(wp64, dtype=gen.tdtype, device=gen.device)
    if name == "routes":
        rev, turn = _route_nodes(*wp64.shape[:2])
        res = gen.profile_routes(wp, node_reverse=rev, node_turn=turn, **_grid_kw(grid))
        assert int(res["spline_counts"].max().item()) == 3
    else:
        res = gen.profile(wp, **_grid_kw(grid))
    torch.cuda.synchronize()
    return gen, res


@functools.lru_cache(maxsize=None)
def clean_run(name, grid, mode, kernel):
    import torch
    _, res = profile(torch, name, bc.clean_batch(name), grid, mode, kernel)
    assert not res["flags"].any().item(), (name, "the clean batch is flagged")
    return {k: res[k].clone() for k in ROWS + ("meta", "flags")}


def bits(t):
    """The tensor's bytes as integers: NaN payloads and signed zeros count."""
    import torch
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bytes(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def check_neighbours(torch, name, plan, dirty, clean, S, fields=ROWS + ("meta",), what=""):
    from vexautonomousplanner_amd import _lib
    good = torch.tensor(bc.good_mask(name, plan), device=dirty["flags"].device)
    for k in fields:
        assert same_bytes(dirty[k][good], clean[k][good]), (what, k, "a good path differs from the clean run")
    assert not dirty["flags"][good].any().item() and not clean["flags"][good].any().item(), (what, "a good path is flagged")
    flags = dirty["flags"].cpu().numpy()
    meta = dirty["meta"].cpu().numpy()
    for b, kind in plan.items():
        f = int(flags[b])
        if kind in bc.FLAG_ASSERTED:
            assert f & _lib.FLAG_DEGENERATE, (what, b, kind, f)
        else:
            print(f"{what} path {b} kind {kind}: flags {f}")
        if f & ~_lib.FLAG_DEGENERATE:
            print(f"{what} path {b} kind {kind}: extra bits {f & ~_lib.FLAG_DEGENERATE}")
        n = float(meta[b, 3])
        assert n == int(n) and 0 <= n <= S, (what, b, kind, n)


def _f32_input(mode):
    return mode != "f64"


# ---- the placements -------------------------------------------------------------------------------------------------------------------
def _runs():
    """(placement, grid, mode, kernel) in the order they run: the small placements, then many8, many64, routes, wide last."""
    out = []
    solo = bc.PLACEMENTS["solo"]["grids"][0]
    for mode in ("f32", "f64", "f32r32"):
        out.append(("solo", solo, mode, "auto"))
    for kernel in ("seq_literal", "seq_fast", "relax", "relax_block", "lanes16", "lanes32", "lanes64"):
        out.append(("solo", solo, "f32", kernel))
    out.append(("solo", solo, "f32r32", "relax_wave"))
    for name in ("interior", "ragged", "lanes16", "lanes32", "lanes64", "many8", "many64", "routes", "wide"):
        p = bc.PLACEMENTS[name]
        for grid in p["grids"]:
            out.append((name, grid, "f32", p["kernel"]))
            if name in ("lanes16", "many8"):
                out.append((name, grid, "f64", p["kernel"]))
    return out


RUNS = _runs()
RUN_IDS = ["-".join([n, "x".join(str(v) for v in g), m, k]) for n, g, m, k in RUNS]


@pytest.mark.parametrize("label", bc.CALL_LABELS)
@pytest.mark.parametrize("name,grid,mode,kernel", RUNS, ids=RUN_IDS)
def test_good_paths_are_bit_for_bit_those_of_the_clean_batch(torch_mod, name, grid, mode, kernel, label):
    wp, plan = bc.dirty_batch(name, label, _f32_input(mode))
    clean = clean_run(name, grid, mode, kernel)
    _, dirty = profile(torch_mod, name, wp, grid, mode, kernel)
    check_neighbours(torch_mod, name, plan, dirty, clean, _capacity(grid), what=f"{name} {grid} {mode} {kernel} {label}")


@pytest.mark.parametrize("mode,tol", DTYPES_TOL)
def test_clean_solo_batch_against_the_oracle(torch_mod, mode, tol):
    from oracle import oracle
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    grid = bc.PLACEMENTS["solo"]["grids"][0]
    clean = clean_run("solo", grid, mode, "auto")
    ref = oracle.profile_batch(bc.clean_batch("solo"), grid[1], DEFAULT_CONSTRAINTS)
    got = {k: clean[k].cpu().numpy().astype(np.float64) for k in ROWS}
    check_fields(got, ref, tol, f"clean solo {mode}")


# ---- the staged calls -----------------------------------------------------------------------------------------------------------------
def _staged(torch, mode, wp64, S):
    from test_gpu_geometry import staged
    out, meta, _, flags = staged(torch, mode, wp64, S=S)
    res = {k: out[k] for k in ROWS}
    res["meta"], res["flags"] = meta, flags
    return res


@functools.lru_cache(maxsize=None)
def clean_staged(mode):
    import torch
    return _staged(torch, mode, bc.clean_batch("solo"), bc.PLACEMENTS["solo"]["grids"][0][1])


@pytest.mark.parametrize("label", bc.CALL_LABELS)
@pytest.mark.parametrize("mode", ["f32", "f64", "f32r32"])
def test_staged_calls_keep_the_neighbours(torch_mod, mode, label):
    """vap_fit -> vap_build_lut -> vap_sample -> vap_velocity_pass on caller-owned buffers, and the clean staged rows are the
    fused call's."""
    S = bc.PLACEMENTS["solo"]["grids"][0][1]
    wp, plan = bc.dirty_batch("solo", label, _f32_input(mode))
    clean = clean_staged(mode)
    fused = clean_run("solo", ("S", S), mode, "auto")
    for k in ROWS + ("meta",):
        assert same_bytes(clean[k], fused[k]), k
    dirty = _staged(torch_mod, mode, wp, S)
    check_neighbours(torch_mod, "solo", plan, dirty, clean, S, what=f"staged {mode} {label}")


# ---- the time domain ------------------------------------------------------------------------------------------------------------------
TIME_CAP = 768


EVENT_CAP = TIME_CAP + 64        # room for the rows of a 0.25 s wait at dt = 0.01 s


def _insert_events(torch, gen, res, tp, waits):
    """vap_time_insert_events (what insert_waits calls) through the C-ABI into sentinel-filled buffers with a sentinel tail
    behind the last path's rows: no turns, no action points."""
    import ctypes as C
    from vexautonomousplanner_amd import _lib
    from vexautonomousplanner_amd._call import ptr
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    B, W = waits.shape
    dev = gen.device
    tail = 4096
    buf = torch.full((B * EVENT_CAP * 8 + tail,), SENTINEL, dtype=torch.float64, device=dev)
    out = {"rows": buf[:B * EVENT_CAP * 8].view(B, EVENT_CAP, 8),
           "counts": torch.full((B, 3), -1, dtype=torch.int32, device=dev),
           "nodes_map": torch.full((B, W), -1, dtype=torch.int32, device=dev),
           "actions_map": torch.full((B, 1), -1, dtype=torch.int32, device=dev)}
    d_wait = torch.tensor(waits, dtype=torch.float64, device=dev)
    d_apt = torch.full((B, 1), float("inf"), dtype=torch.float64, device=dev)
    d_apw = torch.zeros((B, 1), dtype=torch.float64, device=dev)
    c = _lib.make_constraints(DEFAULT_CONSTRAINTS)
    gen.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib().vap_time_insert_events(gen.ctx.handle, B, W, 0, TIME_CAP, EVENT_CAP, 0.01, C.byref(c), ptr(res["meta"]),
                                                 ptr(tp["rows"]), ptr(tp["counts"]), ptr(tp["nodes_map"]), ptr(d_wait), None, None,
                                                 ptr(d_apt), ptr(d_apw), ptr(out["rows"]), ptr(out["counts"]),
                                                 ptr(out["nodes_map"]), ptr(out["actions_map"]), ptr(res["flags"])),
               "vap_time_insert_events")
    torch.cuda.synchronize()
    assert bool((buf[B * EVENT_CAP * 8:] == SENTINEL).all().item()), "rows with waits were written behind the last path's capacity"
    return out


def _time_run(torch, name, wp64, kernel, plan):
    """profile -> time_profile -> vap_time_insert_events with a wait on node 3 of the first bad path and of the first good
    one; both time-domain calls write into sentinel-filled buffers with a sentinel tail behind the last path's rows."""
    p = bc.placement(name)
    B, W = p["B"], p["W"]
    gen = gen_for("f32", "auto")
    gen.set_time_kernel(kernel)
    try:
        res = gen.profile(torch.tensor(wp64, dtype=gen.tdtype, device=gen.device), **_grid_kw(p["grids"][0]))
        tail = 4096
        buf = torch.full((B * TIME_CAP * 8 + tail,), SENTINEL, dtype=torch.float64, device=gen.device)
        out = {"rows": buf[:B * TIME_CAP * 8].view(B, TIME_CAP, 8),
               "counts": torch.full((B, 2), -1, dtype=torch.int32, device=gen.device),
               "nodes_map": torch.full((B, W), -1, dtype=torch.int32, device=gen.device)}
        tp = gen.time_profile(res, capacity_rows=TIME_CAP, out=out)
        torch.cuda.synchronize()
        assert bool((buf[B * TIME_CAP * 8:] == SENTINEL).all().item()), "rows were written behind the last path's capacity"
        waits = np.zeros((B, W))
        first_bad = min(plan) if plan else p["bad"][0]
        first_good = next(b for b in range(B) if b not in p["bad"])
        waits[first_bad, 3] = 0.25
        waits[first_good, 3] = 0.25
        ev = _insert_events(torch, gen, res, tp, waits)
    finally:
        gen.set_time_kernel("auto")
    return res, tp, ev


@functools.lru_cache(maxsize=None)
def clean_time(name, kernel):
    import torch
    res, tp, ev = _time_run(torch, name, bc.clean_batch(name), kernel, {})
    assert not res["flags"].any().item()
    return res, tp, ev


@pytest.mark.parametrize("label", bc.CALL_LABELS)
@pytest.mark.parametrize("kernel", ["lane", "quad", "fused"])
@pytest.mark.parametrize("name", ["solo", "time19"])
def test_time_domain_keeps_the_neighbours(torch_mod, name, kernel, label):
    from vexautonomousplanner_amd import _lib
    torch = torch_mod
    wp, plan = bc.dirty_batch(name, label, True)
    c_res, c_tp, c_ev = clean_time(name, kernel)
    res, tp, ev = _time_run(torch, name, wp, kernel, plan)
    good = torch.tensor(bc.good_mask(name, plan), device=res["flags"].device)
    what = f"time {name} {kernel} {label}"
    # the kinematic rows: whole buffers (sentinel behind every path's count), counts, nodes_map
    for k in ("rows", "counts", "nodes_map"):
        assert same_bytes(tp[k][good], c_tp[k][good]), (what, k)
    assert not res["flags"][good].any().item(), what
    counts = tp["counts"].cpu().numpy()
    flags = res["flags"].cpu().numpy()
    for b, kind in plan.items():
        assert 0 <= counts[b, 0] <= TIME_CAP and 0 <= counts[b, 1] <= bc.placement(name)["W"], (what, b, kind, counts[b])
        if kind in bc.FLAG_ASSERTED:        # still there after time_profile and insert_events
            assert flags[b] & _lib.FLAG_DEGENERATE, (what, b, kind, flags[b])
        if flags[b] & ~_lib.FLAG_DEGENERATE:
            print(f"{what} path {b} kind {kind}: extra bits {flags[b] & ~_lib.FLAG_DEGENERATE}")
    # the rows with waits: whole sentinel-filled buffers of the good paths, their counts and maps; a bad path's counts
    for k in ("rows", "counts", "nodes_map", "actions_map"):
        assert same_bytes(ev[k][good], c_ev[k][good]), (what, "with waits", k)
    ec = ev["counts"].cpu().numpy()
    first_good = int(np.flatnonzero(bc.good_mask(name, plan))[0])
    assert counts[first_good, 0] < ec[first_good, 0] <= EVENT_CAP, (what, "the good path's wait is not in its rows")
    for b, kind in plan.items():
        assert 0 <= ec[b, 0] <= EVENT_CAP and 0 <= ec[b, 1] <= bc.placement(name)["W"], (what, b, kind, ec[b])


# ---- the consumers of the rows ----------------------------------------------------------------------------------------------------------
def _consumers(torch, wp64):
    """Node limits, curve caps, conditioning and closest points on the solo batch, each on a fresh profile."""
    from vexautonomousplanner_amd import drive
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
    p = bc.PLACEMENTS["solo"]
    B, W = p["B"], p["W"]
    gen = gen_for("f32", "auto")
    wp = torch.tensor(wp64, dtype=gen.tdtype, device=gen.device)
    kw = _grid_kw(p["grids"][0])
    out = {}
    mv = np.zeros((B, W))
    mv[:, 3] = 2.0
    stop = np.zeros((B, W), dtype=bool)
    stop[:, 5] = True
    r = gen.apply_node_limits(gen.profile(wp, **kw), node_max_velocity=mv, node_stop=stop)
    out["limits"] = {k: r[k].clone() for k in ("velocity", "vcap", "node_sample", "flags")}
    r = gen.apply_curve_caps(gen.profile(wp, **kw), drive.CurveCaps.from_constraints(DEFAULT_CONSTRAINTS))
    out["caps"] = {k: r[k].clone() for k in ("velocity", "vcap", "n_bound", "flags")}
    res = gen.profile(wp, **kw)
    c = gen.conditioning(res, probes=3, limit=float("inf"))
    out["conditioning"] = {k: c[k].clone() for k in ("cond", "worst_sample", "worst_probe", "flags", "predicted_error")}
    rng = np.random.default_rng(5)
    q = torch.tensor(rng.uniform(-9.0, -1.0, (33, 2)), dtype=torch.float64, device=gen.device)
    for mode in ("gui", "exact"):
        c = gen.closest_points(res, q, mode=mode)
        out["closest_" + mode] = {k: v.clone() for k, v in c.items()}
    out["profile_flags"] = res["flags"].clone()
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def clean_consumers():
    import torch
    return _consumers(torch, bc.clean_batch("solo"))


@pytest.mark.parametrize("label", bc.CALL_LABELS)
def test_consumers_of_the_rows_keep_the_neighbours(torch_mod, label):
    torch = torch_mod
    wp, plan = bc.dirty_batch("solo", label, True)
    clean = clean_consumers()
    dirty = _consumers(torch, wp)
    good = torch.tensor(bc.good_mask("solo", plan), device=dirty["profile_flags"].device)
    assert not dirty["profile_flags"][good].any().item()
    for stage in ("limits", "caps", "conditioning", "closest_gui", "closest_exact"):
        for k, t in dirty[stage].items():
            assert same_bytes(t[good], clean[stage][k][good]), (label, stage, k)
        assert not clean[stage]["flags"].any().item(), (stage, "the clean batch is flagged")


# ---- the ranking ----------------------------------------------------------------------------------------------------------------------
def test_search_update_ranks_the_bad_candidates_last_and_the_rest_as_before(torch_mod):
    """vap_search_update on the first 8192 paths of a dirty many8 call (R = 2 problems of N = 4096 candidates): the bad
    candidates cost +inf and rank behind every finite one; the order of the good ones, the refitted mean and sigma and the
    best-so-far are those of the clean batch with the same candidates forced out by a flag."""
    from vexautonomousplanner_amd import _lib, search
    torch = torch_mod
    p = bc.PLACEMENTS["many8"]
    grid = p["grids"][0]
    wp, plan = bc.dirty_batch("many8", "rot0", True)
    _, dirty = profile(torch, "many8", wp, grid, "f32", "auto")
    clean = clean_run("many8", grid, "f32", "auto")
    R, N, W = 2, 4096, p["W"]
    bad = sorted(b for b in plan if b < R * N)
    assert len(bad) == 6
    dev = dirty["flags"].device
    forced = clean["flags"][:R * N].clone()
    forced[bad] = _lib.FLAG_DEGENERATE

    def update(wp64, meta, flags):
        st = dict(mean=torch.zeros((R, W, 2), dtype=torch.float64, device=dev),
                  sigma=torch.full((R, W, 2), 0.5, dtype=torch.float64, device=dev),
                  best_cost=torch.full((R,), float("inf"), dtype=torch.float64, device=dev),
                  best_waypoints=torch.zeros((R, W, 2), dtype=torch.float32, device=dev),
                  best_terms=torch.zeros((R, 4), dtype=torch.float64, device=dev))
        w = torch.tensor(wp64[:R * N], dtype=torch.float32, device=dev).contiguous()
        res = search.update(w, R, meta=meta[:R * N].contiguous(), flags=flags[:R * N].contiguous(), elites=64, alpha=0.7,
                            sigma_min=1e-3, sigma_max=2.0, **st)
        torch.cuda.synchronize()
        return res, st

    d_res, d_st = update(wp, dirty["meta"], dirty["flags"])
    c_res, c_st = update(bc.clean_batch("many8"), clean["meta"], forced)
    cost = d_res["cost"].cpu().numpy()
    order = d_res["order"].cpu().numpy()
    c_order = c_res["order"].cpu().numpy()
    is_bad = np.zeros(R * N, dtype=bool)
    is_bad[bad] = True
    assert np.all(np.isposinf(cost[is_bad])) and np.all(np.isfinite(cost[~is_bad]))
    for r in range(R):
        bad_r = is_bad[r * N:(r + 1) * N]
        o, co = order[r], c_order[r]
        assert sorted(o.tolist()) == list(range(N))
        n_bad = int(bad_r.sum())
        assert n_bad == (6 if r == 0 else 0) and np.all(bad_r[o[N - n_bad:]]) and not np.any(bad_r[o[:N - n_bad]])     # behind every finite one
        assert np.array_equal(o[~bad_r[o]], co[~bad_r[co]])
    assert same_bytes(d_res["cost"][torch.tensor(~is_bad, device=dev)], c_res["cost"][torch.tensor(~is_bad, device=dev)])
    assert torch.equal(d_res["n_feasible"], c_res["n_feasible"])
    for k in d_st:
        assert same_bytes(d_st[k], c_st[k]), k
