"""Every velocity kernel under other robots and start / end speeds (the cases of robot_cases.py, which
test_velocity_robots_cpu.py proves on the oracle to reach the plateau at max_vel, a lowered start speed, a kept end
speed).

  anchor        seq_fast and seq_literal against the oracle, every robot, every start / end speed but (0, 0), fp32 and
                fp64 rows, at the lanes and register-resident shapes on make_waypoints / straight / manhattan paths.
                Bounds: the ones AUTO is held to in test_gpu_sweeps.test_fuzz_slice_random_shapes_robots_grids — velocity
                1e-5 ("f32") and 1e-7 ("f64"), geometry 1e-5 and 1e-9.  No new tolerance.
  bit identity  relax / relax_block, look-back relax and relax_rounds on long rows, relax_wave, lanes16 / 32 / 64 against
                seq_fast: the velocity rows (the lanes kernels: the curvature rows too) as BIT PATTERNS, every robot, all
                five start / end speeds; the ragged case with zeros past n_samples; limit rows (VCAP, VCAP + ACC); AUTO at
                2048 paths; the constants the recurrence ignores; the residual row behind the time domain.
"f32r32" (the all-fp32 recurrence) is known to leave the oracle bound and is held by bit identity only.
Every comparison with the oracle prints its worst values on a line starting with "ROBOTS" (DESIGN.md quotes them)."""
import numpy as np
import pytest

import robot_cases as rc
from test_gpu_parity import make_gen, torch_mod  # noqa: F401  (fixture)
from test_gpu_sweeps import per_path_errors

pytestmark = pytest.mark.gpu

ROWS = ("x", "y", "heading", "curvature", "velocity")
LANES = ["lanes16", "lanes32", "lanes64"]
BOUNDS = {"f32": (1e-5, 1e-5), "f64": (1e-7, 1e-9)}          # (velocity, geometry)

_GENS = {}        # one generator per (dtype, kernel) for the whole module: no test spends its time creating contexts
_SEQ = {}         # seq_fast's rows per case, shared by the tests that compare a kernel with them; never modified


def gen(dtype, kernel):
    if (dtype, kernel) not in _GENS:
        _GENS[(dtype, kernel)] = make_gen(dtype, velocity_kernel=kernel)
    return _GENS[(dtype, kernel)]


def run(torch, dtype, kernel, wp, cons, sv, ev, want=("curvature", "velocity"), **grid):
    """profile() through the generator of (dtype, kernel); rows as NumPy arrays of the rows' own type."""
    g = gen(dtype, kernel)
    r = g.profile(torch.tensor(wp, dtype=g.tdtype, device=g.device), cons, start_vel=sv, end_vel=ev, want=want, **grid)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items() if k in want or k in ("flags", "meta")}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def seq_rows(torch, dtype, kind, B, W, S, robot, sv, ev):
    key = (dtype, kind, B, W, S, robot, sv, ev)
    if key not in _SEQ:
        r = run(torch, dtype, "seq_fast", rc.paths(kind, B, W), rc.ROBOTS[robot], sv, ev, want=ROWS, samples=S)
        assert not r["flags"].any(), key
        for v in r.values():
            v.setflags(write=False)
        _SEQ[key] = r
    return _SEQ[key]


def assert_equals_seq_fast(torch, dtype, kernels, cases, curvature=False, ends=rc.END_SPEEDS):
    """Each of `kernels` against seq_fast on every (kind, B, W, S) of `cases`, every robot, every start / end speed:
    equal bit patterns of the velocity rows (and the curvature rows).  All mismatches are collected before failing."""
    bad, n = [], 0
    for kind, B, W, S in cases:
        wp = rc.paths(kind, B, W)
        for robot, cons in rc.ROBOTS.items():
            for sv, ev in ends:
                ref = seq_rows(torch, dtype, kind, B, W, S, robot, sv, ev)
                for kernel in kernels:
                    r = run(torch, dtype, kernel, wp, cons, sv, ev, samples=S)
                    n += 1
                    ok = not r["flags"].any() and same_bits(r["velocity"], ref["velocity"])
                    if ok and curvature:
                        ok = same_bits(r["curvature"], ref["curvature"])
                    if not ok:
                        rows = np.nonzero(np.any(bits(r["velocity"]) != bits(ref["velocity"]), axis=1))[0]
                        bad.append((kernel, dtype, kind, B, W, S, robot, sv, ev, r["flags"].tolist()[:4], rows.tolist()[:8]))
    assert not bad, (len(bad), n, bad[:12])
    return n


# ---- anchor: the sequential sweeps against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kernel", ["seq_fast", "seq_literal"])
def test_sequential_sweeps_hold_the_oracle_bound(torch_mod, kernel, dtype):
    """Worst figures observed (MI355X): see DESIGN.md, section 5, "Other robots and start / end speeds"."""
    tol_v, tol_g = BOUNDS[dtype]
    worst = {k: 0.0 for k in ROWS}
    fails = []
    for kind, B, W, S in rc.anchor_cases():
        wp = rc.paths(kind, B, W)
        for robot, cons in rc.ROBOTS.items():
            for sv, ev in rc.ORACLE_END_SPEEDS:
                ref = rc.oracle_rows(kind, B, W, S, robot, sv, ev)
                if kernel == "seq_fast":
                    r = seq_rows(torch_mod, dtype, kind, B, W, S, robot, sv, ev)
                else:
                    r = run(torch_mod, dtype, kernel, wp, cons, sv, ev, want=ROWS, samples=S)
                assert not r["flags"].any(), (kind, B, W, S, robot, sv, ev)
                got = {k: r[k].astype(np.float64) for k in ROWS}
                assert np.all(np.isfinite(got["velocity"]))
                np.testing.assert_allclose(r["meta"][:, 1], ref["total_length"], rtol=1e-14)
                e = {k: float(v.max()) for k, v in per_path_errors(got, ref).items()}
                for k in ROWS:
                    worst[k] = max(worst[k], e[k])
                if not (e["velocity"] <= tol_v and all(e[k] <= tol_g for k in ("curvature", "heading", "x", "y"))):
                    fails.append((kind, B, W, S, robot, sv, ev, e))
    print(f"ROBOTS anchor {kernel} {dtype}: worst " + " ".join(f"{k} {worst[k]:.2e}" for k in ROWS))
    assert not fails, (len(fails), fails[:8])


# ---- bit identity with the sequential sweep ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f32r32", "f64"])
@pytest.mark.parametrize("kernel", ["relax", "relax_block"])
def test_register_resident_relaxation_equals_the_sequential_sweep(torch_mod, kernel, dtype):
    cases = [(kind, B, W, S) for (B, W, S) in rc.LANES_SHAPES + rc.RELAX_SHAPES for kind in rc.PATH_SETS]
    assert_equals_seq_fast(torch_mod, dtype, [kernel], cases)


@pytest.mark.parametrize("dtype", ["f32", "f32r32", "f64"])
@pytest.mark.parametrize("kernel", ["relax", "relax_rounds"])
def test_long_row_kernels_equal_the_sequential_sweep(torch_mod, kernel, dtype):
    """Just past velocity_relax_max_samples, the last super-chunk ragged: look-back ("relax") and one launch per round."""
    B, W, S = rc.LONG_SHAPES[dtype]
    assert_equals_seq_fast(torch_mod, dtype, [kernel], [(kind, B, W, S) for kind in rc.LONG_PATH_SETS])


def test_wave_per_path_kernel_equals_the_sequential_sweep(torch_mod):
    """Two windows, the second of one sample; the fp32 recurrence is the only one this kernel has."""
    assert_equals_seq_fast(torch_mod, "f32r32", ["relax_wave", "relax_block"], [(kind,) + rc.WAVE_SHAPE for kind in rc.PATH_SETS])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kernel", LANES)
def test_lanes_kernels_equal_the_sequential_sweep(torch_mod, kernel, dtype):
    """Velocity AND curvature rows (fp32 rows: this kernel's backward sweep writes the curvature row itself)."""
    cases = [(kind, B, W, S) for (B, W, S) in rc.LANES_SHAPES + rc.RELAX_SHAPES for kind in rc.PATH_SETS]
    assert_equals_seq_fast(torch_mod, dtype, [kernel], cases, curvature=True)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_ragged_rows_equal_the_sequential_sweep_and_end_in_zeros(torch_mod, dtype):
    """The reference's own grid: every path has its own n_samples.  The slots past a row's end hold end_u inside the
    lanes kernel — the last sample of every row IS end_vel, the samples past it are zero, in both rows."""
    wp = rc.paths("walk", rc.RAGGED["B"], rc.RAGGED["W"])
    grid = dict(dd=rc.RAGGED["dd"], capacity=rc.RAGGED["capacity"])
    cols = np.arange(rc.RAGGED["capacity"])[None, :]
    for robot, cons in rc.ROBOTS.items():
        for sv, ev in rc.END_SPEEDS:
            ref = run(torch_mod, dtype, "seq_fast", wp, cons, sv, ev, **grid)
            n = ref["meta"][:, 3].astype(int)
            assert not ref["flags"].any() and len(set(n.tolist())) > 5 and n.max() < rc.RAGGED["capacity"]
            last = ref["velocity"][np.arange(len(wp)), n - 1]
            assert np.array_equal(last, np.full(len(wp), ev, dtype=last.dtype)), (robot, sv, ev)
            for kernel in LANES + ["relax"]:
                r = run(torch_mod, dtype, kernel, wp, cons, sv, ev, **grid)
                what = (kernel, dtype, robot, sv, ev)
                assert not r["flags"].any() and np.array_equal(r["meta"], ref["meta"]), what
                assert same_bits(r["velocity"], ref["velocity"]) and same_bits(r["curvature"], ref["curvature"]), what
                past = cols >= n[:, None]
                assert np.all(bits(r["velocity"])[past] == 0) and np.all(bits(r["curvature"])[past] == 0), what


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("with_acc", [False, True], ids=["vcap", "vcap_acc"])
def test_limit_rows_kernels_equal_the_sequential_sweep(torch_mod, with_acc, dtype):
    """The VCAP and VCAP + ACC instantiations under SLOW_NARROW and FAST_WIDE with (1.2, 0.7): random node max_velocity
    (below the robot's own max_vel), stops and max_acceleration through apply_node_limits, on the reference's grid (ragged
    rows) and on the fixed grid of (70, 5, 449): the lanes kernels and relax equal seq_fast bit for bit."""
    torch = torch_mod
    sv, ev = 1.2, 0.7
    B0, W0, S0 = rc.LANES_SHAPES[0]
    grids = [(rc.paths("walk", rc.RAGGED["B"], rc.RAGGED["W"]), dict(dd=rc.RAGGED["dd"], capacity=rc.RAGGED["capacity"])),
             (rc.paths("walk", B0, W0), dict(samples=S0)), (rc.paths("manhattan", B0, W0), dict(samples=S0))]
    for robot in ("SLOW_NARROW", "FAST_WIDE"):
        cons = rc.ROBOTS[robot]
        for gi, (wp, grid) in enumerate(grids):
            B, W = wp.shape[:2]
            rng = np.random.default_rng([5, gi, int(with_acc)])
            mv = np.where(rng.random((B, W)) < 0.4, rng.uniform(0.25, 0.9, (B, W)) * cons[0], 0.0)
            ma = np.where(rng.random((B, W)) < 0.5, rng.uniform(0.4, 1.75, (B, W)) * cons[1], 0.0) if with_acc else None
            stop = rng.random((B, W)) < 0.2
            stop[:, 0] = stop[:, -1] = False
            rows = {}
            for kernel in ["seq_fast", "relax"] + LANES:
                g = gen(dtype, kernel)
                r = g.profile(torch.tensor(wp, dtype=g.tdtype, device=g.device), cons, start_vel=sv, end_vel=ev, **grid)
                plain = r["velocity"].cpu().numpy()
                g.apply_node_limits(r, cons, node_max_velocity=mv, node_stop=stop, node_max_acceleration=ma, start_vel=sv, end_vel=ev)
                torch.cuda.synchronize()
                assert int(r["flags"].abs().max().item()) == 0, (kernel, robot, gi)
                assert ("acc_forward" in r) == with_acc
                rows[kernel] = r["velocity"].cpu().numpy()
                assert np.mean(rows[kernel] < plain) > 0.05, (kernel, robot, gi)       # the limits bind
            for kernel in ["relax"] + LANES:
                assert same_bits(rows[kernel], rows["seq_fast"]), (kernel, dtype, robot, gi, with_acc)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_auto_takes_the_lanes_kernel_at_2048_paths_under_another_robot(torch_mod, dtype):
    """CRAWL with (2.0, 0.3): AUTO's rows equal forced lanes and seq_fast bit for bit, every 97th path holds the bound."""
    from oracle import oracle
    B, W, S = rc.AUTO_SHAPE
    cons, (sv, ev) = rc.ROBOTS[rc.AUTO_ROBOT], rc.AUTO_ENDS
    wp = rc.paths(rc.AUTO_KIND, B, W)
    a = run(torch_mod, dtype, "auto", wp, cons, sv, ev, want=ROWS, samples=S)
    assert not a["flags"].any()
    for kernel in ("lanes", "seq_fast"):
        r = run(torch_mod, dtype, kernel, wp, cons, sv, ev, samples=S)
        assert not r["flags"].any(), kernel
        assert same_bits(r["velocity"], a["velocity"]) and same_bits(r["curvature"], a["curvature"]), kernel
    idx = rc.AUTO_ORACLE_PATHS
    ref = oracle.profile_batch(wp[idx], S, cons, start_vel=sv, end_vel=ev, n_threads=8)
    e = {k: float(v.max()) for k, v in per_path_errors({k: a[k][idx].astype(np.float64) for k in ROWS}, ref).items()}
    print(f"ROBOTS auto 2048 {dtype}: worst " + " ".join(f"{k} {e[k]:.2e}" for k in ROWS))
    tol_v, tol_g = BOUNDS[dtype]
    assert e["velocity"] <= tol_v and all(e[k] <= tol_g for k in ("curvature", "heading", "x", "y")), e


@pytest.mark.parametrize("kernel", ["seq_fast", "relax", "lanes16", "lanes64"])
def test_ignored_constants_do_not_move_a_bit(torch_mod, kernel):
    """friction_coef, max_jerk and max_dec alone (velocity_consts: cc[2] = max_acc, quirk Q9): the same velocity bits —
    and max_acc alone: other bits, so the comparison can fail."""
    B, W, S = rc.LANES_SHAPES[0]
    for dtype in ("f32", "f64"):
        for kind in ("walk", "manhattan"):
            wp = rc.paths(kind, B, W)
            for robot in ("DEFAULT", "SLOW_NARROW", "ACC_GT_DEC"):
                for sv, ev in ((0.01, 0.01), (1.2, 0.7)):
                    ref = seq_rows(torch_mod, dtype, kind, B, W, S, robot, sv, ev)["velocity"]
                    for name, (i, value) in rc.IGNORED_CONSTANTS.items():
                        cons = list(rc.ROBOTS[robot])
                        cons[i] = value
                        r = run(torch_mod, dtype, kernel, wp, cons, sv, ev, samples=S)
                        assert same_bits(r["velocity"], ref), (kernel, dtype, kind, robot, sv, ev, name)
                    cons = list(rc.ROBOTS[robot])
                    cons[1] *= 0.9375
                    r = run(torch_mod, dtype, kernel, wp, cons, sv, ev, samples=S)
                    assert not same_bits(r["velocity"], ref), (kernel, dtype, kind, robot, sv, ev)


@pytest.mark.parametrize("dt", [0.01, 1 / 60], ids=["0.01", "1/60"])
def test_residual_row_of_the_lanes_kernel_equals_the_sequential_sweeps(torch_mod, dt):
    """The default fp32 mode keeps what every fp32 velocity lost of its fp64 value (VAP_OPT_TIME_DOMAIN_RESIDUAL) for the
    time domain: the lanes kernel writes that row itself, the other kernels have it converted on the host path of
    run_velocity.  Under SLOW_NARROW with (1.2, 0.7): time_profile after a lanes16 / lanes64 / relax velocity pass gives
    the counts, maps, flags and row bytes — all eight columns — it gives after seq_fast."""
    torch = torch_mod
    cons, (sv, ev) = rc.ROBOTS["SLOW_NARROW"], (1.2, 0.7)
    B0, W0, S0 = rc.LANES_SHAPES[0]
    cap = 1500
    for wp, grid in ((rc.paths("walk", B0, W0), dict(samples=S0)), (rc.paths("manhattan", B0, W0), dict(samples=S0)),
                     (rc.paths("walk", rc.RAGGED["B"], rc.RAGGED["W"]), dict(dd=rc.RAGGED["dd"], capacity=rc.RAGGED["capacity"]))):
        got = {}
        for kernel in ("seq_fast", "lanes16", "lanes64", "relax"):
            g = gen("f32", kernel)
            assert g.time_domain_residual
            res = g.profile(torch.tensor(wp, dtype=g.tdtype, device=g.device), cons, start_vel=sv, end_vel=ev, **grid)
            tp = g.time_profile(res, cons, dt=dt, capacity_rows=cap)
            torch.cuda.synchronize()
            got[kernel] = (tp["rows"].cpu().numpy(), tp["counts"].cpu().numpy(), tp["nodes_map"].cpu().numpy(), res["flags"].cpu().numpy())
        rows_a, counts_a, nm_a, flags_a = got["seq_fast"]
        assert not flags_a.any() and counts_a[:, 0].min() >= 20 and counts_a[:, 0].max() < cap
        for kernel in ("lanes16", "lanes64", "relax"):
            rows_b, counts_b, nm_b, flags_b = got[kernel]
            assert np.array_equal(counts_a, counts_b) and np.array_equal(flags_a, flags_b), kernel
            for b in range(len(wp)):
                assert rows_a[b, :counts_a[b, 0]].tobytes() == rows_b[b, :counts_a[b, 0]].tobytes(), (kernel, b, grid)
                assert np.array_equal(nm_a[b, :counts_a[b, 1]], nm_b[b, :counts_a[b, 1]]), (kernel, b, grid)
