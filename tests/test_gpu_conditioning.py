"""GPU: vap_velocity_conditioning against tests/conditioning_ref.py, bit for bit, on caller-written rows.

The replica and the kernel perform the same IEEE fp64 operations in the same order (the library is compiled without
contraction, its divisions are the correctly rounded ones), the signs come from the same Philox block and every maximum is
taken under the same total order: cond, worst_sample, worst_probe, sensitivity and flags are compared as bits.  The velocity
row is vel_sqrt of the unperturbed sweep: the hardware estimate of 1/sqrt, a coupled Newton step and a residual correction,
whose result before the last rounding is within ~2^-90 of the root — it is the correctly rounded root unless the root lies
that close to a rounding boundary, one sample in 2^36 — so it is compared with np.sqrt as bits too.
Rows: 256-sample windows of fixture c3_p0_S10000's curvature and heading rows (8 to 250 state-dependent steps, cond 0.8 to
46), as they are and with the recurrence's special branches planted.  Every output is prefilled with a sentinel."""
import functools

import numpy as np
import pytest

import conditioning_ref as cr
import golden_util as gu

pytestmark = pytest.mark.gpu

OFFSETS = (0, 2048, 5120, 6656, 9728)
WIN = 256
SENT = -777.0


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vexautonomousplanner_amd import _lib
    return torch, _lib.Context(0)


@functools.lru_cache(maxsize=None)
def golden():
    g = gu.load("c3_p0_S10000")
    return g["grid_curvature"], g["grid_heading"], g["grid_velocity"], float(g["dd"]), tuple(float(x) for x in g["constraints"])


def window(off, n=WIN):
    k, h, v, dd, cons = golden()
    return k[off:off + n].copy(), cr.dtheta(h[off:off + n]), float(v[off]), float(v[off + n - 1])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def device_probe(env, kappa, dth, N, dd, cons, sv, ev, K=3, delta=2.0 ** -40, seed=0, first_path=0, limit=np.inf, out=None,
                 rows_dtype=np.float64, **rows):
    """One call on B rows (kappa, dth: (B, S); N, dd: (B,)), every output prefilled; numpy results and the out dict."""
    torch, ctx = env
    from vexautonomousplanner_amd import conditioning
    kappa, dth = np.atleast_2d(kappa), np.atleast_2d(dth)
    B, S = kappa.shape
    meta = np.zeros((B, 4))
    meta[:, 2], meta[:, 3] = dd, N
    dev = torch.device("cuda", 0)
    if out is None:
        out = {"cond": torch.full((B,), SENT, dtype=torch.float64, device=dev),
               "worst_sample": torch.full((B,), -99, dtype=torch.int32, device=dev),
               "worst_probe": torch.full((B,), -99, dtype=torch.int32, device=dev),
               "flags": torch.full((B,), 0x55, dtype=torch.int32, device=dev),
               "sensitivity": torch.full((B, S), SENT, dtype=torch.float64, device=dev),
               "velocity": torch.full((B, S), SENT, dtype=torch.float64, device=dev)}
    tdt = torch.float64 if rows_dtype == np.float64 else torch.float32
    res = conditioning.probe(meta, torch.tensor(kappa.astype(rows_dtype), dtype=tdt, device=dev),
                             torch.tensor(dth.astype(rows_dtype), dtype=tdt, device=dev), constraints=cons, start_vel=sv, end_vel=ev,
                             probes=K, delta=delta, seed=seed, first_path=first_path, limit=limit, per_sample=True, velocity=True,
                             out=out, ctx=ctx, **rows)
    torch.cuda.synchronize()
    assert all(res[k] is out[k] for k in out)
    return {k: v.cpu().numpy() for k, v in res.items()}, out


def replica(kappa, dth, N, dd, cons, sv, ev, K=3, delta=2.0 ** -40, seed=0, first_path=0, limit=np.inf, rows_dtype=np.float64,
            **rows):
    kappa, dth = np.atleast_2d(kappa), np.atleast_2d(dth)
    B, S = kappa.shape
    N, dd = np.broadcast_to(N, (B,)), np.broadcast_to(dd, (B,))
    out = []
    for b in range(B):
        r = {k: (np.asarray(v)[b] if v is not None else None) for k, v in rows.items()}
        r = {{"acc_forward": "acc_fwd", "acc_backward": "acc_bwd", "dec_backward": "dec"}.get(k, k): v for k, v in r.items() if v is not None}
        out.append(cr.probe(kappa[b].astype(rows_dtype).astype(np.float64), dth[b].astype(rows_dtype).astype(np.float64), int(N[b]),
                            float(dd[b]), cons, sv, ev, K=K, delta=delta, seed=seed, path=first_path + b, limit=limit, S=S, **r))
    return out


def check(got, want, what=""):
    """Every output of a call against the replica's paths, as bits."""
    for b, w in enumerate(want):
        tag = (what, b)
        assert bits(got["cond"][b]) == bits(w["cond"]), (tag, got["cond"][b], w["cond"])
        assert (int(got["worst_sample"][b]), int(got["worst_probe"][b])) == (w["worst_sample"], w["worst_probe"]), tag
        assert int(got["flags"][b]) == w["flag"], (tag, got["flags"][b])
        assert np.array_equal(bits(got["sensitivity"][b]), bits(w["sensitivity"])), (tag, "sensitivity")
        assert np.array_equal(bits(got["velocity"][b]), bits(w["velocity"])), (tag, "velocity")


def both(env, *a, **kw):
    got, _ = device_probe(env, *a, **kw)
    want = replica(*a, **kw)
    check(got, want, kw)
    return got, want


@pytest.mark.parametrize("off", OFFSETS)
def test_windows_of_a_golden_path(env, off):
    k, d, sv, ev = window(off)
    _, _, _, dd, cons = golden()
    got, want = both(env, k, d, WIN, dd, cons, sv, ev, limit=5.0)
    print(f"COND window {off}: cond {want[0]['cond']:.3g} at sample {want[0]['worst_sample']} probe {want[0]['worst_probe']}, flag {want[0]['flag']}")
    assert want[0]["cond"] > 0.0


@pytest.mark.parametrize("off", OFFSETS)
def test_planted_branches(env, off):
    """Three zero heading differences (the +-inf and 0 / 0 quotients), four curvatures at 0 and four at 5e-7 (the straight
    branch), one negative curvature."""
    k, d, sv, ev = window(off)
    _, _, _, dd, cons = golden()
    d[[40, 41, 130]] = 0.0
    k[[60, 61, 62, 131]] = 0.0
    k[[90, 91, 92, 200]] = 5e-7
    k[150] = -k[150]
    both(env, k, d, WIN, dd, cons, sv, ev, limit=5.0)


def ragged(B=70, S=WIN):
    """B rows cut from the golden path at scattered offsets, with sample counts 0 .. S: the lanes of a wave end at different
    steps and the batch spans waves for every K."""
    kk, h, _, dd, cons = golden()
    rng = np.random.default_rng(21)
    offs = rng.integers(0, len(kk) - WIN, size=B)
    N = rng.integers(3, WIN + 1, size=B)
    N[:6] = (0, 1, 2, 3, WIN, WIN - 1)
    kap, dth = np.zeros((B, S)), np.zeros((B, S))
    for b in range(B):
        kap[b, :WIN] = kk[offs[b]:offs[b] + WIN]
        dth[b, :WIN] = cr.dtheta(h[offs[b]:offs[b] + WIN])
    return kap, dth, N, np.full(B, dd), cons


@pytest.mark.parametrize("K", [1, 3, 7, 15])
def test_ragged_batch_every_probe_count(env, K):
    kap, dth, N, dd, cons = ragged()
    got, want = both(env, kap, dth, N, dd, cons, 0.3, 0.2, K=K, seed=5, limit=2.0)
    assert [w["cond"] for w in want[:2]] == [0.0, 0.0] and [w["worst_sample"] for w in want[:2]] == [-1, -1]   # N = 0, 1
    assert got["velocity"][1, 0] == 0.2 and not got["velocity"][0].any()                                       # end_vel at sample N - 1
    assert 0 < sum(w["flag"] != 0 for w in want) < len(want)


def test_limit_rows_and_fp32_rows(env):
    """A vcap row with a 0.01 stop mid-row, acceleration rows that change mid-row, and fp32 rows (widened)."""
    kap, dth, N, dd, cons = ragged(B=9)
    N[:] = WIN
    vcap = np.full(kap.shape, cons[0])
    vcap[:, 100] = 0.01
    vcap[:, 180:] = 2.5
    both(env, kap, dth, N, dd, cons, 0.3, 0.2, vcap=vcap)
    af, ab = np.full(kap.shape, cons[1]), np.full(kap.shape, cons[1])
    af[:, 120:], ab[:, 90:] = 5.0, 6.5
    both(env, kap, dth, N, dd, cons, 0.3, 0.2, vcap=vcap, acc_forward=af, acc_backward=ab, dec_backward=np.full(len(kap), 5.0))
    both(env, kap, dth, N, dd, cons, 0.3, 0.2, rows_dtype=np.float32)


def test_split_first_path_and_repeat(env):
    """The host's cut into launches, the batch's position and a second call do not change a bit."""
    torch, ctx = env
    from vexautonomousplanner_amd import _lib
    S = 4096                                                  # 128 KiB of probe rows per path: 8 paths per launch under 1 MiB
    kap, dth, N, dd, cons = ragged(S=S)
    one, out = device_probe(env, kap, dth, N, dd, cons, 0.3, 0.2, seed=9, limit=20.0)
    check(one, replica(kap, dth, N, dd, cons, 0.3, 0.2, seed=9, limit=20.0), "one launch")
    again, _ = device_probe(env, kap, dth, N, dd, cons, 0.3, 0.2, seed=9, limit=20.0, out=out)   # into the same buffers
    ctx.set_option(_lib.OPT_CONDITIONING_SCRATCH_MB, 1)
    try:
        cut, _ = device_probe(env, kap, dth, N, dd, cons, 0.3, 0.2, seed=9, limit=20.0)           # 70 paths: 9 launches
    finally:
        ctx.set_option(_lib.OPT_CONDITIONING_SCRATCH_MB, 512)
    part, _ = device_probe(env, kap[5:10], dth[5:10], N[5:10], dd[5:10], cons, 0.3, 0.2, seed=9, first_path=5, limit=20.0)
    for k in one:
        assert np.array_equal(one[k].view(np.uint8), again[k].view(np.uint8)), ("repeat", k)
        assert np.array_equal(one[k].view(np.uint8), cut[k].view(np.uint8)), ("cut", k)
        assert np.array_equal(one[k][5:10].view(np.uint8), part[k].view(np.uint8)), ("first_path", k)
    other, _ = device_probe(env, kap[5:10], dth[5:10], N[5:10], dd[5:10], cons, 0.3, 0.2, seed=9, first_path=0, limit=20.0)
    assert not np.array_equal(one["cond"][5:10], other["cond"])          # the position is part of the pattern


@pytest.fixture(scope="module")
def gen64():
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    return BatchedTrajectoryGenerator(0, "f64", velocity_kernel="seq_literal")


def test_unperturbed_sweep_is_the_literal_kernel(env, gen64):
    """d_velocity against vap_velocity_pass under VAP_VELOCITY_SEQ_LITERAL on an fp64 profile() of 8 random paths."""
    torch, _ = env
    from vexautonomousplanner_amd import conditioning
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    wp = torch.tensor(make_waypoints(8, 32, 31), dtype=torch.float64, device=gen64.device)
    r = gen64.profile(wp, DEFAULT_CONSTRAINTS, samples=2048)
    out = {"velocity": torch.full((8, 2048), SENT, dtype=torch.float64, device=gen64.device)}
    c = conditioning.probe(r["meta"], r["curvature"], None, constraints=DEFAULT_CONSTRAINTS, velocity=True, out=out, ctx=gen64.ctx)
    torch.cuda.synchronize()
    assert c["velocity"] is out["velocity"] and torch.equal(c["velocity"], r["velocity"])
    cond = c["cond"].cpu().numpy()
    print(f"COND 8 random paths: cond {cond.min():.3g} .. {cond.max():.3g}")
    assert (cond > 0.0).all()


def test_generator_refuses_a_stale_result_and_keeps_the_flags(env, gen64):
    torch, _ = env
    from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS, make_waypoints
    wp = torch.tensor(make_waypoints(4, 8, 32), dtype=torch.float64, device=gen64.device)
    old = gen64.profile(wp, DEFAULT_CONSTRAINTS, samples=512)
    new = gen64.profile(wp, DEFAULT_CONSTRAINTS, samples=512)
    with pytest.raises(ValueError, match="LAST profile"):
        gen64.conditioning(old, limit=1e4)
    with pytest.raises(TypeError):
        gen64.conditioning(new)                                         # no default limit is shipped
    new["flags"].fill_(2)
    c = gen64.conditioning(new, limit=1e-3, per_sample=True)            # every path is above that: all flagged
    torch.cuda.synchronize()
    assert new["flags"].tolist() == [2] * 4 and c["flags"].tolist() == [1024] * 4
    assert set(c) == {"cond", "worst_sample", "worst_probe", "flags", "sensitivity", "predicted_error"}
    from vexautonomousplanner_amd import conditioning
    assert torch.equal(c["predicted_error"], c["cond"] * conditioning.ETA)
    assert torch.equal(c["sensitivity"].max(dim=1).values, c["cond"])


LIMIT = 1e4     # the least a default limit would have had to be; the calibration gave 4.8e3, so none is shipped and callers name one


def test_big_path_is_flagged_and_the_golden_path_is_not(env):
    """big_w2048_p2 through profile() in fp64: cond >= 1e5 and flagged at a limit of 1e4; c3_p0's waypoints: not.  (The issue
    asks for "the shipped default" here; the calibration it prescribes gave a limit of 4.8e3, below the 1e4 at which it
    says to ship none, so the limit is explicit — DESIGN.md section 21.)"""
    torch, _ = env
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    gen = BatchedTrajectoryGenerator(0, "f64")
    g = gu.load("big_w2048_p2")
    N = int(g["n_samples"])
    r = gen.profile(torch.tensor(g["waypoints"][None], dtype=torch.float64, device=gen.device), g["constraints"], dd=float(g["dd"]),
                    capacity=N + 2)
    c = gen.conditioning(r, constraints=g["constraints"], limit=LIMIT)
    torch.cuda.synchronize()
    cond = float(c["cond"][0].item())
    print(f"COND big_w2048_p2 on the device: cond {cond:.3g} at sample {int(c['worst_sample'][0].item())}, predicted error "
          f"{float(c['predicted_error'][0].item()):.2e}")
    assert int(r["meta"][0, 3].item()) == N and cond >= 1e5 and c["flags"].tolist() == [1024]
    g = gu.load("c3_p0_S10000")
    r = gen.profile(torch.tensor(g["waypoints"][None], dtype=torch.float64, device=gen.device), g["constraints"], samples=10000)
    c = gen.conditioning(r, constraints=g["constraints"], limit=LIMIT)
    torch.cuda.synchronize()
    print(f"COND c3_p0 on the device: cond {float(c['cond'][0].item()):.3g}")
    assert c["flags"].tolist() == [0] and float(c["cond"][0].item()) < 1e4
