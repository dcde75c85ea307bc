"""GPU: vap_curve_caps and vap_drive_audit against tests/drive_ref.py, bit for bit, and the layers above them.

The kernels and the replica perform the same IEEE fp64 operations in the same order (the library is compiled without
contraction; its plain divisions and square roots are the correctly rounded ones), so caps, counts, peaks, rows and per-row
columns are compared as bits.  Paths: plain_w5_s0, plain_w8_s0 and a two-waypoint straight line (zero curvature: the lateral
cap is off on every sample) on the reference's grid dd = 0.005 with capacities S = 257 and S = 1024 (the goldens are cut at
257; the straight line ends below it).  The three have different waypoint counts, so the rows of the caller-row modes come
from three profile calls and go into one vap_curve_caps call; the mode that reads the context's own fp64 rows (fp32 rows,
d_curvature NULL) needs ONE profile call behind it and so runs each path as a batch of its own, and a batch of three
8-waypoint paths (plain_w8_s0, plain_w8_s1, eight collinear waypoints).  Its replica takes the fp64 curvature of an fp64
generator on the same (fp32-representable) waypoints; the test first checks that this row rounds to the fp32 row the fp32
generator returned.  Every output is prefilled with a sentinel."""
import math

import numpy as np
import pytest

import conditioning_ref as cr
import drive_ref as dr
import golden_util as gu
import time_ref

pytestmark = pytest.mark.gpu

DD = 0.005
SENT = -777.0
STRAIGHT = np.array([[-1.0, 0.5], [0.125, 0.5]])
ALPHA = 2.0 * 8.0 / (12.5 / 12.0)
SIZES = (257, 1024)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator as G
    return torch, {"f64": G(0, "f64"), "f32": G(0, "f32"), "f32r32": G(0, "f32", recurrence="f32"),
                   "literal": G(0, "f64", velocity_kernel="seq_literal")}


def cons():
    return tuple(float(x) for x in gu.load("plain_w8_s0")["constraints"])


def waypoints(name):
    """fp64 waypoints that fp32 holds exactly, so that generators of both types profile the same path."""
    wp = STRAIGHT if name == "straight" else gu.load(name)["waypoints"]
    return np.asarray(wp, dtype=np.float32).astype(np.float64)


def straight8():
    t = np.linspace(0.0, 1.0, 8)[:, None]
    return ((1 - t) * np.array([[-1.0, 0.5]]) + t * np.array([[0.75, 0.5]])).astype(np.float32).astype(np.float64)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def profile(env, key, wps, S, **kw):
    torch, gens = env
    gen = gens[key]
    wp = torch.tensor(np.asarray(wps), dtype=gen.tdtype, device=gen.device)
    return gen, gen.profile(wp, cons(), dd=DD, capacity=S, **kw)


_rows = {}


def three_paths(env, key, S):
    """(kappa (3, S) in the generator's type, meta (3, 4)) of the three paths, one profile call each."""
    if (key, S) not in _rows:
        torch, _ = env
        kap, meta = [], []
        for name in ("plain_w5_s0", "plain_w8_s0", "straight"):
            _, r = profile(env, key, waypoints(name)[None], S)
            torch.cuda.synchronize()
            kap.append(r["curvature"][0].cpu().numpy())
            meta.append(r["meta"][0].cpu().numpy())
        _rows[(key, S)] = (np.stack(kap), np.stack(meta))
    return _rows[(key, S)]


def offset_tensor(torch, a, dev, shift_bytes=0):
    """``a`` on the device at an address ``shift_bytes`` past an aligned one."""
    a = np.ascontiguousarray(a)
    n = shift_bytes // a.dtype.itemsize
    flat = torch.empty(a.size + n, dtype=torch.float64 if a.dtype == np.float64 else torch.float32, device=dev)
    t = flat[n:].view(a.shape)
    t.copy_(torch.as_tensor(a))
    assert t.data_ptr() % 16 == shift_bytes % 16
    return t


def ref_caps(kap64, meta, A, alpha, vin, out_dtype):
    outs, nbs = [], []
    for b in range(len(kap64)):
        o, nb = dr.caps(kap64[b], meta[b, 3], meta[b, 2], cons()[0], A, alpha, None if vin is None else vin[b], out_dtype)
        outs.append(o)
        nbs.append(nb)
    return np.stack(outs), np.array(nbs, dtype=np.int32)


def incoming(shape, dtype):
    """An incoming row with structure: a running limit that changes, a 0.01 stop, a stretch above max_vel."""
    rng = np.random.default_rng(3)
    v = np.full(shape, 4.0)
    v[:, 40:90] = 2.5
    v[:, 120] = 0.01
    v[:, 150:170] = 4.5
    v[:, 200:] = rng.uniform(0.5, 4.0, size=v[:, 200:].shape)
    return v.astype(dtype)


# ---------------------------------------------------------------- vap_curve_caps

@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("key", ["f64", "f32r32"])
def test_caps_on_caller_rows_bit_for_bit(env, key, S):
    torch, gens = env
    from vexautonomousplanner_amd import drive
    gen = gens[key]
    kap, meta = three_paths(env, key, S)
    N = meta[:, 3].astype(int)
    assert (N < S).any() and (N >= 2).all() and np.abs(kap[2, :N[2]]).max() < 1e-9 and N[2] < 257
    rdt = np.float64 if key == "f64" else np.float32
    k64 = kap.astype(np.float64)
    dev = gen.device
    d_kap, d_meta = offset_tensor(torch, kap, dev), torch.tensor(meta, device=dev)
    for A, alpha in ((3.0, math.inf), (6.0, ALPHA), (math.inf, ALPHA), (25.7, math.inf)):
        caps = drive.CurveCaps(A, alpha)
        # no incoming row: max_vel everywhere
        out = offset_tensor(torch, np.full((3, S), SENT, dtype=rdt), dev)
        nb = torch.full((3, 2), -5, dtype=torch.int32, device=dev)
        got, gnb = drive.curve_caps(d_meta, d_kap, caps, cons(), vcap_out=out, n_bound=nb, ctx=gen.ctx)
        torch.cuda.synchronize()
        assert got is out and gnb is nb
        want, wnb = ref_caps(k64, meta, A, alpha, None, rdt)
        assert same(out.cpu().numpy(), want), (key, S, A, alpha)
        assert np.array_equal(nb.cpu().numpy(), wnb), (key, S, A, alpha, nb.cpu().numpy(), wnb)
        for b in range(3):
            assert (want[b, N[b]:] == rdt(cons()[0])).all()
        if A == 3.0:
            assert wnb[0, 0] > 0 and wnb[1, 0] > 0 and wnb[2].tolist() == [0, 0]
        if alpha == ALPHA:
            assert wnb[0, 1] > 0 and wnb[1, 1] > 0
        # in place on an incoming row, then the same from addresses 8 bytes off the 16-byte grid (rows and curvature)
        vin = incoming((3, S), rdt)
        want, wnb = ref_caps(k64, meta, A, alpha, vin, rdt)
        for shift in (0, 8):
            row = offset_tensor(torch, vin, dev, shift)
            kk = offset_tensor(torch, kap, dev, shift)
            got, gnb = drive.curve_caps(d_meta, kk, caps, cons(), vcap_in=row, vcap_out=row, ctx=gen.ctx)
            torch.cuda.synchronize()
            assert got is row and same(row.cpu().numpy(), want), (key, S, A, alpha, "in place", shift)
            assert np.array_equal(gnb.cpu().numpy(), wnb), (key, S, A, alpha, "in place", shift)
            for b in range(3):
                assert same(want[b, N[b]:], vin[b, N[b]:])
    # a NaN curvature gives a NaN cap and does not count
    bad = kap.copy()
    bad[1, 17] = np.nan
    got, gnb = drive.curve_caps(d_meta, offset_tensor(torch, bad, dev), drive.CurveCaps(3.0, ALPHA), cons(), ctx=gen.ctx)
    torch.cuda.synchronize()
    want, wnb = ref_caps(bad.astype(np.float64), meta, 3.0, ALPHA, None, rdt)
    assert np.isnan(want[1, 17]) and same(got.cpu().numpy(), want) and np.array_equal(gnb.cpu().numpy(), wnb)


def context_case(env, wps, S):
    """The fp32 generator's profile of ``wps`` (B, W, 2) and the fp64 curvature rows of the same paths."""
    torch, gens = env
    _, r64 = profile(env, "f64", wps, S)
    torch.cuda.synchronize()
    k64 = r64["curvature"].cpu().numpy()
    gen, r = profile(env, "f32", wps, S)
    torch.cuda.synchronize()
    assert same(k64.astype(np.float32), r["curvature"].cpu().numpy()), "the fp64 generator's curvature is not the row behind the fp32 one"
    return gen, r, k64


@pytest.mark.parametrize("S", SIZES)
def test_caps_from_the_context_rows_bit_for_bit(env, S):
    """fp32 rows in the default mode, d_curvature NULL: fp64 cap rows from the fp64 curvature the sampling call kept."""
    torch, gens = env
    from vexautonomousplanner_amd import drive
    batches = [waypoints(n)[None] for n in ("plain_w5_s0", "plain_w8_s0", "straight")]
    batches.append(np.stack([waypoints("plain_w8_s0"), waypoints("plain_w8_s1"), straight8()]))
    bound = 0
    for wps in batches:
        gen, r, k64 = context_case(env, wps, S)
        meta = r["meta"].cpu().numpy()
        B = len(wps)
        for A, alpha in ((3.0, math.inf), (6.0, ALPHA)):
            out = torch.full((B, S), SENT, dtype=torch.float64, device=gen.device)
            got, nb = drive.curve_caps(r["meta"], None, drive.CurveCaps(A, alpha), cons(), samples=S, dtype="f32", vcap_out=out, ctx=gen.ctx)
            torch.cuda.synchronize()
            want, wnb = ref_caps(k64, meta, A, alpha, None, np.float64)
            assert same(out.cpu().numpy(), want), (B, S, A, alpha)
            assert np.array_equal(nb.cpu().numpy(), wnb), (B, S, A, alpha, nb.cpu().numpy(), wnb)
            bound += int(wnb.sum())
    assert bound > 0
    # without such rows the NULL is refused: the all-fp32 recurrence keeps none
    g32 = gens["f32r32"]
    _, r = profile(env, "f32r32", batches[0], S)
    with pytest.raises(Exception, match="rows"):
        drive.curve_caps(r["meta"], None, drive.CurveCaps(3.0), cons(), samples=S, dtype="f32", ctx=g32.ctx)
    torch.cuda.synchronize()


def test_caps_behind_node_limits_with_a_stop(env):
    """apply_node_limits (a stop node, a max_velocity node, a max_acceleration node) then apply_curve_caps: the cap row is the
    replica's on the node row, and the literal kernel's velocity is the replica's sweep on both, the acceleration rows passed
    on — bit for bit."""
    torch, gens = env
    gen = gens["literal"]
    S = 1024
    wps = np.stack([waypoints("plain_w8_s0"), waypoints("plain_w8_s1")])
    _, r = profile(env, "literal", wps, S)
    stop = np.zeros((2, 8), dtype=bool)
    stop[:, 3] = True
    mv, ma = np.zeros((2, 8)), np.zeros((2, 8))
    mv[:, 5], ma[:, 2] = 2.5, 5.0
    gen.apply_node_limits(r, cons(), node_max_velocity=mv, node_stop=stop, node_max_acceleration=ma)
    node_row = r["vcap"]
    v_node = r["velocity"].clone()
    from vexautonomousplanner_amd import drive
    gen.apply_curve_caps(r, drive.CurveCaps(3.0), cons())
    torch.cuda.synchronize()
    assert r["vcap"] is not node_row
    vin, meta, kap = node_row.cpu().numpy(), r["meta"].cpu().numpy(), r["curvature"].cpu().numpy()
    assert (vin == 0.01).any() and (vin == 2.5).any()
    want, wnb = ref_caps(kap, meta, 3.0, math.inf, vin, np.float64)
    assert same(r["vcap"].cpu().numpy(), want) and np.array_equal(r["n_bound"].cpu().numpy(), wnb) and (wnb[:, 0] > 0).all()
    af, ab, db = (r[k].cpu().numpy() for k in ("acc_forward", "acc_backward", "dec_backward"))
    vel, head = r["velocity"].cpu().numpy(), r["heading"].cpu().numpy()
    for b in range(2):
        N = int(meta[b, 3])
        U = cr.sweep(kap[b], cr.dtheta(head[b, :N]), N, meta[b, 2], cons(), 0.01, 0.01, vcap=want[b], acc_fwd=af[b], acc_bwd=ab[b], dec=db[b])
        assert same(vel[b, :N], np.sqrt(np.array(U))), b
    assert not torch.equal(v_node, r["velocity"])
    # a second call starts from the node row again, not from its own result
    gen.apply_curve_caps(r, drive.CurveCaps(3.0), cons())
    torch.cuda.synchronize()
    assert same(r["vcap"].cpu().numpy(), want) and same(r["velocity"].cpu().numpy(), vel)


# ---------------------------------------------------------------- velocity under caps

W8 = ("plain_w8_s0", "plain_w8_s1")


def w8_batch():
    return np.stack([waypoints(W8[0]), waypoints(W8[1]), straight8()])


_replica = {}


def replica_w8(env, A, alpha=math.inf):
    """The literal generator's rows of the W = 8 batch and the replica's velocity under the caps (computed once)."""
    torch, gens = env
    if "rows" not in _replica:
        _, r = profile(env, "literal", w8_batch(), 1024)
        torch.cuda.synchronize()
        _replica["rows"] = {k: r[k].cpu().numpy() for k in ("curvature", "heading", "meta", "velocity")}
    rows = _replica["rows"]
    if (A, alpha) not in _replica:
        vel, nbs = np.zeros_like(rows["curvature"]), []
        for b in range(3):
            N = int(rows["meta"][b, 3])
            vcap, nb = (None, [0, 0]) if A == alpha == math.inf else dr.caps(rows["curvature"][b], N, rows["meta"][b, 2], cons()[0], A, alpha)
            U = cr.sweep(rows["curvature"][b], cr.dtheta(rows["heading"][b, :N]), N, rows["meta"][b, 2], cons(), 0.01, 0.01, vcap=vcap)
            vel[b, :N] = np.sqrt(np.array(U))
            nbs.append(nb)
        _replica[(A, alpha)] = (vel, np.array(nbs))
    return rows, _replica[(A, alpha)]


@pytest.mark.parametrize("A,alpha", [(3.0, math.inf), (6.0, math.inf), (math.inf, ALPHA)])
def test_literal_velocity_under_caps_is_the_replica_sweep(env, A, alpha):
    torch, gens = env
    from vexautonomousplanner_amd import drive
    rows, (want, wnb) = replica_w8(env, A, alpha)
    gen, r = profile(env, "literal", w8_batch(), 1024)
    gen.apply_curve_caps(r, drive.CurveCaps(A, alpha), cons())
    torch.cuda.synchronize()
    vel, kap = r["velocity"].cpu().numpy(), rows["curvature"]
    for b in range(3):
        N = int(rows["meta"][b, 3])
        assert same(vel[b, :N], want[b, :N]), (A, alpha, b)
        vel[b, N:] = 0.0
    nb = r["n_bound"].cpu().numpy()
    assert np.array_equal(nb, wnb)
    if A != math.inf:
        lat = np.max(vel[:, 1:] ** 2 * np.abs(kap[:, 1:]), axis=1)
        print(f"DRIVE A={A}: max v^2|k| / A - 1 = {lat[:2] / A - 1}, n_bound {nb.tolist()}")
        assert (nb[:2, 0] > 0).all()


@pytest.mark.parametrize("A", [3.0, 6.0])
def test_lateral_property_holds_on_fp64_rows(env, A):
    """v^2 |k| <= A (1 + 4 * 2^-52) on samples 1 .. N - 1 — in u = v^2, the quantity the pass limits (the stored velocity is
    its rounded root, whose square may lie one more ulp up)."""
    torch, gens = env
    from vexautonomousplanner_amd import drive
    for key in ("literal", "f64"):
        gen, r = profile(env, key, w8_batch(), 1024)
        gen.apply_curve_caps(r, drive.CurveCaps(A), cons())
        torch.cuda.synchronize()
        vel, kap, nb = r["velocity"].cpu().numpy(), r["curvature"].cpu().numpy(), r["n_bound"].cpu().numpy()
        assert (nb[:2, 0] > 0).all() and nb[2, 0] == 0
        for b, n in enumerate(r["meta"][:, 3].cpu().numpy().astype(int)):
            vel[b, n:] = 0.0
        lat = np.max(vel[:, 1:] * vel[:, 1:] * np.abs(kap[:, 1:]), axis=1)
        print(f"DRIVE {key} A={A}: max v^2|k| = A * (1 + {lat / A - 1})")
        assert (lat <= A * (1.0 + 4 * 2.0 ** -52)).all(), (key, lat / A - 1)


def test_cap_that_does_not_bind_changes_no_bit(env):
    torch, gens = env
    from vexautonomousplanner_amd import drive
    for key in ("literal", "f64", "f32", "f32r32"):
        gen, r = profile(env, key, w8_batch(), 1024)
        plain = r["velocity"].clone()
        gen.apply_curve_caps(r, drive.CurveCaps(25.7), cons())
        torch.cuda.synchronize()
        assert torch.equal(plain, r["velocity"]), key
        assert r["vcap"].shape == (3, 1024) and r["n_bound"].shape == (3, 2)


@pytest.mark.parametrize("key,tol", [("f64", 1e-7), ("f32", 1e-5)])
def test_fast_kernels_agree_under_caps(env, key, tol):
    """AUTO, LANES_16 and RELAX_BLOCK: the same bits (include/vap.h), and the replica to the bounds test_gpu_parity.py holds
    those kernels to."""
    torch, gens = env
    from vexautonomousplanner_amd import drive
    gen = gens[key]
    for A, alpha in ((3.0, math.inf), (6.0, ALPHA)):
        _, (want, _) = replica_w8(env, A, alpha)
        got = {}
        try:
            for kernel in ("auto", "lanes16", "relax_block"):
                gen.set_velocity_kernel(kernel)
                _, r = profile(env, key, w8_batch(), 1024)
                gen.apply_curve_caps(r, drive.CurveCaps(A, alpha), cons())
                torch.cuda.synchronize()
                got[kernel] = r["velocity"].cpu().numpy()
                for b, n in enumerate(r["meta"][:, 3].cpu().numpy().astype(int)):
                    got[kernel][b, n:] = 0.0
                assert not (r["flags"].cpu().numpy() & ~2).any()
        finally:
            gen.set_velocity_kernel("auto")
        assert same(got["auto"], got["lanes16"]) and same(got["auto"], got["relax_block"]), (key, A, alpha)
        ok = want > 0
        err = float(np.max(np.abs(got["auto"].astype(np.float64)[ok] - want[ok]) / want[ok]))
        print(f"DRIVE {key} A={A} alpha={alpha}: fast kernels vs replica {err:.2e}")
        assert err <= tol, (key, A, alpha, err)


# ---------------------------------------------------------------- vap_drive_audit

def ref_audit(rows, counts, T, h, limits, cap):
    B = len(rows)
    out = dict(peak=np.zeros((B, 5)), peak_row=np.zeros((B, 5), dtype=np.int32), n_over=np.zeros((B, 5), dtype=np.int32),
               first_over=np.zeros((B, 5), dtype=np.int32), status=np.zeros(B, dtype=np.int32), wheel=[])
    for b in range(B):
        a = dr.audit(rows[b, :, 2], rows[b, :, 5], counts[b], T, h, limits)
        for k in ("peak", "peak_row", "n_over", "first_over", "status"):
            out[k][b] = a[k]
        out["wheel"].append(a["wheel"])
    return out


def device_audit(env, rows, counts, T, h, limits, stride=2, ctx=None, rows_tensor=None):
    """One call with every output prefilled; numpy results.  counts (B,) go into column 0 of a (B, stride) array of -9."""
    torch, gens = env
    from vexautonomousplanner_amd import drive
    dev = gens["f64"].device
    B, cap = rows.shape[0], rows.shape[1]
    c = np.full((B, stride), -9, dtype=np.int32)
    c[:, 0] = counts
    out = {"peak": torch.full((B, 5), SENT, dtype=torch.float64, device=dev), "peak_row": torch.full((B, 5), -99, dtype=torch.int32, device=dev),
           "n_over": torch.full((B, 5), -99, dtype=torch.int32, device=dev), "first_over": torch.full((B, 5), -99, dtype=torch.int32, device=dev),
           "status": torch.full((B,), -99, dtype=torch.int32, device=dev),
           "wheel_rows": torch.full((B, cap, 8), SENT, dtype=torch.float64, device=dev)}
    d_rows = rows_tensor if rows_tensor is not None else torch.tensor(rows, device=dev)
    res = drive.audit(d_rows, torch.tensor(c, device=dev), drive.Limits(T, *limits), time_step=h, per_row=True, out=out, ctx=ctx)
    torch.cuda.synchronize()
    assert all(res[k] is out[k] for k in out)
    return {k: v.cpu().numpy() for k, v in res.items()}


def check_audit(got, want, counts, cap, what):
    assert same(got["peak"], want["peak"]), (what, got["peak"], want["peak"])
    for k in ("peak_row", "n_over", "first_over", "status"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for b, wh in enumerate(want["wheel"]):
        n = len(wh)
        assert same(got["wheel_rows"][b, :n], wh), (what, b, "wheel rows")
        assert (got["wheel_rows"][b, n:] == SENT).all(), (what, b, "written at or above n")


@pytest.mark.parametrize("dt", [0.01, 1 / 60], ids=["0.01", "1/60"])
def test_audit_of_time_profile_rows_bit_for_bit(env, dt):
    torch, gens = env
    gen, r = profile(env, "f64", w8_batch(), 1024)
    tp = gen.time_profile(r, cons(), dt=dt, capacity_rows=1000)
    torch.cuda.synchronize()
    rows, counts = tp["rows"].cpu().numpy(), tp["counts"].cpu().numpy()
    T = cons()[5]
    limits = (4.0, 8.0, 16.0, 3.0, ALPHA)
    want = ref_audit(rows, counts[:, 0], T, dt, limits, 1000)
    got = device_audit(env, rows, counts[:, 0], T, dt, limits, ctx=gen.ctx)
    check_audit(got, want, counts[:, 0], 1000, dt)
    print(f"DRIVE audit dt={dt:.4f}: counts {counts[:, 0].tolist()}, peaks {want['peak'].tolist()}, rows over {want['n_over'].tolist()}")
    assert (counts[:2, 0] > 64).all() and (want["n_over"][:2, 3] > 0).all() and (want["status"] == 0).all()
    # the generator's forwarder, the counts as time_profile left them (stride 2), the time step read from the rows
    from vexautonomousplanner_amd import drive
    fw = gen.drive_audit(tp, drive.Limits(T, *limits))
    torch.cuda.synchronize()
    assert same(fw["peak"].cpu().numpy(), want["peak"]) and "wheel_rows" not in fw


def synthetic(cap=300):
    """Routes of 0, 1, 2, 63, 64, 65 and 257 rows in rows of capacity 300 (no multiple of 64), random but finite; an in-place
    turn block (v = 0, omega != 0) in the longest; garbage (NaN) behind every route's rows."""
    rng = np.random.default_rng(11)
    ns = np.array([0, 1, 2, 63, 64, 65, 257, 200, 130], dtype=np.int32)
    rows = rng.normal(size=(len(ns), cap, 8))
    rows[:, :, 2] = np.abs(rows[:, :, 2]) * 2.0
    rows[6, 100:140, 2] = 0.0
    rows[6, 100:140, 5] = 1.5
    rows[8, 30:50, 2:6] = rows[8, 29, 2:6]                         # a constant stretch: ties between equal rows
    for b, n in enumerate(ns):
        rows[b, n:] = np.nan
    return rows, ns


@pytest.mark.parametrize("stride", [2, 3])
def test_audit_of_caller_rows_bit_for_bit(env, stride):
    rows, ns = synthetic()
    T, h = 1.1, 0.02
    limits = (3.0, 100.0, 5000.0, 2.0, 60.0)
    want = ref_audit(rows, ns, T, h, limits, rows.shape[1])
    got = device_audit(env, rows, ns, T, h, limits, stride=stride)
    check_audit(got, want, ns, rows.shape[1], stride)
    assert np.isnan(want["peak"][0]).all() and want["peak_row"][0].tolist() == [-1] * 5 and (want["n_over"][1:] > 0).any()
    assert want["peak"][6, 0] > 0 and (want["status"] == 0).all()
    # a NaN omega inside route 7: status bit 1, an empty route; its neighbours as before
    bad = rows.copy()
    bad[7, 150, 5] = np.nan
    want_bad = ref_audit(bad, ns, T, h, limits, rows.shape[1])
    got_bad = device_audit(env, bad, ns, T, h, limits, stride=stride)
    check_audit(got_bad, want_bad, ns, rows.shape[1], (stride, "nan"))
    assert got_bad["status"].tolist() == [0] * 7 + [2, 0] and np.isnan(got_bad["peak"][7]).all() and (got_bad["peak_row"][7] == -1).all()
    assert (got_bad["wheel_rows"][7] == SENT).all()
    for k in ("peak", "peak_row", "n_over", "first_over"):
        assert same(np.delete(got_bad[k], 7, axis=0), np.delete(got[k], 7, axis=0)), k
    # counts outside [0, capacity] are clamped; limits of +inf never count; two calls give the same bits
    big = ns.copy()
    big[5], big[0] = 100000, -4
    full = np.nan_to_num(rows, nan=0.25)
    want_c = ref_audit(full, np.clip(big, 0, rows.shape[1]), T, h, [math.inf] * 5, rows.shape[1])
    got_c = device_audit(env, full, big, T, h, [math.inf] * 5, stride=stride)
    check_audit(got_c, want_c, big, rows.shape[1], (stride, "clamp"))
    assert not got_c["n_over"].any() and (got_c["first_over"] == -1).all()
    again = device_audit(env, full, big, T, h, [math.inf] * 5, stride=stride)
    assert all(same(got_c[k], again[k]) for k in got_c)


def test_audit_tiling_does_not_change_a_bit(env):
    """One route of 5000 rows beside short ones (one 256-row step per tile), and 1200 routes (four steps per tile): both
    against the replica, and the long route's result the same inside either batch."""
    rng = np.random.default_rng(12)
    cap = 5000
    rows = rng.normal(size=(3, cap, 8))
    rows[0, 1000:1300, 2:6] = rows[0, 999, 2:6]
    ns = np.array([cap, 700, 4097], dtype=np.int32)
    T, h, limits = 0.9, 0.01, (2.0, 300.0, 30000.0, 1.0, 200.0)
    want = ref_audit(rows, ns, T, h, limits, cap)
    got = device_audit(env, rows, ns, T, h, limits)
    check_audit(got, want, ns, cap, "long")
    many = np.tile(rows[:, :1100], (400, 1, 1))
    ns_many = np.tile(np.array([1100, 700, 1025], dtype=np.int32), 400)
    got_many = device_audit(env, many, ns_many, T, h, limits)
    want_many = ref_audit(many[:3], ns_many[:3], T, h, limits, 1100)
    for k in ("peak", "peak_row", "n_over", "first_over", "status"):
        assert same(got_many[k][:3], want_many[k]) and same(got_many[k][-3:], want_many[k]), k
    assert same(got_many["wheel_rows"][1197, :1100], want_many["wheel"][0])


def test_audit_refusals_and_the_empty_batch(env):
    torch, gens = env
    from vexautonomousplanner_amd import _lib, drive
    dev = gens["f64"].device
    lim = drive.Limits(1.0)
    flat = torch.zeros(2 * 16 * 8 + 1, dtype=torch.float64, device=dev)
    off = flat[1:].view(2, 16, 8)
    assert off.data_ptr() % 16 == 8
    counts = torch.full((2, 2), 16, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.VapError, match="aligned"):
        drive.audit(off, counts, lim, time_step=0.01)
    res = drive.audit(torch.zeros((0, 16, 8), dtype=torch.float64, device=dev), torch.zeros((0, 2), dtype=torch.int32, device=dev), lim,
                      time_step=0.01, per_row=True)
    torch.cuda.synchronize()
    assert res["peak"].shape == (0, 5) and res["wheel_rows"].shape == (0, 16, 8)
    single = drive.audit(np.zeros((5, 8)), None, lim, time_step=0.01)
    torch.cuda.synchronize()
    assert single["peak"].shape == (5,) and single["peak"].tolist() == [0.0] * 5 and single["peak_row"].tolist() == [0] * 5


# ---------------------------------------------------------------- the chain and the search

def test_chain_profile_caps_time_profile_audit(env):
    torch, gens = env
    from vexautonomousplanner_amd import drive
    A, dt, cap = 3.0, 0.01, 1400
    gen, r = profile(env, "f64", w8_batch(), 1024)
    tp0 = gen.time_profile(r, cons(), dt=dt, capacity_rows=cap)
    n0 = tp0["counts"][:, 0].cpu().numpy().copy()
    gen.apply_curve_caps(r, drive.CurveCaps(A), cons())
    tp = gen.time_profile(r, cons(), dt=dt, capacity_rows=cap)
    lim = drive.Limits.from_constraints(cons())
    lim.lateral_acc_max = A
    got = gen.drive_audit(tp, lim, time_step=dt, per_row=True)
    torch.cuda.synchronize()
    rows, counts = tp["rows"].cpu().numpy(), tp["counts"][:, 0].cpu().numpy()
    vel, meta = r["velocity"].cpu().numpy(), r["meta"].cpu().numpy()
    for b in range(3):
        ref, count, truncated = time_ref.integrate(vel[b, :int(meta[b, 3])], meta[b, 1], meta[b, 2], dt, cons()[1], cons()[2], cap)
        assert count == counts[b] and not truncated and same(rows[b, :count, :4], ref[:, :4]), b
    assert (counts[:2] > n0[:2]).all() and counts[2] == n0[2]
    limits = (lim.wheel_speed_max, lim.wheel_acc_max, lim.jerk_max, lim.lateral_acc_max, lim.angular_acc_max)
    want = ref_audit(rows, counts, lim.track_width, dt, limits, cap)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert same(g["peak"], want["peak"]) and all(np.array_equal(g[k], want[k]) for k in ("peak_row", "n_over", "first_over", "status"))
    for b in range(3):
        assert same(g["wheel_rows"][b, :counts[b]], want["wheel"][b])
    print(f"DRIVE chain A={A}: rows {n0.tolist()} -> {counts.tolist()}; time-domain peaks {want['peak'].tolist()}; lateral peak / A = "
          f"{(want['peak'][:, 3] / A).tolist()}; rows over {want['n_over'].tolist()}")


def test_search_with_curve_caps(env):
    torch, gens = env
    import test_gpu_search as tgs
    from vexautonomousplanner_amd import drive, search
    gen = gens["f32"]
    cfg = search.SearchConfig(candidates=256, elites=32, iterations=3, alpha=0.7, weights=search.Weights(clearance_margin=0.05))
    plain = tgs.run(gen, tgs.SEED_A, tgs.scene_a(), cfg)
    none = tgs.run(gen, tgs.SEED_A, tgs.scene_a(), cfg, curve_caps=None)
    capped = tgs.run(gen, tgs.SEED_A, tgs.scene_a(), cfg, curve_caps=drive.CurveCaps(3.0))
    torch.cuda.synchronize()
    assert same(plain["best_cost"].cpu().numpy(), none["best_cost"].cpu().numpy())
    assert same(plain["history"].cpu().numpy(), none["history"].cpu().numpy())
    h = capped["history"].cpu().numpy()
    assert h.shape == (1, 3) and np.isfinite(h).all() and (np.diff(h, axis=1) <= 0).all()
    # the first iteration's candidates are the same under both (one seed): the caps only take time
    one = search.SearchConfig(candidates=256, elites=32, iterations=1, alpha=0.7, weights=search.Weights(clearance_margin=0.05))
    c0 = tgs.run(gen, tgs.SEED_A, tgs.scene_a(), one)["cost"].cpu().numpy()
    c1 = tgs.run(gen, tgs.SEED_A, tgs.scene_a(), one, curve_caps=drive.CurveCaps(3.0))["cost"].cpu().numpy()
    both = np.isfinite(c0) & np.isfinite(c1)
    print(f"DRIVE search: best {float(plain['best_cost'].item()):.4f} s -> {float(capped['best_cost'].item()):.4f} s under A = 3; first iteration: "
          f"{int((c1 > c0)[both].sum())} of {int(both.sum())} candidates longer")
    assert both.any() and (c1[both] > c0[both]).any()
