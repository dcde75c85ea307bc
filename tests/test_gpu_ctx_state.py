"""What a sampling or profile call leaves on a vap_ctx, and what the calls that take NULL for "the context's own" make
of it: the status code of every (producer, consumer, variant) cell, through the C-ABI ("What a call leaves on
the context" — the table below is that table).

Every refusal checked here is made on the host before any launch; no cell asks the device to refuse anything.  Cells the
library accepts without looking at a dimension (S and the dtype in the time domain, every dimension in the explicit
forms) are not run with that mismatch: they would be accepted and read rows of another shape."""
import ctypes as C

import numpy as np
import pytest

B, W, S, CAP = 3, 4, 64, 256        # the smallest shapes with an interior segment and more than one path
CAP_OUT = CAP + 64
SEED = 7
WAIT = 0.05                         # seconds at node 1: five inserted rows per path
OK, INV, UNF, UNS = "ok", "inv", "unf", "uns"

# producer -> (dtype, VAP_OPT_F32_RECURRENCE) of the context it runs on
PRODUCERS = {
    "none": ("f32", "r64"),
    "sample_f32_r64": ("f32", "r64"), "sample_f32_r32": ("f32", "r32"), "sample_f64": ("f64", "r64"),
    "batch_f32_r64": ("f32", "r64"), "batch_f32_r32": ("f32", "r32"), "batch_f64": ("f64", "r64"),
    "routes_1": ("f32", "r64"),                 # vap_profile_routes, max_splines = 1
    "routes_2": ("f32", "r64"),                 # max_splines = 2, one reverse node
    "routes_2_then_sample": ("f32", "r64"),     # the tables stay, relabelled as plain ones
    "batch_then_option_r32": ("f32", "r64"),    # vap_ctx_set_option(VAP_OPT_F32_RECURRENCE, ...) after the batch
    "batch_then_option_r64": ("f32", "r64"),
}
COLUMNS = list(PRODUCERS)

# Read off the parent's code.  One row per consumer cell, one entry per producer in the order of COLUMNS:
#                                none s32h s32l s64  b32h b32l b64  rt1  rt2  r2s  bo32 bo64
TABLE = {
    # vap_velocity_pass, d_dtheta = NULL: rows of B x S in dtype dt
    "velocity_ctx":            "inv  ok   inv  inv  ok   ok   ok   ok   ok   ok   inv  inv",
    "velocity_ctx/B+1":        "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "velocity_ctx/S+1":        "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "velocity_ctx/dtype":      "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    # vap_velocity_pass_limits, fp32 caller rows + d_vcap: refused under VAP_RECURRENCE_F64 whatever the context holds
    "velocity_limits_f32rows": "inv  inv  ok   inv  inv  ok   inv  inv  inv  inv  ok   inv",
    # vap_route_limits: grid of B x W x S; d_lut NULL: tables of B x W; d_lut given: refused for a batch of routes
    "limits_ctx":              "inv  inv  inv  inv  ok   ok   ok   ok   ok   ok   ok   ok",
    "limits_ctx/B+1":          "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "limits_ctx/W+1":          "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "limits_ctx/S+1":          "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "limits_lut":              "inv  ok   ok   ok   ok   ok   ok   inv  inv  ok   ok   ok",
    "limits_lut/B+1":          "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "limits_lut/W+1":          "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "limits_lut/S+1":          "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    # vap_time_profile / vap_time_insert_waits: tables of B x W, plain paths only (max_splines = 1 counts as routes)
    "time_ctx":                "unf  unf  unf  unf  ok   ok   ok   uns  uns  ok   ok   ok",
    "time_ctx/B+1":            "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "time_ctx/W+1":            "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "time_explicit":           "ok   ok   ok   ok   ok   ok   ok   ok   ok   ok   ok   ok",
    "time_seg_only":           "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "time_lut_only":           "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "waits_ctx":               "unf  unf  unf  unf  ok   ok   ok   uns  uns  ok   ok   ok",
    "waits_ctx/B+1":           "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "waits_ctx/W+1":           "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "waits_explicit":          "ok   ok   ok   ok   ok   ok   ok   ok   ok   ok   ok   ok",
    "waits_seg_only":          "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    "waits_lut_only":          "inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv  inv",
    # vap_time_profile_routes / vap_time_insert_events / vap_closest_points: tables of B x W, plain or routes
    "time_routes":             "unf  unf  unf  unf  ok   ok   ok   ok   ok   ok   ok   ok",
    "time_routes/B+1":         "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "time_routes/W+1":         "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "events":                  "unf  unf  unf  unf  ok   ok   ok   ok   ok   ok   ok   ok",
    "events/B+1":              "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "events/W+1":              "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "closest":                 "unf  unf  unf  unf  ok   ok   ok   ok   ok   ok   ok   ok",
    "closest/B+1":             "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
    "closest/W+1":             "unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf  unf",
}
# context form == explicit form, byte for byte, where the context holds the plain tables of this very batch
EQUAL_PAIRS = (("time_ctx", "time_explicit"), ("waits_ctx", "waits_explicit"), ("limits_ctx", "limits_lut"))
EQUAL_ON = ("batch_f32_r64", "batch_f32_r32", "batch_f64", "batch_then_option_r32", "batch_then_option_r64")
# after vap_profile_routes(2) + vap_sample the context-form calls run on a route's tables read as plain ones: accepted
# (that is the entry of the table), but what they compute is not a path's, so their flags are not looked at
MISLABELLED = "routes_2_then_sample"


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Env:
    """The library, the constraints, and one reference batch per (dtype, recurrence): the fused call's rows, the staged
    tables and the time rows of B x W x S, computed once on a context of their own and never written again."""

    def __init__(self, torch):
        from vexautonomousplanner_amd import _lib
        from vexautonomousplanner_amd.synth import DEFAULT_CONSTRAINTS
        self.torch, self.lib, self.L = torch, _lib, _lib.lib()
        self.dev = torch.device("cuda:0")
        self.c = _lib.make_constraints(DEFAULT_CONSTRAINTS)
        self.code = {OK: _lib.VAP_OK, INV: _lib.VAP_ERR_INVALID, UNF: _lib.VAP_ERR_UNFITTED, UNS: _lib.VAP_ERR_UNSUPPORTED}
        self.name = {v: k for k, v in self.code.items()}
        self.refs = {}

    def context(self, rec):
        ctx = self.lib.Context(0)
        ctx.set_stream(self.torch.cuda.current_stream(self.dev).cuda_stream)
        if rec == "r32":
            ctx.set_option(self.lib.OPT_F32_RECURRENCE, self.lib.RECURRENCE_F32)
        return ctx

    def vdt(self, dtype):
        return self.lib.VAP_F64 if dtype == "f64" else self.lib.VAP_F32

    def tdt(self, dtype):
        return self.torch.float64 if dtype == "f64" else self.torch.float32

    def z(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device=self.dev)

    def waypoints(self, dtype):
        from vexautonomousplanner_amd.synth import make_waypoints
        return self.torch.tensor(make_waypoints(B, W, SEED, np.float64 if dtype == "f64" else np.float32), device=self.dev)

    def profile_batch(self, ctx, dtype):
        t, f64 = self.torch, self.torch.float64
        o = {k: self.z((B, S), self.tdt(dtype)) for k in ("x", "y", "heading", "curv", "vel")}
        o["meta"], o["flags"], o["wp"] = self.z((B, 4), f64), self.z((B,), t.int32), self.waypoints(dtype)
        st = self.L.vap_profile_batch(ctx.handle, self.vdt(dtype), B, W, S, 0.0, p(o["wp"]), C.byref(self.c), 0.01, 0.01, p(o["x"]),
                                      p(o["y"]), p(o["heading"]), p(o["curv"]), p(o["vel"]), p(o["meta"]), p(o["flags"]))
        assert st == self.lib.VAP_OK, self.L.vap_last_error()
        return o

    def profile_routes(self, ctx, dtype, max_splines):
        t, f64 = self.torch, self.torch.float64
        o = {k: self.z((B, S), self.tdt(dtype)) for k in ("x", "y", "heading", "curv", "vel")}
        o["meta"], o["flags"], o["wp"] = self.z((B, 4), f64), self.z((B,), t.int32), self.waypoints(dtype)
        o["rev"] = self.z((B, W), t.int32)
        if max_splines > 1:
            o["rev"][0, 1] = 1
        st = self.L.vap_profile_routes(ctx.handle, self.vdt(dtype), B, W, S, 0.0, max_splines, p(o["wp"]), p(o["rev"]), None, None,
                                       None, C.byref(self.c), 0.01, 0.01, p(o["x"]), p(o["y"]), p(o["heading"]), p(o["curv"]),
                                       p(o["vel"]), p(o["meta"]), p(o["flags"]), None)
        assert st == self.lib.VAP_OK, self.L.vap_last_error()
        return o

    def sample(self, ctx, dtype, ref):
        o = {k: self.z((B, S), self.tdt(dtype)) for k in ("x", "y", "heading", "curv", "dth")}
        o["meta"], o["flags"] = ref["meta_staged"].clone(), self.z((B,), self.torch.int32)
        st = self.L.vap_sample(ctx.handle, self.vdt(dtype), B, W, S, 0.0, p(ref["seg"]), p(ref["lut"]), p(o["meta"]), p(o["x"]),
                               p(o["y"]), p(o["heading"]), p(o["curv"]), p(o["dth"]), p(o["flags"]))
        assert st == self.lib.VAP_OK, self.L.vap_last_error()
        return o

    def ref(self, dtype, rec):
        key = (dtype, rec)
        if key in self.refs:
            return self.refs[key]
        t, f64, L = self.torch, self.torch.float64, self.L
        ctx = self.context(rec)
        r = self.profile_batch(ctx, dtype)
        r["ctx"] = ctx
        r["seg"], r["lut"] = self.z((B, W - 1, 6, 2), f64), self.z((B, self.lib.LUT_SAMPLES), f64)
        r["meta_staged"] = self.z((B, 4), f64)
        assert L.vap_fit(ctx.handle, self.vdt(dtype), B, W, p(r["wp"]), None, None, p(r["seg"]), None, p(r["meta_staged"]),
                         p(r["flags"])) == 0, L.vap_last_error()
        assert L.vap_build_lut(ctx.handle, B, W, p(r["seg"]), p(r["lut"]), p(r["meta_staged"]), p(r["flags"])) == 0, L.vap_last_error()
        r["rows"], r["counts"], r["nmap"] = self.z((B, CAP, 8), f64), self.z((B, 2), t.int32), self.z((B, W), t.int32)
        assert L.vap_time_profile(ctx.handle, self.vdt(dtype), B, W, S, p(r["seg"]), p(r["lut"]), p(r["meta"]), p(r["vel"]),
                                  C.byref(self.c), 0.01, CAP, p(r["rows"]), p(r["counts"]), p(r["nmap"]), p(r["flags"])) == 0
        ctx.synchronize()
        assert int(r["flags"].abs().sum().item()) == 0
        assert int(r["counts"][:, 0].min().item()) > 10 and int(r["counts"][:, 0].max().item()) < CAP
        self.refs[key] = r
        return r


@pytest.fixture(scope="module")
def env(torch_mod):
    return Env(torch_mod)


def produce(env, name):
    """A fresh context after producer `name`, and the rows the consumers are given: the producer's own where it made a
    whole plain-equivalent batch, the reference batch's otherwise."""
    dtype, rec = PRODUCERS[name]
    ref = env.ref(dtype, rec)
    ctx = env.context(rec)
    own = None
    if name.startswith("sample"):
        env.sample(ctx, dtype, ref)
    elif name.startswith("batch"):
        own = env.profile_batch(ctx, dtype)
        if name.endswith("option_r32"):
            ctx.set_option(env.lib.OPT_F32_RECURRENCE, env.lib.RECURRENCE_F32)
        elif name.endswith("option_r64"):
            ctx.set_option(env.lib.OPT_F32_RECURRENCE, env.lib.RECURRENCE_F64)
    elif name == "routes_1":
        own = env.profile_routes(ctx, dtype, 1)
    elif name.startswith("routes_2"):
        own = env.profile_routes(ctx, dtype, 2)
        if name == MISLABELLED:
            env.sample(ctx, dtype, ref)
            own = None
    ctx.synchronize()
    if own is not None:
        assert int(own["flags"].abs().sum().item()) == 0
    return ctx, ref, own


def run_cells(env, name, ctx, ref, own):
    """Every consumer cell once on `ctx`: {cell: status name}, {cell: bytes of what an accepted call wrote}."""
    t, L, lib, c = env.torch, env.L, env.lib, env.c
    f64, i32 = t.float64, t.int32
    dtype, _ = PRODUCERS[name]
    vdt, other = env.vdt(dtype), env.vdt("f32" if dtype == "f64" else "f64")
    rows_of = own if own is not None else ref                      # rows that go with the tables on the context
    plain = ref if name == "routes_2" else rows_of                 # rows that go with the reference's plain tables
    rev = own.get("rev") if own is not None else None
    # outputs, sized for every mismatch shape; zeroed before each call
    o_vel = env.z((B + 1) * (S + 1), f64)
    o_lim = env.z((B + 1) * (S + 1), f64)
    o_rows, o_counts, o_nmap = env.z((B + 1, CAP_OUT, 8), f64), env.z((B + 1, 3), i32), env.z((B + 1, W + 1), i32)
    o_close = [env.z((B + 1, 2, 2), f64) for _ in range(5)]
    flags = env.z((B + 1,), i32)
    outs = [o_vel, o_lim, o_rows, o_counts, o_nmap, flags] + o_close
    wait = env.z((B, W), f64)
    wait[:, 1] = WAIT
    ap_t, ap_w, o_amap = t.full((B + 1, 1), float("inf"), dtype=f64, device=env.dev), env.z((B + 1, 1), f64), env.z((B + 1, 1), i32)
    queries = t.tensor([[-5.0, -5.0], [-4.0, -4.5]], dtype=f64, device=env.dev)
    f32_rows = {"curv": ref["curv"] if dtype == "f32" else env.z((B, S), t.float32), "dth": env.z((B, S), t.float32),
                "vcap": t.full((B, S), c.max_vel, dtype=t.float32, device=env.dev)}
    got, data = {}, {}

    def cell(cell_name, call, wrote=()):
        for b in outs:
            b.zero_()
        st = call()
        got[cell_name] = env.name.get(st, st)
        assert L.vap_ctx_synchronize(ctx.handle) == lib.VAP_OK, (cell_name, L.vap_last_error())   # nothing sticky
        if st == lib.VAP_OK:
            if name != MISLABELLED or cell_name.endswith("explicit") or cell_name.startswith("velocity"):
                assert int(flags.abs().sum().item()) == 0, (name, cell_name, flags.tolist())
            data[cell_name] = b"".join(w.cpu().numpy().tobytes() for w in wrote)

    def shapes(base, dims):
        yield base, B, W, S
        if "B" in dims:
            yield base + "/B+1", B + 1, W, S
        if "W" in dims:
            yield base + "/W+1", B, W + 1, S
        if "S" in dims:
            yield base + "/S+1", B, W, S + 1

    # time domain first: the residual row of the producer's velocity pass is still the context's
    def time_profile(b, w, seg, lut, src):
        return lambda: L.vap_time_profile(ctx.handle, vdt, b, w, S, p(seg), p(lut), p(src["meta"]), p(src["vel"]), C.byref(c), 0.01,
                                          CAP, p(o_rows), p(o_counts), p(o_nmap), p(flags))
    for cn, b, w, _ in shapes("time_ctx", "BW"):
        cell(cn, time_profile(b, w, None, None, rows_of), (o_rows, o_counts, o_nmap))
    cell("time_explicit", time_profile(B, W, ref["seg"], ref["lut"], plain), (o_rows, o_counts, o_nmap))
    cell("time_seg_only", time_profile(B, W, ref["seg"], None, plain))
    cell("time_lut_only", time_profile(B, W, None, ref["lut"], plain))

    def waits(b, w, seg, lut, src):
        return lambda: L.vap_time_insert_waits(ctx.handle, b, w, 0, CAP, CAP_OUT, 0.01, p(seg), p(lut), p(src["meta"]), p(ref["rows"]),
                                               p(ref["counts"]), p(ref["nmap"]), p(wait), p(ap_t), p(ap_w), p(o_rows), p(o_counts),
                                               p(o_nmap), p(o_amap), p(flags))
    for cn, b, w, _ in shapes("waits_ctx", "BW"):
        cell(cn, waits(b, w, None, None, rows_of), (o_rows, o_counts, o_nmap))
    cell("waits_explicit", waits(B, W, ref["seg"], ref["lut"], plain), (o_rows, o_counts, o_nmap))
    cell("waits_seg_only", waits(B, W, ref["seg"], None, plain))
    cell("waits_lut_only", waits(B, W, None, ref["lut"], plain))

    rt_rows = {"rows": ref["rows"], "counts": ref["counts"], "nmap": ref["nmap"]}
    for cn, b, w, _ in shapes("time_routes", "BW"):
        cell(cn, lambda: L.vap_time_profile_routes(ctx.handle, vdt, b, w, S, p(rows_of["meta"]), p(rows_of["vel"]), C.byref(c), 0.01,
                                                   CAP, p(rev), p(o_rows), p(o_counts), p(o_nmap), p(flags)))
        if cn == "time_routes" and got[cn] == OK:      # the rows the events go into: this batch's own
            rt_rows = {"rows": o_rows.flatten()[:B * CAP * 8].clone(), "counts": o_counts.flatten()[:B * 2].clone(),
                       "nmap": o_nmap.flatten()[:B * W].clone()}
    for cn, b, w, _ in shapes("events", "BW"):
        cell(cn, lambda: L.vap_time_insert_events(ctx.handle, b, w, 0, CAP, CAP_OUT, 0.01, C.byref(c), p(rows_of["meta"]),
                                                  p(rt_rows["rows"]), p(rt_rows["counts"]), p(rt_rows["nmap"]), p(wait), None,
                                                  p(rev), p(ap_t), p(ap_w), p(o_rows), p(o_counts), p(o_nmap), p(o_amap), p(flags)))
    for cn, b, w, _ in shapes("closest", "BW"):
        cell(cn, lambda: L.vap_closest_points(ctx.handle, b, w, 2, lib.CLOSEST_GUI, 1, p(queries), p(o_close[0]), p(o_close[1]),
                                              p(o_close[2]), p(o_close[3]), p(o_close[4]), p(flags)), o_close)

    def limits(b, w, s, lut):
        return lambda: L.vap_route_limits(ctx.handle, vdt, b, w, 0, s, p(lut), p(rows_of["meta"]), None, None, None, None, None, None,
                                          None, C.byref(c), 0.01, p(o_lim), None, None, None, None, None)
    for cn, b, w, s in shapes("limits_ctx", "BWS"):
        cell(cn, limits(b, w, s, None), (o_lim,))
    for cn, b, w, s in shapes("limits_lut", "BWS"):
        cell(cn, limits(b, w, s, ref["lut"]), (o_lim,))

    def velocity(dt, b, s):
        return lambda: L.vap_velocity_pass(ctx.handle, dt, b, s, C.byref(c), 0.01, 0.01, p(rows_of["meta"]), p(rows_of["curv"]), None,
                                           None, p(o_vel), p(flags))
    cell("velocity_limits_f32rows",
         lambda: L.vap_velocity_pass_limits(ctx.handle, lib.VAP_F32, B, S, C.byref(c), 0.01, 0.01, p(ref["meta"]), p(f32_rows["curv"]),
                                            p(f32_rows["dth"]), p(f32_rows["vcap"]), None, None, None, p(o_vel), p(flags)))
    for cn, b, _, s in shapes("velocity_ctx", "BS"):
        cell(cn, velocity(vdt, b, s), (o_vel,))
    cell("velocity_ctx/dtype", velocity(other, B, S))
    return got, data


@pytest.mark.gpu
@pytest.mark.parametrize("producer", COLUMNS)
def test_status_of_every_consumer_after(env, producer):
    """After `producer` on a fresh context every consumer cell returns the status of TABLE, accepted calls leave all flags
    zero and no call leaves an error behind; where the context holds this batch's plain tables, the context form of a
    call and its explicit form write the same bytes."""
    ctx, ref, own = produce(env, producer)
    got, data = run_cells(env, producer, ctx, ref, own)
    col = COLUMNS.index(producer)
    want = {cell: codes.split()[col] for cell, codes in TABLE.items()}
    assert set(got) == set(want)
    wrong = {cell: (got[cell], want[cell]) for cell in want if got[cell] != want[cell]}
    print(producer, got)
    assert not wrong, f"{producer}: (got, table) {wrong}"
    if producer in EQUAL_ON:
        for a, b in EQUAL_PAIRS:
            assert data[a] == data[b], (producer, a, b)
    if producer.startswith("batch") and "option" not in producer:
        # the context's rows are the producer's: the same velocities again, bit for bit
        assert data["velocity_ctx"][:B * S * own["vel"].element_size()] == own["vel"].cpu().numpy().tobytes()
    ctx.close()
    env.torch.cuda.synchronize()


def test_table_is_complete():
    """Every row of TABLE has one known status per producer."""
    for cell, codes in TABLE.items():
        assert len(codes.split()) == len(COLUMNS), cell
        assert set(codes.split()) <= {OK, INV, UNF, UNS}, cell


@pytest.mark.gpu
def test_context_lifecycle(env):
    """Two contexts one after the other, each through a producer and a consumer of every family and through the calls that
    own the other scratch buffers (host staging, scene, conflict packs, tracking partials, planner grids): destroying the
    first frees what it allocated, and the second works as the first did."""
    from vexautonomousplanner_amd import footprint, plan, tracking
    t, L, lib = env.torch, env.L, env.lib
    seen = []
    for _ in range(2):
        ctx, ref, own = produce(env, "batch_f32_r64")
        got, data = run_cells(env, "batch_f32_r64", ctx, ref, own)
        own2 = env.profile_routes(ctx, "f32", 2)
        got2, data2 = run_cells(env, "routes_2", ctx, ref, own2)
        col1, col2 = COLUMNS.index("batch_f32_r64"), COLUMNS.index("routes_2")
        assert got == {k: v.split()[col1] for k, v in TABLE.items()} and got2 == {k: v.split()[col2] for k, v in TABLE.items()}
        env.sample(ctx, "f32", ref)
        # host staging (io[]), small_in / small_out
        wp = np.ascontiguousarray(ref["wp"].cpu().numpy())
        hv, hmeta, hflags = np.zeros((B, S), np.float32), np.zeros((B, 4)), np.zeros(B, np.uint32)
        hx = np.zeros((B, S), np.float32)
        assert L.vap_profile_batch_host(ctx.handle, lib.VAP_F32, B, W, S, 0.0, wp.ctypes.data_as(C.c_void_p), C.byref(env.c), 0.01,
                                        0.01, hx.ctypes.data_as(C.c_void_p), None, None, None, hv.ctypes.data_as(C.c_void_p),
                                        hmeta.ctypes.data_as(C.c_void_p), hflags.ctypes.data_as(C.c_void_p)) == lib.VAP_OK
        assert hv.tobytes() == own["vel"].cpu().numpy().tobytes() and not hflags.any()
        ts, basis = np.linspace(0.0, 1.0, 5), np.zeros((5, 6))
        assert L.vap_basis_host(ctx.handle, 0, 5, ts.ctypes.data_as(lib.dp), basis.ctypes.data_as(lib.dp)) == lib.VAP_OK
        # scene, conf_*, track_part (more than 256 rollouts per route), plan_free / plan_path
        rows, counts = ref["rows"], ref["counts"]
        robot, scene = footprint.rectangle(12, 12), footprint.Scene(circles=[(0.0, 0.0, 0.5)])
        clear = footprint.clearance(rows, counts, robot, scene, ctx=ctx)
        conf = footprint.conflicts(rows, counts, robot, rows, counts, ctx=ctx)
        roll = tracking.rollouts(rows, counts, tracking.Follower(), tracking.sample_perturbations(B, 257, seed=1), ctx=ctx)
        seeds = plan.seeds((-5.0, -5.0), (4.0, 4.0), scene, W, 0.5, ctx=ctx)
        ctx.synchronize()
        seen.append(b"".join(x.cpu().numpy().tobytes() for x in (clear["min_clearance"], conf["min_clearance"], roll["worst"],
                                                                   seeds["waypoints"])) + data["time_ctx"] + data2["closest"] + basis.tobytes())
        ctx.close()
        t.cuda.synchronize()
    assert seen[0] == seen[1]
