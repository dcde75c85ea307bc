"""CPU: vap_rollout_conflicts' definitions through the NumPy composition of tests/rollout_conflicts_ref.py — the known
answers, the fold, and that the partner routes of tests/test_gpu_rollout_conflicts.py bite (contacts, clear rollouts, mixed
routes, minima in the tail and before the partner starts) — and the host side: the declaration, the argtypes, and the
refusals of the C-ABI, of tracking.rollout_conflicts and of search.refine(robust_conflicts=True), which come before any
device call."""
import os
import re

import numpy as np
import pytest

import golden_util as gu
import pursuit_ref as pr
import rollout_conflicts_ref as xr
import tracking_ref as tr
from vexautonomousplanner_amd import _lib, footprint, search, tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "vap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+vap_rollout_conflicts\s*\(([^;]*)\)\s*;", code)
    assert m, "vap_rollout_conflicts is not declared in include/vap.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert len(args) == 45 and args[:3] == ["vap_ctx *ctx", "int follower_kind", "const void *follower"]
    assert args[12:25] == ["int n_foot_a", "const double *h_foot_a", "int Bo", "long cap_o", "const double *d_rows_o", "const int *d_counts_o",
                           "int stride_o", "int n_foot_o", "const double *h_foot_o", "double margin", "int shift_rows",
                           "const int *d_route_shift", "const int *d_rollout_shift"]
    assert args[32:34] == ["int *d_n_unfinished", "int *d_route_status"] and args[-1] == "int *d_n_conflict_valid"
    assert not any("exec" in a for a in args), "the call takes no executed-row arguments"
    # the follower's own arguments come first, exactly as in vap_rollout_clearance
    c = re.search(r"int\s+vap_rollout_clearance\s*\(([^;]*)\)\s*;", code)
    assert args[:12] == [re.sub(r"\s+", " ", a).strip() for a in c.group(1).split(",")][:12]
    assert len(_lib.lib().vap_rollout_conflicts.argtypes) == len(args)
    assert "vap_rollout_conflicts" in _lib.EXPORTS and hasattr(_lib.lib(), "vap_rollout_conflicts")
    d = re.search(r"#define\s+VAP_ROLLOUT_CONFLICT_OTHERS_MAX\s+(\d+)", code)
    assert d and int(d.group(1)) == tracking.CONFLICT_OTHERS_MAX == _lib.RANGE_MAX_PARTNERS == 16
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    assert callable(BatchedTrajectoryGenerator.rollout_conflicts) and callable(tracking.rollout_conflicts)


def test_abi_checks_its_arguments_before_the_context():
    """With a null context a bad host argument is reported as that argument, a good call as the null context."""
    import ctypes as C
    L = _lib.lib()
    one = (C.c_double * 8)(*tr.NOMINAL)
    cnt = (C.c_int * 2)(4, 0)
    rows = (C.c_double * 32)()
    rows_o = (C.c_double * 32)()
    foot = np.ascontiguousarray(xr.SQUARE)

    def call(kind=0, f=None, K=1, foot_o=foot, Bo=1, shift=0, margin=0.0, unfinished=None, cap_o=4, capacity=4):
        fs = tracking.Follower().as_struct() if f is None else f
        st = L.vap_rollout_conflicts(None, kind, C.cast(C.pointer(fs), C.c_void_p) if fs else None, 1, capacity, rows, cnt, 2, 0.01, K, 0, one,
                                     4, foot.ctypes.data_as(_lib.dp), Bo, cap_o, rows_o, cnt, 2, 4, foot_o.ctypes.data_as(_lib.dp), margin, shift,
                                     None, None, *[None] * 7, unfinished, None, *[None] * 11)
        return st, L.vap_last_error().decode()

    st, msg = call()
    assert st == _lib.VAP_ERR_INVALID and "null context" in msg
    st, msg = call(kind=1, f=tracking.Pursuit().as_struct(), unfinished=cnt, shift=-(1 << 24))
    assert st == _lib.VAP_ERR_INVALID and "null context" in msg
    for kw, word in ((dict(kind=2), "follower_kind"), (dict(f=False), "follower"), (dict(K=0), "K ="), (dict(K=4097), "K ="),
                     (dict(unfinished=cnt), "d_n_unfinished"), (dict(Bo=0), "Bo = 0"), (dict(shift=(1 << 24) + 1), "shift_rows"),
                     (dict(shift=-(1 << 24) - 1), "shift_rows"), (dict(foot_o=np.ascontiguousarray(foot[::-1])), "clockwise"),
                     (dict(margin=float("nan")), "margin"), (dict(cap_o=-1), "cap_o")):
        st, msg = call(**kw)
        assert st == _lib.VAP_ERR_INVALID and word in msg and "null context" not in msg, (kw, msg)
    for kw, word in ((dict(Bo=17), "Bo = 17"), (dict(cap_o=(1 << 31) - 3 * (1 << 24)), "cap_o"), (dict(capacity=(1 << 31) - 3 * (1 << 24)), "capacity")):
        st, msg = call(**kw)
        assert st == _lib.VAP_ERR_UNSUPPORTED and word in msg and "null context" not in msg, (kw, msg)


class _Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """tracking's way to the library without a device: host tensors, and a context whose library raises when touched."""
    import torch
    calls = []

    class FakeLib:
        def __getattr__(self, name):
            calls.append(name)
            raise _Reached(name)

    class FakeCtx:
        _L, handle = FakeLib(), None

        def set_option(self, *a):
            pass

    cpu = torch.device("cpu")

    def time_rows(rows, counts, _, device):
        rows = np.asarray(rows)
        if rows.ndim == 2:
            return torch.as_tensor(rows)[None], torch.tensor([[rows.shape[0], 0]], dtype=torch.int32), True, cpu
        return torch.as_tensor(rows), torch.as_tensor(np.asarray(counts, dtype=np.int32)).reshape(len(rows), 1), False, cpu

    monkeypatch.setattr(tracking, "time_rows", time_rows)
    monkeypatch.setattr(tracking, "device_array", lambda a, dev, dtype: torch.as_tensor(a, dtype=dtype))
    monkeypatch.setattr(tracking, "buffers", lambda out, shapes, dev: {k: torch.zeros(s, dtype=d) for k, (s, d) in shapes.items()})
    monkeypatch.setattr(tracking, "context_for", lambda dev, ctx: FakeCtx())
    return calls


def test_python_refusals_come_before_the_library(no_device):
    rows, rec = np.zeros((4, 8)), np.array([tracking.NOMINAL] * 2)
    foot = footprint.rectangle(18, 18)
    good = dict(rows=rows, counts=None, follower=tracking.Follower(), perturbations=rec, footprint=foot, others_rows=np.zeros((3, 5, 8)),
                others_counts=np.array([5, 5, 0]))

    def call(**kw):
        return tracking.rollout_conflicts(**{**good, **kw})

    with pytest.raises(_Reached):                                   # the stubs do lead to the library
        call()
    with pytest.raises(_Reached):
        call(follower=tracking.Pursuit(), others_rows=np.zeros((5, 8)), others_counts=None, route_shift=[3], rollout_shift=np.array([-4, 4]),
             shift_rows=-(1 << 24), pairs=True)
    assert no_device == ["vap_rollout_conflicts"] * 2
    del no_device[:]
    for kw, exc in ((dict(follower=dict(tr.DEFAULTS)), TypeError),                     # wrong follower type
                    (dict(follower=tracking.Follower(b=0)), ValueError),
                    (dict(footprint=foot[[0, 1, 3, 2]]), ValueError),                  # bad footprint: not convex
                    (dict(footprint=foot[::-1]), ValueError),                          # clockwise
                    (dict(others_footprint=foot[::-1]), ValueError),
                    (dict(others_footprint=foot[:2]), ValueError),
                    (dict(perturbations=np.zeros((0, 8))), ValueError),                # K = 0
                    (dict(perturbations=np.zeros((4097, 8))), ValueError),
                    (dict(perturbations=np.zeros((3, 7))), ValueError),                # records of the wrong shape
                    (dict(others_rows=np.zeros((0, 5, 8)), others_counts=np.zeros(0)), ValueError),      # Bo = 0
                    (dict(others_rows=np.zeros((17, 5, 8)), others_counts=np.zeros(17)), ValueError),    # Bo = 17
                    (dict(shift_rows=(1 << 24) + 1), ValueError),
                    (dict(shift_rows=1.5), ValueError),
                    (dict(route_shift=[1, 2]), ValueError),                            # one route, two entries
                    (dict(rollout_shift=[1, 2, 3]), ValueError),                       # two rollouts, three entries
                    (dict(rollout_shift=[0.5, 1.0]), ValueError),                      # not integer rows
                    (dict(margin=float("nan")), ValueError),
                    (dict(time_step=0.0), ValueError)):
        with pytest.raises(exc):
            call(**kw)
    assert no_device == []


def test_robust_conflicts_needs_a_follower_and_others():
    class Gen:
        device = None

    foot, scene = footprint.rectangle(18, 18), footprint.Scene()
    others = {"rows": None, "counts": None}
    with pytest.raises(ValueError, match="robust_conflicts needs a follower"):
        search.refine(Gen(), np.zeros((5, 2)), 0.5, foot, scene, samples=100, robust_conflicts=True, others=others)
    with pytest.raises(ValueError, match="robust_conflicts needs others"):
        search.refine(Gen(), np.zeros((5, 2)), 0.5, foot, scene, samples=100, robust_conflicts=True, follower=tracking.Follower(),
                      perturbations=np.array([tracking.NOMINAL]))
    with pytest.raises(ValueError, match="others_start_jitter"):
        search.refine(Gen(), np.zeros((5, 2)), 0.5, foot, scene, samples=100, others_start_jitter=[0, 1])
    with pytest.raises(ValueError, match="others_shift_rows"):
        search.refine(Gen(), np.zeros((5, 2)), 0.5, foot, scene, samples=100, others_shift_rows=0.5)


@pytest.mark.parametrize("kind", ["ramsete", "pursuit"])
def test_known_answer(kind):
    """The case of rollout_conflicts_ref.known_case: a straight drive beside a parked partner at the lateral gap g; a record
    that starts dy towards it has g - dy, at the start row, to 1e-12."""
    rows, P, partner, cnt, expect = xr.known_case()
    np.testing.assert_array_equal(xr.SQUARE, footprint.rectangle(18, 18))
    f = tr.follower(settle_rows=xr.KNOWN_SETTLE) if kind == "ramsete" else pr.pursuit(settle_rows=xr.KNOWN_SETTLE)
    o = xr.route(rows, len(rows), kind, f, P, xr.SQUARE, partner, cnt, margin=xr.KNOWN_MARGIN)
    print("known answer:", o["conflict"], "rows", o["conflict_rows"].tolist())
    assert np.abs(o["conflict"] - expect).max() <= 1e-12
    assert o["conflict_rows"].tolist() == [[0, 0, 0, -1], [0, 0, 1, 0], [0, 0, 0, -1]]
    assert o["pair_clearance"].shape == (3, 1) and o["pair_rows"].tolist() == [[[0, -1]], [[0, 0]], [[0, -1]]]
    assert (o["n_conflicting"], o["n_conflict_valid"], o["worst_conflict_rollout"], o["worst_conflict_other"], o["worst_conflict_row"]) == (1, 3, 1, 0, 0)
    assert o["worst_conflict"] == o["conflict"][1] and o["mean_conflict"] == (o["conflict"][0] + o["conflict"][1] + o["conflict"][2]) / 3


def test_a_start_jitter_makes_the_contact():
    """rollout_conflicts_ref.crossing_case: on time the partner crosses the route long after the robot has passed; with the
    jitter that puts it on the route at the robot's instant the two overlap a full footprint, at that row."""
    rows, P, partner, cnt = xr.crossing_case()
    f = tr.follower(settle_rows=xr.KNOWN_SETTLE)
    on_time = xr.route(rows, len(rows), "ramsete", f, P, xr.SQUARE, partner, cnt, margin=0.0, shifts=[0])
    jitter = xr.route(rows, len(rows), "ramsete", f, P, xr.SQUARE, partner, cnt, margin=0.0, shifts=[xr.KNOWN_CROSS_JITTER])
    assert on_time["conflict"][0] > 0.05 and on_time["conflict_rows"][0, 1] >= len(rows) + xr.KNOWN_SETTLE      # clear, and in the tail
    assert on_time["conflict_rows"][0].tolist()[2:] == [0, -1]
    assert abs(jitter["conflict"][0] + 1.5) <= 1e-9 and jitter["conflict_rows"][0].tolist()[:3] == [0, 20, 1]
    assert xr.sums(5, [1 << 25, -3], [-(1 << 25), 7], 2, 2).tolist() == [[5, 5 + (1 << 24) + 7], [5 - 3 - (1 << 24), 9]]      # the clamp


def test_fold_order_ties_and_empty_routes():
    c = np.array([0.3, np.nan, 0.1, 0.1, 0.5])
    r = np.array([[1, 4, 0, -1], [-1, -1, 0, -1], [2, 7, 3, 7], [0, 2, 1, 2], [3, 9, 0, -1]])
    s = xr.fold(c, r, 0.2)
    assert (s["worst_conflict"], s["worst_conflict_rollout"], s["worst_conflict_other"], s["worst_conflict_row"]) == (0.1, 2, 2, 7)
    assert s["mean_conflict"] == (((0.3 + 0.1) + 0.1) + 0.5) / 4 and (s["n_conflicting"], s["n_conflict_valid"]) == (2, 4)
    e = xr.fold(c[1:2], r[1:2], 0.2)
    assert np.isnan(e["worst_conflict"]) and np.isnan(e["mean_conflict"])
    assert [e[k] for k in xr.ROUTE_KEYS[1:4] + xr.ROUTE_KEYS[5:]] == [-1, -1, -1, 0, 0]
    # a rollout without rows, and partners without: NaN, -1, -1, 0, -1 from the composition
    rows, P, partner, cnt, _ = xr.known_case()
    P[1, 3] = -1.0
    o = xr.route(rows, len(rows), "ramsete", tr.follower(settle_rows=0), P, xr.SQUARE, partner, cnt, margin=0.2)
    assert np.isnan(o["conflict"][1]) and o["conflict_rows"][1].tolist() == [-1, -1, 0, -1] and o["n_conflict_valid"] == 2
    o = xr.route(rows, len(rows), "pursuit", pr.pursuit(), P, xr.SQUARE, partner, [0], margin=0.2)
    assert np.isnan(o["conflict"]).all() and (o["pair_rows"] == -1).all() and o["n_conflict_valid"] == 0
    # the smallest o wins a tie across pairs; prefix() is the same walk
    two = np.concatenate([partner, partner])
    o = xr.route(rows, len(rows), "ramsete", tr.follower(settle_rows=0), P[:1], xr.SQUARE, two, [1, 1], margin=0.3)
    assert o["conflict_rows"][0].tolist() == [0, 0, 2, 0]
    cmin, r4 = xr.prefix(o["pair_clearance"][0], o["pair_rows"][0], 2, 0.3)
    assert cmin == o["conflict"][0] and r4.tolist() == o["conflict_rows"][0].tolist()


@pytest.mark.parametrize("kind,K,B,_", xr.LAYOUTS)
def test_the_cases_bite(kind, K, B, _):
    """So that the GPU comparison cannot pass on partners nobody meets: on the reference alone, at the sums of the primary
    delivery, every parametrisation (Bo = 1, 3, 16: prefixes of one partner set) has a rollout in contact, a rollout clear of
    the margin, a route whose rollouts are mixed (K = 1, where that cannot be: a conflicting route and a clear one), a rollout
    whose minimum falls in the tail (row >= n_a) and one whose minimum falls before the partner has started (row < s)."""
    got = xr.bites(kind, K, B, xr.PARTNER_SEEDS[(kind, K, B)])
    for Bo in xr.OTHERS:
        print(f"{kind} K = {K}, B = {B}, Bo = {Bo}: {got[Bo]}")
        assert all(v > 0 for v in got[Bo].values()), (Bo, got[Bo])


@pytest.mark.parametrize("name", ["feat_turn", "feat_reverse", "feat_wait"])
def test_golden_records_stay_off_the_wrap(name):
    """The GPU comparison against the NumPy composition leaves out RAMSETE rollouts whose reference max |e_phi| >= 3.0 rad;
    on the reference's own rows of the golden routes and the records that test uses, that is at most 2 % of them."""
    g = gu.load(name)
    rows = tr.golden_rows(g)
    P = tracking.sample_perturbations(2, 16, seed=11)
    n_exc = 0
    for b in range(2):
        r = tr.rollout(rows, len(rows), tr.follower(), P[b], 0.01)
        n_exc += int((np.nan_to_num(r["stats"][:, 2]) >= 3.0).sum())
    print(f"{name}: {n_exc} of 32 rollouts at the wrap's discontinuity")
    assert n_exc <= 0.02 * 32
