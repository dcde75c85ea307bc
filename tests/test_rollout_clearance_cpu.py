"""CPU: vap_rollout_clearance's definitions through the NumPy composition of tests/rollout_clearance_ref.py — the known
answer, the fold, and that the seeded scenes of tests/test_gpu_rollout_clearance.py hold colliding, clear and mixed
routes — and the host side: the declaration, the argtypes, and the refusals of tracking.rollout_clearance and
search.refine(robust_clearance=True), which come before any call into the library."""
import os
import re

import numpy as np
import pytest

import pursuit_ref as pr
import rollout_clearance_ref as rc
import tracking_ref as tr
from vexautonomousplanner_amd import _lib, footprint, search, tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_entry_point_is_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "vap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+vap_rollout_clearance\s*\(([^;]*)\)\s*;", code)
    assert m, "vap_rollout_clearance is not declared in include/vap.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert len(args) == 39 and args[:3] == ["vap_ctx *ctx", "int follower_kind", "const void *follower"]
    assert args[28:30] == ["int *d_n_unfinished", "int *d_route_status"] and args[-1] == "int *d_n_clear_valid"
    assert not any("exec" in a for a in args), "the call takes no executed-row arguments"
    assert len(_lib.lib().vap_rollout_clearance.argtypes) == len(args)
    assert "vap_rollout_clearance" in _lib.EXPORTS and hasattr(_lib.lib(), "vap_rollout_clearance")
    e = re.search(r"enum\s*\{\s*VAP_FOLLOWER_RAMSETE\s*=\s*(\d+)\s*,\s*VAP_FOLLOWER_PURSUIT\s*=\s*(\d+)\s*\}", code)
    assert e and (int(e.group(1)), int(e.group(2))) == (_lib.FOLLOWER_RAMSETE, _lib.FOLLOWER_PURSUIT) == (0, 1)
    from vexautonomousplanner_amd.batch import BatchedTrajectoryGenerator
    assert callable(BatchedTrajectoryGenerator.rollout_clearance) and callable(tracking.rollout_clearance)


def test_abi_checks_its_arguments_before_the_context():
    """As the rollout calls: with a null context a bad host argument is reported as that argument, a good call as the
    null context."""
    import ctypes as C
    L = _lib.lib()
    one = (C.c_double * 8)(*tr.NOMINAL)
    cnt = (C.c_int * 2)(4, 0)
    rows = (C.c_double * 32)()
    foot = np.ascontiguousarray(rc.SQUARE)
    circ = np.array([[0.0, 3.0, 0.5]])

    def call(kind=0, f=None, K=1, foot=foot, n_foot=4, n_circle=1, margin=0.0, unfinished=None):
        fs = tracking.Follower().as_struct() if f is None else f
        st = L.vap_rollout_clearance(None, kind, C.cast(C.pointer(fs), C.c_void_p) if fs else None, 1, 4, rows, cnt, 2, 0.01, K, 0, one,
                                     n_foot, foot.ctypes.data_as(_lib.dp), None, 0, None, None, n_circle, circ.ctypes.data_as(_lib.dp),
                                     margin, *[None] * 7, unfinished, None, *[None] * 9)
        return st, L.vap_last_error().decode()

    st, msg = call()
    assert st == _lib.VAP_ERR_INVALID and "null context" in msg
    st, msg = call(kind=1, f=tracking.Pursuit().as_struct(), unfinished=cnt)
    assert st == _lib.VAP_ERR_INVALID and "null context" in msg
    for kw, word in ((dict(kind=2), "follower_kind"), (dict(f=False), "follower"), (dict(K=0), "K ="), (dict(K=4097), "K ="),
                     (dict(unfinished=cnt), "d_n_unfinished"), (dict(foot=np.ascontiguousarray(foot[::-1])), "clockwise"),
                     (dict(n_foot=2), "vertices"), (dict(margin=float("nan")), "margin"), (dict(n_circle=-1), "negative")):
        st, msg = call(**kw)
        assert st == _lib.VAP_ERR_INVALID and word in msg and "null context" not in msg, (kw, msg)
    st, msg = call(n_circle=257)
    assert st == _lib.VAP_ERR_UNSUPPORTED and "circles" in msg


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
    monkeypatch.setattr(tracking, "time_rows", lambda rows, counts, _, device: (
        torch.as_tensor(rows)[None], torch.tensor([[rows.shape[0], 0]], dtype=torch.int32), True, cpu))
    monkeypatch.setattr(tracking, "device_array", lambda a, dev, dtype: torch.as_tensor(a, dtype=dtype))
    monkeypatch.setattr(tracking, "buffers", lambda out, shapes, dev: {k: torch.zeros(s, dtype=d) for k, (s, d) in shapes.items()})
    monkeypatch.setattr(tracking, "context_for", lambda dev, ctx: FakeCtx())
    return calls


def test_python_refusals_come_before_the_library(no_device):
    rows, rec = np.zeros((4, 8)), np.array([tracking.NOMINAL])
    foot, scene = footprint.rectangle(18, 18), footprint.Scene(field=None, circles=[(0, 3, 0.5)])
    good = dict(rows=rows, counts=None, follower=tracking.Follower(), perturbations=rec, footprint=foot, scene=scene)

    def call(**kw):
        return tracking.rollout_clearance(**{**good, **kw})

    with pytest.raises(_Reached):                                   # the stubs do lead to the library
        call()
    with pytest.raises(_Reached):
        call(follower=tracking.Pursuit())
    assert no_device == ["vap_rollout_clearance"] * 2
    del no_device[:]
    for kw, exc in ((dict(follower=dict(tr.DEFAULTS)), TypeError),                     # wrong follower type
                    (dict(follower=tracking.Follower(b=0)), ValueError),
                    (dict(footprint=foot[[0, 1, 3, 2]]), ValueError),                  # bad footprint: not convex
                    (dict(footprint=foot[:2]), ValueError),
                    (dict(scene=None), TypeError),
                    (dict(perturbations=np.zeros((0, 8))), ValueError),                # K = 0
                    (dict(perturbations=np.zeros((4097, 8))), ValueError),
                    (dict(perturbations=np.zeros((3, 7))), ValueError),                # records of the wrong shape
                    (dict(perturbations=np.zeros(8)), ValueError),
                    (dict(perturbations=np.zeros((2, 3, 8))), ValueError),             # records for two routes, one route
                    (dict(margin=float("inf")), ValueError),
                    (dict(time_step=0.0), ValueError)):
        with pytest.raises(exc):
            call(**kw)
    assert no_device == []


def test_robust_clearance_needs_a_follower():
    class Gen:
        device = None

    foot, scene = footprint.rectangle(18, 18), footprint.Scene()
    with pytest.raises(ValueError, match="robust_clearance needs a follower"):
        search.refine(Gen(), np.zeros((5, 2)), 0.5, foot, scene, samples=100, robust_clearance=True)
    with pytest.raises(ValueError, match="follower needs perturbations"):
        search.refine(Gen(), np.zeros((5, 2)), 0.5, foot, scene, samples=100, robust_clearance=True, follower=tracking.Follower())


def test_known_answer():
    """The case of rollout_clearance_ref.known_case: the clearance is D -+ dy - 0.75 - r at the start row, to rounding."""
    rows, P, circles, expect, n_col = rc.known_case()
    np.testing.assert_array_equal(rc.SQUARE, footprint.rectangle(18, 18))
    o = rc.route(rows, len(rows), "ramsete", tr.follower(settle_rows=rc.KNOWN_SETTLE), P, rc.SQUARE, circles=circles, margin=rc.KNOWN_MARGIN)
    print("known answer:", o["clearance"], "rows", o["clear_rows"].tolist())
    assert np.abs(o["clearance"] - expect).max() <= 1e-15
    assert o["clear_rows"][:, 0].tolist() == [0, 0, 0] and o["clear_rows"][:, 1].tolist() == [0, 0, 0]
    assert o["clear_rows"][:, 2].tolist() == [-1, 0, -1] and o["clear_rows"][1, 3] > 0 and o["clear_rows"][0, 3] == o["clear_rows"][2, 3] == 0
    assert (o["n_colliding"], o["n_clear_valid"]) == (n_col, 3) == (1, 3)
    assert (o["worst_clear_rollout"], o["worst_clear_row"], o["worst_clear_element"]) == (1, 0, 0)
    assert o["worst_clearance"] == o["clearance"][1] and o["mean_clearance"] == (o["clearance"][0] + o["clearance"][1] + o["clearance"][2]) / 3


def test_known_answer_pure_pursuit():
    """The same case under pure pursuit: rows 0, 1, 0 and, for the record that starts nearer, 1.0147e-4 ft below the start
    row's D - dy - 0.75 - r (the rear corner swings out as the robot turns away); one of three below the margin."""
    rows, P, circles, expect, n_col = rc.known_case()
    o = rc.route(rows, len(rows), "pursuit", pr.pursuit(settle_rows=rc.KNOWN_SETTLE), P, rc.SQUARE, circles=circles, margin=rc.KNOWN_MARGIN)
    want = expect - np.array([0.0, rc.KNOWN_PURSUIT_DIP, 0.0])
    assert np.abs(o["clearance"] - want).max() <= 1e-10
    assert tuple(o["clear_rows"][:, 0]) == rc.KNOWN_PURSUIT_ROWS and o["clear_rows"][:, 1].tolist() == [0, 0, 0]
    assert np.abs(o["per"][1]["rows"][0] - expect[1]) <= 1e-15               # the start row itself is the hand value
    assert (o["n_colliding"], o["n_clear_valid"], o["worst_clear_rollout"], o["worst_clear_row"]) == (n_col, 3, 1, 1)


def test_fold_order_ties_and_empty_routes():
    c = np.array([0.3, np.nan, 0.1, 0.1, 0.5])
    r = np.array([[4, 1, -1, 0], [-1, -1, -1, 0], [7, 2, 7, 3], [2, 0, 2, 1], [9, -1, -1, 0]])
    s = rc.fold(c, r, 0.2)
    assert (s["worst_clearance"], s["worst_clear_rollout"], s["worst_clear_row"], s["worst_clear_element"]) == (0.1, 2, 7, 2)
    assert s["mean_clearance"] == (((0.3 + 0.1) + 0.1) + 0.5) / 4 and (s["n_colliding"], s["n_clear_valid"]) == (2, 4)
    e = rc.fold(c[1:2], r[1:2], 0.2)
    assert np.isnan(e["worst_clearance"]) and np.isnan(e["mean_clearance"])
    assert (e["worst_clear_rollout"], e["worst_clear_row"], e["worst_clear_element"], e["n_colliding"], e["n_clear_valid"]) == (-1, -1, -1, 0, 0)
    # a rollout without rows: NaN, -1, -1, -1, 0 from the composition
    rows, P, circles, _, _ = rc.known_case()
    P[1, 3] = -1.0
    o = rc.route(rows, len(rows), "ramsete", tr.follower(settle_rows=0), P, rc.SQUARE, circles=circles, margin=0.15)
    assert np.isnan(o["clearance"][1]) and o["clear_rows"][1].tolist() == [-1, -1, -1, 0] and o["n_clear_valid"] == 2
    o = rc.route(rows, 0, "pursuit", pr.pursuit(), P, rc.SQUARE, circles=circles, margin=0.15)
    assert np.isnan(o["clearance"]).all() and (o["clear_rows"][:, :3] == -1).all() and o["n_clear_valid"] == 0


@pytest.mark.parametrize("kind,K,B,seed", rc.LAYOUTS)
def test_seeded_scenes_are_mixed(kind, K, B, seed):
    """So that the GPU comparison cannot pass on an empty or an all-colliding scene: on the reference alone every
    parametrisation has a rollout with clearance < 0, one with clearance > margin, and a route with 0 < n_colliding <
    n_clear_valid — for K = 1, where a route has one rollout and that cannot be, a colliding route and a clear one."""
    rows, counts, P = rc.layout_case(kind, K, B)
    field, polygons, circles = rc.layout_scene(rows, counts, seed)
    assert len(polygons) == 3 and len(circles) == 3
    f = rc.ref_follower(kind)
    out = [rc.route(rows[b], counts[b], kind, f, P[b], rc.SQUARE, field, polygons, circles, rc.MARGIN) for b in range(B)]
    c = np.concatenate([o["clearance"] for o in out])
    ncol, nval = np.array([o["n_colliding"] for o in out]), np.array([o["n_clear_valid"] for o in out])
    print(f"{kind} K = {K}, B = {B}: {int((c < 0).sum())} rollouts in contact, {int((c > rc.MARGIN).sum())} clear of the margin, "
          f"{int(((ncol > 0) & (ncol < nval)).sum())} mixed routes, {int((nval == 0).sum())} routes without a valid rollout")
    assert (c < 0).any() and (c > rc.MARGIN).any()
    if K > 1:
        assert ((ncol > 0) & (ncol < nval)).any()
    else:
        assert (ncol > 0).any() and ((nval > 0) & (ncol == 0)).any()
    assert (nval == 0).any()                                        # the edge cases are in: a route without a valid rollout
