#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — generate golden vectors by running the real reference.

Runs ONLY in the build container (needs /root/reference; no-op elsewhere).  It calls the
reference's own public functions on seeded synthetic waypoints and stores inputs + outputs as small
``.npz`` fixtures under ``tests/golden/``.  No reference source is copied: a fixture is data.

    python oracle/gen_golden.py            # all small cases (~1 min)
    python oracle/gen_golden.py --c2       # additionally the 256-waypoint x 1e6-sample case (~4 min)
    python oracle/gen_golden.py --geom     # only the structured-geometry cases of tests/golden/geom/ (~1 min)
    python oracle/gen_golden.py --events   # only the event edge routes of tests/golden/events/ (~1.5 min)

What is captured per case (all fp64; waypoints are fp32-representable so that the fp32 device path
and the fp64 reference see identical inputs):
  inputs : waypoints, constraints(6), dd, start/end velocity, per-node / action-point attributes
  fit    : per-spline segment blocks (G,6,2), segment_lengths, parameters[-1]
           (quintic_hermite_spline.py:30-138)
  LUT    : lookup_table.distances / parameters / total_length (spline_manager.py:426-475)
  tables : strided + head/tail entries of the curvature / heading tables (spline_manager.py:477-548)
  grid   : for every distance sample of forward_backward_pass (motion_profile_generator.py:112-176)
           the parameter t, curvature, heading, point, and the final velocities it returns
  runsum : (case runsum_w2000) the samples where the running sum current_dist += dd selects another table
           entry than k*dd would
  profile: (case c1 only) the 9-tuple of generate_motion_profile (motion_profile_generator.py:389)

The --geom leg runs the same capture on a fixed list of paths from tests/path_families.py (straight and
axis-aligned runs, exact cusps, uneven steps, far / tiny coordinates, circles, zig-zags, two routes) and
writes them to the subdirectory tests/golden/geom/, so golden_util.names() and the tests parametrised over it do
not change.

The --events leg (tests/golden/events/) runs routes whose events sit where the reference decides.
Per case: the inputs, fit, LUT and tables as above, dd and dt as given to generate_motion_profile (profile_dd,
profile_dt), the WHOLE velocity row (velocity_row) and parameter row (t_row) of forward_backward_pass, the 9-tuple, and
the rest of the grid walk every 8th sample.  A case is written only if the reference's sample count, row count, nodes_map
and actions_map are the same on two copies of the waypoints perturbed by +-1e-6 relative; the leg fails otherwise.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refimport  # noqa: E402
from vexautonomousplanner_amd.synth import (DEFAULT_CONSTRAINTS, DEFAULT_DD, END_VEL,  # noqa: E402
                                             START_VEL, make_waypoints)

OUT = os.path.join(ROOT, "tests", "golden")
ROW_PIECE = 1 << 18
NODE_FIELDS = ("is_reverse_node", "turn", "wait_time", "stop", "max_velocity", "max_acceleration")


def build_manager(sm_mod, wp, node_attrs=None, action_points=None):
    W = len(wp)
    nodes = []
    for i in range(W):
        kw = dict(node_attrs[i]) if node_attrs else {}
        if "tangent" in kw and kw["tangent"] is not None:
            kw["tangent"] = np.asarray(kw["tangent"], dtype=float)
        nodes.append(refimport.Node(**kw))
    aps = [refimport.ActionPoint(**a) for a in (action_points or [])]
    mgr = sm_mod.QuinticHermiteSplineManager()
    ok = mgr.build_path(np.array(wp, dtype=float), nodes, aps)
    assert ok
    return mgr


def walk_grid(mgr, dd, max_keep=None):
    """Re-walk the distance grid of forward_backward_pass with the reference's own accessors."""
    total = mgr.get_total_arc_length()
    ts, ks, hs, xs, ys = [], [], [], [], []
    s = 0
    while s < total:
        t = mgr.distance_to_time(s)
        ts.append(float(t))
        ks.append(float(mgr.get_curvature(t)))
        hs.append(float(mgr.get_heading(t)))
        p = mgr.get_point_at_parameter(t)
        xs.append(float(p[0]))
        ys.append(float(p[1]))
        s += dd
    t = mgr.distance_to_time(total)
    ts.append(float(t))
    ks.append(float(mgr.get_curvature(t)))
    hs.append(float(mgr.get_heading(t)))
    p = mgr.get_point_at_parameter(t)
    xs.append(float(p[0]))
    ys.append(float(p[1]))
    return (np.array(ts), np.array(ks), np.array(hs), np.array(xs), np.array(ys))


def node_arrays(W, node_attrs):
    out = {}
    for f in NODE_FIELDS:
        out["node_" + f] = np.array([float((node_attrs[i] if node_attrs else {}).get(f, 0))
                                     for i in range(W)])
    tan = np.full((W, 2), np.nan)
    mag = np.full((W, 2), np.nan)
    if node_attrs:
        for i, a in enumerate(node_attrs):
            if a.get("tangent") is not None:
                tan[i] = a["tangent"]
                mag[i] = (a["incoming_magnitude"], a["outgoing_magnitude"])
    out["node_tangent"] = tan
    out["node_magnitudes"] = mag
    return out


def run_case(mods, name, wp, dd=DEFAULT_DD, samples=None, node_attrs=None, action_points=None,
             constraints=DEFAULT_CONSTRAINTS, full_profile=False, keep="all", out_dir=None, profile_dt=None, profile_dd=None):
    sm_mod, _, mpg = mods
    out_dir = out_dir or OUT
    t0 = time.time()
    wp = np.asarray(wp, dtype=np.float64)
    W = len(wp)
    mgr = build_manager(sm_mod, wp, node_attrs, action_points)
    mgr.rebuild_tables()
    total = mgr.get_total_arc_length()
    if samples is not None:
        # "fixed sample count" grid of this build: dd = L/(S-1.5) gives exactly S-1 loop samples
        # (k*dd < L for k <= S-2 with half a step of margin) plus the appended end sample.
        dd = float(total) / (samples - 1.5)
    c = mpg.Constraints(*constraints)
    vel = np.array(mpg.forward_backward_pass(mgr, c, dd), dtype=np.float64)
    ts, ks, hs, xs, ys = walk_grid(mgr, dd)
    assert len(vel) == len(ts), (len(vel), len(ts))
    if samples is not None:
        assert len(vel) == samples, (len(vel), samples)
    d = {
        "waypoints": wp,
        "constraints": np.array(constraints, dtype=np.float64),
        "dd": np.float64(dd),
        "samples": np.int64(samples if samples is not None else 0),
        "start_vel": np.float64(START_VEL),
        "end_vel": np.float64(END_VEL),
        "n_splines": np.int64(len(mgr.splines)),
        "lut_distances": np.asarray(mgr.lookup_table.distances),
        "lut_parameters": np.asarray(mgr.lookup_table.parameters),
        "total_length": np.float64(total),
        "n_samples": np.int64(len(vel)),
    }
    d.update(node_arrays(W, node_attrs))
    if action_points:
        d["ap_t"] = np.array([a["t"] for a in action_points], dtype=np.float64)
        for f in ("stop", "wait_time", "max_velocity", "max_acceleration"):
            d["ap_" + f] = np.array([float(a.get(f, 0)) for a in action_points])
    for si, sp in enumerate(mgr.splines):
        d[f"spline{si}_segments"] = np.array(sp.segments)
        d[f"spline{si}_segment_lengths"] = np.array(sp.segment_lengths, dtype=np.float64)
        d[f"spline{si}_param_last"] = np.float64(sp.parameters[-1])
        d[f"spline{si}_n_points"] = np.int64(len(sp.control_points))
    props = mgr._precomputed_properties
    n_tab = len(props["parameters"])
    idx = np.unique(np.concatenate([np.arange(0, min(16, n_tab)), np.arange(0, n_tab, 97),
                                    np.arange(max(0, n_tab - 16), n_tab)]))
    d["tab_n"] = np.int64(n_tab)
    d["tab_idx"] = idx
    d["tab_parameters"] = props["parameters"][idx]
    d["tab_curvatures"] = props["curvatures"][idx]
    d["tab_headings"] = props["headings"][idx]
    if keep == "all":
        sel = np.arange(len(vel))
    elif keep == "runsum":
        # long native grid: the samples where the reference's running sum (current_dist += dd) picks another
        # table entry than k*dd would, their neighbours, and a strided subset
        n = len(vel)
        k_est = np.array([float(mgr.get_curvature(mgr.distance_to_time(k * dd))) for k in range(n - 1)])
        flips = np.nonzero(k_est != ks[:n - 1])[0]
        d["runsum_flip_idx"] = flips
        near = np.concatenate([flips + o for o in (-1, 0, 1)]) if len(flips) else np.array([], dtype=int)
        sel = np.unique(np.clip(np.concatenate([near, np.arange(0, 256), np.arange(0, n, 499), np.arange(n - 256, n)]), 0, n - 1))
    elif keep == "events":
        # tests/golden/events/: the WHOLE velocity and parameter rows (the event decisions are read off the parameters,
        # MPG:124, 142-146), the rest of the geometry walk strided
        n = len(vel)
        d["velocity_row"] = vel
        d["t_row"] = ts
        sel = np.unique(np.concatenate([np.arange(0, n, 8), np.arange(max(0, n - 8), n)]))
    else:  # large case: strided + windows
        n = len(vel)
        sel = np.unique(np.concatenate([np.arange(0, 512), np.arange(0, n, 997),
                                        np.arange(n // 2, n // 2 + 4096), np.arange(n - 512, n)]))
        if keep == "dense_velocity":
            # ... and the WHOLE velocity row: the recurrence amplifies, so its worst sample can sit
            # anywhere; geometry stays strided
            d["velocity_full"] = vel
    d["grid_idx"] = sel
    d["grid_t"] = ts[sel]
    d["grid_curvature"] = ks[sel]
    d["grid_heading"] = hs[sel]
    d["grid_x"] = xs[sel]
    d["grid_y"] = ys[sel]
    d["grid_velocity"] = vel[sel]
    d["velocity_sum"] = np.float64(np.sum(vel))
    if full_profile:
        mgr2 = build_manager(sm_mod, wp, node_attrs, action_points)
        pkw = {}
        if profile_dt is not None:
            pkw["dt"] = d["profile_dt"] = np.float64(profile_dt)
        if profile_dd is not None:
            pkw["dd"] = d["profile_dd"] = np.float64(profile_dd)
        res = mpg.generate_motion_profile(mgr2, mpg.Constraints(*constraints), **{k: float(v) for k, v in pkw.items()})
        names = ("times", "positions", "linear_vels", "accelerations", "headings", "angular_vels",
                 "nodes_map", "actions_map")
        for nm, arr in zip(names, res[:8]):
            d["profile_" + nm] = np.array(arr, dtype=np.float64)
        d["profile_coords"] = np.array([np.asarray(p, dtype=np.float64) for p in res[8]])
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, name + ".npz")
    if "velocity_full" in d:
        # the whole row goes beside the fixture in pieces of 2^18 samples (a committed file stays under 1 MiB);
        # tests/golden_util.load joins them
        full = d.pop("velocity_full")
        os.makedirs(os.path.join(out_dir, "rows"), exist_ok=True)
        for k in range(0, len(full), ROW_PIECE):
            np.savez_compressed(os.path.join(out_dir, "rows", f"{name}.velocity_full.{k // ROW_PIECE}.npz"),
                                rows=full[k:k + ROW_PIECE])
    np.savez_compressed(path, **d)
    print(f"{name}: W={W} N={len(vel)} L={total:.6f} dd={dd:.6g} "
          f"{os.path.getsize(path) / 1024:.0f} KiB  {time.time() - t0:.1f}s", flush=True)


def run_api_pins(mods):
    """Reference values for the call surface the hot path does not touch: the
    Gauss-Legendre arc-length API of QuinticHermiteSpline, the manager's exact heading / curvature, and
    QuinticHermiteSpline.fit / set_*_tangent used directly (supplied derivatives, split tangents, 2-point splines)."""
    sm_mod, qh, _ = mods
    d = {}
    wp = np.asarray(make_waypoints(1, 8, 31)[0], dtype=np.float64)
    mgr = build_manager(sm_mod, wp)
    mgr.rebuild_tables()
    sp = mgr.splines[0]
    d["wp"] = wp
    d["total_arc_length"] = np.float64(sp.get_total_arc_length())                      # QHS:592-644 over the whole range
    pairs = np.array([[0.0, 7.0], [0.0, 0.5], [0.25, 0.75], [1.0, 2.0], [2.3, 6.9], [6.5, 7.0], [3.0, 3.001]])
    d["arc_pairs"] = pairs
    d["arc_lengths"] = np.array([sp.get_arc_length(a, b) for a, b in pairs])
    d["arc_lengths_n5"] = np.array([sp.get_arc_length(a, b, num_points=5) for a, b in pairs])
    s_q = np.array([0.0, 0.01, 0.5, 1.0, 2.5, 4.0, float(d["total_arc_length"]) * 0.999, float(d["total_arc_length"])])
    d["inv_s"] = s_q
    d["inv_t"] = np.array([sp.get_parameter_by_arc_length(float(v)) for v in s_q])     # QHS:646-717
    d["inv_t_tol3"] = np.array([sp.get_parameter_by_arc_length(float(v), tolerance=1e-3) for v in s_q])
    pct = np.array([0.0, 12.5, 50.0, 99.0, 100.0])
    d["percent"] = pct
    d["percent_parameter"] = np.array([sp.percent_to_parameter(float(v)) for v in pct])   # QHS:253-286
    d["percent_point"] = np.array([sp.percent_to_point(float(v)) for v in pct])
    d["end_parameter"] = np.float64(sp.get_end_parameter())
    d["magnitudes"] = np.array([sp.get_magnitude(i) for i in range(7)])
    ts = np.concatenate([np.linspace(0.0, 7.0, 41), [0.5, 1.0, 6.999999, 3.3333]])
    d["exact_t"] = ts
    d["exact_heading"] = np.array([mgr._get_heading(float(t)) for t in ts])            # SM:348-379
    d["exact_curvature"] = np.array([mgr._get_curvature(float(t)) for t in ts])        # SM:381-418
    d["step_heading"] = np.array([mgr.get_heading(float(t)) for t in ts])              # SM:332-346 (table step lookup)
    d["step_curvature"] = np.array([mgr.get_curvature(float(t)) for t in ts])
    d["mgr_percent_parameter"] = np.array([mgr.percent_to_parameter(float(v)) for v in (0.0, 0.3, 0.5, 0.99, 1.0)])  # SM:277-289
    mags = []
    for i in range(8):                                                                  # SM:174-202
        try:
            mags.append([float(v) for v in mgr.get_magnitudes_at_parameter(i)])
        except IndexError:
            # the last node when parameters[-1] is not exactly len(nodes)-1: local_t == end fails and the general
            # branch indexes one past the last segment
            mags.append([np.nan, np.nan])
    d["mgr_magnitudes"] = np.array(mags, dtype=np.float64)

    # ---- QuinticHermiteSpline used directly ----
    k = 6
    pts = np.asarray(make_waypoints(1, k, 32)[0], dtype=np.float64)
    rng = np.random.default_rng(7)
    fd = rng.normal(size=(k, 2))
    sd = rng.normal(size=(k, 2)) * 0.5
    d["cls_points"] = pts
    d["cls_first"] = fd
    d["cls_second"] = sd

    def fresh():
        q = qh.QuinticHermiteSpline()
        q.set_all_tangents([[None, None]] * k)
        return q
    q = fresh()
    assert q.fit(pts[:, 0], pts[:, 1])
    d["cls_plain_segments"] = np.array(q.segments)
    d["cls_plain_first"] = np.array(q.first_derivatives)
    d["cls_plain_second"] = np.array(q.second_derivatives)
    q = fresh()
    assert q.fit(pts[:, 0], pts[:, 1], first_derivatives=fd.copy(), second_derivatives=sd.copy())      # QHS:52-68
    d["cls_both_segments"] = np.array(q.segments)
    q = fresh()
    assert q.fit(pts[:, 0], pts[:, 1], first_derivatives=fd.copy())        # one array only: overwritten by the estimates
    d["cls_first_only_segments"] = np.array(q.segments)
    d["cls_first_only_first"] = np.array(q.first_derivatives)
    st, en = np.array([0.3, -0.7]), np.array([-0.2, 0.9])
    d["cls_start_tangent"], d["cls_end_tangent"] = st, en
    q = fresh()
    q.starting_tangent = st.copy()
    q.ending_tangent = en.copy()
    assert q.fit(pts[:, 0], pts[:, 1])                                      # QHS:129-132 (quirk Q3)
    d["cls_tangents_segments"] = np.array(q.segments)
    d["cls_tangents_first"] = np.array(q.first_derivatives)
    q = fresh()
    assert q.fit(pts[:, 0], pts[:, 1])
    assert q.set_starting_tangent(st.copy()) and q.set_ending_tangent(en.copy())      # QHS:543-590 after the fit
    d["cls_setters_segments"] = np.array(q.segments)
    d["cls_setters_point"] = np.array([q.get_point(t) for t in (0.2, 4.5, 4.99)])
    d["cls_setters_derivative"] = np.array([q.get_derivative(t) for t in (0.2, 4.5, 4.99)])
    assert q.set_starting_tangent([0.3, -0.7]) is False                      # not an ndarray: refused
    # second fit of the same object: the derivatives of the first one are reused (attributes, QHS:66)
    pts2 = pts + rng.normal(size=pts.shape) * 0.05
    q = fresh()
    assert q.fit(pts[:, 0], pts[:, 1])
    assert q.fit(pts2[:, 0], pts2[:, 1])
    d["cls_refit_points"] = pts2
    d["cls_refit_segments"] = np.array(q.segments)
    # 2-point splines: the chord stays un-normalised where the other end has a split tangent (QHS:170-172, 181-182)
    p2 = pts[:2]
    for tag, s_t, e_t in (("end", None, en), ("start", st, None), ("both", st, en), ("none", None, None)):
        q = qh.QuinticHermiteSpline()
        q.set_all_tangents([[None, None]] * 2)
        if s_t is not None:
            q.starting_tangent = s_t.copy()
        if e_t is not None:
            q.ending_tangent = e_t.copy()
        assert q.fit(p2[:, 0], p2[:, 1])
        d[f"cls_two_{tag}_segments"] = np.array(q.segments)
        d[f"cls_two_{tag}_first"] = np.array(q.first_derivatives)
    # Q1: fit before set_all_tangents
    d["cls_q1_fit_returns"] = np.int64(bool(qh.QuinticHermiteSpline().fit(pts[:, 0], pts[:, 1])))
    out = os.path.join(OUT, "api")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "pin_spline_api.npz")
    np.savez_compressed(path, **d)
    print(f"api/pin_spline_api: {len(d)} arrays, {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


def run_basis_pins(mods):
    """The four basis helpers of QuinticHermiteSpline (QHS:288-469), the never-called third-derivative one included,
    at local parameters inside, at and slightly outside [0, 1]."""
    qh = mods[1].QuinticHermiteSpline()
    rng = np.random.default_rng(12)
    ts = np.concatenate([np.linspace(0.0, 1.0, 41), rng.random(64), [1e-12, 1 - 1e-12, 0.5, 1.0 / 3.0, -0.25, 1.25]])
    d = {"t": ts}
    for order, f in enumerate((qh._get_basis_functions, qh._get_basis_derivatives, qh._get_basis_second_derivatives,
                               qh._get_basis_third_derivatives)):
        d[f"basis{order}"] = np.array([np.asarray(f(float(t)), dtype=np.float64) for t in ts])
    out = os.path.join(OUT, "api")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "pin_basis.npz")
    np.savez_compressed(path, **d)
    print(f"api/pin_basis: {len(d)} arrays, {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


def run_table_size_pins(mods):
    """build_lookup_table(min_samples != 1000) and precompute_path_properties(samples_per_node != 1000) (SM:426-475,
    477-548): tables, lookups and the velocity pass of the reference with non-default sizes, on a plain path and on a
    route that a reverse node splits."""
    sm_mod, _, mpg = mods
    d = {}
    wp8 = np.asarray(make_waypoints(1, 8, 11)[0], dtype=np.float64)
    na = [{} for _ in range(8)]
    na[3] = {"is_reverse_node": True}
    cases = (("plain", None, 257, 64), ("plain_big", None, 3001, 1500), ("split", na, 129, 333), ("tiny", None, 2, 1))
    for tag, attrs, lut_n, spn in cases:
        mgr = build_manager(sm_mod, wp8, attrs)
        mgr.build_lookup_table(min_samples=lut_n)
        mgr.precompute_path_properties(samples_per_node=spn)
        total = float(mgr.get_total_arc_length())
        d[f"{tag}_sizes"] = np.array([lut_n, spn], dtype=np.int64)
        d[f"{tag}_reverse"] = np.array([float((attrs[i] if attrs else {}).get("is_reverse_node", 0)) for i in range(8)])
        d[f"{tag}_lut_distances"] = np.asarray(mgr.lookup_table.distances)
        d[f"{tag}_lut_parameters"] = np.asarray(mgr.lookup_table.parameters)
        d[f"{tag}_total_length"] = np.float64(total)
        s_q = np.concatenate([np.linspace(0.0, total, 37), [total * 0.5001, 1e-9, total - 1e-9]])
        d[f"{tag}_s"] = s_q
        d[f"{tag}_distance_to_time"] = np.array([float(mgr.distance_to_time(float(v))) for v in s_q])
        ts = np.concatenate([np.linspace(0.0, 7.0, 57), [0.5, 3.0, 6.999999, 3.3333]])
        d[f"{tag}_t"] = ts
        d[f"{tag}_heading"] = np.array([float(mgr.get_heading(float(t))) for t in ts])
        d[f"{tag}_curvature"] = np.array([float(mgr.get_curvature(float(t))) for t in ts])
        c = mpg.Constraints(*DEFAULT_CONSTRAINTS)
        dd = total / (400 - 1.5)
        d[f"{tag}_dd"] = np.float64(dd)
        d[f"{tag}_velocity"] = np.array(mpg.forward_backward_pass(mgr, c, dd), dtype=np.float64)   # MPG:70-316: no rebuild
    d["wp"] = wp8
    # min_samples = 1: np.linspace(..., 1)[1] raises IndexError (SM:444)
    mgr = build_manager(sm_mod, wp8, None)
    try:
        mgr.build_lookup_table(min_samples=1)
        d["one_sample_raises"] = np.int64(0)
    except IndexError:
        d["one_sample_raises"] = np.int64(1)
    out = os.path.join(OUT, "api")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "pin_table_sizes.npz")
    np.savez_compressed(path, **d)
    print(f"api/pin_table_sizes: {len(d)} arrays, {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


def geom_cases():
    """The fixed list of tests/golden/geom/: (name, waypoints, run_case keywords).  Every family of tests/path_families.py
    two or three times, one fixed grid (S = 64 or 257) and one reference grid (dd = 0.005 or 0.011) each; by construction
    among them exactly east / west / north / south straight paths, a 2-waypoint straight path, exact cusps (the cusp
    node an entry of the property table), a path at -1000 ft, one shorter than 0.2 ft, a 2-turn circle, two cases on which
    the reference is discontinuous (a +-1 fp64 ulp change of the waypoints moves a velocity by > 1e-9:
    straight_disc_*, manhattan_disc_*), and two routes (a reverse node on the cusp, 90-degree turns on corners)."""
    import path_families as pf
    cases = []

    def add(name, wp, **kw):
        cases.append((name, np.asarray(wp, dtype=np.float64), kw))

    st5, st8 = pf.make("straight", 5, 5, 1), pf.make("straight", 5, 8, 2)          # east, north, west, south, random
    add("straight_east_w5_S64", st5[0], samples=64, full_profile=True)
    add("straight_north_w5_S257", st5[1], samples=257)
    add("straight_west_w8_dd011", st8[2], dd=0.011)
    add("straight_south_w8_dd005", st8[3], dd=0.005)
    add("straight_w2_S64", pf.make("straight", 5, 2, 3)[4], samples=64)
    add("straight_disc_w13_S257", pf.make("straight", 1, 13, 7)[0], samples=257)
    mh = pf.make("manhattan", 10, 13, 7)
    add("manhattan_w8_S257", pf.make("manhattan", 1, 8, 1)[0], samples=257)
    add("manhattan_w13_dd005", mh[0], dd=0.005, full_profile=True)
    add("manhattan_disc_w13_dd011", mh[9], dd=0.011)
    add("uneven_w8_S257", pf.make("uneven", 1, 8, 1)[0], samples=257)
    add("uneven_w5_dd011", pf.make("uneven", 1, 5, 2)[0], dd=0.011)
    rv4, rv13, rv5 = pf.make("reversal", 3, 4, 1), pf.make("reversal", 3, 13, 1), pf.make("reversal", 3, 5, 1)
    add("reversal_f1_w4_S257", rv4[0], samples=257)                                 # factor 1: node i+1 = node i-1
    add("reversal_f1_w13_dd011", rv13[0], dd=0.011)
    add("reversal_half_w5_S64", rv5[1], samples=64)
    # a grid that READS the cusp's table entry: the step lookup returns the entry at a node only for a sample whose
    # parameter is the node's exactly (SM:550-580), so dd is a quarter of the arc-length table's distance at the node
    (node, _factor), = pf.reversal_cusps(1, 4, 1)
    add("reversal_f1_w4_ddcusp", rv4[0], dd_to_node=(node, 4))
    sc = pf.make("scale", 3, 8, 1)
    add("scale_minus1000_w8_S257", sc[2], samples=257)
    add("scale_plus100_w8_dd011", sc[1], dd=0.011)
    add("scale_tiny_w5_dd005", pf.f32(make_waypoints(1, 5, 41)[0].astype(np.float64) * 0.02), dd=0.005)
    th = np.arange(13) * 1.05                                                       # 12.6 rad: two turns of the unit circle
    add("loops_two_turns_w13_S257", pf.f32(np.stack([np.cos(th), np.sin(th)], axis=1)), samples=257)
    add("loops_w8_dd005", pf.make("loops", 1, 8, 1)[0], dd=0.005, full_profile=True)
    add("west_w8_S64", pf.make("west", 1, 8, 1)[0], samples=64)
    add("west_w5_dd011", pf.make("west", 1, 5, 2)[0], dd=0.011)
    add("zigzag_w8_S257", pf.make("zigzag", 1, 8, 1)[0], samples=257)
    add("zigzag_w5_dd005", pf.make("zigzag", 1, 5, 2)[0], dd=0.005)
    # routes as users drive them: back up at the cusp, turn on the spot at corners
    (node, _factor), = pf.reversal_cusps(1, 8, 3)
    na = [{} for _ in range(8)]
    na[node] = {"is_reverse_node": True}
    add("route_reversal_w8", pf.make("reversal", 1, 8, 3)[0], node_attrs=na, full_profile=True)
    wp, turns = pf.manhattan_turns(pf.make("manhattan", 4, 8, 5)[3])
    na = [{} for _ in range(8)]
    for i in np.nonzero(turns)[0][:2]:
        na[int(i)] = {"turn": float(turns[i])}
    add("route_manhattan_w8", wp, node_attrs=na, full_profile=True)
    return cases


def run_geom(mods, want):
    out = os.path.join(OUT, "geom")
    total = 0
    for name, wp, kw in geom_cases():
        if want(name):
            if "dd_to_node" in kw:
                node, div = kw.pop("dd_to_node")
                mgr = build_manager(mods[0], wp)
                mgr.rebuild_tables()
                par = np.asarray(mgr.lookup_table.parameters)
                j = int(np.argmin(np.abs(par - node)))
                assert par[j] == float(node)
                kw["dd"] = float(np.asarray(mgr.lookup_table.distances)[j]) / div
            run_case(mods, name, wp, out_dir=out, **kw)
            total += os.path.getsize(os.path.join(out, name + ".npz"))
    print(f"geom: {total / 1024:.0f} KiB", flush=True)


EVENTS_REL = 1e-6      # the stability perturbation of the --events leg


def events_cases():
    """The fixed list of tests/golden/events/: (name, waypoints, run_case keywords).  Routes whose events sit where the
    reference DECIDES (MPG:112-165, 425-600): action points at t = 0, on a node, on each other, unsorted, at and behind
    the end; stops / waits on the end nodes; int(wait / dt); reverse at node 0 and on neighbours; turns of +-180, 360
    and 0.5 degrees; limits above the robot's and tiny ones; a segment shorter than dd; dt off 0.01."""
    cases = []
    wp8 = make_waypoints(1, 8, 11)[0]

    def add(name, wp=None, nodes=None, aps=None, **kw):
        wp = make_waypoints(1, 8, EVENTS_SEED.get(name, 11))[0] if wp is None else wp
        W = len(wp)
        na = [dict((nodes or {}).get(i, {})) for i in range(W)]
        cases.append((name, np.asarray(wp, dtype=np.float64), dict(node_attrs=na, action_points=aps, **kw)))

    stop01 = {"stop": True, "wait_time": 0.1}
    add("plain")
    add("ap_t0", aps=[{"t": 0.0, "stop": True}, {"t": 2.5, "max_velocity": 2.0}])
    add("ap_negative", aps=[{"t": -1.0, "stop": True, "wait_time": 0.1}, {"t": 2.5, "max_velocity": 2.0}])
    add("ap_on_node3", aps=[{"t": 3.0, "stop": True, "wait_time": 0.2}])
    add("ap_on_node3_limits", nodes={3: {"max_velocity": 2.0, "max_acceleration": 4.0}},
        aps=[{"t": 3.0, "max_acceleration": 3.0, "wait_time": 0.2}])
    add("ap_same_t", aps=[{"t": 2.5, "max_velocity": 2.0}, dict(stop01, t=2.5), {"t": 4.5, "max_velocity": 1.5}])
    add("ap_close", aps=[{"t": 2.5, "max_velocity": 2.0}, dict(stop01, t=2.5000001), {"t": 4.5, "max_velocity": 1.5}])
    add("ap_unsorted", aps=[{"t": 4.5, "max_velocity": 2.0}, dict(stop01, t=2.5)])
    add("ap_last_seg", aps=[dict(stop01, t=6.95), {"t": 6.9999, "max_velocity": 1.0}])
    add("ap_at_end", aps=[dict(stop01, t=7.0)])
    add("ap_beyond", aps=[dict(stop01, t=7.5)])
    add("ap_wait_trunc", aps=[{"t": 2.5, "wait_time": 0.009}, {"t": 4.5, "wait_time": 0.29}])     # int(wait / dt) = 0, 28 / 29
    add("stop_first_last", nodes={0: {"stop": True}, 7: {"stop": True, "wait_time": 0.3, "max_velocity": 1.0}})
    add("wait_trunc", nodes={0: {"wait_time": 0.29}, 2: {"wait_time": 0.3}, 4: {"wait_time": 0.07}, 5: {"wait_time": 0.009}})
    add("wait_dt02", nodes={0: {"wait_time": 0.3}, 3: {"wait_time": 0.5}}, profile_dt=0.02)
    add("turn_wait_dt60", nodes={3: {"turn": 90.0}, 5: {"wait_time": 0.25}}, aps=[{"t": 4.5, "wait_time": 0.1}], profile_dt=1.0 / 60.0)
    add("rev_node0", nodes={0: {"is_reverse_node": True, "wait_time": 0.2}})
    add("rev_consecutive", nodes={2: {"is_reverse_node": True}, 3: {"is_reverse_node": True}})
    add("rev_1_and_6", nodes={1: {"is_reverse_node": True}, 6: {"is_reverse_node": True}})
    add("rev_ap_same_t", nodes={3: {"is_reverse_node": True}},
        aps=[{"t": 4.5, "max_velocity": 2.0}, dict(stop01, t=4.5), {"t": 5.5, "max_velocity": 1.5}])
    add("turn_180", nodes={3: {"turn": 180.0}})
    add("turn_m180", nodes={3: {"turn": -180.0}})
    add("turn_small", nodes={3: {"turn": 0.5}})
    add("turn_wait_rev", nodes={3: {"turn": 90.0, "is_reverse_node": True, "wait_time": 0.2}})
    add("vmax_above", nodes={2: {"max_velocity": 9.0}, 4: {"max_acceleration": 30.0}})
    add("vmax_tiny", nodes={2: {"max_velocity": 0.05}, 4: {"max_acceleration": 0.2}})
    add("limits_node0", nodes={0: {"max_velocity": 0.5, "max_acceleration": 1.0}})
    short = make_waypoints(1, 8, EVENTS_SEED.get("short_seg", 11))[0].astype(np.float64)
    short[4] = short[3] + (0.002, 0.001)
    short = short.astype(np.float32)
    add("short_seg", short, nodes={4: {"stop": True}, 5: {"max_velocity": 2.0, "wait_time": 0.2}})
    add("short_seg_plain", short)
    add("dec_ne_acc_events", nodes={2: {"max_acceleration": 3.0}, 4: {"stop": True}}, aps=[{"t": 5.5, "max_acceleration": 5.0}],
        constraints=(4.0, 12.0, 6.0, 0.8, 16.0, 12.5 / 12))
    add("w2_ap", make_waypoints(1, 2, 5)[0], nodes={0: {"wait_time": 0.2}}, aps=[{"t": 0.5, "stop": True, "wait_time": 0.15}])
    add("w3_rev1", make_waypoints(1, 3, 5)[0], nodes={1: {"is_reverse_node": True, "turn": 45.0}})
    add("turn_360", nodes={3: {"turn": 360.0}})
    add("turn_consecutive", nodes={3: {"turn": 90.0}, 4: {"turn": -90.0}})
    return cases


# Cases on which the reference itself flips on seed 11's path under the 1e-6 perturbation (a nodes_map entry moves by 1;
# turn_consecutive: 578 / 577 rows): each runs on the first later path seed on which the stability assertion holds
# (short_seg, stable on seed 11, goes with short_seg_plain, whose path it shares).  The reference's step lookups make a
# route's discrete outputs this fragile on about one route in five; the default for a case is seed 11.
EVENTS_SEED = {"ap_last_seg": 12, "wait_dt02": 12, "rev_ap_same_t": 12, "limits_node0": 12, "turn_360": 12, "turn_consecutive": 12,
               "short_seg": 17, "short_seg_plain": 17}


def events_discrete(mods, wp, kw):
    """(samples, rows, nodes_map, actions_map) of the reference on one route: what must not move under the perturbation."""
    sm_mod, _, mpg = mods
    cons = kw.get("constraints", DEFAULT_CONSTRAINTS)
    dd = kw.get("profile_dd", DEFAULT_DD)
    mgr = build_manager(sm_mod, wp, kw["node_attrs"], kw["action_points"])
    mgr.rebuild_tables()
    n = len(mpg.forward_backward_pass(mgr, mpg.Constraints(*cons), dd))
    mgr = build_manager(sm_mod, wp, kw["node_attrs"], kw["action_points"])
    res = mpg.generate_motion_profile(mgr, mpg.Constraints(*cons), dt=kw.get("profile_dt", 0.01), dd=dd)
    return n, len(res[0]), [int(v) for v in res[6]], [int(v) for v in res[7]]


def run_events(mods, want):
    """tests/golden/events/: every case is written only if the reference's discrete outputs are the same on the case's
    waypoints and on two copies perturbed by +-1e-6 relative — more than ten times the fp32 input rounding (6e-8) and inside
    the fp32 mode's row tolerance (1e-5) — so that a discrete flip on the device at a written case is the device's
    decision, not the reference's sensitivity."""
    out = os.path.join(OUT, "events")
    total = 0
    unstable = []
    for name, wp, kw in events_cases():
        if not want(name):
            continue
        noise = np.random.default_rng(20).normal(size=wp.shape)
        base = events_discrete(mods, wp, kw)
        moved = [events_discrete(mods, wp * (1.0 + s * EVENTS_REL * noise), kw) for s in (1.0, -1.0)]
        if any(m != base for m in moved):
            unstable.append(name)
            print(f"{name}: UNSTABLE under {EVENTS_REL:g}: {base[:2]} {base[3]} vs {[(m[:2], m[3]) for m in moved]}: not written", flush=True)
            continue
        kw = dict(kw, profile_dt=kw.get("profile_dt", 0.01), profile_dd=kw.get("profile_dd", DEFAULT_DD))
        run_case(mods, name, wp, out_dir=out, full_profile=True, keep="events", dd=kw["profile_dd"], **kw)
        print(f"    samples {base[0]} rows {base[1]} nodes_map {base[2]} actions_map {base[3]}", flush=True)
        total += os.path.getsize(os.path.join(out, name + ".npz"))
    print(f"events: {total / 1024:.0f} KiB", flush=True)
    assert not unstable, unstable


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2", action="store_true", help="also run the 1e6-sample single-path case")
    ap.add_argument("--big", action="store_true", help="also the 2048-waypoint cases big_w2048_p* (~1-2 min of reference each)")
    ap.add_argument("--geom", action="store_true", help="only the structured-geometry cases (tests/golden/geom/)")
    ap.add_argument("--events", action="store_true", help="only the event edge routes (tests/golden/events/)")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None, help="write the fixtures here instead of tests/golden/")
    args = ap.parse_args()
    if not refimport.available():
        print("reference tree absent: nothing to do")
        return
    mods = refimport.load()
    if args.out:
        global OUT
        OUT = args.out

    def want(name):
        return args.only is None or args.only in name

    if args.geom:
        run_geom(mods, want)
        return
    if args.events:
        run_events(mods, want)
        return

    # plain-node paths at the reference's native grid (dd = 0.005 ft)
    for W in (2, 5, 8, 32):
        for seed in range(5):
            name = f"plain_w{W}_s{seed}"
            if want(name):
                run_case(mods, name, make_waypoints(1, W, 100 + seed)[0],
                         full_profile=(W in (5, 8) and seed == 0))
    # config 1: single 8-waypoint path, default constraints, seed 1 (+ full time-domain profile)
    if want("c1_w8"):
        run_case(mods, "c1_w8", make_waypoints(1, 8, 1)[0], full_profile=True)
    # fixed-sample-count grids (bench semantics): slices of config 3's batch (seed 3)
    c3 = make_waypoints(8, 32, 3)
    if want("c3_p0_S10000"):
        run_case(mods, "c3_p0_S10000", c3[0], samples=10000)
    for p in (1, 2, 3):
        if want(f"c3_p{p}_S1024"):
            run_case(mods, f"c3_p{p}_S1024", c3[p], samples=1024)
    # config 5 slice: 8 waypoints, 1024 samples
    c5 = make_waypoints(4, 8, 5)
    for p in range(2):
        if want(f"c5_p{p}_S1024"):
            run_case(mods, f"c5_p{p}_S1024", c5[p], samples=1024)
    # a long path on the reference's native grid: the running sum of dd drifts from k*dd by enough to pick
    # other table entries (quirk: the grid is current_dist += dd, MPG:112-122)
    if want("runsum_w2000"):
        run_case(mods, "runsum_w2000", make_waypoints(1, 2000, 17)[0], dd=0.002, keep="runsum")
    # the large-W randomized sweep's worst case (tools/fuzz_parity.py big, case 115: 5 paths x 2048 waypoints on the
    # reference's own grid, dd drawn by the tool): ~4.1e5 samples per path, the 1000-entry arc-length table is sparse
    # (2 segments per entry) and the recurrence amplifies last-bit differences; the whole velocity row is kept
    big = make_waypoints(5, 2048, 640273585)
    for p in range(5):
        if args.big and want(f"big_w2048_p{p}"):
            run_case(mods, f"big_w2048_p{p}", big[p], dd=0.0032122917796428277, keep="dense_velocity")
    # a 256-waypoint path on a moderate grid
    c2wp = make_waypoints(1, 256, 2)[0]
    if want("c2_w256_S20000"):
        run_case(mods, "c2_w256_S20000", c2wp, samples=20000, keep="strided")
    if args.c2 and want("c2_w256_S1000000"):
        run_case(mods, "c2_w256_S1000000", c2wp, samples=1000000, keep="strided")

    # robots whose max_dec differs from max_acc: boundary_map always holds sample 0 (MPG:110), so the
    # reference overwrites max_dec with max_acc before the first forward step (MPG:194-196) and the
    # backward sweep decelerates with max_acc; only the time loop sees the given max_dec (MPG:572-573)
    for tag, cons in (("dec_lt_acc", (4.0, 12.0, 6.0, 0.8, 16.0, 12.5 / 12)),
                      ("dec_gt_acc", (4.0, 6.0, 12.0, 0.8, 16.0, 12.5 / 12)),
                      ("other_robot", (6.5, 10.0, 7.0, 0.8, 16.0, 0.75))):
        if want(f"cons_{tag}_w8"):
            run_case(mods, f"cons_{tag}_w8", make_waypoints(1, 8, 21)[0], constraints=cons, full_profile=True)
        if want(f"cons_{tag}_S1024"):
            run_case(mods, f"cons_{tag}_S1024", make_waypoints(1, 8, 22)[0], samples=1024, constraints=cons)

    # ---- feature cases for SURVEY.md §8(f) "next" rows (node / action-point semantics) ----
    wp8 = make_waypoints(1, 8, 11)[0]
    if want("feat_stop"):
        na = [{} for _ in range(8)]
        na[3] = {"stop": True}
        run_case(mods, "feat_stop", wp8, node_attrs=na, full_profile=True)
    if want("feat_limits"):
        na = [{} for _ in range(8)]
        na[0] = {"max_velocity": 3.0, "max_acceleration": 5.0}
        na[2] = {"max_velocity": 2.0}
        na[4] = {"max_acceleration": 3.0}
        na[5] = {"max_velocity": 3.5, "max_acceleration": 6.0}
        run_case(mods, "feat_limits", wp8, node_attrs=na, full_profile=True)
    if want("feat_tangent"):
        na = [{} for _ in range(8)]
        na[2] = {"tangent": [0.6, 0.8], "incoming_magnitude": 0.7, "outgoing_magnitude": 0.4}
        na[5] = {"tangent": [-0.8, 0.6], "incoming_magnitude": 0.5, "outgoing_magnitude": 0.9}
        run_case(mods, "feat_tangent", wp8, node_attrs=na, full_profile=True)
    if want("feat_action"):
        aps = [{"t": 1.4, "max_velocity": 2.5}, {"t": 3.3, "stop": True, "max_acceleration": 4.0},
               {"t": 5.6, "wait_time": 0.2}]
        run_case(mods, "feat_action", wp8, action_points=aps, full_profile=True)
    if want("feat_reverse"):
        na = [{} for _ in range(8)]
        na[3] = {"is_reverse_node": True}
        run_case(mods, "feat_reverse", wp8, node_attrs=na, full_profile=True)
    if want("feat_turn"):
        na = [{} for _ in range(8)]
        na[4] = {"turn": 90}
        run_case(mods, "feat_turn", wp8, node_attrs=na, full_profile=True)
    if want("feat_wait"):
        na = [{} for _ in range(8)]
        na[0] = {"wait_time": 0.3}
        na[3] = {"wait_time": 0.5}
        run_case(mods, "feat_wait", wp8, node_attrs=na, full_profile=True)
    if want("feat_split2"):
        # splits that leave 2-node splines at both ends: reverse at node 1 (spline of nodes 0-1 with an ending tangent),
        # turn at node 4 (spline of nodes 4-5 with a starting tangent) — QHS:170-172, 181-182, 543-590
        wp6 = make_waypoints(1, 6, 12)[0]
        na = [{} for _ in range(6)]
        na[1] = {"is_reverse_node": True}
        na[4] = {"turn": 60}
        run_case(mods, "feat_split2", wp6, node_attrs=na, full_profile=True)
    if want("api_pins"):
        run_api_pins(mods)
    if want("table_size_pins"):
        run_table_size_pins(mods)
    if want("basis_pins"):
        run_basis_pins(mods)
    if want("feat_mixed"):
        na = [{} for _ in range(8)]
        na[2] = {"is_reverse_node": True, "wait_time": 0.1}
        na[4] = {"turn": -45, "max_velocity": 2.0}
        na[6] = {"stop": True, "tangent": [1.0, 0.0], "incoming_magnitude": 0.5,
                 "outgoing_magnitude": 0.5}
        aps = [{"t": 0.5, "max_velocity": 1.5}, {"t": 5.2, "stop": True}]
        run_case(mods, "feat_mixed", wp8, node_attrs=na, action_points=aps, full_profile=True)


if __name__ == "__main__":
    main()
