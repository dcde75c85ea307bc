"""The cases of robot_cases.py on the oracle alone (no GPU): they test what they claim.

test_gpu_velocity_robots.py holds every velocity kernel to the sequential sweep, and the sweep to the oracle, under the
robots, start / end speeds, shapes and paths of robot_cases.py.  That proves something only while those inputs reach the
clauses of the recurrence they are there for; a later change of a seed or a shape must not empty them quietly.  So, on
the reference's own rows:
  * another robot's rows differ from DEFAULT's on most samples;
  * the `straight` family reaches the plateau v == max_vel under the slow robots (make_waypoints rows never do);
  * a start speed above the backward envelope is lowered at sample 0, an end speed above max_vel is kept;
  * friction_coef, max_jerk and max_dec do not move a bit of a velocity row;
  * every path that is compared with the oracle is well conditioned.
The floors are caps, not measurements; every test prints what it measured on a line starting with "ROBOTS"."""
import numpy as np
import pytest

import robot_cases as rc

DEFAULT_ENDS = rc.END_SPEEDS[0]


def all_shapes():
    """(kind, B, W, S) of every fixed-grid batch of the GPU file."""
    out = rc.anchor_cases()
    for B, W, S in sorted(set(rc.LONG_SHAPES.values())):
        out += [(kind, B, W, S) for kind in rc.LONG_PATH_SETS]
    out.append(("walk",) + rc.WAVE_SHAPE)
    out.append((rc.AUTO_KIND,) + rc.AUTO_SHAPE)
    return out


@pytest.mark.parametrize("robot", rc.OTHER_ROBOTS)
def test_other_robots_rows_differ_from_the_default_robots(robot):
    """At every shape with rows of more than three samples, on every path set, under every start / end speed: at least
    half of the samples differ from DEFAULT's.  The two tiny shapes cannot tell robots apart and are there for the
    kernels' edge paths only: a row of S = 2 is (start_vel, end_vel) whatever the robot, and the one interior sample of
    S = 3 lies L / 1.5 — feet — from both ends, where every robot is at its max_vel, which four of the six share.
    For the same reason the samples at which a robot that shares DEFAULT's max_vel sits on that plateau together with
    DEFAULT are not counted (only `straight` rows have any: 64 % of the 13-waypoint rows of 10305 samples)."""
    lowest = 1.0
    max_vel = rc.ROBOTS["DEFAULT"][0]
    for kind, B, W, S in all_shapes():
        if S <= 3:
            continue
        for sv, ev in rc.ORACLE_END_SPEEDS if (kind, B, W, S) in rc.anchor_cases() else [DEFAULT_ENDS]:
            d = rc.oracle_rows(kind, B, W, S, "DEFAULT", sv, ev)["velocity"]
            v = rc.oracle_rows(kind, B, W, S, robot, sv, ev)["velocity"]
            counted = ~((v == max_vel) & (d == max_vel))
            frac = float(np.mean(v[counted] != d[counted]))
            lowest = min(lowest, frac)
            assert counted.mean() >= 0.25 and frac >= 0.5, (robot, kind, B, W, S, sv, ev, frac, counted.mean())
    print(f"ROBOTS {robot}: lowest share of samples that differ from DEFAULT's, over all shapes with S > 3: {lowest:.3f}")


@pytest.mark.parametrize("robot,floor", [("CRAWL", 0.5), ("SLOW_NARROW", 0.3)])
def test_straight_paths_reach_the_plateau(robot, floor):
    """v == max_vel EXACTLY on a large share of the samples of the `straight` batches, at every shape with more than
    three samples (a row of two is (start_vel, end_vel), a row of three has one sample that can be on the plateau: both
    are printed, not asserted) — and make_waypoints rows never hold max_vel at all (asserted: that is the gap)."""
    max_vel = rc.ROBOTS[robot][0]
    for kind, B, W, S in all_shapes():
        if kind != "straight":
            continue
        v = rc.oracle_rows(kind, B, W, S, robot, *DEFAULT_ENDS)["velocity"]
        frac = float(np.mean(v == max_vel))
        print(f"ROBOTS plateau {robot} straight ({B}, {W}, {S}): v == max_vel on {frac:.3f} of samples")
        if S > 3:
            assert frac >= floor, (robot, B, W, S, frac)
    for kind, B, W, S in all_shapes():
        if kind == "walk" and S >= 257:
            v = rc.oracle_rows(kind, B, W, S, "DEFAULT", *DEFAULT_ENDS)["velocity"]
            assert not np.any(v == rc.ROBOTS["DEFAULT"][0]), (B, W, S)


@pytest.mark.parametrize("ends", [(2.0, 0.3), (1.2, 0.7)])
def test_start_speed_is_lowered_on_manhattan_paths(ends):
    """CRAWL on `manhattan`: some path starts below min(start_vel, max_vel) — the backward sweep, not the clamp to
    max_vel, decides sample 0 — and every path starts at or below start_vel."""
    sv, ev = ends
    cap = min(sv, rc.ROBOTS["CRAWL"][0])
    for kind, B, W, S in rc.anchor_cases():
        if kind != "manhattan" or S < 3:
            continue
        v0 = rc.oracle_rows(kind, B, W, S, "CRAWL", sv, ev)["velocity"][:, 0]
        print(f"ROBOTS start {ends} manhattan ({B}, {W}, {S}): {int(np.sum(v0 < cap))} of {B} paths start below "
              f"min(start_vel, max_vel) = {cap}, lowest v[0] = {v0.min():.4f}")
        assert np.all(v0 <= sv) and np.any(v0 < cap), (B, W, S, v0.min())


@pytest.mark.parametrize("robot", ["CRAWL", "SLOW_NARROW"])
def test_end_speed_above_max_vel_is_kept(robot):
    """(0.3, 2.0): the reference leaves end_vel unclamped (a quirk) — the last sample of every path of every batch is
    2.0, above max_vel, and the row's maximum."""
    sv, ev = 0.3, 2.0
    assert ev > rc.ROBOTS[robot][0]
    for kind, B, W, S in rc.anchor_cases():
        v = rc.oracle_rows(kind, B, W, S, robot, sv, ev)["velocity"]
        assert np.all(v[:, -1] == ev) and np.all(v.max(axis=1) == ev), (robot, kind, B, W, S)
    print(f"ROBOTS end {robot}: v[-1] == {ev} > max_vel = {rc.ROBOTS[robot][0]} on every path of {len(rc.anchor_cases())} batches")


@pytest.mark.parametrize("name", sorted(rc.IGNORED_CONSTANTS))
def test_ignored_constants_stay_ignored(name):
    """Changing friction_coef, max_jerk or max_dec alone leaves the oracle's velocity rows bit-identical (max_dec: the
    velocity pass decelerates with max_acc, quirk Q9; the time loop is where max_dec acts)."""
    i, value = rc.IGNORED_CONSTANTS[name]
    for robot in ("DEFAULT", "SLOW_NARROW", "ACC_GT_DEC"):
        cons = list(rc.ROBOTS[robot])
        assert cons[i] != value
        cons[i] = value
        for kind, (B, W, S) in (("walk", rc.LANES_SHAPES[0]), ("manhattan", rc.RELAX_SHAPES[1])):
            for sv, ev in ((0.01, 0.01), (1.2, 0.7)):
                ref = rc.oracle_rows(kind, B, W, S, robot, sv, ev)["velocity"]
                got = rc.oracle_velocity(rc.paths(kind, B, W), S, cons, sv, ev)
                assert np.array_equal(got.view(np.int64), ref.view(np.int64)), (name, robot, kind, B, W, S)
    # ... and the constants that are NOT ignored do move the rows (the comparison above can fail at all)
    B, W, S = rc.LANES_SHAPES[0]
    cons = list(rc.ROBOTS["DEFAULT"])
    cons[1] = 7.5
    assert not np.array_equal(rc.oracle_velocity(rc.paths("walk", B, W), S, cons, 0.01, 0.01),
                              rc.oracle_rows("walk", B, W, S, "DEFAULT", 0.01, 0.01)["velocity"])
    print(f"ROBOTS ignored constant {name}: velocity rows bit-identical")


# The bounds the GPU file holds the sequential sweep to against the oracle (test_gpu_sweeps.py's): 1e-5 for fp32 rows,
# 1e-7 for fp64.  A path qualifies when an ulp of its waypoints moves the oracle's own row by at most 1/8 of that.
BOUNDS = {"f32": 1e-5, "f64": 1e-7}


@pytest.mark.parametrize("kind", rc.PATH_SETS)
def test_oracle_bound_paths_are_well_conditioned(kind):
    """Every path the GPU file compares with the oracle, under every robot and start / end speed it is compared under:
    the oracle's fp64 velocity row moves by at most 1/8 of the bound when every waypoint coordinate moves by one ulp.

    The ulp is fp64's, for both row types: the waypoints are fp32-representable and reach the kernels exactly, the fit,
    the tables and (in the default mode) the recurrence are fp64 — what separates a kernel from the oracle is fp64
    rounding inside them, and the fp32 rows add one output rounding.  Against an fp32 ulp NO make_waypoints row of more
    than three samples qualifies: 6e-8 times the amplification of an ordinary path (25 and more) is above 1e-5 / 8 (the
    smallest seen is 1.5e-6); that figure is printed for DEFAULT, for the record.  Paths that did not qualify were
    replaced (robot_cases.RESEEDED), the bounds stay."""
    cases = [c + (None, None, None) for c in rc.anchor_cases() if c[0] == kind]
    if kind == rc.AUTO_KIND:
        cases.append((kind,) + rc.AUTO_SHAPE + ([rc.AUTO_ROBOT], [rc.AUTO_ENDS], rc.AUTO_ORACLE_PATHS))
    limit = min(BOUNDS.values()) / 8
    for kind, B, W, S, robots, ends, idx in cases:
        wp = rc.paths(kind, B, W)
        if idx is not None:
            wp = wp[idx]
        c = rc.worst_conditioning(wp, S, "f64", robots, ends)
        c32 = rc.conditioning(wp, S, rc.ROBOTS["DEFAULT"], *DEFAULT_ENDS, ulp="f32")
        print(f"ROBOTS conditioning {kind} ({B}, {W}, {S}): velocity moves by up to {c.max():.2e} under +-1 fp64 ulp "
              f"(limit {limit:.3g}); under +-1 fp32 ulp, DEFAULT: {c32.min():.2e} .. {c32.max():.2e}")
        assert np.all(c <= limit), (kind, B, W, S, np.nonzero(c > limit)[0].tolist(), float(c.max()))
