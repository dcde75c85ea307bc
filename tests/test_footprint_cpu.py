"""CPU: the footprint-clearance definitions (include/vap.h, vap_footprint_clearance) on hand-computed cases through the
NumPy reference, the rectangle helper, and the host-side Scene validation of vexautonomousplanner_amd.footprint."""
import math

import numpy as np
import pytest

import footprint_ref as fr
from vexautonomousplanner_amd import footprint as fp

SQUARE = np.array([[-0.75, -0.75], [0.75, -0.75], [0.75, 0.75], [-0.75, 0.75]])   # 1.5 ft, counter-clockwise


def row(heading=0.0, x=0.0, y=0.0):
    r = np.zeros((1, 8))
    r[0, 4], r[0, 6], r[0, 7] = heading, x, y
    return r


def one(r, **scene):
    v, el, _ = fr.row_clearance(r, SQUARE, **scene)
    return float(v[0]), int(el[0])


def test_wall_square_at_origin():
    field = (-10.0, -10.0, 1.25, 10.0)
    v, el = one(row(0.0), field=field)
    assert v == pytest.approx(0.5, abs=1e-15) and el == -1
    # phi = -heading = pi/4: a corner points at +x, 0.75*sqrt(2) from the centre
    v, el = one(row(-math.pi / 4), field=field)
    assert v == pytest.approx(1.25 - 0.75 * math.sqrt(2), abs=1e-15) and el == -1
    # the sign of the heading does not matter for a square; the pose does: a corner off the field is negative
    v, _ = one(row(math.pi / 4, x=1.0), field=field)
    assert v == pytest.approx(0.25 - 0.75 * math.sqrt(2), abs=1e-15)


def test_polygon_penetration_and_distance():
    box = np.array([[0.55, -1.0], [2.0, -1.0], [2.0, 1.0], [0.55, 1.0]])
    v, el = one(row(0.0), polygons=[box])
    assert v == pytest.approx(-0.2, abs=1e-15) and el == 0
    # moved away by 0.5 ft along -x: separated by 0.3 ft
    v, _ = one(row(0.0, x=-0.5), polygons=[box])
    assert v == pytest.approx(0.3, abs=1e-15)
    # separated diagonally: corner (0.75, 0.75) to corner (2, 2) of a box at [2, 3]^2
    v, _ = one(row(0.0), polygons=[[[2.0, 2.0], [3.0, 2.0], [3.0, 3.0], [2.0, 3.0]]])
    assert v == pytest.approx(1.25 * math.sqrt(2), abs=1e-15)
    # touching
    v, _ = one(row(0.0), polygons=[[[0.75, -1.0], [2.0, -1.0], [2.0, 1.0], [0.75, 1.0]]])
    assert v == 0.0


def test_circle():
    v, el = one(row(0.0), circles=[(2.0, 0.0, 1.25)])
    assert v == pytest.approx(0.0, abs=1e-15) and el == 0
    v, _ = one(row(0.0), circles=[(0.25, 0.0, 0.1)])          # centre inside: -(0.5) - 0.1
    assert v == pytest.approx(-0.6, abs=1e-15)
    v, _ = one(row(0.0), circles=[(2.0, 2.0, 0.5)])           # nearest footprint point is the corner
    assert v == pytest.approx(1.25 * math.sqrt(2) - 0.5, abs=1e-15)


def test_ties_go_to_the_smallest_id():
    box = [[1.25, -1.0], [2.0, -1.0], [2.0, 1.0], [1.25, 1.0]]          # 0.5 from the footprint, like the wall
    field = (-10.0, -10.0, 1.25, 10.0)
    v, el = one(row(0.0), field=field, polygons=[box])
    assert v == pytest.approx(0.5) and el == -1
    v, el = one(row(0.0), polygons=[box, box], circles=[(1.75, 0.0, 0.5)])
    assert v == pytest.approx(0.5) and el == 0
    s = fr.route_summary(np.concatenate([row(0.0), row(0.0)]), 2, SQUARE, field=field)
    assert s["min_row"] == 0 and s["min_element"] == -1 and s["n_below"] == 0 and s["first_row"] == -1


def test_route_summary_without_rows():
    s = fr.route_summary(np.zeros((4, 8)), 0, SQUARE, field=fp.DEFAULT_FIELD)
    assert math.isnan(s["min_clearance"]) and (s["min_row"], s["min_element"], s["first_row"], s["n_below"]) == (-1, -1, -1, 0)


def test_rectangle_units_and_orientation():
    r = fp.rectangle(18, 24)
    assert r.shape == (4, 2)
    np.testing.assert_array_equal(r.max(axis=0), [1.0, 0.75])           # length along body x, width along body y, feet
    np.testing.assert_array_equal(r.min(axis=0), [-1.0, -0.75])
    area2 = np.sum(r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1])
    assert area2 > 0                                                     # counter-clockwise
    o = fp.rectangle(18, 24, forward_offset_in=6)
    np.testing.assert_array_equal(o[:, 0], r[:, 0] + 0.5)
    np.testing.assert_array_equal(o[:, 1], r[:, 1])
    # the front faces the direction of travel: heading 0 (phi 0) puts the front at +x
    P = fr.posed(o, np.array([0.0]), np.array([0.0]), np.array([0.0]))[0]
    assert P[:, 0].max() == pytest.approx(1.5)
    with pytest.raises(ValueError):
        fp.rectangle(0, 18)


def test_scene_reorders_clockwise_and_rejects_bad_polygons():
    cw = [[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.0]]
    s = fp.Scene(polygons=[cw])
    np.testing.assert_array_equal(s.polygons[0], np.array(cw)[::-1])
    np.testing.assert_array_equal(s.poly_start, [0, 4])
    np.testing.assert_array_equal(s.field, fp.DEFAULT_FIELD)
    assert fp.Scene(field=None).field is None
    with pytest.raises(ValueError, match="convex"):
        fp.Scene(polygons=[[[0, 0], [2, 0], [1, 0.5], [2, 2], [0, 2]]])
    with pytest.raises(ValueError, match="duplicate"):
        fp.Scene(polygons=[[[0, 0], [1, 0], [1, 0], [1, 1]]])
    with pytest.raises(ValueError, match="collinear"):
        fp.Scene(polygons=[[[0, 0], [1, 0], [2, 0], [1, 1]]])
    with pytest.raises(ValueError, match="simple"):                     # a pentagram turns left at every vertex
        star = [[math.cos(a), math.sin(a)] for a in np.arange(5) * 4 * math.pi / 5]
        fp.Scene(polygons=[star])
    with pytest.raises(ValueError):
        fp.Scene(circles=[(0.0, 0.0, 0.0)])
    with pytest.raises(ValueError):
        fp.Scene(field=(1.0, 0.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        fp.convex_polygon([[0, 0], [1, 0]], "footprint")


def test_scene_limits():
    tri = [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]
    fp.Scene(polygons=[tri] * 256, circles=[(0.0, 0.0, 1.0)] * 256)
    with pytest.raises(ValueError, match="at most"):
        fp.Scene(polygons=[tri] * 257)
    with pytest.raises(ValueError, match="at most"):
        fp.Scene(circles=[(0.0, 0.0, 1.0)] * 257)
    sixteen = [[math.cos(a), math.sin(a)] for a in np.arange(16) * 2 * math.pi / 16]
    fp.Scene(polygons=[sixteen] * 256)                                  # 4096 vertices, the most a scene can hold
    seventeen = [[math.cos(a), math.sin(a)] for a in np.arange(17) * 2 * math.pi / 17]
    with pytest.raises(ValueError, match="vertices"):
        fp.Scene(polygons=[seventeen])


def test_reference_against_a_dense_brute_force():
    """The reference's separated-polygon distance against the distance between densely sampled boundaries; its
    penetration depth against the bounding-circle bound."""
    rng = np.random.default_rng(3)
    foot = fp.rectangle(18, 24)
    hexagon = np.array([[math.cos(a), math.sin(a)] for a in np.arange(6) * math.pi / 3]) * 0.8 + [2.0, 0.5]
    for _ in range(20):
        r = row(rng.uniform(-math.pi, math.pi), rng.uniform(-1, 3), rng.uniform(-1, 2))
        v = fr.polygon_clearance(fr.posed(foot, r[:, 4], r[:, 6], r[:, 7]), hexagon)[0]
        P = fr.posed(foot, r[:, 4], r[:, 6], r[:, 7])[0]
        if v > 0:
            t = np.linspace(0, 1, 401)[:, None]
            bp = np.concatenate([P[i] + t * (P[(i + 1) % 4] - P[i]) for i in range(4)])
            bq = np.concatenate([hexagon[i] + t * (hexagon[(i + 1) % 6] - hexagon[i]) for i in range(6)])
            d = np.min(np.linalg.norm(bp[:, None] - bq[None], axis=-1))
            assert d == pytest.approx(v, abs=5e-3)
        else:
            assert -v <= 0.8 + math.hypot(1.0, 0.75) + 1e-12


def test_scene_c_args():
    """Scene.c_args(): the six scene arguments of the C-ABI in its order, the counts beside their arrays, None for no field and
    for the empty arrays; poly_start always has its leading 0."""
    import ctypes as C
    tri = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    quad = np.array([[2.0, 2.0], [3.0, 2.0], [3.0, 3.0], [2.0, 3.0]])
    s = fp.Scene(field=(-6.0, -5.0, 6.0, 5.0), polygons=[tri, quad], circles=[(0.5, 0.25, 0.125), (1.0, 2.0, 3.0), (4.0, 4.0, 0.5)])
    a = s.c_args()
    assert isinstance(a, tuple) and len(a) == 6
    field, n_poly, start, xy, n_circle, circles = a
    assert (n_poly, n_circle) == (2, 3) == (s.n_polygons, s.n_circles)
    assert [field[i] for i in range(4)] == [-6.0, -5.0, 6.0, 5.0]
    assert [start[i] for i in range(3)] == [0, 3, 7]
    assert [xy[i] for i in range(14)] == list(np.concatenate([tri, quad]).ravel())
    assert [circles[i] for i in range(9)] == [0.5, 0.25, 0.125, 1.0, 2.0, 3.0, 4.0, 4.0, 0.5]
    assert C.cast(xy, C.c_void_p).value == s.poly_xy.ctypes.data and C.cast(circles, C.c_void_p).value == s.circles.ctypes.data
    field, n_poly, start, xy, n_circle, circles = fp.Scene(field=None).c_args()
    assert field is None and xy is None and circles is None and (n_poly, n_circle) == (0, 0) and start[0] == 0
    assert fp.Scene().c_args()[0][2] == fp.DEFAULT_FIELD[2]
