// vap_raycast.h — the ray cast two files share: vap_range.hip (what a range sensor reads along given rows) and
// vap_odometry.hip (the same reading taken inside a rollout, on the pose while it is in registers).  One ray against the
// field walls, the packed scene's convex polygons and its circles, by the rules of vap_range_readings (include/vap.h,
// candidates 1-3), and the sensors' host-side checks.  Both files compile these definitions,
// so a reading is the same bits in both.
//
// `Args` in the templates below is any struct with the members
//     int o_poly, o_pv, o_circ, n_poly, n_circle, has_field, cull;  double xmin, ymin, xmax, ymax, slack;
// (RangeArgs, OdoScene; the offsets are scene_block's), and S the packed block, in LDS or global memory:
//     foot [n_foot_o][8] (vap_range.hip's partners; none elsewhere) | poly [n_poly][4] | pv [nv][8] | circ [n_circle][4]
// in vap_footprint.h's layouts.
#pragma once
#include <cmath>

#include "vap_footprint.h"

namespace vap {

constexpr int kRangeMaxSens = 8;
constexpr double kRangeGuard = 1.0 - 0x1p-40;   // tn * guard >= best * den  =>  fl(tn / den) >= best

// true when nothing within `rad` of (cx, cy) can be hit by the ray at a parameter below best
__device__ __forceinline__ bool ray_culled(double ox, double oy, double ux, double uy, double best, double slack, double cx,
                                           double cy, double rad)
{
    const double dx = cx - ox, dy = cy - oy;
    const double along = dx * ux + dy * uy, perp = dx * uy - dy * ux;
    const double reach = rad + slack;
    return fabs(perp) > reach || along < -reach || along - reach > best;     // false for a NaN
}

// Edge a -> a + e of a packed polygon row v = {ax, ay, nx, ny, ex, ey, ..} against the ray: a hit with a parameter strictly
// below best replaces it.  den = u x e, t = ((a - o) x e) / den, w = ((a - o) x u) / den; t >= 0 and 0 <= w <= 1 are read
// off the numerators once den is made positive (a correctly rounded quotient is <= 1 exactly when the numerator is <= the
// denominator), and t is divided out only when the guard product says it may be below best.
__device__ __forceinline__ void edge_test(const double *v, double ox, double oy, double ux, double uy, int face, int el,
                                          double &best, double &bcos, int &bface, int &bel)
{
    const double ax = v[0], ay = v[1], ex = v[4], ey = v[5];
    double den = ux * ey - uy * ex;
    const double dx = ax - ox, dy = ay - oy;
    double tn = dx * ey - dy * ex, wn = dx * uy - dy * ux;
    if (den < 0.0) { den = -den; tn = -tn; wn = -wn; }
    if (den > 0.0 && tn >= 0.0 && wn >= 0.0 && wn <= den && !(tn * kRangeGuard >= best * den)) {
        const double t = tn / den;
        if (t < best) {
            best = t;
            bcos = fabs(ux * v[2] + uy * v[3]);
            bface = face;
            bel = el;
        }
    }
}

// Candidate 1, the wall, from inside or on the box only: the start of every cast (best = inf, element -2 without one).
template <class Args>
__device__ __forceinline__ void cast_wall(const Args &g, double ox, double oy, double ux, double uy, double &best, double &bcos,
                                          int &bface, int &bel)
{
    best = INFINITY;
    bcos = NAN;
    bface = 0;
    bel = -2;
    if (g.has_field && ox >= g.xmin && ox <= g.xmax && oy >= g.ymin && oy <= g.ymax) {
        double tx = INFINITY, ty = INFINITY;
        int fx = 0, fy = 1;
        if (ux > 0.0) { tx = (g.xmax - ox) / ux; fx = 2; }
        else if (ux < 0.0) tx = (g.xmin - ox) / ux;
        if (uy > 0.0) { ty = (g.ymax - oy) / uy; fy = 3; }
        else if (uy < 0.0) ty = (g.ymin - oy) / uy;
        const bool y_side = ty < tx;                      // a tie: the x side
        const double t = y_side ? ty : tx;
        if (t < best) {
            best = t;
            bcos = y_side ? fabs(uy) : fabs(ux);
            bface = y_side ? fy : fx;
            bel = -1;
        }
    }
}

// the culling slack of one ray
template <class Args>
__device__ __forceinline__ double ray_slack(const Args &g, double ox, double oy)
{
    return g.slack + kCullSlack * (fabs(ox) + fabs(oy));
}

// Candidates 1-3: the wall, the polygons, the circles.  The element loops are uniform across the wave: call it from
// converged code, `live` false in the lanes that have no ray; an element is skipped when no live lane needs it.
template <class Args>
__device__ __forceinline__ void cast_scene(const Args &g, const double *S, bool live, double ox, double oy, double ux, double uy,
                                           double slack, double &best, double &bcos, int &bface, int &bel)
{
    cast_wall(g, ox, oy, ux, uy, best, bcos, bface, bel);
    // 2. polygons
#pragma unroll 1
    for (int k = 0; k < g.n_poly; k++) {
        const double *pk = S + g.o_poly + k * 4;
        if (g.cull && !__any(live && !ray_culled(ox, oy, ux, uy, best, slack, pk[0], pk[1], pk[2]))) continue;
        const int pc = (int)pk[3];
        const int p0 = pc >> 5, m = pc & 31;
#pragma unroll 1
        for (int j = 0; j < m; j++) edge_test(S + g.o_pv + (p0 + j) * 8, ox, oy, ux, uy, j, k, best, bcos, bface, bel);
    }
    // 3. circles
#pragma unroll 1
    for (int k = 0; k < g.n_circle; k++) {
        const double *ck = S + g.o_circ + k * 4;
        const double cx = ck[0], cy = ck[1], rad = ck[2];
        if (g.cull && !__any(live && !ray_culled(ox, oy, ux, uy, best, slack, cx, cy, rad))) continue;
        const double dx = ox - cx, dy = oy - cy;
        const double b = dx * ux + dy * uy, q = (dx * dx + dy * dy) - rad * rad;
        const double disc = b * b - q;
        if (disc >= 0.0) {
            const double sq = sqrt(disc);
            double t = -b - sq;
            if (t < 0.0) t = -b + sq;
            if (t >= 0.0 && t < best) {
                best = t;
                bcos = fabs(ux * ((ox + t * ux) - cx) + uy * ((oy + t * uy) - cy)) / rad;
                bface = 0;
                bel = g.n_poly + k;
            }
        }
    }
}

// h_sensors [n_sens][8] = {mx, my, ux, uy, r_min, r_max, min_cos, 0}: vap_range_readings' checks of the rows
inline int check_sensor_rows(int n_sens, const double *h_sensors)
{
    if (!h_sensors) return vap_fail(VAP_ERR_INVALID, "null sensors");
    for (int s = 0; s < n_sens; s++) {
        const double *q = h_sensors + 8 * (size_t)s;
        for (int j = 0; j < 8; j++)
            if (!std::isfinite(q[j])) return vap_fail(VAP_ERR_INVALID, "sensor %d: entry %d is not finite", s, j);
        if (!(std::fabs(std::hypot(q[2], q[3]) - 1.0) <= 1e-12))
            return vap_fail(VAP_ERR_INVALID, "sensor %d: the beam direction (%g, %g) is not a unit vector", s, q[2], q[3]);
        if (!(0.0 <= q[4] && q[4] <= q[5])) return vap_fail(VAP_ERR_INVALID, "sensor %d: window %g .. %g (0 <= r_min <= r_max)", s, q[4], q[5]);
        if (!(0.0 <= q[6] && q[6] <= 1.0)) return vap_fail(VAP_ERR_INVALID, "sensor %d: min_cos %g outside [0, 1]", s, q[6]);
    }
    return VAP_OK;
}

}  // namespace vap
