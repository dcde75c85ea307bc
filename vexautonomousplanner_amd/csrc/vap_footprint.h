// vap_footprint.h — what the footprint checks share: vap_footprint.hip (a footprint against a static scene) and
// vap_conflict.hip (two moving footprints against each other).  Limits, the culling slack, the point-to-segment distance
// and the host-side polygon validation and packing (defined in vap_footprint.hip).
#pragma once
#include "vap_internal.h"

namespace vap {

constexpr int kFootMaxVerts = 16;        // footprint and each polygon
constexpr double kCullSlack = 1e-9;      // ft, per ft of coordinate magnitude (rounding of the bound and of the exact tests)

// squared distance from p to the segment a -> a + e (il2 = 1 / |e|^2)
__device__ __forceinline__ double seg_dist2(double px, double py, double ax, double ay, double ex, double ey, double il2)
{
    const double wx = px - ax, wy = py - ay;
    double t = (wx * ex + wy * ey) * il2;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double dx = wx - t * ex, dy = wy - t * ey;
    return dx * dx + dy * dy;
}

// A convex, counter-clockwise, simple polygon of 3..16 finite vertices with no collinear or duplicate vertices.
int check_convex(const double *v, int n, const char *what, int idx);
// [n][8] rows of a polygon: x, y, outward unit normal of the edge to the next vertex, that edge, 1 / |edge|^2, 0
void pack_polygon(const double *v, int n, double *out);
// centre (vertex mean) and bounding radius of a polygon
void bound_polygon(const double *v, int n, double &cx, double &cy, double &r);

}  // namespace vap
