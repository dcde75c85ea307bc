// vap_footprint.h — what the footprint checks share: vap_footprint.hip (a footprint against a static scene),
// vap_conflict.hip (two moving footprints against each other) and vap_plan.hip (a disc against the same scene, on a grid).
// Limits, the culling slack, the point-to-segment distance and the host-side scene validation, packing and upload
// (defined in vap_footprint.hip).
#pragma once
#include "vap_internal.h"

namespace vap {

constexpr int kFootMaxVerts = 16;        // footprint and each polygon
constexpr int kFootMaxPolys = 256;
constexpr int kFootMaxPolyVerts = 4096;  // all polygons together
constexpr int kFootMaxCircles = 256;
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
// The field box, polygons and circles of a scene: limits and geometry, on the host.  scale: the largest coordinate
// magnitude; nv: the polygons' vertices together.
int check_scene(const double *h_field, int n_poly, const int *h_poly_start, const double *h_poly_xy, int n_circle,
                const double *h_circles, double &scale, int &nv);
// The packed scene's way to the device: scene_stage gives the zeroed pinned host block (free of the previous upload) and
// makes room in ctx->scene; scene_upload copies it on the context's stream.
int scene_stage(vap_ctx *ctx, size_t bytes, double **h);
int scene_upload(vap_ctx *ctx, size_t bytes);

}  // namespace vap
