// vap_footprint.h — what the footprint checks share: vap_footprint.hip (a footprint against a static scene),
// vap_conflict.hip (two moving footprints against each other), vap_plan.hip (a disc against the same scene, on a grid) and
// the rollout kernels in their clearance mode (vap_tracking.hip, vap_pursuit.hip for vap_rollout_clearance.hip).
// Limits, the culling slack, the point-to-segment distance, the packed scene and the clearance of one posed footprint
// against it (device, inline), and the host-side scene validation, packing and upload (defined in vap_footprint.hip).
#pragma once
#include <climits>
#include <cmath>

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

// Packed scene (fp64):
//   foot  [n_foot][8]  body vertex x, y; outward unit normal of the edge to the next vertex nx, ny; that edge ex, ey;
//                      1 / |e|^2; 0
//   poly  [n_poly][4]  centre x, y; bounding radius; first vertex * 32 + vertex count (as a double)
//   pv    [nv][8]      the polygons' vertices, same layout as foot, in world coordinates; slot 7 holds |e| = sqrt(ex ex + ey ey)
//                      (read by k_plan_clearance only)
//   circ  [n_circle][4] cx, cy, r, 0
struct FootScene {
    const double *__restrict__ foot;
    const double *__restrict__ poly;
    const double *__restrict__ pv;
    const double *__restrict__ circ;
    double fcx, fcy, fR;                  // footprint centre (body frame) and bounding radius
    double xmin, ymin, xmax, ymax;
    double slack;                         // kCullSlack * (1 + scene coordinate scale)
    int has_field, n_foot, n_poly, n_circle, cull;
};

// the footprint's vertex i at the row's pose
__device__ __forceinline__ void foot_vertex(const FootScene &s, int i, double x, double y, double c, double sn, double &wx,
                                            double &wy)
{
    const double bx = s.foot[i * 8 + 0], by = s.foot[i * 8 + 1];
    wx = x + (c * bx - sn * by);
    wy = y + (sn * bx + c * by);
}

// Polygon element [p0, p0 + m): separated -> distance, overlapping -> minus the smallest overlap over the edge normals
// of both polygons.
inline __device__ double poly_clearance(const FootScene &s, int p0, int m, double x, double y, double c, double sn)
{
    const int n = s.n_foot;
    double sep = INFINITY;
    bool separated = false;
    // axes of the footprint's edges (rotated body normals)
#pragma unroll 1
    for (int i = 0; i < n && !separated; i++) {
        const double bnx = s.foot[i * 8 + 2], bny = s.foot[i * 8 + 3];
        const double nx = c * bnx - sn * bny, ny = sn * bnx + c * bny;
        double f0 = INFINITY, f1 = -INFINITY, q0 = INFINITY, q1 = -INFINITY;
#pragma unroll 1
        for (int j = 0; j < n; j++) {
            double wx, wy;
            foot_vertex(s, j, x, y, c, sn, wx, wy);
            const double d = nx * wx + ny * wy;
            f0 = fmin(f0, d);
            f1 = fmax(f1, d);
        }
#pragma unroll 1
        for (int k = 0; k < m; k++) {
            const double *v = s.pv + (size_t)(p0 + k) * 8;
            const double d = nx * v[0] + ny * v[1];
            q0 = fmin(q0, d);
            q1 = fmax(q1, d);
        }
        const double ov = fmin(f1, q1) - fmax(f0, q0);
        sep = fmin(sep, ov);
        separated = !(ov > 0.0);
    }
    // axes of the polygon's edges
#pragma unroll 1
    for (int k = 0; k < m && !separated; k++) {
        const double *vk = s.pv + (size_t)(p0 + k) * 8;
        const double nx = vk[2], ny = vk[3];
        double f0 = INFINITY, f1 = -INFINITY, q0 = INFINITY, q1 = -INFINITY;
#pragma unroll 1
        for (int j = 0; j < n; j++) {
            double wx, wy;
            foot_vertex(s, j, x, y, c, sn, wx, wy);
            const double d = nx * wx + ny * wy;
            f0 = fmin(f0, d);
            f1 = fmax(f1, d);
        }
#pragma unroll 1
        for (int j = 0; j < m; j++) {
            const double *v = s.pv + (size_t)(p0 + j) * 8;
            const double d = nx * v[0] + ny * v[1];
            q0 = fmin(q0, d);
            q1 = fmax(q1, d);
        }
        const double ov = fmin(f1, q1) - fmax(f0, q0);
        sep = fmin(sep, ov);
        separated = !(ov > 0.0);
    }
    if (!separated) return -sep;
    // separated or touching: the distance is attained between a vertex of one and an edge of the other
    double d2 = INFINITY;
#pragma unroll 1
    for (int i = 0; i < n; i++) {
        double ax, ay;
        foot_vertex(s, i, x, y, c, sn, ax, ay);
        const double bex = s.foot[i * 8 + 4], bey = s.foot[i * 8 + 5], il2 = s.foot[i * 8 + 6];
        const double ex = c * bex - sn * bey, ey = sn * bex + c * bey;
#pragma unroll 1
        for (int k = 0; k < m; k++) {
            const double *v = s.pv + (size_t)(p0 + k) * 8;
            d2 = fmin(d2, seg_dist2(ax, ay, v[0], v[1], v[4], v[5], v[6]));    // footprint vertex i, polygon edge k
            d2 = fmin(d2, seg_dist2(v[0], v[1], ax, ay, ex, ey, il2));         // polygon vertex k, footprint edge i
        }
    }
    return sqrt(d2);
}

// Circle element: signed distance from the centre to the footprint (positive outside) minus r.
inline __device__ double circle_clearance(const FootScene &s, double qx, double qy, double r, double x, double y, double c, double sn)
{
    double smax = -INFINITY, d2 = INFINITY;
#pragma unroll 1
    for (int i = 0; i < s.n_foot; i++) {
        double ax, ay;
        foot_vertex(s, i, x, y, c, sn, ax, ay);
        const double bnx = s.foot[i * 8 + 2], bny = s.foot[i * 8 + 3];
        const double bex = s.foot[i * 8 + 4], bey = s.foot[i * 8 + 5], il2 = s.foot[i * 8 + 6];
        const double nx = c * bnx - sn * bny, ny = sn * bnx + c * bny;
        const double ex = c * bex - sn * bey, ey = sn * bex + c * bey;
        smax = fmax(smax, nx * (qx - ax) + ny * (qy - ay));
        d2 = fmin(d2, seg_dist2(qx, qy, ax, ay, ex, ey, il2));
    }
    return (smax > 0.0 ? sqrt(d2) : smax) - r;
}

// true when an element of centre (ox, oy) and bounding radius orad cannot go below best at this row
__device__ __forceinline__ bool culled(const FootScene &s, double best, double slack, double fx, double fy, double ox, double oy,
                                       double orad)
{
    if (!s.cull) return false;
    const double reach = best + slack + orad + s.fR;   // skip when |o - f| > reach
    if (reach < 0.0) return true;
    const double dx = ox - fx, dy = oy - fy;
    return dx * dx + dy * dy > reach * reach;          // false for best = +inf or NaN
}

// The clearance of one row and the element that gives it.  A NaN in the pose gives NaN (fmin and fmax drop a NaN operand,
// so the tests below would turn one into +-inf or into a finite overlap).
inline __device__ double row_clearance(const FootScene &s, double heading, double x, double y, int &elem)
{
    const double phi = -heading;
    double sn, c;
    sincos(phi, &sn, &c);
    double best = INFINITY;
    elem = INT_MAX;
    if (heading != heading || x != x || y != y) return NAN;
    if (s.has_field) {
        double w = INFINITY;
#pragma unroll 1
        for (int i = 0; i < s.n_foot; i++) {
            double px, py;
            foot_vertex(s, i, x, y, c, sn, px, py);
            w = fmin(w, fmin(fmin(px - s.xmin, s.xmax - px), fmin(py - s.ymin, s.ymax - py)));
        }
        best = w;
        elem = -1;
    }
    const double fx = x + (c * s.fcx - sn * s.fcy), fy = y + (sn * s.fcx + c * s.fcy);
    const double slack = s.slack + kCullSlack * (fabs(x) + fabs(y));
#pragma unroll 1
    for (int k = 0; k < s.n_poly; k++) {
        const double *pk = s.poly + (size_t)k * 4;
        if (culled(s, best, slack, fx, fy, pk[0], pk[1], pk[2])) continue;
        const int code = (int)pk[3];
        const double v = poly_clearance(s, code >> 5, code & 31, x, y, c, sn);
        if (v < best) { best = v; elem = k; }
    }
#pragma unroll 1
    for (int k = 0; k < s.n_circle; k++) {
        const double *ck = s.circ + (size_t)k * 4;
        if (culled(s, best, slack, fx, fy, ck[0], ck[1], ck[2])) continue;
        const double v = circle_clearance(s, ck[0], ck[1], ck[2], x, y, c, sn);
        if (v < best) { best = v; elem = s.n_poly + k; }
    }
    return best;
}

// row_clearance for a caller that keeps a minimum over rows.  `cap`: the caller has no use for a clearance of `cap` or more
// (it keeps a minimum that already is that small), so an element that cannot go below min(running best, cap) is culled
// too; a result below `cap` is then still exact, with its element, and one of `cap` or more is only a bound from above.  Otherwise row_clearance, line for line.
inline __device__ double row_clearance_capped(const FootScene &s, double heading, double x, double y, int &elem, double cap)
{
    const double phi = -heading;
    double sn, c;
    sincos(phi, &sn, &c);
    double best = INFINITY;
    elem = INT_MAX;
    if (heading != heading || x != x || y != y) return NAN;
    if (s.has_field) {
        double w = INFINITY;
#pragma unroll 1
        for (int i = 0; i < s.n_foot; i++) {
            double px, py;
            foot_vertex(s, i, x, y, c, sn, px, py);
            w = fmin(w, fmin(fmin(px - s.xmin, s.xmax - px), fmin(py - s.ymin, s.ymax - py)));
        }
        best = w;
        elem = -1;
    }
    const double fx = x + (c * s.fcx - sn * s.fcy), fy = y + (sn * s.fcx + c * s.fcy);
    const double slack = s.slack + kCullSlack * (fabs(x) + fabs(y));
#pragma unroll 1
    for (int k = 0; k < s.n_poly; k++) {
        const double *pk = s.poly + (size_t)k * 4;
        if (culled(s, fmin(best, cap), slack, fx, fy, pk[0], pk[1], pk[2])) continue;
        const int code = (int)pk[3];
        const double v = poly_clearance(s, code >> 5, code & 31, x, y, c, sn);
        if (v < best) { best = v; elem = k; }
    }
#pragma unroll 1
    for (int k = 0; k < s.n_circle; k++) {
        const double *ck = s.circ + (size_t)k * 4;
        if (culled(s, fmin(best, cap), slack, fx, fy, ck[0], ck[1], ck[2])) continue;
        const double v = circle_clearance(s, ck[0], ck[1], ck[2], x, y, c, sn);
        if (v < best) { best = v; elem = s.n_poly + k; }
    }
    return best;
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
// The one packer of the block, for every kernel that reads a scene: where the parts begin (in doubles; the footprint rows, if
// any, begin at 0) and the block's length.  The staged and uploaded block is bytes() long: one more double behind n_dbl, so
// that an empty scene is still a block.  scene_fill writes h[0 .. n_dbl) only; that last double is zero because scene_stage
// clears the whole staged block, and no kernel reads it.
struct SceneLayout {
    int o_poly, o_pv, o_circ, n_dbl;
    size_t bytes() const { return ((size_t)n_dbl + 1) * sizeof(double); }
};
// scene_layout and scene_fill are the arithmetic, without a device call: the offsets, and every double of h[0 .. n_dbl) from
// a validated footprint (n_foot = 0: none) and scene (check_scene gives nv).  scene_block stages, fills and uploads the block
// on the context's stream (scene_stage, scene_upload: the only device calls); the block is then ctx->scene.ptr.
SceneLayout scene_layout(int n_foot, int n_poly, int nv, int n_circle);
void scene_fill(const SceneLayout &b, int n_foot, const double *h_foot, int n_poly, const int *h_poly_start, const double *h_poly_xy,
                int n_circle, const double *h_circles, double *h);
int scene_block(vap_ctx *ctx, int n_foot, const double *h_foot, int n_poly, const int *h_poly_start, const double *h_poly_xy,
                int n_circle, const double *h_circles, int nv, SceneLayout &b);
// scene_block for a validated footprint and scene (check_convex, check_scene give scale and nv), and `s` filled for a kernel
// on the context's stream.
int scene_pack(vap_ctx *ctx, int n_foot, const double *h_footprint, const double *h_field, int n_poly, const int *h_poly_start,
               const double *h_poly_xy, int n_circle, const double *h_circles, double scale, int nv, FootScene &s);

}  // namespace vap
