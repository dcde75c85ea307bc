// vap_conflict.h — what the robot-to-robot calls share: vap_conflict.hip (vap_footprint_conflicts, one start shift),
// vap_conflict_shifts.hip (vap_conflict_shifts, a window of them) and vap_schedule.hip (vap_schedule_tables, a delay in
// front of every slot of a routine).  The packed footprint and side, the pack kernel
// (defined in vap_conflict.hip), the exact polygon pair in one footprint's body frame and the bounding-circle cull.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "vap_footprint.h"

namespace vap {

constexpr int kConfTile = 16;                          // routes per side of a tile
constexpr int kConfThreads = kConfTile * kConfTile;    // one pair per thread
constexpr int kConfBlock = 64;                         // rows per bounding block and per LDS chunk
constexpr int kConfRouteStride = kConfBlock * 4 + 2;   // doubles per staged route: 16 routes' rows 16 banks apart

// One footprint: [n][8] = vertex x, y relative to the bounding circle's centre; outward unit normal of the edge to the
// next vertex; that edge; 1 / |edge|^2; the smallest projection of the vertices on that normal (the largest is the
// edge's own vertex).  cx, cy: the bounding circle's centre in the body frame; R its radius.
struct ConfFoot {
    double v[kFootMaxVerts * 8];
    double cx, cy, R;
    int n;
};

struct ConfSide {
    const double *rows;
    const int *counts;
    long cap;
    int stride, B;
    long shift;       // this side starts that many rows late
};

__device__ __forceinline__ long conf_count(const ConfSide &s, int b)
{
    const long n = s.counts[(size_t)b * s.stride];
    return n < 0 ? 0 : (n > s.cap ? s.cap : n);
}

// pack[b][Tp][4] = {cx, cy, cos, sin} of horizon row r (route row clamp(r - shift, 0, n - 1)); blk[b][nblk][4] = centre,
// radius of a circle around the 64 centres of a block, 0.  A wave per block.
__global__ __launch_bounds__(256) void k_conflict_pack(ConfSide s, double fcx, double fcy, long Tp, int nblk, int groups,
                                                       double *__restrict__ pack, double *__restrict__ blk);

// The separating-axis half over the edge normals of F, in F's frame; G's vertices sit at t + R(c, s) v.  Lowers sep to the
// smallest projection overlap seen; false as soon as an axis separates (or touches).
__device__ __forceinline__ bool sat_axes(const double *F, int nf, const double *G, int ng, double tx, double ty, double c,
                                         double s, double &sep)
{
#pragma unroll 1
    for (int i = 0; i < nf; i++) {
        const double nx = F[i * 8 + 2], ny = F[i * 8 + 3];
        const double gx = c * nx + s * ny, gy = c * ny - s * nx;    // the axis in G's frame
        double q0 = INFINITY, q1 = -INFINITY;
#pragma unroll 1
        for (int k = 0; k < ng; k++) {
            const double d = gx * G[k * 8 + 0] + gy * G[k * 8 + 1];
            q0 = fmin(q0, d);
            q1 = fmax(q1, d);
        }
        const double off = nx * tx + ny * ty;
        const double f1 = nx * F[i * 8 + 0] + ny * F[i * 8 + 1], f0 = F[i * 8 + 7];
        const double ov = fmin(f1, q1 + off) - fmax(f0, q0 + off);
        sep = fmin(sep, ov);
        if (!(ov > 0.0)) return false;
    }
    return true;
}

// vap.h's polygon clearance between footprint A at pose {ax, ay, ac, as} and footprint O at {ox, oy, oc, os} (the posed
// bounding-circle centres and the cos / sin of the body angles).
__device__ double pair_clearance(const double *FA, int na, const double *FO, int no, double ax, double ay, double ac, double as,
                                 double ox, double oy, double oc, double os)
{
    const double dx = ox - ax, dy = oy - ay;
    const double c = ac * oc + as * os, s = ac * os - as * oc;          // R(phi_o - phi_a)
    const double tx = ac * dx + as * dy, ty = ac * dy - as * dx;        // O's centre in A's frame
    // A NaN in either pose gives NaN: fmin and fmax drop a NaN operand, so sat_axes would see a footprint's own extent as
    // the overlap and report the deepest contact.  Every pose entry reaches c + s + tx + ty.
    const double any = (c + s) + (tx + ty);
    if (any != any) return NAN;
    double sep = INFINITY;
    bool overlap = sat_axes(FA, na, FO, no, tx, ty, c, s, sep);
    if (overlap) {
        const double ux = -(oc * dx + os * dy), uy = -(oc * dy - os * dx);   // A's centre in O's frame
        overlap = sat_axes(FO, no, FA, na, ux, uy, c, -s, sep);
    }
    if (overlap) return -sep;
    // separated or touching: the distance is attained between a vertex of one and an edge of the other (A's frame)
    double d2 = INFINITY;
#pragma unroll 1
    for (int k = 0; k < no; k++) {
        const double gx = FO[k * 8 + 0], gy = FO[k * 8 + 1], gex = FO[k * 8 + 4], gey = FO[k * 8 + 5], gil2 = FO[k * 8 + 6];
        const double px = tx + (c * gx - s * gy), py = ty + (s * gx + c * gy);
        const double ex = c * gex - s * gey, ey = s * gex + c * gey;
#pragma unroll 1
        for (int i = 0; i < na; i++) {
            const double vx = FA[i * 8 + 0], vy = FA[i * 8 + 1];
            d2 = fmin(d2, seg_dist2(vx, vy, px, py, ex, ey, gil2));                                   // A vertex i, O edge k
            d2 = fmin(d2, seg_dist2(px, py, vx, vy, FA[i * 8 + 4], FA[i * 8 + 5], FA[i * 8 + 6]));    // O vertex k, A edge i
        }
    }
    return sqrt(d2);
}

// skip when |d| > reach: the lower bound |d| - radii exceeds thresh + slack
__device__ __forceinline__ bool conf_culled(double reach, double dx, double dy)
{
    return reach < 0.0 || dx * dx + dy * dy > reach * reach;    // false for reach = +inf or NaN
}

static void conf_foot(const double *h, int n, ConfFoot &f)
{
    std::memset(&f, 0, sizeof f);
    bound_polygon(h, n, f.cx, f.cy, f.R);
    double rel[kFootMaxVerts * 2];
    for (int i = 0; i < n; i++) {
        rel[2 * i] = h[2 * i] - f.cx;
        rel[2 * i + 1] = h[2 * i + 1] - f.cy;
    }
    pack_polygon(rel, n, f.v);
    f.R = 0.0;
    for (int i = 0; i < n; i++) f.R = std::fmax(f.R, std::hypot(rel[2 * i], rel[2 * i + 1]));
    for (int i = 0; i < n; i++) {
        double lo = INFINITY;
        for (int j = 0; j < n; j++) lo = std::fmin(lo, f.v[i * 8 + 2] * rel[2 * j] + f.v[i * 8 + 3] * rel[2 * j + 1]);
        f.v[i * 8 + 7] = lo;
    }
    f.n = n;
}

}  // namespace vap
