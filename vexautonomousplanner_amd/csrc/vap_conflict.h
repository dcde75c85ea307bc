// vap_conflict.h — what the robot-to-robot calls share: vap_conflict.hip (vap_footprint_conflicts, one start shift),
// vap_conflict_shifts.hip (vap_conflict_shifts, a window of them) and vap_schedule.hip (vap_schedule_tables, a delay in
// front of every slot of a routine).
// Device: the packed footprint and side, the packed pose of a row (conf_pose, which the rollout lanes of
// vap_rollout_conflicts form on the chip), the pack kernel (defined in vap_conflict.hip), the exact polygon pair in one
// footprint's body frame (pair_clearance; pair_at on two packed rows), the bounding-circle cull of a row and of a 64-row
// block (row_culled, block_culled), minima as integer keys (conf_key / conf_unkey), clampl, floordiv64, wave_min / wave_max.
// Host: ConfInput (a side as an entry point receives it), the shared argument checks (conf_check_shape, conf_check_sides),
// ConfPacked (the shared kernel arguments) and conf_pack_sides (scratch, footprints, slack, fields, the two pack launches).
// The band sweep of the two window calls is in vap_band_sweep.h.
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

// The kernel arguments the three calls share (conf_pack_sides fills them); each call's own block derives from it.  The
// field order is measured, not taste: with cull in front of slack k_schedule_sweep spills 38 SGPRs instead of 35.
struct ConfPacked {
    const double *pack_a, *pack_o, *blk_a, *blk_o;
    ConfSide a, o;
    long Tpa, Tpo;            // packed rows per route
    int nblk_a, nblk_o;       // bounding blocks per route
    double slack;             // kCullSlack * (1 + R_a + R_o)
    int cull;
};

__device__ __forceinline__ long floordiv64(long x) { return x >= 0 ? x / 64 : -((63 - x) / 64); }
__device__ __forceinline__ long clampl(long x, long lo, long hi) { return x < lo ? lo : (x > hi ? hi : x); }

// an order-preserving map of doubles (no NaN) to unsigned 64-bit keys, and back: a minimum of doubles as an integer atomic
__device__ __forceinline__ unsigned long long conf_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double conf_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

template <typename T>
__device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// The packed pose {cx, cy, cos, sin} of a row (heading, x, y): cos and sin of the body angle -heading and the posed centre
// of the footprint's bounding circle, (fcx, fcy) in the body frame.  The pack kernel and the rollout lanes
// (vap_rollout_conflicts) both call this, so a pose formed on the chip has the bits of the same row packed from memory.
__device__ __forceinline__ void conf_pose(double heading, double x, double y, double fcx, double fcy, double &cx, double &cy, double &c,
                                          double &sn)
{
    sincos(-heading, &sn, &c);
    cx = x + (c * fcx - sn * fcy);
    cy = y + (sn * fcx + c * fcy);
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

// the clearance of two packed poses; rows of four doubles, 16-byte aligned
__device__ __forceinline__ double pair_at(const double *sfa, int na, const double *sfo, int no, const double *ra, const double *ro)
{
    const double2 a01 = *(const double2 *)ra, a23 = *(const double2 *)(ra + 2);
    const double2 o01 = *(const double2 *)ro, o23 = *(const double2 *)(ro + 2);
    return pair_clearance(sfa, na, sfo, no, a01.x, a01.y, a23.x, a23.y, o01.x, o01.y, o23.x, o23.y);
}

// skip when |d| > reach: the lower bound |d| - radii exceeds thresh + slack
__device__ __forceinline__ bool conf_culled(double reach, double dx, double dy)
{
    return reach < 0.0 || dx * dx + dy * dy > reach * reach;    // false for reach = +inf or NaN
}

// A row whose posed circle centres are (ax, ay) and (ox, oy) cannot come to thresh or below: radii = R_a + R_o, the slack
// grows with the coordinates' magnitude.
__device__ __forceinline__ bool row_culled(const ConfPacked &g, double radii, double thresh, double ax, double ay, double ox, double oy)
{
    const double slack = g.slack + kCullSlack * (fabs(ax) + fabs(ay) + fabs(ox) + fabs(oy));
    return conf_culled(thresh + slack + radii, ox - ax, oy - ay);
}
// The same for two 64-row blocks, from their circles (centre, radius ar / orr): no row of the two can.
__device__ __forceinline__ bool block_culled(const ConfPacked &g, double radii, double thresh, double ax, double ay, double ar, double ox,
                                             double oy, double orr)
{
    const double slack = g.slack + kCullSlack * (fabs(ax) + fabs(ay) + fabs(ox) + fabs(oy) + ar + orr);
    return conf_culled(thresh + slack + radii + ar + orr, ox - ax, oy - ay);
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

// ---- host: what the three entry points check and set up alike ------------------------------------------------------------
// one side of a call, as the entry point received it
struct ConfInput {
    int B;
    long cap;
    const double *rows;
    const int *counts;
    int stride, n_foot;
    const double *foot;
};

// `name_a`: what the entry point calls side A's route count ("Ba", "R")
static int conf_check_shape(const char *name_a, const ConfInput &a, const ConfInput &o)
{
    if (a.B < 0 || o.B < 0 || a.cap < 0 || o.cap < 0)
        return vap_fail(VAP_ERR_INVALID, "bad shape %s=%d cap_a=%ld Bo=%d cap_o=%ld", name_a, a.B, a.cap, o.B, o.cap);
    return VAP_OK;
}

// Everything else about the two sides, in the order the entry points report it.  `Bo_used`: side O's routes as far as its
// pointers are needed; `other_null`: a further pointer of the entry point's that is null though needed, reported with the
// rows and counts under `nulls`.
static int conf_check_sides(const ConfInput &a, const ConfInput &o, int Bo_used, bool matched, double margin, bool other_null,
                            const char *nulls)
{
    if (a.stride < 1 || o.stride < 1) return vap_fail(VAP_ERR_INVALID, "count strides must be >= 1 (got %d, %d)", a.stride, o.stride);
    if (matched && a.B != o.B) return vap_fail(VAP_ERR_INVALID, "matched pairing needs Ba == Bo (got %d, %d)", a.B, o.B);
    if (other_null || (a.B > 0 && (!a.counts || (a.cap > 0 && !a.rows))) || (Bo_used > 0 && (!o.counts || (o.cap > 0 && !o.rows))))
        return vap_fail(VAP_ERR_INVALID, "%s", nulls);
    if (!std::isfinite(margin)) return vap_fail(VAP_ERR_INVALID, "margin must be finite");
    if (!a.foot || !o.foot) return vap_fail(VAP_ERR_INVALID, "null footprint");
    VAP_TRY(check_convex(a.foot, a.n_foot, "footprint", 0));
    VAP_TRY(check_convex(o.foot, o.n_foot, "footprint", 1));
    return VAP_OK;
}

// the packed horizon of `rows` rows (at least one block): 64-row blocks, packed rows, pack workgroups per route
struct ConfHorizon {
    long nblk, Tp;
    int groups;
};
static ConfHorizon conf_horizon(long rows)
{
    const long nblk = ((rows < 1 ? 1 : rows) + kConfBlock - 1) / kConfBlock;
    return ConfHorizon{nblk, nblk * kConfBlock, (int)((nblk + 3) / 4)};
}

// Pack both sides on the context's stream, side O starting shift_o rows late: the scratch, the two footprints, and the
// fields of ConfPacked.  A side without routes is not launched.
static int conf_pack_sides(vap_ctx *ctx, const ConfInput &a, const ConfInput &o, long shift_o, const ConfHorizon &ha, const ConfHorizon &ho,
                           ConfFoot &fa, ConfFoot &fo, ConfPacked &g)
{
    VAP_TRY(ctx->ensure(ctx->conf_pack_a, (size_t)a.B * (size_t)ha.Tp * 32));
    VAP_TRY(ctx->ensure(ctx->conf_pack_o, (size_t)o.B * (size_t)ho.Tp * 32));
    VAP_TRY(ctx->ensure(ctx->conf_blk_a, (size_t)a.B * (size_t)ha.nblk * 32));
    VAP_TRY(ctx->ensure(ctx->conf_blk_o, (size_t)o.B * (size_t)ho.nblk * 32));
    conf_foot(a.foot, a.n_foot, fa);
    conf_foot(o.foot, o.n_foot, fo);
    g.a = ConfSide{a.rows, a.counts, a.cap, a.stride, a.B, 0};
    g.o = ConfSide{o.rows, o.counts, o.cap, o.stride, o.B, shift_o};
    g.pack_a = (const double *)ctx->conf_pack_a.ptr;
    g.pack_o = (const double *)ctx->conf_pack_o.ptr;
    g.blk_a = (const double *)ctx->conf_blk_a.ptr;
    g.blk_o = (const double *)ctx->conf_blk_o.ptr;
    g.Tpa = ha.Tp;
    g.Tpo = ho.Tp;
    g.nblk_a = (int)ha.nblk;
    g.nblk_o = (int)ho.nblk;
    g.cull = ctx->footprint_cull;
    g.slack = kCullSlack * (1.0 + fa.R + fo.R);
    const auto pack = [&](const ConfSide &s, const ConfFoot &f, const ConfHorizon &h, const double *rows, const double *blocks) {
        if (s.B > 0)
            hipLaunchKernelGGL(k_conflict_pack, dim3((unsigned)((long)s.B * h.groups)), dim3(256), 0, ctx->stream, s, f.cx, f.cy, h.Tp,
                               (int)h.nblk, h.groups, (double *)rows, (double *)blocks);
    };
    pack(g.a, fa, ha, g.pack_a, g.blk_a);
    pack(g.o, fo, ho, g.pack_o, g.blk_o);
    return VAP_OK;
}

}  // namespace vap
