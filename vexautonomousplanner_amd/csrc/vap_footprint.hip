// vap_footprint.hip — robot-footprint clearance of time-domain rows against a field scene (vap_footprint_clearance).
//
// The reference previews the robot's footprint (gui/path.py:764-809 PathWidget.draw_rect, the robot rectangle rotated
// to the path direction) but never checks it against anything.  This file checks it at every row of a batch of
// trajectories: the footprint polygon posed at (x, y) with body angle phi = -heading (MPG:555-563), against the field
// walls, convex polygons and circles of one scene shared by the whole batch.  Definitions: include/vap.h.
//
// One workgroup of kFootThreads per route; its threads stride over the route's rows (a wave holds 64 consecutive rows,
// which are close together on the field, so culling decisions agree across a wave most of the time).  Per row: the wall
// first, then the elements in id order, each skipped when its bounding-circle lower bound
// |c_obj - c_foot| - R_obj - R_foot exceeds the row's running best by more than a slack that covers rounding — so a
// skipped element could not have replaced the best, which changes only on a strictly smaller value: culling on and off
// give the same outputs bit for bit.  Then a wave argmin of (clearance, row), one across waves in LDS, one thread writes
// the route's outputs.  No reduction across workgroups.
//
// The scene (a few KB) lives in one device block read at wave-uniform addresses; rows are read with 8-byte loads of
// columns 4, 6 and 7 (the only columns the check needs).  The scene's layout and the per-row device functions are in
// vap_footprint.h: the rollout kernels take the clearance of their executed rows with them (vap_rollout_clearance.hip).
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "vap_footprint.h"

namespace vap {

constexpr int kFootThreads = 256;
constexpr int kFootWaves = kFootThreads / 64;

__global__ __launch_bounds__(kFootThreads) void k_footprint_clearance(FootScene s, long capacity, const double *__restrict__ rows,
                                                                      const int *__restrict__ counts, int counts_stride, double margin,
                                                                      double *__restrict__ row_out, double *__restrict__ min_c,
                                                                      int *__restrict__ min_row, int *__restrict__ min_el,
                                                                      int *__restrict__ first_row, int *__restrict__ n_below)
{
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    long n = counts[(size_t)b * counts_stride];
    n = n < 0 ? 0 : (n > capacity ? capacity : n);
    const double *__restrict__ R = rows + (size_t)b * (size_t)capacity * 8;
    double tbest = INFINITY;
    int trow = INT_MAX, tel = -1, tfirst = INT_MAX, tnb = 0;
#pragma unroll 1
    for (long r = tid; r < n; r += kFootThreads) {
        const double *row = R + (size_t)r * 8;
        int el;
        const double v = row_clearance(s, row[4], row[6], row[7], el);
        if (row_out) row_out[(size_t)b * (size_t)capacity + (size_t)r] = v;
        if (v < margin) {
            tnb++;
            if ((int)r < tfirst) tfirst = (int)r;
        }
        if (v < tbest) { tbest = v; trow = (int)r; tel = el; }    // rows ascend per thread: the first at the minimum stays
    }
    if (row_out) {
#pragma unroll 1
        for (long r = n + tid; r < capacity; r += kFootThreads) row_out[(size_t)b * (size_t)capacity + (size_t)r] = NAN;
    }
    // (clearance, row) argmin, first-row min and count: the wave, then the workgroup in LDS
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(tbest, off);
        const int orow = __shfl_xor(trow, off);
        const int oel = __shfl_xor(tel, off);
        if (ob < tbest || (ob == tbest && orow < trow)) { tbest = ob; trow = orow; tel = oel; }
        tfirst = min(tfirst, __shfl_xor(tfirst, off));
        tnb += __shfl_xor(tnb, off);
    }
    __shared__ double sb[kFootWaves];
    __shared__ int srow[kFootWaves], sel[kFootWaves], sfirst[kFootWaves], snb[kFootWaves];
    const int wave = tid / 64;
    if ((tid & 63) == 0) {
        sb[wave] = tbest;
        srow[wave] = trow;
        sel[wave] = tel;
        sfirst[wave] = tfirst;
        snb[wave] = tnb;
    }
    __syncthreads();
    if (tid == 0) {
        double best = sb[0];
        int brow = srow[0], bel = sel[0], first = sfirst[0], nb = snb[0];
        for (int w = 1; w < kFootWaves; w++) {
            if (sb[w] < best || (sb[w] == best && srow[w] < brow)) { best = sb[w]; brow = srow[w]; bel = sel[w]; }
            first = min(first, sfirst[w]);
            nb += snb[w];
        }
        const bool none = brow == INT_MAX;   // no rows (or no finite clearance)
        if (min_c) min_c[b] = none ? NAN : best;
        if (min_row) min_row[b] = none ? -1 : brow;
        if (min_el) min_el[b] = none ? -1 : bel;
        if (first_row) first_row[b] = first == INT_MAX ? -1 : first;
        if (n_below) n_below[b] = nb;
    }
}

// ---- host: scene validation and packing -------------------------------------------------------------------------

// A convex, counter-clockwise, simple polygon of 3..16 finite vertices with no collinear or duplicate vertices.
int check_convex(const double *v, int n, const char *what, int idx)
{
    if (n < 3 || n > kFootMaxVerts)
        return vap_fail(VAP_ERR_INVALID, "%s %d has %d vertices (3..%d)", what, idx, n, kFootMaxVerts);
    double turn = 0.0;
    for (int i = 0; i < n; i++) {
        const double *a = v + 2 * i, *b = v + 2 * ((i + 1) % n), *c = v + 2 * ((i + 2) % n);
        if (!std::isfinite(a[0]) || !std::isfinite(a[1])) return vap_fail(VAP_ERR_INVALID, "%s %d: non-finite vertex", what, idx);
        const double e1x = b[0] - a[0], e1y = b[1] - a[1], e2x = c[0] - b[0], e2y = c[1] - b[1];
        const double cr = e1x * e2y - e1y * e2x, dt = e1x * e2x + e1y * e2y;
        const double l1 = std::hypot(e1x, e1y), l2 = std::hypot(e2x, e2y);
        if (l1 == 0.0 || l2 == 0.0) return vap_fail(VAP_ERR_INVALID, "%s %d: duplicate vertex %d", what, idx, (i + 1) % n);
        if (std::fabs(cr) <= 1e-12 * l1 * l2) return vap_fail(VAP_ERR_INVALID, "%s %d: collinear vertices at %d", what, idx, (i + 1) % n);
        if (cr < 0.0) return vap_fail(VAP_ERR_INVALID, "%s %d: clockwise or non-convex at vertex %d (vertices must be counter-clockwise)",
                                      what, idx, (i + 1) % n);
        turn += std::atan2(cr, dt);
    }
    if (std::fabs(turn - 2.0 * M_PI) > 1e-6) return vap_fail(VAP_ERR_INVALID, "%s %d is not simple (it winds %.3f times)", what, idx, turn / (2.0 * M_PI));
    return VAP_OK;
}

// [n][8] rows of a polygon: x, y, outward unit normal of the edge to the next vertex, that edge, 1 / |edge|^2, 0
void pack_polygon(const double *v, int n, double *out)
{
    for (int i = 0; i < n; i++) {
        const double ax = v[2 * i], ay = v[2 * i + 1];
        const double ex = v[2 * ((i + 1) % n)] - ax, ey = v[2 * ((i + 1) % n) + 1] - ay;
        const double len = std::hypot(ex, ey);
        double *o = out + (size_t)i * 8;
        o[0] = ax;
        o[1] = ay;
        o[2] = ey / len;     // counter-clockwise: the outside is on the right of the edge
        o[3] = -ex / len;
        o[4] = ex;
        o[5] = ey;
        o[6] = 1.0 / (ex * ex + ey * ey);
        o[7] = 0.0;
    }
}

// centre (vertex mean) and bounding radius of a polygon
void bound_polygon(const double *v, int n, double &cx, double &cy, double &r)
{
    cx = cy = 0.0;
    for (int i = 0; i < n; i++) { cx += v[2 * i]; cy += v[2 * i + 1]; }
    cx /= n;
    cy /= n;
    r = 0.0;
    for (int i = 0; i < n; i++) r = std::fmax(r, std::hypot(v[2 * i] - cx, v[2 * i + 1] - cy));
}

// The field box, polygons and circles of a scene (include/vap.h, vap_footprint_clearance): limits and geometry.  scale: the
// largest coordinate magnitude; nv: the polygons' vertices together.  Host only, no device call.
int check_scene(const double *h_field, int n_poly, const int *h_poly_start, const double *h_poly_xy, int n_circle,
                const double *h_circles, double &scale, int &nv)
{
    if (n_poly < 0 || n_circle < 0) return vap_fail(VAP_ERR_INVALID, "negative element count");
    if (n_poly > kFootMaxPolys) return vap_fail(VAP_ERR_UNSUPPORTED, "%d polygons (at most %d)", n_poly, kFootMaxPolys);
    if (n_circle > kFootMaxCircles) return vap_fail(VAP_ERR_UNSUPPORTED, "%d circles (at most %d)", n_circle, kFootMaxCircles);
    scale = 0.0;
    if (h_field) {
        for (int i = 0; i < 4; i++) {
            if (!std::isfinite(h_field[i])) return vap_fail(VAP_ERR_INVALID, "non-finite field box");
            scale = std::fmax(scale, std::fabs(h_field[i]));
        }
        if (!(h_field[0] < h_field[2]) || !(h_field[1] < h_field[3]))
            return vap_fail(VAP_ERR_INVALID, "empty field box (%g, %g, %g, %g)", h_field[0], h_field[1], h_field[2], h_field[3]);
    }
    nv = 0;
    if (n_poly > 0) {
        if (!h_poly_start || !h_poly_xy) return vap_fail(VAP_ERR_INVALID, "null polygon arrays");
        if (h_poly_start[0] != 0) return vap_fail(VAP_ERR_INVALID, "poly_start[0] must be 0");
        for (int k = 0; k < n_poly; k++) {
            const int m = h_poly_start[k + 1] - h_poly_start[k];
            if (m < 3 || m > kFootMaxVerts) return vap_fail(VAP_ERR_INVALID, "polygon %d has %d vertices (3..%d)", k, m, kFootMaxVerts);
            if (h_poly_start[k + 1] > kFootMaxPolyVerts)
                return vap_fail(VAP_ERR_UNSUPPORTED, "more than %d polygon vertices", kFootMaxPolyVerts);
        }
        nv = h_poly_start[n_poly];
        for (int k = 0; k < n_poly; k++)
            VAP_TRY(check_convex(h_poly_xy + 2 * (size_t)h_poly_start[k], h_poly_start[k + 1] - h_poly_start[k], "polygon", k));
        for (int i = 0; i < 2 * nv; i++) scale = std::fmax(scale, std::fabs(h_poly_xy[i]));
    }
    if (n_circle > 0) {
        if (!h_circles) return vap_fail(VAP_ERR_INVALID, "null circles");
        for (int k = 0; k < n_circle; k++) {
            const double *ck = h_circles + 3 * (size_t)k;
            if (!std::isfinite(ck[0]) || !std::isfinite(ck[1]) || !std::isfinite(ck[2]))
                return vap_fail(VAP_ERR_INVALID, "circle %d is not finite", k);
            if (!(ck[2] > 0.0)) return vap_fail(VAP_ERR_INVALID, "circle %d has radius %g (must be > 0)", k, ck[2]);
            scale = std::fmax(scale, std::fabs(ck[0]) + std::fabs(ck[1]) + ck[2]);
        }
    }
    return VAP_OK;
}

// The pinned host block of the packed scene, at least `bytes` long and free of the previous upload, and room for it on
// the device (ctx->scene).
int scene_stage(vap_ctx *ctx, size_t bytes, double **h)
{
    if (!ctx->scene_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->scene_ev, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(ctx->scene_ev));      // the previous upload has left the host block
    if (bytes > ctx->scene_host_cap) {
        if (ctx->scene_host) HIP_TRY(hipHostFree(ctx->scene_host));
        ctx->scene_host = nullptr;
        ctx->scene_host_cap = 0;
        HIP_TRY(hipHostMalloc(&ctx->scene_host, bytes, hipHostMallocDefault));
        ctx->scene_host_cap = bytes;
    }
    VAP_TRY(ctx->ensure(ctx->scene, bytes));
    *h = (double *)ctx->scene_host;
    std::memset(*h, 0, bytes);
    return VAP_OK;
}

// Upload the staged block on the context's stream.
int scene_upload(vap_ctx *ctx, size_t bytes)
{
    HIP_TRY(hipMemcpyAsync(ctx->scene.ptr, ctx->scene_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->scene_ev, ctx->stream));
    return VAP_OK;
}

// Where the parts of the packed block begin: foot [n_foot][8] | poly [n_poly][4] | pv [nv][8] | circ [n_circle][4].  No device call.
SceneLayout scene_layout(int n_foot, int n_poly, int nv, int n_circle)
{
    SceneLayout b;
    b.o_poly = n_foot * 8;
    b.o_pv = b.o_poly + n_poly * 4;
    b.o_circ = b.o_pv + nv * 8;
    b.n_dbl = b.o_circ + n_circle * 4;
    return b;
}

// Every double of h[0 .. b.n_dbl) from a validated footprint (or none) and scene, in vap_footprint.h's layouts.  No device call.
void scene_fill(const SceneLayout &b, int n_foot, const double *h_foot, int n_poly, const int *h_poly_start, const double *h_poly_xy,
                int n_circle, const double *h_circles, double *h)
{
    if (n_foot > 0) pack_polygon(h_foot, n_foot, h);
    for (int k = 0; k < n_poly; k++) {
        const int p0 = h_poly_start[k], m = h_poly_start[k + 1] - p0;
        double *pk = h + b.o_poly + (size_t)k * 4, *rows = h + b.o_pv + (size_t)p0 * 8;
        bound_polygon(h_poly_xy + 2 * (size_t)p0, m, pk[0], pk[1], pk[2]);
        pk[3] = (double)(p0 * 32 + m);
        pack_polygon(h_poly_xy + 2 * (size_t)p0, m, rows);
        for (int e = 0; e < m; e++) rows[e * 8 + 7] = std::sqrt(rows[e * 8 + 4] * rows[e * 8 + 4] + rows[e * 8 + 5] * rows[e * 8 + 5]);
    }
    for (int k = 0; k < n_circle; k++) {
        double *ck = h + b.o_circ + (size_t)k * 4;
        for (int j = 0; j < 3; j++) ck[j] = h_circles[3 * (size_t)k + j];
        ck[3] = 0.0;
    }
}

// Stage, fill and upload the block of a validated footprint (n_foot = 0: none) and scene on the context's stream; the block is
// ctx->scene.ptr.
int scene_block(vap_ctx *ctx, int n_foot, const double *h_foot, int n_poly, const int *h_poly_start, const double *h_poly_xy,
                int n_circle, const double *h_circles, int nv, SceneLayout &b)
{
    b = scene_layout(n_foot, n_poly, nv, n_circle);
    double *h = nullptr;
    VAP_TRY(scene_stage(ctx, b.bytes(), &h));
    scene_fill(b, n_foot, h_foot, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, h);
    return scene_upload(ctx, b.bytes());
}

// The packed scene of a validated footprint and scene on the device, and `s` filled for a kernel on the context's stream.
int scene_pack(vap_ctx *ctx, int n_foot, const double *h_footprint, const double *h_field, int n_poly, const int *h_poly_start,
               const double *h_poly_xy, int n_circle, const double *h_circles, double scale, int nv, FootScene &s)
{
    SceneLayout b;
    VAP_TRY(scene_block(ctx, n_foot, h_footprint, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, nv, b));
    bound_polygon(h_footprint, n_foot, s.fcx, s.fcy, s.fR);
    const double *d = (const double *)ctx->scene.ptr;
    s.foot = d;
    s.poly = d + b.o_poly;
    s.pv = d + b.o_pv;
    s.circ = d + b.o_circ;
    s.has_field = h_field ? 1 : 0;
    s.xmin = h_field ? h_field[0] : 0.0;
    s.ymin = h_field ? h_field[1] : 0.0;
    s.xmax = h_field ? h_field[2] : 0.0;
    s.ymax = h_field ? h_field[3] : 0.0;
    s.slack = kCullSlack * (1.0 + scale + s.fR);
    s.n_foot = n_foot;
    s.n_poly = n_poly;
    s.n_circle = n_circle;
    s.cull = ctx->footprint_cull;
    return VAP_OK;
}

}  // namespace vap

extern "C" {

int vap_footprint_clearance(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                            int n_foot, const double *h_footprint, const double *h_field, int n_poly, const int *h_poly_start,
                            const double *h_poly_xy, int n_circle, const double *h_circles, double margin,
                            double *d_row_clearance, double *d_min_clearance, int *d_min_row, int *d_min_element,
                            int *d_first_row, int *d_n_below)
{
    using namespace vap;
    VAP_TRY(vap_set_device(ctx));
    if (B < 0 || capacity < 0) return vap_fail(VAP_ERR_INVALID, "bad shape B=%d capacity=%ld", B, capacity);
    if (capacity > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld above %d rows", capacity, INT_MAX);
    if (counts_stride < 1) return vap_fail(VAP_ERR_INVALID, "counts_stride must be >= 1 (got %d)", counts_stride);
    if (B > 0 && (!d_counts || (capacity > 0 && !d_rows))) return vap_fail(VAP_ERR_INVALID, "null rows / counts");
    if (!std::isfinite(margin)) return vap_fail(VAP_ERR_INVALID, "margin must be finite");
    // the scene
    if (!h_footprint) return vap_fail(VAP_ERR_INVALID, "null footprint");
    VAP_TRY(check_convex(h_footprint, n_foot, "footprint", 0));
    double scale = 0.0;
    int nv = 0;
    VAP_TRY(check_scene(h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, scale, nv));
    if (B == 0) return VAP_OK;

    FootScene s;
    VAP_TRY(scene_pack(ctx, n_foot, h_footprint, h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, scale, nv, s));
    hipLaunchKernelGGL(k_footprint_clearance, dim3(B), dim3(kFootThreads), 0, ctx->stream, s, capacity, d_rows, d_counts,
                       counts_stride, margin, d_row_clearance, d_min_clearance, d_min_row, d_min_element, d_first_row, d_n_below);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
