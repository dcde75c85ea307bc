// vap_occupancy.hip — time-domain rows rasterised onto the planner's grid (vap_plan_occupancy).
//
// The reference poses the robot's footprint in one place only (gui/path.py:764-809 PathWidget.draw_rect) and never asks
// which part of the field a routine occupies, or when.  This file does: every row of a batch of routes is posed as
// vap_footprint_clearance poses it, the clearance of every cell centre of vap_plan_grid's grid against the posed polygon is
// that call's polygon formula minus the disc's radius, and per cell the first and last covering instant, the number of
// covering rows and the smallest clearance come out.  Definitions: include/vap.h.
//
//   k_occ_init      the never-covered values (INT_MAX, INT_MIN, 0, the key of +inf).
//   k_occupancy     a work item is a chunk of 64 consecutive rows of one route; workgroups of 256 threads take work items
//                   w = block, block + grid, ...
//                     pose    wave 0, a lane per row: sincos once, the posed vertices, then per edge the edge vector,
//                             1 / |e|^2 and |e| — six doubles an edge in LDS (n_foot x 48 B a row, 12 KB a chunk for a
//                             rectangle, 48 KB for 16 vertices) — and the row's position and squared reach (NaN for a
//                             row that takes no part: a non-finite pose, or one so large that an edge has |e|^2 = 0).  A wave
//                             min / max of (position -+ reach) gives the chunk's box and from it a range of cells.
//                     test    a thread per cell of that range (of the whole grid when the minimum is asked for), a loop
//                             over the chunk's rows at wave-uniform LDS addresses (broadcast reads).  A row is skipped
//                             when the cell centre is farther from its position than the reach (it cannot cover) and,
//                             for the minimum, when its lower bound |p - o| - R_foot - radius exceeds the cell's running
//                             minimum; both bounds carry a slack that covers rounding, so a skipped pair could not have
//                             changed an output: culling on and off give the same bits.
//                     merge   per cell and chunk one integer atomicMin / atomicMax / atomicAdd, and for the minimum an
//                             atomicMin on the sortable 64-bit key of the double (k_search_update's order).  They commute:
//                             two calls give the same bits.  A plain load of the cell's current value first: the values
//                             only fall (rise), so a stale one culls less, never wrongly, and an atomic that cannot
//                             change the value is not sent.
//   k_occ_finish    the keys back into doubles, in place.
// No floating-point atomic anywhere.
#include <climits>
#include <cmath>
#include <cstdint>

#include "vap_plan.h"

namespace vap {

constexpr int kOccThreads = 256;
constexpr int kOccChunk = 64;           // rows per work item: one wave poses them
constexpr int kOccMaxBlocks = 1 << 16;
constexpr int kOccEdge = 6;             // doubles per posed edge: ax, ay, ex, ey, 1 / |e|^2, |e|
constexpr int kOccRow = 4;              // doubles per row: x, y, squared reach, slack

struct OccArgs {
    PlanGrid g;
    const double *rows;
    const int *counts;
    long capacity, chunks, total;       // chunks per route; work items
    int counts_stride, n_foot;
    double foot[2 * kFootMaxVerts];     // body-frame vertices
    double fR;                          // the largest |vertex|
    double radius, margin, slack;
    int shift, hold_first, hold_last, cull;
    int *first, *last, *count;
    unsigned long long *minkey;
};

// a double's bits as an unsigned key whose integer order is the order of the doubles, and back (as in vap_search.hip)
__device__ __forceinline__ unsigned long long occ_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double occ_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(kOccThreads) void k_occ_init(int ncell, int *first, int *last, int *count, unsigned long long *minkey)
{
    const int idx = blockIdx.x * kOccThreads + threadIdx.x;
    if (idx >= ncell) return;
    if (first) first[idx] = INT_MAX;
    if (last) last[idx] = INT_MIN;
    if (count) count[idx] = 0;
    if (minkey) minkey[idx] = occ_key(INFINITY);
}

__global__ __launch_bounds__(kOccThreads) void k_occ_finish(int ncell, unsigned long long *minkey)
{
    const int idx = blockIdx.x * kOccThreads + threadIdx.x;
    if (idx < ncell) reinterpret_cast<double *>(minkey)[idx] = occ_value(minkey[idx]);
}

// the range of cell indices whose centres lie in [lo, hi], one cell wider either way, clamped to 0 .. n - 1
__device__ __forceinline__ void occ_range(double lo, double hi, double origin, double cell, int n, int &i0, int &i1)
{
    double a = floor((lo - origin) / cell - 0.5) - 1.0, b = ceil((hi - origin) / cell - 0.5) + 1.0;
    a = a > 0.0 ? (a < (double)n ? a : (double)n) : 0.0;             // NaN: 0
    b = b < (double)(n - 1) ? (b > -1.0 ? b : -1.0) : (double)(n - 1);   // NaN: n - 1
    i0 = (int)a;
    i1 = (int)b;
}

__global__ __launch_bounds__(kOccThreads) void k_occupancy(OccArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double occ_lds[];
    __shared__ double s_box[4];
    const PlanGrid g = a.g;
    const int tid = threadIdx.x, nf = a.n_foot;
    double *s_row = occ_lds;                                         // [kOccChunk][kOccRow]
    double *s_edge = occ_lds + kOccChunk * kOccRow;                  // [kOccChunk][nf][kOccEdge]
    const bool want_min = a.minkey != nullptr;
    const double reach0 = a.fR + a.radius + a.margin;                // a row covers nothing farther from its position

#pragma unroll 1
    for (long w = blockIdx.x; w < a.total; w += gridDim.x) {
        const long b = w / a.chunks;
        const long r0 = (w - b * a.chunks) * kOccChunk;
        long n = a.counts[(size_t)b * a.counts_stride];
        n = n < 0 ? 0 : (n > a.capacity ? a.capacity : n);
        if (r0 >= n) continue;                                       // the same in every thread
        const int nr = (int)(n - r0 < kOccChunk ? n - r0 : kOccChunk);
        __syncthreads();                                             // the previous work item is done with the LDS
        if (tid < kOccChunk) {
            double bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
            if (tid < nr) {
                const double *row = a.rows + ((size_t)b * (size_t)a.capacity + (size_t)(r0 + tid)) * 8;
                const double heading = row[4], x = row[6], y = row[7];
                double sn, c;
                sincos(-heading, &sn, &c);
                double *e = s_edge + (size_t)tid * nf * kOccEdge;
                bool posed = isfinite(heading) && isfinite(x) && isfinite(y);
                for (int i = 0; i < nf; i++) {
                    const double bx = a.foot[2 * i], by = a.foot[2 * i + 1];
                    e[i * kOccEdge + 0] = x + (c * bx - sn * by);
                    e[i * kOccEdge + 1] = y + (sn * bx + c * by);
                }
                for (int i = 0; i < nf; i++) {
                    const int k = i + 1 < nf ? i + 1 : 0;
                    const double ex = e[k * kOccEdge + 0] - e[i * kOccEdge + 0], ey = e[k * kOccEdge + 1] - e[i * kOccEdge + 1];
                    const double ll = ex * ex + ey * ey;
                    e[i * kOccEdge + 2] = ex;
                    e[i * kOccEdge + 3] = ey;
                    e[i * kOccEdge + 4] = 1.0 / ll;
                    e[i * kOccEdge + 5] = sqrt(ll);
                    posed = posed && ll > 0.0 && ll < INFINITY;     // a pose so large that the vertices fall together
                }
                const double slack = a.slack + kCullSlack * (fabs(x) + fabs(y));
                const double reach = reach0 + slack;
                s_row[tid * kOccRow + 0] = x;
                s_row[tid * kOccRow + 1] = y;
                s_row[tid * kOccRow + 2] = posed ? (reach >= 0.0 ? reach * reach : -1.0) : NAN;    // NaN: the row is left out
                s_row[tid * kOccRow + 3] = slack;
                if (posed) {
                    const double rr = reach >= 0.0 ? reach : 0.0;
                    bx0 = x - rr;
                    bx1 = x + rr;
                    by0 = y - rr;
                    by1 = y + rr;
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                bx0 = fmin(bx0, __shfl_xor(bx0, off));
                bx1 = fmax(bx1, __shfl_xor(bx1, off));
                by0 = fmin(by0, __shfl_xor(by0, off));
                by1 = fmax(by1, __shfl_xor(by1, off));
            }
            if (tid == 0) {
                s_box[0] = bx0;
                s_box[1] = bx1;
                s_box[2] = by0;
                s_box[3] = by1;
            }
        }
        __syncthreads();
        // the cells a row of the chunk can cover
        int ci0 = 0, ci1 = g.nx - 1, cj0 = 0, cj1 = g.ny - 1;
        if (a.cull) {
            occ_range(s_box[0], s_box[1], g.xmin, g.cell, g.nx, ci0, ci1);
            occ_range(s_box[2], s_box[3], g.ymin, g.cell, g.ny, cj0, cj1);
        }
        const bool some = ci0 <= ci1 && cj0 <= cj1;
        // the cells this work item visits: those, or every cell for the minimum
        const int vi0 = want_min ? 0 : ci0, vi1 = want_min ? g.nx - 1 : ci1, vj0 = want_min ? 0 : cj0, vj1 = want_min ? g.ny - 1 : cj1;
        const int vw = vi1 - vi0 + 1, vn = (vi1 >= vi0 && vj1 >= vj0) ? vw * (vj1 - vj0 + 1) : 0;
#pragma unroll 1
        for (int t = tid; t < vn; t += kOccThreads) {
            const int jj = t / vw, i = vi0 + (t - jj * vw), j = vj0 + jj, idx = j * g.nx + i;
            const double px = plan_centre(g.xmin, i, g.cell), py = plan_centre(g.ymin, j, g.cell);
            const bool near = some && i >= ci0 && i <= ci1 && j >= cj0 && j <= cj1;
            double cur = INFINITY;
            if (want_min) cur = occ_value(__atomic_load_n(&a.minkey[idx], __ATOMIC_RELAXED));
            if (!near) {
                if (!want_min) continue;
                // the whole chunk against the running minimum: the box holds every row's circle of radius max(reach, 0)
                // round its position o, so |p - o| >= distance to the box + that radius, and the row's clearance, at
                // least |p - o| - R_foot - radius, exceeds the distance to the box + margin (the slack covers rounding)
                const double ddx = fmax(fmax(s_box[0] - px, px - s_box[1]), 0.0), ddy = fmax(fmax(s_box[2] - py, py - s_box[3]), 0.0);
                if (a.cull && sqrt(ddx * ddx + ddy * ddy) + a.margin > cur) continue;
            }
            double best = cur;
            int first = INT_MAX, last = INT_MIN, cnt = 0;
#pragma unroll 1
            for (int k = 0; k < nr; k++) {
                const double *rw = s_row + k * kOccRow;
                if (rw[2] != rw[2]) continue;                        // a non-finite or collapsed pose
                if (a.cull) {
                    const double dx = px - rw[0], dy = py - rw[1], d2c = dx * dx + dy * dy;
                    bool need = d2c <= rw[2];                        // may cover
                    if (!need && want_min) {                         // may lower the minimum: |p - o| <= best + R + radius + slack
                        const double q = best + (a.fR + a.radius + rw[3]);
                        need = q >= 0.0 && !(d2c > q * q);
                    }
                    if (!need) continue;
                }
                const double *e = s_edge + (size_t)k * nf * kOccEdge;
                double smax = -INFINITY, d2 = INFINITY;
#pragma unroll 1
                for (int v = 0; v < nf; v++, e += kOccEdge) {
                    const double wx = px - e[0], wy = py - e[1];
                    smax = fmax(smax, (wx * e[3] - wy * e[2]) / e[5]);
                    d2 = fmin(d2, seg_dist2(px, py, e[0], e[1], e[2], e[3], e[4]));
                }
                const double c = (smax > 0.0 ? sqrt(d2) : smax) - a.radius;
                if (c < a.margin) {
                    const long r = r0 + k;
                    const int inst = (int)(r + a.shift);
                    cnt++;
                    first = min(first, (r == 0 && a.hold_first) ? INT_MIN : inst);
                    last = max(last, (r == n - 1 && a.hold_last) ? INT_MAX : inst);
                }
                if (c < best) best = c;
            }
            if (cnt) {
                if (a.first && first < __atomic_load_n(&a.first[idx], __ATOMIC_RELAXED)) atomicMin(&a.first[idx], first);
                if (a.last && last > __atomic_load_n(&a.last[idx], __ATOMIC_RELAXED)) atomicMax(&a.last[idx], last);
                if (a.count) atomicAdd(&a.count[idx], cnt);
            }
            if (want_min && best < cur) atomicMin(&a.minkey[idx], occ_key(best));
        }
    }
}

}  // namespace vap

extern "C" {

int vap_plan_occupancy(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride, int n_foot,
                       const double *h_footprint, const double *h_field, double cell, double radius, double margin, int shift_rows,
                       int hold_first, int hold_last, int *d_first, int *d_last, int *d_count, double *d_min_clearance, int *nx_out,
                       int *ny_out)
{
    using namespace vap;
    if (B < 0 || capacity < 0) return vap_fail(VAP_ERR_INVALID, "bad shape B=%d capacity=%ld", B, capacity);
    if (capacity >= INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld: at most %d rows", capacity, INT_MAX - 1);
    // every instant lies strictly between the two hold values
    if ((long)shift_rows <= (long)INT_MIN || (long)shift_rows + capacity >= (long)INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "shift_rows %d with capacity %ld leaves the int32 instants", shift_rows, capacity);
    if (counts_stride < 1) return vap_fail(VAP_ERR_INVALID, "counts_stride must be >= 1 (got %d)", counts_stride);
    if (B > 0 && (!d_counts || (capacity > 0 && !d_rows))) return vap_fail(VAP_ERR_INVALID, "null rows / counts");
    if (!(cell > 0.0) || !std::isfinite(cell)) return vap_fail(VAP_ERR_INVALID, "cell must be positive and finite (got %g)", cell);
    if (!(radius >= 0.0) || !std::isfinite(radius)) return vap_fail(VAP_ERR_INVALID, "radius must be >= 0 and finite (got %g)", radius);
    if (!std::isfinite(margin)) return vap_fail(VAP_ERR_INVALID, "margin must be finite");
    if (!h_footprint) return vap_fail(VAP_ERR_INVALID, "null footprint");
    VAP_TRY(check_convex(h_footprint, n_foot, "footprint", 0));
    if (!h_field) return vap_fail(VAP_ERR_INVALID, "the occupancy needs a field box");
    double scale = 0.0;
    int nv = 0;
    VAP_TRY(check_scene(h_field, 0, nullptr, nullptr, 0, nullptr, scale, nv));
    OccArgs a{};
    VAP_TRY(plan_grid_of(h_field, cell, a.g));
    if (nx_out) *nx_out = a.g.nx;
    if (ny_out) *ny_out = a.g.ny;
    if (!d_first && !d_last && !d_count && !d_min_clearance) return VAP_OK;     // the shape only
    VAP_TRY(vap_set_device(ctx));

    const int ncell = a.g.nx * a.g.ny, cells_blocks = (ncell + kOccThreads - 1) / kOccThreads;
    unsigned long long *minkey = reinterpret_cast<unsigned long long *>(d_min_clearance);
    hipLaunchKernelGGL(k_occ_init, dim3(cells_blocks), dim3(kOccThreads), 0, ctx->stream, ncell, d_first, d_last, d_count, minkey);
    HIP_TRY(hipGetLastError());
    a.chunks = (capacity + kOccChunk - 1) / kOccChunk;
    a.total = (long)B * a.chunks;
    if (a.total > 0) {
        a.rows = d_rows;
        a.counts = d_counts;
        a.capacity = capacity;
        a.counts_stride = counts_stride;
        a.n_foot = n_foot;
        a.fR = 0.0;
        for (int i = 0; i < n_foot; i++) {
            a.foot[2 * i] = h_footprint[2 * i];
            a.foot[2 * i + 1] = h_footprint[2 * i + 1];
            a.fR = std::fmax(a.fR, std::hypot(h_footprint[2 * i], h_footprint[2 * i + 1]));
        }
        a.radius = radius;
        a.margin = margin;
        // the last column or row may reach past the box by up to a cell
        a.slack = kCullSlack * (1.0 + scale + cell + a.fR + radius + std::fabs(margin));
        a.shift = shift_rows;
        a.hold_first = hold_first != 0;
        a.hold_last = hold_last != 0;
        a.cull = ctx->footprint_cull;
        a.first = d_first;
        a.last = d_last;
        a.count = d_count;
        a.minkey = minkey;
        const size_t lds = (size_t)kOccChunk * (kOccRow + (size_t)n_foot * kOccEdge) * sizeof(double);   // <= 50 KB
        const long blocks = a.total < kOccMaxBlocks ? a.total : kOccMaxBlocks;
        hipLaunchKernelGGL(k_occupancy, dim3((unsigned)blocks), dim3(kOccThreads), lds, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (minkey) {
        hipLaunchKernelGGL(k_occ_finish, dim3(cells_blocks), dim3(kOccThreads), 0, ctx->stream, ncell, minkey);
        HIP_TRY(hipGetLastError());
    }
    return VAP_OK;
}

}  // extern "C"
