// vap_plan.hip — seed routes through a scene on a grid (vap_plan_grid, vap_plan_seeds, vap_plan_travel).
//
// The route search refines a route that is already roughly right; this file finds one.  The robot is a disc of radius
// rho on a grid over the field box; a cell is free when the disc at its centre clears the walls, polygons and circles by
// the margin; an 8-connected shortest-path field from the goal's cell, a steepest-descent trace from the start's, a
// line-of-sight pull of the traced cells and an equal-arc resample give W waypoints per (start, goal) pair.  Every
// decision is an integer comparison or a comparison of single IEEE additions, so the result does not depend on the order
// of the work.  Definitions: include/vap.h.
//
//   k_plan_clearance  a thread per cell.  The polygons pass through LDS 32 at a time (their packed edge rows, 32 KB), the
//                     circles in one piece (8 KB); a thread walks them at wave-uniform LDS addresses (broadcast reads).
//   k_plan_seeds      persistent workgroups of 1024 threads, each taking problems r = block, block + grid, ...  LDS holds
//                     the whole distance field (8 B a cell, 128 KB at the 16384-cell limit), the free mask as bits (2 KB)
//                     and, per cell, the byte of its allowed moves (16 KB) — both built once per workgroup, since every
//                     problem shares the scene: 146 KB of gfx950's 160 KB, one workgroup per CU at the limit.
//                     With an occupancy (vap_plan_seeds_occupied) the static bits stay where they are and a second
//                     bitset (2 KB more: 148 KB) holds the problem's own mask, static bits minus the cells occupied in
//                     the problem's window; it and the move bytes are rebuilt per problem, from LDS and 8 B a cell of
//                     L2-resident occupancy.  Without one the kernel runs as before, on the static bits.
//                       relax   Jacobi sweeps: a read phase (each thread keeps the new values of its <= 16 cells in
//                               registers), a barrier, a write phase, and __syncthreads_or of "changed" as the second
//                               barrier.  Neighbours are at constant offsets; the move byte has done the bounds, the
//                               free test and the no-corner-cutting rule once.
//                       snap    a workgroup argmin over (distance^2, cell index): wave shuffles, then 16 partials in LDS.
//                       trace   one lane; the cell list goes to a global workspace (the LDS has no room for a worst-case
//                               list), one list per resident workgroup.
//                       pull    candidates b = n-1, n-2, ... one per lane, 1024 at a time; a lane runs the integer
//                               supercover test along the major axis (at most four cells per step can satisfy it); the
//                               largest visible b is an integer atomicMax in LDS.  The pulled list overwrites the front of
//                               the traced one.
//                       resample  segment lengths a thread each, their running sum on one lane (a fixed order), then a
//                               thread per waypoint.  The sums live where the distance field was.
//                     No float atomics: two calls give the same bits.
//   k_plan_travel     all ordered pairs of a problem's P points: the same workgroups over the R x P (problem, goal) items.
//                     An item relaxes its goal's field once and keeps it in LDS while every start is snapped, traced,
//                     pulled and resampled against it, so the sums live in the workgroup's global workspace, in front of
//                     its cell list.  The mask and the moves are rebuilt only when the workgroup's next item belongs to
//                     another problem (and only with an occupancy).
// Both kernels run a problem through one core: PlanLds states the dynamic LDS once for the kernels and the
// host; plan_begin (the carve, the static bits, the moves), plan_problem_mask, plan_admit, plan_goal, plan_start and
// plan_store_waypoints string the stages together, so a travel entry is the seeds' route by construction.  A kernel keeps
// its loop, where the sums live and its own outputs.  On the host plan_prepare carries what the two entry points share
// behind their shape checks, and the scene goes to the device through scene_block (vap_footprint.h) like every other scene.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "vap_kernels.h"
#include "vap_plan.h"

namespace vap {

constexpr int kPlanThreads = 1024;
constexpr int kPlanWaves = kPlanThreads / 64;
constexpr int kPlanCellsPerThread = kPlanMaxCells / kPlanThreads;   // 16
constexpr int kPlanMaxBlocks = 1024;                                // x 32 KB of cell list at the limit
constexpr int kPlanGridThreads = 256;
constexpr int kPlanChunkPolys = 32;                                 // polygons in LDS at a time
constexpr size_t kPlanStaticLds = 512;                              // bound on k_plan_seeds' static LDS
constexpr double kPlanSqrt2 = 1.4142135623730951;

// The parts of scene_block's packed scene (fp64, vap_footprint.h's layouts, no footprint rows) that k_plan_clearance reads:
//   poly  [n_poly][4]   slot 3: first vertex * 32 + vertex count (as a double); the bounds in slots 0-2 are not read
//   pv    [nv][8]       vertex x, y (0, 1); the edge to the next vertex ex, ey (4, 5); 1 / |e|^2 (6); |e| = sqrt(ex ex + ey ey) (7)
//   circ  [n_circle][4] cx, cy, r, 0
struct PlanScene {
    const double *poly, *pv, *circ;
    int n_poly, n_circle;
};

// the cell of a finite coordinate, clamped to the grid
__device__ __forceinline__ int plan_cell_of(double x, double lo, double cell, int n)
{
    double f = floor((x - lo) / cell);
    f = f < 0.0 ? 0.0 : (f > (double)(n - 1) ? (double)(n - 1) : f);
    return (int)f;
}

__global__ __launch_bounds__(kPlanGridThreads) void k_plan_clearance(PlanGrid g, PlanScene s, double radius, double margin,
                                                                     double *__restrict__ clearance, uint8_t *__restrict__ free_mask)
{
    __shared__ double s_pv[kPlanChunkPolys * kFootMaxVerts * 8];
    __shared__ double s_circ[kFootMaxCircles * 4];
    __shared__ int s_code[kPlanChunkPolys];
    const int tid = threadIdx.x;
    const int idx = blockIdx.x * kPlanGridThreads + tid;
    const bool live = idx < g.nx * g.ny;
    const int j = live ? idx / g.nx : 0, i = live ? idx - j * g.nx : 0;
    const double px = plan_centre(g.xmin, i, g.cell), py = plan_centre(g.ymin, j, g.cell);
    double best = fmin(fmin(px - g.xmin, g.xmax - px), fmin(py - g.ymin, g.ymax - py));
#pragma unroll 1
    for (int k0 = 0; k0 < s.n_poly; k0 += kPlanChunkPolys) {
        const int k1 = min(k0 + kPlanChunkPolys, s.n_poly);
        const int v0 = (int)s.poly[(size_t)k0 * 4 + 3] >> 5;
        const int last = (int)s.poly[(size_t)(k1 - 1) * 4 + 3];
        const int nrow = (last >> 5) + (last & 31) - v0;             // <= 32 x 16
        __syncthreads();
        for (int t = tid; t < nrow * 8; t += kPlanGridThreads) s_pv[t] = s.pv[(size_t)v0 * 8 + t];
        for (int t = tid; t < k1 - k0; t += kPlanGridThreads) s_code[t] = (int)s.poly[(size_t)(k0 + t) * 4 + 3];
        __syncthreads();
        if (!live) continue;
#pragma unroll 1
        for (int k = 0; k < k1 - k0; k++) {
            const int code = s_code[k], m = code & 31;
            const double *row = s_pv + (size_t)((code >> 5) - v0) * 8;
            double smax = -INFINITY, d2 = INFINITY;
#pragma unroll 1
            for (int e = 0; e < m; e++, row += 8) {
                const double wx = px - row[0], wy = py - row[1];
                smax = fmax(smax, (wx * row[5] - wy * row[4]) / row[7]);
                d2 = fmin(d2, seg_dist2(px, py, row[0], row[1], row[4], row[5], row[6]));
            }
            best = fmin(best, smax > 0.0 ? sqrt(d2) : smax);
        }
    }
    __syncthreads();
    for (int t = tid; t < s.n_circle * 4; t += kPlanGridThreads) s_circ[t] = s.circ[t];
    __syncthreads();
    if (!live) return;
#pragma unroll 1
    for (int k = 0; k < s.n_circle; k++) {
        const double dx = px - s_circ[k * 4 + 0], dy = py - s_circ[k * 4 + 1];
        best = fmin(best, sqrt(dx * dx + dy * dy) - s_circ[k * 4 + 2]);
    }
    const double c = best - radius;
    if (clearance) clearance[idx] = c;
    if (free_mask) free_mask[idx] = c >= margin ? 1 : 0;
}

struct SeedArgs {
    PlanGrid g;
    int R, W, max_vertices;
    const double *starts, *goals;
    const uint8_t *free_mask;
    uint16_t *path_ws;          // [gridDim.x][nx * ny]
    double *wp, *length;
    uint32_t *flags;
    int *n_vertices;
    double *vertices, *distance;
    const int *occ_first, *occ_last;   // [ny][nx], both or neither
    const int *windows;                // [R][2] (t0, t1), NULL: every instant
};

__device__ __forceinline__ bool plan_free(const uint32_t *fb, int idx) { return (fb[idx >> 5] >> (idx & 31)) & 1u; }

__device__ __forceinline__ int plan_floordiv(int a, int b)
{
    int q = a / b;
    if (a % b != 0 && ((a < 0) != (b < 0))) q--;
    return q;
}

// Every cell (i, j) of the bounding box of the two cells with 2 |(i - i0) dy - (j - j0) dx| <= |dx| + |dy| is free.  With
// |dy| <= |dx| the bound is at most |dx|, so j - j0 lies within 1 of (i - i0) dy / dx: the four cells floor(.) - 1 ..
// floor(.) + 2 of each column hold every cell the condition can pick (and likewise along y).
__device__ bool plan_visible(const uint32_t *fb, int nx, int c0, int c1)
{
    const int j0 = c0 / nx, i0 = c0 - j0 * nx, j1 = c1 / nx, i1 = c1 - j1 * nx;
    const int dx = i1 - i0, dy = j1 - j0, lim = abs(dx) + abs(dy);
    const int ilo = min(i0, i1), ihi = max(i0, i1), jlo = min(j0, j1), jhi = max(j0, j1);
    if (abs(dx) >= abs(dy)) {
        if (dx == 0) return true;                                    // the same cell
        for (int i = ilo; i <= ihi; i++) {
            const int q = plan_floordiv((i - i0) * dy, dx);
            for (int j = max(j0 + q - 1, jlo); j <= min(j0 + q + 2, jhi); j++)
                if (2 * abs((i - i0) * dy - (j - j0) * dx) <= lim && !plan_free(fb, j * nx + i)) return false;
        }
    } else {
        for (int j = jlo; j <= jhi; j++) {
            const int q = plan_floordiv((j - j0) * dx, dy);
            for (int i = max(i0 + q - 1, ilo); i <= min(i0 + q + 2, ihi); i++)
                if (2 * abs((i - i0) * dy - (j - j0) * dx) <= lim && !plan_free(fb, j * nx + i)) return false;
        }
    }
    return true;
}

// The free cell nearest to (px, py) by dx dx + dy dy to its centre, the lowest index on a tie; the whole workgroup calls it.
__device__ int plan_nearest_free(const PlanGrid &g, const uint32_t *fb, double px, double py, double *s_key, int *s_idx)
{
    const int tid = threadIdx.x, ncell = g.nx * g.ny;
    double best = INFINITY;
    int bi = INT_MAX;
    for (int idx = tid; idx < ncell; idx += kPlanThreads) {          // ascending per thread: the first minimum stays
        if (!plan_free(fb, idx)) continue;
        const int j = idx / g.nx, i = idx - j * g.nx;
        const double dx = plan_centre(g.xmin, i, g.cell) - px, dy = plan_centre(g.ymin, j, g.cell) - py;
        const double d2 = dx * dx + dy * dy;
        if (d2 < best) { best = d2; bi = idx; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if ((tid & 63) == 0) {
        s_key[tid >> 6] = best;
        s_idx[tid >> 6] = bi;
    }
    __syncthreads();
    best = s_key[0];
    bi = s_idx[0];
    for (int w = 1; w < kPlanWaves; w++)
        if (s_key[w] < best || (s_key[w] == best && s_idx[w] < bi)) { best = s_key[w]; bi = s_idx[w]; }
    __syncthreads();                                                 // the partials may be rewritten
    return bi;
}

// Each cell's byte of allowed moves from the free bits; the whole workgroup calls it, and a barrier follows.
__device__ __forceinline__ void plan_moves(const uint32_t *fb, uint8_t *mv, int nx, int ny)
{
    for (int idx = threadIdx.x; idx < nx * ny; idx += kPlanThreads) {
        unsigned m = 0;
        if (plan_free(fb, idx)) {
            const int j = idx / nx, i = idx - j * nx;
            const bool e = i + 1 < nx && plan_free(fb, idx + 1), n = j + 1 < ny && plan_free(fb, idx + nx);
            const bool w = i > 0 && plan_free(fb, idx - 1), s = j > 0 && plan_free(fb, idx - nx);
            m = (e ? 1u : 0u) | (n ? 2u : 0u) | (w ? 4u : 0u) | (s ? 8u : 0u);
            if (e && n && plan_free(fb, idx + nx + 1)) m |= 16u;     // a diagonal needs both axis cells beside it
            if (w && n && plan_free(fb, idx + nx - 1)) m |= 32u;
            if (w && s && plan_free(fb, idx - nx - 1)) m |= 64u;
            if (e && s && plan_free(fb, idx - nx + 1)) m |= 128u;
        }
        mv[idx] = (uint8_t)m;
    }
}

// The stages of one problem, shared by k_plan_seeds and k_plan_travel.  `off` holds the eight moves in the header's order as
// offsets in the grid; an axis move costs wa, a diagonal one wd.

// The problem's own mask: the static bits minus the cells occupied in [t0, t1).  The whole workgroup calls it; returns
// whether a cell is free at all (a barrier).
__device__ __forceinline__ bool plan_window_mask(const uint32_t *fbs, uint32_t *fb, int nwords, const int *occ_first,
                                                 const int *occ_last, int t0, int t1)
{
    int some = 0;
    for (int w = threadIdx.x; w < nwords; w += kPlanThreads) {
        uint32_t bits = fbs[w];
        if (t0 < t1) {
            for (uint32_t left = bits; left; left &= left - 1) {
                const int b = __ffs(left) - 1, idx = w * 32 + b;
                if (occ_first[idx] < t1 && occ_last[idx] >= t0) bits &= ~(1u << b);
            }
        }
        fb[w] = bits;
        some |= bits != 0;
    }
    return __syncthreads_or(some);
}

// relax: d[gc] = 0, d[v] = min over allowed moves v -> u of fl(d[u] + w), by Jacobi sweeps.  The whole workgroup calls it;
// returns whether a sweep changed nothing within ncell sweeps.
__device__ __forceinline__ bool plan_relax(double *d, const uint8_t *mv, const int (&off)[8], double wa, double wd, int ncell, int gc)
{
    const int tid = threadIdx.x;
    for (int idx = tid; idx < ncell; idx += kPlanThreads) d[idx] = idx == gc ? 0.0 : INFINITY;
    __syncthreads();
    bool converged = false;
#pragma unroll 1
    for (int sweep = 0; sweep < ncell && !converged; sweep++) {
        double nv[kPlanCellsPerThread];
#pragma unroll
        for (int c = 0; c < kPlanCellsPerThread; c++) {
            const int idx = tid + c * kPlanThreads;
            nv[c] = INFINITY;
            if (idx < ncell) {
                const unsigned m = mv[idx];
                const double *p = d + idx;                           // the cell's address once, the neighbours off it
                double best = INFINITY;
                if (m) {
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        if (m & (1u << k)) best = fmin(best, p[off[k]] + (k < 4 ? wa : wd));
                }
                nv[c] = best;
            }
        }
        __syncthreads();                                             // every read of this sweep is done
        int changed = 0;
#pragma unroll
        for (int c = 0; c < kPlanCellsPerThread; c++) {
            const int idx = tid + c * kPlanThreads;
            if (idx < ncell && nv[c] < d[idx]) {
                d[idx] = nv[c];
                changed = 1;
            }
        }
        converged = !__syncthreads_or(changed);
    }
    return converged;
}

// trace: from cell sc to the allowed neighbour with the smallest fl(d[u] + w), the first on a tie, until d = 0.  One lane
// calls it; returns the number of cells written to path, `fail` when the walk ended above d = 0.
__device__ __forceinline__ int plan_trace(const double *d, const uint8_t *mv, const int (&off)[8], double wa, double wd, int ncell,
                                          int sc, uint16_t *path, int &fail)
{
    int cur = sc, n = 0;
    path[n++] = (uint16_t)cur;
    while (d[cur] > 0.0 && n < ncell) {
        const unsigned m = mv[cur];
        double best = INFINITY;
        int bu = -1;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (!(m & (1u << k))) continue;
            const double c = d[cur + off[k]] + (k < 4 ? wa : wd);
            if (c < best) { best = c; bu = cur + off[k]; }
        }
        if (bu < 0) break;
        cur = bu;
        path[n++] = (uint16_t)cur;
    }
    fail = d[cur] > 0.0;
    return n;
}

// pull: from anchor a the largest b whose cell is visible from a's, else a + 1.  The whole workgroup calls it; the pulled
// list overwrites the front of the traced one.  Returns the number of pulled cells.
__device__ __forceinline__ int plan_pull(const uint32_t *fb, int nx, uint16_t *path, int n, int *s_best)
{
    const int tid = threadIdx.x;
    int nv = 1, anchor = 0;
    while (anchor < n - 1) {
        if (tid == 0) *s_best = anchor + 1;
        __syncthreads();
        const int ca = path[anchor];
        int bb = anchor + 1;
        for (int base = n - 1; base > anchor + 1; base -= kPlanThreads) {
            const int b = base - tid;
            if (b > anchor + 1 && plan_visible(fb, nx, ca, path[b])) atomicMax(s_best, b);
            __syncthreads();
            bb = *s_best;
            __syncthreads();
            if (bb > anchor + 1) break;
        }
        if (tid == 0) path[nv] = path[bb];                           // nv <= bb: the front of the list is done with
        nv++;
        anchor = bb;
    }
    __syncthreads();
    return nv;
}

// A route's ends and its pulled cells.  Vertex m: the start, the centres of the pulled cells, the goal.
struct PlanRoute {
    double sx, sy, gx, gy;
    const uint16_t *path;
    int nvtx;
};

__device__ __forceinline__ void plan_vertex(const PlanGrid &g, const PlanRoute &rt, int m, double &x, double &y)
{
    if (m == 0) { x = rt.sx; y = rt.sy; return; }
    if (m == rt.nvtx - 1) { x = rt.gx; y = rt.gy; return; }
    const int c = rt.path[m], j = c / g.nx;
    x = plan_centre(g.xmin, c - j * g.nx, g.cell);
    y = plan_centre(g.ymin, j, g.cell);
}

// lengths: the segment lengths a thread each, their running sum c_0 .. c_(nvtx-1) on one lane (a fixed order).  The whole
// workgroup calls it.
__device__ __forceinline__ void plan_lengths(const PlanGrid &g, const PlanRoute &rt, double *cum)
{
    const int tid = threadIdx.x;
    for (int m = tid; m < rt.nvtx - 1; m += kPlanThreads) {
        double x0, y0, x1, y1;
        plan_vertex(g, rt, m, x0, y0);
        plan_vertex(g, rt, m + 1, x1, y1);
        const double dx = x1 - x0, dy = y1 - y0;
        cum[m + 1] = sqrt(dx * dx + dy * dy);
    }
    __syncthreads();
    if (tid == 0) {
        cum[0] = 0.0;
        for (int m = 1; m < rt.nvtx; m++) cum[m] = cum[m - 1] + cum[m];
    }
    __syncthreads();
}

// resample: waypoint k of W at arc (k L) / (W - 1); 0 and W - 1 are the ends' own bits.  A thread per waypoint.
__device__ __forceinline__ void plan_waypoint(const PlanGrid &g, const PlanRoute &rt, const double *cum, double L, int k, int W,
                                              double &x, double &y)
{
    x = rt.gx;
    y = rt.gy;
    if (k == 0) {
        x = rt.sx;
        y = rt.sy;
    } else if (k < W - 1) {
        const double s = ((double)k * L) / (double)(W - 1);
        for (int m = 0; m < rt.nvtx - 1; m++) {
            if (!(cum[m + 1] >= s)) continue;
            double x0, y0, x1, y1;
            plan_vertex(g, rt, m, x0, y0);
            plan_vertex(g, rt, m + 1, x1, y1);
            const double dx = x1 - x0, dy = y1 - y0, l = sqrt(dx * dx + dy * dy);
            if (!(l > 0.0)) continue;
            const double t = (s - cum[m]) / l;
            x = x0 + t * dx;
            y = y0 + t * dy;
            break;
        }
    }
}

// The static free bits from the byte mask; the whole workgroup calls it; returns whether a cell is free at all (a barrier).
__device__ __forceinline__ bool plan_static_bits(const uint8_t *free_mask, uint32_t *fbs, int ncell, int nwords)
{
    int any = 0;
    for (int w = threadIdx.x; w < nwords; w += kPlanThreads) {
        uint32_t bits = 0;
        for (int b = 0; b < 32; b++) {
            const int idx = w * 32 + b;
            if (idx < ncell && free_mask[idx]) bits |= 1u << b;
        }
        fbs[w] = bits;
        any |= bits != 0;
    }
    return __syncthreads_or(any);
}

// ---- one problem, as both kernels run it: the stages above strung together once ------------------------------------------

// The dynamic LDS of a planning workgroup, stated once for the kernels and for the host that sizes their launch:
//   d [nd] the distance field (nd = ncell; at least 2 where the running sums c_0, c_1 of a one-cell grid go where the field was)
//   | fbs [nwords] the static free bits | fb [nwords] the problem's own mask (with an occupancy; without one fb is fbs)
//   | mv [ncell up to a multiple of 16] each cell's byte of allowed moves
struct PlanLds {
    int ncell, nd, nwords;
    bool occupied;
    PlanLds() = default;
    __host__ __device__ PlanLds(int ncell_, bool occupied_, bool sums_in_lds)
        : ncell(ncell_), nd(sums_in_lds && ncell_ < 2 ? 2 : ncell_), nwords((ncell_ + 31) / 32), occupied(occupied_) {}
    __host__ __device__ size_t bytes() const
    {
        return (size_t)nd * sizeof(double) + (size_t)(occupied ? 2 : 1) * nwords * sizeof(uint32_t) + (size_t)((ncell + 15) & ~15);
    }
    __device__ double *d(unsigned char *lds) const { return reinterpret_cast<double *>(lds); }
    __device__ uint32_t *fbs(unsigned char *lds) const { return reinterpret_cast<uint32_t *>(d(lds) + nd); }
    __device__ uint32_t *fb(unsigned char *lds) const { return occupied ? fbs(lds) + nwords : fbs(lds); }
    __device__ uint8_t *mv(unsigned char *lds) const { return reinterpret_cast<uint8_t *>(fb(lds) + nwords); }
};

// The static LDS of both kernels: the argmin's partials, and what the tracing lane and the pull hand the workgroup.
struct PlanShared {
    double key[kPlanWaves];
    int idx[kPlanWaves];
    int n, best, fail;
};

// What a workgroup's problems share.  `Args` below is SeedArgs or TravelArgs: g, free_mask, path_ws, occ_first, occ_last, windows.
struct PlanCore {
    PlanGrid g;
    PlanLds l;                  // ncell, nwords, occupied, and where the four pieces below begin
    double *d;
    uint32_t *fbs, *fb;
    uint8_t *mv;
    uint16_t *path;             // the workgroup's cell list
    PlanShared *sh;
    int off[8];                 // the eight moves in the header's order, as offsets in the grid
    double wa, wd;              // the cost of an axis move and of a diagonal one
    bool any_free;
};

// Once per workgroup: the carve, the static free bits and, without an occupancy, each free cell's allowed moves.
template <class Args>
__device__ __forceinline__ void plan_begin(PlanCore &c, const Args &a, unsigned char *lds, bool sums_in_lds, PlanShared *sh)
{
    c.g = a.g;
    const int nx = c.g.nx, ny = c.g.ny;
    c.l = PlanLds(nx * ny, a.occ_first != nullptr, sums_in_lds);
    c.d = c.l.d(lds);
    c.fbs = c.l.fbs(lds);
    c.fb = c.l.fb(lds);
    c.mv = c.l.mv(lds);
    c.path = a.path_ws + (size_t)blockIdx.x * (size_t)c.l.ncell;
    c.sh = sh;
    const int off[8] = {1, nx, -1, -nx, nx + 1, nx - 1, -nx - 1, -nx + 1};
#pragma unroll
    for (int k = 0; k < 8; k++) c.off[k] = off[k];
    c.wa = c.g.cell;
    c.wd = c.g.cell * kPlanSqrt2;
    c.any_free = plan_static_bits(a.free_mask, c.fbs, c.l.ncell, c.l.nwords);
    if (!c.l.occupied) {
        plan_moves(c.fb, c.mv, nx, ny);
        __syncthreads();
    }
}

// Problem r's own mask and moves under its window: the static bits minus the cells occupied in [t0, t1).  Nothing without an
// occupancy.  The whole workgroup calls it.
template <class Args>
__device__ __forceinline__ void plan_problem_mask(PlanCore &c, const Args &a, int r)
{
    if (!c.l.occupied) return;
    const int t0 = a.windows ? a.windows[(size_t)r * 2] : INT_MIN, t1 = a.windows ? a.windows[(size_t)r * 2 + 1] : INT_MAX;
    c.any_free = plan_window_mask(c.fbs, c.fb, c.l.nwords, a.occ_first, a.occ_last, t0, t1);
    plan_moves(c.fb, c.mv, c.g.nx, c.g.ny);
    __syncthreads();
}

// Is there anything to plan: four finite coordinates, then a free cell.  The flag of the first that fails.
__device__ __forceinline__ bool plan_admit(const PlanCore &c, const PlanRoute &rt, uint32_t &flags)
{
    if (!(isfinite(rt.sx) && isfinite(rt.sy) && isfinite(rt.gx) && isfinite(rt.gy))) {
        flags |= VAP_FLAG_DEGENERATE;
        return false;
    }
    if (!c.any_free) {
        flags |= VAP_PLAN_NO_FREE;
        return false;
    }
    return true;
}

// the cell of a point, or the free cell nearest to it (`snapped` is raised); every condition is the same in all threads
__device__ __forceinline__ int plan_snap(const PlanCore &c, double x, double y, uint32_t snapped, uint32_t &flags)
{
    const PlanGrid &g = c.g;
    int cell = plan_cell_of(y, g.ymin, g.cell, g.ny) * g.nx + plan_cell_of(x, g.xmin, g.cell, g.nx);
    if (!plan_free(c.fb, cell)) {
        cell = plan_nearest_free(g, c.fb, x, y, c.sh->key, c.sh->idx);
        flags |= snapped;
    }
    return cell;
}

// The goal's share: its cell, snapped if need be, and the field relaxed from it into c.d.  The whole workgroup calls it, with
// finite coordinates and a free cell somewhere.
__device__ __forceinline__ void plan_goal(const PlanCore &c, double gx, double gy, uint32_t &flags)
{
    const int gc = plan_snap(c, gx, gy, VAP_PLAN_SNAPPED_GOAL, flags);
    if (!plan_relax(c.d, c.mv, c.off, c.wa, c.wd, c.l.ncell, gc)) flags |= VAP_FLAG_NOCONVERGE;
}

// The start's share on a relaxed field: its cell, snapped if need be, the reach test, the trace on one lane, the pull; fills
// rt.nvtx and leaves the pulled cells in c.path.  The whole workgroup calls it, after plan_admit; false: no route.
__device__ __forceinline__ bool plan_start(const PlanCore &c, PlanRoute &rt, uint32_t &flags)
{
    const int sc = plan_snap(c, rt.sx, rt.sy, VAP_PLAN_SNAPPED_START, flags);
    if (c.d[sc] == INFINITY) {
        flags |= VAP_PLAN_UNREACHABLE;
        return false;
    }
    if (threadIdx.x == 0) {
        int fail;
        c.sh->n = plan_trace(c.d, c.mv, c.off, c.wa, c.wd, c.l.ncell, sc, c.path, fail);
        c.sh->fail = fail;
    }
    __syncthreads();
    const int n = c.sh->n;
    const bool fail = c.sh->fail;
    __syncthreads();
    if (fail) {
        flags |= VAP_FLAG_NOCONVERGE;
        return false;
    }
    const int nv = plan_pull(c.fb, c.g.nx, c.path, n, &c.sh->best);
    rt.nvtx = n == 1 ? 2 : nv;
    return true;
}

// wp [W][2]: the route resampled at equal arcs, NaN without one.  A thread per waypoint.
__device__ __forceinline__ void plan_store_waypoints(const PlanGrid &g, const PlanRoute &rt, const double *cum, double L, bool ok,
                                                     int W, double *wp)
{
    for (int k = threadIdx.x; k < W; k += kPlanThreads) {
        double x = NAN, y = NAN;
        if (ok) plan_waypoint(g, rt, cum, L, k, W, x, y);
        wp[2 * k] = x;
        wp[2 * k + 1] = y;
    }
}

__global__ __launch_bounds__(kPlanThreads) void k_plan_seeds(SeedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char plan_lds[];
    __shared__ PlanShared sh;
    PlanCore c;
    plan_begin(c, a, plan_lds, true, &sh);
    const PlanGrid &g = c.g;
    const int tid = threadIdx.x, ncell = c.l.ncell;
#pragma unroll 1
    for (int r = blockIdx.x; r < a.R; r += gridDim.x) {
        PlanRoute rt{a.starts[(size_t)r * 2], a.starts[(size_t)r * 2 + 1], a.goals[(size_t)r * 2], a.goals[(size_t)r * 2 + 1], c.path, 0};
        uint32_t flags = 0;
        plan_problem_mask(c, a, r);
        bool ok = plan_admit(c, rt, flags);
        if (!ok && a.distance)                                       // no field: +inf everywhere
            for (int idx = tid; idx < ncell; idx += kPlanThreads) a.distance[(size_t)r * ncell + idx] = INFINITY;
        if (ok) {
            plan_goal(c, rt.gx, rt.gy, flags);
            if (a.distance)
                for (int idx = tid; idx < ncell; idx += kPlanThreads) a.distance[(size_t)r * ncell + idx] = c.d[idx];
            ok = plan_start(c, rt, flags);
        }
        double *cum = c.d;                                           // the field is done with: c_0 .. c_(nvtx-1)
        if (ok) plan_lengths(g, rt, cum);
        const double L = ok ? cum[rt.nvtx - 1] : INFINITY;
        plan_store_waypoints(g, rt, cum, L, ok, a.W, a.wp + (size_t)r * a.W * 2);
        if (a.vertices) {
            double *vo = a.vertices + (size_t)r * a.max_vertices * 2;
            for (int m = tid; m < a.max_vertices; m += kPlanThreads) {
                double x = NAN, y = NAN;
                if (ok && m < rt.nvtx) plan_vertex(g, rt, m, x, y);
                vo[2 * m] = x;
                vo[2 * m + 1] = y;
            }
            if (ok && rt.nvtx > a.max_vertices) flags |= VAP_PLAN_VERTICES_TRUNCATED;
        }
        if (tid == 0) {
            if (a.length) a.length[r] = L;
            if (a.flags) a.flags[r] = flags;
            if (a.n_vertices) a.n_vertices[r] = ok ? rt.nvtx : 0;
        }
        __syncthreads();                                             // the next problem rewrites the field and the list
    }
}

struct TravelArgs {
    PlanGrid g;
    int R, P, W;
    const double *points;       // [R][P][2]
    const uint8_t *free_mask;
    uint16_t *path_ws;          // [gridDim.x][nx * ny]
    double *cum_ws;             // [gridDim.x][max(nx * ny, 2)]
    double *travel;             // [R][P][P]
    uint32_t *flags;
    int *n_vertices;
    double *wp;                 // [R][P][P][W][2]
    const int *occ_first, *occ_last;   // [ny][nx], both or neither
    const int *windows;                // [R][2] (t0, t1), NULL: every instant
};

// Entry (r, a, b) is k_plan_seeds' problem (start = point a, goal = point b), by the same functions: an item is one
// (problem, goal), whose field is relaxed once and stays in LDS while every start a != b is snapped, traced, pulled and
// resampled against it.  The running sums therefore live in the workgroup's global workspace, not where the field is.
__global__ __launch_bounds__(kPlanThreads) void k_plan_travel(TravelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char plan_lds[];
    __shared__ PlanShared sh;
    PlanCore c;
    plan_begin(c, a, plan_lds, false, &sh);
    const PlanGrid &g = c.g;
    const int tid = threadIdx.x, ncell = c.l.ncell, P = a.P;
    double *cum = a.cum_ws + (size_t)blockIdx.x * (size_t)(ncell < 2 ? 2 : ncell);
    const int items = a.R * P;
    int built = -1;                                                  // the problem whose mask and moves are in LDS
#pragma unroll 1
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int r = it / P, b = it - r * P;
        const double *pts = a.points + (size_t)r * P * 2;
        const double gx = pts[2 * b], gy = pts[2 * b + 1];
        if (r != built) {
            plan_problem_mask(c, a, r);
            built = r;
        }
        // the goal's share of every pair: its cell and its field
        uint32_t gflags = 0;
        if (isfinite(gx) && isfinite(gy) && c.any_free) plan_goal(c, gx, gy, gflags);
#pragma unroll 1
        for (int s = 0; s < P; s++) {
            const size_t e = ((size_t)r * P + s) * P + b;
            double *wp = a.wp ? a.wp + e * a.W * 2 : nullptr;
            if (s == b) {                                            // the diagonal: nowhere to go
                for (int k = tid; wp && k < a.W; k += kPlanThreads) {
                    wp[2 * k] = gx;
                    wp[2 * k + 1] = gy;
                }
                if (tid == 0) {
                    a.travel[e] = 0.0;
                    if (a.flags) a.flags[e] = 0;
                    if (a.n_vertices) a.n_vertices[e] = 0;
                }
                continue;
            }
            PlanRoute rt{pts[2 * s], pts[2 * s + 1], gx, gy, c.path, 0};
            uint32_t flags = 0;
            bool ok = plan_admit(c, rt, flags);
            if (ok) {
                flags = gflags;
                ok = plan_start(c, rt, flags);
            }
            if (ok) plan_lengths(g, rt, cum);
            const double L = ok ? cum[rt.nvtx - 1] : INFINITY;
            if (wp) plan_store_waypoints(g, rt, cum, L, ok, a.W, wp);
            if (tid == 0) {
                a.travel[e] = L;
                if (a.flags) a.flags[e] = flags;
                if (a.n_vertices) a.n_vertices[e] = ok ? rt.nvtx : 0;
            }
            __syncthreads();                                         // the next start rewrites the list and the sums
        }
    }
}

int plan_grid_of(const double *h_field, double cell, PlanGrid &g)
{
    const double fx = std::ceil((h_field[2] - h_field[0]) / cell), fy = std::ceil((h_field[3] - h_field[1]) / cell);
    if (!(fx >= 1.0) || !(fy >= 1.0) || !std::isfinite(fx) || !std::isfinite(fy))
        return vap_fail(VAP_ERR_INVALID, "the field box over cell %g gives no grid", cell);
    if (fx * fy > (double)kPlanMaxCells)
        return vap_fail(VAP_ERR_UNSUPPORTED, "a grid of %.0f x %.0f cells (at most %d cells)", fx, fy, kPlanMaxCells);
    g.xmin = h_field[0];
    g.ymin = h_field[1];
    g.xmax = h_field[2];
    g.ymax = h_field[3];
    g.cell = cell;
    g.nx = (int)fx;
    g.ny = (int)fy;
    return VAP_OK;
}

// The arguments both calls share, checked on the host before anything touches the device; fills the grid.
static int plan_check(const double *h_field, int n_poly, const int *h_poly_start, const double *h_poly_xy, int n_circle,
                      const double *h_circles, double cell, double radius, double margin, PlanGrid &g, int &nv)
{
    if (!(cell > 0.0) || !std::isfinite(cell)) return vap_fail(VAP_ERR_INVALID, "cell must be positive and finite (got %g)", cell);
    if (!(radius >= 0.0) || !std::isfinite(radius)) return vap_fail(VAP_ERR_INVALID, "radius must be >= 0 and finite (got %g)", radius);
    if (!std::isfinite(margin)) return vap_fail(VAP_ERR_INVALID, "margin must be finite");
    if (!h_field) return vap_fail(VAP_ERR_INVALID, "the planner needs a scene with a field box");
    double scale = 0.0;
    VAP_TRY(check_scene(h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, scale, nv));
    return plan_grid_of(h_field, cell, g);
}

// Upload the scene's block (scene_block: no footprint rows), then the clearance kernel over the grid.
static int plan_launch_grid(vap_ctx *ctx, const PlanGrid &g, int nv, int n_poly, const int *h_poly_start, const double *h_poly_xy,
                            int n_circle, const double *h_circles, double radius, double margin, double *d_clearance,
                            uint8_t *d_free)
{
    SceneLayout b;
    VAP_TRY(scene_block(ctx, 0, nullptr, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, nv, b));
    const double *d = (const double *)ctx->scene.ptr;
    PlanScene s{d + b.o_poly, d + b.o_pv, d + b.o_circ, n_poly, n_circle};
    const int ncell = g.nx * g.ny;
    hipLaunchKernelGGL(k_plan_clearance, dim3((ncell + kPlanGridThreads - 1) / kPlanGridThreads), dim3(kPlanGridThreads), 0,
                       ctx->stream, g, s, radius, margin, d_clearance, d_free);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

// Dynamic LDS above the default limit has to be granted by the runtime; a device attribute that reports more than the default
// is the opt-in limit and is checked too.
static int plan_grant_lds(vap_ctx *ctx, const void *kernel, size_t lds, const PlanGrid &g)
{
    if (lds <= 64 * 1024) return VAP_OK;
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) lds_max = 0;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess || (lds_max > 64 * 1024 && lds + kPlanStaticLds > (size_t)lds_max))
        return vap_fail(VAP_ERR_UNSUPPORTED, "a grid of %d x %d cells needs %zu bytes of LDS; the device gives a workgroup %d (%s)",
                        g.nx, g.ny, lds + kPlanStaticLds, lds_max, hipGetErrorString(e));
    return VAP_OK;
}

// What vap_plan_seeds_occupied and vap_plan_travel do between their own shape checks and their launch.
struct PlanLaunch {
    PlanGrid g;
    size_t lds, cum_bytes;          // cum_bytes: every workgroup's running sums in front of the cell lists (0: they are in LDS)
    int blocks;                     // 0: nothing to launch
};

static int plan_check_occupancy(const int *d_occ_first, const int *d_occ_last)
{
    if ((d_occ_first == nullptr) != (d_occ_last == nullptr))
        return vap_fail(VAP_ERR_INVALID, "the occupancy needs both its first and its last instants (or neither)");
    return VAP_OK;
}

// The shared checks and the grid, the device, the kernel's LDS (PlanLds) and its grant, one workgroup per item up to
// kPlanMaxBlocks, the free mask and the workspace ([sums, if not in LDS][cell lists]) and the clearance kernel into the mask.
static int plan_prepare(vap_ctx *ctx, const double *h_field, int n_poly, const int *h_poly_start, const double *h_poly_xy, int n_circle,
                        const double *h_circles, double cell, double radius, double margin, bool occupied, const void *kernel,
                        long long items, bool sums_in_lds, PlanLaunch &pl)
{
    int nv = 0;
    pl.blocks = 0;
    VAP_TRY(plan_check(h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, cell, radius, margin, pl.g, nv));
    VAP_TRY(vap_set_device(ctx));
    if (items == 0) return VAP_OK;
    const size_t ncell = (size_t)pl.g.nx * pl.g.ny;
    pl.lds = PlanLds((int)ncell, occupied, sums_in_lds).bytes();
    VAP_TRY(plan_grant_lds(ctx, kernel, pl.lds, pl.g));
    const int blocks = items < kPlanMaxBlocks ? (int)items : kPlanMaxBlocks;
    pl.cum_bytes = sums_in_lds ? 0 : (size_t)blocks * (ncell < 2 ? 2 : ncell) * sizeof(double);
    VAP_TRY(ctx->ensure(ctx->plan_free, ncell));
    VAP_TRY(ctx->ensure(ctx->plan_path, pl.cum_bytes + (size_t)blocks * ncell * sizeof(uint16_t)));
    VAP_TRY(plan_launch_grid(ctx, pl.g, nv, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, radius, margin, nullptr,
                             (uint8_t *)ctx->plan_free.ptr));
    pl.blocks = blocks;
    return VAP_OK;
}

}  // namespace vap

extern "C" {

int vap_plan_grid(vap_ctx *ctx, const double *h_field, int n_poly, const int *h_poly_start, const double *h_poly_xy, int n_circle,
                  const double *h_circles, double cell, double radius, double margin, double *d_clearance, uint8_t *d_free,
                  int *nx_out, int *ny_out)
{
    using namespace vap;
    PlanGrid g{};
    int nv = 0;
    VAP_TRY(plan_check(h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, cell, radius, margin, g, nv));
    if (nx_out) *nx_out = g.nx;
    if (ny_out) *ny_out = g.ny;
    if (!d_clearance && !d_free) return VAP_OK;                      // the shape only
    VAP_TRY(vap_set_device(ctx));
    return plan_launch_grid(ctx, g, nv, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, radius, margin, d_clearance, d_free);
}

int vap_plan_seeds(vap_ctx *ctx, int R, int W, const double *d_starts, const double *d_goals, const double *h_field, int n_poly,
                   const int *h_poly_start, const double *h_poly_xy, int n_circle, const double *h_circles, double cell,
                   double radius, double margin, int max_vertices, double *d_waypoints, double *d_length, uint32_t *d_flags,
                   int *d_n_vertices, double *d_vertices, double *d_distance)
{
    return vap_plan_seeds_occupied(ctx, R, W, d_starts, d_goals, h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, cell,
                                   radius, margin, max_vertices, nullptr, nullptr, nullptr, d_waypoints, d_length, d_flags,
                                   d_n_vertices, d_vertices, d_distance);
}

int vap_plan_seeds_occupied(vap_ctx *ctx, int R, int W, const double *d_starts, const double *d_goals, const double *h_field,
                            int n_poly, const int *h_poly_start, const double *h_poly_xy, int n_circle, const double *h_circles,
                            double cell, double radius, double margin, int max_vertices, const int *d_occ_first,
                            const int *d_occ_last, const int *d_windows, double *d_waypoints, double *d_length, uint32_t *d_flags,
                            int *d_n_vertices, double *d_vertices, double *d_distance)
{
    using namespace vap;
    VAP_TRY(plan_check_occupancy(d_occ_first, d_occ_last));
    if (R < 0) return vap_fail(VAP_ERR_INVALID, "bad shape R=%d", R);
    if (W < 2) return vap_fail(VAP_ERR_INVALID, "W=%d: a route needs at least 2 waypoints", W);
    if (W > kMaxWaypoints) return vap_fail(VAP_ERR_UNSUPPORTED, "W=%d exceeds %d", W, kMaxWaypoints);
    if (d_vertices && max_vertices < 2) return vap_fail(VAP_ERR_INVALID, "max_vertices = %d: the vertex output needs at least 2", max_vertices);
    if (R > 0 && (!d_starts || !d_goals || !d_waypoints)) return vap_fail(VAP_ERR_INVALID, "null starts / goals / waypoints");
    PlanLaunch pl{};
    VAP_TRY(plan_prepare(ctx, h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, cell, radius, margin, d_occ_first != nullptr,
                         reinterpret_cast<const void *>(k_plan_seeds), R, true, pl));
    if (!pl.blocks) return VAP_OK;
    SeedArgs a{};
    a.g = pl.g;
    a.R = R;
    a.W = W;
    a.max_vertices = max_vertices;
    a.starts = d_starts;
    a.goals = d_goals;
    a.free_mask = (const uint8_t *)ctx->plan_free.ptr;
    a.path_ws = (uint16_t *)ctx->plan_path.ptr;
    a.wp = d_waypoints;
    a.length = d_length;
    a.flags = d_flags;
    a.n_vertices = d_n_vertices;
    a.vertices = d_vertices;
    a.distance = d_distance;
    a.occ_first = d_occ_first;
    a.occ_last = d_occ_last;
    a.windows = d_occ_first ? d_windows : nullptr;
    hipLaunchKernelGGL(k_plan_seeds, dim3((unsigned)pl.blocks), dim3(kPlanThreads), pl.lds, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

int vap_plan_travel(vap_ctx *ctx, int R, int P, int W, const double *d_points, const double *h_field, int n_poly,
                    const int *h_poly_start, const double *h_poly_xy, int n_circle, const double *h_circles, double cell,
                    double radius, double margin, int max_vertices, const int *d_occ_first, const int *d_occ_last,
                    const int *d_windows, double *d_travel, uint32_t *d_flags, int *d_n_vertices, double *d_waypoints)
{
    using namespace vap;
    (void)max_vertices;                                              // no output of this call is cut to it
    VAP_TRY(plan_check_occupancy(d_occ_first, d_occ_last));
    if (R < 0 || P < 2) return vap_fail(VAP_ERR_INVALID, "bad shape R=%d P=%d", R, P);
    if (P > VAP_PLAN_TRAVEL_MAX_POINTS) return vap_fail(VAP_ERR_UNSUPPORTED, "P=%d exceeds %d", P, VAP_PLAN_TRAVEL_MAX_POINTS);
    if (d_waypoints && W < 2) return vap_fail(VAP_ERR_INVALID, "W=%d: a route needs at least 2 waypoints", W);
    if (d_waypoints && W > kMaxWaypoints) return vap_fail(VAP_ERR_UNSUPPORTED, "W=%d exceeds %d", W, kMaxWaypoints);
    if (R > 0 && (!d_points || !d_travel)) return vap_fail(VAP_ERR_INVALID, "null points / travel");
    if ((long long)R * P > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "R=%d problems of P=%d points exceed %d goals", R, P, INT_MAX);
    PlanLaunch pl{};
    VAP_TRY(plan_prepare(ctx, h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, cell, radius, margin, d_occ_first != nullptr,
                         reinterpret_cast<const void *>(k_plan_travel), (long long)R * P, false, pl));
    if (!pl.blocks) return VAP_OK;
    TravelArgs a{};
    a.g = pl.g;
    a.R = R;
    a.P = P;
    a.W = W;
    a.points = d_points;
    a.free_mask = (const uint8_t *)ctx->plan_free.ptr;
    a.cum_ws = (double *)ctx->plan_path.ptr;
    a.path_ws = (uint16_t *)((char *)ctx->plan_path.ptr + pl.cum_bytes);
    a.travel = d_travel;
    a.flags = d_flags;
    a.n_vertices = d_n_vertices;
    a.wp = d_waypoints;
    a.occ_first = d_occ_first;
    a.occ_last = d_occ_last;
    a.windows = d_occ_first ? d_windows : nullptr;
    hipLaunchKernelGGL(k_plan_travel, dim3((unsigned)pl.blocks), dim3(kPlanThreads), pl.lds, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
