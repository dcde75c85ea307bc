// vap_conflict.hip — robot-to-robot clearance between two batches of time-domain rows (vap_footprint_conflicts).
//
// vap_footprint_clearance treats the field as empty of other robots.  This file answers "which of my candidates get along
// with my partner's routine": side A's footprint at every row of every A route against side O's footprint at the same
// instant of every O route (or of the matching one).  Definitions: include/vap.h.
//
// Three steps on the context's stream:
//   pack    one thread per (route, horizon row): sincos(-heading) once, the posed centre of the footprint's bounding
//           circle, {cx, cy, cos, sin} (32 B) to scratch; rows outside the route's own repeat the parked pose, so row r of
//           both sides is the same instant and the pair kernel never looks at counts or the shift again.  Per 64 rows one
//           bounding circle of those centres.
//   pairs   a workgroup owns a tile of 16 A routes x 16 O routes, one pair per thread.  Per 64-row block: the block bound
//           from the two block circles; when at least one pair of the tile needs the block, the 32 routes' packed rows are
//           staged in LDS once (a packed row is read from memory once per tile, not once per pair), then a wave takes
//           its pairs that need the block one after another, a lane per row: the bounding-circle bound
//           |c_a - c_o| - R_a - R_o, then the exact polygon pair, then a wave (clearance, row) argmin.  A pair's state
//           lives in one lane and every reduction has a fixed order, so the outputs do not depend on scheduling.
//   reduce  per-tile partials (min, smallest other at the min, its row, conflicts, earliest first row) to the per-route
//           outputs, tiles in ascending order; no float atomics (they cannot keep the tie rules).
//
// Culling.  With thresh = the pair's running minimum (while no earlier row below the margin has been seen: the larger of
// it and the margin), a row is skipped when its bound exceeds thresh by more than a slack that covers rounding.  The bound
// never exceeds the exact clearance (both polygons lie inside their bounding circles), so a skipped row is neither below
// the margin (when that still matters) nor at or below the running minimum: it could not change any output.  thresh never
// rises.  The running minimum is seeded, before the walk, with four exactly tested rows of the block where the two block
// circles are nearest; the (clearance, row) minimum and the first row below the margin do not depend on the order rows
// are taken in, so the seeds change nothing but how soon the walk can skip.
// For a block: every centre of the block lies within rb of the block circle's centre cb, so for each of its rows
// |c_a - c_o| >= |cb_a - cb_o| - rb_a - rb_o, and the block bound |cb_a - cb_o| - rb_a - rb_o - R_a - R_o is at most every
// row bound of the block; no row of a skipped block could have lowered thresh, so each would have been skipped too.
// VAP_OPT_FOOTPRINT_CULL = 0 tests every row exactly; the outputs are the same bit for bit.
//
// The exact pair is vap_footprint.hip's polygon clearance (separating axes over the edge normals of both, else the
// vertex-to-edge distance), evaluated in one footprint's body frame: the other sits at t + R(rel) v, so the frame's own
// vertices, normals and projection extents are call constants (LDS) and only the other's vertices are transformed.
//
// This file defines the pack kernel all three robot-to-robot calls launch (conf_pack_sides, vap_conflict.h) and keeps its
// own tile walk; the exact pair on two packed rows, the row and block bounds and the argument checks are vap_conflict.h's.
#include "vap_conflict.h"

namespace vap {

// pack[b][Tp][4] = {cx, cy, cos, sin} of horizon row r (route row clamp(r - shift, 0, n - 1)); blk[b][nblk][4] = centre,
// radius of a circle around the 64 centres of a block, 0.  A wave per block.
__global__ __launch_bounds__(256) void k_conflict_pack(ConfSide s, double fcx, double fcy, long Tp, int nblk, int groups,
                                                       double *__restrict__ pack, double *__restrict__ blk)
{
    const int b = blockIdx.x / groups;
    const int block = (blockIdx.x % groups) * 4 + threadIdx.x / 64;
    if (block >= nblk) return;                          // whole waves leave; no barrier below
    const int lane = threadIdx.x & 63;
    const long r = (long)block * kConfBlock + lane;
    const long n = conf_count(s, b);
    double cx = 0.0, cy = 0.0, c = 1.0, sn = 0.0;
    if (n > 0) {
        long src = r - s.shift;
        src = src < 0 ? 0 : (src > n - 1 ? n - 1 : src);
        const double *row = s.rows + ((size_t)b * (size_t)s.cap + (size_t)src) * 8;
        conf_pose(row[4], row[6], row[7], fcx, fcy, cx, cy, c, sn);
    }
    double *o = pack + ((size_t)b * (size_t)Tp + (size_t)r) * 4;
    o[0] = cx;
    o[1] = cy;
    o[2] = c;
    o[3] = sn;
    double x0 = cx, x1 = cx, y0 = cy, y1 = cy;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        x0 = fmin(x0, __shfl_xor(x0, off));
        x1 = fmax(x1, __shfl_xor(x1, off));
        y0 = fmin(y0, __shfl_xor(y0, off));
        y1 = fmax(y1, __shfl_xor(y1, off));
    }
    const double mx = 0.5 * (x0 + x1), my = 0.5 * (y0 + y1);
    double d2 = (cx - mx) * (cx - mx) + (cy - my) * (cy - my);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d2 = fmax(d2, __shfl_xor(d2, off));
    if (lane == 0) {
        double *q = blk + ((size_t)b * (size_t)nblk + (size_t)block) * 4;
        q[0] = mx;
        q[1] = my;
        q[2] = sqrt(d2);
        q[3] = 0.0;
    }
}

struct ConfArgs : ConfPacked {    // both sides are packed to one horizon: Tpa == Tpo, nblk_a == nblk_o
    int nto;                  // O tiles per A route (1 when matched)
    double margin;
    double *pair_c;           // [Ba][P], optional
    int *pair_row, *pair_first;
    double *part_c;           // [Ba][nto] per-tile partials: min clearance (+inf: no valid pair) ...
    int *part_i;              // ... [Ba][nto][4] = other, row, conflicts, first row (INT_MAX: none)
};

template <bool MATCHED>
__global__ __launch_bounds__(kConfThreads) void k_conflict_pairs(ConfFoot fa, ConfFoot fo, ConfArgs g)
{
    __shared__ double sfa[kFootMaxVerts * 8], sfo[kFootMaxVerts * 8];
    __shared__ __attribute__((aligned(16))) double stage[MATCHED ? 2 : 2 * kConfTile * kConfRouteStride];
    __shared__ int s_T;
    const int tid = threadIdx.x;
    if (tid < kFootMaxVerts * 8) {
        sfa[tid] = fa.v[tid];
        sfo[tid] = fo.v[tid];
    }
    if (tid == 0) s_T = 0;
    const int ta = MATCHED ? 0 : blockIdx.x / g.nto, to = MATCHED ? 0 : blockIdx.x % g.nto;
    const int la = tid / kConfTile, lo = tid % kConfTile;
    const int ia = MATCHED ? blockIdx.x * kConfThreads + tid : ta * kConfTile + la;
    const int io = MATCHED ? ia : to * kConfTile + lo;
    const bool inside = ia < g.a.B && io < g.o.B;
    const long n_a = inside ? conf_count(g.a, ia) : 0, n_o = inside ? conf_count(g.o, io) : 0;
    const bool valid = n_a > 0 && n_o > 0;
    long Tl = 0;
    if (valid) {
        Tl = n_a > n_o + g.o.shift ? n_a : n_o + g.o.shift;
        Tl = Tl < 1 ? 1 : Tl;
    }
    const int T = (int)Tl;                                   // <= Tp <= INT_MAX
    __syncthreads();
    if (valid) atomicMax(&s_T, T);
    __syncthreads();
    const int nchunk = (s_T + kConfBlock - 1) / kConfBlock;  // the tile's horizon; rows past a pair's own T are not examined
    const int na = fa.n, no = fo.n;
    const double radii = fa.R + fo.R;
    const double *pa = g.pack_a + (size_t)ia * (size_t)g.Tpa * 4, *po = g.pack_o + (size_t)io * (size_t)g.Tpa * 4;

    double best = INFINITY;
    int brow = INT_MAX, first = INT_MAX;
    // a row's exact clearance into the pair's running (clearance, row) minimum and first row below the margin; the
    // rules do not depend on the order the rows come in
    auto take = [&](double v, int r) {
        if (v < g.margin && r < first) first = r;
        if (v < best || (v == best && r < brow)) { best = v; brow = r; }
    };
    if (valid && g.cull) {
        // Seed the running minimum where the pair is likely closest: four rows of the block whose circles are nearest,
        // tested exactly.  Two robots that approach each other lower the minimum at every row on the way, so a walk
        // from row 0 alone would cull nothing until they part.
        const int nb = (T + kConfBlock - 1) / kConfBlock;
        double near = INFINITY;
        int kn = 0;
#pragma unroll 1
        for (int k = 0; k < nb; k++) {
            const double *qa = g.blk_a + ((size_t)ia * g.nblk_a + k) * 4, *qo = g.blk_o + ((size_t)io * g.nblk_a + k) * 4;
            const double dx = qo[0] - qa[0], dy = qo[1] - qa[1];
            const double d = sqrt(dx * dx + dy * dy) - qa[2] - qo[2];
            if (d < near) { near = d; kn = k; }
        }
#pragma unroll 1
        for (int i = 0; i < 4; i++) {
            const int r = min(kn * kConfBlock + i * 21, T - 1);
            take(pair_at(sfa, na, sfo, no, pa + (size_t)r * 4, po + (size_t)r * 4), r);
        }
    }
#pragma unroll 1
    for (int k = 0; k < nchunk; k++) {
        const int r0 = k * kConfBlock;
        bool need = valid && r0 < T;
        if (need && g.cull) {
            const double *qa = g.blk_a + ((size_t)ia * g.nblk_a + k) * 4, *qo = g.blk_o + ((size_t)io * g.nblk_a + k) * 4;
            const double thresh = first < r0 ? best : fmax(best, g.margin);
            need = !block_culled(g, radii, thresh, qa[0], qa[1], qa[2], qo[0], qo[1], qo[2]);
        }
        if (!MATCHED) {
            if (!__syncthreads_or(need)) continue;           // also: every thread has left the previous chunk's rows
            // the tile's 32 routes x 64 rows x 32 B, 16 B per lane, consecutive lanes on consecutive addresses
            constexpr int kPer = kConfBlock * 2;             // 16-byte pieces per route
#pragma unroll 4
            for (int j = tid; j < 2 * kConfTile * kPer; j += kConfThreads) {
                const int route = j / kPer, piece = j % kPer;
                const bool side_o = route >= kConfTile;
                const int idx = side_o ? to * kConfTile + (route - kConfTile) : ta * kConfTile + route;
                if (idx < (side_o ? g.o.B : g.a.B)) {
                    const double *src = (side_o ? g.pack_o : g.pack_a) + ((size_t)idx * (size_t)g.Tpa + (size_t)r0) * 4;
                    *(double2 *)(stage + route * kConfRouteStride + piece * 2) = *(const double2 *)(src + piece * 2);
                }
            }
            __syncthreads();
        }
        // The wave's pairs that need the block, one after another, a lane per row: rows of one pair at neighbouring
        // instants agree on whether they need the exact test, which lanes holding different pairs would not.  Every row
        // is judged against thresh as it stood when the block began (at least what a row-by-row walk would use), and
        // the block's (clearance, row) minimum and first row below the margin go to the lane that owns the pair.
        const double thresh0 = first < r0 ? best : fmax(best, g.margin);
        const int lane = tid & 63;
        unsigned long long todo = __ballot(need);
        while (todo) {
            const int l = __ffsll(todo) - 1;
            todo &= todo - 1;
            const int T_l = __shfl(T, l);
            const double th = __shfl(thresh0, l);
            const double *rla, *rlo;
            if (MATCHED) {
                const size_t route = (size_t)blockIdx.x * kConfThreads + (tid - lane) + l;
                rla = g.pack_a + (route * (size_t)g.Tpa + (size_t)r0) * 4;
                rlo = g.pack_o + (route * (size_t)g.Tpa + (size_t)r0) * 4;
            } else {
                const int pair = (tid - lane) + l;
                rla = stage + (pair / kConfTile) * kConfRouteStride;
                rlo = stage + (kConfTile + pair % kConfTile) * kConfRouteStride;
            }
            double v = INFINITY;
            int vr = INT_MAX, vf = INT_MAX;
            if (r0 + lane < T_l) {
                const double2 a01 = *(const double2 *)(rla + lane * 4), o01 = *(const double2 *)(rlo + lane * 4);
                if (!g.cull || !row_culled(g, radii, th, a01.x, a01.y, o01.x, o01.y)) {
                    const double c = pair_at(sfa, na, sfo, no, rla + lane * 4, rlo + lane * 4);
                    if (c == c) {                            // a NaN clearance takes part in nothing
                        v = c;
                        vr = r0 + lane;
                        if (c < g.margin) vf = r0 + lane;
                    }
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(v, off);
                const int orow = __shfl_xor(vr, off);
                if (ov < v || (ov == v && orow < vr)) { v = ov; vr = orow; }
                vf = min(vf, __shfl_xor(vf, off));
            }
            if (lane == l) {
                if (vf < first) first = vf;
                if (v < best || (v == best && vr < brow)) { best = v; brow = vr; }
            }
        }
    }

    const bool have = brow != INT_MAX;                       // a valid pair with a finite clearance
    if (inside) {
        const size_t p = MATCHED ? (size_t)ia : (size_t)ia * (size_t)g.o.B + (size_t)io;
        if (g.pair_c) g.pair_c[p] = have ? best : NAN;
        if (g.pair_row) g.pair_row[p] = have ? brow : -1;
        if (g.pair_first) g.pair_first[p] = have && first != INT_MAX ? first : -1;
    }
    // the tile's partial per A route: (clearance, other) argmin with that pair's row, conflicts, earliest first row
    double pc = have ? best : INFINITY;
    int pother = have ? io : INT_MAX, prow = brow, ncon = have && best < g.margin ? 1 : 0, pfirst = have ? first : INT_MAX;
    if (!MATCHED) {
#pragma unroll
        for (int off = kConfTile / 2; off >= 1; off >>= 1) {
            const double oc = __shfl_xor(pc, off);
            const int oo = __shfl_xor(pother, off), orow = __shfl_xor(prow, off);
            if (oc < pc || (oc == pc && oo < pother)) { pc = oc; pother = oo; prow = orow; }
            ncon += __shfl_xor(ncon, off);
            pfirst = min(pfirst, __shfl_xor(pfirst, off));
        }
    }
    if ((MATCHED ? inside : lo == 0 && ia < g.a.B)) {
        const size_t p = (size_t)ia * g.nto + to;
        g.part_c[p] = pc;
        g.part_i[p * 4 + 0] = pother;
        g.part_i[p * 4 + 1] = prow;
        g.part_i[p * 4 + 2] = ncon;
        g.part_i[p * 4 + 3] = pfirst;
    }
}

// per A route: its tiles' partials in ascending order (a strictly smaller clearance replaces: the smallest other stays)
__global__ __launch_bounds__(64) void k_conflict_reduce(int Ba, int nto, const double *__restrict__ part_c,
                                                        const int *__restrict__ part_i, double *__restrict__ min_c,
                                                        int *__restrict__ min_other, int *__restrict__ min_row,
                                                        int *__restrict__ n_conf, int *__restrict__ first_row)
{
    const int ia = blockIdx.x * 64 + threadIdx.x;
    if (ia >= Ba) return;
    double best = INFINITY;
    int other = INT_MAX, row = -1, ncon = 0, first = INT_MAX;
#pragma unroll 1
    for (int t = 0; t < nto; t++) {
        const size_t p = (size_t)ia * nto + t;
        const int *pi = part_i + p * 4;
        if (part_c[p] < best) { best = part_c[p]; other = pi[0]; row = pi[1]; }
        ncon += pi[2];
        first = min(first, pi[3]);
    }
    const bool none = other == INT_MAX;
    if (min_c) min_c[ia] = none ? NAN : best;
    if (min_other) min_other[ia] = none ? -1 : other;
    if (min_row) min_row[ia] = none ? -1 : row;
    if (n_conf) n_conf[ia] = ncon;
    if (first_row) first_row[ia] = first == INT_MAX ? -1 : first;
}

}  // namespace vap

extern "C" {

int vap_footprint_conflicts(vap_ctx *ctx, int pairing, int shift_rows, double margin,
                            int Ba, long cap_a, const double *d_rows_a, const int *d_counts_a, int stride_a, int n_foot_a,
                            const double *h_foot_a,
                            int Bo, long cap_o, const double *d_rows_o, const int *d_counts_o, int stride_o, int n_foot_o,
                            const double *h_foot_o,
                            double *d_pair_clearance, int *d_pair_row, int *d_pair_first_row,
                            double *d_min_clearance, int *d_min_other, int *d_min_row, int *d_n_conflicts, int *d_first_row)
{
    using namespace vap;
    const ConfInput a{Ba, cap_a, d_rows_a, d_counts_a, stride_a, n_foot_a, h_foot_a}, o{Bo, cap_o, d_rows_o, d_counts_o, stride_o, n_foot_o, h_foot_o};
    const bool matched = pairing == VAP_CONFLICT_MATCHED;
    VAP_TRY(vap_set_device(ctx));
    if (pairing != VAP_CONFLICT_ALL_PAIRS && !matched) return vap_fail(VAP_ERR_INVALID, "unknown pairing %d", pairing);
    VAP_TRY(conf_check_shape("Ba", a, o));
    if (cap_a > INT_MAX || cap_o > INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld above %d rows", cap_a > cap_o ? cap_a : cap_o, INT_MAX);
    VAP_TRY(conf_check_sides(a, o, Bo, matched, margin, false, "null rows / counts"));
    if (Ba == 0 || Bo == 0) return VAP_OK;

    // the horizon every pair fits in: T = max(n_a, n_o + shift, 1) <= max(cap_a, cap_o + shift, 1)
    long Tcap = cap_a > cap_o + (long)shift_rows ? cap_a : cap_o + (long)shift_rows;
    Tcap = Tcap < 1 ? 1 : Tcap;
    const ConfHorizon h = conf_horizon(Tcap);
    if (h.Tp > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "horizon of %ld rows above %d", Tcap, INT_MAX);
    const long nta = (Ba + kConfTile - 1) / kConfTile, nto = matched ? 1 : (Bo + kConfTile - 1) / kConfTile;
    const long grid_pairs = matched ? (Ba + kConfThreads - 1) / kConfThreads : nta * nto;
    const long grid_pack = (long)(Ba > Bo ? Ba : Bo) * h.groups;
    if (grid_pairs > INT_MAX || grid_pack > INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "%d x %d routes over %ld rows: too many workgroups for one launch", Ba, Bo, Tcap);

    ConfFoot fa, fo;
    ConfArgs g;
    VAP_TRY(conf_pack_sides(ctx, a, o, shift_rows, h, h, fa, fo, g));
    const size_t n_part = (size_t)Ba * (size_t)nto;
    VAP_TRY(ctx->ensure(ctx->conf_part, n_part * (sizeof(double) + 4 * sizeof(int))));
    g.nto = (int)nto;
    g.margin = margin;
    g.pair_c = d_pair_clearance;
    g.pair_row = d_pair_row;
    g.pair_first = d_pair_first_row;
    g.part_c = (double *)ctx->conf_part.ptr;
    g.part_i = (int *)(g.part_c + n_part);

    if (matched)
        hipLaunchKernelGGL(k_conflict_pairs<true>, dim3((unsigned)grid_pairs), dim3(kConfThreads), 0, ctx->stream, fa, fo, g);
    else
        hipLaunchKernelGGL(k_conflict_pairs<false>, dim3((unsigned)grid_pairs), dim3(kConfThreads), 0, ctx->stream, fa, fo, g);
    if (d_min_clearance || d_min_other || d_min_row || d_n_conflicts || d_first_row)
        hipLaunchKernelGGL(k_conflict_reduce, dim3((unsigned)((Ba + 63) / 64)), dim3(64), 0, ctx->stream, Ba, (int)nto, g.part_c,
                           g.part_i, d_min_clearance, d_min_other, d_min_row, d_n_conflicts, d_first_row);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
