// vap_tracking.hip — closed-loop tracking rollouts of time-domain rows (vap_tracking_rollouts).
//
// The clearance calls judge the nominal rows vap_time_profile writes; the robot drives what a path follower makes of
// them.  This file rolls a differential-drive robot with a RAMSETE follower along every route of a batch, K times per
// route under K perturbation records, and reports how far it strays (and, on request, the executed rows in the
// time-profile layout).  Definitions: include/vap.h.
//
// One kernel, a lane per rollout:
//   layout   K <= 256: a workgroup takes R = 256 / K whole routes (thread = route-in-group * K + k; the last
//            256 - R * K threads idle); K > 256: a route takes ceil(K / 256) workgroups.  A workgroup's lanes therefore
//            never straddle a route boundary other than at a multiple of K.
//   staging  every rollout of a route reads the same five columns {v, heading, angular_vel, x, y} of the same row at
//            the same step, so the workgroup stages its routes' rows in LDS, 40 B per row, in tiles of kTrackRows / R rows
//            (at most 64): the next tile's loads are issued before the current tile is marched and land in the other LDS
//            buffer after it, one barrier per tile.  The settle rows (r >= n) are made by the loader (the last pose,
//            v = omega = 0), so the march never looks at counts.  Staged as [row][column][route]: lanes of one route
//            read one address (a broadcast), lanes of different routes consecutive ones.
//   march    the header's steps 1-6 per row in fp64; the per-rollout constants (gains, T * track_scale,
//            a = 1 - exp(-h / tau)) are computed once before the loop.  Executed rows go out as four 16-byte stores per
//            lane and step.
//   summary  K <= 256: the first lane of each route walks its K rollouts in LDS in ascending k (a fixed order: the
//            worst keeps the smallest k on a tie, the mean is one running sum).  K > 256: the rollouts' (max e_pos,
//            row) go to context scratch and k_tracking_reduce walks them the same way, a lane per route.  No float
//            atomics anywhere, so two calls give the same bits.
//   modes    the march is one function template, tracking_rollouts<MODE>: plain, with the executed rows written
//            (k_tracking_rollouts<false / true>), or with the scene clearance of every executed row taken where it would
//            be written (k_tracking_clearance) or by further lanes of the workgroup a tile later
//            (k_tracking_clearance_split); the last two for vap_rollout_clearance.hip, through tracking_setup / tracking_launch.
#include <climits>
#include <cmath>
#include <cstdint>

#include "vap_internal.h"
#include "vap_track_common.h"

namespace vap {

constexpr int kTrackRows = 512;        // staged rows per LDS buffer, over all routes of the workgroup
constexpr int kTrackTileMax = 64;      // rows of one route per tile, at most

// The rollouts of one workgroup.  MODE: what becomes of the executed row (kTrackPlain, kTrackExec, kTrackClear,
// kTrackSplit); `c` is read with the last two only.
template <int MODE>
__device__ __forceinline__ void tracking_rollouts(const TrackArgs &g, const TrackClear *c)
{
    constexpr bool EXEC = MODE == kTrackExec, SPLIT = MODE == kTrackSplit;
    __shared__ __attribute__((aligned(16))) double stage[2][kTrackRows * 5];
    __shared__ int s_n[kTrackThreads];
    __shared__ int s_total;
    const int tid = threadIdx.x;
    const int R = g.R, tile = g.tile;
    const bool producer = !SPLIT || tid < kTrackThreads;     // SPLIT: the threads behind the rollout lanes take clearances
    double *s_pose = nullptr, *s_cap = nullptr;
    if constexpr (SPLIT) {
        s_pose = lds_doubles<2 * kSplitTile, 0>();
        s_cap = lds_doubles<2 * kTrackThreads, 1>();
    }
    // which rollout this lane walks
    const int b0 = g.wpr > 1 ? (int)(blockIdx.x / g.wpr) : (int)blockIdx.x * R;
    const int lr = g.wpr > 1 ? 0 : tid / g.K;                                  // route within the workgroup
    const int k = g.wpr > 1 ? (int)(blockIdx.x % g.wpr) * kTrackThreads + tid : tid % g.K;
    const int b = b0 + lr;
    const bool inside = producer && lr < R && b < g.B && k < g.K;
    if (tid == 0) s_total = 0;
    if (tid < R) {
        int n = 0;
        if (b0 + tid < g.B) {
            const long c = g.counts[(size_t)(b0 + tid) * g.stride];
            n = (int)(c < 0 ? 0 : (c > g.cap ? g.cap : c));
        }
        s_n[tid] = n;
    }
    __syncthreads();
    if (tid < R && s_n[tid] > 0) atomicMax(&s_total, s_n[tid] + g.settle);
    __syncthreads();
    const int wg_total = s_total;                     // steps of the longest route of the workgroup
    const int n = lr < R ? s_n[lr] : 0;
    const size_t gi = (size_t)b * g.K + k;            // flattened (b, k)

    // the rollout's constants and start state
    TrackPlant pl;
    bool valid = false;
    if (inside && n > 0) {
        const double *p = g.perturb + (g.shared ? (size_t)k : gi) * 8;
        const double2 p01 = *(const double2 *)p, p23 = *(const double2 *)(p + 2), p45 = *(const double2 *)(p + 4),
                      p67 = *(const double2 *)(p + 6);
        const double tau = p67.x;
        valid = isfinite(p01.x) && isfinite(p01.y) && isfinite(p23.x) && isfinite(p23.y) && isfinite(p45.x) &&
                isfinite(p45.y) && isfinite(p67.x) && isfinite(p67.y) && p23.y > 0.0 && p45.x > 0.0 && p45.y > 0.0 && tau >= 0.0;
        if (valid) {
            const double *row0 = g.rows + (size_t)b * (size_t)g.cap * 8;
            const double v0 = row0[2], w0 = -row0[5];
            pl.x = row0[6] + p01.x;
            pl.y = row0[7] + p01.y;
            pl.phi = -row0[4] + p23.x;
            pl.wl = v0 - w0 * g.T / 2.0;
            pl.wr = v0 + w0 * g.T / 2.0;
            pl.gl = p23.y;
            pl.gr = p45.x;
            pl.tts = g.T * p45.y;
            pl.a = tau == 0.0 ? 1.0 : 1.0 - exp(-g.h / tau);
        }
    }
    const int my_total = valid ? n + g.settle : 0;
    double maxe = -INFINITY, maxey = -INFINITY, maxeph = -INFINITY;
    int mrow = -1, nsat = 0;
    double *erow = EXEC && valid ? g.exec_rows + gi * (size_t)g.cap_exec * 8 : nullptr;
    ClearAcc acc;

    // the loader: item j < R * tile is row j % tile of route j / tile of the tile (consecutive threads on consecutive
    // rows of a route); at most two items per thread
    const int items = R * tile;
    double lv[2], lh[2], lw[2], lx[2], ly[2];
    auto load = [&](int ti) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int j = tid + i * kTrackThreads;
            lv[i] = lh[i] = lw[i] = lx[i] = ly[i] = 0.0;
            if (producer && j < items) {
                const int route = j / tile, r = ti * tile + j % tile, nr = s_n[route];
                if (nr > 0 && r < nr + g.settle) {
                    const int src = r < nr ? r : nr - 1;
                    const double *q = g.rows + ((size_t)(b0 + route) * (size_t)g.cap + (size_t)src) * 8;
                    const double2 hw = *(const double2 *)(q + 4), xy = *(const double2 *)(q + 6);
                    lv[i] = r < nr ? q[2] : 0.0;
                    lh[i] = hw.x;
                    lw[i] = r < nr ? hw.y : 0.0;
                    lx[i] = xy.x;
                    ly[i] = xy.y;
                }
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int j = tid + i * kTrackThreads;
            if (producer && j < items) {
                double *d = stage[buf] + (size_t)(j % tile) * 5 * R + j / tile;
                d[0] = lv[i];
                d[R] = lh[i];
                d[2 * R] = lw[i];
                d[3 * R] = lx[i];
                d[4 * R] = ly[i];
            }
        }
    };

    const int ntiles = (wg_total + tile - 1) / tile;
    if (ntiles > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    const int nit = SPLIT ? ntiles + 2 : ntiles;       // SPLIT: tile ti is marched, tile ti - 1 cleared, tile ti - 2 folded
#pragma unroll 1
    for (int ti = 0; ti < nit; ti++) {
        if (SPLIT && !producer) {
            if (ti >= 1 && ti <= ntiles)
                split_clear(*c, s_pose, s_cap, ti - 1, min(tile, wg_total - (ti - 1) * tile), tid - kTrackThreads,
                            (int)blockDim.x - kTrackThreads);
        } else {
            if (SPLIT && ti >= 2)
                split_fold(acc, s_pose, ti - 2, (ti - 2) * tile, min(tile, wg_total - (ti - 2) * tile), my_total, tid, c->margin);
            if (SPLIT) s_cap[(size_t)(ti & 1) * kTrackThreads + tid] = acc.best;
            if (!SPLIT || ti < ntiles) {
        const bool more = ti + 1 < ntiles;
        if (more) load(ti + 1);                        // in flight while this tile is marched
        const double *cur = stage[ti & 1] + (lr < R ? lr : 0);
        const int r0 = ti * tile;
        const int rend = min(tile, wg_total - r0);
#pragma unroll 1
        for (int t = 0; t < rend; t++) {
            const int r = r0 + t;
            if (r >= my_total) {
                if (SPLIT) split_put(s_pose, ti & 1, t, tid, NAN, 0.0, 0.0);
                continue;
            }
            const double *q = cur + (size_t)t * 5 * R;
            const double vr = q[0], phr = -q[R], wref = -q[2 * R], xr = q[3 * R], yr = q[4 * R];
            // 1. errors in the body frame
            double sp, cp;
            sincos(pl.phi, &sp, &cp);
            const double dx = xr - pl.x, dy = yr - pl.y;
            const double ex = cp * dx + sp * dy, ey = cp * dy - sp * dx;
            const double eph = track_wrap(phr - pl.phi);
            const double epos = hypot(ex, ey);
            // 2. statistics
            if (epos > maxe) { maxe = epos; mrow = r; }
            if (fabs(ey) > maxey) maxey = fabs(ey);
            if (fabs(eph) > maxeph) maxeph = fabs(eph);
            // 3. the executed row
            if (EXEC) pl.write_row(erow, r, g.dt);
            if (MODE == kTrackClear) acc.take(c->s, c->margin, pl, r);
            if (SPLIT) split_put(s_pose, ti & 1, t, tid, -track_wrap(pl.phi), pl.x, pl.y);
            // 4. RAMSETE
            double se, ce;
            sincos(eph, &se, &ce);
            const double kk = g.two_zeta * sqrt(wref * wref + g.b * vr * vr);
            const double vc = vr * ce + kk * ex;
            const double wc = wref + kk * eph + g.b * vr * track_sinc(eph, se) * ey;
            double cl = vc - wc * g.T / 2.0, cr = vc + wc * g.T / 2.0;
            // 5. saturation, keeping c_L : c_R
            if (track_saturate(cl, cr, g.wmax)) nsat++;
            // 6. substeps: first-order wheel lag, then the exact arc
            pl.advance(cl, cr, g.nsub, g.h);
        }
        if (more) store((ti + 1) & 1);
            }
        }
        __syncthreads();
    }

    // 7. final errors against row n - 1, and the rollout's outputs
    const bool have = mrow >= 0;
    if (inside) {
        double fpos = NAN, fphi = NAN;
        if (have) {
            const double *ql = g.rows + ((size_t)b * (size_t)g.cap + (size_t)(n - 1)) * 8;
            fpos = hypot(ql[6] - pl.x, ql[7] - pl.y);
            fphi = fabs(track_wrap(-ql[4] - pl.phi));
        }
        if (g.stats) {
            double2 *o = (double2 *)(g.stats + gi * 6);
            o[0] = make_double2(have ? maxe : NAN, have ? maxey : NAN);
            o[1] = make_double2(have ? maxeph : NAN, fpos);
            o[2] = make_double2(fphi, have ? 0.0 : NAN);
        }
        if (g.stat_rows) {
            g.stat_rows[gi * 2] = mrow;
            g.stat_rows[gi * 2 + 1] = have ? nsat : -1;
        }
        if (g.exec_counts) {
            g.exec_counts[gi * 2] = my_total;
            g.exec_counts[gi * 2 + 1] = 0;
        }
        if (g.part_e) {
            g.part_e[gi] = maxe;
            g.part_row[gi] = mrow;
        }
        if (MODE == kTrackClear || SPLIT) acc.store(*c, gi);
    }
    if (g.wpr > 1) return;                              // the route's summary: k_tracking_reduce
    // the route's summary inside the workgroup: the stage buffers are free (the last barrier is behind every thread)
    double *s_e = stage[0];
    int *s_r = s_n;
    __syncthreads();                                    // s_n was read above
    if (producer) {
        s_e[tid] = maxe;
        s_r[tid] = inside ? mrow : -1;
    }
    // the clearance summary's columns lie in the other stage buffer
    double *s_c = stage[1];
    int *s_cr = (int *)(stage[1] + kTrackThreads), *s_ce = s_cr + kTrackThreads;
    if ((MODE == kTrackClear || SPLIT) && producer) {
        s_c[tid] = acc.best;
        s_cr[tid] = inside ? acc.row : -1;
        s_ce[tid] = acc.el;
    }
    __syncthreads();
    if (inside && k == 0) {
        TrackSummary sum;
#pragma unroll 1
        for (int kk = 0; kk < g.K; kk++) sum.take(s_e[tid + kk], s_r[tid + kk], kk, g.tol);
        sum.store(g, b);
        if ((MODE == kTrackClear || SPLIT) && c->summary()) {
            ClearSummary cs;
#pragma unroll 1
            for (int kk = 0; kk < g.K; kk++) cs.take(s_c[tid + kk], s_cr[tid + kk], s_ce[tid + kk], kk, c->margin);
            cs.store(*c, b);
        }
    }
}

template <bool EXEC>
__global__ __launch_bounds__(kTrackThreads) void k_tracking_rollouts(TrackArgs g)
{
    tracking_rollouts<EXEC ? kTrackExec : kTrackPlain>(g, nullptr);
}

// vap_rollout_clearance: the same march, the clearance of every executed row taken in the lane that made it
__global__ __launch_bounds__(kTrackThreads) void k_tracking_clearance(TrackArgs g, TrackClear c)
{
    tracking_rollouts<kTrackClear>(g, &c);
}

// the same with the clearance split off: kTrackThreads rollout lanes and, behind them, lanes that take the clearance of the
// tile the rollout lanes marched before
__global__ __launch_bounds__(kSplitThreads) void k_tracking_clearance_split(TrackArgs g, TrackClear c)
{
    tracking_rollouts<kTrackSplit>(g, &c);
}

// K > 256: per route, its rollouts' partials in ascending k
__global__ __launch_bounds__(64) void k_tracking_reduce(TrackArgs g)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= g.B) return;
    TrackSummary sum;
#pragma unroll 1
    for (int kk = 0; kk < g.K; kk++) {
        const size_t p = (size_t)b * g.K + kk;
        sum.take(g.part_e[p], g.part_row[p], kk, g.tol);
    }
    sum.store(g, b);
}

int tracking_setup(int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride, double time_step,
                   const vap_follower *f, int K, int shared_perturb, const double *d_perturb, double *d_stats, int *d_stat_rows,
                   double *d_worst, double *d_mean, int *d_worst_rollout, int *d_worst_row, int *d_n_exceeding, long cap_exec,
                   double *d_exec_rows, int *d_exec_counts, TrackArgs &g)
{
    // host validation first: it needs no device
    if (!f) return vap_fail(VAP_ERR_INVALID, "null follower");
    if (!(f->track_width > 0.0) || !(f->b > 0.0) || !(f->zeta > 0.0) || !(f->wheel_speed_max > 0.0) ||
        !std::isfinite(f->track_width) || !std::isfinite(f->b) || !std::isfinite(f->zeta) || !std::isfinite(f->wheel_speed_max))
        return vap_fail(VAP_ERR_INVALID, "follower: track_width, b, zeta and wheel_speed_max must be positive and finite (got %g, %g, %g, %g)",
                        f->track_width, f->b, f->zeta, f->wheel_speed_max);
    if (std::isnan(f->tolerance)) return vap_fail(VAP_ERR_INVALID, "follower: tolerance is NaN");
    if (!(time_step > 0.0) || !std::isfinite(time_step)) return vap_fail(VAP_ERR_INVALID, "time_step must be positive and finite (got %g)", time_step);
    if (f->n_substeps < 1 || f->n_substeps > 16) return vap_fail(VAP_ERR_INVALID, "follower: n_substeps %d outside 1..16", f->n_substeps);
    if (f->settle_rows < 0 || f->settle_rows > 10000) return vap_fail(VAP_ERR_INVALID, "follower: settle_rows %d outside 0..10000", f->settle_rows);
    if (K < 1 || K > 4096) return vap_fail(VAP_ERR_INVALID, "K = %d rollouts per route outside 1..4096", K);
    if (B < 0 || capacity < 0) return vap_fail(VAP_ERR_INVALID, "bad shape B=%d capacity=%ld", B, capacity);
    if (counts_stride < 1) return vap_fail(VAP_ERR_INVALID, "counts_stride must be >= 1 (got %d)", counts_stride);
    if (B > 0 && (!d_counts || (capacity > 0 && !d_rows))) return vap_fail(VAP_ERR_INVALID, "null rows / counts");
    if (B > 0 && !d_perturb) return vap_fail(VAP_ERR_INVALID, "null perturbation records");
    if (capacity + f->settle_rows > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld + settle rows above %d", capacity, INT_MAX);
    if (d_exec_rows && cap_exec < capacity + f->settle_rows)
        return vap_fail(VAP_ERR_INVALID, "cap_exec %ld below capacity + settle_rows = %ld", cap_exec, capacity + f->settle_rows);
    if ((((uintptr_t)d_rows | (uintptr_t)d_perturb | (uintptr_t)d_stats | (uintptr_t)d_exec_rows) & 15) != 0)
        return vap_fail(VAP_ERR_INVALID, "rows, perturbation records, stats and executed rows must be 16-byte aligned");
    g.rows = d_rows;
    g.counts = d_counts;
    g.cap = capacity;
    g.stride = counts_stride;
    g.B = B;
    g.K = K;
    g.shared = shared_perturb != 0;
    g.perturb = d_perturb;
    g.T = f->track_width;
    g.b = f->b;
    g.two_zeta = 2.0 * f->zeta;
    g.wmax = f->wheel_speed_max;
    g.tol = f->tolerance;
    g.dt = time_step;
    g.h = time_step / (double)f->n_substeps;
    g.nsub = f->n_substeps;
    g.settle = f->settle_rows;
    g.stats = d_stats;
    g.stat_rows = d_stat_rows;
    g.worst = d_worst;
    g.mean = d_mean;
    g.worst_rollout = d_worst_rollout;
    g.worst_row = d_worst_row;
    g.n_exceeding = d_n_exceeding;
    g.cap_exec = cap_exec;
    g.exec_rows = d_exec_rows;
    g.exec_counts = d_exec_counts;
    return VAP_OK;
}

int tracking_launch(vap_ctx *ctx, TrackArgs &g, TrackClear *clear)
{
    const int B = g.B, K = g.K;
    const bool summary = g.worst || g.mean || g.worst_rollout || g.worst_row || g.n_exceeding;
    // context scratch, K > 256 only: the rollouts' partials of the summary, then those of the clearance summary
    size_t part_bytes = 0;
    const size_t clear_bytes = clear_part_bytes(clear, B, K);
    long grid;
    if (K <= kTrackThreads) {
        g.R = kTrackThreads / K;
        g.wpr = 1;
        grid = ((long)B + g.R - 1) / g.R;
    } else {
        g.R = 1;
        g.wpr = (K + kTrackThreads - 1) / kTrackThreads;
        grid = (long)B * g.wpr;
        if (summary) part_bytes = (size_t)B * (size_t)K * (sizeof(double) + sizeof(int));
        part_bytes = (part_bytes + 15) & ~(size_t)15;
    }
    if (grid > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "%d routes x %d rollouts: too many workgroups for one launch", B, K);
    if (part_bytes + clear_bytes) VAP_TRY(ctx->ensure(ctx->track_part, part_bytes + clear_bytes));
    if (g.wpr > 1 && summary) {
        g.part_e = (double *)ctx->track_part.ptr;
        g.part_row = (int *)(g.part_e + (size_t)B * (size_t)K);
    }
    if (clear_bytes) clear_part_place(clear, (char *)ctx->track_part.ptr + part_bytes, B, K);
    g.tile = kTrackRows / g.R < kTrackTileMax ? kTrackRows / g.R : kTrackTileMax;
    // the clearance split off the rollout lanes where every workgroup gets a CU of its own (K = 16 at config 3: one rollout
    // wave per SIMD, which cannot hide the clearance's loads); with more workgroups than CUs the lanes' own clearance,
    // several workgroups to a CU, measured faster
    const bool split = clear && grid <= track_cus(ctx->device);
    if (split) g.tile = g.tile < kSplitRows ? g.tile : kSplitRows;

    if (split)
        hipLaunchKernelGGL(k_tracking_clearance_split, dim3((unsigned)grid), dim3(kSplitThreads), 0, ctx->stream, g, *clear);
    else if (clear)
        hipLaunchKernelGGL(k_tracking_clearance, dim3((unsigned)grid), dim3(kTrackThreads), 0, ctx->stream, g, *clear);
    else if (g.exec_rows)
        hipLaunchKernelGGL(k_tracking_rollouts<true>, dim3((unsigned)grid), dim3(kTrackThreads), 0, ctx->stream, g);
    else
        hipLaunchKernelGGL(k_tracking_rollouts<false>, dim3((unsigned)grid), dim3(kTrackThreads), 0, ctx->stream, g);
    if (g.wpr > 1 && summary)
        hipLaunchKernelGGL(k_tracking_reduce, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // namespace vap

extern "C" {

int vap_tracking_rollouts(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                          double time_step, const vap_follower *f, int K, int shared_perturb, const double *d_perturb,
                          double *d_stats, int *d_stat_rows, double *d_worst, double *d_mean, int *d_worst_rollout,
                          int *d_worst_row, int *d_n_exceeding, long cap_exec, double *d_exec_rows, int *d_exec_counts)
{
    using namespace vap;
    TrackArgs g{};
    VAP_TRY(tracking_setup(B, capacity, d_rows, d_counts, counts_stride, time_step, f, K, shared_perturb, d_perturb, d_stats,
                           d_stat_rows, d_worst, d_mean, d_worst_rollout, d_worst_row, d_n_exceeding, cap_exec, d_exec_rows,
                           d_exec_counts, g));
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;
    return tracking_launch(ctx, g, nullptr);
}

}  // extern "C"
