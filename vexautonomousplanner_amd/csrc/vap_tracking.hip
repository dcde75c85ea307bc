// vap_tracking.hip — closed-loop tracking rollouts of time-domain rows (vap_tracking_rollouts).
//
// The clearance calls judge the nominal rows vap_time_profile writes; the robot drives what a path follower makes of
// them.  This file rolls a differential-drive robot with a RAMSETE follower along every route of a batch, K times per
// route under K perturbation records, and reports how far it strays (and, on request, the executed rows in the
// time-profile layout).  Definitions: include/vap.h.
//
// One kernel, a lane per rollout.  This file holds RAMSETE's march, its statistics and the follower's own argument checks;
// the lane's place in the launch, the perturbation record, the staged rows, the summaries and the host's common half are
// vap_track_common.h and vap_rollout_host.h:
//   layout   RolloutLane: K <= 256 a workgroup takes 256 / K whole routes, K > 256 a route takes ceil(K / 256) workgroups.
//   staging  RowStage: every rollout of a route reads the same five columns of the same row at the same step, so the
//            workgroup marches its routes' rows out of double-buffered LDS tiles, one barrier per tile.
//   march    the header's steps 1-6 per row in fp64; the per-rollout constants (gains, T * track_scale,
//            a = 1 - exp(-h / tau)) are computed once before the loop (PlantRecord).  Executed rows go out as four 16-byte
//            stores per lane and step.
//   summary  K <= 256: the summary's columns alias the stage buffers, free behind the last tile's barrier (the
//            clearance summary's the second buffer), and the first lane of each route walks its K rollouts in ascending k
//            (route_summary: the worst keeps the smallest k on a tie, the mean is one running sum).  K > 256: the rollouts'
//            (max e_pos, row) go to context scratch and k_route_reduce walks them the same way, a lane per route.  No
//            float atomics anywhere, so two calls give the same bits.
//   modes    the march is one function template, tracking_rollouts<MODE>: plain, with the executed rows written
//            (k_tracking_rollouts<false / true>), or with the scene clearance of every executed row taken where it would
//            be written (k_tracking_clearance) or by further lanes of the workgroup a tile later
//            (k_tracking_clearance_split, SplitLds); the last two for vap_rollout_clearance.hip, through tracking_setup /
//            tracking_launch.  k_tracking_conflicts takes, at the same place, the row's clearance to the partner's routes
//            (ConflictLane) for vap_rollout_conflicts.hip.
#include "vap_rollout_host.h"

namespace vap {

// The rollouts of one workgroup.  MODE: what becomes of the executed row (kTrackPlain, kTrackExec, kTrackClear,
// kTrackSplit, kTrackConflict); `c` is read with kTrackClear and kTrackSplit only, `x` and the footprints with kTrackConflict.
template <int MODE>
__device__ __forceinline__ void tracking_rollouts(const TrackArgs &g, const TrackClear *c, const TrackConflict *x = nullptr,
                                                  const ConfFoot *fa = nullptr, const ConfFoot *fo = nullptr)
{
    constexpr bool EXEC = MODE == kTrackExec, SPLIT = MODE == kTrackSplit, CLEAR = MODE == kTrackClear || SPLIT;
    constexpr bool CONF = MODE == kTrackConflict;
    const int tid = threadIdx.x;
    const int R = g.R, tile = g.tile;
    const bool producer = !SPLIT || tid < kTrackThreads;     // SPLIT: the threads behind the rollout lanes take clearances
    SplitLds sl;
    if constexpr (SPLIT) sl.begin();
    const RolloutLane ln(g, producer);
    ConflictLane cf;
    if constexpr (CONF) cf.begin(*x, *fa, *fo, ln.inside, ln.b, ln.k);
    RowStage st;
    st.begin(g, ln.b0, producer);
    const int wg_total = st.total;
    const int n = ln.lr < R ? st.n[ln.lr] : 0;
    const int b = ln.b;
    const size_t gi = ln.gi;

    // the rollout's constants and start state
    TrackPlant pl;
    bool valid = false;
    if (ln.inside && n > 0) {
        const PlantRecord rec(g, ln);
        valid = rec.valid();
        if (valid) rec.start(g, g.rows + (size_t)b * (size_t)g.cap * 8, pl);
    }
    const int my_total = valid ? n + g.settle : 0;
    double maxe = -INFINITY, maxey = -INFINITY, maxeph = -INFINITY;
    int mrow = -1, nsat = 0;
    double *erow = EXEC && valid ? g.exec_rows + gi * (size_t)g.cap_exec * 8 : nullptr;
    ClearAcc acc;

    const int ntiles = st.tiles(g);
    const int nit = SPLIT ? ntiles + 2 : ntiles;
#pragma unroll 1
    for (int ti = 0; ti < nit; ti++) {
        if (!SPLIT || sl.step(*c, acc, producer, ti, ntiles, tile, wg_total, my_total)) {
            const bool more = ti + 1 < ntiles;
            if (more) st.load(g, ti + 1);                  // in flight while this tile is marched
            const int r0 = ti * tile;
            const int rend = min(tile, wg_total - r0);
#pragma unroll 1
            for (int t = 0; t < rend; t++) {
                const int r = r0 + t;
                if (r >= my_total) {
                    if (SPLIT) sl.put(ti, t, tid, NAN, 0.0, 0.0);
                    continue;
                }
                const double *q = st.row(g, ti, t, ln.lr);
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
                if (SPLIT) sl.put(ti, t, tid, -track_wrap(pl.phi), pl.x, pl.y);
                if constexpr (CONF) cf.take(*x, pl, r);
                // 4. RAMSETE, 5. saturation, keeping c_L : c_R
                double cl, cr;
                ramsete_command(g, vr, wref, ex, ey, eph, cl, cr);
                if (track_saturate(cl, cr, g.wmax)) nsat++;
                // 6. substeps: first-order wheel lag, then the exact arc
                pl.advance(cl, cr, g.nsub, g.h);
            }
            if (more) st.store(g, (ti + 1) & 1);
        }
        __syncthreads();
    }

    // kTrackConflict: the instants after the last executed row, the rollout parked at its pose
    if constexpr (CONF) cf.tail(*x, my_total);

    // 7. final errors against row n - 1, and the rollout's outputs
    const bool have = mrow >= 0;
    double cmin = INFINITY;
    int crow = -1, cother = -1;
    if (ln.inside) {
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
        rollout_outputs(g, gi, my_total, maxe, mrow);
        if (CLEAR) acc.store(*c, gi);
        if constexpr (CONF) cf.finish(*x, gi, cmin, crow, cother);
    }
    if (g.wpr > 1) return;                              // the route's summary: k_route_reduce
    // the route's summary inside the workgroup: the stage buffers are free (the last barrier is behind every thread)
    double *s_e = st.buf;
    int *s_r = st.n;
    __syncthreads();                                    // st.n was read above
    if (producer) {
        s_e[tid] = maxe;
        s_r[tid] = ln.inside ? mrow : -1;
    }
    // the clearance summary's columns lie in the other stage buffer
    double *s_c = st.buf + kTrackRows * 5;
    int *s_cr = (int *)(s_c + kTrackThreads), *s_ce = s_cr + kTrackThreads;
    if (CLEAR && producer) {
        s_c[tid] = acc.best;
        s_cr[tid] = ln.inside ? acc.row : -1;
        s_ce[tid] = acc.el;
    }
    if (CONF && producer) {
        s_c[tid] = cmin;
        s_cr[tid] = crow;
        s_ce[tid] = cother;
    }
    __syncthreads();
    route_summary<TrackSummary>(g, ln, g.K, s_e, s_r, nullptr, g.tol);
    if constexpr (CONF)
        if (x->summary()) route_summary<ConflictSummary>(*x, ln, g.K, s_c, s_cr, s_ce, x->margin);
    if (CLEAR && c->summary()) route_summary<ClearSummary>(*c, ln, g.K, s_c, s_cr, s_ce, c->margin);
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

int tracking_setup(const RolloutCall &c, const vap_follower *f, TrackArgs &g)
{
    // host validation first: it needs no device
    if (!f) return vap_fail(VAP_ERR_INVALID, "null follower");
    if (!(f->track_width > 0.0) || !(f->b > 0.0) || !(f->zeta > 0.0) || !(f->wheel_speed_max > 0.0) ||
        !std::isfinite(f->track_width) || !std::isfinite(f->b) || !std::isfinite(f->zeta) || !std::isfinite(f->wheel_speed_max))
        return vap_fail(VAP_ERR_INVALID, "follower: track_width, b, zeta and wheel_speed_max must be positive and finite (got %g, %g, %g, %g)",
                        f->track_width, f->b, f->zeta, f->wheel_speed_max);
    VAP_TRY(rollout_check(c, "follower", *f, g));
    g.b = f->b;
    g.two_zeta = 2.0 * f->zeta;
    return VAP_OK;
}

// vap_rollout_conflicts: the same march, the clearance of every executed row to the partner's routes taken in the lane
// that made it, and the parked instants after the march
__global__ __launch_bounds__(kTrackThreads) void k_tracking_conflicts(TrackArgs g, TrackConflict x, ConfFoot fa, ConfFoot fo)
{
    tracking_rollouts<kTrackConflict>(g, nullptr, &x, &fa, &fo);
}

int tracking_launch(vap_ctx *ctx, TrackArgs &g, TrackClear *clear, ConflictCall *conf)
{
    long grid;
    VAP_TRY(rollout_place(ctx, g, g.summary(), 1, 0, clear, grid, conf ? &conf->x : nullptr));
    g.tile = stage_tile(g.R, rollout_split(ctx, clear, grid));
    return rollout_run<TrackSummary>(ctx, g, clear, grid,
                                     RolloutKernels<TrackArgs>{k_tracking_rollouts<false>, k_tracking_rollouts<true>, k_tracking_clearance,
                                                               k_tracking_clearance_split, k_tracking_conflicts},
                                     conf);
}

}  // namespace vap

extern "C" {

int vap_tracking_rollouts(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                          double time_step, const vap_follower *f, int K, int shared_perturb, const double *d_perturb,
                          double *d_stats, int *d_stat_rows, double *d_worst, double *d_mean, int *d_worst_rollout,
                          int *d_worst_row, int *d_n_exceeding, long cap_exec, double *d_exec_rows, int *d_exec_counts)
{
    using namespace vap;
    const RolloutCall call{B, capacity, d_rows, d_counts, counts_stride, time_step, K, shared_perturb, d_perturb, d_stats, d_stat_rows,
                           d_worst, d_mean, d_worst_rollout, d_worst_row, d_n_exceeding, nullptr, nullptr, cap_exec, d_exec_rows,
                           d_exec_counts};
    TrackArgs g{};
    VAP_TRY(tracking_setup(call, f, g));
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;
    return tracking_launch(ctx, g, nullptr);
}

}  // extern "C"
