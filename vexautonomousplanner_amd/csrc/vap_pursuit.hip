// vap_pursuit.hip — closed-loop rollouts of time-domain rows under a pure-pursuit follower (vap_pursuit_rollouts).
//
// vap_tracking.hip rolls the robot with RAMSETE, which is fed (x, y, heading, v, omega) row by row on the clock.  Pure
// pursuit is indexed by where the robot is on the path: it reads the polyline P_i = columns 6, 7 and the speeds v_i =
// column 2 and nothing else, steers for a goal one lookahead further along the chord length, and so never sees the
// heading column's steps.  Same perturbation records, same plant (vap_track_common.h), same outputs' layout; slot 7 of a
// record is the rollout's lookahead, so K spans perturbations x lookaheads.  Definitions: include/vap.h.
//
// Two kernels (three with K > 256):
//   check    a workgroup per route: rows 0 .. n - 1 for a negative speed (bit 0) and a non-finite x, y or v (bit 1), ORed
//            with integer atomics in LDS; the mask goes to context scratch for the rollouts and to d_route_status.
//   rollouts a lane per rollout in the followers' common layout (K <= 256: 256 / K whole routes per workgroup; K > 256:
//            ceil(K / 256) workgroups per route), written out here (below).  Unlike RAMSETE's, the lanes of a route are not at
//            the same row: each carries its own closest segment ic and lookahead segment il, which only advance.  A lane
//            keeps the three points P_ic, P_ic+1, P_ic+2 and the two points P_il, P_il+1 in registers with the chord
//            length c and the segment length of each pointer; an advance loads one point (the K lanes of a route hit the
//            same few lines, L1 / L2 serve them) and costs one sqrt.  Both pointers form the same sum c_(i+1) = c_i +
//            len_i in index order, so c is the same number whichever pointer computed it.  The total chord length and
//            the last tangent are needed only once il has reached the last segment; they are formed there.  Nothing
//            waits across lanes: every loop is bounded by n.
//   summary  as vap_tracking.hip, with PursuitSummary (the rollouts that never arrived): K <= 256 the first lane of each
//            route walks its K rollouts in LDS in ascending k; K > 256 the partials, the row of arrival
//            among them, go to context scratch and k_route_reduce walks them, a lane per route.  No float atomics, so two
//            calls give the same bits.
//   modes    as vap_tracking.hip: pursuit_rollouts<MODE> is the march; k_pursuit_rollouts<false / true>,
//            k_pursuit_clearance and k_pursuit_clearance_split (vap_rollout_clearance.hip, through pursuit_setup /
//            pursuit_launch) instantiate it.  Only the split cuts the row loop into tiles of kSplitRows rows with a barrier
//            each, on SplitLds' buffers.
// The plant, the count clamp, the outputs every follower writes, the reduce kernel, the split's buffers and the host's common
// checks, grid and launches are vap_track_common.h and vap_rollout_host.h.  This file holds the pure-pursuit march,
// k_pursuit_check, PursuitSummary and the checks of vap_pursuit's own fields, and, unlike the other two followers, its own
// lane mapping, record parsing, plant start, split schedule and summary walk in LDS: these kernels sit where any change
// around the march moves their scalar spills and scratch (see PursuitArgs in vap_track_common.h).
#include "vap_rollout_host.h"

namespace vap {

constexpr int kCheckThreads = 256;

__global__ __launch_bounds__(kCheckThreads) void k_pursuit_check(PursuitArgs g)
{
    __shared__ int s_mask;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_mask = 0;
    __syncthreads();
    const int n = route_rows(g, b);
    int m = 0;
    for (int r = tid; r < n; r += kCheckThreads) {
        const double *q = g.rows + ((size_t)b * (size_t)g.cap + (size_t)r) * 8;
        const double v = q[2];
        const double2 xy = *(const double2 *)(q + 6);
        if (v < 0.0) m |= 1;
        if (!(isfinite(v) && isfinite(xy.x) && isfinite(xy.y))) m |= 2;
    }
    if (m) atomicOr(&s_mask, m);
    __syncthreads();
    if (tid == 0) {
        g.status[b] = s_mask;
        if (g.route_status) g.route_status[b] = s_mask;
    }
}

struct PursuitPoint {
    double x, y, v;
};

__device__ __forceinline__ PursuitPoint pursuit_point(const double *route, int i)
{
    const double *q = route + (size_t)i * 8;
    const double2 xy = *(const double2 *)(q + 6);
    return {xy.x, xy.y, q[2]};
}

__device__ __forceinline__ double pursuit_len(double ax, double ay, double bx, double by)
{
    const double sx = bx - ax, sy = by - ay;
    return sqrt(sx * sx + sy * sy);
}

// the point (x, y) on the segment a -> b: t = clamp(((p - a) . s) / (s . s), 0, 1) (0 on a segment without length) and the
// squared distance to a + t s
__device__ __forceinline__ void pursuit_project(double ax, double ay, double bx, double by, double x, double y, double &t, double &D)
{
    const double sx = bx - ax, sy = by - ay;
    const double ss = sx * sx + sy * sy;
    t = 0.0;
    if (ss != 0.0) t = fmin(fmax(((x - ax) * sx + (y - ay) * sy) / ss, 0.0), 1.0);
    const double ex = x - (ax + t * sx), ey = y - (ay + t * sy);
    D = ex * ex + ey * ey;
}

// the route's summary adds the valid rollouts that never arrived
struct PursuitSummary : TrackSummary {
    int nun = 0;
    __device__ void take(double e, int r, int arrived, int kk, double tol)
    {
        TrackSummary::take(e, r, 0, kk, tol);
        nun += r >= 0 && arrived < 0 ? 1 : 0;
    }
    __device__ void store(const PursuitArgs &g, int b) const
    {
        TrackSummary::store(g, b);
        if (g.n_unfinished) g.n_unfinished[b] = nun;
    }
};

// The rollouts of one workgroup.  MODE: what becomes of the executed row (kTrackPlain, kTrackExec, kTrackClear,
// kTrackSplit, kTrackConflict); `c` is read with kTrackClear and kTrackSplit only, `x` and the footprints with kTrackConflict.
template <int MODE>
__device__ __forceinline__ void pursuit_rollouts(const PursuitArgs &g, const TrackClear *c, const TrackConflict *x = nullptr,
                                                 const ConfFoot *fa = nullptr, const ConfFoot *fo = nullptr)
{
    constexpr bool EXEC = MODE == kTrackExec, SPLIT = MODE == kTrackSplit, CONF = MODE == kTrackConflict;
    __shared__ double s_e[kTrackThreads];
    __shared__ int s_r[kTrackThreads], s_a[kTrackThreads];
    const int tid = threadIdx.x;
    const int R = g.R;
    const bool producer = !SPLIT || tid < kTrackThreads;     // SPLIT: the threads behind the rollout lanes take clearances
    SplitLds sl;
    if constexpr (SPLIT) sl.begin();
    // which rollout this lane walks
    const int b0 = g.wpr > 1 ? (int)(blockIdx.x / g.wpr) : (int)blockIdx.x * R;
    const int lr = g.wpr > 1 ? 0 : tid / g.K;                                  // route within the workgroup
    const int k = g.wpr > 1 ? (int)(blockIdx.x % g.wpr) * kTrackThreads + tid : tid % g.K;
    const int b = b0 + lr;
    const bool inside = producer && lr < R && b < g.B && k < g.K;
    const size_t gi = (size_t)b * g.K + k;            // flattened (b, k)
    ConflictLane cf;
    if constexpr (CONF) cf.begin(*x, *fa, *fo, inside, b, k);
    int n = 0;
    if (inside && g.status[b] == 0) n = route_rows(g, b);
    const double *route = g.rows + (size_t)(inside ? b : 0) * (size_t)g.cap * 8;

    // the rollout's constants and start state
    TrackPlant pl;
    double L = g.L;
    bool valid = false;
    if (n > 0) {
        const double *p = g.perturb + (g.shared ? (size_t)k : gi) * 8;
        const double2 p01 = *(const double2 *)p, p23 = *(const double2 *)(p + 2), p45 = *(const double2 *)(p + 4),
                      p67 = *(const double2 *)(p + 6);
        const double tau = p67.x;
        valid = isfinite(p01.x) && isfinite(p01.y) && isfinite(p23.x) && isfinite(p23.y) && isfinite(p45.x) &&
                isfinite(p45.y) && isfinite(p67.x) && isfinite(p67.y) && p23.y > 0.0 && p45.x > 0.0 && p45.y > 0.0 && tau >= 0.0 &&
                p67.y >= 0.0;
        if (valid) {
            const double v0 = route[2], w0 = -route[5];
            pl.x = route[6] + p01.x;
            pl.y = route[7] + p01.y;
            pl.phi = -route[4] + p23.x;
            pl.wl = v0 - w0 * g.T / 2.0;
            pl.wr = v0 + w0 * g.T / 2.0;
            pl.gl = p23.y;
            pl.gr = p45.x;
            pl.tts = g.T * p45.y;
            pl.a = tau == 0.0 ? 1.0 : 1.0 - exp(-g.h / tau);
            if (p67.y > 0.0) L = p67.y;
        }
    }
    const int my_total = valid ? n + g.settle : 0;
    double maxe = -INFINITY;
    int mrow = -1, nsat = 0, arrived = -1;
    double *erow = EXEC && valid ? g.exec_rows + gi * (size_t)g.cap_exec * 8 : nullptr;
    ClearAcc acc;

    // the two pointers: the closest segment ic with P_ic, P_ic+1, P_ic+2 (A, Bp, Cn), its chord length and length; the
    // lookahead segment il with P_il, P_il+1 (Lp, Lq).  Both start on segment 0.
    int ic = 0, il = 0;
    PursuitPoint A{0.0, 0.0, 0.0}, Bp = A, Cn = A;
    double c_ic = 0.0, len_ic = 0.0, c_il = 0.0, len_il = 0.0;
    double lpx = 0.0, lpy = 0.0, lqx = 0.0, lqy = 0.0;
    double lastx = 0.0, lasty = 0.0, ux = 1.0, uy = 0.0;
    bool have_u = false;
    if (valid) {
        A = pursuit_point(route, 0);
        const PursuitPoint last = pursuit_point(route, n - 1);
        lastx = last.x;
        lasty = last.y;
        if (n >= 2) {
            Bp = pursuit_point(route, 1);
            if (n >= 3) Cn = pursuit_point(route, 2);
            len_ic = pursuit_len(A.x, A.y, Bp.x, Bp.y);
            lpx = A.x, lpy = A.y, lqx = Bp.x, lqy = Bp.y;
            len_il = len_ic;
        }
    }

    // SPLIT: in iteration ti tile ti is marched, tile ti - 1 cleared, tile ti - 2 folded; the steps of the longest rollout
    // of the workgroup set the number of tiles for every thread
    int wg_total = my_total;
    if constexpr (SPLIT) {
        __shared__ int s_total;
        if (tid == 0) s_total = 0;
        __syncthreads();
        if (my_total > 0) atomicMax(&s_total, my_total);
        __syncthreads();
        wg_total = s_total;
    }
    const int ntiles = (wg_total + kSplitRows - 1) / kSplitRows;
    const int nit = SPLIT ? ntiles + 2 : 1;
#pragma unroll 1
    for (int ti = 0; ti < nit; ti++) {
        int rbeg = 0, rstop = my_total;
        if (SPLIT) {
            rbeg = rstop = ti * kSplitRows;
            if (!producer) {
                if (ti >= 1 && ti <= ntiles)
                    sl.clear(*c, ti - 1, min(kSplitRows, wg_total - (ti - 1) * kSplitRows), tid - kTrackThreads,
                                (int)blockDim.x - kTrackThreads);
            } else {
                if (ti >= 2)
                    sl.fold(acc, ti - 2, (ti - 2) * kSplitRows, min(kSplitRows, wg_total - (ti - 2) * kSplitRows), my_total,
                               tid, c->margin);
                sl.cap[(size_t)(ti & 1) * kTrackThreads + tid] = acc.best;
                if (ti < ntiles) rstop = min(rbeg + kSplitRows, wg_total);
            }
        }
#pragma unroll 1
        for (int r = rbeg; r < rstop; r++) {
            if (SPLIT && r >= my_total) {
                sl.put(ti, r - rbeg, tid, NAN, 0.0, 0.0);
                continue;
            }
            // 1. the closest point: ic advances while the next segment is no farther
            double t = 1.0, D, ect, vt, sc = 0.0;
            bool at_end = true;
            if (n >= 2) {
                pursuit_project(A.x, A.y, Bp.x, Bp.y, pl.x, pl.y, t, D);
#pragma unroll 1
                while (ic < n - 2) {
                    double t1, D1;
                    pursuit_project(Bp.x, Bp.y, Cn.x, Cn.y, pl.x, pl.y, t1, D1);
                    if (!(D1 <= D)) break;
                    c_ic += len_ic;
                    A = Bp;
                    Bp = Cn;
                    ic++;
                    len_ic = pursuit_len(A.x, A.y, Bp.x, Bp.y);
                    if (ic + 2 < n) Cn = pursuit_point(route, ic + 2);
                    t = t1;
                    D = D1;
                }
                ect = sqrt(D);
                vt = A.v + t * (Bp.v - A.v);
                sc = c_ic + t * len_ic;
                at_end = ic == n - 2 && t == 1.0;
            } else {
                const double ex = pl.x - A.x, ey = pl.y - A.y;
                ect = sqrt(ex * ex + ey * ey);
                vt = A.v;
            }
            // 2. statistics
            if (ect > maxe) { maxe = ect; mrow = r; }
            // 3. the executed row
            if (EXEC) pl.write_row(erow, r, g.dt);
            if (MODE == kTrackClear) acc.take(c->s, c->margin, pl, r);
            if (SPLIT) sl.put(ti, r - rbeg, tid, -track_wrap(pl.phi), pl.x, pl.y);
            if constexpr (CONF) cf.take(*x, pl, r);
            // 4. arrival
            if (arrived < 0) {
                const double ex = lastx - pl.x, ey = lasty - pl.y;
                if (at_end || sqrt(ex * ex + ey * ey) <= g.atol) arrived = r;
            }
            // 5. the goal one lookahead further along the chord length, and the command (n >= 2: one row has arrived)
            double cl = 0.0, cr = 0.0;
            if (arrived < 0) {
                const double star = sc + L;
                if (il < ic) {
                    il = ic;
                    lpx = A.x, lpy = A.y, lqx = Bp.x, lqy = Bp.y;
                    c_il = c_ic;
                    len_il = len_ic;
                }
#pragma unroll 1
                while (il < n - 2 && c_il + len_il < star) {
                    c_il += len_il;
                    lpx = lqx, lpy = lqy;
                    il++;
                    const double2 q = *(const double2 *)(route + (size_t)(il + 1) * 8 + 6);
                    lqx = q.x, lqy = q.y;
                    len_il = pursuit_len(lpx, lpy, lqx, lqy);
                }
                // star >= c_(n-1)?  c_(il+1) >= star here unless il is the last segment, so short of it the two can only be
                // equal, with every later segment adding nothing
                const double cnext = c_il + len_il;
                bool beyond = il == n - 2 ? star >= cnext : cnext == star;
                if (beyond && il < n - 2) {
                    double px = lqx, py = lqy;
#pragma unroll 1
                    for (int j = il + 1; j < n - 1; j++) {
                        const double2 q = *(const double2 *)(route + (size_t)(j + 1) * 8 + 6);
                        if (cnext + pursuit_len(px, py, q.x, q.y) != cnext) { beyond = false; break; }
                        px = q.x, py = q.y;
                    }
                }
                double gx, gy;
                if (beyond) {
                    if (!have_u) {                       // the direction of the last segment with a length
                        have_u = true;
                        double qx = lastx, qy = lasty;
#pragma unroll 1
                        for (int j = n - 2; j >= 0; j--) {
                            const double2 q = *(const double2 *)(route + (size_t)j * 8 + 6);
                            const double l = pursuit_len(q.x, q.y, qx, qy);
                            if (l > 0.0) {
                                ux = (qx - q.x) / l;
                                uy = (qy - q.y) / l;
                                break;
                            }
                            qx = q.x, qy = q.y;
                        }
                    }
                    gx = lastx + (star - cnext) * ux;
                    gy = lasty + (star - cnext) * uy;
                } else {
                    double f = 0.0;
                    if (len_il != 0.0) f = fmin(fmax((star - c_il) / len_il, 0.0), 1.0);
                    gx = lpx + f * (lqx - lpx);
                    gy = lpy + f * (lqy - lpy);
                }
                double sp, cp;
                sincos(pl.phi, &sp, &cp);
                const double dx = gx - pl.x, dy = gy - pl.y;
                const double ly = cp * dy - sp * dx;
                const double a2 = dx * dx + dy * dy;
                const double kap = a2 == 0.0 ? 0.0 : 2.0 * ly / a2;
                const double spd = fmax(vt, g.vmin);
                cl = spd - spd * kap * g.T / 2.0;
                cr = spd + spd * kap * g.T / 2.0;
            }
            // 6. saturation, keeping c_L : c_R
            if (track_saturate(cl, cr, g.wmax)) nsat++;
            // 7. substeps: first-order wheel lag, then the exact arc
            pl.advance(cl, cr, g.nsub, g.h);
        }
        if (SPLIT) __syncthreads();
    }

    // kTrackConflict: the instants after the last executed row, the rollout parked at its pose
    if constexpr (CONF) cf.tail(*x, my_total);

    // the final position error against the last point, and the rollout's outputs
    const bool have = mrow >= 0;
    double cmin = INFINITY;
    int crow = -1, cother = -1;
    if (inside) {
        if (g.stats) {
            double2 *o = (double2 *)(g.stats + gi * 6);
            if (have) {
                const double ex = lastx - pl.x, ey = lasty - pl.y;
                o[0] = make_double2(maxe, sqrt(ex * ex + ey * ey));
                o[1] = make_double2(arrived >= 0 ? (double)arrived * g.dt : NAN, L);
                o[2] = make_double2(0.0, 0.0);
            } else {
                o[0] = o[1] = o[2] = make_double2(NAN, NAN);
            }
        }
        if (g.stat_rows) {
            int *o = g.stat_rows + gi * 4;
            o[0] = mrow;
            o[1] = have ? nsat : -1;
            o[2] = have ? arrived : -1;
            o[3] = have ? ic : -1;
        }
        rollout_outputs(g, gi, my_total, maxe, mrow);
        if (g.part_e) g.part_aux[gi] = arrived;
        if (MODE == kTrackClear || SPLIT) acc.store(*c, gi);
        if constexpr (CONF) cf.finish(*x, gi, cmin, crow, cother);
    }
    if (g.wpr > 1) return;                              // the route's summary: k_pursuit_reduce
    if (producer) {
        s_e[tid] = maxe;
        s_r[tid] = inside ? mrow : -1;
        s_a[tid] = arrived;
    }
    __syncthreads();
    if (inside && k == 0) {
        PursuitSummary sum;
#pragma unroll 1
        for (int kk = 0; kk < g.K; kk++) sum.take(s_e[tid + kk], s_r[tid + kk], s_a[tid + kk], kk, g.tol);
        sum.store(g, b);
    }
    if (MODE == kTrackClear || SPLIT) {                 // the clearance summary, over the same three columns
        __syncthreads();
        if (producer) {
            s_e[tid] = acc.best;
            s_r[tid] = inside ? acc.row : -1;
            s_a[tid] = acc.el;
        }
        __syncthreads();
        if (inside && k == 0 && c->summary()) {
            ClearSummary cs;
#pragma unroll 1
            for (int kk = 0; kk < g.K; kk++) cs.take(s_e[tid + kk], s_r[tid + kk], s_a[tid + kk], kk, c->margin);
            cs.store(*c, b);
        }
    }
    if constexpr (CONF) {                               // the conflict summary, over the same three columns
        __syncthreads();
        s_e[tid] = cmin;
        s_r[tid] = crow;
        s_a[tid] = cother;
        __syncthreads();
        if (inside && k == 0 && x->summary()) route_walk<ConflictSummary>(s_e + tid, s_r + tid, s_a + tid, g.K, x->margin).store(*x, b);
    }
}

template <bool EXEC>
__global__ __launch_bounds__(kTrackThreads) void k_pursuit_rollouts(PursuitArgs g)
{
    pursuit_rollouts<EXEC ? kTrackExec : kTrackPlain>(g, nullptr);
}

// vap_rollout_clearance: the same march, the clearance of every executed row taken in the lane that made it
__global__ __launch_bounds__(kTrackThreads) void k_pursuit_clearance(PursuitArgs g, TrackClear c)
{
    pursuit_rollouts<kTrackClear>(g, &c);
}

// the same with the clearance split off the rollout lanes (vap_track_common.h)
__global__ __launch_bounds__(kSplitThreads) void k_pursuit_clearance_split(PursuitArgs g, TrackClear c)
{
    pursuit_rollouts<kTrackSplit>(g, &c);
}

// vap_rollout_conflicts: the same march, the clearance of every executed row to the partner's routes taken in the lane
// that made it, and the parked instants after the march
__global__ __launch_bounds__(kTrackThreads) void k_pursuit_conflicts(PursuitArgs g, TrackConflict x, ConfFoot fa, ConfFoot fo)
{
    pursuit_rollouts<kTrackConflict>(g, nullptr, &x, &fa, &fo);
}

int pursuit_setup(const RolloutCall &c, const vap_pursuit *f, PursuitArgs &g)
{
    // host validation first: it needs no device
    if (!f) return vap_fail(VAP_ERR_INVALID, "null follower");
    if (!(f->track_width > 0.0) || !(f->lookahead > 0.0) || !(f->wheel_speed_max > 0.0) || !std::isfinite(f->track_width) ||
        !std::isfinite(f->lookahead) || !std::isfinite(f->wheel_speed_max))
        return vap_fail(VAP_ERR_INVALID, "pursuit: track_width, lookahead and wheel_speed_max must be positive and finite (got %g, %g, %g)",
                        f->track_width, f->lookahead, f->wheel_speed_max);
    if (!(f->min_speed >= 0.0) || !(f->arrive_tolerance >= 0.0) || !std::isfinite(f->min_speed) || !std::isfinite(f->arrive_tolerance))
        return vap_fail(VAP_ERR_INVALID, "pursuit: min_speed and arrive_tolerance must be >= 0 and finite (got %g, %g)", f->min_speed,
                        f->arrive_tolerance);
    VAP_TRY(rollout_check(c, "pursuit", *f, g));
    g.L = f->lookahead;
    g.vmin = f->min_speed;
    g.atol = f->arrive_tolerance;
    g.n_unfinished = c.n_unfinished;
    g.route_status = c.route_status;
    return VAP_OK;
}

int pursuit_launch(vap_ctx *ctx, PursuitArgs &g, TrackClear *clear, ConflictCall *conf)
{
    // context scratch: the routes' status words, then the partials
    long grid;
    VAP_TRY(rollout_place(ctx, g, g.summary(), 2, (((size_t)g.B * sizeof(int)) + 15) & ~(size_t)15, clear, grid, conf ? &conf->x : nullptr));
    g.status = (int *)ctx->track_part.ptr;
    hipLaunchKernelGGL(k_pursuit_check, dim3((unsigned)g.B), dim3(kCheckThreads), 0, ctx->stream, g);
    return rollout_run<PursuitSummary>(ctx, g, clear, grid,
                                       RolloutKernels<PursuitArgs>{k_pursuit_rollouts<false>, k_pursuit_rollouts<true>, k_pursuit_clearance,
                                                                   k_pursuit_clearance_split, k_pursuit_conflicts},
                                       conf);
}

}  // namespace vap

extern "C" {

int vap_pursuit_rollouts(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                         double time_step, const vap_pursuit *f, int K, int shared_perturb, const double *d_perturb,
                         double *d_stats, int *d_stat_rows, double *d_worst, double *d_mean, int *d_worst_rollout,
                         int *d_worst_row, int *d_n_exceeding, int *d_n_unfinished, int *d_route_status, long cap_exec,
                         double *d_exec_rows, int *d_exec_counts)
{
    using namespace vap;
    const RolloutCall call{B, capacity, d_rows, d_counts, counts_stride, time_step, K, shared_perturb, d_perturb, d_stats, d_stat_rows,
                           d_worst, d_mean, d_worst_rollout, d_worst_row, d_n_exceeding, d_n_unfinished, d_route_status, cap_exec,
                           d_exec_rows, d_exec_counts};
    PursuitArgs g{};
    VAP_TRY(pursuit_setup(call, f, g));
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;
    return pursuit_launch(ctx, g, nullptr);
}

}  // extern "C"
