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
//   rollouts a lane per rollout, vap_tracking.hip's route-to-workgroup mapping (K <= 256: 256 / K whole routes per
//            workgroup; K > 256: ceil(K / 256) workgroups per route).  Unlike RAMSETE's, the lanes of a route are not at
//            the same row: each carries its own closest segment ic and lookahead segment il, which only advance.  A lane
//            keeps the three points P_ic, P_ic+1, P_ic+2 and the two points P_il, P_il+1 in registers with the chord
//            length c and the segment length of each pointer; an advance loads one point (the K lanes of a route hit the
//            same few lines, L1 / L2 serve them) and costs one sqrt.  Both pointers form the same sum c_(i+1) = c_i +
//            len_i in index order, so c is the same number whichever pointer computed it.  The total chord length and
//            the last tangent are needed only once il has reached the last segment; they are formed there.  Nothing
//            waits across lanes: every loop is bounded by n.
//   summary  as vap_tracking.hip: K <= 256 the first lane of each route walks its K rollouts in LDS in ascending k;
//            K > 256 the partials go to context scratch and k_pursuit_reduce walks them, a lane per route.  No float
//            atomics, so two calls give the same bits.
//   modes    as vap_tracking.hip: pursuit_rollouts<MODE> is the march; k_pursuit_rollouts<false / true>,
//            k_pursuit_clearance and k_pursuit_clearance_split (vap_rollout_clearance.hip, through pursuit_setup /
//            pursuit_launch) instantiate it.  Only the split cuts the row loop into tiles with a barrier each.
#include <climits>
#include <cmath>
#include <cstdint>

#include "vap_internal.h"
#include "vap_track_common.h"

namespace vap {

constexpr int kCheckThreads = 256;

__global__ __launch_bounds__(kCheckThreads) void k_pursuit_check(PursuitArgs g)
{
    __shared__ int s_mask;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_mask = 0;
    __syncthreads();
    const long c = g.counts[(size_t)b * g.stride];
    const int n = (int)(c < 0 ? 0 : (c > g.cap ? g.cap : c));
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
        TrackSummary::take(e, r, kk, tol);
        nun += r >= 0 && arrived < 0 ? 1 : 0;
    }
    __device__ void store(const PursuitArgs &g, int b) const
    {
        TrackSummary::store(g, b);
        if (g.n_unfinished) g.n_unfinished[b] = nun;
    }
};

// The rollouts of one workgroup.  MODE: what becomes of the executed row (kTrackPlain, kTrackExec, kTrackClear,
// kTrackSplit); `c` is read with the last two only.
template <int MODE>
__device__ __forceinline__ void pursuit_rollouts(const PursuitArgs &g, const TrackClear *c)
{
    constexpr bool EXEC = MODE == kTrackExec, SPLIT = MODE == kTrackSplit;
    __shared__ double s_e[kTrackThreads];
    __shared__ int s_r[kTrackThreads], s_a[kTrackThreads];
    const int tid = threadIdx.x;
    const int R = g.R;
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
    const size_t gi = (size_t)b * g.K + k;            // flattened (b, k)
    int n = 0;
    if (inside && g.status[b] == 0) {
        const long c = g.counts[(size_t)b * g.stride];
        n = (int)(c < 0 ? 0 : (c > g.cap ? g.cap : c));
    }
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
                    split_clear(*c, s_pose, s_cap, ti - 1, min(kSplitRows, wg_total - (ti - 1) * kSplitRows), tid - kTrackThreads,
                                (int)blockDim.x - kTrackThreads);
            } else {
                if (ti >= 2)
                    split_fold(acc, s_pose, ti - 2, (ti - 2) * kSplitRows, min(kSplitRows, wg_total - (ti - 2) * kSplitRows), my_total,
                               tid, c->margin);
                s_cap[(size_t)(ti & 1) * kTrackThreads + tid] = acc.best;
                if (ti < ntiles) rstop = min(rbeg + kSplitRows, wg_total);
            }
        }
#pragma unroll 1
        for (int r = rbeg; r < rstop; r++) {
            if (SPLIT && r >= my_total) {
                split_put(s_pose, ti & 1, r - rbeg, tid, NAN, 0.0, 0.0);
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
            if (SPLIT) split_put(s_pose, ti & 1, r - rbeg, tid, -track_wrap(pl.phi), pl.x, pl.y);
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

    // the final position error against the last point, and the rollout's outputs
    const bool have = mrow >= 0;
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
        if (g.exec_counts) {
            g.exec_counts[gi * 2] = my_total;
            g.exec_counts[gi * 2 + 1] = 0;
        }
        if (g.part_e) {
            g.part_e[gi] = maxe;
            g.part_row[gi] = mrow;
            g.part_arr[gi] = arrived;
        }
        if (MODE == kTrackClear || SPLIT) acc.store(*c, gi);
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

// K > 256: per route, its rollouts' partials in ascending k
__global__ __launch_bounds__(64) void k_pursuit_reduce(PursuitArgs g)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= g.B) return;
    PursuitSummary sum;
#pragma unroll 1
    for (int kk = 0; kk < g.K; kk++) {
        const size_t p = (size_t)b * g.K + kk;
        sum.take(g.part_e[p], g.part_row[p], g.part_arr[p], kk, g.tol);
    }
    sum.store(g, b);
}

int pursuit_setup(int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride, double time_step,
                  const vap_pursuit *f, int K, int shared_perturb, const double *d_perturb, double *d_stats, int *d_stat_rows,
                  double *d_worst, double *d_mean, int *d_worst_rollout, int *d_worst_row, int *d_n_exceeding, int *d_n_unfinished,
                  int *d_route_status, long cap_exec, double *d_exec_rows, int *d_exec_counts, PursuitArgs &g)
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
    if (std::isnan(f->tolerance)) return vap_fail(VAP_ERR_INVALID, "pursuit: tolerance is NaN");
    if (!(time_step > 0.0) || !std::isfinite(time_step)) return vap_fail(VAP_ERR_INVALID, "time_step must be positive and finite (got %g)", time_step);
    if (f->n_substeps < 1 || f->n_substeps > 16) return vap_fail(VAP_ERR_INVALID, "pursuit: n_substeps %d outside 1..16", f->n_substeps);
    if (f->settle_rows < 0 || f->settle_rows > 10000) return vap_fail(VAP_ERR_INVALID, "pursuit: settle_rows %d outside 0..10000", f->settle_rows);
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
    g.L = f->lookahead;
    g.vmin = f->min_speed;
    g.atol = f->arrive_tolerance;
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
    g.n_unfinished = d_n_unfinished;
    g.route_status = d_route_status;
    g.cap_exec = cap_exec;
    g.exec_rows = d_exec_rows;
    g.exec_counts = d_exec_counts;
    return VAP_OK;
}

int pursuit_launch(vap_ctx *ctx, PursuitArgs &g, TrackClear *clear)
{
    const int B = g.B, K = g.K;
    const bool summary = g.worst || g.mean || g.worst_rollout || g.worst_row || g.n_exceeding || g.n_unfinished;
    // context scratch: the routes' status words, then (K > 256 with a summary) the rollouts' partials, then those of the
    // clearance summary
    const size_t status_bytes = (((size_t)B * sizeof(int)) + 15) & ~(size_t)15;
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
        if (summary) part_bytes = (size_t)B * (size_t)K * (sizeof(double) + 2 * sizeof(int));
    }
    if (grid > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "%d routes x %d rollouts: too many workgroups for one launch", B, K);
    VAP_TRY(ctx->ensure(ctx->track_part, status_bytes + part_bytes + clear_bytes));
    g.status = (int *)ctx->track_part.ptr;
    if (part_bytes) {
        const size_t np = (size_t)B * (size_t)K;
        g.part_e = (double *)((char *)ctx->track_part.ptr + status_bytes);
        g.part_row = (int *)(g.part_e + np);
        g.part_arr = g.part_row + np;
    }
    if (clear_bytes) clear_part_place(clear, (char *)ctx->track_part.ptr + status_bytes + part_bytes, B, K);

    hipLaunchKernelGGL(k_pursuit_check, dim3((unsigned)B), dim3(kCheckThreads), 0, ctx->stream, g);
    // the clearance split off the rollout lanes where every workgroup gets a CU of its own (K = 16 at config 3: one rollout
    // wave per SIMD, which cannot hide the clearance's loads); with more workgroups than CUs the lanes' own clearance,
    // several workgroups to a CU, measured faster
    const bool split = clear && grid <= track_cus(ctx->device);
    if (split)
        hipLaunchKernelGGL(k_pursuit_clearance_split, dim3((unsigned)grid), dim3(kSplitThreads), 0, ctx->stream, g, *clear);
    else if (clear)
        hipLaunchKernelGGL(k_pursuit_clearance, dim3((unsigned)grid), dim3(kTrackThreads), 0, ctx->stream, g, *clear);
    else if (g.exec_rows)
        hipLaunchKernelGGL(k_pursuit_rollouts<true>, dim3((unsigned)grid), dim3(kTrackThreads), 0, ctx->stream, g);
    else
        hipLaunchKernelGGL(k_pursuit_rollouts<false>, dim3((unsigned)grid), dim3(kTrackThreads), 0, ctx->stream, g);
    if (g.wpr > 1 && summary)
        hipLaunchKernelGGL(k_pursuit_reduce, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
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
    PursuitArgs g{};
    VAP_TRY(pursuit_setup(B, capacity, d_rows, d_counts, counts_stride, time_step, f, K, shared_perturb, d_perturb, d_stats,
                          d_stat_rows, d_worst, d_mean, d_worst_rollout, d_worst_row, d_n_exceeding, d_n_unfinished, d_route_status,
                          cap_exec, d_exec_rows, d_exec_counts, g));
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;
    return pursuit_launch(ctx, g, nullptr);
}

}  // extern "C"
