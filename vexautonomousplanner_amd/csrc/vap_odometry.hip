// vap_odometry.hip — tracking rollouts that steer on a dead-reckoned pose with range resets (vap_odometry_rollouts).
//
// vap_tracking_rollouts feeds the follower the true pose; on a robot the pose is dead reckoning, pulled back by a wall-facing
// range sensor whenever its reading passes a gate.  This file rolls the same plant under the same RAMSETE follower, but the
// follower sees an estimate: integrated from the wheel speeds and the turn rate through an odometry record (an encoder factor
// per side, a gyro scale and drift), and reset in x or y by the readings vap_range_readings would give for the true pose.
// Definitions: include/vap.h.
//
// One kernel, a lane per rollout, built from the followers' common pieces (vap_track_common.h): RolloutLane's layout, R =
// 256 / K whole routes per workgroup for K <= 256, several workgroups per route above it; RowStage's five reference columns in
// double-buffered LDS tiles, the next tile's loads in flight while the current one is marched; PlantRecord's start state and
// ramsete_command on the control errors; the route summary in LDS (K <= 256) or by k_route_reduce, in ascending k.  The host
// checks and the grid are tracking_setup's and rollout_place's (vap_rollout_host.h).
// What is new is in the march:
//   resets    on a row r with r % every == 0 (the same rows for every lane of the workgroup) each sensor casts the true ray
//             through the scene (vap_raycast.h: the code vap_range.hip compiles, so the reading is that call's bits) and the
//             expected ray from the estimate against the walls.  The packed scene is staged in LDS once per workgroup when it
//             fits kOdoLdsDoubles (k_odometry_rollouts<true>), else read from the global block at wave-uniform addresses.  The
//             whole wave enters the cast, finished rollouts with live = false, so the element loops and the cull stay
//             wave-uniform.
//   estimate  after each of the plant's substeps the estimate's, from the wheel speeds and turn rate the plant just used.
//             With the ideal record and no start offset it repeats the plant's operations, so it equals the true pose bit
//             for bit and the call equals vap_tracking_rollouts.
// No executed rows are needed for the readings: the ray is cast on the pose while it is in registers.  No float atomics;
// two calls give the same bits.
#include <cstring>

#include "vap_raycast.h"
#include "vap_rollout_host.h"

namespace vap {
namespace {

constexpr int kOdoLdsDoubles = 2048;   // a packed scene of up to 16 KiB is staged in LDS (vap_range.hip's budget)

// the scene as vap_raycast.h reads it
struct OdoScene {
    const double *block;
    int o_poly, o_pv, o_circ, n_dbl, n_poly, n_circle, has_field, cull;
    double xmin, ymin, xmax, ymax, slack;
};

struct OdoArgs {
    TrackArgs t;                      // rows, follower, perturbation records, the tracking outputs; stats is [B][K][8] here
    OdoScene sc;
    const double *odo;                // [B][K][8] or [K][8]
    int shared_odo, n_sens, every;
    double gate, min_cos, gain;
    double sens[kRangeMaxSens][8];
    double *est_rows;                 // [B*K][cap_exec][4]
};

template <bool LDS>
__global__ __launch_bounds__(kTrackThreads) void k_odometry_rollouts(OdoArgs a)
{
    __shared__ double s_scene[LDS ? kOdoLdsDoubles : 1];
    const TrackArgs &g = a.t;
    const int tid = threadIdx.x;
    const int R = g.R, tile = g.tile, ns = a.n_sens;
    const RolloutLane ln(g, true);
    const double *S = a.sc.block;
    if (LDS) {                                        // RowStage::begin's first barrier covers these writes
        for (int i = tid; i < a.sc.n_dbl; i += kTrackThreads) s_scene[i] = a.sc.block[i];
        S = s_scene;
    }
    RowStage st;
    st.begin(g, ln.b0, true);
    const int wg_total = st.total;
    const int n = ln.lr < R ? st.n[ln.lr] : 0;
    const int b = ln.b;
    const size_t gi = ln.gi;

    // the rollout's constants and start state: the plant's and the estimate's
    TrackPlant pl;
    double hx = 0.0, hy = 0.0, hphi = 0.0;            // the estimate
    double encl = 1.0, encr = 1.0, hscale = 1.0, hdrift = 0.0, rscale = 1.0, rbias = 0.0;
    bool valid = false;
    if (ln.inside && n > 0) {
        const PlantRecord rec(g, ln);
        const double *o = a.odo + (a.shared_odo ? (size_t)ln.k : gi) * 8;
        const double2 o01 = *(const double2 *)o, o23 = *(const double2 *)(o + 2), o45 = *(const double2 *)(o + 4),
                      o67 = *(const double2 *)(o + 6);
        valid = rec.valid() && isfinite(o01.x) && isfinite(o01.y) && isfinite(o23.x) && isfinite(o23.y) && isfinite(o45.x) &&
                isfinite(o45.y) && isfinite(o67.x) && isfinite(o67.y) && o01.x > 0.0 && o01.y > 0.0 && o23.x > 0.0 && o45.x > 0.0;
        if (valid) {
            const double *row0 = g.rows + (size_t)b * (size_t)g.cap * 8;
            hx = row0[6];
            hy = row0[7];
            hphi = -row0[4];
            rec.start(g, row0, pl);
            encl = o01.x;
            encr = o01.y;
            hscale = o23.x;
            hdrift = o23.y;
            rscale = o45.x;
            rbias = o45.y;
        }
    }
    const int my_total = valid ? n + g.settle : 0;
    double maxe = -INFINITY, maxey = -INFINITY, maxeph = -INFINITY, maxest = -INFINITY, maxestph = -INFINITY;
    int mrow = -1, nsat = 0, nacc = 0, nrej = 0;
    double *erow = g.exec_rows && valid ? g.exec_rows + gi * (size_t)g.cap_exec * 8 : nullptr;
    double *hrow = a.est_rows && valid ? a.est_rows + gi * (size_t)g.cap_exec * 4 : nullptr;

    const int ntiles = st.tiles(g);
#pragma unroll 1
    for (int ti = 0; ti < ntiles; ti++) {
        const bool more = ti + 1 < ntiles;
        if (more) st.load(g, ti + 1);                  // in flight while this tile is marched
        const int r0 = ti * tile;
        const int rend = min(tile, wg_total - r0);
#pragma unroll 1
        for (int t = 0; t < rend; t++) {
            const int r = r0 + t;
            const bool act = r < my_total;
            // cos and sin of the estimated heading, once per row: the resets never change it
            double sh, ch;
            sincos(hphi, &sh, &ch);
            int mask = 0;
            // 1. resets (the whole wave; r, ns and every are the workgroup's)
            if (ns > 0 && r % a.every == 0 && __any(act)) {
                const double wphi = track_wrap(pl.phi);         // executed row r's heading is -wphi
                const bool bad = !(isfinite(wphi) && isfinite(pl.x) && isfinite(pl.y));
                double sn, c;
                sincos(wphi, &sn, &c);
#pragma unroll 1
                for (int s = 0; s < ns; s++) {
                    const double mx = a.sens[s][0], my = a.sens[s][1], bx = a.sens[s][2], by = a.sens[s][3];
                    // (a) the true reading
                    const double ox = pl.x + (c * mx - sn * my), oy = pl.y + (sn * mx + c * my);
                    const double ux = c * bx - sn * by, uy = sn * bx + c * by;
                    double best, bcos;
                    int face, el;
                    cast_scene(a.sc, S, act && !bad, ox, oy, ux, uy, ray_slack(a.sc, ox, oy), best, bcos, face, el);
                    const bool read = act && !bad && el != -2 && !(best < a.sens[s][4]) && !(best > a.sens[s][5]) &&
                                      !(bcos < a.sens[s][6]);   // status 0
                    if (read) {
                        const double z = rscale * best + rbias;
                        // (b) the expected reading: the estimate against the walls
                        const double eox = hx + (ch * mx - sh * my), eoy = hy + (sh * mx + ch * my);
                        const double eux = ch * bx - sh * by, euy = sh * bx + ch * by;
                        double that, hcos;
                        int hface, hel;
                        cast_wall(a.sc, eox, eoy, eux, euy, that, hcos, hface, hel);
                        if (hel == -1 && hcos >= a.min_cos && fabs(z - that) <= a.gate) {
                            // (c) the accepted correction
                            if (hface == 0 || hface == 2) hx += a.gain * (that - z) * eux;
                            else hy += a.gain * (that - z) * euy;
                            mask |= 1 << s;
                            nacc++;
                        } else {
                            nrej++;
                        }
                    }
                }
            }
            if (!act) continue;
            const double *q = st.row(g, ti, t, ln.lr);
            const double vr = q[0], phr = -q[R], wref = -q[2 * R], xr = q[3 * R], yr = q[4 * R];
            // 2. errors in the body frame: the true ones, and the ones the follower sees
            double sp, cp;
            sincos(pl.phi, &sp, &cp);
            const double dx = xr - pl.x, dy = yr - pl.y;
            const double ex = cp * dx + sp * dy, ey = cp * dy - sp * dx;
            const double eph = track_wrap(phr - pl.phi);
            const double epos = hypot(ex, ey);
            const double hdx = xr - hx, hdy = yr - hy;
            const double hex = ch * hdx + sh * hdy, hey = ch * hdy - sh * hdx;
            const double heph = track_wrap(phr - hphi);
            const double eest = hypot(hx - pl.x, hy - pl.y), eestph = fabs(track_wrap(hphi - pl.phi));
            // 3. statistics
            if (epos > maxe) { maxe = epos; mrow = r; }
            if (fabs(ey) > maxey) maxey = fabs(ey);
            if (fabs(eph) > maxeph) maxeph = fabs(eph);
            if (eest > maxest) maxest = eest;
            if (eestph > maxestph) maxestph = eestph;
            // 4. the executed row and the estimate row
            if (erow) pl.write_row(erow, r, g.dt);
            if (hrow) {
                double2 *o = (double2 *)(hrow + (size_t)r * 4);
                o[0] = make_double2(-track_wrap(hphi), hx);
                o[1] = make_double2(hy, (double)mask);
            }
            // 5. RAMSETE on the control errors
            double cl, cr;
            ramsete_command(g, vr, wref, hex, hey, heph, cl, cr);
            // 6. saturation, keeping c_L : c_R
            if (track_saturate(cl, cr, g.wmax)) nsat++;
            // 7. substeps: the plant's, then the estimate's from the wheel speeds and the turn rate the plant just used
#pragma unroll 1
            for (int s = 0; s < g.nsub; s++) {
                pl.advance(cl, cr, 1, g.h);
                const double hv = (encl * (pl.gl * pl.wl) + encr * (pl.gr * pl.wr)) / 2.0;
                const double om = (pl.gr * pl.wr - pl.gl * pl.wl) / pl.tts;
                const double dl = (hscale * om) * g.h + hdrift * g.h;
                const double hu = dl / 2.0;
                double sa, ca;
                sincos(hphi + hu, &sa, &ca);
                const double hd = hv * g.h * track_sinc(hu, sin(hu));
                hx += hd * ca;
                hy += hd * sa;
                hphi += dl;
            }
        }
        if (more) st.store(g, (ti + 1) & 1);
        __syncthreads();
    }

    // final errors against row n - 1, and the rollout's outputs
    const bool have = mrow >= 0;
    if (ln.inside) {
        double fpos = NAN, fphi = NAN, fest = NAN;
        if (have) {
            const double *ql = g.rows + ((size_t)b * (size_t)g.cap + (size_t)(n - 1)) * 8;
            fpos = hypot(ql[6] - pl.x, ql[7] - pl.y);
            fphi = fabs(track_wrap(-ql[4] - pl.phi));
            fest = hypot(hx - pl.x, hy - pl.y);
        }
        if (g.stats) {
            double2 *o = (double2 *)(g.stats + gi * 8);
            o[0] = make_double2(have ? maxe : NAN, have ? maxey : NAN);
            o[1] = make_double2(have ? maxeph : NAN, fpos);
            o[2] = make_double2(fphi, have ? maxest : NAN);
            o[3] = make_double2(have ? maxestph : NAN, fest);
        }
        if (g.stat_rows) {
            int *o = g.stat_rows + gi * 4;
            o[0] = mrow;
            o[1] = have ? nsat : -1;
            o[2] = have ? nacc : -1;
            o[3] = have ? nrej : -1;
        }
        rollout_outputs(g, gi, my_total, maxe, mrow);
    }
    if (g.wpr > 1) return;                              // the route's summary: k_route_reduce
    // the route's summary inside the workgroup: the stage buffers are free (the last barrier is behind every thread)
    double *s_e = st.buf;
    int *s_r = st.n;
    __syncthreads();                                    // st.n was read above
    s_e[tid] = maxe;
    s_r[tid] = ln.inside ? mrow : -1;
    __syncthreads();
    route_summary<TrackSummary>(g, ln, g.K, s_e, s_r, nullptr, g.tol);
}

}  // namespace
}  // namespace vap

extern "C" {

int vap_odometry_rollouts(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                          double time_step, const vap_follower *f, int K, int shared_perturb, const double *d_perturb,
                          int shared_odometry, const double *d_odometry, int n_sens, const double *h_sensors,
                          const vap_reset_rule *rule, const double *h_field, int n_poly, const int *h_poly_start,
                          const double *h_poly_xy, int n_circle, const double *h_circles, double *d_stats, int *d_stat_rows,
                          double *d_worst, double *d_mean, int *d_worst_rollout, int *d_worst_row, int *d_n_exceeding,
                          long cap_exec, double *d_exec_rows, int *d_exec_counts, double *d_est_rows)
{
    using namespace vap;
    // host validation first: it needs no device
    OdoArgs a{};
    TrackArgs &g = a.t;
    const RolloutCall call{B, capacity, d_rows, d_counts, counts_stride, time_step, K, shared_perturb, d_perturb, d_stats, d_stat_rows,
                           d_worst, d_mean, d_worst_rollout, d_worst_row, d_n_exceeding, nullptr, nullptr, cap_exec, d_exec_rows,
                           d_exec_counts};
    VAP_TRY(tracking_setup(call, f, g));
    if (B > 0 && !d_odometry) return vap_fail(VAP_ERR_INVALID, "null odometry records");
    if ((((uintptr_t)d_odometry | (uintptr_t)d_est_rows) & 15) != 0)
        return vap_fail(VAP_ERR_INVALID, "odometry records and estimate rows must be 16-byte aligned");
    if (d_est_rows && cap_exec < capacity + f->settle_rows)
        return vap_fail(VAP_ERR_INVALID, "cap_exec %ld below capacity + settle_rows = %ld", cap_exec, capacity + f->settle_rows);
    if (n_sens < 0 || n_sens > kRangeMaxSens) return vap_fail(VAP_ERR_INVALID, "%d sensors (0..%d)", n_sens, kRangeMaxSens);
    if (n_sens > 0 && !rule) return vap_fail(VAP_ERR_INVALID, "null reset rule with %d sensors", n_sens);
    if (n_sens > 0) VAP_TRY(check_sensor_rows(n_sens, h_sensors));
    if (rule) {
        if (!(rule->gate >= 0.0) || !std::isfinite(rule->gate)) return vap_fail(VAP_ERR_INVALID, "reset rule: gate %g must be >= 0 and finite", rule->gate);
        if (!(0.0 <= rule->min_cos && rule->min_cos <= 1.0)) return vap_fail(VAP_ERR_INVALID, "reset rule: min_cos %g outside [0, 1]", rule->min_cos);
        if (!(0.0 <= rule->gain && rule->gain <= 1.0)) return vap_fail(VAP_ERR_INVALID, "reset rule: gain %g outside [0, 1]", rule->gain);
        if (rule->every < 1 || rule->every > 10000) return vap_fail(VAP_ERR_INVALID, "reset rule: every %d outside 1..10000", rule->every);
    }
    double scale = 0.0;
    int nv = 0;
    VAP_TRY(check_scene(h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, scale, nv));
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;

    a.odo = d_odometry;
    a.shared_odo = shared_odometry != 0;
    a.n_sens = n_sens;
    a.est_rows = d_est_rows;
    a.every = 1;
    if (n_sens > 0) {
        a.every = rule->every;
        a.gate = rule->gate;
        a.min_cos = rule->min_cos;
        a.gain = rule->gain;
        std::memcpy(a.sens, h_sensors, (size_t)n_sens * 8 * sizeof(double));
        OdoScene &sc = a.sc;
        SceneLayout blk;
        VAP_TRY(scene_block(ctx, 0, nullptr, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, nv, blk));
        sc.o_poly = blk.o_poly, sc.o_pv = blk.o_pv, sc.o_circ = blk.o_circ, sc.n_dbl = blk.n_dbl;
        sc.block = (const double *)ctx->scene.ptr;
        sc.n_poly = n_poly;
        sc.n_circle = n_circle;
        sc.has_field = h_field ? 1 : 0;
        if (h_field) sc.xmin = h_field[0], sc.ymin = h_field[1], sc.xmax = h_field[2], sc.ymax = h_field[3];
        sc.slack = kCullSlack * (1.0 + scale);
        sc.cull = ctx->footprint_cull;
    }

    long grid;
    VAP_TRY(rollout_place(ctx, g, g.summary(), 1, 0, nullptr, grid));
    g.tile = stage_tile(g.R, false);
    if (n_sens > 0 && a.sc.n_dbl > kOdoLdsDoubles)
        hipLaunchKernelGGL(k_odometry_rollouts<false>, dim3((unsigned)grid), dim3(kTrackThreads), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(k_odometry_rollouts<true>, dim3((unsigned)grid), dim3(kTrackThreads), 0, ctx->stream, a);
    rollout_reduce<TrackSummary>(ctx, g);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
