// vap_rollout_conflicts.hip — clearance of the disturbed rollouts to the partner's routines (vap_rollout_conflicts).
//
// vap_rollout_clearance asks whether a disturbed run still clears the scene; this call asks whether it still clears the
// partner.  The pair of calls that answers it writes every executed row of every rollout and packs all B x K executed
// routes a second time, once per distinct start shift.  Here the rollouts run as they do in the followers' own calls and a
// lane takes, where the executed row would be written, its clearance to every partner route at the same instant, the
// partner starting shift_rows + route_shift[b] + rollout_shift[k] rows late.  Definitions: include/vap.h.
//
//   pack     side O once, with shift 0, by the pack kernel of vap_footprint_conflicts (conf_pack_sides): {cx, cy, cos, sin},
//            32 B per row.  A lane reads O's row clamp(r - s, 0, n_o - 1) itself; lanes of a wave sit at the same instant, so
//            these loads are broadcasts or neighbours.
//   march    the followers' own (vap_tracking.hip, vap_pursuit.hip) in one further mode, kTrackConflict, a lane per rollout:
//            at step 3 the lane forms its packed pose with the pack kernel's own function (conf_pose, vap_conflict.h) and
//            takes pair_clearance against each partner's packed row, culled by row_culled against the pair's own threshold.
//            Per partner (minimum, first row at it, first row below the margin) live in dynamic LDS, [o][lane], 4 KiB per
//            partner (ConflictLane, vap_track_common.h).
//   tail     a pair is examined until max(n_a, n_o + s, 1).  After the march the lane takes the remaining instants with its
//            pose parked at the last executed one; where the partner has not started either, one evaluation stands for
//            the stretch, so the loop is bounded by the partner's rows, never by s.
//   summary  per rollout the lane's walk over its partners in ascending o; per route ConflictSummary as ClearSummary: K <=
//            256 in LDS inside the kernel, K > 256 from B x K partials behind the follower's by k_route_reduce.  No float
//            atomics.
// This file holds the entry point; the followers' arguments are checked by tracking_setup / pursuit_setup, the sides by
// conf_check_sides.
#include "vap_rollout_host.h"

extern "C" {

int vap_rollout_conflicts(vap_ctx *ctx, int follower_kind, const void *follower, int B, long capacity, const double *d_rows,
                          const int *d_counts, int counts_stride, double time_step, int K, int shared_perturb,
                          const double *d_perturb, int n_foot_a, const double *h_foot_a, int Bo, long cap_o, const double *d_rows_o,
                          const int *d_counts_o, int stride_o, int n_foot_o, const double *h_foot_o, double margin, int shift_rows,
                          const int *d_route_shift, const int *d_rollout_shift, double *d_stats, int *d_stat_rows, double *d_worst,
                          double *d_mean, int *d_worst_rollout, int *d_worst_row, int *d_n_exceeding, int *d_n_unfinished,
                          int *d_route_status, double *d_pair_clearance, int *d_pair_rows, double *d_conflict, int *d_conflict_rows,
                          double *d_worst_conflict, int *d_worst_conflict_rollout, int *d_worst_conflict_other,
                          int *d_worst_conflict_row, double *d_mean_conflict, int *d_n_conflicting, int *d_n_conflict_valid)
{
    using namespace vap;
    // host validation first: it needs no device
    if (follower_kind != VAP_FOLLOWER_RAMSETE && follower_kind != VAP_FOLLOWER_PURSUIT)
        return vap_fail(VAP_ERR_INVALID, "follower_kind %d is neither VAP_FOLLOWER_RAMSETE nor VAP_FOLLOWER_PURSUIT", follower_kind);
    const bool pursuit = follower_kind == VAP_FOLLOWER_PURSUIT;
    if (!pursuit && (d_n_unfinished || d_route_status))
        return vap_fail(VAP_ERR_INVALID, "d_n_unfinished and d_route_status are the pure-pursuit follower's: NULL with VAP_FOLLOWER_RAMSETE");
    const RolloutCall call{B, capacity, d_rows, d_counts, counts_stride, time_step, K, shared_perturb, d_perturb, d_stats, d_stat_rows,
                           d_worst, d_mean, d_worst_rollout, d_worst_row, d_n_exceeding, d_n_unfinished, d_route_status, 0, nullptr, nullptr};
    TrackArgs tg{};
    PursuitArgs pg{};
    if (pursuit) VAP_TRY(pursuit_setup(call, (const vap_pursuit *)follower, pg));
    else VAP_TRY(tracking_setup(call, (const vap_follower *)follower, tg));
    // the two sides: side A's rows are the rollouts', so only its footprint is checked here
    if (Bo < 1) return vap_fail(VAP_ERR_INVALID, "Bo = %d: at least one partner route", Bo);
    if (Bo > VAP_ROLLOUT_CONFLICT_OTHERS_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "Bo = %d partner routes above %d", Bo, VAP_ROLLOUT_CONFLICT_OTHERS_MAX);
    if (shift_rows < -kConflictShiftMax || shift_rows > kConflictShiftMax)
        return vap_fail(VAP_ERR_INVALID, "shift_rows %d outside +-%ld", shift_rows, kConflictShiftMax);
    const ConfInput a{0, 0, nullptr, nullptr, 1, n_foot_a, h_foot_a}, o{Bo, cap_o, d_rows_o, d_counts_o, stride_o, n_foot_o, h_foot_o};
    VAP_TRY(conf_check_shape("B", a, o));
    VAP_TRY(conf_check_sides(a, o, B > 0 ? Bo : 0, false, margin, false, "null rows / counts of side O"));
    // a horizon row is below n + 3 * 2^24 with n a row count of either side: it has to stay an int
    const int settle = pursuit ? pg.settle : tg.settle;
    const long row_max = (long)INT_MAX - 3 * kConflictShiftMax;
    if (capacity + settle > row_max || cap_o > row_max)
        return vap_fail(VAP_ERR_UNSUPPORTED, "capacity + settle_rows = %ld or cap_o = %ld above %ld rows: a shifted row index could pass %d",
                        capacity + settle, cap_o, row_max, INT_MAX);
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;

    const ConfHorizon ha = conf_horizon(0), ho = conf_horizon(cap_o);
    if ((long)Bo * ho.groups > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "%d partner routes of %ld rows: too many workgroups for one launch", Bo, cap_o);
    ConflictCall cc{};
    VAP_TRY(conf_pack_sides(ctx, a, o, 0, ha, ho, cc.fa, cc.fo, cc.x.p));
    TrackConflict &x = cc.x;
    x.fcx = cc.fa.cx;
    x.fcy = cc.fa.cy;
    x.radii = cc.fa.R + cc.fo.R;
    x.na = cc.fa.n;
    x.no = cc.fo.n;
    x.shift = shift_rows;
    x.route_shift = d_route_shift;
    x.rollout_shift = d_rollout_shift;
    x.margin = margin;
    x.pair_c = d_pair_clearance;
    x.pair_rows = d_pair_rows;
    x.conflict = d_conflict;
    x.conflict_rows = d_conflict_rows;
    x.worst = d_worst_conflict;
    x.mean = d_mean_conflict;
    x.worst_rollout = d_worst_conflict_rollout;
    x.worst_other = d_worst_conflict_other;
    x.worst_row = d_worst_conflict_row;
    x.n_conflicting = d_n_conflicting;
    x.n_valid = d_n_conflict_valid;
    return pursuit ? pursuit_launch(ctx, pg, nullptr, &cc) : tracking_launch(ctx, tg, nullptr, &cc);
}

}  // extern "C"
