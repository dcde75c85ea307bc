// vap_rollout_clearance.hip — scene clearance of the disturbed rollouts (vap_rollout_clearance).
//
// vap_tracking_rollouts / vap_pursuit_rollouts can write every executed row of every rollout and vap_footprint_clearance
// can read them back: B x K x rows x 64 bytes through memory for five numbers per rollout.  This call runs the same
// rollouts and takes the clearance of an executed row where the follower's kernel would have written it, while the pose
// is in registers, so no executed row leaves the chip.  Definitions: include/vap.h.
//
// The kernels are the followers' own (vap_tracking.hip, vap_pursuit.hip) in two further modes.  kTrackClear: a lane per
// rollout, the march unchanged, and at step 3 row_clearance_capped (vap_footprint.h) of the pose write_row would store,
// heading = -wrap(phi), capped by the rollout's own minimum so far.  kTrackSplit: the same with the clearance taken by
// further lanes of the workgroup from poses the rollout lanes leave in LDS (vap_track_common.h); it runs where the launch
// has no more workgroups than the device has CUs, one rollout wave per SIMD, which cannot hide the clearance's loads.  A lane keeps (min, first row at it, element, first row below the margin, rows below) by the
// footprint kernel's rules; rows ascend in a lane, so no tie-break across lanes is needed.  The lanes of a wave are
// rollouts of the same few routes at the same row (RAMSETE) or near it (pure pursuit): their poses lie together and the
// culling decisions mostly agree across the wave.
//   summary  K <= 256: inside the follower's kernel, the first lane of each route walks its K rollouts in LDS in ascending
//            k after the follower's own summary.  K > 256: the rollouts' (clearance, row, element) go to context scratch
//            behind the follower's partials and k_route_reduce<ClearSummary> walks them, a lane per route, launched with
//            the follower's own reduce by rollout_run (vap_rollout_host.h).  No float atomics.
// This file holds the entry point; the scene is validated, packed and uploaded by vap_footprint.hip's host functions, the
// followers' arguments by tracking_setup / pursuit_setup.
#include "vap_rollout_host.h"

extern "C" {

int vap_rollout_clearance(vap_ctx *ctx, int follower_kind, const void *follower, int B, long capacity, const double *d_rows,
                          const int *d_counts, int counts_stride, double time_step, int K, int shared_perturb,
                          const double *d_perturb, int n_foot, const double *h_footprint, const double *h_field, int n_poly,
                          const int *h_poly_start, const double *h_poly_xy, int n_circle, const double *h_circles, double margin,
                          double *d_stats, int *d_stat_rows, double *d_worst, double *d_mean, int *d_worst_rollout,
                          int *d_worst_row, int *d_n_exceeding, int *d_n_unfinished, int *d_route_status, double *d_clearance,
                          int *d_clear_rows, double *d_worst_clearance, int *d_worst_clear_rollout, int *d_worst_clear_row,
                          int *d_worst_clear_element, double *d_mean_clearance, int *d_n_colliding, int *d_n_clear_valid)
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
    if (!std::isfinite(margin)) return vap_fail(VAP_ERR_INVALID, "margin must be finite");
    // the scene
    if (!h_footprint) return vap_fail(VAP_ERR_INVALID, "null footprint");
    VAP_TRY(check_convex(h_footprint, n_foot, "footprint", 0));
    double scale = 0.0;
    int nv = 0;
    VAP_TRY(check_scene(h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, scale, nv));
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;

    TrackClear c{};
    VAP_TRY(scene_pack(ctx, n_foot, h_footprint, h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, scale, nv, c.s));
    c.margin = margin;
    c.clearance = d_clearance;
    c.clear_rows = d_clear_rows;
    c.worst = d_worst_clearance;
    c.mean = d_mean_clearance;
    c.worst_rollout = d_worst_clear_rollout;
    c.worst_row = d_worst_clear_row;
    c.worst_element = d_worst_clear_element;
    c.n_colliding = d_n_colliding;
    c.n_valid = d_n_clear_valid;
    return pursuit ? pursuit_launch(ctx, pg, &c) : tracking_launch(ctx, tg, &c);
}

}  // extern "C"
