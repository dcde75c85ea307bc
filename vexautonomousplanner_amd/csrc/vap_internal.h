// vap_internal.h — context and error plumbing shared by the C-ABI translation units.
#pragma once
#include "../../include/vap.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

int vap_fail(int status, const char *fmt, ...);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return vap_fail(VAP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define VAP_TRY(expr)            \
    do {                         \
        int s_ = (expr);         \
        if (s_ != VAP_OK) return s_; \
    } while (0)

struct VapBuffer {
    void *ptr = nullptr;
    size_t cap = 0;
};

// What the last sampling or profile call left on the context, for the calls that take NULL as "the context's own"
// ("What a call leaves on the context").  leave() is its one writer — apart from the two tags a
// later call withdraws: rows (VAP_OPT_F32_RECURRENCE) and vres_for (every velocity pass) — and vap_ctx_state.h its readers.
enum VapRows { VAP_ROWS_NONE, VAP_ROWS_DTH, VAP_ROWS_HI };
struct VapLeft {
    int tab_B = 0, tab_W = 0;   // seg / lut hold the tables of a tab_B x tab_W batch:
    int NS = 0;                 //   > 0: of routes with up to NS splines each (with sptab / nspl), 0: of plain paths
    int B = 0, W = 0, S = 0;    // aux / runs hold the distance grid of a B x W x S batch
    // rows for a velocity pass of B x S with d_dtheta == NULL:
    //   VAP_ROWS_HI:  k64 / dth64 hold the fp64 curvature and |dtheta| rows of a VAP_F32 call (fused or staged)
    //   VAP_ROWS_DTH: dth holds the |dtheta| rows in rows_dt (the fused calls only; curvature comes from the caller)
    VapRows rows = VAP_ROWS_NONE;
    int rows_dt = 0;            // dtype of the call that left the grid
    // VAP_F32 with the fp64 recurrence (and VAP_OPT_TIME_DOMAIN_RESIDUAL on): the velocity pass also leaves, for the
    // time-domain entry points, the fp32 residual row v64 - (double)(float)v64 of the fp32 velocity row vres_for of a
    // [vres_B][vres_S] batch in `vres` (the lane-per-path kernel writes it itself; the others leave fp64 velocities in
    // `vhi` / `ufwd`, converted right after the launch).  Row + residual is the fp64 velocity to 2^-48.
    const void *vres_for = nullptr;
    int vres_B = 0, vres_S = 0;

    bool routes() const { return NS > 0; }
    // Grid and rows of a B x W x S batch in dt, NS as given; with `tables` also its tables.  Without (vap_sample: the
    // tables are the caller's) tab_B x tab_W stay as they are, now under the new NS.
    void leave(int B_, int W_, int S_, vap_dtype dt, VapRows r, int NS_, bool tables)
    {
        B = B_, W = W_, S = S_;
        rows = r;
        rows_dt = dt;
        NS = NS_;
        if (tables) tab_B = B_, tab_W = W_;
    }
};

struct vap_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    bool timing = false;
    int velocity_kernel = 0;  // VAP_OPT_VELOCITY_KERNEL
    int f32_recurrence = 0;   // VAP_OPT_F32_RECURRENCE (VAP_RECURRENCE_F64 = 0: the default)
    hipEvent_t ev[VAP_T_COUNT + 1] = {};
    VapLeft left;
    // scratch arena (grow-only, reused across calls); `owned`: every buffer ensure() has allocated, for vap_ctx_destroy
    std::vector<VapBuffer *> owned;
    VapBuffer seg, power, lut, aux, runs, meta, dth, flags, io[8], small_in, small_out, small_seg, small_lut;
    VapBuffer ufwd, lstate, lcount;   // long-row velocity pass
    VapBuffer vhi, vres;              // fp64 velocities behind an fp32 row, and their fp32 residual (VapLeft::vres_for)
    int keep_residual = 1;    // VAP_OPT_TIME_DOMAIN_RESIDUAL
    int time_kernel = 0;      // VAP_OPT_TIME_KERNEL
    VapBuffer k64, dth64;             // fp64 curvature / |dtheta| rows behind fp32 outputs (VAP_RECURRENCE_F64)
    VapBuffer sptab, nspl;            // spline tables of the last vap_profile_routes batch
    // vap_footprint_clearance: the packed scene is built in pinned host memory and uploaded on the stream; scene_ev marks
    // the end of the last upload, which the next call waits for before it rewrites the host block
    int footprint_cull = 1;           // VAP_OPT_FOOTPRINT_CULL
    VapBuffer scene;
    void *scene_host = nullptr;
    size_t scene_host_cap = 0;
    hipEvent_t scene_ev = nullptr;
    // vap_footprint_conflicts: packed poses and per-64-row bounding circles of either side, per-tile partial results
    VapBuffer conf_pack_a, conf_pack_o, conf_blk_a, conf_blk_o, conf_part;
    // vap_tracking_rollouts with more than 256 rollouts per route: per-rollout (max e_pos, row) for the reduce kernel
    VapBuffer track_part;
    // vap_plan_seeds: the grid's free mask, and the traced cell lists (one per resident workgroup)
    VapBuffer plan_free, plan_path;
    // vap_velocity_conditioning: the probes' squared velocities of one launch, at most cond_scratch_mb MiB of them
    VapBuffer cond_u;
    int cond_scratch_mb = 512;        // VAP_OPT_CONDITIONING_SCRATCH_MB
    // vap_drive_audit: the routes' status words and the per-tile partial peaks and counts
    VapBuffer drive_part;
    // vap_range_readings: the per-tile records (min / max valid range, counts per status, the channels' gap records)
    VapBuffer range_part;

    int ensure(VapBuffer &b, size_t bytes)
    {
        if (bytes <= b.cap) return VAP_OK;
        if (b.ptr) {
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(hipFree(b.ptr));
            b.ptr = nullptr;
            b.cap = 0;
        } else {
            owned.push_back(&b);    // its first allocation (or the one after a failed one: vap_ctx_destroy frees a buffer once)
        }
        size_t want = bytes + bytes / 8 + 256;
        HIP_TRY(hipMalloc(&b.ptr, want));
        b.cap = want;
        return VAP_OK;
    }
};

int vap_set_device(vap_ctx *ctx);

// rows of an in-place turn of `angle` radians: turn_profile(...).n of vap_turn.h, in fp64 so that the caller can bound it
// (vap_routine_timeline, vap_plan_order_timed)
inline double vap_turn_rows_host(double angle, double vmax, double amax, double tw, double dt)
{
    const double arc = std::fabs(angle) * tw / 2;
    double t_acc = vmax / amax, total;
    const double d_acc = 0.5 * amax * (t_acc * t_acc);
    if (2 * d_acc > arc) total = 2 * std::sqrt(arc / amax);
    else total = 2 * t_acc + (arc - 2 * d_acc) / vmax;
    return std::ceil((total + dt) / dt);
}
