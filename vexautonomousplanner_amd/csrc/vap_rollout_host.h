// vap_rollout_host.h — the host side of the closed-loop rollouts (device side: vap_track_common.h).  An entry point fills a
// RolloutCall from its parameters; the follower's *_setup checks its own struct and calls rollout_check for everything the
// followers share (no device call up to here); rollout_place sizes the grid and the context scratch; rollout_run picks the
// kernel of the mode and launches it with the reduce kernels K > 256 needs.  vap_tracking.hip and vap_pursuit.hip define
// the *_setup / *_launch pairs below, so that vap_rollout_clearance, vap_rollout_conflicts and vap_odometry_rollouts run the
// same code.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include "vap_internal.h"
#include "vap_track_common.h"

namespace vap {

// the parameters every rollout entry point has
struct RolloutCall {
    int B;
    long capacity;
    const double *rows;
    const int *counts;
    int counts_stride;
    double time_step;
    int K, shared_perturb;
    const double *perturb;
    double *stats;
    int *stat_rows;
    double *worst, *mean;
    int *worst_rollout, *worst_row, *n_exceeding, *n_unfinished, *route_status;      // the last two: pure pursuit's, else NULL
    long cap_exec;
    double *exec_rows;
    int *exec_counts;
};

// The checks the followers share, in the order the entry points report them, and the shared kernel arguments.  F is
// vap_follower or vap_pursuit, already checked for its own fields; `who` prefixes the messages about it.
template <class F, class Args>
int rollout_check(const RolloutCall &c, const char *who, const F &f, Args &g)
{
    if (std::isnan(f.tolerance)) return vap_fail(VAP_ERR_INVALID, "%s: tolerance is NaN", who);
    if (!(c.time_step > 0.0) || !std::isfinite(c.time_step)) return vap_fail(VAP_ERR_INVALID, "time_step must be positive and finite (got %g)", c.time_step);
    if (f.n_substeps < 1 || f.n_substeps > 16) return vap_fail(VAP_ERR_INVALID, "%s: n_substeps %d outside 1..16", who, f.n_substeps);
    if (f.settle_rows < 0 || f.settle_rows > 10000) return vap_fail(VAP_ERR_INVALID, "%s: settle_rows %d outside 0..10000", who, f.settle_rows);
    if (c.K < 1 || c.K > 4096) return vap_fail(VAP_ERR_INVALID, "K = %d rollouts per route outside 1..4096", c.K);
    if (c.B < 0 || c.capacity < 0) return vap_fail(VAP_ERR_INVALID, "bad shape B=%d capacity=%ld", c.B, c.capacity);
    if (c.counts_stride < 1) return vap_fail(VAP_ERR_INVALID, "counts_stride must be >= 1 (got %d)", c.counts_stride);
    if (c.B > 0 && (!c.counts || (c.capacity > 0 && !c.rows))) return vap_fail(VAP_ERR_INVALID, "null rows / counts");
    if (c.B > 0 && !c.perturb) return vap_fail(VAP_ERR_INVALID, "null perturbation records");
    if (c.capacity + f.settle_rows > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld + settle rows above %d", c.capacity, INT_MAX);
    if (c.exec_rows && c.cap_exec < c.capacity + f.settle_rows)
        return vap_fail(VAP_ERR_INVALID, "cap_exec %ld below capacity + settle_rows = %ld", c.cap_exec, c.capacity + f.settle_rows);
    if ((((uintptr_t)c.rows | (uintptr_t)c.perturb | (uintptr_t)c.stats | (uintptr_t)c.exec_rows) & 15) != 0)
        return vap_fail(VAP_ERR_INVALID, "rows, perturbation records, stats and executed rows must be 16-byte aligned");
    g.rows = c.rows, g.counts = c.counts, g.cap = c.capacity, g.stride = c.counts_stride;
    g.B = c.B, g.K = c.K, g.shared = c.shared_perturb != 0, g.perturb = c.perturb;
    g.T = f.track_width, g.wmax = f.wheel_speed_max, g.tol = f.tolerance;
    g.dt = c.time_step, g.h = c.time_step / (double)f.n_substeps, g.nsub = f.n_substeps, g.settle = f.settle_rows;
    g.stats = c.stats, g.stat_rows = c.stat_rows;
    g.worst = c.worst, g.mean = c.mean, g.worst_rollout = c.worst_rollout, g.worst_row = c.worst_row, g.n_exceeding = c.n_exceeding;
    g.cap_exec = c.cap_exec, g.exec_rows = c.exec_rows, g.exec_counts = c.exec_counts;
    return VAP_OK;
}

// The launch shape (vap_track_common.h, the lane) and the context scratch: `head` bytes of the follower's own, then, for
// K > 256 with a summary, the rollouts' partials [B][K] of a double and part_ints ints (1: the row; 2: a third column
// too) rounded up to 16 bytes, then those of the clearance summary or of the conflict summary.  Fills g.R, g.wpr and the
// partials' pointers.
template <class Args>
int rollout_place(vap_ctx *ctx, Args &g, bool summary, int part_ints, size_t head, TrackClear *clear, long &grid, TrackConflict *conf = nullptr)
{
    const size_t np = (size_t)g.B * (size_t)g.K;
    size_t part_bytes = 0, clear_bytes = 0;
    if (g.K <= kTrackThreads) {
        g.R = kTrackThreads / g.K;
        g.wpr = 1;
        grid = ((long)g.B + g.R - 1) / g.R;
    } else {
        g.R = 1;
        g.wpr = (g.K + kTrackThreads - 1) / kTrackThreads;
        grid = (long)g.B * g.wpr;
        if (summary) part_bytes = (np * (sizeof(double) + (size_t)part_ints * sizeof(int)) + 15) & ~(size_t)15;
        if ((clear && clear->summary()) || (conf && conf->summary())) clear_bytes = np * (sizeof(double) + 2 * sizeof(int));
    }
    if (grid > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "%d routes x %d rollouts: too many workgroups for one launch", g.B, g.K);
    if (head + part_bytes + clear_bytes) VAP_TRY(ctx->ensure(ctx->track_part, head + part_bytes + clear_bytes));
    char *base = (char *)ctx->track_part.ptr + head;
    if (part_bytes) {
        g.part_e = (double *)base;
        g.part_row = (int *)(g.part_e + np);
        if (part_ints > 1) g.part_aux = g.part_row + np;
    }
    if (clear_bytes && clear) {
        clear->part_c = (double *)(base + part_bytes);
        clear->part_row = (int *)(clear->part_c + np);
        clear->part_el = clear->part_row + np;
    }
    if (clear_bytes && conf) {
        conf->part_c = (double *)(base + part_bytes);
        conf->part_row = (int *)(conf->part_c + np);
        conf->part_o = conf->part_row + np;
    }
    return VAP_OK;
}

// K > 256: the route summaries from the partials, after the rollout kernel
template <class Summary, class Args>
void rollout_reduce(vap_ctx *ctx, const Args &g)
{
    if (g.part_e)
        hipLaunchKernelGGL((k_route_reduce<Summary, Args>), dim3((unsigned)((g.B + 63) / 64)), dim3(64), 0, ctx->stream, g, g.B, g.K,
                           (const double *)g.part_e, (const int *)g.part_row, (const int *)g.part_aux, g.tol);
}

// CUs of a device: the split runs where every workgroup of the launch gets a CU of its own
inline int track_cus(int device)
{
    static int n[64] = {};
    const int d = device < 0 || device >= 64 ? 0 : device;
    if (n[d] == 0) {
        int cu = 0;
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cu <= 0) cu = 1;
        n[d] = cu;
    }
    return n[d];
}

// the clearance split off the rollout lanes: where every workgroup of the launch gets a CU of its own
inline bool rollout_split(vap_ctx *ctx, const TrackClear *clear, long grid)
{
    return clear && grid <= track_cus(ctx->device);
}

// vap_rollout_conflicts on the host: the kernel block and the two footprints that travel beside it
struct ConflictCall {
    TrackConflict x;
    ConfFoot fa, fo;
};

// a follower's kernels, one per mode (kTrackPlain, kTrackExec, kTrackClear, kTrackSplit, kTrackConflict)
template <class Args>
struct RolloutKernels {
    void (*plain)(Args);
    void (*exec)(Args);
    void (*clear)(Args, TrackClear);
    void (*split)(Args, TrackClear);
    void (*conflict)(Args, TrackConflict, ConfFoot, ConfFoot);
};

// The conflict kernels keep a rollout lane's state per partner in dynamic LDS, 4 KiB per partner.  With the kernel's own
// static LDS up to 64 KiB every device launches it as it is; above, the request has to fit the device's workgroup limit
// and is put to the runtime first.  Refused here, before anything is launched.
template <class Kernel>
int conflict_grant_lds(vap_ctx *ctx, Kernel kernel, int Bo, size_t dyn)
{
    hipFuncAttributes attr;
    HIP_TRY(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(kernel)));
    const size_t need = dyn + attr.sharedSizeBytes;
    if (need <= 64 * 1024) return VAP_OK;
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) lds_max = 0;
    const size_t avail = lds_max > 64 * 1024 ? (size_t)lds_max : (size_t)64 * 1024;
    if (need > avail)
        return vap_fail(VAP_ERR_UNSUPPORTED, "rollout conflicts against Bo=%d routes need %zu bytes of LDS; the device gives a workgroup %zu",
                        Bo, need, avail);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e != hipSuccess)
        return vap_fail(VAP_ERR_UNSUPPORTED, "rollout conflicts against Bo=%d routes need %zu bytes of LDS; the device gives a workgroup %zu "
                        "and the request was not granted (%s)", Bo, need, avail, hipGetErrorString(e));
    return VAP_OK;
}

// Enqueues the rollouts of a placed launch and the reduce kernels.  With `clear` the rollouts take the clearance of their
// executed rows (no executed rows are written then): split off the rollout lanes where every workgroup gets a CU of its own
// (K = 16 at config 3: one rollout wave per SIMD, which cannot hide the clearance's loads); with more workgroups than CUs
// the lanes' own clearance, several workgroups to a CU, measured faster
// With `conf` (and no `clear`) they take the clearance to the partner's routes instead, a lane per rollout.
template <class Summary, class Args>
int rollout_run(vap_ctx *ctx, Args &g, TrackClear *clear, long grid, const RolloutKernels<Args> &kn, ConflictCall *conf = nullptr)
{
    const dim3 blocks((unsigned)grid);
    const auto rollouts = g.exec_rows ? kn.exec : kn.plain;
    if (conf) {
        const size_t dyn = conflict_lds_bytes(conf->x.p.o.B);
        VAP_TRY(conflict_grant_lds(ctx, kn.conflict, conf->x.p.o.B, dyn));
        hipLaunchKernelGGL(kn.conflict, blocks, dim3(kTrackThreads), dyn, ctx->stream, g, conf->x, conf->fa, conf->fo);
    } else if (rollout_split(ctx, clear, grid)) {
        hipLaunchKernelGGL(kn.split, blocks, dim3(kSplitThreads), 0, ctx->stream, g, *clear);
    } else if (clear)
        hipLaunchKernelGGL(kn.clear, blocks, dim3(kTrackThreads), 0, ctx->stream, g, *clear);
    else
        hipLaunchKernelGGL(rollouts, blocks, dim3(kTrackThreads), 0, ctx->stream, g);
    rollout_reduce<Summary>(ctx, g);
    if (clear && clear->part_c)
        hipLaunchKernelGGL((k_route_reduce<ClearSummary, TrackClear>), dim3((unsigned)((g.B + 63) / 64)), dim3(64), 0, ctx->stream, *clear,
                           g.B, g.K, (const double *)clear->part_c, (const int *)clear->part_row, (const int *)clear->part_el, clear->margin);
    if (conf && conf->x.part_c)
        hipLaunchKernelGGL((k_route_reduce<ConflictSummary, TrackConflict>), dim3((unsigned)((g.B + 63) / 64)), dim3(64), 0, ctx->stream, conf->x,
                           g.B, g.K, (const double *)conf->x.part_c, (const int *)conf->x.part_row, (const int *)conf->x.part_o, conf->x.margin);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

// The two followers' calls in two halves: *_setup checks the host arguments (no device call) and fills the kernel arguments;
// *_launch sizes the grid and the context scratch and enqueues the kernels.
int tracking_setup(const RolloutCall &c, const vap_follower *f, TrackArgs &g);
int tracking_launch(vap_ctx *ctx, TrackArgs &g, TrackClear *clear, ConflictCall *conf = nullptr);
int pursuit_setup(const RolloutCall &c, const vap_pursuit *f, PursuitArgs &g);
int pursuit_launch(vap_ctx *ctx, PursuitArgs &g, TrackClear *clear, ConflictCall *conf = nullptr);

}  // namespace vap
