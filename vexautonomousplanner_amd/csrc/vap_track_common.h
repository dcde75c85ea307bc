// vap_track_common.h — the device side of the closed-loop rollouts (vap_tracking.hip: RAMSETE; vap_pursuit.hip: pure
// pursuit; vap_odometry.hip: RAMSETE on an estimate; vap_rollout_clearance.hip: two further modes of the first two;
// vap_rollout_conflicts.hip: one more).
// A follower file holds its march, its statistics and its kernels; everything around the march is here, once (pure pursuit
// keeps its own lane mapping, record parsing, split schedule and summary walk, see PursuitArgs):
//   1. the plant           the angle wrap, sinc, the saturation, TrackPlant
//   2. the arguments       RolloutArgs and what TrackArgs adds; PursuitArgs, which keeps a block of its own; TrackClear for
//                          the clearance modes; the RAMSETE command (ramsete_command)
//   3. the lane            which rollout a lane walks (the struct RolloutLane), a route's rows (route_rows), the
//                          perturbation record and the plant's start state (PlantRecord)
//   4. the row stage       RowStage: the routes' rows in double-buffered LDS tiles
//   5. the clearance       ClearAcc, and SplitLds: the clearance split off the rollout lanes (kTrackSplit)
//                          ConflictLane: a rollout's clearance to the partner's routes (kTrackConflict; TrackConflict)
//   6. the outputs         a rollout's common outputs, the fixed-order summaries of a route's rollouts (TrackSummary,
//                          ClearSummary, ConflictSummary), the walk over them (route_walk) in LDS or, for K > 256, in k_route_reduce
// The host side (the argument checks, the grid, the launches) is vap_rollout_host.h.
#pragma once
#include <cmath>

#include "vap_conflict.h"
#include "vap_footprint.h"

namespace vap {

constexpr int kTrackThreads = 256;
constexpr double kPi = 3.14159265358979323846;

// ---- 1. the plant -------------------------------------------------------------------------------------------------------
// ((a + pi) mod 2 pi) - pi with the floored mod (MPG:560-562); fmod is exact
__device__ __forceinline__ double track_wrap(double a)
{
    double m = fmod(a + kPi, 2.0 * kPi);
    if (m < 0.0) m += 2.0 * kPi;
    return m - kPi;
}

__device__ __forceinline__ double track_sinc(double x, double sin_x)
{
    return fabs(x) < 1e-4 ? 1.0 - x * x / 6.0 : sin_x / x;
}

// wheel-speed saturation that keeps c_L : c_R (hence the curvature); true where the row is saturated
__device__ __forceinline__ bool track_saturate(double &cl, double &cr, double wmax)
{
    const double mx = fmax(fabs(cl), fabs(cr));
    if (mx > wmax) {
        const double scale = wmax / mx;
        cl *= scale;
        cr *= scale;
        return true;
    }
    return false;
}

// the plant of one rollout: the wheel gains, T * track_scale, the lag's a = 1 - exp(-h / tau); the pose, the actual wheel
// speeds and the distance travelled
struct TrackPlant {
    double gl = 1.0, gr = 1.0, tts = 1.0, a = 1.0;
    double x = 0.0, y = 0.0, phi = 0.0, wl = 0.0, wr = 0.0, dist = 0.0, vprev = 0.0;

    // the executed row r in the time-profile layout, four 16-byte stores
    __device__ __forceinline__ void write_row(double *erow, int r, double dt)
    {
        const double v = (gl * wl + gr * wr) / 2.0;
        const double om = (gr * wr - gl * wl) / tts;
        double2 *o = (double2 *)(erow + (size_t)r * 8);
        o[0] = make_double2((double)r * dt, dist);
        o[1] = make_double2(v, r > 0 ? (v - vprev) / dt : 0.0);
        o[2] = make_double2(-track_wrap(phi), -om);
        o[3] = make_double2(x, y);
        vprev = v;
    }

    // nsub substeps of h towards the commands: first-order wheel lag, then the exact arc
    __device__ __forceinline__ void advance(double cl, double cr, int nsub, double h)
    {
#pragma unroll 1
        for (int s = 0; s < nsub; s++) {
            wl += (cl - wl) * a;
            wr += (cr - wr) * a;
            const double v = (gl * wl + gr * wr) / 2.0;
            const double om = (gr * wr - gl * wl) / tts;
            const double u = om * h / 2.0;
            double sa, ca;
            sincos(phi + u, &sa, &ca);
            const double d = v * h * track_sinc(u, sin(u));
            x += d * ca;
            y += d * sa;
            phi += om * h;
            dist += fabs(d);
        }
    }
};

// ---- 2. the arguments ---------------------------------------------------------------------------------------------------
struct RolloutArgs {
    const double *rows;       // [B][cap][8]
    const int *counts;
    long cap;
    int stride, B, K, shared;
    const double *perturb;    // [B][K][8] or [K][8]
    double T, wmax, tol, dt, h;
    int nsub, settle;
    double *stats;            // [B][K][6] (odometry: [8])
    int *stat_rows;           // [B][K][2] (pure pursuit, odometry: [4])
    double *worst, *mean;     // [B]
    int *worst_rollout, *worst_row, *n_exceeding;
    long cap_exec;
    double *exec_rows;        // [B*K][cap_exec][8]
    int *exec_counts;         // [B*K][2]
    double *part_e;           // K > 256: [B][K] the rollouts' maximum error (row < 0: takes no part)
    int *part_row, *part_aux; // ... its row; part_aux: a third column for k_route_reduce, NULL here
    int R, tile, wpr;         // routes per workgroup, rows per tile of the row stage (RAMSETE, odometry), workgroups per route
    __host__ __device__ bool summary() const { return worst || mean || worst_rollout || worst_row || n_exceeding; }
};

struct TrackArgs : RolloutArgs {
    double b, two_zeta;
};

// Pure pursuit's block is its own, in its own field order, and its march keeps its own lane mapping, record parsing, split
// schedule and summary walk (vap_pursuit.hip): on the shared base and pieces k_pursuit_clearance spilled 129 SGPRs to VGPR
// lanes instead of 95, and with single pieces shared the split kernel's scratch grew above 204 B.  The
// shared pieces that take any argument block (route_rows, rollout_outputs, the host's rollout_check / rollout_place /
// rollout_run) read it by field name.
struct PursuitArgs {
    const double *rows;       // [B][cap][8]
    const int *counts;
    long cap;
    int stride, B, K, shared;
    const double *perturb;    // [B][K][8] or [K][8]
    double T, L, vmin, atol, wmax, tol, dt, h;
    int nsub, settle;
    double *stats;            // [B][K][6]
    int *stat_rows;           // [B][K][4]
    double *worst, *mean;     // [B]
    int *worst_rollout, *worst_row, *n_exceeding, *n_unfinished;
    int *status;              // [B] context scratch: the check kernel's mask
    int *route_status;        // [B] the caller's, or NULL
    long cap_exec;
    double *exec_rows;        // [B*K][cap_exec][8]
    int *exec_counts;         // [B*K][2]
    double *part_e;           // K > 256: [B][K] max e_ct (row < 0: takes no part)
    int *part_row, *part_aux; // ... its row and the row of arrival
    int R, wpr;               // routes per workgroup, workgroups per route
    __host__ __device__ bool summary() const { return worst || mean || worst_rollout || worst_row || n_exceeding || n_unfinished; }
};

// What a rollout kernel does with the executed row r (include/vap.h, step 3): nothing, write it, take its scene clearance
// while the pose is in registers, or hand the pose to further lanes of the workgroup that take it (vap_rollout_clearance);
// or take its clearance to the partner's routes at the same instant (vap_rollout_conflicts).
enum { kTrackPlain = 0, kTrackExec = 1, kTrackClear = 2, kTrackSplit = 3, kTrackConflict = 4 };

// vap_rollout_clearance: the scene, the margin and the clearance outputs beside a follower's own arguments.
struct TrackClear {
    FootScene s;
    double margin;
    double *clearance;        // [B][K]
    int *clear_rows;          // [B][K][4] = first row at the minimum, element, first row below margin, rows below
    double *worst, *mean;     // [B]
    int *worst_rollout, *worst_row, *worst_element, *n_colliding, *n_valid;
    double *part_c;           // K > 256: [B][K] clearance (row < 0: takes no part)
    int *part_row, *part_el;
    __host__ __device__ bool summary() const { return worst || mean || worst_rollout || worst_row || worst_element || n_colliding || n_valid; }
};

// vap_rollout_conflicts: the partner's routes (side O, packed once with shift 0), the two footprints' call constants, the
// shifts and the conflict outputs beside a follower's own arguments.  The footprints' vertex tables travel beside it.
constexpr int kConflictOthersMax = 16;     // VAP_ROLLOUT_CONFLICT_OTHERS_MAX
constexpr long kConflictShiftMax = 1L << 24;
struct TrackConflict {
    ConfPacked p;             // pack_o, Tpo, o (counts, Bo), slack, cull; side A is the rollout lanes'
    double fcx, fcy, radii;   // footprint A's bounding-circle centre in the body frame; R_a + R_o
    int na, no;               // vertices of the two footprints
    long shift;               // the host's shift_rows
    const int *route_shift, *rollout_shift;   // [B], [K] or NULL
    double margin;
    double *pair_c;           // [B][K][Bo]
    int *pair_rows;           // [B][K][Bo][2] = first row at the minimum, first row below the margin
    double *conflict;         // [B][K]
    int *conflict_rows;       // [B][K][4] = other at the minimum, its row, pairs below the margin, earliest first row
    double *worst, *mean;     // [B]
    int *worst_rollout, *worst_other, *worst_row, *n_conflicting, *n_valid;
    double *part_c;           // K > 256: [B][K] conflict clearance (row < 0: takes no part)
    int *part_row, *part_o;
    __host__ __device__ bool summary() const { return worst || mean || worst_rollout || worst_other || worst_row || n_conflicting || n_valid; }
};

// dynamic LDS of a conflict kernel: a rollout lane's (minimum, its row, first row below the margin) per partner
inline size_t conflict_lds_bytes(int Bo) { return (size_t)Bo * kTrackThreads * (sizeof(double) + 2 * sizeof(int)); }

// RAMSETE's command from the reference (v_r, omega_r) and the errors in the body frame, before the saturation
__device__ __forceinline__ void ramsete_command(const TrackArgs &g, double vr, double wref, double ex, double ey, double eph, double &cl, double &cr)
{
    double se, ce;
    sincos(eph, &se, &ce);
    const double kk = g.two_zeta * sqrt(wref * wref + g.b * vr * vr);
    const double vc = vr * ce + kk * ex;
    const double wc = wref + kk * eph + g.b * vr * track_sinc(eph, se) * ey;
    cl = vc - wc * g.T / 2.0;
    cr = vc + wc * g.T / 2.0;
}

// ---- 3. the lane --------------------------------------------------------------------------------------------------------
// K <= 256: a workgroup takes R = 256 / K whole routes (thread = route-in-group * K + k; the last 256 - R * K threads idle);
// K > 256: a route takes wpr = ceil(K / 256) workgroups.  `producer`: false for the threads behind the rollout lanes
struct RolloutLane {
    int b0, lr, k, b;         // the workgroup's first route, the lane's route within the workgroup, its rollout, its route
    bool inside;
    size_t gi;                // flattened (b, k)
    __device__ __forceinline__ RolloutLane(const RolloutArgs &g, bool producer)
    {
        const int tid = threadIdx.x;
        b0 = g.wpr > 1 ? (int)(blockIdx.x / g.wpr) : (int)blockIdx.x * g.R;
        lr = g.wpr > 1 ? 0 : tid / g.K;
        k = g.wpr > 1 ? (int)(blockIdx.x % g.wpr) * kTrackThreads + tid : tid % g.K;
        b = b0 + lr;
        inside = producer && lr < g.R && b < g.B && k < g.K;
        gi = (size_t)b * g.K + k;
    }
};

// rows of route b: its count within [0, cap]
template <class Args>
__device__ __forceinline__ int route_rows(const Args &g, int b)
{
    const long c = g.counts[(size_t)b * g.stride];
    return (int)(c < 0 ? 0 : (c > g.cap ? g.cap : c));
}

// the lane's perturbation record (include/vap.h): (dx, dy), (dphi, gain_left), (gain_right, track_scale), (tau, slot 7)
struct PlantRecord {
    double2 p01, p23, p45, p67;
    __device__ __forceinline__ PlantRecord(const RolloutArgs &g, const RolloutLane &ln)
    {
        const double *p = g.perturb + (g.shared ? (size_t)ln.k : ln.gi) * 8;
        p01 = *(const double2 *)p, p23 = *(const double2 *)(p + 2), p45 = *(const double2 *)(p + 4), p67 = *(const double2 *)(p + 6);
    }
    __device__ __forceinline__ bool valid() const
    {
        return isfinite(p01.x) && isfinite(p01.y) && isfinite(p23.x) && isfinite(p23.y) && isfinite(p45.x) && isfinite(p45.y) &&
               isfinite(p67.x) && isfinite(p67.y) && p23.y > 0.0 && p45.x > 0.0 && p45.y > 0.0 && p67.x >= 0.0;
    }
    // the plant's constants and its state on row 0 of the route
    __device__ __forceinline__ void start(const RolloutArgs &g, const double *row0, TrackPlant &pl) const
    {
        const double tau = p67.x;
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
};

// ---- 4. the row stage ---------------------------------------------------------------------------------------------------
// Every rollout of a route reads the same five columns {v, heading, angular_vel, x, y} of the same row at the same step, so
// the workgroup stages its routes' rows in LDS, 40 B per row, in tiles of kTrackRows / R rows (at most kTrackTileMax): the
// next tile's loads are issued before the current tile is marched (load) and land in the other buffer after it (store), one
// barrier per tile, which is the caller's.  The settle rows (r >= n) are made by the loader (the last pose, v = omega = 0),
// so the march never looks at counts.  Staged as [row][column][route]: lanes of one route read one address (a broadcast),
// lanes of different routes consecutive ones.
constexpr int kTrackRows = 512;        // staged rows per LDS buffer, over all routes of the workgroup
constexpr int kTrackTileMax = 64;      // rows of one route per tile, at most
constexpr int kSplitRows = 8;          // ... and with the clearance split off (SplitLds): two tiles of 256 poses x 24 B are 96 KiB of LDS

// RolloutArgs::tile for R routes per workgroup
inline int stage_tile(int R, bool split)
{
    const int tile = kTrackRows / R < kTrackTileMax ? kTrackRows / R : kTrackTileMax;
    return split && tile > kSplitRows ? kSplitRows : tile;
}

struct RowStage {
    double *buf;              // LDS [2][kTrackRows * 5]
    int *n;                   // LDS [kTrackThreads]: the rows of the workgroup's routes
    int total;                // steps of the longest route of the workgroup
    int b0, tid, items;
    bool producer;
    double lv[2], lh[2], lw[2], lx[2], ly[2];

    // the routes' counts and the first tile; ends behind a barrier
    __device__ __forceinline__ void begin(const RolloutArgs &g, int b0_, bool producer_)
    {
        __shared__ __attribute__((aligned(16))) double s_stage[2 * kTrackRows * 5];
        __shared__ int s_n[kTrackThreads];
        __shared__ int s_total;
        buf = s_stage, n = s_n, b0 = b0_, tid = threadIdx.x, producer = producer_, items = g.R * g.tile;
        if (tid == 0) s_total = 0;
        if (tid < g.R) s_n[tid] = b0 + tid < g.B ? route_rows(g, b0 + tid) : 0;
        __syncthreads();
        if (tid < g.R && s_n[tid] > 0) atomicMax(&s_total, s_n[tid] + g.settle);
        __syncthreads();
        total = s_total;
        if (tiles(g) > 0) {
            load(g, 0);
            store(g, 0);
        }
        __syncthreads();
    }
    __device__ __forceinline__ int tiles(const RolloutArgs &g) const { return (total + g.tile - 1) / g.tile; }
    // item j < R * tile is row j % tile of route j / tile of the tile (consecutive threads on consecutive rows of a route);
    // at most two items per thread
    __device__ __forceinline__ void load(const RolloutArgs &g, int ti)
    {
        const int tile = g.tile;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int j = tid + i * kTrackThreads;
            lv[i] = lh[i] = lw[i] = lx[i] = ly[i] = 0.0;
            if (producer && j < items) {
                const int route = j / tile, r = ti * tile + j % tile, nr = n[route];
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
    }
    __device__ __forceinline__ void store(const RolloutArgs &g, int b)
    {
        const int tile = g.tile, R = g.R;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int j = tid + i * kTrackThreads;
            if (producer && j < items) {
                double *d = buf + (size_t)b * kTrackRows * 5 + (size_t)(j % tile) * 5 * R + j / tile;
                d[0] = lv[i];
                d[R] = lh[i];
                d[2 * R] = lw[i];
                d[3 * R] = lx[i];
                d[4 * R] = ly[i];
            }
        }
    }
    // row t of tile ti for the lane's route lr: {v, heading, angular_vel, x, y} at q[0], q[R] .. q[4 R]
    __device__ __forceinline__ const double *row(const RolloutArgs &g, int ti, int t, int lr) const
    {
        return buf + (size_t)(ti & 1) * kTrackRows * 5 + (lr < g.R ? lr : 0) + (size_t)t * 5 * g.R;
    }
};

// ---- 5. the clearance of the executed rows ------------------------------------------------------------------------------
// A rollout's clearance over its executed rows in row order, by vap_footprint_clearance's rules: a strictly smaller value
// replaces (the first row stays on a tie, a NaN never replaces); rows below the margin are counted and the first is kept.
// A row changes these only if its clearance is below max(best so far, margin), so that is the row's `cap`: once a rollout
// has come near something, the far elements of every later row are culled by the rollout's own minimum, which the
// two-call form, a thread per row, cannot do.  Values below the cap are exact, so the outputs keep their bits.
struct ClearAcc {
    double best = INFINITY;
    int row = -1, el = -1, first = -1, nb = 0;
    // the pose of executed row r is what TrackPlant::write_row stores: heading = -wrap(phi), x, y
    __device__ __forceinline__ void take(const FootScene &s, double margin, const TrackPlant &pl, int r)
    {
        int e;
        const double v = row_clearance_capped(s, -track_wrap(pl.phi), pl.x, pl.y, e, fmax(best, margin));
        fold(v, e, r, margin);
    }
    // row r's clearance v and element e, taken elsewhere
    __device__ __forceinline__ void fold(double v, int e, int r, double margin)
    {
        if (v < margin) {
            nb++;
            if (first < 0) first = r;
        }
        if (v < best) { best = v; row = r; el = e; }
    }
    __device__ __forceinline__ void store(const TrackClear &c, size_t gi) const
    {
        if (c.clearance) c.clearance[gi] = row >= 0 ? best : NAN;
        if (c.clear_rows) {
            int *o = c.clear_rows + gi * 4;
            o[0] = row;
            o[1] = row >= 0 ? el : -1;
            o[2] = first;
            o[3] = nb;
        }
        if (c.part_c) {
            c.part_c[gi] = best;
            c.part_row[gi] = row;
            c.part_el[gi] = el;
        }
    }
};

// The clearance split off the rollout lanes (kTrackSplit).  A workgroup of kSplitThreads: the first kTrackThreads lanes
// march their rollouts a tile of at most kSplitRows rows at a time and put (heading, x, y) of every executed row into LDS,
// [buffer][column][row][lane]; the lanes behind them take the clearance of the tile marched in the iteration before and
// leave (clearance, element) where the pose was; the rollout lanes fold the tile before that in row order.  So a march of
// ntiles tiles takes ntiles + 2 iterations, and one barrier per iteration (the caller's) separates the three.  Results and
// outputs are the lane-per-rollout kernel's, bit for bit: the same row_clearance on the same pose, folded in the same order.
constexpr int kSplitThreads = 1024;    // 4 rollout waves and 12 clearance waves (768 threads kept the march out of scratch and measured slower)
constexpr int kSplitTile = 3 * kSplitRows * kTrackThreads;      // doubles of one pose buffer

struct SplitLds {
    double *pose = nullptr, *cap = nullptr;     // [2][kSplitTile] and [2][kTrackThreads]

    __device__ __forceinline__ void begin()
    {
        __shared__ double s_pose[2 * kSplitTile], s_cap[2 * kTrackThreads];
        pose = s_pose, cap = s_cap;
    }
    // a rollout lane: row t of tile ti
    __device__ __forceinline__ void put(int ti, int t, int lane, double heading, double x, double y) const
    {
        double *pz = pose + (size_t)(ti & 1) * kSplitTile + (size_t)t * kTrackThreads + lane;
        pz[0] = heading;                                     // NaN: no pose, nothing to clear
        pz[kSplitRows * kTrackThreads] = x;
        pz[2 * kSplitRows * kTrackThreads] = y;
    }
    // a clearance lane (number ctid of nc): the rend rows of tile tj, 64 rollouts of one row to a wave.  The cap of a
    // rollout is its minimum as of the fold before the tile was marched: older than the row's own, so no smaller, and still
    // a valid cap
    __device__ __forceinline__ void clear(const TrackClear &c, int tj, int rend, int ctid, int nc) const
    {
        double *pz = pose + (size_t)(tj & 1) * kSplitTile;
        const double *cp = cap + (size_t)(tj & 1) * kTrackThreads;
#pragma unroll 1
        for (int p = ctid; p < rend * kTrackThreads; p += nc) {
            const double hd = pz[p];
            double v = NAN;
            int e = -1;
            if (hd == hd)
                v = row_clearance_capped(c.s, hd, pz[kSplitRows * kTrackThreads + p], pz[2 * kSplitRows * kTrackThreads + p], e,
                                  fmax(cp[p & (kTrackThreads - 1)], c.margin));
            pz[p] = v;
            pz[kSplitRows * kTrackThreads + p] = (double)e;
        }
    }
    // a rollout lane: its rows of tile tj (first row r0) in row order, before the buffer is written again
    __device__ __forceinline__ void fold(ClearAcc &acc, int tj, int r0, int rend, int my_total, int lane, double margin) const
    {
        const double *pz = pose + (size_t)(tj & 1) * kSplitTile + lane;
#pragma unroll 1
        for (int t = 0; t < rend && r0 + t < my_total; t++)
            acc.fold(pz[t * kTrackThreads], (int)pz[(kSplitRows + t) * kTrackThreads], r0 + t, margin);
    }
    // iteration ti of ntiles + 2 over tiles of `tile` rows: a clearance lane clears tile ti - 1; a rollout lane folds tile
    // ti - 2 and leaves its minimum as the cap of tile ti.  True where the lane is to march tile ti now
    __device__ __forceinline__ bool step(const TrackClear &c, ClearAcc &acc, bool producer, int ti, int ntiles, int tile, int wg_total,
                                         int my_total) const
    {
        const int tid = threadIdx.x;
        if (!producer) {
            if (ti >= 1 && ti <= ntiles)
                clear(c, ti - 1, min(tile, wg_total - (ti - 1) * tile), tid - kTrackThreads, (int)blockDim.x - kTrackThreads);
            return false;
        }
        if (ti >= 2) fold(acc, ti - 2, (ti - 2) * tile, min(tile, wg_total - (ti - 2) * tile), my_total, tid, c.margin);
        cap[(size_t)(ti & 1) * kTrackThreads + tid] = acc.best;
        return ti < ntiles;
    }
};

// The clearance of a rollout to the partner's routes (kTrackConflict), by vap_footprint_conflicts' rules for the pairs
// (this rollout's executed rows, partner o), o = 0 .. Bo - 1, side O starting s rows late: at horizon row r the partner is
// at its row clamp(r - s, 0, n_o - 1), and the pair is examined up to T = max(n_a, n_o + s, 1).  The lane forms its packed
// pose with the pack kernel's own function (conf_pose) and reads O's packed rows, so every clearance has the bits the pair
// of calls computes.  Per partner the lane keeps (minimum, first row at it, first row below the margin) in dynamic LDS,
// [o][lane]: rows ascend in a lane, so a strictly smaller value replaces and nothing is tie-broken across lanes.  A row is
// culled against the pair's own threshold as k_conflict_pairs forms it.
struct ConflictLane {
    const double *sfa, *sfo;  // LDS: the footprints' vertex tables
    const int *no_rows;       // LDS [Bo]: the partners' counts
    double *best;             // LDS [Bo][kTrackThreads]
    int *row, *first;
    long s = 0;               // this rollout's shift
    double ax = 0.0, ay = 0.0, ac = 1.0, as = 0.0;      // the packed pose of the last executed row

    // every thread of the workgroup; ends behind a barrier.  (b, k): the lane's rollout, read where `inside`
    __device__ __forceinline__ void begin(const TrackConflict &x, const ConfFoot &fa, const ConfFoot &fo, bool inside, int b, int k)
    {
        extern __shared__ __attribute__((aligned(16))) double s_conflict[];
        __shared__ double s_fa[kFootMaxVerts * 8], s_fo[kFootMaxVerts * 8];
        __shared__ int s_no[kConflictOthersMax];
        const int tid = threadIdx.x, Bo = x.p.o.B;
        sfa = s_fa, sfo = s_fo, no_rows = s_no;
        best = s_conflict + tid;
        row = (int *)(s_conflict + (size_t)Bo * kTrackThreads) + tid;
        first = row + (size_t)Bo * kTrackThreads;
        if (tid < kFootMaxVerts * 8) {
            s_fa[tid] = fa.v[tid];
            s_fo[tid] = fo.v[tid];
        }
        if (tid < Bo) s_no[tid] = (int)conf_count(x.p.o, tid);
#pragma unroll 1
        for (int o = 0; o < Bo; o++) {
            best[o * kTrackThreads] = INFINITY;
            row[o * kTrackThreads] = -1;
            first[o * kTrackThreads] = -1;
        }
        if (inside) {
            s = x.shift;
            if (x.route_shift) s += clampl(x.route_shift[b], -kConflictShiftMax, kConflictShiftMax);
            if (x.rollout_shift) s += clampl(x.rollout_shift[k], -kConflictShiftMax, kConflictShiftMax);
        }
        __syncthreads();
    }
    // horizon row r of the pair with partner o, the lane's own pose being (ax, ay, ac, as)
    __device__ __forceinline__ void pair(const TrackConflict &x, int o, long r)
    {
        const long n_o = no_rows[o];
        if (n_o <= 0) return;                               // an invalid pair
        const double *q = x.p.pack_o + ((size_t)o * (size_t)x.p.Tpo + (size_t)clampl(r - s, 0, n_o - 1)) * 4;
        const double2 o01 = *(const double2 *)q;
        const double bo = best[o * kTrackThreads];
        const int fo = first[o * kTrackThreads];
        if (x.p.cull && row_culled(x.p, x.radii, fo >= 0 ? bo : fmax(bo, x.margin), ax, ay, o01.x, o01.y)) return;
        const double2 o23 = *(const double2 *)(q + 2);
        const double c = pair_clearance(sfa, x.na, sfo, x.no, ax, ay, ac, as, o01.x, o01.y, o23.x, o23.y);
        if (c == c) {                                       // a NaN clearance takes part in nothing
            if (c < x.margin && fo < 0) first[o * kTrackThreads] = (int)r;
            if (c < bo) {
                best[o * kTrackThreads] = c;
                row[o * kTrackThreads] = (int)r;
            }
        }
    }
    // executed row r: the pose is what TrackPlant::write_row stores, heading = -wrap(phi), x, y
    __device__ __forceinline__ void take(const TrackConflict &x, const TrackPlant &pl, int r)
    {
        conf_pose(-track_wrap(pl.phi), pl.x, pl.y, x.fcx, x.fcy, ax, ay, ac, as);
#pragma unroll 1
        for (int o = 0; o < x.p.o.B; o++) pair(x, o, r);
    }
    // The instants after the rollout's last executed row n_a - 1, at whose pose it stays parked, per partner up to n_o + s.
    // While the partner has not started either (rows in [n_a, s)) nothing moves: the stretch's first row stands for it.
    // So the loop takes at most n_o + 1 rows, whatever s is.  No barriers.
    __device__ __forceinline__ void tail(const TrackConflict &x, int n_a)
    {
        if (n_a <= 0) return;
#pragma unroll 1
        for (int o = 0; o < x.p.o.B; o++) {
            const long T = (long)no_rows[o] + s;
            long r = n_a;
            if (no_rows[o] <= 0 || r >= T) continue;
            if (s > r) {
                pair(x, o, r);
                r = s;
            }
#pragma unroll 1
            for (; r < T; r++) pair(x, o, r);
        }
    }
    // the walk over the partners in ascending o (a strictly smaller minimum replaces: the smallest o stays), the outputs of
    // rollout gi, and (minimum, its row, its partner) for the route's summary
    __device__ __forceinline__ void finish(const TrackConflict &x, size_t gi, double &cmin, int &crow, int &cother) const
    {
        const int Bo = x.p.o.B;
        double m = INFINITY;
        int other = -1, mrow = -1, ncon = 0, f0 = -1;
#pragma unroll 1
        for (int o = 0; o < Bo; o++) {
            const double bo = best[o * kTrackThreads];
            const int ro = row[o * kTrackThreads], fo = first[o * kTrackThreads];
            if (x.pair_c) x.pair_c[gi * Bo + o] = ro >= 0 ? bo : NAN;
            if (x.pair_rows) {
                x.pair_rows[(gi * Bo + o) * 2] = ro;
                x.pair_rows[(gi * Bo + o) * 2 + 1] = fo;
            }
            if (ro < 0) continue;
            if (bo < m) { m = bo; other = o; mrow = ro; }
            ncon += bo < x.margin ? 1 : 0;
            if (fo >= 0 && (f0 < 0 || fo < f0)) f0 = fo;
        }
        if (x.conflict) x.conflict[gi] = other >= 0 ? m : NAN;
        if (x.conflict_rows) {
            int *q = x.conflict_rows + gi * 4;
            q[0] = other;
            q[1] = mrow;
            q[2] = ncon;
            q[3] = f0;
        }
        if (x.part_c) {
            x.part_c[gi] = m;
            x.part_row[gi] = mrow;
            x.part_o[gi] = other;
        }
        cmin = m, crow = mrow, cother = other;
    }
};

// ---- 6. the outputs -----------------------------------------------------------------------------------------------------
// what every follower writes per rollout beside its own statistics: the executed rows' count and, for K > 256, the
// summary's partials
template <class Args>
__device__ __forceinline__ void rollout_outputs(const Args &g, size_t gi, int my_total, double maxe, int mrow)
{
    if (g.exec_counts) {
        g.exec_counts[gi * 2] = my_total;
        g.exec_counts[gi * 2 + 1] = 0;
    }
    if (g.part_e) {
        g.part_e[gi] = maxe;
        g.part_row[gi] = mrow;
    }
}

// A route's rollouts in ascending k: worst (a strictly larger error replaces: the smallest k stays), running sum, count
// above the tolerance.  `Args` carries the per-route output pointers worst, mean, worst_rollout, worst_row, n_exceeding.
// Every summary takes (value, row, a third column or nothing, k, limit) and stores itself for route b.
struct TrackSummary {
    double worst = -INFINITY, sum = 0.0;
    int k = -1, row = -1, cnt = 0, nex = 0;
    __device__ void take(double e, int r, int, int kk, double tol)
    {
        if (r < 0) return;
        if (e > worst) { worst = e; k = kk; row = r; }
        sum += e;
        cnt++;
        nex += e > tol ? 1 : 0;
    }
    template <class Args>
    __device__ void store(const Args &g, int b) const
    {
        if (g.worst) g.worst[b] = cnt ? worst : NAN;
        if (g.mean) g.mean[b] = cnt ? sum / (double)cnt : NAN;
        if (g.worst_rollout) g.worst_rollout[b] = k;
        if (g.worst_row) g.worst_row[b] = row;
        if (g.n_exceeding) g.n_exceeding[b] = nex;
    }
};

// the smallest clearance (a strictly smaller one replaces: the smallest k stays), the running sum, the rollouts below the
// margin and the valid ones (min row >= 0)
struct ClearSummary {
    double worst = INFINITY, sum = 0.0;
    int k = -1, row = -1, el = -1, cnt = 0, ncol = 0;
    __device__ void take(double c, int r, int e, int kk, double margin)
    {
        if (r < 0) return;
        if (c < worst) { worst = c; k = kk; row = r; el = e; }
        sum += c;
        cnt++;
        ncol += c < margin ? 1 : 0;
    }
    __device__ void store(const TrackClear &c, int b) const
    {
        if (c.worst) c.worst[b] = cnt ? worst : NAN;
        if (c.mean) c.mean[b] = cnt ? sum / (double)cnt : NAN;
        if (c.worst_rollout) c.worst_rollout[b] = k;
        if (c.worst_row) c.worst_row[b] = row;
        if (c.worst_element) c.worst_element[b] = k >= 0 ? el : -1;
        if (c.n_colliding) c.n_colliding[b] = ncol;
        if (c.n_valid) c.n_valid[b] = cnt;
    }
};

// vap_rollout_conflicts' route summary: ClearSummary's walk, the third column being the partner at the minimum
struct ConflictSummary : ClearSummary {
    __device__ void store(const TrackConflict &x, int b) const
    {
        if (x.worst) x.worst[b] = cnt ? worst : NAN;
        if (x.mean) x.mean[b] = cnt ? sum / (double)cnt : NAN;
        if (x.worst_rollout) x.worst_rollout[b] = k;
        if (x.worst_other) x.worst_other[b] = k >= 0 ? el : -1;
        if (x.worst_row) x.worst_row[b] = row;
        if (x.n_conflicting) x.n_conflicting[b] = ncol;
        if (x.n_valid) x.n_valid[b] = cnt;
    }
};

// the K rollouts of a route in ascending k from three columns (aux may be NULL), in LDS or in context scratch
template <class Summary>
__device__ __forceinline__ Summary route_walk(const double *v, const int *r, const int *aux, int K, double lim)
{
    Summary s;
#pragma unroll 1
    for (int kk = 0; kk < K; kk++) s.take(v[kk], r[kk], aux ? aux[kk] : 0, kk, lim);
    return s;
}

// K <= 256: the first lane of each route walks its K rollouts in the workgroup's columns, [thread], behind a barrier
template <class Summary, class Out>
__device__ __forceinline__ void route_summary(const Out &out, const RolloutLane &ln, int K, const double *v, const int *r, const int *aux, double lim)
{
    const int tid = threadIdx.x;
    if (ln.inside && ln.k == 0) route_walk<Summary>(v + tid, r + tid, aux ? aux + tid : nullptr, K, lim).store(out, ln.b);
}

// K > 256: the same walk over the partials [B][K] in context scratch, a lane per route
template <class Summary, class Out>
__global__ __launch_bounds__(64) void k_route_reduce(Out out, int B, int K, const double *v, const int *r, const int *aux, double lim)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const size_t p = (size_t)b * K;
    route_walk<Summary>(v + p, r + p, aux ? aux + p : nullptr, K, lim).store(out, b);
}

}  // namespace vap
