// vap_track_common.h — what the follower rollouts share (vap_tracking.hip: RAMSETE; vap_pursuit.hip: pure pursuit):
// the angle wrap, sinc, the plant, the fixed-order summary of a route's rollouts and the kernels' arguments; and what
// vap_rollout_clearance.hip adds to both: the scene clearance of the executed rows, taken where the row would be written.
#pragma once
#include <cmath>

#include "vap_footprint.h"

namespace vap {

constexpr int kTrackThreads = 256;
constexpr double kPi = 3.14159265358979323846;

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

// a route's rollouts in ascending k: worst (a strictly larger error replaces: the smallest k stays), running sum, count
// above the tolerance.  `Args` carries the per-route output pointers worst, mean, worst_rollout, worst_row, n_exceeding.
struct TrackSummary {
    double worst = -INFINITY, sum = 0.0;
    int k = -1, row = -1, cnt = 0, nex = 0;
    __device__ void take(double e, int r, int kk, double tol)
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

// What a rollout kernel does with the executed row r (include/vap.h, step 3): nothing, write it, take its scene clearance
// while the pose is in registers, or hand the pose to further lanes of the workgroup that take it (vap_rollout_clearance).
enum { kTrackPlain = 0, kTrackExec = 1, kTrackClear = 2, kTrackSplit = 3 };

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

// ---- the clearance split off the rollout lanes (kTrackSplit) ----------------------------------------------------------
// A workgroup of kSplitThreads: the first kTrackThreads lanes march their rollouts a tile of kSplitRows rows at a time and
// put (heading, x, y) of every executed row into LDS, [buffer][column][row][lane]; the lanes behind them take the clearance
// of the tile marched in the iteration before and leave (clearance, element) where the pose was; the rollout lanes fold
// the tile before that in row order.  One barrier per iteration separates the three.  Results and outputs are the
// lane-per-rollout kernel's, bit for bit: the same row_clearance on the same pose, folded in the same order.
constexpr int kSplitRows = 8;          // rows per tile: two tiles of 256 poses x 24 B are 96 KiB of LDS
constexpr int kSplitThreads = 1024;    // 4 rollout waves and 12 clearance waves (768 threads kept the march out of scratch and measured slower)
constexpr int kSplitTile = 3 * kSplitRows * kTrackThreads;      // doubles of one pose buffer

template <int N, int TAG>
__device__ __forceinline__ double *lds_doubles()
{
    __shared__ double a[N];
    return a;
}

// a rollout lane: row t of the tile in buffer `buf`
__device__ __forceinline__ void split_put(double *s_pose, int buf, int t, int lane, double heading, double x, double y)
{
    double *pz = s_pose + (size_t)buf * kSplitTile + (size_t)t * kTrackThreads + lane;
    pz[0] = heading;                                     // NaN: no pose, nothing to clear
    pz[kSplitRows * kTrackThreads] = x;
    pz[2 * kSplitRows * kTrackThreads] = y;
}

// a clearance lane (number ctid of nc): tile tj, 64 rollouts of one row to a wave.  The cap of a rollout is its minimum as
// of the fold before the tile was marched: older than the row's own, so no smaller, and still a valid cap
__device__ __forceinline__ void split_clear(const TrackClear &c, double *s_pose, const double *s_cap, int tj, int rend, int ctid, int nc)
{
    double *pz = s_pose + (size_t)(tj & 1) * kSplitTile;
    const double *cap = s_cap + (size_t)(tj & 1) * kTrackThreads;
#pragma unroll 1
    for (int p = ctid; p < rend * kTrackThreads; p += nc) {
        const double hd = pz[p];
        double v = NAN;
        int e = -1;
        if (hd == hd)
            v = row_clearance_capped(c.s, hd, pz[kSplitRows * kTrackThreads + p], pz[2 * kSplitRows * kTrackThreads + p], e,
                              fmax(cap[p & (kTrackThreads - 1)], c.margin));
        pz[p] = v;
        pz[kSplitRows * kTrackThreads + p] = (double)e;
    }
}

// a rollout lane: its rows of tile tj (first row r0) in row order, before the buffer is written again
__device__ __forceinline__ void split_fold(ClearAcc &acc, const double *s_pose, int tj, int r0, int rend, int my_total, int lane, double margin)
{
    const double *pz = s_pose + (size_t)(tj & 1) * kSplitTile + lane;
#pragma unroll 1
    for (int t = 0; t < rend && r0 + t < my_total; t++)
        acc.fold(pz[t * kTrackThreads], (int)pz[(kSplitRows + t) * kTrackThreads], r0 + t, margin);
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

// a route's rollouts in ascending k: the smallest clearance (a strictly smaller one replaces: the smallest k stays), the
// running sum, the rollouts below the margin and the valid ones (min row >= 0)
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

struct TrackArgs {
    const double *rows;       // [B][cap][8]
    const int *counts;
    long cap;
    int stride, B, K, shared;
    const double *perturb;    // [B][K][8] or [K][8]
    double T, b, two_zeta, wmax, tol, dt, h;
    int nsub, settle;
    double *stats;            // [B][K][6]
    int *stat_rows;           // [B][K][2]
    double *worst, *mean;     // [B]
    int *worst_rollout, *worst_row, *n_exceeding;
    long cap_exec;
    double *exec_rows;        // [B*K][cap_exec][8]
    int *exec_counts;         // [B*K][2]
    double *part_e;           // K > 256: [B][K] max e_pos (row < 0: takes no part)
    int *part_row;
    int R, tile, wpr;         // routes per workgroup, rows per tile, workgroups per route
};


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
    int *part_row, *part_arr;
    int R, wpr;               // routes per workgroup, workgroups per route
};


// The two followers' calls in two halves, so that vap_rollout_clearance runs the same code: *_setup checks the host
// arguments (no device call) and fills the kernel arguments; *_launch sizes the grid and the context scratch and enqueues
// the kernels, with `clear` the rollouts take the clearance of their executed rows (no executed rows are written then).
int tracking_setup(int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride, double time_step,
                   const vap_follower *f, int K, int shared_perturb, const double *d_perturb, double *d_stats, int *d_stat_rows,
                   double *d_worst, double *d_mean, int *d_worst_rollout, int *d_worst_row, int *d_n_exceeding, long cap_exec,
                   double *d_exec_rows, int *d_exec_counts, TrackArgs &g);
int tracking_launch(vap_ctx *ctx, TrackArgs &g, TrackClear *clear);
int pursuit_setup(int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride, double time_step,
                  const vap_pursuit *f, int K, int shared_perturb, const double *d_perturb, double *d_stats, int *d_stat_rows,
                  double *d_worst, double *d_mean, int *d_worst_rollout, int *d_worst_row, int *d_n_exceeding, int *d_n_unfinished,
                  int *d_route_status, long cap_exec, double *d_exec_rows, int *d_exec_counts, PursuitArgs &g);
int pursuit_launch(vap_ctx *ctx, PursuitArgs &g, TrackClear *clear);
// K > 256 with a clearance summary: the bytes of the clearance partials, and their place at `base` (8-byte aligned) in
// ctx->track_part, behind the follower's own scratch
inline size_t clear_part_bytes(const TrackClear *c, int B, int K)
{
    return c && c->summary() && K > kTrackThreads ? (size_t)B * (size_t)K * (sizeof(double) + 2 * sizeof(int)) : 0;
}
inline void clear_part_place(TrackClear *c, void *base, int B, int K)
{
    const size_t np = (size_t)B * (size_t)K;
    c->part_c = (double *)base;
    c->part_row = (int *)(c->part_c + np);
    c->part_el = c->part_row + np;
}

}  // namespace vap
