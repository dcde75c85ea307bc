// vap_tables.hip — K1 fit, K2 arc-length table, the distance grid and the one-value accessors (gfx950 / CDNA4).
// ------------------------------------------------------------------------------------------------
// K1: fit.  One workgroup per path.  QHS:30-138, 149-219, 719-736; SM:65-77 tangent overrides.
// LDS (dynamic): pts[W][2], dist[G], fd[W][2], sd[W][2]  (fp64)
// ------------------------------------------------------------------------------------------------
#include "vap_device.h"
#include "vap_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace vap {

// ex (optional, QuinticHermiteSpline's own call surface): caller-supplied derivatives — used only when BOTH arrays are
// given (QHS:52-68: with one of them missing _compute_derivatives overwrites both) — and the starting / ending
// tangent of a split spline (QHS:129-132, 543-590; quirk Q3: both patch the LAST segment).
struct FitExtras {
    const double *first = nullptr, *second = nullptr;    // [B][W][2]
    const double *start_tan = nullptr, *end_tan = nullptr;   // [B][2], NaN = not set
    double *out_first = nullptr, *out_second = nullptr;      // [B][W][2]: the derivatives the segments were built from
};

// The fit of path b by the calling workgroup (sh: 7*W doubles of LDS).  Ends with a workgroup barrier; the segments,
// coefficient blocks, meta[0] and flags of the path are then written (visible to this workgroup after a fence).
template <typename IT>
__device__ __forceinline__ void fit_path(int b, int W, const IT *__restrict__ waypoints, const double *__restrict__ tan_in,
                                         const double *__restrict__ tan_out, const FitExtras &ex, double *__restrict__ segments,
                                         double *__restrict__ power, double *__restrict__ seglen, double *__restrict__ meta,
                                         uint32_t *__restrict__ flags, double *sh, int tid = threadIdx.x, int nt = blockDim.x,
                                         uint32_t *flag_word = nullptr)
{
    // (tid, nt: the threads that work on THIS path — the whole workgroup, or a sub-group of it when k_fit_many packs
    // several short paths into one; every __syncthreads below is reached by all threads of the workgroup either way)
    const int G = W - 1;
    double *pts = sh;             // 2W
    double *dist = pts + 2 * W;   // G (W slots)
    double *fd = dist + W;        // 2W
    double *sd = fd + 2 * W;      // 2W
    __shared__ uint32_t s_flag_one;
    uint32_t &s_flag = flag_word ? *flag_word : s_flag_one;
    if (tid == 0) s_flag = 0;
    const IT *wp = waypoints + (size_t)b * W * 2;
    for (int i = tid; i < 2 * W; i += nt) pts[i] = (double)wp[i];
    __syncthreads();
    for (int i = tid; i < G; i += nt) {
        const double dx = pts[2 * (i + 1)] - pts[2 * i], dy = pts[2 * (i + 1) + 1] - pts[2 * i + 1];
        const double d = sqrt(dx * dx + dy * dy);  // np.linalg.norm(diffs, axis=1), QHS:160
        dist[i] = d;
        if (!(d > 0.0) || !isfinite(d)) atomicOr(&s_flag, VAP_FLAG_DEGENERATE_BIT);
    }
    __syncthreads();
    if (tid == 0) {
        // QHS:719-736: only parameters[-1] is ever read; sequential np.cumsum order
        double cum = 0.0;
        for (int i = 0; i < G; i++) cum += dist[i];
        const double t_max = (cum == 0.0) ? (double)G : cum * (double)G / cum;
        meta[(size_t)b * kMetaStride + 0] = t_max;
    }
    const bool have_d = ex.first && ex.second;
    const bool has_st = ex.start_tan && !isnan(ex.start_tan[(size_t)b * 2]);
    const bool has_en = ex.end_tan && !isnan(ex.end_tan[(size_t)b * 2]);
    // QHS:163-195 first derivatives
    for (int i = tid; i < W; i += nt) {
        double fx, fy;
        if (have_d) {
            fx = ex.first[((size_t)b * W + i) * 2];
            fy = ex.first[((size_t)b * W + i) * 2 + 1];
        } else if (i == 0) {
            // QHS:170-172: a 2-point spline with an ending tangent keeps the chord un-normalised
            const double d = (W == 2 && has_en) ? 1.0 : dist[0];
            fx = (pts[2] - pts[0]) / d;
            fy = (pts[3] - pts[1]) / d;
        } else if (i == W - 1) {
            const double d = (W == 2 && has_st) ? 1.0 : dist[G - 1];   // QHS:181-182
            fx = (pts[2 * i] - pts[2 * (i - 1)]) / d;
            fy = (pts[2 * i + 1] - pts[2 * (i - 1) + 1]) / d;
        } else {
            const double px = (pts[2 * i] - pts[2 * (i - 1)]) / dist[i - 1];
            const double py = (pts[2 * i + 1] - pts[2 * (i - 1) + 1]) / dist[i - 1];
            const double nx = (pts[2 * (i + 1)] - pts[2 * i]) / dist[i];
            const double ny = (pts[2 * (i + 1) + 1] - pts[2 * i + 1]) / dist[i];
            fx = (px + nx) / 2;
            fy = (py + ny) / 2;
        }
        fd[2 * i] = fx;
        fd[2 * i + 1] = fy;
    }
    __syncthreads();
    // QHS:197-219 second derivatives (zero at both ends)
    for (int i = tid; i < W; i += nt) {
        double sx = 0.0, sy = 0.0;
        if (have_d) {
            sx = ex.second[((size_t)b * W + i) * 2];
            sy = ex.second[((size_t)b * W + i) * 2 + 1];
        } else if (i > 0 && i < W - 1) {
            const double avg = (dist[i - 1] + dist[i]) / 2;
            sx = (fd[2 * (i + 1)] - fd[2 * (i - 1)]) / (avg * 0.5);
            sy = (fd[2 * (i + 1) + 1] - fd[2 * (i - 1) + 1]) / (avg * 0.5);
        }
        sd[2 * i] = sx;
        sd[2 * i + 1] = sy;
    }
    __syncthreads();
    if (ex.out_first && ex.out_second) {
        // the attributes the reference leaves behind: estimates (or the caller's arrays), with the tangent setters'
        // writes to first_derivatives[0] / [-1] (QHS:557, 582)
        for (int i = tid; i < 2 * W; i += nt) {
            double f = fd[i];
            if (has_st && i < 2) f = ex.start_tan[(size_t)b * 2 + i];
            if (has_en && i >= 2 * (W - 1)) f = ex.end_tan[(size_t)b * 2 + i - 2 * (W - 1)];   // (applied second, as QHS:131-132)
            ex.out_first[(size_t)b * W * 2 + i] = f;
            ex.out_second[(size_t)b * W * 2 + i] = sd[i];
        }
    }
    // QHS:76-127 segment assembly
    for (int i = tid; i < G; i += nt) {
        const double L = dist[i];  // == np.linalg.norm(p1 - p0)
        double r[12];
        r[0] = pts[2 * i];       r[1] = pts[2 * i + 1];
        r[2] = pts[2 * (i + 1)]; r[3] = pts[2 * (i + 1) + 1];
        if (L > 0) {
            const double L2 = L * L;
            r[4] = fd[2 * i] * L;          r[5] = fd[2 * i + 1] * L;
            r[6] = fd[2 * (i + 1)] * L;    r[7] = fd[2 * (i + 1) + 1] * L;
            r[8] = sd[2 * i] * L2;         r[9] = sd[2 * i + 1] * L2;
            r[10] = sd[2 * (i + 1)] * L2;  r[11] = sd[2 * (i + 1) + 1] * L2;
            if (tan_out) {
                const double *t = tan_out + ((size_t)b * W + i) * 2;
                if (!isnan(t[0])) { r[4] = t[0]; r[5] = t[1]; }
            }
            if (tan_in) {
                const double *t = tan_in + ((size_t)b * W + i + 1) * 2;
                if (!isnan(t[0])) { r[6] = t[0]; r[7] = t[1]; }
            }
        } else {
            r[4] = fd[2 * i];          r[5] = fd[2 * i + 1];
            r[6] = fd[2 * (i + 1)];    r[7] = fd[2 * (i + 1) + 1];
            r[8] = sd[2 * i];          r[9] = sd[2 * i + 1];
            r[10] = sd[2 * (i + 1)];   r[11] = sd[2 * (i + 1) + 1];
        }
        if (i == G - 1) {   // QHS:129-132 -> 543-590: both setters write into segments[-1] (quirk Q3)
            if (has_st) { r[4] = ex.start_tan[(size_t)b * 2]; r[5] = ex.start_tan[(size_t)b * 2 + 1]; }
            if (has_en) { r[6] = ex.end_tan[(size_t)b * 2]; r[7] = ex.end_tan[(size_t)b * 2 + 1]; }
        }
        double *sg = segments + ((size_t)b * G + i) * 12;
#pragma unroll
        for (int k = 0; k < 12; k++) sg[k] = r[k];
        if (power) make_coef_block(r, power + ((size_t)b * G + i) * kCoefDoubles);
        if (seglen) seglen[(size_t)b * G + i] = L;
    }
    __syncthreads();
    if (tid == 0 && flags) flags[b] = s_flag;
}

template <typename IT>
__global__ __launch_bounds__(256) void k_fit(int W, const IT *__restrict__ waypoints,
                                             const double *__restrict__ tan_in,
                                             const double *__restrict__ tan_out, FitExtras ex,
                                             double *__restrict__ segments, double *__restrict__ power,
                                             double *__restrict__ seglen, double *__restrict__ meta,
                                             uint32_t *__restrict__ flags)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];
    fit_path<IT>(blockIdx.x, W, waypoints, tan_in, tan_out, ex, segments, power, seglen, meta, flags, sh);
}

// K1 for very many short paths (config 5: 131 072 paths of 8 waypoints): k_fit gives a path a workgroup of 64 threads of
// which W work; here a workgroup of 256 threads takes 256 / L paths, L = the power of two >= W lanes each — the same
// fit_path, the same rows.
template <typename IT>
__global__ __launch_bounds__(256) void k_fit_many(int B, int W, int L, const IT *__restrict__ waypoints, double *__restrict__ segments,
                                                  double *__restrict__ power, double *__restrict__ meta, uint32_t *__restrict__ flags)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];   // (256 / L) paths x 7W doubles
    __shared__ uint32_t s_flags[64];
    const int per = 256 / L, sub = threadIdx.x / L, lane = threadIdx.x % L;
    int b = blockIdx.x * per + sub;
    // (paths past the batch: the last path once more — same values into the same places, so every thread reaches the barriers)
    b = b < B ? b : B - 1;
    fit_path<IT>(b, W, waypoints, nullptr, nullptr, FitExtras(), segments, power, nullptr, meta, flags, sh + (size_t)sub * 7 * W, lane, L,
                 &s_flags[sub]);
}

// ------------------------------------------------------------------------------------------------
// Grid definition: one thread per path.  MPG:112-122 sample count, or this build's fixed-S grid.
// ------------------------------------------------------------------------------------------------
__global__ void k_grid(int B, int W, int S, double dd_in, double *__restrict__ meta, double *__restrict__ aux,
                       double *__restrict__ runs, uint32_t *__restrict__ flags)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    grid_define(b, W, S, dd_in, meta[(size_t)b * kMetaStride + 1], meta[(size_t)b * kMetaStride + 0], meta, aux, runs, flags);
}

// ------------------------------------------------------------------------------------------------
// K2: arc-length lookup table.  One workgroup per path.  SM:426-475.
// 1000 uniform-parameter samples of |P'(t)| (reference basis, reference order), trapezoid, and a
// SEQUENTIAL cumulative sum (np.cumsum order) so the table is bit-identical to the reference's.
// ------------------------------------------------------------------------------------------------
// Routes cut into several splines (rt.sptab set): grid = (routes, spline slots); the workgroup builds the partial
// (un-offset) table of one spline, SM:436-454, and k_route_offsets (vap_routes_batch.hip) does the rest.
constexpr int kLutPad = (kLutN + 31) / 32 * 32;
template <bool SEG_LDS>
__device__ __forceinline__ void lut_path(int W, const double *__restrict__ segments, double *__restrict__ lut,
                                         double *__restrict__ slopes, double *__restrict__ meta, uint32_t *__restrict__ flags,
                                         const GridArgs &grid, const RouteTables &rt, long long *__restrict__ stats, double *s_seg,
                                         double *cum)
{
    const long long tl0 = stats ? __builtin_amdgcn_s_memtime() : 0;
    constexpr int kPad = kLutPad;   // the sequential sum walks whole groups of 32
    // cum (LDS, kLutPad doubles, 16-byte aligned): magnitudes, then (in place) trapezoid increments, then cumulative distances
    double *mag = cum;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    int G = W - 1;
    double t_max;
    const double *seg = segments + (size_t)b * (W - 1) * 12;
    size_t row = (size_t)b;                 // table row: the path, or (route, spline slot)
    if (rt.sptab) {
        const int sl = blockIdx.y, n = rt.nspl[b];
        if (sl >= n) return;
        const double *sp = rt.sptab + ((size_t)b * rt.NS + sl) * kSplineStride;
        const int first = (int)sp[3], last = sl + 1 < n ? (int)sp[kSplineStride + 3] : W - 1;
        G = last - first;
        t_max = sp[0];
        seg += (size_t)first * 12;
        row = (size_t)b * rt.NS + sl;
    } else {
        t_max = meta[(size_t)b * kMetaStride + 0];
    }
    if constexpr (SEG_LDS) {
        lds_fill<4>(s_seg, seg, G * 12, tid, nt);
        __syncthreads();
        seg = s_seg;
    }
    for (int j = tid; j < kLutN; j += nt) {
        const double t = linspace_at(t_max, kLutN, j);
        double lt;
        int idx;
        normalize_parameter(t, t_max, G, lt, idx);
        double dx, dy;
        hermite_d1_ref(seg + (size_t)idx * 12, lt, dx, dy);
        mag[j] = sqrt(dx * dx + dy * dy);  // np.linalg.norm(derivatives, axis=1), SM:448
    }
    __syncthreads();
    const long long tl1 = stats ? __builtin_amdgcn_s_memtime() : 0;
    // trapezoid increments in parallel (SM:452-454: (m[j-1] + m[j]) * 0.5 * dt, that association) ...
    const double dt = linspace_at(t_max, kLutN, 1) - linspace_at(t_max, kLutN, 0);  // SM:444
    {
        constexpr int kPer = kPad / 128 + 1;   // increments per thread for the smallest launch (128 threads)
        double inc[kPer];
#pragma unroll
        for (int it = 0; it < kPer; it++) {
            const int j = tid + it * nt;
            inc[it] = (j > 0 && j < kLutN) ? (mag[j - 1] + mag[j]) * 0.5 * dt : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kPer; it++) {
            const int j = tid + it * nt;
            if (j < kPad) cum[j] = inc[it];
        }
    }
    __syncthreads();
    // ... and np.cumsum's strictly left-to-right sum.  Lane 0 walks the whole chain but keeps only the
    // running sum at every 32nd element (no stores on the chain); then lane g replays group g from its
    // exact starting sum — the same adds in the same order, so every prefix is bit-identical to the
    // one-lane result — and stores it.
    __shared__ double s_start[kPad / 32];
    __shared__ double s_total;
    if (tid == 0) {
        double acc = 0.0;   // cum[0] = 0: the first add is the exact 0 + 0 of partial_distances[0]
        // (+ current_dist of SM:457 is + 0.0 for a single spline: a no-op on these non-negative sums)
        const double2 *cum2 = reinterpret_cast<const double2 *>(cum);
#pragma unroll 1
        for (int g0 = 0; g0 < kPad / 32; g0++) {
            s_start[g0] = acc;
            double2 v[16];
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = cum2[g0 * 16 + k];
#pragma unroll
            for (int k = 0; k < 16; k++) { acc += v[k].x; acc += v[k].y; }
        }
        if (!rt.sptab) meta[(size_t)b * kMetaStride + 1] = acc;   // elements past kLutN-1 are zero increments
        s_total = acc;
        if (flags && !(acc > 0.0 && isfinite(acc))) atomicOr(&flags[b], VAP_FLAG_DEGENERATE_BIT);
    }
    __syncthreads();
    // the fused call knows the grid spacing already: the last thread (a wave with nothing to do during the
    // replay below) defines the path's distance grid, which would otherwise be a launch of its own
    if (grid.aux && !rt.sptab && tid == nt - 1) grid_define(b, W, grid.S, grid.dd, s_total, t_max, meta, grid.aux, grid.runs, flags);
    if (tid < kPad / 32) {
        double acc = s_start[tid];
        double2 *cum2 = reinterpret_cast<double2 *>(cum) + tid * 16;
        double2 v[16];
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = cum2[k];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            acc += v[k].x;
            v[k].x = acc;
            acc += v[k].y;
            v[k].y = acc;
        }
#pragma unroll
        for (int k = 0; k < 16; k++) cum2[k] = v[k];
    }
    __syncthreads();
    const long long tl2 = stats ? __builtin_amdgcn_s_memtime() : 0;
    const double lstep = t_max / (double)(kLutN - 1);
    for (int j = tid; j < kLutN; j += nt) {
        lut[row * kLutN + j] = cum[j];
        if (slopes) {
            // (t1 - t0)/(d1 - d0) of SM:311-317 for the interval ending at entry j
            double w = 0.0;
            if (j > 0) {
                const double t0 = (double)(j - 1) * lstep, t1 = (j == kLutN - 1) ? t_max : (double)j * lstep;
                w = div_inrange(t1 - t0, cum[j] - cum[j - 1]);
            }
            slopes[row * kLutN + j] = w;
        }
    }
    if (stats && tid == 0) {
        stats[(size_t)b * 4 + 0] = tl1 - tl0;
        stats[(size_t)b * 4 + 1] = tl2 - tl1;
        stats[(size_t)b * 4 + 2] = __builtin_amdgcn_s_memtime() - tl2;
    }
}

template <bool SEG_LDS>
__global__ __launch_bounds__(256) void k_lut(int W, const double *__restrict__ segments,
                                             double *__restrict__ lut, double *__restrict__ slopes,
                                             double *__restrict__ meta, uint32_t *__restrict__ flags,
                                             GridArgs grid, RouteTables rt, long long *__restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) double s_seg[];   // G * 12 when SEG_LDS
    __shared__ __attribute__((aligned(16))) double cum[kLutPad];
    lut_path<SEG_LDS>(W, segments, lut, slopes, meta, flags, grid, rt, stats, s_seg, cum);
}

// K1 + K2 in one launch for the fused call on plain paths (vap_profile_batch): the workgroup that fits a path builds its
// table right away — one launch and its ramp less per step (24 + 57 us as two kernels at config 3).  The same two
// bodies: same segments, same table.  Sized so that a CU holds sixteen of these workgroups at once — config 3's 4096
// paths are then ONE round over the 256 CUs, not a full one and a third: at most 64 registers, and one LDS array for both
// phases (the fit's arrays, then the table: max(1024, 7 W) doubles), the segment rows read back through L1.
template <typename IT>
__global__ __launch_bounds__(128, 8) void k_fit_lut(int W, const IT *__restrict__ waypoints, double *__restrict__ segments,
                                                    double *__restrict__ power, double *__restrict__ lut,
                                                    double *__restrict__ meta, uint32_t *__restrict__ flags, GridArgs grid,
                                                    long long *__restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) double sh[];     // max(kLutPad, 7 * W) doubles
    const long long t0 = stats ? __builtin_amdgcn_s_memtime() : 0;
    fit_path<IT>(blockIdx.x, W, waypoints, nullptr, nullptr, FitExtras(), segments, power, nullptr, meta, flags, sh);
    __threadfence_block();      // the segments and meta[0] this workgroup wrote, read back below
    __syncthreads();
    if (stats && threadIdx.x == 0) stats[(size_t)blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memtime() - t0;
    lut_path<false>(W, segments, lut, nullptr, meta, flags, grid, RouteTables(), stats, nullptr, sh);
}

// K2 for very many short paths (config 5: 131 072 paths x 8 waypoints): one workgroup builds the tables of 64 paths.
// The 1000-entry sequential sum — np.cumsum's order, kept for bit-identity — costs a one-lane chain of 1000
// dependent fp64 adds per path in k_lut; here the 64 lanes of one wavefront each walk their own path's chain, so
// the chain is paid once per 64 paths.  Entries go through LDS in tiles of 32 per path: all threads evaluate
// magnitudes and trapezoid increments (lanes = consecutive entries of a path, so segment rows are read as
// broadcasts), the scanner wave adds, all threads store distances and slopes (256-byte rows).
// Same expressions in the same order as k_lut: the tables are bit-identical.
// Two group sizes: 64 paths per workgroup for very many short paths (W <= 9: config 5), 8 for large batches of paths of up
// to 64 waypoints (config 4's share: 1000 entries of 8 paths are one entry per thread and tile, the eight chains run in
// eight lanes).
constexpr int kLutManyTile = 32;
constexpr int kLutManyMinPaths = 32768;   // P = 64: batches from here on (and W <= 9)
constexpr int kLutGroupMinPaths = 8192;   // P = 8: batches from here on (and W <= 64); measured at 4096 x 32: 59 us against
                                          // k_lut's 57 (two workgroups per CU are too few to hide the barriers), at 8192: 75 against 93
template <int kLutManyPaths, int kLutManyThreads>
__global__ __launch_bounds__(kLutManyThreads, kLutManyThreads == 512 ? 4 : 1) void k_lut_many(int B, int W, const double *__restrict__ segments,
                                                               double *__restrict__ lut, double *__restrict__ slopes,
                                                               double *__restrict__ meta, uint32_t *__restrict__ flags,
                                                               GridArgs grid)
{
    constexpr int P = kLutManyPaths, TE = kLutManyTile, ST = TE + 1;   // row stride 33: lane = path reads hit 64 banks
    extern __shared__ __attribute__((aligned(16))) double s_seg[];     // the 64 paths' segment rows: P * G * 12
    __shared__ double s_mag[P * ST], s_inc[P * ST];
    __shared__ double s_prev_mag[P], s_carry[P], s_prev_cum[P], s_tmax[P], s_step[P];
    // Paths whose parameters[-1] is exactly W-1 (most: 78 % of config 5's — the rest are an ulp off, QHS:719-736) share
    // their table parameters linspace(0, W-1, 1000), hence segment index, local parameter and the six basis values of
    // every entry: those are evaluated ONCE per entry and workgroup (the reference's expressions, so the same bits), one
    // tile ahead, and a path of that class reads them instead of repeating ~40 of its ~130 operations per entry.
    // (one buffer, rewritten for the next tile right after the barrier that ends a tile's magnitude phase; bytes where
    // bytes do: two of these workgroups share a CU's 160 KB only while each stays under 80 KB)
    __shared__ double s_H[TE][6];
    __shared__ unsigned char s_hidx[TE], s_std[P];
    const int tid = threadIdx.x, b0 = blockIdx.x * P;
    const int G = W - 1;
    auto shared_basis = [&](int tile) {      // threads 0..TE-1: the class's entries of `tile`
        const int j = tile * TE + tid;
        if (tid < TE && j < kLutN) {
            const double t_max = (double)G;
            const double step = t_max / (double)(kLutN - 1);
            const double t = (j == kLutN - 1) ? t_max : (double)j * step;
            double lt, H[6];
            int idx;
            normalize_parameter(t, t_max, G, lt, idx);
            hermite_d1_basis_ref(lt, H);
#pragma unroll
            for (int i = 0; i < 6; i++) s_H[tid][i] = H[i];
            s_hidx[tid] = (unsigned char)idx;    // (W <= 64 in both group sizes)
        }
    };
    const int n_paths = B - b0 < P ? B - b0 : P;
    lds_fill<4>(s_seg, segments + (size_t)b0 * G * 12, n_paths * G * 12, tid, kLutManyThreads);
    if (tid < P) {
        s_prev_mag[tid] = 0.0; s_carry[tid] = 0.0; s_prev_cum[tid] = 0.0;
        const double tm = tid < n_paths ? meta[(size_t)(b0 + tid) * kMetaStride + 0] : 1.0;
        s_tmax[tid] = tm;
        // np.linspace's step (SM:443), once per path: the per-entry expressions below used to repeat this division —
        // and its twin in dt and in the slope — for every one of the 1000 entries (five IEEE divisions per entry
        // where one is needed)
        s_step[tid] = tm / (double)(kLutN - 1);
        s_std[tid] = tm == (double)G;
    }
    shared_basis(0);
    __syncthreads();
    constexpr int kTiles = (kLutN + TE - 1) / TE;
#pragma unroll 1
    for (int tl = 0; tl < kTiles; tl++) {
        const int j0 = tl * TE;
        // magnitudes |P'(t_j)| (SM:447-448): item = (path, entry), a wavefront covers two paths' 32 entries
#pragma unroll 2
        for (int r = 0; r < P * TE / kLutManyThreads; r++) {
            const int it = tid + r * kLutManyThreads, p = it / TE, e = it % TE, j = j0 + e, b = b0 + p;
            double m = 0.0;
            if (b < B && j < kLutN) {
                double H[6];
                int idx;
                if (s_std[p]) {
#pragma unroll
                    for (int i = 0; i < 6; i++) H[i] = s_H[e][i];
                    idx = s_hidx[e];
                } else {
                    const double t_max = s_tmax[p];
                    const double t = (j == kLutN - 1) ? t_max : (double)j * s_step[p];   // linspace_at(t_max, kLutN, j)
                    double lt;
                    normalize_parameter(t, t_max, G, lt, idx);
                    hermite_d1_basis_ref(lt, H);
                }
                double dx, dy;
                hermite_combine_ref(s_seg + ((size_t)p * G + idx) * 12, H, dx, dy);
                m = sqrt(dx * dx + dy * dy);
            }
            s_mag[p * ST + e] = m;
        }
        __syncthreads();
        if (tl + 1 < kTiles) shared_basis(tl + 1);     // (this tile's readers are past the barrier; the next tile's come after two more)
        // trapezoid increments (SM:452-454: (m[j-1] + m[j]) * 0.5 * dt, that association)
#pragma unroll
        for (int r = 0; r < P * TE / kLutManyThreads; r++) {
            const int it = tid + r * kLutManyThreads, p = it / TE, e = it % TE, j = j0 + e, b = b0 + p;
            double inc = 0.0;
            if (b < B && j > 0 && j < kLutN) {
                const double dt = (double)1 * s_step[p] - (double)0 * s_step[p];   // SM:444: local_params[1] - local_params[0]
                const double mp = e > 0 ? s_mag[p * ST + e - 1] : s_prev_mag[p];
                inc = (mp + s_mag[p * ST + e]) * 0.5 * dt;
            }
            s_inc[p * ST + e] = inc;
        }
        __syncthreads();
        // np.cumsum's strictly left-to-right sum, one lane per path
        if (tid < P) {
            double acc = s_carry[tid];
            const double last_mag = s_mag[tid * ST + TE - 1];
#pragma unroll
            for (int h = 0; h < TE; h += 8) {      // eight reads in flight, eight dependent adds, eight writes
                double v[8];
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = s_inc[tid * ST + h + e];
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    acc += v[e];
                    v[e] = acc;
                }
#pragma unroll
                for (int e = 0; e < 8; e++) s_mag[tid * ST + h + e] = v[e];   // the tile's distances
            }
            s_prev_mag[tid] = last_mag;
            s_carry[tid] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < P * TE / kLutManyThreads; r++) {
            const int it = tid + r * kLutManyThreads, p = it / TE, e = it % TE, j = j0 + e, b = b0 + p;
            if (b < B && j < kLutN) {
                const double c = s_mag[p * ST + e];
                lut[(size_t)b * kLutN + j] = c;
                if (slopes) {
                    // (t1 - t0)/(d1 - d0) of SM:311-317 for the interval ending at entry j
                    double w = 0.0;
                    if (j > 0) {
                        const double t_max = s_tmax[p];
                        const double lstep = s_step[p];
                        const double t0 = (double)(j - 1) * lstep, t1 = (j == kLutN - 1) ? t_max : (double)j * lstep;
                        const double cp = e > 0 ? s_mag[p * ST + e - 1] : s_prev_cum[p];
                        w = div_inrange(t1 - t0, c - cp);
                    }
                    slopes[(size_t)b * kLutN + j] = w;
                }
            }
        }
        __syncthreads();
        if (tid < P) s_prev_cum[tid] = s_mag[tid * ST + TE - 1];
        // (the next tile's first barrier orders this write before its readers)
    }
    if (tid < P && b0 + tid < B) {
        const int b = b0 + tid;
        const double acc = s_carry[tid];
        meta[(size_t)b * kMetaStride + 1] = acc;
        if (flags && !(acc > 0.0 && isfinite(acc))) atomicOr(&flags[b], VAP_FLAG_DEGENERATE_BIT);
        if (grid.aux) grid_define(b, W, grid.S, grid.dd, acc, meta[(size_t)b * kMetaStride + 0], meta, grid.aux, grid.runs, flags);
    }
}

// Slopes for a distance table that came in through the staged API.
__global__ void k_lut_slopes(int B, const double *__restrict__ lut, const double *__restrict__ meta,
                             double *__restrict__ slopes)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * kLutN) return;
    const int b = i / kLutN, j = i % kLutN;
    const double t_max = meta[(size_t)b * kMetaStride + 0];
    const double lstep = t_max / (double)(kLutN - 1);
    double w = 0.0;
    if (j > 0) {
        const double t0 = (double)(j - 1) * lstep, t1 = (j == kLutN - 1) ? t_max : (double)j * lstep;
        w = div_inrange(t1 - t0, lut[i] - lut[i - 1]);
    }
    slopes[i] = w;
}

// ------------------------------------------------------------------------------------------------
// Segment blocks -> monomial coefficients (scratch used by k_sample).
// ------------------------------------------------------------------------------------------------
__global__ void k_power(int n_seg, const double *__restrict__ segments, double *__restrict__ power)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seg) return;
    double r[12];
#pragma unroll
    for (int k = 0; k < 12; k++) r[k] = segments[(size_t)i * 12 + k];
    make_coef_block(r, power + (size_t)i * kCoefDoubles);
}

// ------------------------------------------------------------------------------------------------
// Scalar/vector accessors of one fitted path (the calls the GUI and L2 make one value at a time):
// SM:204-241 point / derivative / second derivative at a parameter.
// ------------------------------------------------------------------------------------------------
__global__ void k_eval(int W, const double *__restrict__ seg, double t_max, int order, int n,
                       const double *__restrict__ t, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x, y;
    hermite_eval_ref(seg, t_max, W - 1, order, t[i], x, y);
    out[2 * i] = x;
    out[2 * i + 1] = y;
}

// QHS:288-469 _get_basis_functions / _derivatives / _second_derivatives / _third_derivatives at n LOCAL parameters
__global__ void k_basis(int order, int n, const double *__restrict__ t, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double H[6];
    hermite_basis_ref(order, t[i], H);
#pragma unroll
    for (int k = 0; k < 6; k++) out[(size_t)i * 6 + k] = H[k];
}

// what: 0 = SM:291-318 distance_to_time, 1 = SM:340-346 get_curvature, 2 = SM:332-338 get_heading
__global__ void k_lookup(int W, const double *__restrict__ seg, double t_max, const double *__restrict__ lut,
                         int what, int n, const double *__restrict__ in, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double end_param = (double)(W - 1);
    if (what == 0) {
        out[i] = distance_to_time(lut, lut[kLutN - 1], t_max, end_param, in[i]);
        return;
    }
    const int tab_n = W * kSamplesPerNode;
    const int jj = table_index(in[i], tab_n, end_param);
    const double tp = linspace_at(end_param, tab_n, jj);
    double d1x, d1y;
    hermite_eval_ref(seg, t_max, W - 1, 1, tp, d1x, d1y);
    if (what == 2) {
        out[i] = atan2(d1y, d1x);  // SM:536
    } else {
        double d2x, d2y;
        hermite_eval_ref(seg, t_max, W - 1, 2, tp, d2x, d2y);
        const double ss = d1x * d1x + d1y * d1y;
        const double num = d1x * d2y - d1y * d2x;
        out[i] = (ss >= 1e-10) ? num / (ss * sqrt(ss)) : 0.0;  // SM:517-527
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
template <typename IT>
static hipError_t launch_fit_t(hipStream_t st, int B, int W, const void *wp, const double *tin,
                               const double *tout, const FitExtras &ex, double *seg, double *pw, double *seglen, double *meta,
                               uint32_t *flags)
{
    const size_t lds = sizeof(double) * (size_t)(7 * W);
    const bool plain = !tin && !tout && !seglen && !ex.first && !ex.second && !ex.start_tan && !ex.end_tan && !ex.out_first && !ex.out_second;
    if (plain && W <= 16 && B >= 8192) {
        // very many short paths: 256 / L paths per workgroup, L lanes each (k_fit would leave 56 of its 64 lanes idle at W = 8)
        int L = 4;
        while (L < W) L *= 2;
        const int per = 256 / L;
        hipLaunchKernelGGL(k_fit_many<IT>, dim3((B + per - 1) / per), dim3(256), lds * per, st, B, W, L, (const IT *)wp, seg, pw, meta, flags);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_fit<IT>, dim3(B), dim3(W <= 64 ? 64 : 256), lds, st, W, (const IT *)wp, tin, tout, ex,
                       seg, pw, seglen, meta, flags);
    return hipGetLastError();
}

hipError_t launch_fit(hipStream_t st, bool f64, int B, int W, const void *wp, const double *tin,
                      const double *tout, double *seg, double *pw, double *seglen, double *meta, uint32_t *flags,
                      const double *first, const double *second, const double *start_tan, const double *end_tan,
                      double *out_first, double *out_second)
{
    FitExtras ex;
    ex.first = first;
    ex.second = second;
    ex.start_tan = start_tan;
    ex.end_tan = end_tan;
    ex.out_first = out_first;
    ex.out_second = out_second;
    return f64 ? launch_fit_t<double>(st, B, W, wp, tin, tout, ex, seg, pw, seglen, meta, flags)
               : launch_fit_t<float>(st, B, W, wp, tin, tout, ex, seg, pw, seglen, meta, flags);
}

// K1 + K2 as one launch (k_fit_lut) where the fused call can take it: plain paths, segments that fit the table
// kernel's LDS staging, batches below the grouped table kernel's threshold.
bool fit_lut_fusable(int B, int W) { return W - 1 <= 512 && !(B >= kLutGroupMinPaths && W <= 64) && !(B >= kLutManyMinPaths && W <= 9); }
hipError_t launch_fit_lut(hipStream_t st, bool f64, int B, int W, const void *wp, double *seg, double *pw, double *lut,
                          double *meta, uint32_t *flags, GridArgs grid)
{
    const size_t n = (size_t)(7 * W > kLutPad ? 7 * W : kLutPad);
    // developer knob: VAP_LUT_STATS=1 prints in-kernel cycle shares (synchronises!)
    static const bool want_stats = getenv("VAP_LUT_STATS") != nullptr;
    long long *stats = nullptr;
    if (want_stats) (void)hipMalloc(&stats, (size_t)B * 4 * sizeof(long long));
    if (f64)
        hipLaunchKernelGGL(k_fit_lut<double>, dim3(B), dim3(128), sizeof(double) * n, st, W, (const double *)wp, seg, pw, lut, meta, flags, grid, stats);
    else
        hipLaunchKernelGGL(k_fit_lut<float>, dim3(B), dim3(128), sizeof(double) * n, st, W, (const float *)wp, seg, pw, lut, meta, flags, grid, stats);
    if (stats) {
        std::vector<long long> h((size_t)B * 4);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h.data(), stats, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
        (void)hipFree(stats);
        double sum[4] = {0, 0, 0, 0};
        for (int b = 0; b < B; b++)
            for (int k = 0; k < 4; k++) sum[k] += (double)h[(size_t)b * 4 + k];
        fprintf(stderr, "[fit+lut] mean ticks per workgroup: fit %.0f  magnitudes %.0f  increments+sum %.0f  store %.0f\n", sum[3] / B,
                sum[0] / B, sum[1] / B, sum[2] / B);
    }
    return hipGetLastError();
}

hipError_t launch_lut(hipStream_t st, int B, int W, const double *seg, double *lut, double *slopes, double *meta,
                      uint32_t *flags, GridArgs grid, RouteTables rt)
{
    static const bool want_stats = getenv("VAP_LUT_STATS") != nullptr;
    long long *stats = nullptr;
    if (want_stats) (void)hipMalloc(&stats, (size_t)B * 4 * sizeof(long long));
    // (the 64 paths' segment rows are staged in LDS: 6 KB per segment column, so short paths only)
    if (!want_stats && !rt.sptab && W <= 9 && B >= kLutManyMinPaths) {
        // very many paths: 64 per workgroup, the sequential sums of 64 paths in the lanes of one wavefront
        // (512 threads: two of these workgroups share a CU — LDS: 80 KB each — and eight waves each give its SIMDs four)
        hipLaunchKernelGGL((k_lut_many<64, 512>), dim3((B + 63) / 64), dim3(512), sizeof(double) * 64 * (W - 1) * 12, st, B, W, seg, lut,
                           slopes, meta, flags, grid);
        return hipGetLastError();
    }
    if (!want_stats && !rt.sptab && W <= 64 && B >= kLutGroupMinPaths) {
        hipLaunchKernelGGL((k_lut_many<8, 256>), dim3((B + 7) / 8), dim3(256), sizeof(double) * 8 * (W - 1) * 12, st, B, W, seg, lut,
                           slopes, meta, flags, grid);
        return hipGetLastError();
    }
    // 128 threads: the sequential sum keeps one lane busy, so residency (16 workgroups per CU) is what hides it
    const dim3 lgrid(B, rt.sptab ? rt.NS : 1);
    if (W - 1 <= 512) hipLaunchKernelGGL(k_lut<true>, lgrid, dim3(128), sizeof(double) * 12 * (W - 1), st, W, seg, lut, slopes, meta, flags, grid, rt, stats);
    else hipLaunchKernelGGL(k_lut<false>, lgrid, dim3(128), 0, st, W, seg, lut, slopes, meta, flags, grid, rt, stats);
    if (stats) {
        std::vector<long long> h((size_t)B * 4);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h.data(), stats, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
        (void)hipFree(stats);
        double sum[3] = {0, 0, 0};
        for (int b = 0; b < B; b++)
            for (int k = 0; k < 3; k++) sum[k] += (double)h[(size_t)b * 4 + k];
        fprintf(stderr, "[lut] mean ticks: magnitudes %.0f  increments+sum %.0f  store+slopes %.0f\n", sum[0] / B, sum[1] / B, sum[2] / B);
    }
    return hipGetLastError();
}

hipError_t launch_lut_slopes(hipStream_t st, int B, const double *lut, const double *meta, double *slopes)
{
    hipLaunchKernelGGL(k_lut_slopes, dim3((B * kLutN + 255) / 256), dim3(256), 0, st, B, lut, meta, slopes);
    return hipGetLastError();
}

hipError_t launch_grid(hipStream_t st, int B, int W, int S, double dd, double *meta, double *aux, double *runs,
                       uint32_t *flags)
{
    hipLaunchKernelGGL(k_grid, dim3((B + 63) / 64), dim3(64), 0, st, B, W, S, dd, meta, aux, runs, flags);
    return hipGetLastError();
}

hipError_t launch_power(hipStream_t st, int n_seg, const double *seg, double *pw)
{
    hipLaunchKernelGGL(k_power, dim3((n_seg + 255) / 256), dim3(256), 0, st, n_seg, seg, pw);
    return hipGetLastError();
}

hipError_t launch_eval(hipStream_t st, int W, const double *seg, double t_max, int order, int n, const double *t,
                       double *out)
{
    hipLaunchKernelGGL(k_eval, dim3((n + 255) / 256), dim3(256), 0, st, W, seg, t_max, order, n, t, out);
    return hipGetLastError();
}

hipError_t launch_basis(hipStream_t st, int order, int n, const double *t, double *out)
{
    hipLaunchKernelGGL(k_basis, dim3((n + 255) / 256), dim3(256), 0, st, order, n, t, out);
    return hipGetLastError();
}

hipError_t launch_lookup(hipStream_t st, int W, const double *seg, double t_max, const double *lut, int what,
                         int n, const double *in, double *out)
{
    hipLaunchKernelGGL(k_lookup, dim3((n + 255) / 256), dim3(256), 0, st, W, seg, t_max, lut, what, n, in, out);
    return hipGetLastError();
}

}  // namespace vap
