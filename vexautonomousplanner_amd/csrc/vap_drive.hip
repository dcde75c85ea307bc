// Can the drivetrain do this?  Two things the reference computes and never uses (include/vap.h, "drive limits"):
//
//   vap_curve_caps   per-sample velocity caps from the path's curvature, written into the `vcap` row the velocity pass
//                    already consumes: the lateral-acceleration cap sqrt(A / |k|) — what friction_coef is for — and the
//                    curvature-rate cap of MPG:41-50 on the finite difference of MPG:178-186 (dormant in the reference:
//                    commented out of both sweeps, MPG:215-220, 276-281), its end-point plus signs included.
//                    k_curve_caps: one thread per four consecutive samples, rows moved 16 bytes at a time where the row
//                    address allows and element by element otherwise (as k_limit_fill), the neighbour samples of the
//                    finite difference read once more at a thread's two edges; the per-path counts by integer atomics.
//   vap_drive_audit  wheel speeds (MPG:594-599), wheel accelerations (MPG:612-616), jerk, lateral and angular acceleration
//                    of time-domain rows: per route the peak of each, the first row attaining it, the rows above a limit.
//                    k_drive_rows<false>: a workgroup per tile of a route's rows, a lane per row; a row's two predecessors
//                    come from LDS (the last two rows of a 256-row step are handed to the next step there), each lane keeps
//                    (value, first row) per quantity and the workgroup reduces them under one total order — larger value,
//                    then lower row — so the result does not depend on the tiling; k_drive_finish: a wave per route over
//                    the tiles' partials.  k_drive_rows<true> writes the per-row columns, after the route's status is known.
//                    No float atomics anywhere: two calls give the same bits.
#include "vap_ctx_state.h"

#include <climits>

namespace vap {
namespace {

constexpr int kDriveThreads = 256;
constexpr int kGridYMax = 65535;
constexpr int kQ = 5;                    // audited quantities
constexpr int kPartInts = 16;            // per tile: peak row [5], rows over [5], first row over [5], non-finite
constexpr int kMetaStride = 4;           // meta [B][4]: parameters[-1], total_length, dd, n_samples

// ---- vap_curve_caps -------------------------------------------------------------------------------------------------------

template <typename T>
__device__ inline void load4(const T *__restrict__ p, int k0, int S, double (&x)[4])
{
    if (k0 + 3 < S && ((uintptr_t)p & 15) == 0) {          // the address, not the offset: the caller's base may sit anywhere
        if constexpr (sizeof(T) == 8) {
            const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
            x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
        } else {
            const float4 a = *reinterpret_cast<const float4 *>(p);
            x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w;
        }
    } else {
        for (int j = 0; j < 4; j++) x[j] = k0 + j < S ? (double)p[j] : 0.0;
    }
}

template <typename T>
__device__ inline void store4(T *__restrict__ p, int k0, int S, const double (&x)[4])
{
    if (k0 + 3 < S && ((uintptr_t)p & 15) == 0) {
        if constexpr (sizeof(T) == 8) {
            *reinterpret_cast<double2 *>(p) = make_double2(x[0], x[1]);
            *reinterpret_cast<double2 *>(p + 2) = make_double2(x[2], x[3]);
        } else {
            *reinterpret_cast<float4 *>(p) = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
        }
    } else {
        for (int j = 0; j < 4 && k0 + j < S; j++) p[j] = (T)x[j];
    }
}

// KT: type of the curvature row, R: type of the cap rows.  vin may be null (max_vel everywhere) and may be vout.
template <typename KT, typename R>
__global__ void __launch_bounds__(kDriveThreads)
k_curve_caps(int b0, int S, double max_vel, double A, double alpha, const double *__restrict__ meta, const KT *__restrict__ curv,
             const R *vin, R *vout, int *__restrict__ n_bound)
{
    __shared__ int s_cnt[2];
    const int b = b0 + blockIdx.y;
    const double m3 = meta[(size_t)b * kMetaStride + 3], dd = meta[(size_t)b * kMetaStride + 2];
    const int N = !(m3 >= 0.0) ? 0 : (m3 > (double)S ? S : (int)m3);
    const bool ang_on = N >= 2 && alpha != INFINITY;
    if (n_bound) {
        if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
        __syncthreads();
    }
    const KT *K = curv + (size_t)b * S;
    int c_lat = 0, c_ang = 0;
    for (int k0 = (blockIdx.x * kDriveThreads + threadIdx.x) * 4; k0 < S; k0 += gridDim.x * kDriveThreads * 4) {
        const size_t o = (size_t)b * S + k0;
        double x[4];
        if (vin) load4(vin + o, k0, S, x);
        else x[0] = x[1] = x[2] = x[3] = max_vel;
        if (k0 < N) {
            double kk[6];                                   // samples k0 - 1 .. k0 + 4
            double mid[4];
            load4(K + k0, k0, S, mid);
            kk[0] = k0 > 0 ? (double)K[k0 - 1] : 0.0;
            kk[1] = mid[0], kk[2] = mid[1], kk[3] = mid[2], kk[4] = mid[3];
            kk[5] = k0 + 4 < N ? (double)K[k0 + 4] : 0.0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = k0 + j;
                if (i >= N) break;
                const double k = kk[j + 1], ak = fabs(k);
                const double cap_lat = ak > 0.0 ? sqrt(A / ak) : INFINITY;
                double cap_ang = INFINITY;
                if (ang_on) {
                    // MPG:178-186, the sums at the two ends as the reference has them
                    const double dk = i == 0 ? (kk[j + 2] + k) / dd : (i == N - 1 ? (k + kk[j]) / dd : (kk[j + 2] - kk[j]) / (2.0 * dd));
                    const double adk = fabs(dk);
                    if (adk < 1e-9) {                       // MPG:45-46
                        cap_ang = max_vel;
                    } else {
                        const double s = sqrt(alpha / adk); // MPG:47-50: min(sqrt, max_vel) keeps the left operand on a tie or NaN
                        cap_ang = max_vel < s ? max_vel : s;
                    }
                }
                const double in = x[j];
                double out = in;
                if (cap_lat < out) out = cap_lat;
                if (cap_ang < out) out = cap_ang;
                if (k != k) out = k;                        // a NaN curvature: a NaN cap (the pass flags such a path)
                c_lat += cap_lat < in;
                c_ang += cap_ang < in;
                x[j] = out;
            }
        }
        store4(vout + o, k0, S, x);
    }
    if (n_bound) {
        if (c_lat) atomicAdd(&s_cnt[0], c_lat);
        if (c_ang) atomicAdd(&s_cnt[1], c_ang);
        __syncthreads();
        if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&n_bound[(size_t)b * 2 + threadIdx.x], s_cnt[threadIdx.x]);
    }
}

template <typename KT, typename R>
void launch_curve_caps(hipStream_t st, int B, int S, double max_vel, double A, double alpha, const double *meta, const void *curv,
                       const void *vin, void *vout, int *n_bound)
{
    const unsigned gx = (unsigned)((S + 1023) / 1024 < 64 ? (S + 1023) / 1024 : 64);
    for (int b0 = 0; b0 < B; b0 += kGridYMax) {
        const int nb = B - b0 < kGridYMax ? B - b0 : kGridYMax;
        hipLaunchKernelGGL((k_curve_caps<KT, R>), dim3(gx, (unsigned)nb), dim3(kDriveThreads), 0, st, b0, S, max_vel, A, alpha, meta,
                           (const KT *)curv, (const R *)vin, (R *)vout, n_bound);
    }
}

// ---- vap_drive_audit ------------------------------------------------------------------------------------------------------

struct AuditArgs {
    const double *rows;
    const int *counts;
    int stride, cap, B, b0;
    int iters;              // 256-row steps per tile
    int tiles;              // tiles per route
    double T, h, lim[kQ];
    double *part_val;       // [B][tiles][5]
    int *part_int;          // [B][tiles][16]
    int *status;            // [B] context scratch
    double *peak;
    int *peak_row, *n_over, *first_over, *route_status;
    double *wheel;
};

struct Best {
    double val;             // -1: none yet (every quantity is an absolute value)
    int row;
};

// one total order — the larger value, then the lower row — so that any order of combining gives the first row of the maximum
__device__ inline void take(Best &a, double val, int row)
{
    if (val > a.val || (val == a.val && row < a.row)) a.val = val, a.row = row;
}

__device__ inline double shfl_down_f64(double x, int d)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __shfl_down(lo, d);
    hi = __shfl_down(hi, d);
    return __hiloint2double(hi, lo);
}

struct Acc {
    Best best[kQ];
    int over[kQ], first[kQ], bad;
};

__device__ inline void acc_init(Acc &a)
{
    for (int q = 0; q < kQ; q++) a.best[q] = Best{-1.0, INT_MAX}, a.over[q] = 0, a.first[q] = INT_MAX;
    a.bad = 0;
}

__device__ inline void acc_wave_reduce(Acc &a)
{
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int q = 0; q < kQ; q++) {
            const double v = shfl_down_f64(a.best[q].val, d);
            const int r = __shfl_down(a.best[q].row, d);
            take(a.best[q], v, r);
            a.over[q] += __shfl_down(a.over[q], d);
            const int f = __shfl_down(a.first[q], d);
            a.first[q] = f < a.first[q] ? f : a.first[q];
        }
        a.bad |= __shfl_down(a.bad, d);
    }
}

// WHEEL = false: the tile's partial (peaks, counts, a non-finite v or omega).  WHEEL = true: the per-row columns of the routes
// whose status is 0.
template <bool WHEEL>
__global__ void __launch_bounds__(kDriveThreads) k_drive_rows(AuditArgs g)
{
    __shared__ double s_v[2][kDriveThreads + 2], s_w[2][kDriveThreads + 2];
    __shared__ double s_val[kDriveThreads / 64][kQ];
    __shared__ int s_int[kDriveThreads / 64][kPartInts];
    const int b = g.b0 + blockIdx.y, t = threadIdx.x;
    int n = g.counts[(size_t)b * g.stride];
    n = n < 0 ? 0 : (n > g.cap ? g.cap : n);
    const int tile_rows = g.iters * kDriveThreads;
    const int r_begin = blockIdx.x * tile_rows;
    if (r_begin >= n) return;                               // (the whole workgroup: nothing of this route here)
    if constexpr (WHEEL)
        if (g.status[b]) return;
    const double *R = g.rows + (size_t)b * g.cap * 8;
    Acc a;
    acc_init(a);
    for (int it = 0; it < g.iters; it++) {
        const int r0 = r_begin + it * kDriveThreads;
        if (r0 >= n) break;
        const int r = r0 + t, cur = it & 1;
        double v = 0.0, w = 0.0;
        if (r < n) {
            v = R[(size_t)r * 8 + 2];
            w = R[(size_t)r * 8 + 5];
        }
        s_v[cur][t + 2] = v;
        s_w[cur][t + 2] = w;
        if (t < 2) {
            // the two rows in front of this step: the route's own (nothing moves before row 0) on a tile's first step, then
            // the last two rows of the step before, which are still in the other buffer
            double hv = 0.0, hw = 0.0;
            if (it == 0) {
                const int hr = r0 - 2 + t;
                if (hr >= 0) {
                    hv = R[(size_t)hr * 8 + 2];
                    hw = R[(size_t)hr * 8 + 5];
                }
            } else {
                hv = s_v[cur ^ 1][kDriveThreads + t];
                hw = s_w[cur ^ 1][kDriveThreads + t];
            }
            s_v[cur][t] = hv;
            s_w[cur][t] = hw;
        }
        __syncthreads();
        if (r < n) {
            const double v1 = s_v[cur][t + 1], v2 = s_v[cur][t], w1 = s_w[cur][t + 1];
            const double half = (w * g.T) / 2.0, half1 = (w1 * g.T) / 2.0;
            const double wl = v - half, wr = v + half;                  // MPG:594-599
            const double wl1 = v1 - half1, wr1 = v1 + half1;
            const double al = (wl - wl1) / g.h, ar = (wr - wr1) / g.h;  // MPG:612-616 (row 0: from a wheel that stands still)
            const double bb = (v - v1) / g.h, b1 = (v1 - v2) / g.h;
            const double jj = (bb - b1) / g.h;
            const double ll = v * w;
            const double gg = (w - w1) / g.h;
            if constexpr (WHEEL) {
                double2 *o = reinterpret_cast<double2 *>(g.wheel + ((size_t)b * g.cap + r) * 8);
                o[0] = make_double2(wl, wr);
                o[1] = make_double2(al, ar);
                o[2] = make_double2(bb, jj);
                o[3] = make_double2(ll, gg);
            } else {
                const double awl = fabs(wl), awr = fabs(wr), aal = fabs(al), aar = fabs(ar);
                const double q[kQ] = {awl < awr ? awr : awl, aal < aar ? aar : aal, fabs(jj), fabs(ll), fabs(gg)};
#pragma unroll
                for (int i = 0; i < kQ; i++) {
                    if (q[i] == q[i] && q[i] > a.best[i].val) a.best[i] = Best{q[i], r};   // (a lane's rows ascend)
                    if (q[i] > g.lim[i]) {
                        a.over[i]++;
                        if (r < a.first[i]) a.first[i] = r;
                    }
                }
                if (!isfinite(v) || !isfinite(w)) a.bad = 1;
            }
        }
    }
    if constexpr (!WHEEL) {
        acc_wave_reduce(a);
        const int wave = t >> 6;
        if ((t & 63) == 0) {
            for (int q = 0; q < kQ; q++) {
                s_val[wave][q] = a.best[q].val;
                s_int[wave][q] = a.best[q].row;
                s_int[wave][kQ + q] = a.over[q];
                s_int[wave][2 * kQ + q] = a.first[q];
            }
            s_int[wave][3 * kQ] = a.bad;
        }
        __syncthreads();
        if (t == 0) {
            for (int wv = 1; wv < kDriveThreads / 64; wv++) {
                for (int q = 0; q < kQ; q++) {
                    take(a.best[q], s_val[wv][q], s_int[wv][q]);
                    a.over[q] += s_int[wv][kQ + q];
                    a.first[q] = s_int[wv][2 * kQ + q] < a.first[q] ? s_int[wv][2 * kQ + q] : a.first[q];
                }
                a.bad |= s_int[wv][3 * kQ];
            }
            const size_t p = (size_t)b * g.tiles + blockIdx.x;
            for (int q = 0; q < kQ; q++) {
                g.part_val[p * kQ + q] = a.best[q].val;
                g.part_int[p * kPartInts + q] = a.best[q].row;
                g.part_int[p * kPartInts + kQ + q] = a.over[q];
                g.part_int[p * kPartInts + 2 * kQ + q] = a.first[q];
            }
            g.part_int[p * kPartInts + 3 * kQ] = a.bad;
        }
    }
}

// One wave per route: the tiles' partials, lanes striding over the tiles.
__global__ void __launch_bounds__(64) k_drive_finish(AuditArgs g)
{
    const int b = blockIdx.x, t = threadIdx.x;
    int n = g.counts[(size_t)b * g.stride];
    n = n < 0 ? 0 : (n > g.cap ? g.cap : n);
    const int tile_rows = g.iters * kDriveThreads;
    const int nt = (int)(((long)n + tile_rows - 1) / tile_rows);
    Acc a;
    acc_init(a);
    for (int i = t; i < nt; i += 64) {
        const size_t p = (size_t)b * g.tiles + i;
        for (int q = 0; q < kQ; q++) {
            take(a.best[q], g.part_val[p * kQ + q], g.part_int[p * kPartInts + q]);
            a.over[q] += g.part_int[p * kPartInts + kQ + q];
            const int f = g.part_int[p * kPartInts + 2 * kQ + q];
            a.first[q] = f < a.first[q] ? f : a.first[q];
        }
        a.bad |= g.part_int[p * kPartInts + 3 * kQ];
    }
    acc_wave_reduce(a);
    if (t != 0) return;
    g.status[b] = a.bad ? 2 : 0;
    if (g.route_status) g.route_status[b] = a.bad ? 2 : 0;
    for (int q = 0; q < kQ; q++) {
        const bool none = a.bad || a.best[q].row == INT_MAX;     // no rows, a non-finite route, or every value a NaN
        const size_t o = (size_t)b * kQ + q;
        if (g.peak) g.peak[o] = none ? NAN : a.best[q].val;
        if (g.peak_row) g.peak_row[o] = none ? -1 : a.best[q].row;
        if (g.n_over) g.n_over[o] = a.bad ? 0 : a.over[q];
        if (g.first_over) g.first_over[o] = (a.bad || a.first[q] == INT_MAX) ? -1 : a.first[q];
    }
}

}  // namespace
}  // namespace vap

extern "C" {

int vap_curve_caps(vap_ctx *ctx, vap_dtype dt, int B, int S, const vap_constraints *c, const vap_curve_limits *lim,
                   const double *d_meta, const void *d_curvature, const void *d_vcap_in, void *d_vcap_out, int *d_n_bound)
{
    if (dt != VAP_F32 && dt != VAP_F64) return vap_fail(VAP_ERR_INVALID, "bad dtype %d", (int)dt);
    if (B < 0) return vap_fail(VAP_ERR_INVALID, "batch must be >= 0 (got %d)", B);
    if (B > 0) {
        if (S < 2) return vap_fail(VAP_ERR_INVALID, "S must be >= 2 (got %d)", S);
        if (!c || !lim || !d_meta || !d_vcap_out) return vap_fail(VAP_ERR_INVALID, "null constraints, limits, meta or output row");
    }
    if (lim && (!(lim->lateral_acc_max > 0.0) || !(lim->angular_acc_max > 0.0)))
        return vap_fail(VAP_ERR_INVALID, "curve limits must be positive (+inf: off), got lateral %g, angular %g", lim->lateral_acc_max,
                        lim->angular_acc_max);
    if (c && (!std::isfinite(c->max_vel) || !std::isfinite(c->track_width)))
        return vap_fail(VAP_ERR_INVALID, "max_vel and track_width must be finite (got %g, %g)", c->max_vel, c->track_width);
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;
    // the curvature row: the caller's in `dt`, or the fp64 row the last sampling call left on the context
    bool k64 = dt == VAP_F64;
    if (!d_curvature) {
        const void *dth = nullptr;
        bool r64 = false;
        VAP_TRY(vap_ctx_rows(ctx, dt, B, S, d_curvature, dth, r64));
        if (!r64 || !d_curvature)
            return vap_fail(VAP_ERR_INVALID, "d_curvature is NULL and the context holds no fp64 curvature rows (VAP_F32 with "
                                             "VAP_RECURRENCE_F64 only)");
        k64 = true;
    }
    const bool r64 = vap_limit_rows_dtype(ctx, dt) == (int)VAP_F64;
    if (k64 && !r64) return vap_fail(VAP_ERR_INVALID, "fp64 curvature rows with fp32 limit rows");
    if (d_n_bound) HIP_TRY(hipMemsetAsync(d_n_bound, 0, (size_t)B * 2 * sizeof(int), ctx->stream));
    const double A = lim->lateral_acc_max, alpha = lim->angular_acc_max;
    if (k64)
        vap::launch_curve_caps<double, double>(ctx->stream, B, S, c->max_vel, A, alpha, d_meta, d_curvature, d_vcap_in, d_vcap_out, d_n_bound);
    else if (r64)
        vap::launch_curve_caps<float, double>(ctx->stream, B, S, c->max_vel, A, alpha, d_meta, d_curvature, d_vcap_in, d_vcap_out, d_n_bound);
    else
        vap::launch_curve_caps<float, float>(ctx->stream, B, S, c->max_vel, A, alpha, d_meta, d_curvature, d_vcap_in, d_vcap_out, d_n_bound);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

int vap_drive_audit(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                    double time_step, const vap_drive_limits *lim, double *d_peak, int *d_peak_row, int *d_n_over,
                    int *d_first_over, int *d_route_status, double *d_wheel_rows)
{
    if (B < 0 || capacity < 0) return vap_fail(VAP_ERR_INVALID, "bad shape B=%d capacity=%ld", B, capacity);
    if (counts_stride < 1) return vap_fail(VAP_ERR_INVALID, "counts_stride must be >= 1 (got %d)", counts_stride);
    if (!(time_step > 0.0) || !std::isfinite(time_step)) return vap_fail(VAP_ERR_INVALID, "time_step must be positive and finite (got %g)", time_step);
    if (B > 0 && (!d_rows || !d_counts || !lim)) return vap_fail(VAP_ERR_INVALID, "null rows, counts or limits");
    if (lim) {
        if (!(lim->track_width > 0.0) || !std::isfinite(lim->track_width))
            return vap_fail(VAP_ERR_INVALID, "track_width must be positive and finite (got %g)", lim->track_width);
        const double l[5] = {lim->wheel_speed_max, lim->wheel_acc_max, lim->jerk_max, lim->lateral_acc_max, lim->angular_acc_max};
        for (int q = 0; q < 5; q++)
            if (!(l[q] >= 0.0)) return vap_fail(VAP_ERR_INVALID, "drive limit %d is NaN or negative (%g; +inf: never exceeded)", q, l[q]);
    }
    if ((((uintptr_t)d_rows | (uintptr_t)d_wheel_rows) & 15) != 0)
        return vap_fail(VAP_ERR_INVALID, "rows and wheel rows must be 16-byte aligned");
    if (capacity > INT_MAX - 2048) return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld above %d", capacity, INT_MAX - 2048);
    VAP_TRY(vap_set_device(ctx));
    if (B == 0) return VAP_OK;

    vap::AuditArgs g{};
    g.rows = d_rows;
    g.counts = d_counts;
    g.stride = counts_stride;
    g.cap = (int)capacity;
    g.B = B;
    g.T = lim->track_width;
    g.h = time_step;
    g.lim[0] = lim->wheel_speed_max, g.lim[1] = lim->wheel_acc_max, g.lim[2] = lim->jerk_max, g.lim[3] = lim->lateral_acc_max;
    g.lim[4] = lim->angular_acc_max;
    // long tiles (four 256-row steps, one reduction) once there are workgroups enough to fill the device; a short batch of
    // long routes keeps one step per tile, so that one chained routine still spreads over the CUs
    const long tiles4 = (capacity + 4 * vap::kDriveThreads - 1) / (4 * vap::kDriveThreads);
    g.iters = (long)B * tiles4 >= 1024 ? 4 : 1;
    const long tile_rows = (long)g.iters * vap::kDriveThreads;
    g.tiles = (int)((capacity + tile_rows - 1) / tile_rows);
    g.peak = d_peak;
    g.peak_row = d_peak_row;
    g.n_over = d_n_over;
    g.first_over = d_first_over;
    g.route_status = d_route_status;
    g.wheel = d_wheel_rows;
    // context scratch: the routes' status words, the tiles' values, the tiles' integers
    const size_t np = (size_t)B * (size_t)(g.tiles > 0 ? g.tiles : 1);
    const size_t status_bytes = (((size_t)B * sizeof(int)) + 15) & ~(size_t)15;
    const size_t val_bytes = np * vap::kQ * sizeof(double);
    VAP_TRY(ctx->ensure(ctx->drive_part, status_bytes + val_bytes + np * vap::kPartInts * sizeof(int)));
    g.status = (int *)ctx->drive_part.ptr;
    g.part_val = (double *)((char *)ctx->drive_part.ptr + status_bytes);
    g.part_int = (int *)((char *)g.part_val + val_bytes);

    auto rows_pass = [&](bool wheel) {
        if (g.tiles == 0) return;
        for (int b0 = 0; b0 < B; b0 += vap::kGridYMax) {
            const int nb = B - b0 < vap::kGridYMax ? B - b0 : vap::kGridYMax;
            g.b0 = b0;
            if (wheel) hipLaunchKernelGGL(vap::k_drive_rows<true>, dim3((unsigned)g.tiles, (unsigned)nb), dim3(vap::kDriveThreads), 0, ctx->stream, g);
            else hipLaunchKernelGGL(vap::k_drive_rows<false>, dim3((unsigned)g.tiles, (unsigned)nb), dim3(vap::kDriveThreads), 0, ctx->stream, g);
        }
    };
    rows_pass(false);
    hipLaunchKernelGGL(vap::k_drive_finish, dim3((unsigned)B), dim3(64), 0, ctx->stream, g);
    if (d_wheel_rows) rows_pass(true);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
