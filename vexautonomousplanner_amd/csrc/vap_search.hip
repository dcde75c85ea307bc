// vap_search.hip — cross-entropy route search over batches of candidate trajectories (vap_search_sample,
// vap_search_update).
//
// The evaluation calls judge candidates; these two make them and act on the verdicts.  R routes ("problems") are refined
// at a time with N candidates each: vap_search_sample draws the candidates' waypoints around a mean, the existing calls
// profile and check them, vap_search_update scores and ranks them, refits the mean and sigma to the elites and keeps the
// best route so far.  Nothing here reads a result on the host.  Definitions: include/vap.h.
//
//   k_search_sample  a thread per (candidate, waypoint): one Philox4x32-10 block gives the waypoint's two normals
//                    (Box-Muller in fp64), the pair goes out as one 8-byte (fp32) or 16-byte (fp64) store, consecutive
//                    threads on consecutive addresses.  The counter is (n, w, iteration, problem), so a candidate does
//                    not depend on R, N or the launch shape.
//   k_search_update  a workgroup per problem.  The costs become sortable 64-bit keys in LDS (the sign-flipped bits of
//                    the double, so that integer order is the order of the costs) beside the candidate's index; a
//                    workgroup-wide bitonic sort orders the (key, index) pairs, which are unique, so the order is the
//                    same in every run: 4096 x 12 B = 48 KiB of LDS.  Then a thread per coordinate walks the elites in
//                    rank order (two passes: mean, population variance); consecutive threads read consecutive
//                    coordinates of one elite.  Thread 0 decides on the best-so-far, all threads copy its waypoints.
//                    No float atomics: two calls give the same bits.
#include <climits>
#include <cmath>
#include <cstdint>

#include "vap_internal.h"
#include "vap_kernels.h"
#include "vap_philox.h"          // philox4x32_10 (shared with vap_conditioning.hip)

namespace vap {

constexpr int kSearchMaxCandidates = 4096;
constexpr int kSearchSampleThreads = 256;

template <typename T>
struct Pair;
template <>
struct Pair<float> {
    using type = float2;
    static __device__ __forceinline__ float2 make(double a, double b) { return make_float2((float)a, (float)b); }
};
template <>
struct Pair<double> {
    using type = double2;
    static __device__ __forceinline__ double2 make(double a, double b) { return make_double2(a, b); }
};

struct SampleArgs {
    int R, N, W;
    size_t total;              // R * N * W
    const double *mean, *sigma;
    const void *best_wp;
    const double *best_cost;
    uint32_t seed_lo, seed_hi, iteration, first_problem;
    void *out;
};

template <typename T>
__global__ __launch_bounds__(kSearchSampleThreads) void k_search_sample(SampleArgs g)
{
    using P = typename Pair<T>::type;
    const size_t t = (size_t)blockIdx.x * kSearchSampleThreads + threadIdx.x;
    if (t >= g.total) return;
    const int w = (int)(t % (size_t)g.W);
    const size_t c = t / (size_t)g.W;
    const int n = (int)(c % (size_t)g.N), r = (int)(c / (size_t)g.N);
    const size_t node = (size_t)r * g.W + w;
    const double2 m = ((const double2 *)g.mean)[node];
    P o;
    if (n == 0) {
        // elitism: the best route so far, or the mean while there is none
        if (g.best_wp && g.best_cost && isfinite(g.best_cost[r]))
            o = ((const P *)g.best_wp)[node];
        else
            o = Pair<T>::make(m.x, m.y);
    } else {
        const double2 s = ((const double2 *)g.sigma)[node];
        const uint4x x = philox4x32_10(uint4x{(uint32_t)n, (uint32_t)w, g.iteration, g.first_problem + (uint32_t)r}, g.seed_lo, g.seed_hi);
        const double u1 = ((double)x.x + 0.5) * 0x1p-32, u2 = ((double)x.y + 0.5) * 0x1p-32;
        const double rho = sqrt(-2.0 * log(u1));
        double sn, cs;
        sincos(6.283185307179586 * u2, &sn, &cs);
        const double zx = rho * cs, zy = rho * sn;
        // a sigma of 0 pins the coordinate: the mean's own bits
        o = Pair<T>::make(s.x == 0.0 ? m.x : m.x + s.x * zx, s.y == 0.0 ? m.y : m.y + s.y * zy);
    }
    ((P *)g.out)[t] = o;
}

struct UpdateArgs {
    int R, N, W, P;            // P: N rounded up to a power of two
    const void *wp;            // [R * N][W][2]
    const int *counts;
    int stride;
    double time_step;
    const double *meta;
    const uint32_t *flags;
    const double *clearance, *conflict, *tracking;
    vap_search_weights w;
    int E;
    double alpha, sigma_min, sigma_max;
    double *mean, *sigma;
    double *cost, *violation;
    int *order, *n_feasible;
    double *best_cost;
    void *best_wp;
    double *best_terms, *history;
    int history_stride;
    uint32_t iteration;
};

// the cost of candidate b (include/vap.h); dur, len, viol: its terms
__device__ __forceinline__ double search_cost(const UpdateArgs &g, size_t b, double &dur, double &len, double &viol)
{
    bool bad = false, nan_term = false;
    dur = 0.0;
    len = 0.0;
    viol = 0.0;
    if (g.counts) {
        const int c = g.counts[b * (size_t)g.stride];
        bad |= c <= 0;
        dur = (double)c * g.time_step;
    }
    if (g.meta) {
        len = g.meta[b * 4 + 1];
        bad |= isnan(len);
    }
    if (g.flags) bad |= g.flags[b] != 0u;
    if (g.clearance) {
        const double v = g.clearance[b];
        nan_term |= isnan(v);
        viol += fmax(0.0, g.w.clearance_margin - v);
    }
    if (g.conflict) {
        const double v = g.conflict[b];
        nan_term |= isnan(v);
        viol += fmax(0.0, g.w.conflict_margin - v);
    }
    if (g.tracking) {
        const double v = g.tracking[b];
        nan_term |= isnan(v);
        viol += fmax(0.0, v - g.w.tracking_tolerance);
    }
    if (nan_term) viol = NAN;
    double cost = g.w.w_time * dur + g.w.w_length * len;
    if (viol > 0.0) cost = cost + (g.w.infeasible_base + g.w.w_violation * viol);
    if (bad || nan_term || isnan(cost)) cost = INFINITY;
    return cost;
}

// a double's bits as an unsigned key whose integer order is the order of the doubles (-inf < ... < +inf), and back
__device__ __forceinline__ unsigned long long sortable_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

template <typename T>
__global__ __launch_bounds__(1024) void k_search_update(UpdateArgs g)
{
    __shared__ unsigned long long s_key[kSearchMaxCandidates];
    __shared__ int s_idx[kSearchMaxCandidates];
    __shared__ int s_nfeas, s_nfinite, s_replace;
    const int r = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, P = g.P, W2 = 2 * g.W;
    const size_t b0 = (size_t)r * N;
    if (tid == 0) s_nfeas = s_nfinite = s_replace = 0;
    __syncthreads();

    // score: keys into LDS; the padding sorts behind +inf
    for (int i = tid; i < P; i += nt) {
        unsigned long long key = ~0ull;
        if (i < N) {
            double dur, len, viol;
            const double cost = search_cost(g, b0 + i, dur, len, viol);
            if (g.cost) g.cost[b0 + i] = cost;
            if (g.violation) g.violation[b0 + i] = viol;
            if (cost < INFINITY) {
                atomicAdd(&s_nfinite, 1);               // integer counts: the order of the adds does not matter
                if (viol == 0.0) atomicAdd(&s_nfeas, 1);
            }
            key = sortable_key(cost);
        }
        s_key[i] = key;
        s_idx[i] = i;
    }

    // rank: bitonic sort of the (key, index) pairs, ascending
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < P; i += nt) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long ka = s_key[i], kb = s_key[l];
                    const int ia = s_idx[i], ib = s_idx[l];
                    const bool gt = ka > kb || (ka == kb && ia > ib);
                    if (gt == ((i & k) == 0)) {
                        s_key[i] = kb;
                        s_key[l] = ka;
                        s_idx[i] = ib;
                        s_idx[l] = ia;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (g.order)
        for (int i = tid; i < N; i += nt) g.order[b0 + i] = s_idx[i];
    if (tid == 0 && g.n_feasible) g.n_feasible[r] = s_nfeas;

    // refit: a thread per coordinate walks the elites in rank order
    const int ne = g.E < s_nfinite ? g.E : s_nfinite;
    const T *wp = (const T *)g.wp;
    if (g.mean && ne > 0) {
        for (int j = tid; j < W2; j += nt) {
            const size_t mj = (size_t)r * W2 + j;
            const double sg = g.sigma[mj];
            if (sg == 0.0) continue;                     // pinned: mean and sigma keep their bits
            double sum = 0.0;
#pragma unroll 1
            for (int e = 0; e < ne; e++) sum += (double)wp[(b0 + s_idx[e]) * (size_t)W2 + j];
            const double me = sum / (double)ne;
            double sq = 0.0;
#pragma unroll 1
            for (int e = 0; e < ne; e++) {
                const double d = (double)wp[(b0 + s_idx[e]) * (size_t)W2 + j] - me;
                sq += d * d;
            }
            const double var = sq / (double)ne;
            g.mean[mj] = (1.0 - g.alpha) * g.mean[mj] + g.alpha * me;
            const double s = sqrt((1.0 - g.alpha) * (sg * sg) + g.alpha * var);
            g.sigma[mj] = fmin(fmax(s, g.sigma_min), g.sigma_max);
        }
    }

    // best so far: replaced only by a strictly lower cost
    if (!g.best_cost) return;
    const int top = s_idx[0];
    if (tid == 0) {
        double dur, len, viol;
        const double c = search_cost(g, b0 + top, dur, len, viol);   // == key_value(s_key[0])
        double best = g.best_cost[r];
        if (c < INFINITY && c < best) {
            best = c;
            g.best_cost[r] = c;
            if (g.best_terms) {
                double *t = g.best_terms + (size_t)r * 4;
                t[0] = dur;
                t[1] = len;
                t[2] = viol;
                t[3] = (double)top;
            }
            s_replace = 1;
        }
        if (g.history) g.history[(size_t)r * g.history_stride + g.iteration] = best;
    }
    __syncthreads();
    if (s_replace && g.best_wp) {
        T *dst = (T *)g.best_wp + (size_t)r * W2;
        for (int j = tid; j < W2; j += nt) dst[j] = wp[(b0 + top) * (size_t)W2 + j];
    }
}

}  // namespace vap

extern "C" {

int vap_search_sample(vap_ctx *ctx, int dt, int R, int N, int W, const double *d_mean, const double *d_sigma,
                      const void *d_best_waypoints, const double *d_best_cost, uint64_t seed, uint32_t iteration,
                      uint32_t first_problem, void *d_waypoints)
{
    using namespace vap;
    if (dt != VAP_F32 && dt != VAP_F64) return vap_fail(VAP_ERR_INVALID, "bad dtype %d", dt);
    if (R < 0) return vap_fail(VAP_ERR_INVALID, "bad shape R=%d", R);
    if (N < 1 || N > kSearchMaxCandidates) return vap_fail(VAP_ERR_INVALID, "N = %d candidates per problem outside 1..%d", N, kSearchMaxCandidates);
    if (W < 2) return vap_fail(VAP_ERR_INVALID, "W=%d: a route needs at least 2 waypoints", W);
    if (W > kMaxWaypoints) return vap_fail(VAP_ERR_UNSUPPORTED, "W=%d exceeds %d", W, kMaxWaypoints);
    if ((long)R * N > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "%d problems x %d candidates: more than %d routes", R, N, INT_MAX);
    if (R > 0 && (!d_mean || !d_sigma || !d_waypoints)) return vap_fail(VAP_ERR_INVALID, "null mean / sigma / waypoints");
    const uintptr_t pair = dt == VAP_F64 ? 15 : 7;
    if ((((uintptr_t)d_mean | (uintptr_t)d_sigma) & 15) != 0 || (((uintptr_t)d_waypoints | (uintptr_t)d_best_waypoints) & pair) != 0)
        return vap_fail(VAP_ERR_INVALID, "mean and sigma must be 16-byte aligned, the waypoints to a pair of their type");
    VAP_TRY(vap_set_device(ctx));
    if (R == 0) return VAP_OK;

    SampleArgs g{};
    g.R = R;
    g.N = N;
    g.W = W;
    g.total = (size_t)R * (size_t)N * (size_t)W;
    g.mean = d_mean;
    g.sigma = d_sigma;
    g.best_wp = d_best_waypoints;
    g.best_cost = d_best_cost;
    g.seed_lo = (uint32_t)(seed & 0xffffffffull);
    g.seed_hi = (uint32_t)(seed >> 32);
    g.iteration = iteration;
    g.first_problem = first_problem;
    g.out = d_waypoints;
    const size_t grid = (g.total + kSearchSampleThreads - 1) / kSearchSampleThreads;
    if (grid > (size_t)INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "%d x %d x %d waypoints: too many workgroups for one launch", R, N, W);
    if (dt == VAP_F64)
        hipLaunchKernelGGL(k_search_sample<double>, dim3((unsigned)grid), dim3(kSearchSampleThreads), 0, ctx->stream, g);
    else
        hipLaunchKernelGGL(k_search_sample<float>, dim3((unsigned)grid), dim3(kSearchSampleThreads), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

int vap_search_update(vap_ctx *ctx, int dt, int R, int N, int W, const void *d_waypoints, const int *d_counts, int counts_stride,
                      double time_step, const double *d_meta, const uint32_t *d_flags, const double *d_clearance,
                      const double *d_conflict_clearance, const double *d_tracking_worst, const vap_search_weights *weights,
                      int E, double alpha, double sigma_min, double sigma_max, double *d_mean, double *d_sigma, double *d_cost,
                      double *d_violation, int *d_order, int *d_n_feasible, double *d_best_cost, void *d_best_waypoints,
                      double *d_best_terms, double *d_history, int history_stride, uint32_t iteration)
{
    using namespace vap;
    if (dt != VAP_F32 && dt != VAP_F64) return vap_fail(VAP_ERR_INVALID, "bad dtype %d", dt);
    if (R < 0) return vap_fail(VAP_ERR_INVALID, "bad shape R=%d", R);
    if (N < 1 || N > kSearchMaxCandidates) return vap_fail(VAP_ERR_INVALID, "N = %d candidates per problem outside 1..%d", N, kSearchMaxCandidates);
    if (W < 2) return vap_fail(VAP_ERR_INVALID, "W=%d: a route needs at least 2 waypoints", W);
    if (W > kMaxWaypoints) return vap_fail(VAP_ERR_UNSUPPORTED, "W=%d exceeds %d", W, kMaxWaypoints);
    if ((long)R * N > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "%d problems x %d candidates: more than %d routes", R, N, INT_MAX);
    if (!weights) return vap_fail(VAP_ERR_INVALID, "null weights");
    const double nonneg[4] = {weights->w_time, weights->w_length, weights->w_violation, weights->infeasible_base};
    for (double v : nonneg)
        if (!(v >= 0.0) || !std::isfinite(v))
            return vap_fail(VAP_ERR_INVALID, "weights: w_time, w_length, w_violation and infeasible_base must be >= 0 and finite (got %g, %g, %g, %g)",
                            nonneg[0], nonneg[1], nonneg[2], nonneg[3]);
    if (!std::isfinite(weights->clearance_margin) || !std::isfinite(weights->conflict_margin) || !std::isfinite(weights->tracking_tolerance))
        return vap_fail(VAP_ERR_INVALID, "weights: the margins and the tracking tolerance must be finite");
    if (d_counts && (counts_stride < 1 || !(time_step > 0.0) || !std::isfinite(time_step)))
        return vap_fail(VAP_ERR_INVALID, "counts need counts_stride >= 1 and a positive, finite time_step (got %d, %g)", counts_stride, time_step);
    const bool needs_wp = d_mean || d_best_waypoints;
    if (R > 0 && needs_wp && !d_waypoints) return vap_fail(VAP_ERR_INVALID, "null waypoints");
    if (d_mean) {
        if (!d_sigma) return vap_fail(VAP_ERR_INVALID, "a mean needs its sigma");
        if (E < 1 || E > N) return vap_fail(VAP_ERR_INVALID, "E = %d elites outside 1..N = %d", E, N);
        if (!(alpha >= 0.0 && alpha <= 1.0)) return vap_fail(VAP_ERR_INVALID, "alpha %g outside [0, 1]", alpha);
        if (!(sigma_min >= 0.0) || !(sigma_max >= sigma_min)) return vap_fail(VAP_ERR_INVALID, "need 0 <= sigma_min <= sigma_max (got %g, %g)", sigma_min, sigma_max);
    }
    if ((d_best_waypoints || d_best_terms) && !d_best_cost) return vap_fail(VAP_ERR_INVALID, "best waypoints / terms need best_cost");
    if (d_history && (!d_best_cost || history_stride < 1 || iteration >= (uint32_t)history_stride))
        return vap_fail(VAP_ERR_INVALID, "history needs best_cost and iteration %u < history_stride %d", iteration, history_stride);
    VAP_TRY(vap_set_device(ctx));
    if (R == 0) return VAP_OK;

    UpdateArgs g{};
    g.R = R;
    g.N = N;
    g.W = W;
    g.P = 1;
    while (g.P < N) g.P <<= 1;
    g.wp = d_waypoints;
    g.counts = d_counts;
    g.stride = counts_stride;
    g.time_step = time_step;
    g.meta = d_meta;
    g.flags = d_flags;
    g.clearance = d_clearance;
    g.conflict = d_conflict_clearance;
    g.tracking = d_tracking_worst;
    g.w = *weights;
    g.E = E;
    g.alpha = alpha;
    g.sigma_min = sigma_min;
    g.sigma_max = sigma_max;
    g.mean = d_mean;
    g.sigma = d_sigma;
    g.cost = d_cost;
    g.violation = d_violation;
    g.order = d_order;
    g.n_feasible = d_n_feasible;
    g.best_cost = d_best_cost;
    g.best_wp = d_best_waypoints;
    g.best_terms = d_best_terms;
    g.history = d_history;
    g.history_stride = history_stride;
    g.iteration = iteration;
    // a thread per pair of the sort's widest stage, in whole waves: 64 .. 1024
    int threads = g.P / 2 < 64 ? 64 : (g.P / 2 > 1024 ? 1024 : g.P / 2);
    if (dt == VAP_F64)
        hipLaunchKernelGGL(k_search_update<double>, dim3((unsigned)R), dim3(threads), 0, ctx->stream, g);
    else
        hipLaunchKernelGGL(k_search_update<float>, dim3((unsigned)R), dim3(threads), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
