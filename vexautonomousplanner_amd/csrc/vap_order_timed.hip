// vap_order_timed.hip — the visiting order of a routine's sites by the clock (vap_plan_order_timed).
//
// Held-Karp over (site set, last site, site before it) in integer rows: what a routine costs is the rows of its timeline,
// and the turn in front of a leg depends on the leg before it, so the state carries the last two sites.  g[S][j][i] is the
// fewest rows of a sequence that starts at point 0, visits exactly the sites of S, stands on j and came from i; slot i = j
// stands for "came from the start" and is finite for S = {j} only.  Every step adds one precomputed int32,
// c3[h][i][j] = turn(hl(h, i), hf(i, j)) + n(i, j) + w(j), saturating at INT_MAX ("none"): the addends are non-negative, so
// saturating step by step gives what a 64-bit sum tested against INT_MAX gives.  Definitions: include/vap.h.
//
//   k_plan_order_timed   persistent workgroups of 256 threads, each taking problems r = block, block + grid, ...
//     prologue   one thread per (a, b): leg index, flag, count, the two end rows' heading, x and y -> n, hf, hl in LDS;
//                one thread per site for the dwell rows and the precedence mask, one per set for value(S).  After a
//                barrier one thread per (h, i, j) computes c3 (one turn_profile each) and one per site the start's c0.
//     table      dynamic LDS: g (2^M M M int32, 64 KiB at M = 8) and a parent byte each (16 KiB), laid out pair-major,
//                g[((j - 1) M + (i - 1)) 2^M + S], k_plan_order's layout.  One sweep per set size with a barrier between
//                the sizes.  A sweep's entries (set, last, previous) are spread over all 256 threads, the set running
//                fastest through a table of the sets ordered by size, so that the lanes of a wave take different sets
//                (a thread per set would leave the full set's 8 * 7 * 6 steps to one thread; in this layout the price is a
//                bank conflict between sets that differ in bits 6, 7 only).  The inner loop is an unsigned add, a min and
//                a compare.
//     selection  every thread scans its set's (j, i) entries under the row limit and keeps the best (value, rows, code),
//                code = S << 8 | j << 4 | i; the key is a total order on distinct entries, so the shuffle reduction over a
//                wave and the four-entry one over the waves give the same winner whatever the schedule.  Thread 0 walks the
//                parents back and writes order, arrivals and totals.  No atomics.
#include <climits>
#include <cmath>
#include <cstdint>

#include "vap_internal.h"
#include "vap_turn.h"

namespace vap {

constexpr int kOtThreads = 256;
constexpr int kOtMaxSites = VAP_PLAN_ORDER_TIMED_MAX_SITES;
constexpr int kOtMaxPoints = kOtMaxSites + 1;
constexpr int kOtMaxBlocks = 1024;
constexpr int kOtRow = 8;   // time, position, velocity, acceleration, heading, angular velocity, x, y

struct OrderTimedArgs {
    int R, M, L, cap, counts_stride, end;
    double dt, turn_min, max_vel, max_acc, track_width;
    const double *rows;             // [L][cap][8]
    const int *counts;              // [L * counts_stride]
    const int *leg;                 // [R][P][P]
    const uint32_t *leg_flags;      // [L] or NULL
    const double *dwell;            // [R][P] or NULL
    const double *start_heading;    // [R] or NULL
    const double *value;            // [R][P] or NULL
    const int *budget;              // [R] or NULL: full mode
    const uint32_t *before;         // [R][P] or NULL
    int *order, *n_visited, *rows_total, *arrival;
    double *value_total;
    uint32_t *flags;
};

__device__ inline int ot_sat(long long v) { return v < (long long)INT_MAX ? (int)v : INT_MAX; }

__device__ inline int ot_binom(int n, int k)    // C(n, k), 0 for n < k; n <= 8
{
    int c = 1;
    for (int i = 1; i <= k; i++) c = c * (n - k + i) / i;
    return c;
}
__device__ inline int ot_nth_bit(unsigned S, int n)   // the position of the n-th lowest set bit of S, n = 0 ..
{
    for (int k = 0; k < n; k++) S &= S - 1;
    return __ffs(S) - 1;
}

// (value, rows, code): a larger value, then fewer rows, then the smaller code wins; rows == INT_MAX is "none"
__device__ inline bool ot_better(double va, int ra, int ca, double vb, int rb, int cb)
{
    if (ra == INT_MAX) return false;
    if (rb == INT_MAX) return true;
    if (va != vb) return va > vb;
    if (ra != rb) return ra < rb;
    return ca < cb;
}

__global__ __launch_bounds__(kOtThreads) void k_plan_order_timed(OrderTimedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ot_lds[];
    __shared__ double s_hf[kOtMaxPoints * kOtMaxPoints], s_hl[kOtMaxPoints * kOtMaxPoints];
    __shared__ double s_val[1 << kOtMaxSites];
    __shared__ double s_red_v[kOtThreads / 64];
    __shared__ int s_red_r[kOtThreads / 64], s_red_c[kOtThreads / 64];
    __shared__ int s_n[kOtMaxPoints * kOtMaxPoints];
    __shared__ int s_c3[kOtMaxPoints * kOtMaxPoints * kOtMaxPoints];
    __shared__ int s_c0[kOtMaxPoints], s_w[kOtMaxPoints];
    __shared__ uint32_t s_before[kOtMaxPoints];
    __shared__ int s_off[kOtMaxSites + 2];
    __shared__ uint8_t s_sets[1 << kOtMaxSites];
    const int tid = threadIdx.x, M = a.M, P = M + 1, nset = 1 << M;
    int *g = reinterpret_cast<int *>(ot_lds);
    uint8_t *par = reinterpret_cast<uint8_t *>(g + (size_t)nset * M * M);
    const double dt = a.dt;
    // the sets ordered by size (within a size by their rank in the combinatorial number system), once per workgroup
    if (tid < nset) {
        int rank = 0, k = 0;
        for (unsigned left = (unsigned)tid; left; left &= left - 1) rank += ot_binom(__ffs(left) - 1, ++k);
        int before = 0;
        for (int sz = 0; sz < k; sz++) before += ot_binom(M, sz);
        s_sets[before + rank] = (uint8_t)tid;
    }
    if (tid <= M + 1) {
        int before = 0;
        for (int sz = 0; sz < tid; sz++) before += ot_binom(M, sz);
        s_off[tid] = before;
    }
    __syncthreads();
#pragma unroll 1
    for (int r = blockIdx.x; r < a.R; r += gridDim.x) {
        const double h0 = a.start_heading ? a.start_heading[r] : NAN;
        const bool bad_start = h0 == h0 && !tl_heading_ok(h0);
        // ---- prologue: the legs' rows and end headings, the dwell rows, the masks, value(S)
        for (int t = tid; t < P * P; t += kOtThreads) {
            const int pa = t / P, pb = t - pa * P;
            int n = 0;
            double hf = 0, hl = 0;
            if (pb != 0 && pa != pb) {
                const int li = a.leg[(size_t)r * P * P + t];
                if (li >= 0 && li < a.L && !(a.leg_flags && a.leg_flags[li] != 0u)) {
                    int cnt = a.counts[(size_t)li * a.counts_stride];
                    cnt = cnt > a.cap ? a.cap : cnt;
                    if (cnt > 0) {
                        const double *f = a.rows + (size_t)li * a.cap * kOtRow;
                        const double *l = f + (size_t)(cnt - 1) * kOtRow;
                        hf = f[4];
                        hl = l[4];
                        if (tl_heading_ok(hf) && tl_finite(f[6]) && tl_finite(f[7]) && tl_heading_ok(hl) && tl_finite(l[6]) &&
                            tl_finite(l[7]))
                            n = cnt;
                    }
                }
            }
            s_n[t] = n; s_hf[t] = hf; s_hl[t] = hl;
        }
        for (int t = tid; t < P; t += kOtThreads) {
            int nd = 0;
            const double w = a.dwell && t > 0 ? a.dwell[(size_t)r * P + t] : 0.0;
            if (w > 0.0) {              // int(dwell / dt), the timeline's
                const double q = w / dt;
                nd = q < (double)INT_MAX ? (int)q : INT_MAX;
            }
            s_w[t] = nd;
            s_before[t] = a.before ? a.before[(size_t)r * P + t] & (uint32_t)(nset - 1) : 0u;
        }
        for (int S = tid; S < nset; S += kOtThreads) {
            double v = 0.0;
            for (unsigned left = S; left; left &= left - 1) {        // ascending j, from 0.0
                const int j = __ffs(left);
                double x = a.value ? a.value[(size_t)r * P + j] : 1.0;
                if (!(x >= 0.0) || x == INFINITY) x = 0.0;           // NaN, negative, infinite: worth nothing
                v = v + x;
            }
            s_val[S] = v;
        }
        __syncthreads();
        // ---- the step costs: c3[h][i][j], h = 0 for the start, and the first step c0[j]
        for (int t = tid; t < P * P * P; t += kOtThreads) {
            const int h = t / (P * P), rem = t - h * P * P, i = rem / P, j = rem - i * P;
            int c = INT_MAX;
            if (i >= 1 && j >= 1 && i != j && h != i && h != j) {
                const int n_in = s_n[h * P + i], n_leg = s_n[i * P + j];
                if (n_in > 0 && n_leg > 0) {
                    const double h_front = s_hl[h * P + i], first_h = s_hf[i * P + j];
                    int n_turn = 0;
                    const double d = tl_wrap_delta(first_h - h_front);
                    if (!(fabs(d) < a.turn_min)) n_turn = turn_profile(-d, a.max_vel, a.max_acc, a.track_width, dt).n;
                    c = ot_sat((long long)n_turn + (long long)n_leg + (long long)s_w[j]);
                }
            }
            s_c3[t] = c;
        }
        for (int j = tid; j < P; j += kOtThreads) {
            int c = INT_MAX;
            const int n_leg = j >= 1 ? s_n[j] : 0;
            if (n_leg > 0 && !bad_start) {
                const double h_front = h0, first_h = s_hf[j];
                int n_turn = 0;
                if (h_front == h_front) {
                    const double d = tl_wrap_delta(first_h - h_front);
                    if (!(fabs(d) < a.turn_min)) n_turn = turn_profile(-d, a.max_vel, a.max_acc, a.track_width, dt).n;
                }
                c = ot_sat((long long)n_turn + (long long)n_leg + (long long)s_w[j]);
            }
            s_c0[j] = c;
        }
        __syncthreads();
        // ---- the table, one sweep per set size
#pragma unroll 1
        for (int size = 1; size <= M; size++) {
            const int first = s_off[size], n_sets = s_off[size + 1] - first, items = n_sets * size * size;
            for (int t = tid; t < items; t += kOtThreads) {          // entry (set, last, previous): the set runs fastest
                const int q = t / n_sets, jpos = q / size, ipos = q - jpos * size;
                const unsigned S = s_sets[first + (t - q * n_sets)];
                const int jb = ot_nth_bit(S, jpos), j = jb + 1, ib = ot_nth_bit(S, ipos), i = ib + 1;
                const unsigned rest = S ^ (1u << jb);
                const bool ok = (s_before[j] & ~rest) == 0;          // everything j waits for has been visited
                int best = INT_MAX, bp = 0;
                if (ib == jb) {                                      // from the start
                    if (size == 1 && ok) best = s_c0[j];
                    bp = j;
                } else if (ok) {
                    const int *crow = s_c3 + i * P + j;
                    for (unsigned lh = rest; lh; lh &= lh - 1) {
                        const int hb = __ffs(lh) - 1;
                        const int hidx = hb == ib ? 0 : hb + 1;
                        const unsigned v = (unsigned)g[(size_t)(ib * M + hb) * nset + rest] + (unsigned)crow[hidx * P * P];
                        const int vi = v < (unsigned)INT_MAX ? (int)v : INT_MAX;
                        if (vi < best) { best = vi; bp = hb + 1; }
                    }
                }
                g[(size_t)(jb * M + ib) * nset + S] = best;
                par[(size_t)(jb * M + ib) * nset + S] = (uint8_t)bp;
            }
            __syncthreads();
        }
        // ---- selection: the best (value, rows, code) under the row limit
        const bool full_mode = a.budget == nullptr;
        int limit = INT_MAX - 1;
        if (!full_mode) {
            const int b = a.budget[r];
            limit = b < 0 ? 0 : (b < limit ? b : limit);
        }
        double bv = 0.0;
        int br = INT_MAX, bc = 0;
        if (tid < nset) {
            const unsigned S = (unsigned)tid;
            if (S == 0u) {
                if (!full_mode && a.end < 1 && !bad_start) br = 0;   // the empty routine
            } else if (!full_mode || S == (unsigned)(nset - 1)) {
                bv = s_val[S];
                for (unsigned left = S; left; left &= left - 1) {
                    const int jb = __ffs(left) - 1;
                    if (a.end >= 1 && jb + 1 != a.end) continue;
                    for (unsigned li = S; li; li &= li - 1) {
                        const int ib = __ffs(li) - 1;
                        const int rows = g[(size_t)(jb * M + ib) * nset + S];
                        if (rows <= limit && rows < br) { br = rows; bc = (int)(S << 8) | (jb + 1) << 4 | (ib + 1); }
                    }
                }
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off);
            const int orr = __shfl_xor(br, off), oc = __shfl_xor(bc, off);
            if (ot_better(ov, orr, oc, bv, br, bc)) { bv = ov; br = orr; bc = oc; }
        }
        if ((tid & 63) == 0) { s_red_v[tid >> 6] = bv; s_red_r[tid >> 6] = br; s_red_c[tid >> 6] = bc; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < kOtThreads / 64; k++)
                if (ot_better(s_red_v[k], s_red_r[k], s_red_c[k], bv, br, bc)) { bv = s_red_v[k]; br = s_red_r[k]; bc = s_red_c[k]; }
            int *order = a.order + (size_t)r * M, *arrival = a.arrival + (size_t)r * M;
            const bool none = br == INT_MAX;
            unsigned S = none ? 0u : (unsigned)bc >> 8;
            int j = (bc >> 4) & 15, i = bc & 15;
            const int k = __popc(S);
            for (int m = M - 1; m >= k; m--) { order[m] = -1; arrival[m] = -1; }
            for (int m = k - 1; m >= 0; m--) {
                const size_t at = (size_t)((j - 1) * M + (i - 1)) * nset + S;
                order[m] = j;
                arrival[m] = g[at] - s_w[j];
                const int p = par[at];
                S ^= 1u << (j - 1);
                j = i;
                i = p;
            }
            a.n_visited[r] = k;
            a.rows_total[r] = none ? -1 : br;
            a.value_total[r] = none ? NAN : bv;
            if (a.flags) a.flags[r] = none ? VAP_ORDER_INFEASIBLE : 0u;
        }
        __syncthreads();                                             // the next problem rewrites the tables
    }
}

}  // namespace vap

extern "C" {

int vap_plan_order_timed(vap_ctx *ctx, int R, int P, int L, int capacity, double time_step, const vap_constraints *c,
                         double turn_min, const double *d_rows, const int *d_counts, int counts_stride, const int *d_leg,
                         const uint32_t *d_leg_flags, const double *d_dwell, const double *d_start_heading, const double *d_value,
                         const int *d_budget_rows, int end, const uint32_t *d_before, int *d_order, int *d_n_visited,
                         int *d_rows_total, int *d_arrival_rows, double *d_value_total, uint32_t *d_flags)
{
    using namespace vap;
    if (R < 0 || P < 2 || L < 0 || capacity < 0 || counts_stride < 1)
        return vap_fail(VAP_ERR_INVALID, "bad shape R=%d P=%d L=%d capacity=%d counts_stride=%d", R, P, L, capacity, counts_stride);
    if (P > kOtMaxPoints) return vap_fail(VAP_ERR_UNSUPPORTED, "P=%d: at most %d sites beside the start", P, kOtMaxSites);
    const int M = P - 1;
    if (end != -1 && (end < 1 || end > M)) return vap_fail(VAP_ERR_INVALID, "end=%d: -1 or a site 1..%d", end, M);
    if (!(time_step > 0) || !std::isfinite(time_step)) return vap_fail(VAP_ERR_INVALID, "time_step must be positive and finite");
    if (!(turn_min >= 0) || !std::isfinite(turn_min)) return vap_fail(VAP_ERR_INVALID, "turn_min must be >= 0 and finite");
    if (!c) return vap_fail(VAP_ERR_INVALID, "null constraints");
    if (!(c->max_vel > 0 && c->max_acc > 0 && c->track_width > 0) || !std::isfinite(c->max_vel) || !std::isfinite(c->max_acc) ||
        !std::isfinite(c->track_width))
        return vap_fail(VAP_ERR_INVALID, "in-place turns need a positive, finite max_vel, max_acc and track_width");
    if (R > 0 && (!d_leg || !d_order || !d_n_visited || !d_rows_total || !d_arrival_rows || !d_value_total))
        return vap_fail(VAP_ERR_INVALID, "null leg / order / n_visited / rows_total / arrival_rows / value_total");
    if (R > 0 && L > 0 && (!d_counts || (!d_rows && capacity > 0))) return vap_fail(VAP_ERR_INVALID, "null rows or counts");
    // the timeline's bound: the longest turn a usable pair of headings can ask for is a full one
    if (!(vap_turn_rows_host(2 * M_PI, c->max_vel, c->max_acc, c->track_width, time_step) <= 1048576.0))
        return vap_fail(VAP_ERR_INVALID, "a turn of more than 2^20 rows at this time step");
    VAP_TRY(vap_set_device(ctx));
    if (R == 0) return VAP_OK;
    const size_t lds = ((size_t)(M * M) << M) * (sizeof(int) + 1);
    if (lds > 64 * 1024) {                                           // above the default limit the runtime has to grant the size
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_plan_order_timed),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return vap_fail(VAP_ERR_UNSUPPORTED, "%d sites need %zu bytes of LDS (%s)", M, lds, hipGetErrorString(e));
    }
    OrderTimedArgs a;
    a.R = R; a.M = M; a.L = L; a.cap = capacity; a.counts_stride = counts_stride; a.end = end;
    a.dt = time_step; a.turn_min = turn_min; a.max_vel = c->max_vel; a.max_acc = c->max_acc; a.track_width = c->track_width;
    a.rows = d_rows; a.counts = d_counts; a.leg = d_leg; a.leg_flags = d_leg_flags; a.dwell = d_dwell;
    a.start_heading = d_start_heading; a.value = d_value; a.budget = d_budget_rows; a.before = d_before;
    a.order = d_order; a.n_visited = d_n_visited; a.rows_total = d_rows_total; a.arrival = d_arrival_rows;
    a.value_total = d_value_total; a.flags = d_flags;
    const int blocks = R < kOtMaxBlocks ? R : kOtMaxBlocks;
    hipLaunchKernelGGL(k_plan_order_timed, dim3((unsigned)blocks), dim3(kOtThreads), lds, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
