// vap_order.hip — the cheapest visiting order of a routine's sites from a cost matrix (vap_plan_order).
//
// Held-Karp over site sets.  Point 0 is where the routine starts, points 1 .. M are the sites (M <= 10); f[S][j] is the
// cheapest way to start at 0, visit exactly the sites of S and stand on j, built by one IEEE addition per predecessor in
// increasing predecessor order under a strict <, so the result does not depend on the order of the work.  Definitions:
// include/vap.h.
//
//   k_plan_order  persistent workgroups of 256 threads, each taking problems r = block, block + grid, ...  Dynamic LDS
//                 holds f (2^M x M doubles, 80 KB at M = 10) and the parents, a byte each (10 KB).  The table is laid out
//                 site-major, f[(j - 1) 2^M + S]: a thread takes set S = its lane's index (+ 256, ...), so the lanes of a
//                 wave read f[i][S \ {j}] at consecutive 8-byte words for every (i, j) of the inner loops — the b64 pattern
//                 of k_plan_seeds' relaxation, without bank conflicts.  One sweep per set size: a thread whose set has
//                 another size skips it, and a barrier separates the sizes.  The sanitised costs (121 doubles) and the
//                 precedence masks sit in static LDS and are read at wave-uniform or near-uniform addresses.  The walk back
//                 over the parents is M steps on one lane.  Integer work beside one addition and one comparison per
//                 (set, site, predecessor); no atomics.
#include <cmath>
#include <cstdint>

#include "vap_internal.h"

namespace vap {

constexpr int kOrderThreads = 256;
constexpr int kOrderMaxSites = VAP_PLAN_ORDER_MAX_SITES;
constexpr int kOrderMaxPoints = kOrderMaxSites + 1;
constexpr int kOrderMaxBlocks = 1024;

struct OrderArgs {
    int R, M, end;
    const double *cost;         // [R][P][P], P = M + 1
    const uint32_t *before;     // [R][P] or NULL
    int *order;                 // [R][M]
    double *total;              // [R]
    uint32_t *flags;            // [R] or NULL
};

__global__ __launch_bounds__(kOrderThreads) void k_plan_order(OrderArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char order_lds[];
    __shared__ double s_c[kOrderMaxPoints * kOrderMaxPoints];
    __shared__ uint32_t s_before[kOrderMaxPoints];
    const int tid = threadIdx.x, M = a.M, P = M + 1, nset = 1 << M;
    double *f = reinterpret_cast<double *>(order_lds);
    uint8_t *par = reinterpret_cast<uint8_t *>(f + (size_t)nset * M);
#pragma unroll 1
    for (int r = blockIdx.x; r < a.R; r += gridDim.x) {
        for (int t = tid; t < P * P; t += kOrderThreads) {
            const double v = a.cost[(size_t)r * P * P + t];
            s_c[t] = (v != v || v == -INFINITY) ? INFINITY : v;      // NaN and -inf forbid the leg
        }
        for (int t = tid; t < P; t += kOrderThreads) s_before[t] = a.before ? a.before[(size_t)r * P + t] & (uint32_t)(nset - 1) : 0u;
        __syncthreads();
#pragma unroll 1
        for (int size = 1; size <= M; size++) {
            for (int S = tid; S < nset; S += kOrderThreads) {
                if (__popc(S) != size) continue;
                for (unsigned left = S; left; left &= left - 1) {
                    const int jb = __ffs(left) - 1, j = jb + 1;
                    const unsigned rest = (unsigned)S ^ (1u << jb);
                    double best = INFINITY;
                    int bp = 0;
                    if ((s_before[j] & ~rest) == 0) {                // everything j waits for has been visited
                        if (size == 1) {
                            best = s_c[j];                           // c[0][j]
                        } else {
                            for (unsigned li = rest; li; li &= li - 1) {
                                const int ib = __ffs(li) - 1;
                                const double v = f[(size_t)ib * nset + rest] + s_c[(ib + 1) * P + j];
                                if (v < best) { best = v; bp = ib + 1; }
                            }
                        }
                    }
                    f[(size_t)jb * nset + S] = best;
                    par[(size_t)jb * nset + S] = (uint8_t)bp;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int full = nset - 1;
            int last = a.end;
            if (last < 0) {                                          // the smallest total, the lowest site on a tie
                last = 1;
                for (int j = 2; j <= M; j++)
                    if (f[(size_t)(j - 1) * nset + full] < f[(size_t)(last - 1) * nset + full]) last = j;
            }
            const double total = f[(size_t)(last - 1) * nset + full];
            int *order = a.order + (size_t)r * M;
            if (total == INFINITY) {
                for (int k = 0; k < M; k++) order[k] = -1;
            } else {
                int S = full, j = last;
                for (int k = M - 1; k >= 0; k--) {
                    order[k] = j;
                    const int p = par[(size_t)(j - 1) * nset + S];
                    S ^= 1 << (j - 1);
                    j = p;
                }
            }
            a.total[r] = total;
            if (a.flags) a.flags[r] = total == INFINITY ? VAP_ORDER_INFEASIBLE : 0u;
        }
        __syncthreads();                                             // the next problem rewrites the costs and the table
    }
}

}  // namespace vap

extern "C" {

int vap_plan_order(vap_ctx *ctx, int R, int P, const double *d_cost, int end, const uint32_t *d_before, int *d_order, double *d_total,
                   uint32_t *d_flags)
{
    using namespace vap;
    if (R < 0 || P < 2) return vap_fail(VAP_ERR_INVALID, "bad shape R=%d P=%d", R, P);
    if (P > kOrderMaxPoints) return vap_fail(VAP_ERR_UNSUPPORTED, "P=%d: at most %d sites beside the start", P, kOrderMaxSites);
    const int M = P - 1;
    if (end != -1 && (end < 1 || end > M)) return vap_fail(VAP_ERR_INVALID, "end=%d: -1 or a site 1..%d", end, M);
    if (R > 0 && (!d_cost || !d_order || !d_total)) return vap_fail(VAP_ERR_INVALID, "null cost / order / total");
    VAP_TRY(vap_set_device(ctx));
    if (R == 0) return VAP_OK;
    const size_t lds = ((size_t)M << M) * (sizeof(double) + 1);
    if (lds > 64 * 1024) {                                           // above the default limit the runtime has to grant the size
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_plan_order), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return vap_fail(VAP_ERR_UNSUPPORTED, "%d sites need %zu bytes of LDS (%s)", M, lds, hipGetErrorString(e));
    }
    OrderArgs a{R, M, end, d_cost, d_before, d_order, d_total, d_flags};
    const int blocks = R < kOrderMaxBlocks ? R : kOrderMaxBlocks;
    hipLaunchKernelGGL(k_plan_order, dim3((unsigned)blocks), dim3(kOrderThreads), lds, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
