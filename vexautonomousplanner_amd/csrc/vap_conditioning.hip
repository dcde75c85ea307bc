// vap_conditioning.hip — vap_velocity_conditioning: how far a path's velocity recurrence amplifies a relative change of its
// curvature and heading-difference rows, measured with twin sweeps (definition: include/vap.h).
//
//   k_conditioning   one lane per (path, probe).  The G = K + 1 probes of a path are adjacent lanes, so a wave holds 64 / G
//                    paths and the lanes of a group run the same number of steps.  Probe 0 sweeps the rows as they are,
//                    probe k > 0 rows whose curvature and |dtheta| are multiplied by 1 +- delta, the signs from one
//                    Philox4x32-10 block per (sample, probe, path): a probe does not depend on the batch or on how the
//                    host cuts it into launches.  Every sweep is the literal statement of MPG:188-311 in u = v^2 —
//                    sample_limits / forward_step / backward_step of vap_device.h, called as k_velocity_seq<literal> calls
//                    them, so probe 0 is that kernel's row bit for bit.
//                    Forward: a lane writes its squared velocities to scratch, probe-interleaved ([path][sample][probe]),
//                    so a group stores G x 8 contiguous bytes per step.  Backward: lane k takes probe 0's squared velocity
//                    of the sample from the group's first lane by a cross-lane move, forms its relative deviation and keeps
//                    its own running maximum; the per-sample maximum (d_sensitivity) and the final (cond, sample, probe)
//                    are butterfly reductions over the group under a total order, so they do not depend on the schedule.
//                    The rows of step i + 2 are loaded, and the state-independent limits of step i + 1 (sample_limits: its
//                    divisions) computed, while step i's dependent division is in flight.  No atomics, no LDS.
#include <cmath>
#include <cstdint>

#include "vap_device.h"
#include "vap_kernels.h"
#include "vap_philox.h"

namespace vap {

constexpr uint32_t kCondTag = 0x434f4e44u;   // "COND": third word of the Philox counter

struct CondKernelArgs {
    int B, S, b0;                // paths of this launch, row length, first path of the launch within the call
    VelConsts<double> c;
    double start_u, end_u, delta, inv2d, limit;
    uint32_t seed_lo, seed_hi, first_path;
    const double *meta;
    const void *curv, *dth, *vcap, *acc_fwd, *acc_bwd, *acc_dec;   // rows of the whole call, in R
    double *U;                   // scratch [B][S][G]
    double *cond;
    int *worst_sample, *worst_probe;
    uint32_t *flags;
    double *sens, *vel;          // optional [.][S]
};

struct CondStep {
    double k, dt, x, a;          // curvature and |dtheta| of the probe; x: initial velocity (forward) / forward value (backward)
};

template <typename R, int G>
__global__ __launch_bounds__(64) void k_conditioning(CondKernelArgs a)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int pl = t / G, k = t % G;
    if (pl >= a.B) return;       // whole groups leave: G divides 64
    const int b = a.b0 + pl, S = a.S;
    const double *m = a.meta + (size_t)b * kMetaStride;
    const double twodd = 2.0 * m[2];
    int N = (int)m[3];
    N = N < 0 ? 0 : (N > S ? S : N);
    const size_t row = (size_t)b * S;
    const R *K = (const R *)a.curv + row, *DT = (const R *)a.dth + row;
    const R *VC = a.vcap ? (const R *)a.vcap + row : nullptr;
    const R *AF = a.acc_fwd ? (const R *)a.acc_fwd + row : nullptr, *AB = a.acc_bwd ? (const R *)a.acc_bwd + row : nullptr;
    double *U = a.U + (size_t)pl * S * G + k;          // sample j of this probe: U[j * G]
    const VelConsts<double> c = a.c;
    const double vmax2 = c.vmax * c.vmax;
    const uint32_t path = a.first_path + (uint32_t)b;
    const double fp = 1.0 + a.delta, fm = 1.0 - a.delta;
    // the factors of sample j's curvature and |dtheta| in this probe (probe 0: the rows as they are)
    auto factors = [&](int j, double &fk, double &ft) {
        fk = ft = 1.0;
        if (k) {
            const uint4x x = philox4x32_10(uint4x{(uint32_t)j, (uint32_t)k, kCondTag, path}, a.seed_lo, a.seed_hi);
            fk = (x.x & 1u) ? fp : fm;
            ft = (x.y & 1u) ? fp : fm;
        }
    };

    // forward, MPG:188-249
    if (N >= 1) U[0] = a.start_u;
    if (N >= 2) {
        auto load = [&](int j) {                       // what forward step j reads
            CondStep s;
            double fk, ft;
            factors(j, fk, ft);
            s.k = (double)K[j] * fk;
            s.dt = (double)DT[j] * ft;
            s.x = VC ? (double)VC[j + 1] : 0.0;
            s.a = AF ? (double)AF[j] : c.amax;
            return s;
        };
        double u = a.start_u, wprev = 0.0;
        CondStep s1 = load(0), s2 = load(1 < N - 1 ? 1 : N - 2);
        SampleLimits<double> L1 = sample_limits(c, fabs(s1.k), s1.a, AF ? s1.a : c.adec);
        for (int i = 0; i < N - 1; i++) {
            const CondStep s0 = s1;
            const SampleLimits<double> L0 = L1;
            s1 = s2;
            s2 = load(i + 2 < N - 1 ? i + 2 : N - 2);
            L1 = sample_limits(c, fabs(s1.k), s1.a, AF ? s1.a : c.adec);
            const double un = (i + 1 == N - 1) ? a.end_u : (VC ? s0.x * s0.x : vmax2);
            u = forward_step(c, L0, s0.a, twodd, u, wprev, s0.dt, un);
            U[(size_t)(i + 1) * G] = u;
        }
    }

    // backward, MPG:251-311; sample j's squared velocity is final when the sweep arrives there
    double best = 0.0;
    int best_j = -1;
    const int lane0 = (threadIdx.x / G) * G;
    auto arrive = [&](int j, double u) {
        const double u0 = __shfl(u, lane0);
        double r;
        if (u0 > 0.0) r = fabs(u - u0) / u0;
        else if (u0 == 0.0) r = u == 0.0 ? 0.0 : INFINITY;
        else r = NAN;
        if (r > 0.0 && r >= best) {                    // j descends: among equals the smallest sample stays
            best = r;
            best_j = j;
        }
        if (a.sens) {
            double mx = r > 0.0 ? r : 0.0;             // the maximum over the probes from 0.0 under a strict >: a NaN never wins
#pragma unroll
            for (int o = G >> 1; o; o >>= 1) {
                const double ox = __shfl_xor(mx, o);
                mx = ox > mx ? ox : mx;
            }
            if (k == 0) a.sens[row + j] = mx * a.inv2d;
        }
        if (a.vel && k == 0) a.vel[row + j] = vel_sqrt(u);
    };
    if (N >= 1) {
        double u = a.end_u, wprev = 0.0;
        if (N >= 2) {
            const double cur_dec = a.acc_dec ? (double)((const R *)a.acc_dec)[b] : c.adec;
            double fk_at, ft_unused;
            factors(N - 1, fk_at, ft_unused);          // the factor of the curvature the next load reads
            auto load = [&](int j) {                   // what backward step j (>= 1) reads; steps are loaded in descending order
                CondStep s;
                s.k = (double)K[j] * fk_at;
                double ft;
                factors(j - 1, fk_at, ft);
                s.dt = (double)DT[j - 1] * ft;
                s.x = U[(size_t)(j - 1) * G];
                s.a = AB ? (double)AB[j] : c.amax;
                return s;
            };
            CondStep s1 = load(N - 1), s2 = load(N - 2 > 1 ? N - 2 : 1);
            SampleLimits<double> L1 = sample_limits(c, fabs(s1.k), s1.a, cur_dec);
            for (int i = N - 1; i > 0; i--) {
                const CondStep s0 = s1;
                const SampleLimits<double> L0 = L1;
                s1 = s2;
                s2 = load(i - 2 > 1 ? i - 2 : 1);      // (behind step 1 the loads repeat and are not used)
                L1 = sample_limits(c, fabs(s1.k), s1.a, cur_dec);
                arrive(i, u);
                u = backward_step(c, L0, s0.a, twodd, u, wprev, s0.dt, s0.x);
            }
        }
        arrive(0, u);
    }
    for (int j = N + k; j < S; j += G) {
        if (a.sens) a.sens[row + j] = 0.0;
        if (a.vel) a.vel[row + j] = 0.0;
    }

    // (cond, sample, probe): the largest deviation, then the smallest sample, then the smallest probe
    int best_k = best_j >= 0 ? k : -1;
#pragma unroll
    for (int o = G >> 1; o; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(best_j, o), ok = __shfl_xor(best_k, o);
        if (ob > best || (ob == best && (oj < best_j || (oj == best_j && ok < best_k)))) {
            best = ob;
            best_j = oj;
            best_k = ok;
        }
    }
    if (k == 0) {
        const double cond = best * a.inv2d;
        a.cond[b] = cond;
        if (a.worst_sample) a.worst_sample[b] = best_j;
        if (a.worst_probe) a.worst_probe[b] = best_k;
        if (a.flags && cond > a.limit) a.flags[b] |= VAP_FLAG_ILLCONDITIONED_BIT;
    }
}

template <typename R>
static void launch_cond_t(hipStream_t st, int G, const CondKernelArgs &a)
{
    const dim3 grid((unsigned)(((size_t)a.B * G + 63) / 64));
    switch (G) {
        case 2: hipLaunchKernelGGL((k_conditioning<R, 2>), grid, dim3(64), 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_conditioning<R, 4>), grid, dim3(64), 0, st, a); break;
        case 8: hipLaunchKernelGGL((k_conditioning<R, 8>), grid, dim3(64), 0, st, a); break;
        default: hipLaunchKernelGGL((k_conditioning<R, 16>), grid, dim3(64), 0, st, a); break;
    }
}

hipError_t launch_conditioning(hipStream_t st, bool r64, const CondArgs &g, int b0, int nb, double *scratch)
{
    CondKernelArgs a;
    a.B = nb; a.S = g.S; a.b0 = b0;
    a.c = make_consts<double>(g.c);
    a.start_u = g.start_vel * g.start_vel;
    a.end_u = g.end_vel * g.end_vel;
    a.delta = g.delta;
    a.inv2d = 1.0 / (2.0 * g.delta);                    // delta is a power of two: the scaling is exact
    a.limit = g.limit;
    a.seed_lo = (uint32_t)(g.seed & 0xffffffffu);
    a.seed_hi = (uint32_t)(g.seed >> 32);
    a.first_path = g.first_path;
    a.meta = g.meta;
    a.curv = g.curv; a.dth = g.dth; a.vcap = g.vcap;
    a.acc_fwd = g.acc.fwd; a.acc_bwd = g.acc.bwd; a.acc_dec = g.acc.dec;
    a.U = scratch;
    a.cond = g.cond; a.worst_sample = g.worst_sample; a.worst_probe = g.worst_probe; a.flags = g.flags;
    a.sens = g.sens; a.vel = g.vel;
    if (r64) launch_cond_t<double>(st, g.K + 1, a);
    else launch_cond_t<float>(st, g.K + 1, a);
    return hipGetLastError();
}

}  // namespace vap
