// vap_velocity_seq.hip — K5a, the sequential velocity sweep (gfx950 / CDNA4).
// ------------------------------------------------------------------------------------------------
// K5a: forward/backward velocity pass, one lane per path, strictly sequential — MPG:188-311 in
// squared-velocity space.  FAST = false is the literal statement (every min/max of the reference);
// FAST = true uses the collapsed limits of vap_device.h and is bit-identical to the relaxation
// kernel (vap_velocity_relax.hip), which makes it the in-library check of that kernel.
// ------------------------------------------------------------------------------------------------
#include "vap_device.h"
#include "vap_kernels.h"

#include <type_traits>

namespace vap {

// Per-sample max_acceleration for routes whose nodes / action points change it (all NULL: the constraints'):
//   fwd [B][S]  max_acc (= max_dec) in force for the forward step FROM sample i     MPG:194-196
//   bwd [B][S]  max_acc the backward sweep has in force for its step FROM sample i  MPG:256-257
//   dec [B]     max_dec of the whole backward sweep (what the forward sweep left)
// (AccRows<R>: vap_device.h)

// R = arithmetic type (and type of the curvature / dtheta rows), IO = type of the caller's rows (initial
// velocities, max_acceleration rows, the velocity output): IO = float with R = double is the fp64 recurrence
// behind fp32 outputs.
template <typename R, typename IO, bool FAST>
__global__ __launch_bounds__(64) void k_velocity_seq(int B, int S, VelConsts<R> c, R start_u, R end_u,
                                                     const double *__restrict__ meta,
                                                     const R *__restrict__ curv, const R *__restrict__ dtheta,
                                                     const R *__restrict__ vcap, AccRows<R> acc, IO *__restrict__ vel,
                                                     R *__restrict__ usq)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *m = meta + (size_t)b * kMetaStride;
    const R twodd = (R)2 * (R)m[2];
    const int N = (int)m[3];
    const size_t row = (size_t)b * S;
    const R *K = curv + row, *DT = dtheta + row;
    // the sweeps run on squared velocities in the arithmetic type: in place when the output row has that type,
    // otherwise in the scratch row `usq`
    R *V;
    if constexpr (std::is_same<R, IO>::value) V = vel + row;
    else V = usq + row;
    const R vmax2 = c.vmax * c.vmax;
    const FastConsts<R> fc = make_fast(c, twodd);
    // same per-path decision as the relaxation kernel: does any step have a zero heading difference?
    bool dup = false;
    if constexpr (FAST) {
        for (int i = 0; i < N - 1; i++) {
            const R kabs = (R)fabs(K[i]);
            dup |= fast_gq(fast_gg(fc, DT[i]), kabs * kabs) < (R)0;
        }
    }
    // Both sweeps read the rows of step i + 1 while step i is computed (a lane waits a memory round trip per step
    // otherwise: the chain of a step is a few hundred cycles, a load from L2 about as long again).
    // forward, MPG:188-249
    R u = start_u, wprev = (R)0;   // FAST: wprev carries the previous squared velocity instead
    V[0] = u;
    auto load_fwd = [&](int j, R &k, R &dt, R &cap, R &a) {      // what forward step j reads
        k = K[j];
        dt = DT[j];
        cap = vcap ? (R)vcap[row + j + 1] : (R)0;
        a = acc.fwd ? (R)acc.fwd[row + j] : c.amax;
    };
    R k1 = (R)0, d1 = (R)0, c1 = (R)0, a1 = c.amax, kprev = (R)0;
    if (N > 1) load_fwd(0, k1, d1, c1, a1);
    for (int i = 0; i < N - 1; i++) {
        const R k0 = k1, d0 = d1, c0 = c1, cur = a1;
        load_fwd(i + 1 < N - 1 ? i + 1 : i, k1, d1, c1, a1);
        const R un = (i + 1 == N - 1) ? end_u : (vcap ? c0 * c0 : vmax2);
        // MPG:194-196: max_acc = max_dec = the value in force from the last boundary at or before sample i (`cur`)
        if constexpr (FAST) {
            R rho, gq, A, cap;
            const R amaxp = acc.fwd ? twodd * cur : fc.amaxp;
            fast_derive(fc, (R)fabs(k0), i > 0 ? (R)fabs(kprev) : (R)0, d0, amaxp, rho, gq, A, cap);
            if (acc.fwd) A = fast_cap_A(fc, (R)fabs(k0), A);
            R am, g;
            fast_scale(amaxp, gq, A, am, g);
            u = fast_forward_a(am, rho, g, A, cap, u, wprev, un);
        } else {
            const SampleLimits<R> L = sample_limits(c, (R)fabs(k0), cur, acc.fwd ? cur : c.adec);
            u = forward_step(c, L, cur, twodd, u, wprev, d0, un);
        }
        kprev = k0;
        V[i + 1] = u;
    }
    // backward, MPG:251-311
    u = end_u;
    wprev = (R)0;
    // MPG:256-257: max_acc as the backward sweep finds it at sample i; max_dec is what the forward sweep left
    const R cur_dec = acc.dec ? (R)acc.dec[b] : c.adec;
    auto load_bwd = [&](int j, R &k, R &dt, R &vf, R &a) {      // what backward step j (>= 1) reads
        k = K[j];
        dt = DT[j - 1];
        vf = V[j - 1];
        a = acc.bwd ? (R)acc.bwd[row + j] : c.amax;
    };
    R v1 = (R)0, knext = (R)0;
    if (N > 1) load_bwd(N - 1, k1, d1, v1, a1);
    for (int i = N - 1; i > 0; i--) {
        R up;
        const R k0 = k1, d0 = d1, vf = v1, cur_acc = a1;
        load_bwd(i - 1 > 0 ? i - 1 : i, k1, d1, v1, a1);
        if constexpr (FAST) {
            R rho, gq, A, cap;
            const R kabs = (R)fabs(k0);
            fast_derive(fc, kabs, i + 1 <= N - 1 ? (R)fabs(knext) : (R)0, d0, acc.bwd ? twodd * cur_dec : fc.adecp, rho, gq, A, cap);
            if (acc.bwd) A = fast_cap_A(fc, kabs, A);
            // a straight sample is limited by max_dec alone (MPG:270-272), and so is a sample with a zero heading
            // difference whose angular velocity does not rise (the wheel limit is then +inf, MPG:52-59)
            // (amaxp = A there: the clamp decides, and kHuge times any non-zero rise of the angular velocity still wins)
            const R amaxp = acc.bwd ? ((kabs < (R)1e-6 || gq < (R)0) ? A : twodd * cur_acc) : fc.amaxp;
            R am, g;
            fast_scale(amaxp, gq, A, am, g);
            up = dup ? fast_backward_a<true>(am, rho, g, A, cap, u, wprev, vf)
                     : fast_backward_a<false>(am, rho, g, A, cap, u, wprev, vf);
        } else {
            const SampleLimits<R> L = sample_limits(c, (R)fabs(k0), cur_acc, cur_dec);
            up = backward_step(c, L, cur_acc, twodd, u, wprev, d0, vf);
        }
        knext = k0;
        // (R != IO: V[i] — the scratch row, the forward value of sample i — is dead from here on and receives the
        // velocity in the arithmetic type: the fp64 row the time-domain resample integrates behind fp32 rows)
        const R vv = vel_sqrt(u);
        vel[row + i] = (IO)vv;
        if constexpr (!std::is_same<R, IO>::value) V[i] = vv;
        u = up;
    }
    {
        const R vv = vel_sqrt(u);
        vel[row] = (IO)vv;
        if constexpr (!std::is_same<R, IO>::value) V[0] = vv;
    }
    for (int i = N; i < S; i++) {
        vel[row + i] = (IO)0;
        if constexpr (!std::is_same<R, IO>::value) V[i] = (R)0;
    }
}

template <typename R, typename IO>
static void launch_seq_t(hipStream_t st, bool fast, int B, int S, const double c[6], double sv, double ev, const double *meta,
                         const void *curv, const void *dth, const void *vcap, const AccRowsV &accv, void *vel, void *usq)
{
    const dim3 grid((B + 63) / 64);
    const AccRows<R> acc = acc_rows<R>(accv);
    const R s = (R)sv, e = (R)ev;
    auto k = fast ? k_velocity_seq<R, IO, true> : k_velocity_seq<R, IO, false>;
    hipLaunchKernelGGL(k, grid, dim3(64), 0, st, B, S, make_consts<R>(c), s * s, e * e, meta, (const R *)curv,
                       (const R *)dth, (const R *)vcap, acc, (IO *)vel, (R *)usq);
}

// r64: arithmetic (and curvature / dtheta rows) in fp64; io64: the caller's rows (vcap, acc, vel) are fp64.
// usq: [B][S] scratch of the arithmetic type, needed when the two differ.
hipError_t launch_velocity_seq(hipStream_t st, bool r64, bool io64, bool fast, int B, int S, const double c[6], double sv,
                               double ev, const double *meta, const void *curv, const void *dth, const void *vcap,
                               const AccRowsV &accv, void *vel, void *usq)
{
    if (r64 && io64) launch_seq_t<double, double>(st, fast, B, S, c, sv, ev, meta, curv, dth, vcap, accv, vel, usq);
    else if (r64) launch_seq_t<double, float>(st, fast, B, S, c, sv, ev, meta, curv, dth, vcap, accv, vel, usq);
    else launch_seq_t<float, float>(st, fast, B, S, c, sv, ev, meta, curv, dth, vcap, accv, vel, usq);
    return hipGetLastError();
}

}  // namespace vap
