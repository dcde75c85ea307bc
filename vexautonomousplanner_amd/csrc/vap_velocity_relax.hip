// vap_velocity_relax.hip — K5b, K5c and K5c': the relaxation kernels, register-resident and two-level (gfx950 / CDNA4).
// ------------------------------------------------------------------------------------------------
// K5b: velocity pass by speculative chunk relaxation.  One workgroup per path; thread c owns the L
// consecutive samples [c*L, c*L+L) and keeps their step coefficients (rho, g*k^2, A, cap — vap_device.h)
// and squared velocities in registers.  The recurrence is sequential only through the 2-word state
// (u_i, u_{i-1}) that crosses a chunk boundary, so a thread whose incoming state changed re-runs its L
// steps from that state and hands its outgoing state on; a thread whose incoming state is bit-identical
// to the one it last used is already final.  Chunk 0's incoming state is exact, so by induction chunk c
// is exact after at most c+1 evaluations, and the fixed point (no state changed) is bit-identical to
// the sequential sweep.  Two trajectories started from different states merge (bitwise) after ~240
// samples on average, so config 3 needs ~29 + 23 evaluations by the busiest wavefront, not 250
// (DESIGN.md §5, K5).
// States move lane to lane by DPP inside a wavefront and through a 2-word LDS record per wavefront
// across wavefronts, one workgroup barrier per 8 evaluations.  HBM traffic: one read of (curvature,
// dtheta) per sweep direction and the final velocity store.
// ------------------------------------------------------------------------------------------------
// K5b and K5c / K5c' are one translation unit on purpose.  They share the helpers below and the `smem_raw` symbol
// of their dynamic LDS, and the compiler's code for ten k_velocity_long instantiations is not the same once
// k_velocity_relax is compiled elsewhere (device assembly compared kernel by kernel with both layouts).
#include "vap_device.h"
#include "vap_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace vap {

template <typename R> struct BitsOf;
template <> struct BitsOf<float> { using type = uint32_t; };
template <> struct BitsOf<double> { using type = uint64_t; };
template <typename R>
__device__ __forceinline__ bool same_bits(R a, R b)
{
    using U = typename BitsOf<R>::type;
    return __builtin_bit_cast(U, a) == __builtin_bit_cast(U, b);
}

// Cooperative, fully coalesced copy of one row (n elements) between HBM and the padded LDS stage:
// element i lives at stage[i + i / L], so thread c's chunk [c*L, c*L+L) is read with lane stride
// L+1 words (odd => no bank conflicts) while HBM sees 16 bytes per lane.
template <typename R, int L>
__device__ __forceinline__ int stage_pos(int i) { return i + i / L; }

// One thread's share of a row on its way from HBM to the stage.  Fetch and put are separate so that a
// row's loads can be in flight while the previous row is being consumed.
template <typename R, int L>
struct RowRegs {
    static constexpr int V = 16 / sizeof(R);
    static constexpr int ITER = (L + V - 1) / V + 1;   // covers cap_n <= T*L + V elements
    using VT = typename std::conditional<sizeof(R) == 4, float4, double2>::type;
    VT v[ITER];      // rows that start 16-byte aligned: 16 bytes per lane
    R s[L + 1];      // other rows: one element per lane
};

template <typename R, int L>
__device__ __forceinline__ void row_fetch(RowRegs<R, L> &r, const R *__restrict__ src, int n, bool aligned, int tid, int T)
{
    using RR = RowRegs<R, L>;
    constexpr int V = RR::V;
    if (aligned) {
        const typename RR::VT *src4 = reinterpret_cast<const typename RR::VT *>(src);
        // all loads first (independent, so the memory latency is paid once); the one group that straddles
        // the end of the row is assembled element by element, zero-padded
#pragma unroll
        for (int it = 0; it < RR::ITER; it++) {
            const int i = tid + it * T;
            if ((i + 1) * V <= n) {
                r.v[it] = src4[i];
            } else {
                R *e = reinterpret_cast<R *>(&r.v[it]);
#pragma unroll
                for (int k = 0; k < V; k++) e[k] = (i * V + k < n) ? src[i * V + k] : (R)0;
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < L + 1; it++) {
            const int i = tid + it * T;
            r.s[it] = i < n ? src[i] : (R)0;
        }
    }
}

template <typename R, int L>
__device__ __forceinline__ void stage_put(R *__restrict__ stage, const RowRegs<R, L> &r, int cap_n, bool aligned, int tid, int T)
{
    using RR = RowRegs<R, L>;
    constexpr int V = RR::V;
    if (aligned) {
#pragma unroll
        for (int it = 0; it < RR::ITER; it++) {
            const int i = tid + it * T;
            const R *e = reinterpret_cast<const R *>(&r.v[it]);
            if (i * V < cap_n) {   // the stage has room for a whole group past cap_n (T*L + T + 8 words)
                const int p0 = stage_pos<R, L>(i * V);
#pragma unroll
                for (int k = 0; k < V; k++)   // L % V == 0: the V elements share a chunk
                    stage[(L % V == 0) ? p0 + k : stage_pos<R, L>(i * V + k)] = e[k];
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < L + 1; it++) {
            const int i = tid + it * T;
            if (i < cap_n) stage[stage_pos<R, L>(i)] = r.s[it];
        }
    }
}

template <typename R, int L>
__device__ __forceinline__ void stage_load(R *__restrict__ stage, const R *__restrict__ src, int n, int cap_n,
                                           bool aligned, int tid, int T)
{
    RowRegs<R, L> r;
    row_fetch<R, L>(r, src, n, aligned, tid, T);
    stage_put<R, L>(stage, r, cap_n, aligned, tid, T);
}

// Boundary state of the recurrence between two chunks: the last two squared velocities.
template <typename R>
struct alignas(2 * sizeof(R)) BoundaryState {
    R u, w;
};

// Whole-wave lane shifts by DPP (no LDS round trip): lane i receives lane i-1 (up) / i+1 (down);
// lane 0 (up) / lane 63 (down) keep their own value.
__device__ __forceinline__ float wave_shift_up(float x)
{
    const int v = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shift_down(float x)
{
    const int v = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ double wave_shift_up(double x)
{
    const uint64_t v = __builtin_bit_cast(uint64_t, x);
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t l2 = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    const uint32_t h2 = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((uint64_t)h2 << 32) | l2);
}
__device__ __forceinline__ double wave_shift_down(double x)
{
    const uint64_t v = __builtin_bit_cast(uint64_t, x);
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t l2 = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xf, 0xf, false);
    const uint32_t h2 = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((uint64_t)h2 << 32) | l2);
}

// VCAP: the caller gave per-sample initial velocities (MPG:121,127,153,172: node / action-point max_velocity and
// stops); the forward step into sample j is then also limited by vcap[j]^2 — folded into that slot's cap.
// R = arithmetic type and type of the curvature / dtheta rows; IO = type of the caller's rows (vcap, acc, vel).
// backward step of either form: FOLDED = the forward value of the sample is already folded into cap (commit mode)
template <bool DUP, bool FOLDED>
__device__ __forceinline__ float bwd_step(float am, float rho, float g, float A, float cap, float u, float &uprev, float u_prev)
{
    return fast_backward_a<DUP>(am, rho, g, A, cap, u, uprev, FOLDED ? Huge<float>::v : u_prev);   // (one v_min3 either way)
}
template <bool DUP, bool FOLDED>
__device__ __forceinline__ double bwd_step(double am, double rho, double g, double A, double cap, double u, double &uprev, double u_prev)
{
    return fast_backward_a<DUP, !FOLDED>(am, rho, g, A, cap, u, uprev, u_prev);
}

template <typename R, typename IO, int L, int MAXT, int MINW, bool VCAP, bool ACC>
__global__ __launch_bounds__(MAXT, MINW) void k_velocity_relax(int S, VelConsts<R> c, R start_u, R end_u,
                                                               const double *__restrict__ meta,
                                                               const R *__restrict__ curv,
                                                               const R *__restrict__ dtheta,
                                                               const R *__restrict__ vcap, AccRows<R> acc,
                                                               IO *__restrict__ vel, uint32_t *__restrict__ flags,
                                                               long long *__restrict__ stats, R *__restrict__ vhi)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    R *stage = reinterpret_cast<R *>(smem_raw);   // (T*L + T + 2) elements
    // boundary states, double-buffered by round parity so one barrier per round suffices
    __shared__ BoundaryState<R> s_bs[2][MAXT / 64 + 2];   // states crossing a wavefront boundary
    __shared__ int s_any[3];   // "some chunk's incoming state changed" per round, rotating slots
    __shared__ int s_dup;
    const long long t_start = stats ? __builtin_amdgcn_s_memtime() : 0;
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const double *m = meta + (size_t)b * kMetaStride;
    const R twodd = (R)2 * (R)m[2];
    const int N = (int)m[3];
    const size_t row = (size_t)b * S;
    const R *K = curv + row, *DT = dtheta + row;
    const FastConsts<R> fc = make_fast(c, twodd);
    const R adecp_b = ACC ? twodd * (R)acc.dec[b] : fc.adecp;   // ACC: the backward sweep's max_dec (AccRows)
    const int lo = tid * L;
    const int TL = T * L;
    const bool aligned = (S % (16 / (int)sizeof(R))) == 0;
    // the step's `am` (fast_scale, vap_device.h) per slot: fp32 only for routes whose nodes change max_acceleration
    // (ACC), the scaled fp64 step always
    constexpr bool PSA = ACC || ScaledStep<R>::value;
    // CM ("commit mode", the fp64 instantiations — registers): no array of squared velocities.  The forward rounds
    // only move boundary states and one commit evaluation writes the forward result over cp[] (the cap is dead by
    // then); the backward sweep folds it into its own cap, min(cap, forward value), and commits into cp[] again.
    constexpr bool CM = ScaledStep<R>::value;
    R q[L], g[L], A[L], cp[L], u[CM ? 1 : L];
    R am[PSA ? L : 1];
    if (tid == 0) { s_any[0] = 0; s_any[1] = 0; s_any[2] = 0; s_dup = 0; }

    // ---------------- forward sweep: the step (j-1 -> j) into owned sample j uses k[j-1], dth[j-1]
    // (and k[j-2] for rho).  q[] holds rho, g[] holds g*k^2 (vap_device.h) once both rows are consumed.
    // Stage positions of this thread's window: sample lo + k sits at cbase + k for 0 <= k < L, one word
    // further for the next chunk's samples and one word nearer for the previous chunk's.
    const int cbase = tid * (L + 1);
    auto cpos = [&](int k) { return k < 0 ? cbase + k - 1 : (k < L ? cbase + k : cbase + k + 1); };
    // rows are read up to the capacity S, not the sample count N (samples past N hold zeros): the loads
    // then do not wait for the meta record
    stage_load<R, L>(stage, K, S < TL ? S : TL, TL, aligned, tid, T);
    RowRegs<R, L> rd;   // the dtheta row is fetched while the curvature row is consumed
    row_fetch<R, L>(rd, DT, S < TL ? S : TL, aligned, tid, T);
    __syncthreads();
    // Samples are handled BK at a time: BK unconditional LDS reads in one batch (one wait), then
    // straight-line arithmetic, one sample after the other (the opaque() keeps the scheduler from
    // interleaving all L of them, which costs registers the rounds need).
    constexpr int BK = (L % 8 == 0) ? 8 : ((L % 5 == 0) ? 5 : 4);
    {
        // k[lo-2], k[lo-1] first (tid 0 has no previous chunk: clamped to word 0 and masked)
        R kp = (R)fabs(stage[(lo >= 2) ? cpos(-2) : 0]);
        R kc = (R)fabs(stage[(lo >= 1) ? cpos(-1) : 0]);
#pragma unroll
        for (int s0 = 0; s0 < L; s0 += BK) {
            R kn[BK];
#pragma unroll
            for (int i = 0; i < BK; i++) kn[i] = (R)fabs(stage[cpos(s0 + i)]);
#pragma unroll
            for (int i = 0; i < BK; i++) {
                const int s = s0 + i, j = lo + s;
                const bool valid = j >= 1 && j <= N - 1;
                R base = fc.amaxp;
                if constexpr (ACC) {   // the step into j starts at sample j-1: its max_acc (= max_dec), MPG:194-196
                    base = valid ? twodd * (R)acc.fwd[row + j - 1] : fc.amaxp;
                    am[s] = base;
                }
                fast_derive_k(fc, kc, (j >= 2) ? kp : (R)0, base, q[s], g[s], A[s], cp[s]);   // g[s] = k^2 for now
                if constexpr (ACC) A[s] = fast_cap_A(fc, kc, A[s]);
                if (!valid) idle_coef(q[s], g[s], A[s], cp[s]);
                q[s] = opaque(q[s]);
                kp = kc;
                kc = kn[i];
            }
        }
    }
    __syncthreads();
    stage_put<R, L>(stage, rd, TL, aligned, tid, T);
    __syncthreads();
    bool dup = false;
#pragma unroll
    for (int s0 = 0; s0 < L; s0 += BK) {
        R dn[BK];
#pragma unroll
        for (int i = 0; i < BK; i++) dn[i] = stage[(lo + s0 + i >= 1) ? cpos(s0 + i - 1) : 0];
#pragma unroll
        for (int i = 0; i < BK; i++) {
            const int s = s0 + i, j = lo + s;
            const bool valid = j >= 1 && j <= N - 1;
            const R gq = fast_gq(fast_gg(fc, dn[i]), g[s]);
            R amv, gv;
            fast_scale(ACC ? am[ACC ? s : 0] : fc.amaxp, valid ? gq : (R)0, A[s], amv, gv);
            g[s] = opaque(gv);
            if constexpr (PSA) am[s] = amv;
            dup |= g[s] < (R)0;
            if constexpr (!CM) u[s] = start_u;
        }
    }
    if constexpr (VCAP) {
        // the forward step into sample j (1 <= j <= N-2; the end sample is fixed by the backward sweep) also
        // honours the sample's initial velocity: min(.., cap, vcap^2) — one number per slot
        const R *VC = vcap + row;
#pragma unroll
        for (int s0 = 0; s0 < L; s0 += BK) {    // BK loads in flight, then BK selects (as the phases above)
            R vc[BK];
#pragma unroll
            for (int i = 0; i < BK; i++) {
                const int j = lo + s0 + i;
                vc[i] = (j >= 1 && j <= N - 2) ? (R)VC[j] : Huge<R>::v * (R)1e-20;   // (squares without overflow)
            }
#pragma unroll
            for (int i = 0; i < BK; i++) cp[s0 + i] = opaque(vmin(cp[s0 + i], vc[i] * vc[i]));
        }
    }
    // boundary state = the last two squared velocities (u, u_prev)
    R in_u, in_w;
    if (tid == 0) { in_u = start_u; in_w = (R)0; }
    else { in_u = cp[0]; in_w = in_u; }
    const bool fwd_active = lo <= N - 1;       // the chunk holds at least one real sample
    bool need = fwd_active;
    R out_u = in_u, out_w = in_w;
    int rounds = 0;
    if (dup) s_dup = 1;
    __syncthreads();
    const bool any_dup = s_dup != 0;
    const long long t_fwd0 = stats ? __builtin_amdgcn_s_memtime() : 0;
    // A round: up to kInner times { lanes whose incoming state changed re-run their chunk; the outgoing
    // states move one lane up inside each wavefront by DPP }, then the states that cross a wavefront
    // boundary go through LDS (buffer r&1) behind one workgroup barrier, picked up together with the
    // "someone still has work" flag of round r-1.  The flags rotate over three slots (this round's, the
    // next one's being cleared, the previous one's being read), so termination lags one cheap round and
    // needs no second barrier.  Chains are ~6 chunks long on average: most end inside one round.
    constexpr int kInner = 8;
    const int wv = tid >> 6, lane = tid & 63;
    int f_cur = 0, f_nxt = 1, f_prv = 2;
    const bool fwd_nb = lane > 0 && fwd_active;
    while (true) {
        if constexpr (CM) {
            // Commit mode keeps no per-sample result, so re-running a chunk whose incoming state has not changed is
            // harmless: the whole wavefront evaluates whenever any of its lanes has to (no per-lane branch, no exec
            // bookkeeping between an evaluation and the next — ~35 instructions on the chain of a ramp otherwise), and
            // the loop is left on the ballot of the lanes whose incoming state moved.
            if (__ballot(need) != 0) {
#pragma unroll 1
                for (int k = 0; k < kInner; k++) {
                    R uu = in_u, wp = in_w;
#pragma unroll
                    for (int s = 0; s < L; s++) {
                        const R nx = step_fwd(am[PSA ? s : 0], q[s], g[s], A[s], cp[s], uu, wp);
                        if (s == 0) {   // sample 0 is the given start velocity (MPG:189): thread 0 skips its first slot
                            const R w1 = wp;               // (step_fwd has moved uu into wp)
                            wp = tid == 0 ? in_w : w1;
                            uu = tid == 0 ? in_u : nx;
                        } else {
                            uu = nx;
                        }
                    }
                    out_u = uu;
                    out_w = wp;
                    const R nu = wave_shift_up(out_u), nw = wave_shift_up(out_w);
                    need = fwd_nb && !(same_bits(nu, in_u) && same_bits(nw, in_w));
                    in_u = fwd_nb ? nu : in_u;
                    in_w = fwd_nb ? nw : in_w;
                    if (__ballot(need) == 0) break;
                }
            }
        } else {
#pragma unroll 1
        for (int k = 0; k < kInner; k++) {
            if (need) {
                R uu = in_u, wp = in_w;
#pragma unroll
                for (int s = 0; s < L; s++) {
                    if (s == 0 && tid == 0) continue;   // sample 0 is the given start velocity (MPG:189)
                    uu = step_fwd(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp);
                    if constexpr (!CM) u[s] = uu;
                }
                out_u = uu;
                out_w = wp;
            }
            const R nu = wave_shift_up(out_u), nw = wave_shift_up(out_w);
            need = false;
            if (lane > 0 && fwd_active) {
                need = !(same_bits(nu, in_u) && same_bits(nw, in_w));
                in_u = nu;
                in_w = nw;
            }
            if (__ballot(need) == 0) break;
        }
        }
        const int pb = rounds & 1;
        if (lane == 63) s_bs[pb][wv + 1] = BoundaryState<R>{out_u, out_w};
        if (tid == 0) s_any[f_nxt] = 0;
        __syncthreads();
        const int changed_last = s_any[f_prv];
        const BoundaryState<R> nb = s_bs[pb][wv];
        if (rounds > 0 && changed_last == 0) break;   // nobody had work left last round
        if (lane == 0 && tid > 0 && fwd_active) {
            need = !(same_bits(nb.u, in_u) && same_bits(nb.w, in_w));
            in_u = nb.u;
            in_w = nb.w;
        }
        if (need) s_any[f_cur] = 1;
        { const int t = f_prv; f_prv = f_cur; f_cur = f_nxt; f_nxt = t; }
        rounds++;
        if (rounds > 2 * T + 8) {
            if (tid == 0 && flags) atomicOr(&flags[b], VAP_FLAG_NOCONVERGE_BIT);
            break;
        }
    }
    if constexpr (CM) {
        // forward commit: the converged incoming states are final; write the sweep's result over the caps
        R uu = in_u, wp = in_w;
#pragma unroll
        for (int s = 0; s < L; s++) {
            if (s == 0 && tid == 0) { cp[0] = start_u; continue; }
            uu = step_fwd(am[PSA ? s : 0], q[s], g[s], A[s], cp[s], uu, wp);
            cp[s] = uu;
        }
    }
    const int fwd_rounds = rounds;
    const long long t_fwd1 = stats ? __builtin_amdgcn_s_memtime() : 0;

    // ---------------- backward sweep: the step (j+1 -> j) into owned sample j uses k[j+1], dth[j]
    // (and k[j+2] for rho).  Slots at or past the fixed end sample N-1 are idle slots holding
    // u = end_u: walking through them restarts the chain exactly as MPG:252-253 does.
    // (The stage still holds dtheta.)
    RowRegs<R, L> rk;   // the curvature row comes back while dtheta is read out of the stage
    row_fetch<R, L>(rk, K, S < TL + 2 ? S : TL + 2, aligned, tid, T);
#pragma unroll
    for (int s = 0; s < L; s++) g[s] = stage[cpos(s)];   // dtheta[j] for now
    __syncthreads();
    stage_put<R, L>(stage, rk, TL + 2, aligned, tid, T);
    __syncthreads();
    {
        R kc = (R)fabs(stage[cpos(1)]);
#pragma unroll
        for (int s0 = 0; s0 < L; s0 += BK) {
            R kn[BK];
#pragma unroll
            for (int i = 0; i < BK; i++) kn[i] = (R)fabs(stage[cpos(s0 + i + 2)]);
#pragma unroll
            for (int i = 0; i < BK; i++) {
                const int s = s0 + i, j = lo + s;
                const bool valid = j <= N - 2;
                R qq;
                R base = fc.adecp;
                if constexpr (ACC) {
                    // the step into j starts at sample j+1: the clamp comes from the sweep's max_dec, the wheel limit
                    // from the max_acc the sweep has at j+1 (MPG:256-257); a straight sample has max_dec alone
                    base = adecp_b;
                }
                [[maybe_unused]] const R ufwd_s = cp[s];   // CM: the forward result sits where the new cap goes
                fast_derive_k(fc, kc, (j + 2 <= N - 1) ? kn[i] : (R)0, base, q[s], qq, A[s], cp[s]);
                g[s] = fast_gq(fast_gg(fc, g[s]), qq);
                if constexpr (ACC) {
                    A[s] = fast_cap_A(fc, kc, A[s]);
                    // (a zero heading difference, g < 0: the wheel limit is +inf unless the angular velocity rises)
                    // — there the clamp decides: amaxp = A (kHuge times any non-zero rise still wins against it)
                    am[s] = (valid && !(kc < (R)1e-6) && !(g[s] < (R)0)) ? twodd * (R)acc.bwd[row + j + 1] : A[s];
                }
                if constexpr (CM) {
                    if (!valid) { idle_coef(q[s], g[s], A[s], cp[s]); cp[s] = end_u; }
                    else cp[s] = vmin(cp[s], ufwd_s);
                } else {
                    if (!valid) { idle_coef(q[s], g[s], A[s], cp[s]); u[s] = end_u; }
                }
                {
                    R amv, gv;
                    fast_scale(ACC ? am[ACC ? s : 0] : fc.amaxp, g[s], A[s], amv, gv);
                    g[s] = gv;
                    if constexpr (PSA) am[s] = amv;
                }
                q[s] = opaque(q[s]);
                kc = kn[i];
            }
        }
    }
    const int last_chunk = (N - 1) / L;     // chunk that owns the fixed end sample
    if (tid >= last_chunk) { in_u = end_u; in_w = (R)0; }
    else { in_u = CM ? cp[L - 1] : u[CM ? 0 : L - 1]; in_w = in_u; }
    // The backward step reads the forward value of the sample it overwrites, so a chunk cannot be
    // re-run in place: the rounds only propagate boundary states (u[] stays the forward result) and
    // one commit evaluation with the final incoming state stores the backward velocities.
    const bool bwd_active = tid <= last_chunk;
    need = bwd_active;
    out_u = in_u;
    out_w = in_w;
    rounds = 0;
    if (tid == 0) { s_any[0] = 0; s_any[1] = 0; s_any[2] = 0; }
    __syncthreads();
    f_cur = 0; f_nxt = 1; f_prv = 2;
    const bool bwd_nb = lane < 63 && tid < last_chunk;
    while (true) {   // mirror image: states move one lane down, wave w+1 hands its first chunk's state to wave w
        if constexpr (CM) {
            if (__ballot(need) != 0) {   // (as in the forward sweep: the wavefront evaluates as one)
#pragma unroll 1
                for (int k = 0; k < kInner; k++) {
                    R uu = in_u, wp = in_w;
                    if (any_dup) {
#pragma unroll
                        for (int s = L - 1; s >= 0; s--) uu = bwd_step<true, true>(am[PSA ? s : 0], q[s], g[s], A[s], cp[s], uu, wp, (R)0);
                    } else {
#pragma unroll
                        for (int s = L - 1; s >= 0; s--) uu = bwd_step<false, true>(am[PSA ? s : 0], q[s], g[s], A[s], cp[s], uu, wp, (R)0);
                    }
                    out_u = uu;
                    out_w = wp;
                    const R nu = wave_shift_down(out_u), nw = wave_shift_down(out_w);
                    need = bwd_nb && !(same_bits(nu, in_u) && same_bits(nw, in_w));
                    in_u = bwd_nb ? nu : in_u;
                    in_w = bwd_nb ? nw : in_w;
                    if (__ballot(need) == 0) break;
                }
            }
        } else
#pragma unroll 1
        for (int k = 0; k < kInner; k++) {
            if (need) {
                R uu = in_u, wp = in_w;
                if (any_dup) {
#pragma unroll
                    for (int s = L - 1; s >= 0; s--) uu = bwd_step<true, CM>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, u[CM ? 0 : s]);
                } else {
#pragma unroll
                    for (int s = L - 1; s >= 0; s--) uu = bwd_step<false, CM>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, u[CM ? 0 : s]);
                }
                out_u = uu;
                out_w = wp;
            }
            const R nu = wave_shift_down(out_u), nw = wave_shift_down(out_w);
            need = false;
            if (lane < 63 && tid < last_chunk) {
                need = !(same_bits(nu, in_u) && same_bits(nw, in_w));
                in_u = nu;
                in_w = nw;
            }
            if (__ballot(need) == 0) break;
        }
        const int pb = rounds & 1;
        if (lane == 0) s_bs[pb][wv] = BoundaryState<R>{out_u, out_w};
        if (tid == 0) s_any[f_nxt] = 0;
        __syncthreads();
        const int changed_last = s_any[f_prv];
        const BoundaryState<R> nb = s_bs[pb][wv + 1];
        if (rounds > 0 && changed_last == 0) break;
        if (lane == 63 && tid < last_chunk) {
            need = !(same_bits(nb.u, in_u) && same_bits(nb.w, in_w));
            in_u = nb.u;
            in_w = nb.w;
        }
        if (need) s_any[f_cur] = 1;
        { const int t = f_prv; f_prv = f_cur; f_cur = f_nxt; f_nxt = t; }
        rounds++;
        if (rounds > 2 * T + 8) {
            if (tid == 0 && flags) atomicOr(&flags[b], VAP_FLAG_NOCONVERGE_BIT);
            break;
        }
    }
    const long long t_bwd1 = stats ? __builtin_amdgcn_s_memtime() : 0;
    if (bwd_active) {
        R uu = in_u, wp = in_w;
        if (any_dup) {
#pragma unroll
            for (int s = L - 1; s >= 0; s--) (CM ? cp[s] : u[CM ? 0 : s]) = uu = bwd_step<true, CM>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, u[CM ? 0 : s]);
        } else {
#pragma unroll
            for (int s = L - 1; s >= 0; s--) (CM ? cp[s] : u[CM ? 0 : s]) = uu = bwd_step<false, CM>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, u[CM ? 0 : s]);
        }
    }
    // velocities leave through the stage (as IO elements, same padded positions) so the row is written with
    // 16 bytes per lane
    __syncthreads();
    IO *ostage = reinterpret_cast<IO *>(smem_raw);
#pragma unroll
    for (int s = 0; s < L; s++) {
        const int j = lo + s;
        ostage[cpos(s)] = j < N ? (IO)vel_sqrt(CM ? cp[s] : u[CM ? 0 : s]) : (IO)0;
    }
    __syncthreads();
    IO *V = vel + row;
    {
        constexpr int VW = 16 / sizeof(IO);
        const int n = S < TL ? S : TL;
        if ((S % VW) == 0) {
            using VT = typename std::conditional<sizeof(IO) == 4, float4, double2>::type;
            VT *dst = reinterpret_cast<VT *>(V);
            for (int i = tid; i < n / VW; i += T) {
                VT v;
                IO *e = reinterpret_cast<IO *>(&v);
                const int p0 = stage_pos<IO, L>(i * VW);
#pragma unroll
                for (int k = 0; k < VW; k++)   // L % VW == 0: the VW elements share a chunk
                    e[k] = ostage[(L % VW == 0) ? p0 + k : stage_pos<IO, L>(i * VW + k)];
                dst[i] = v;
            }
            for (int i = (n / VW) * VW + tid; i < n; i += T) V[i] = ostage[stage_pos<IO, L>(i)];
        } else {
            for (int i = tid; i < n; i += T) V[i] = ostage[stage_pos<IO, L>(i)];
        }
    }
    for (int j = TL + tid; j < S; j += T) V[j] = (IO)0;
    if constexpr (!std::is_same<R, IO>::value) {
        // the velocities in the arithmetic type as well (vhi: [B][S], what the time-domain resample integrates behind
        // fp32 rows); straight from the registers — this kernel serves the small batches
        if (vhi) {
#pragma unroll
            for (int s = 0; s < L; s++) {
                const int j = lo + s;
                if (j < S) vhi[row + j] = j < N ? vel_sqrt(CM ? cp[s] : u[CM ? 0 : s]) : (R)0;
            }
            for (int j = TL + tid; j < S; j += T) vhi[row + j] = (R)0;
        }
    }
    if (stats && tid == 0) {
        long long *st = stats + (size_t)b * 8;
        st[0] = fwd_rounds;
        st[1] = rounds;
        st[2] = t_fwd0 - t_start;                       // load + derive
        st[3] = t_fwd1 - t_fwd0;                        // forward rounds
        st[4] = t_bwd1 - t_fwd1;                        // backward derive + rounds
        st[5] = __builtin_amdgcn_s_memtime() - t_bwd1;  // commit + store
    }
}

// ------------------------------------------------------------------------------------------------
// K5c: rows longer than the register-resident kernel covers (config 2: one path, 10^6 samples).
// Same relaxation, two levels: a row is cut into super-chunks of SC = MAXT*L samples, one workgroup
// each, which relax internally exactly like K5b for a given incoming interface state; the interface
// states between super-chunks live in HBM and are iterated by re-launching ("super-rounds") until no
// interface changes.  A super-chunk whose incoming state is bit-identical to the one it last used
// returns at once.  Forward velocities go through an HBM scratch row (the backward sweep of a
// super-chunk may be re-run), final velocities are written by the backward kernel.
//   bnd   [2][B][nsc+1][2]  interface states by super-round parity
//   used  [B][nsc][2]       incoming state of the last evaluation      (NaN pattern = never)
//   outst [B][nsc][2]       outgoing state of the last evaluation
// ------------------------------------------------------------------------------------------------
template <typename R>
__global__ void k_dup_scan(int B, int S, VelConsts<R> c, const double *__restrict__ meta, const R *__restrict__ curv,
                           const R *__restrict__ dth, int *__restrict__ dup)
{
    const int b = blockIdx.y;
    const int N = (int)meta[(size_t)b * kMetaStride + 3];
    const FastConsts<R> fc = make_fast(c, (R)2 * (R)meta[(size_t)b * kMetaStride + 2]);
    bool any = false;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N - 1; i += gridDim.x * blockDim.x) {
        const size_t o = (size_t)b * S + i;
        const R kabs = (R)fabs(curv[o]);
        any |= fast_gq(fast_gg(fc, dth[o]), kabs * kabs) < (R)0;   // the kernels' own predicate
    }
    if (__syncthreads_or(any ? 1 : 0) && threadIdx.x == 0) atomicOr(&dup[b], 1);
}

template <typename R, typename IO, int L, int MAXT, int MINW, bool BWD>
__global__ __launch_bounds__(MAXT, MINW) void k_velocity_long(int S, int nsc, int round, int seq_sc, VelConsts<R> c, R start_u,
                                                              R end_u, const double *__restrict__ meta,
                                                              const R *__restrict__ curv,
                                                              const R *__restrict__ dtheta, R *__restrict__ ufwd,
                                                              IO *__restrict__ vel, R *__restrict__ bnd,
                                                              R *__restrict__ used, R *__restrict__ outst,
                                                              const int *__restrict__ dupflag,
                                                              int *__restrict__ changed, uint32_t *__restrict__ flags,
                                                              R *__restrict__ vhi)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    R *stage = reinterpret_cast<R *>(smem_raw);
    __shared__ BoundaryState<R> s_bs[2][MAXT / 64 + 2];   // states crossing a wavefront boundary
    __shared__ int s_any[3];
    constexpr int T = MAXT;
    constexpr int SC = T * L;
    // seq_sc >= 0: "sequential windows" mode — this launch handles super-chunk seq_sc of every path and
    // its incoming interface state (published by the previous launch) is final, so it is evaluated once.
    const bool seq = seq_sc >= 0;
    const int sc = seq ? seq_sc : blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int B = gridDim.y;
    const double *m = meta + (size_t)b * kMetaStride;
    const R twodd = (R)2 * (R)m[2];
    const int N = (int)m[3];
    const int base = sc * SC;
    const int last_sc = (N - 1) / SC;
    if (sc > last_sc) return;
    const size_t row = (size_t)b * S;
    const R *K = curv + row, *DT = dtheta + row;
    const FastConsts<R> fc = make_fast(c, twodd);
    const bool any_dup = dupflag[b] != 0;
    const int lo = tid * L;
    // interface arrays
    const size_t ifs = (size_t)(nsc + 1) * 2;                          // per path
    R *bnd_prev = bnd + ((size_t)(seq ? 0 : ((round + 1) & 1)) * B + b) * ifs;
    R *bnd_cur = bnd + ((size_t)(seq ? 0 : (round & 1)) * B + b) * ifs;
    R *my_used = used + ((size_t)b * nsc + sc) * 2;
    R *my_out = outst + ((size_t)b * nsc + sc) * 2;
    const int if_in = BWD ? sc + 1 : sc, if_out = BWD ? sc : sc + 1;
    const bool exact_in = BWD ? (sc == last_sc) : (sc == 0);
    R in0_u = exact_in ? (BWD ? end_u : start_u) : (R)0, in0_w = (R)0;
    if (seq && !exact_in) { in0_u = bnd_prev[if_in * 2]; in0_w = bnd_prev[if_in * 2 + 1]; }
    if (!seq && round > 0) {
        if (!exact_in) { in0_u = bnd_prev[if_in * 2]; in0_w = bnd_prev[if_in * 2 + 1]; }
        if (exact_in || (same_bits(in0_u, my_used[0]) && same_bits(in0_w, my_used[1]))) {
            // nothing new came in: republish the last outgoing state for the next super-round
            if (tid == 0) { bnd_cur[if_out * 2] = my_out[0]; bnd_cur[if_out * 2 + 1] = my_out[1]; }
            return;
        }
    }
    if (tid == 0) { s_any[0] = 0; s_any[1] = 0; s_any[2] = 0; }
    R q[L], g[L], A[L], cp[L], u[L];   // q[] = rho, g[] = g*k^2 (vap_device.h)
    constexpr bool PSA = ScaledStep<R>::value;   // the scaled fp64 step keeps its `am` per slot (fast_scale)
    R am[PSA ? L : 1];
    const R base_p = BWD ? fc.adecp : fc.amaxp;
    // element e of the stage = global sample g0 + e; a forward super-chunk needs k[base-2 ..]
    constexpr int VW = 16 / (int)sizeof(R);
    const int g0 = BWD ? base : (base > 0 ? base - VW : 0);
    const int n_k = BWD ? SC + 2 : SC + VW;
    const bool aligned = (S % VW) == 0;
    {
        int n = N - g0;
        n = n < 0 ? 0 : (n > n_k ? n_k : n);
        stage_load<R, L>(stage, K + g0, n, n_k, aligned, tid, T);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < L; s++) {
        const int j = base + lo + s;                                  // global owned sample
        const bool valid = BWD ? (j <= N - 2) : (j >= 1 && j <= N - 1);
        const int src = BWD ? j + 1 : j - 1;                          // curvature sample of the step
        const int prv = BWD ? j + 2 : j - 2;                          // ... and of the step before it
        const bool has_prv = valid && prv >= 0 && prv <= N - 1;
        const R kabs = (R)fabs(stage[stage_pos<R, L>(valid ? src - g0 : 0)]);
        const R kpv = (R)fabs(stage[stage_pos<R, L>(has_prv ? prv - g0 : 0)]);
        fast_derive_k(fc, kabs, has_prv ? kpv : (R)0, base_p, q[s], g[s], A[s], cp[s]);   // g[s] = k^2 for now
        if (!valid) idle_coef(q[s], g[s], A[s], cp[s]);
        u[s] = BWD ? end_u : start_u;
    }
    __syncthreads();
    {
        int n = N - g0;
        n = n < 0 ? 0 : (n > n_k ? n_k : n);
        stage_load<R, L>(stage, DT + g0, n, n_k, aligned, tid, T);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < L; s++) {
        const int j = base + lo + s;
        const bool valid = BWD ? (j <= N - 2) : (j >= 1 && j <= N - 1);
        const int src = BWD ? j : j - 1;                              // dtheta sample of the step
        const R dth = stage[stage_pos<R, L>(valid ? src - g0 : 0)];
        const R gq = fast_gq(fast_gg(fc, dth), g[s]);
        R amv, gv;
        fast_scale(fc.amaxp, valid ? gq : (R)0, A[s], amv, gv);
        g[s] = gv;
        if constexpr (PSA) am[s] = amv;
    }
    if constexpr (BWD) {
        // forward velocities of the owned samples (idle slots hold end_u)
        __syncthreads();
        int n = N - base;
        n = n < 0 ? 0 : (n > SC ? SC : n);
        stage_load<R, L>(stage, ufwd + row + base, n, SC, (S % (16 / (int)sizeof(R))) == 0, tid, T);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < L; s++) {
            const int j = base + lo + s;
            if (j <= N - 2) u[s] = stage[stage_pos<R, L>(lo + s)];
        }
    }
    // chunk-local incoming states
    R in_u, in_w;
    const int local_last = BWD ? ((N - 1 - base) / L) : 0;   // BWD: chunk holding the fixed end sample (if in range)
    const bool bwd_has_end = BWD && sc == last_sc;
    if constexpr (!BWD) {
        if (tid == 0) {
            if (!exact_in && round == 0 && !seq) { in0_u = cp[0]; in0_w = in0_u; }
            in_u = in0_u; in_w = in0_w;
        } else { in_u = cp[0]; in_w = in_u; }
    } else {
        const bool tail = bwd_has_end ? tid >= local_last : false;
        if (tail) { in_u = end_u; in_w = (R)0; }
        else if (tid == T - 1) {
            if (round == 0 && !seq) { in0_u = u[L - 1]; in0_w = in0_u; }
            in_u = in0_u; in_w = in0_w;
        } else { in_u = u[L - 1]; in_w = in_u; }
    }
    const bool active = BWD ? (!bwd_has_end || tid <= local_last) : (base + lo <= N - 1);
    bool need = active;
    R out_u = in_u, out_w = in_w;
    int rounds = 0;
    __syncthreads();
    // same round structure as k_velocity_relax: up to kInner evaluations per workgroup barrier, states
    // handed lane to lane by DPP inside a wavefront, through LDS across wavefronts
    constexpr int kInner = 8;
    const int wv = tid >> 6, lane = tid & 63;
    const bool in_wave_nb = BWD ? (lane < 63 && tid < T - 1 && (!bwd_has_end || tid < local_last)) : (lane > 0 && active);
    const bool edge_nb = BWD ? (lane == 63 && tid < T - 1 && (!bwd_has_end || tid < local_last)) : (lane == 0 && tid > 0 && active);
    int f_cur = 0, f_nxt = 1, f_prv = 2;
    while (true) {
#pragma unroll 1
        for (int k = 0; k < kInner; k++) {
            if (need) {
                R uu = in_u, wp = in_w;
                if constexpr (!BWD) {
#pragma unroll
                    for (int s = 0; s < L; s++) {
                        if (s == 0 && tid == 0 && base == 0) continue;   // sample 0 is the given start velocity
                        uu = step_fwd(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp);
                        u[s] = uu;
                    }
                } else if (any_dup) {
#pragma unroll
                    for (int s = L - 1; s >= 0; s--) uu = fast_backward_a<true>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, u[s]);
                } else {
#pragma unroll
                    for (int s = L - 1; s >= 0; s--) uu = fast_backward_a<false>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, u[s]);
                }
                out_u = uu;
                out_w = wp;
            }
            const R nu = BWD ? wave_shift_down(out_u) : wave_shift_up(out_u);
            const R nw = BWD ? wave_shift_down(out_w) : wave_shift_up(out_w);
            need = false;
            if (in_wave_nb) {
                need = !(same_bits(nu, in_u) && same_bits(nw, in_w));
                in_u = nu;
                in_w = nw;
            }
            if (__ballot(need) == 0) break;
        }
        const int pb = rounds & 1;
        if (lane == (BWD ? 0 : 63)) s_bs[pb][wv + (BWD ? 0 : 1)] = BoundaryState<R>{out_u, out_w};
        if (tid == 0) s_any[f_nxt] = 0;
        __syncthreads();
        const int changed_last = s_any[f_prv];
        const BoundaryState<R> nb = s_bs[pb][wv + (BWD ? 1 : 0)];
        if (rounds > 0 && changed_last == 0) break;
        if (edge_nb) {
            need = !(same_bits(nb.u, in_u) && same_bits(nb.w, in_w));
            in_u = nb.u;
            in_w = nb.w;
        }
        if (need) s_any[f_cur] = 1;
        { const int t = f_prv; f_prv = f_cur; f_cur = f_nxt; f_nxt = t; }
        rounds++;
        if (rounds > 2 * T + 8) {
            if (tid == 0 && flags) atomicOr(&flags[b], VAP_FLAG_NOCONVERGE_BIT);
            break;
        }
    }
    if constexpr (BWD) {
        if (active) {
            R uu = in_u, wp = in_w;
            if (any_dup) {
#pragma unroll
                for (int s = L - 1; s >= 0; s--) u[s] = uu = fast_backward_a<true>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, u[s]);
            } else {
#pragma unroll
                for (int s = L - 1; s >= 0; s--) u[s] = uu = fast_backward_a<false>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, u[s]);
            }
        }
    }
    // publish the super-chunk's outgoing interface state: the out-state of its last (forward) / first
    // (backward) chunk, which that thread holds
    const int owner = BWD ? 0 : T - 1;
    if (tid == owner) {
        const R ou = out_u, ow = out_w;
        const bool diff = !seq && (round == 0 || !(same_bits(ou, bnd_prev[if_out * 2]) && same_bits(ow, bnd_prev[if_out * 2 + 1])));
        bnd_cur[if_out * 2] = ou;
        bnd_cur[if_out * 2 + 1] = ow;
        my_out[0] = ou;
        my_out[1] = ow;
        // a guessed incoming state (super-round 0) is recorded as "never": the next super-round
        // re-evaluates with whatever the neighbour published
        const bool guessed = round == 0 && !exact_in && !seq;
        my_used[0] = guessed ? (R)NAN : in0_u;
        my_used[1] = guessed ? (R)NAN : in0_w;
        if (diff) atomicAdd(changed, 1);
    }
    // rows leave through the stage: forward -> u (squared velocity) scratch, backward -> final velocity
    __syncthreads();
    int n = S - base;
    n = n > SC ? SC : n;
    if constexpr (BWD) {
        IO *ostage = reinterpret_cast<IO *>(smem_raw);
#pragma unroll
        for (int s = 0; s < L; s++) {
            const int j = base + lo + s;
            ostage[stage_pos<IO, L>(lo + s)] = j < N ? (IO)vel_sqrt(u[s]) : (IO)0;
        }
        __syncthreads();
        IO *dst = vel + row + base;
        for (int i = tid; i < n; i += T) dst[i] = ostage[stage_pos<IO, L>(i)];
        if (sc == last_sc)
            for (int j = (last_sc + 1) * SC + tid; j < S; j += T) vel[row + j] = (IO)0;
        if constexpr (!std::is_same<R, IO>::value) {
            if (vhi) {   // the velocities in the arithmetic type as well (the time-domain resample behind fp32 rows)
#pragma unroll
                for (int s = 0; s < L; s++) {
                    const int j = base + lo + s;
                    if (j < S) vhi[row + j] = j < N ? vel_sqrt(u[s]) : (R)0;
                }
                if (sc == last_sc)
                    for (int j = (last_sc + 1) * SC + tid; j < S; j += T) vhi[row + j] = (R)0;
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < L; s++) stage[stage_pos<R, L>(lo + s)] = u[s];
        __syncthreads();
        R *dst = ufwd + row + base;
        for (int i = tid; i < n; i += T) dst[i] = stage[stage_pos<R, L>(i)];
    }
}

// ------------------------------------------------------------------------------------------------
// K5c': the same two-level relaxation with the interfaces handed on INSIDE a launch — decoupled
// look-back between super-chunks, one launch per direction, no host round trip (config 2).
// A workgroup is one wavefront and owns the super-chunk of 64*L samples its TICKET names (tickets are
// drawn in dispatch order, so a workgroup only ever waits for workgroups that already run: no
// residency assumption, any number of super-chunks).  It relaxes its super-chunk from a guessed
// incoming state and publishes a record {incoming state used, outgoing state}; then it looks back at
// the records of its (up to) 64 predecessors at once, one per lane:
//   * predecessor's outgoing state differs from the state it used -> relax again from that state
//     (only the entry lane starts; the change ripples as far as it has to) and publish again;
//   * it is FINAL as soon as some predecessor j is final and every link between j and itself is
//     consistent (record k used exactly what record k-1 published): a record's outgoing state is a
//     function of the incoming state it names, so such a chain carries the sequential sweep's values
//     whatever the moments the records were read at.  Finality therefore travels 64 super-chunks per
//     hop where nothing changes, and at the speed of the recurrence where a ramp is being walked.
// Super-chunk 0 (backwards: the one holding the end sample) knows its incoming state and is final
// after one evaluation.  Records are 8-byte {tag, half-word} granules written by single agent-scope
// stores; a record is taken only when all its tags agree (tag = version, top bit = final; zeroed
// before every launch).  Every spin is bounded: a workgroup that waits longer than kChaseTimeout
// raises VAP_FLAG_NOCONVERGE, publishes what it has as final and goes on, so the grid always drains.
// The fixed point is the sequential sweep bit for bit, like k_velocity_long's.
// ------------------------------------------------------------------------------------------------
using gu64 = __attribute__((address_space(1))) unsigned long long;
using gu32 = __attribute__((address_space(1))) unsigned int;
constexpr int kChaseRecGranules = 8;                 // 64-byte records
constexpr uint32_t kChaseFinal = 0x80000000u;
constexpr long long kChaseTimeout = 100000000ll;     // wall_clock64 ticks (100 MHz): 1 s

template <typename R>
__device__ __forceinline__ R wave_bcast(R x, int src)
{
    if constexpr (sizeof(R) == 8) {
        const uint64_t v = __builtin_bit_cast(uint64_t, x);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
        return __builtin_bit_cast(R, ((uint64_t)hi << 32) | lo);
    } else {
        return __builtin_bit_cast(R, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src));
    }
}

// the four values of a record, wave-uniform, leave as G = 4 * sizeof(R) / 4 granules from lanes 0..G-1
template <typename R>
__device__ __forceinline__ void chase_publish(gu64 *rec, uint32_t tag, R in_u, R in_w, R out_u, R out_w, int lane)
{
    constexpr int H = sizeof(R) / 4, G = 4 * H;
    const int vi = lane / H, h = lane % H;
    const R sel = vi == 0 ? in_u : (vi == 1 ? in_w : (vi == 2 ? out_u : out_w));
    uint32_t half;
    if constexpr (sizeof(R) == 8) {
        const uint64_t b = __builtin_bit_cast(uint64_t, sel);
        half = h ? (uint32_t)(b >> 32) : (uint32_t)b;
    } else {
        half = __builtin_bit_cast(uint32_t, sel);
    }
    if (lane < G) __hip_atomic_store(rec + lane, ((unsigned long long)tag << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The sign-aware backward step (fast_backward_a<true, false>, vap_device.h) with its compare / select / max taken off the
// dependent chain: the penalty max(t, other)*|g| with other = (g < 0 ? 0 : -t) is the larger of t*|g| and -t*gn,
// gn = (g < 0 ? 0 : |g|), and rounding is monotone, so
//     clamp01(am - max(t, other)*|g|) = clamp01(min(fma(-t, |g|, am), fma(t, gn, am)))        bit for bit
// (g >= 0: the two FMAs are am -+ |t||g|, the smaller one is the old value; g < 0: t > 0 gives am - t|g| <= am = the
// second, t <= 0 gives max(t, 0) = 0 -> am = the second exactly).  Two independent FMAs and a min with the clamp modifier
// instead of xor / cndmask / cndmask / max / fma: the chain is fma, fma, min, fma, min.
__device__ __forceinline__ double bwd_step_dup2(double am, double rho, double g, double gn, double A, double cap, double u,
                                                double &uprev)
{
    double r, c2;
    asm("v_fma_f64 %0, -%3, %4, %2\n\t"
        "v_fma_f64 %1, %0, %6, %7\n\t"
        "v_fma_f64 %0, -%0, |%5|, %7\n\t"
        "v_min_f64 %0, %0, %1 clamp\n\t"
        "v_fma_f64 %0, %8, %0, %2\n\t"
        "v_min_f64 %0, %0, %9"
        : "=&v"(r), "=&v"(c2)
        : "v"(u), "v"(rho), "v"(uprev), "v"(g), "v"(gn), "v"(am), "v"(A), "v"(cap));
    uprev = u;
    return r;
}
__device__ __forceinline__ float bwd_step_dup2(float am, float rho, float g, float gn, float A, float cap, float u, float &uprev)
{
    (void)gn;
    return bwd_step<true, true>(am, rho, g, A, cap, u, uprev, 0.0f);
}

template <typename R, typename IO, int L, bool BWD>
__global__ __launch_bounds__(64, 2) void k_velocity_chase(int B, int S, int nsc, VelConsts<R> c, R start_u, R end_u,
                                                          const double *__restrict__ meta, const R *__restrict__ curv,
                                                          const R *__restrict__ dtheta, R *__restrict__ ufwd,
                                                          IO *__restrict__ vel, unsigned long long *records,
                                                          unsigned int *ticket, int *dupflag, uint32_t *__restrict__ flags,
                                                          R *__restrict__ vhi, long long *__restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    R *stage = reinterpret_cast<R *>(smem_raw);
    constexpr int T = 64;
    constexpr int SC = T * L;
    constexpr int H = sizeof(R) / 4, G = 4 * H;
    const int tid = threadIdx.x, lane = tid;
    // dispatch-ordered ticket -> (path, position in the sweep's order)
    unsigned int tk = 0;
    if (lane == 0) tk = __hip_atomic_fetch_add((gu32 *)ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tk = (unsigned int)__builtin_amdgcn_readfirstlane((int)tk);
    const int b = (int)(tk / (unsigned int)nsc), idx = (int)(tk % (unsigned int)nsc);
    if (b >= B) return;
    const double *m = meta + (size_t)b * kMetaStride;
    const R twodd = (R)2 * (R)m[2];
    const int N = (int)m[3];
    const int last_sc = (N - 1) / SC;
    const int sc = BWD ? last_sc - idx : idx;
    if (idx > last_sc) return;                          // nobody looks back at these
    const int base = sc * SC;
    const size_t row = (size_t)b * S;
    const R *K = curv + row, *DT = dtheta + row;
    const FastConsts<R> fc = make_fast(c, twodd);
    // zero heading differences anywhere on the path (the sign-aware backward step): the forward launch finds them,
    // the backward launch reads the flag
    const bool any_dup = BWD ? dupflag[b] != 0 : false;
    const long long t_start = stats ? wall_clock64() : 0;
    const int lo = tid * L;
    gu64 *path_recs = (gu64 *)records + (size_t)b * nsc * kChaseRecGranules;
    gu64 *my_rec = path_recs + (size_t)idx * kChaseRecGranules;
    const bool exact_in = idx == 0;
    R in0_u = exact_in ? (BWD ? end_u : start_u) : (R)0, in0_w = (R)0;

    // q[] = rho, g[] = g*k^2 (vap_device.h).  Backwards the forward value of a sample is folded into its cap once
    // (min is exact, so min(min(x, cap), u_fwd) = min(x, min(cap, u_fwd)): k_velocity_relax's commit mode) and the
    // results are committed into cp[] — one dependent instruction less per step and no u[] to keep in registers
    R q[L], g[L], A[L], cp[L], u[BWD ? 1 : L];
    constexpr bool PSA = ScaledStep<R>::value;
    R am[PSA ? L : 1];
    R gn[(PSA && BWD) ? L : 1];   // backwards: g with the zero-heading-difference slots zeroed (the sign-aware step)
    const R base_p = BWD ? fc.adecp : fc.amaxp;
    constexpr int VW = 16 / (int)sizeof(R);
    const int g0 = BWD ? base : (base > 0 ? base - VW : 0);
    const int n_k = BWD ? SC + 2 : SC + VW;
    const bool aligned = (S % VW) == 0;
    {
        int n = N - g0;
        n = n < 0 ? 0 : (n > n_k ? n_k : n);
        stage_load<R, L>(stage, K + g0, n, n_k, aligned, tid, T);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < L; s++) {
        const int j = base + lo + s;
        const bool valid = BWD ? (j <= N - 2) : (j >= 1 && j <= N - 1);
        const int src = BWD ? j + 1 : j - 1;
        const int prv = BWD ? j + 2 : j - 2;
        const bool has_prv = valid && prv >= 0 && prv <= N - 1;
        const R kabs = (R)fabs(stage[stage_pos<R, L>(valid ? src - g0 : 0)]);
        const R kpv = (R)fabs(stage[stage_pos<R, L>(has_prv ? prv - g0 : 0)]);
        fast_derive_k(fc, kabs, has_prv ? kpv : (R)0, base_p, q[s], g[s], A[s], cp[s]);
        if (!valid) idle_coef(q[s], g[s], A[s], cp[s]);
        if constexpr (!BWD) u[s] = start_u;
    }
    __syncthreads();
    {
        int n = N - g0;
        n = n < 0 ? 0 : (n > n_k ? n_k : n);
        stage_load<R, L>(stage, DT + g0, n, n_k, aligned, tid, T);
    }
    __syncthreads();
    bool saw_dup = false;
#pragma unroll
    for (int s = 0; s < L; s++) {
        const int j = base + lo + s;
        const bool valid = BWD ? (j <= N - 2) : (j >= 1 && j <= N - 1);
        const int src = BWD ? j : j - 1;
        const R dth = stage[stage_pos<R, L>(valid ? src - g0 : 0)];
        const R gq = fast_gq(fast_gg(fc, dth), g[s]);
        if constexpr (!BWD) saw_dup |= valid && gq < (R)0;   // k_dup_scan's predicate, on the same values
        R amv, gv;
        fast_scale(fc.amaxp, valid ? gq : (R)0, A[s], amv, gv);
        g[s] = gv;
        if constexpr (PSA) am[s] = amv;
        if constexpr (PSA && BWD) gn[s] = gv < (R)0 ? (R)0 : gv;
    }
    if constexpr (!BWD) {
        if (__ballot(saw_dup) != 0ull && tid == 0) atomicOr(&dupflag[b], 1);
    }
    if constexpr (BWD) {
        __syncthreads();
        int n = N - base;
        n = n < 0 ? 0 : (n > SC ? SC : n);
        stage_load<R, L>(stage, ufwd + row + base, n, SC, aligned, tid, T);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < L; s++) {
            const int j = base + lo + s;
            const R uf = j <= N - 2 ? stage[stage_pos<R, L>(lo + s)] : end_u;   // (a slot that holds no step restarts the chain at end_u)
            cp[s] = vmin(cp[s], uf);
            if (s == L - 1) u[0] = uf;
        }
    }
    // chunk-local incoming states (k_velocity_long's, for one wavefront)
    R in_u, in_w;
    const int local_last = BWD ? ((N - 1 - base) / L) : 0;
    const bool bwd_has_end = BWD && sc == last_sc;
    constexpr int entry = BWD ? T - 1 : 0;              // the lane a neighbour's state comes in at
    constexpr int owner = BWD ? 0 : T - 1;              // the lane whose outgoing state leaves the super-chunk
    if constexpr (!BWD) {
        if (!exact_in) { in0_u = wave_bcast(cp[0], 0); in0_w = in0_u; }
        if (tid == 0) { in_u = in0_u; in_w = in0_w; }
        else { in_u = cp[0]; in_w = in_u; }
    } else {
        if (!exact_in) { in0_u = wave_bcast(u[0], T - 1); in0_w = in0_u; }
        const bool tail = bwd_has_end ? tid >= local_last : false;
        if (tail) { in_u = end_u; in_w = (R)0; }
        else if (tid == T - 1) { in_u = in0_u; in_w = in0_w; }
        else { in_u = u[0]; in_w = in_u; }
    }
    const bool active = BWD ? (!bwd_has_end || tid <= local_last) : (base + lo <= N - 1);
    const bool in_wave_nb = BWD ? (lane < 63 && (!bwd_has_end || tid < local_last)) : (lane > 0 && active);
    R out_u = in_u, out_w = in_w;
    bool need = active;
    uint32_t version = 0;
    bool timed_out = false;
    const long long t_begin = wall_clock64();
    long long t_first = 0;
    int n_evals = 0, n_iters = 0, n_polls = 0;
    while (true) {
        // relax the super-chunk for the incoming state in0: states move lane to lane by DPP
        int it = 0;
        while (true) {
            if (need) {
                R uu = in_u, wp = in_w;
                if constexpr (!BWD) {
#pragma unroll
                    for (int s = 0; s < L; s++) {
                        if (s == 0 && tid == 0 && base == 0) continue;   // sample 0 is the given start velocity
                        uu = step_fwd(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp);
                        u[s] = uu;
                    }
                } else if (any_dup) {
#pragma unroll
                    for (int s = L - 1; s >= 0; s--) uu = bwd_step_dup2(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], gn[(PSA && BWD) ? s : 0], A[s], cp[s], uu, wp);
                } else {
#pragma unroll
                    for (int s = L - 1; s >= 0; s--) uu = bwd_step<false, true>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, (R)0);
                }
                out_u = uu;
                out_w = wp;
            }
            const R nu = BWD ? wave_shift_down(out_u) : wave_shift_up(out_u);
            const R nw = BWD ? wave_shift_down(out_w) : wave_shift_up(out_w);
            need = false;
            if (in_wave_nb) {
                need = !(same_bits(nu, in_u) && same_bits(nw, in_w));
                in_u = nu;
                in_w = nw;
            }
            n_iters++;
            if (__ballot(need) == 0) break;
            if (++it > 2 * T + 8) {
                if (tid == 0 && flags) atomicOr(&flags[b], VAP_FLAG_NOCONVERGE_BIT);
                break;
            }
        }
        const R pub_u = wave_bcast(out_u, owner), pub_w = wave_bcast(out_w, owner);
        if (stats && n_evals == 0) t_first = wall_clock64();
        n_evals++;
        if (exact_in) {
            chase_publish<R>(my_rec, kChaseFinal | 1u, in0_u, in0_w, pub_u, pub_w, lane);
            break;
        }
        // look back: lane i reads the record of predecessor idx-1-i
        bool final_now = false, again = false;
        bool published = false;
        while (true) {
            n_polls++;
            const int p = idx - 1 - lane;
            unsigned long long gr[G];
            if (p >= 0) {
                gu64 *pr = path_recs + (size_t)p * kChaseRecGranules;
#pragma unroll
                for (int k = 0; k < G; k++) gr[k] = __hip_atomic_load(pr + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
#pragma unroll
                for (int k = 0; k < G; k++) gr[k] = 0ull;
            }
            const uint32_t tag = (uint32_t)(gr[0] >> 32);
            bool ok = p >= 0 && tag != 0u;
#pragma unroll
            for (int k = 1; k < G; k++) ok = ok && (uint32_t)(gr[k] >> 32) == tag;
            R pv[4];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                if constexpr (sizeof(R) == 8)
                    pv[v] = __builtin_bit_cast(R, ((gr[2 * v + 1] & 0xffffffffull) << 32) | (gr[2 * v] & 0xffffffffull));
                else
                    pv[v] = __builtin_bit_cast(R, (uint32_t)gr[v]);
            }
            const unsigned long long okmask = __ballot(ok);
            const bool ok0 = (okmask & 1ull) != 0;
            const R cand_u = wave_bcast(pv[2], 0), cand_w = wave_bcast(pv[3], 0);
            if (ok0 && !(same_bits(cand_u, in0_u) && same_bits(cand_w, in0_w))) {
                in0_u = cand_u;
                in0_w = cand_w;
                again = true;
            }
            // links: record k (lane i) used what record k-1 (lane i+1) published
            const R nxt_u = wave_shift_down(pv[2]), nxt_w = wave_shift_down(pv[3]);
            const bool nxt_ok = lane < 63 && ((okmask >> (lane + 1)) & 1ull) != 0;
            const bool link = ok && nxt_ok && same_bits(pv[0], nxt_u) && same_bits(pv[1], nxt_w);
            const unsigned long long fin = __ballot(ok && (tag & kChaseFinal) != 0u);
            const unsigned long long links = __ballot(link);
            bool chain = false;
            if (ok0 && fin != 0ull) {
                const int j = __builtin_ctzll(fin);
                const unsigned long long mask = (j == 0) ? 0ull : (~0ull >> (64 - j));
                chain = (links & mask) == mask;
            }
            if (again) { final_now = false; break; }   // relax from the new state first; the next look-back decides
            if (chain) { final_now = true; break; }
            if (!published) {
                // what this evaluation produced, for the successors to work with meanwhile
                version++;
                chase_publish<R>(my_rec, version, in0_u, in0_w, pub_u, pub_w, lane);
                published = true;
            }
            if (wall_clock64() - t_begin > kChaseTimeout) { timed_out = true; break; }
            __builtin_amdgcn_s_sleep(4);
        }
        if (timed_out) {
            if (tid == 0 && flags) atomicOr(&flags[b], VAP_FLAG_NOCONVERGE_BIT);
            version++;
            chase_publish<R>(my_rec, kChaseFinal | version, in0_u, in0_w, pub_u, pub_w, lane);
            break;
        }
        if (final_now) {
            version++;
            chase_publish<R>(my_rec, kChaseFinal | version, in0_u, in0_w, pub_u, pub_w, lane);
            break;
        }
        // again: the entry lane restarts from the new incoming state
        need = false;
        if (lane == entry) {
            need = true;
            in_u = in0_u;
            in_w = in0_w;
        }
    }
    const long long t_final = stats ? wall_clock64() : 0;
    if constexpr (BWD) {
        if (active) {
            R uu = in_u, wp = in_w;
            if (any_dup) {
#pragma unroll
                for (int s = L - 1; s >= 0; s--) cp[s] = uu = bwd_step_dup2(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], gn[(PSA && BWD) ? s : 0], A[s], cp[s], uu, wp);
            } else {
#pragma unroll
                for (int s = L - 1; s >= 0; s--) cp[s] = uu = bwd_step<false, true>(PSA ? am[PSA ? s : 0] : fc.amaxp, q[s], g[s], A[s], cp[s], uu, wp, (R)0);
            }
        }
    }
    // rows leave through the stage: forward -> u (squared velocity) scratch, backward -> final velocity
    __syncthreads();
    int n = S - base;
    n = n > SC ? SC : n;
    if constexpr (BWD) {
        IO *ostage = reinterpret_cast<IO *>(smem_raw);
#pragma unroll
        for (int s = 0; s < L; s++) {
            const int j = base + lo + s;
            ostage[stage_pos<IO, L>(lo + s)] = j < N ? (IO)vel_sqrt(cp[s]) : (IO)0;
        }
        __syncthreads();
        IO *dst = vel + row + base;
        for (int i = tid; i < n; i += T) dst[i] = ostage[stage_pos<IO, L>(i)];
        if (sc == last_sc)
            for (int j = (last_sc + 1) * SC + tid; j < S; j += T) vel[row + j] = (IO)0;
        if constexpr (!std::is_same<R, IO>::value) {
            if (vhi) {   // the velocities in the arithmetic type as well (the time-domain resample behind fp32 rows)
#pragma unroll
                for (int s = 0; s < L; s++) {
                    const int j = base + lo + s;
                    if (j < S) vhi[row + j] = j < N ? vel_sqrt(cp[s]) : (R)0;
                }
                if (sc == last_sc)
                    for (int j = (last_sc + 1) * SC + tid; j < S; j += T) vhi[row + j] = (R)0;
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < L; s++) stage[stage_pos<R, L>(lo + s)] = u[s];
        __syncthreads();
        R *dst = ufwd + row + base;
        for (int i = tid; i < n; i += T) dst[i] = stage[stage_pos<R, L>(i)];
    }
    if (stats && tid == 0) {
        long long *my = stats + ((size_t)b * nsc + idx) * 8;
        my[0] = t_start;
        my[1] = t_begin;
        my[2] = t_first;
        my[3] = t_final;
        my[4] = wall_clock64();
        my[5] = n_evals;
        my[6] = n_iters;
        my[7] = n_polls;
    }
}

// Largest sample capacity the register-resident relaxation kernel covers.
// (plain fp64 rows are walked in windows and could be of any length; beyond 64 windows the two-level kernel, which
// spreads a row over many workgroups, is the better tool)
int velocity_relax_max_samples(bool f64, bool limits) { (void)limits; return f64 ? 512 * 20 : 512 * 40; }
// ... and with per-sample max_acceleration rows (one more register array per thread)
int velocity_relax_acc_max_samples(bool f64) { return f64 ? 512 * 8 : 512 * 20; }

template <typename R, typename IO, int L, int MAXT, int MINW, bool ACC = false>
static void launch_relax_t(hipStream_t st, int B, int S, const double c[6], double sv, double ev,
                           const double *meta, const void *curv, const void *dth, const void *vcap, const AccRowsV &accv,
                           void *vel, uint32_t *flags, void *vhi)
{
    const AccRows<R> acc = acc_rows<R>(accv);
    int T = (S + L - 1) / L;
    T = (T + 63) / 64 * 64;
    const R s = (R)sv, e = (R)ev;
    // developer knob: VAP_RELAX_STATS=1 prints rounds and in-kernel cycle shares (synchronises!)
    static const bool want_stats = getenv("VAP_RELAX_STATS") != nullptr;
    long long *stats = nullptr;
    if (want_stats) (void)hipMalloc(&stats, (size_t)B * 8 * sizeof(long long));
    const size_t lds = sizeof(R) * ((size_t)T * L + T + 8);
    if constexpr (ACC)
        hipLaunchKernelGGL((k_velocity_relax<R, IO, L, MAXT, MINW, true, true>), dim3(B), dim3(T), lds, st, S, make_consts<R>(c), s * s,
                           e * e, meta, (const R *)curv, (const R *)dth, (const R *)vcap, acc, (IO *)vel, flags, stats, (R *)vhi);
    else if (vcap)
        hipLaunchKernelGGL((k_velocity_relax<R, IO, L, MAXT, MINW, true, false>), dim3(B), dim3(T), lds, st, S, make_consts<R>(c), s * s,
                           e * e, meta, (const R *)curv, (const R *)dth, (const R *)vcap, acc, (IO *)vel, flags, stats, (R *)vhi);
    else
        hipLaunchKernelGGL((k_velocity_relax<R, IO, L, MAXT, MINW, false, false>), dim3(B), dim3(T), lds, st, S, make_consts<R>(c), s * s,
                           e * e, meta, (const R *)curv, (const R *)dth, (const R *)nullptr, acc, (IO *)vel, flags, stats, (R *)vhi);
    if (stats) {
        std::vector<long long> h((size_t)B * 8);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h.data(), stats, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
        (void)hipFree(stats);
        double sum[6] = {0, 0, 0, 0, 0, 0};
        long long mx[6] = {0, 0, 0, 0, 0, 0};
        for (int b = 0; b < B; b++)
            for (int k = 0; k < 6; k++) {
                sum[k] += (double)h[(size_t)b * 8 + k];
                if (h[(size_t)b * 8 + k] > mx[k]) mx[k] = h[(size_t)b * 8 + k];
            }
        fprintf(stderr, "[relax L=%d T=%d] rounds fwd mean %.1f max %lld | bwd mean %.1f max %lld | ticks mean: load %.0f fwd %.0f bwd %.0f commit %.0f | max: %lld %lld %lld %lld\n",
                L, T, sum[0] / B, mx[0], sum[1] / B, mx[1], sum[2] / B, sum[3] / B, sum[4] / B, sum[5] / B, mx[2], mx[3], mx[4], mx[5]);
    }
}

hipError_t launch_velocity_relax(hipStream_t st, bool r64, bool io64, int B, int S, const double c[6], double sv, double ev,
                                 const double *meta, const void *curv, const void *dth, const void *vcap,
                                 const AccRowsV &acc, void *vel, uint32_t *flags, void *vhi)
{
    if (acc.fwd) {
        // per-sample max_acceleration: one more register array per thread, so shorter chunks
        // (velocity_relax_acc_max_samples() is the limit the caller checks)
#define VAP_RELAX_ACC(R_, IO_, L_, MAXT_, W_) launch_relax_t<R_, IO_, L_, MAXT_, W_, true>(st, B, S, c, sv, ev, meta, curv, dth, vcap, acc, vel, flags, vhi)
        if (r64 && io64) {
            if (S <= 64 * 4) VAP_RELAX_ACC(double, double, 4, 256, 4);
            else VAP_RELAX_ACC(double, double, 8, 512, 4);
        } else if (r64) {
            if (S <= 64 * 4) VAP_RELAX_ACC(double, float, 4, 256, 4);
            else VAP_RELAX_ACC(double, float, 8, 512, 4);
        } else {
            if (S <= 64 * 4) VAP_RELAX_ACC(float, float, 4, 1024, 8);
            else if (S <= 512 * 16) VAP_RELAX_ACC(float, float, 16, 512, 4);
            else VAP_RELAX_ACC(float, float, 20, 512, 2);
        }
#undef VAP_RELAX_ACC
        return hipGetLastError();
    }
#define VAP_RELAX(R_, IO_, L_, MAXT_, W_) launch_relax_t<R_, IO_, L_, MAXT_, W_>(st, B, S, c, sv, ev, meta, curv, dth, vcap, acc, vel, flags, vhi)
    // chunk length: the longest instantiated L whose thread count still covers the row — fewer, longer
    // chunks mean fewer rounds (rounds ~ longest unclamped run / L) and fewer waves to synchronise
    const bool one_wave = S > 64 * 4 && S <= 64 * 16;
    if (r64 && io64) {
        if (S <= 64 * 4) VAP_RELAX(double, double, 4, 256, 4);
        else if (one_wave) VAP_RELAX(double, double, 16, 64, 2);   // one wavefront per path: no workgroup barrier at all
        else if (S <= 512 * 8) VAP_RELAX(double, double, 8, 512, 4);
        else VAP_RELAX(double, double, 20, 512, 2);
        return hipGetLastError();
    }
    if (r64) {
        if (S <= 64 * 4) VAP_RELAX(double, float, 4, 256, 4);
        else if (one_wave) VAP_RELAX(double, float, 16, 64, 2);
        else if (S <= 512 * 8) VAP_RELAX(double, float, 8, 512, 4);
        else VAP_RELAX(double, float, 20, 512, 2);
        return hipGetLastError();
    }
    if (S <= 64 * 4) VAP_RELAX(float, float, 4, 1024, 8);
    else if (S <= 256 * 16) VAP_RELAX(float, float, 16, 512, 4);
    else VAP_RELAX(float, float, 40, 512, 2);
#undef VAP_RELAX
    return hipGetLastError();
}

template <typename R, typename IO, int L, int MAXT, int MINW>
static hipError_t velocity_long_t(hipStream_t st, int B, int S, const double c[6], double sv, double ev,
                                  const double *meta, const void *curv, const void *dth, void *vel, uint32_t *flags,
                                  void *ufwd, void *state, int *counters, void *vhi)
{
    constexpr int SC = MAXT * L;
    const int nsc = (S + SC - 1) / SC;
    const R s = (R)sv, e = (R)ev;
    const size_t lds = sizeof(R) * ((size_t)MAXT * L + MAXT + 8);
    // state layout: bnd [2][B][nsc+1][2] | used [B][nsc][2] | outst [B][nsc][2]
    R *bnd = (R *)state;
    R *used = bnd + (size_t)2 * B * (nsc + 1) * 2;
    R *outst = used + (size_t)B * nsc * 2;
    int *dup = counters;            // [B]
    int *changed = counters + B;    // [2 * (nsc + 2)] one counter per super-round and direction
    hipError_t err;
    if ((err = hipMemsetAsync(counters, 0, sizeof(int) * ((size_t)B + 2 * (nsc + 2)), st)) != hipSuccess) return err;
    hipLaunchKernelGGL(k_dup_scan<R>, dim3(64, B), dim3(256), 0, st, B, S, make_consts<R>(c), meta, (const R *)curv,
                       (const R *)dth, dup);
    // Super-round convergence is decided on the host, one 4-byte read per check — but a super-round in
    // which nothing changes costs a few microseconds (every workgroup returns at once), a host round trip
    // ~35: rounds are launched three at a time and only the last one's counter is read.
    // The first check of a sweep comes after as many rounds as the previous call of this shape needed (a caller that
    // profiles batch after batch of similar routes — the bench loop — then pays one round trip per sweep instead of
    // one per three rounds); purely a launch-count heuristic, the result does not depend on it.
    constexpr int kRoundsPerCheck = 3;
    static thread_local int expect_rounds[2] = {kRoundsPerCheck, kRoundsPerCheck};
    static thread_local int expect_nsc = -1;
    if (expect_nsc != nsc) { expect_rounds[0] = expect_rounds[1] = kRoundsPerCheck; expect_nsc = nsc; }
    for (int dir = 0; dir < 2; dir++) {
        int round = 0;
        int batch = expect_rounds[dir];
        while (round <= nsc + 1) {
            int *ch = nullptr;
            for (int k = 0; k < batch && round <= nsc + 1; k++, round++) {
                ch = changed + dir * (nsc + 2) + round;
                if (dir == 0)
                    hipLaunchKernelGGL((k_velocity_long<R, IO, L, MAXT, MINW, false>), dim3(nsc, B), dim3(MAXT), lds, st, S, nsc,
                                       round, -1, make_consts<R>(c), s * s, e * e, meta, (const R *)curv, (const R *)dth,
                                       (R *)ufwd, (IO *)vel, bnd, used, outst, dup, ch, flags, (R *)vhi);
                else
                    hipLaunchKernelGGL((k_velocity_long<R, IO, L, MAXT, MINW, true>), dim3(nsc, B), dim3(MAXT), lds, st, S, nsc,
                                       round, -1, make_consts<R>(c), s * s, e * e, meta, (const R *)curv, (const R *)dth,
                                       (R *)ufwd, (IO *)vel, bnd, used, outst, dup, ch, flags, (R *)vhi);
                if ((err = hipGetLastError()) != hipSuccess) return err;
            }
            int h = 0;
            if ((err = hipMemcpyAsync(&h, ch, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return err;
            if ((err = hipStreamSynchronize(st)) != hipSuccess) return err;
            if (h == 0) break;   // round >= 1 here: the last launched round saw no interface change
            batch = kRoundsPerCheck;
        }
        expect_rounds[dir] = round < kRoundsPerCheck ? kRoundsPerCheck : (round > 48 ? 48 : round);
    }
    return hipSuccess;
}

size_t velocity_long_state_bytes(bool f64, int B, int S)
{
    const int SC = f64 ? 64 * 16 : 64 * 40;   // the smallest super-chunk launch_velocity_long may pick
    const int nsc = (S + SC - 1) / SC;
    return (f64 ? 8 : 4) * ((size_t)2 * B * (nsc + 1) * 2 + (size_t)2 * B * nsc * 2) + 64;
}
size_t velocity_long_counter_bytes(bool f64, int B, int S)
{
    const int SC = f64 ? 64 * 16 : 64 * 40;   // as above: the smallest super-chunk
    const int nsc = (S + SC - 1) / SC;
    return sizeof(int) * ((size_t)B + 2 * (nsc + 2)) + 64;
}

hipError_t launch_velocity_long(hipStream_t st, bool f64, bool io64, int B, int S, const double c[6], double sv, double ev,
                                const double *meta, const void *curv, const void *dth, void *vel, uint32_t *flags,
                                void *ufwd, void *state, int *counters, void *vhi)
{
    // super-chunk = 512, 128 or 64 threads x 16 samples (fp64): few long rows (config 2: one) are cut finer so that the
    // chip has more workgroups to run and a super-round is shorter
    if (f64) {
        const long blocks512 = (long)B * ((S + 512 * 16 - 1) / (512 * 16));
        const int t64 = blocks512 < 256 ? 64 : (blocks512 < 1024 ? 128 : 512);
#define VAP_LONG64(IO_, T_) velocity_long_t<double, IO_, 16, T_, 2>(st, B, S, c, sv, ev, meta, curv, dth, vel, flags, ufwd, state, counters, vhi)
        if (io64) return t64 == 64 ? VAP_LONG64(double, 64) : (t64 == 128 ? VAP_LONG64(double, 128) : VAP_LONG64(double, 512));
        return t64 == 64 ? VAP_LONG64(float, 64) : (t64 == 128 ? VAP_LONG64(float, 128) : VAP_LONG64(float, 512));
#undef VAP_LONG64
    }
    // super-chunk = 256 or 64 threads x 40 samples: few long rows (config 2: one) are cut finer so that the
    // chip has more workgroups to run and a super-round is shorter
    const long blocks256 = (long)B * ((S + 256 * 40 - 1) / (256 * 40));
    if (blocks256 < 512)
        return velocity_long_t<float, float, 40, 64, 2>(st, B, S, c, sv, ev, meta, curv, dth, vel, flags, ufwd, state, counters, nullptr);
    return velocity_long_t<float, float, 40, 256, 2>(st, B, S, c, sv, ev, meta, curv, dth, vel, flags, ufwd, state, counters, nullptr);
}

// K5c': one launch per direction, interfaces handed on by look-back (k_velocity_chase).
//   state    [2][B][nsc] records of 64 bytes (zeroed per call: tag 0 = nothing published)
//   counters [B] dup flags | [2] tickets
template <typename R, typename IO, int L>
static hipError_t velocity_chase_t(hipStream_t st, int B, int S, const double c[6], double sv, double ev, const double *meta,
                                   const void *curv, const void *dth, void *vel, uint32_t *flags, void *ufwd, void *state,
                                   int *counters, void *vhi)
{
    constexpr int SC = 64 * L;
    const int nsc = (S + SC - 1) / SC;
    const R s = (R)sv, e = (R)ev;
    const size_t lds = sizeof(R) * ((size_t)64 * L + 64 + 8);
    const size_t rec_bytes = (size_t)B * nsc * kChaseRecGranules * 8;
    unsigned long long *rec = (unsigned long long *)state;
    int *dup = counters;
    unsigned int *ticket = (unsigned int *)(counters + B);
    hipError_t err;
    if ((err = hipMemsetAsync(state, 0, 2 * rec_bytes, st)) != hipSuccess) return err;
    if ((err = hipMemsetAsync(counters, 0, sizeof(int) * ((size_t)B + 2), st)) != hipSuccess) return err;
    const unsigned int grid = (unsigned int)((size_t)B * nsc);
    // developer knob: VAP_CHASE_STATS=1 prints the timeline of the super-chunks (synchronises!)
    static const bool want_stats = getenv("VAP_CHASE_STATS") != nullptr;
    long long *stats = nullptr;
    if (want_stats) {
        (void)hipMalloc(&stats, (size_t)2 * grid * 8 * sizeof(long long));
        (void)hipMemsetAsync(stats, 0, (size_t)2 * grid * 8 * sizeof(long long), st);
    }
    hipLaunchKernelGGL((k_velocity_chase<R, IO, L, false>), dim3(grid), dim3(64), lds, st, B, S, nsc, make_consts<R>(c), s * s,
                       e * e, meta, (const R *)curv, (const R *)dth, (R *)ufwd, (IO *)vel, rec, ticket, dup, flags, (R *)vhi,
                       stats);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL((k_velocity_chase<R, IO, L, true>), dim3(grid), dim3(64), lds, st, B, S, nsc, make_consts<R>(c), s * s,
                       e * e, meta, (const R *)curv, (const R *)dth, (R *)ufwd, (IO *)vel, rec + rec_bytes / 8, ticket + 1, dup,
                       flags, (R *)vhi, stats ? stats + (size_t)grid * 8 : nullptr);
    if (stats) {
        std::vector<long long> h((size_t)2 * grid * 8);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h.data(), stats, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
        (void)hipFree(stats);
        for (int dir = 0; dir < 2; dir++) {
            const long long *d = h.data() + (size_t)dir * grid * 8;
            long long t0 = 0, t_end = 0;
            for (unsigned int i = 0; i < grid; i++)
                if (d[i * 8]) {
                    if (!t0 || d[i * 8] < t0) t0 = d[i * 8];
                    if (d[i * 8 + 4] > t_end) t_end = d[i * 8 + 4];
                }
            double ev = 0, it = 0, po = 0;
            long long mev = 0, n = 0;
            for (unsigned int i = 0; i < grid; i++)
                if (d[i * 8]) {
                    n++;
                    ev += (double)d[i * 8 + 5];
                    it += (double)d[i * 8 + 6];
                    po += (double)d[i * 8 + 7];
                    if (d[i * 8 + 5] > mev) mev = d[i * 8 + 5];
                }
            fprintf(stderr, "[chase %s L=%d] %lld super-chunks, span %.1f us | per super-chunk: evaluations mean %.2f max %lld, inner rounds %.1f, look-backs %.1f\n",
                    dir ? "bwd" : "fwd", L, n, (double)(t_end - t0) * 0.01, ev / (double)n, mev, it / (double)n, po / (double)n);
            // the first path's timeline (us from the first start): where finality advanced by more than 3 us from one
            // super-chunk to the next, and every 1/8 of the row
            const int step = nsc >= 8 ? nsc / 8 : 1;
            long long prev_final = 0;
            for (int i = 0; i < nsc; i++) {
                const long long *r = d + (size_t)i * 8;
                if (!r[0]) continue;
                if (i % step == 0 || r[3] - prev_final > 300)
                    fprintf(stderr, "   idx %5d: start %7.1f derived %7.1f relaxed %7.1f final %7.1f (+%5.1f) end %7.1f | evals %lld rounds %lld polls %lld\n", i,
                            (double)(r[0] - t0) * 0.01, (double)(r[1] - t0) * 0.01, (double)(r[2] - t0) * 0.01, (double)(r[3] - t0) * 0.01,
                            (double)(r[3] - prev_final) * 0.01, (double)(r[4] - t0) * 0.01, r[5], r[6], r[7]);
                prev_final = r[3];
            }
        }
    }
    return hipGetLastError();
}

size_t velocity_chase_state_bytes(bool f64, int B, int S)
{
    const int SC = f64 ? 64 * 16 : 64 * 40;
    const int nsc = (S + SC - 1) / SC;
    return 2 * (size_t)B * nsc * kChaseRecGranules * 8 + 64;
}
size_t velocity_chase_counter_bytes(int B) { return sizeof(int) * ((size_t)B + 2) + 64; }

hipError_t launch_velocity_chase(hipStream_t st, bool f64, bool io64, int B, int S, const double c[6], double sv, double ev,
                                 const double *meta, const void *curv, const void *dth, void *vel, uint32_t *flags,
                                 void *ufwd, void *state, int *counters, void *vhi)
{
    if (f64) {
        if (io64) return velocity_chase_t<double, double, 16>(st, B, S, c, sv, ev, meta, curv, dth, vel, flags, ufwd, state, counters, vhi);
        return velocity_chase_t<double, float, 16>(st, B, S, c, sv, ev, meta, curv, dth, vel, flags, ufwd, state, counters, vhi);
    }
    return velocity_chase_t<float, float, 40>(st, B, S, c, sv, ev, meta, curv, dth, vel, flags, ufwd, state, counters, nullptr);
}

// K5b': many paths, fp32: one wave per path walks the row in windows of 64*L samples, one launch per
// window and direction (stream-ordered, no host synchronisation).  A window's incoming interface state
// is final when its launch starts, so every window is relaxed exactly once; a row of 5 registers per
// sample no longer has to stay resident, so eight paths share a CU instead of two.
size_t velocity_windows_state_bytes(int B, int S)
{
    const int nsc = (S + 64 * 40 - 1) / (64 * 40);
    return 4 * ((size_t)2 * B * (nsc + 1) * 2 + (size_t)2 * B * nsc * 2) + 64;
}

hipError_t launch_velocity_windows(hipStream_t st, int B, int S, const double c[6], double sv, double ev,
                                   const double *meta, const void *curv, const void *dth, void *vel, uint32_t *flags,
                                   void *ufwd, void *state, int *counters)
{
    using R = float;
    constexpr int L = 40, T = 64, SC = T * L;
    const int nsc = (S + SC - 1) / SC;
    const R s = (R)sv, e = (R)ev;
    const size_t lds = sizeof(R) * ((size_t)T * L + T + 8);
    R *bnd = (R *)state;
    R *used = bnd + (size_t)2 * B * (nsc + 1) * 2;
    R *outst = used + (size_t)B * nsc * 2;
    int *dup = counters, *changed = counters + B;
    hipError_t err;
    if ((err = hipMemsetAsync(counters, 0, sizeof(int) * ((size_t)B + 8), st)) != hipSuccess) return err;
    hipLaunchKernelGGL(k_dup_scan<R>, dim3(8, B), dim3(256), 0, st, B, S, make_consts<R>(c), meta, (const R *)curv,
                       (const R *)dth, dup);
    for (int sc = 0; sc < nsc; sc++)
        hipLaunchKernelGGL((k_velocity_long<R, R, L, T, 2, false>), dim3(1, B), dim3(T), lds, st, S, nsc, 0, sc,
                           make_consts<R>(c), s * s, e * e, meta, (const R *)curv, (const R *)dth, (R *)ufwd, (R *)vel, bnd,
                           used, outst, dup, changed, flags, (R *)nullptr);
    for (int sc = nsc - 1; sc >= 0; sc--)
        hipLaunchKernelGGL((k_velocity_long<R, R, L, T, 2, true>), dim3(1, B), dim3(T), lds, st, S, nsc, 0, sc,
                           make_consts<R>(c), s * s, e * e, meta, (const R *)curv, (const R *)dth, (R *)ufwd, (R *)vel, bnd,
                           used, outst, dup, changed, flags, (R *)nullptr);
    return hipGetLastError();
}

}  // namespace vap
