// vap_schedule.hip — a routine's waits against its partners, every slot at once (vap_schedule_tables,
// vap_schedule_solve).
//
// vap_conflict_shifts delays a whole route.  A chained routine stands still at every slot boundary anyway, so it may wait
// there for free: this file answers how many rows to wait in front of every slot so that the whole routine clears every
// partner and finishes as early as possible.  Definitions: include/vap.h.
//
// vap_schedule_tables, three steps on the context's stream:
//   pack     vap_conflict.hip's k_conflict_pack on each side's own rows (shift 0), exactly as vap_conflict_shifts runs
//            it: every packed value, and so every clearance, is that call's number.
//   sweep    a workgroup (one wave) owns one routine and a band of up to 64 cumulative delays, a lane per delay k, and
//            takes the partners one after another.  Per partner ONE walk over the routine's 64-row blocks: row i meets
//            the partner's pose at instant i + k q, so the lanes of a band read one staged run of 64 + (band - 1) q
//            partner rows.  Every (segment, delay) minimum is an order-preserving key in LDS: a row's result goes to
//            the key of the segment its row lies in, so a block may hold any number of segment boundaries and the walk
//            never restarts.  Culling and the exact test are k_shift_sweep's: the bounding-circle bound against the
//            lane's running minimum of the row's segment, survivors queued in LDS and tested 64 at a time whatever lanes
//            they came from, an integer atomic-min per result (a minimum does not depend on the order: two calls give
//            the same bits, culling on or off).  A segment's minimum is seeded with three exactly tested rows of it.
//              tail   the routine parked at its last row meets partner rows n + k q .. n_o - 1: the lanes' ranges are
//                     nested suffixes of one run, so each of those rows is tested ONCE per band (a lane per row), a
//                     suffix minimum inside the wave, and lane k reads the entry its range starts at.
//              holds  wait[m][u]: the hold pose of slot m against q instants per partner, a lane per u; the instants
//                     behind the partner's last row repeat its parked pose and are tested once.
//   The same workgroup writes both tables; band 0 writes n_seg and the flag.
//
// vap_schedule_solve: one wave per routine, a lane per 64 delays.  ok() bits come from ballots over coalesced reads of
// the tables; G_m = F_{m-1} | (G_m << 1 & ok(wait)) is a carry chain: Kogge-Stone inside a lane's word, the words'
// generate / propagate bits as two ballots, the same recurrence on those two words for the carries.  F_m and ok(wait_m)
// stay in LDS, bit-packed (M C / 4 bytes), for the backtrack, which is a handful of ballots per slot.
//
// Scratch: the two packs and their block circles.  Nothing grows with R x M x C beside the caller's two tables.
//
// Kept here: the slot map, the per-segment keys and seeds, the parked tail, the hold poses, the solve.  The stage, the
// block test and the survivor queue are vap_band_sweep.h's; the row bound, the checks and the packing vap_conflict.h's.
#include "vap_band_sweep.h"

namespace vap {

// k_schedule_sweep's static LDS: two footprints, the A block, the tail's suffix minima, the slot map, the queue, the rows'
// segments.  The keys and the staged partner band follow it as dynamic LDS, read 16 bytes at a time.
constexpr size_t kSchedStaticLds =
    (2 * kFootMaxVerts * 8 * 8 + kConfBlock * 32 + kSweepLanes * 8 + (VAP_TIMELINE_MAX_LEGS + 1) * 4 + kSweepQueue * 2 + kConfBlock + 15) / 16 * 16;

struct SchedArgs : ConfPacked {
    const int *seg_start;     // [R][M]
    int M, C, q;
    int band, nbands;         // delays per workgroup (a power of two <= 64), bands per routine
    double *move, *wait;      // [R][M][C]; null: not asked for
    int *n_seg;
    uint32_t *flags;
};

__global__ __launch_bounds__(kSweepLanes) void k_schedule_sweep(ConfFoot fa, ConfFoot fo, SchedArgs g)
{
    __shared__ double sfa[kFootMaxVerts * 8], sfo[kFootMaxVerts * 8];
    __shared__ __attribute__((aligned(16))) double stage_a[kConfBlock * 4];
    __shared__ double s_suf[kSweepLanes];
    __shared__ int s_b[VAP_TIMELINE_MAX_LEGS + 1];
    __shared__ unsigned short s_queue[kSweepQueue];
    __shared__ unsigned char s_seg_of[kConfBlock];
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
    unsigned long long *s_key = s_dyn;                                   // [M][64]: the (segment, delay) minima
    double *stage_o = (double *)(s_dyn + (size_t)g.M * kSweepLanes);     // [64 + (band - 1) q][4]

    const int lane = threadIdx.x;
    sweep_load_feet(sfa, sfo, fa, fo, lane);
    const int r = blockIdx.x / g.nbands, gi = blockIdx.x % g.nbands;
    const int k0 = gi * g.band, k = k0 + lane;
    const int nb = min(g.band, g.C - k0);                    // live lanes of this band
    const bool live = lane < nb;
    const int M = g.M;
    const long n = conf_count(g.a, r);
    const size_t out0 = (size_t)r * (size_t)M * (size_t)g.C + (size_t)k;

    // the slot map: S used slots, and whether they are a legal cut of the routine's rows
    const int mine = lane < M ? g.seg_start[(size_t)r * M + lane] : -1;
    const unsigned long long used = __ballot(mine >= 0);
    const int S = __popcll(used);
    if (lane < M) s_b[lane] = mine;
    __syncthreads();
    bool wrong = false;
    if (lane < S) wrong = lane == 0 ? mine != 0 : !(mine > s_b[lane - 1]);
    if (S > 0 && lane == S - 1) wrong = wrong || !((long)mine < n);
    const bool bad = S > 0 && n > 0 && (used != (S >= 64 ? ~0ull : (1ull << S) - 1ull) || __any(wrong));
    if (n == 0 || S == 0 || bad) {                           // uniform: the whole workgroup leaves
        if (live)
            for (int m = 0; m < M; m++) {
                if (g.move) g.move[out0 + (size_t)m * g.C] = NAN;
                if (g.wait) g.wait[out0 + (size_t)m * g.C] = NAN;
            }
        if (gi == 0 && lane == 0) {
            if (g.n_seg) g.n_seg[r] = 0;
            if (bad && g.flags) atomicOr(g.flags + r, VAP_FLAG_BAD_ROUTE);
        }
        return;
    }
    __syncthreads();
    if (lane == 0) s_b[S] = (int)n;
    for (int m = 0; m < M; m++) s_key[m * kSweepLanes + lane] = conf_key(INFINITY);
    __syncthreads();

    const int q = g.q;
    const long kq = (long)(live ? k : k0) * q;               // the lane's delay in rows
    const int off_o = live ? lane * q : 0;                   // the lane's partner row of block row tt sits at stage slot tt + off_o
    const int nq = kConfBlock + (nb - 1) * q;                // staged partner rows
    const int na = fa.n, no = fo.n;
    const double radii = fa.R + fo.R;
    const double *pa = g.pack_a + (size_t)r * (size_t)g.Tpa * 4;
    const double *qa_all = g.blk_a + (size_t)r * (size_t)g.nblk_a * 4;
    const int nblocks = (int)((n + kConfBlock - 1) / kConfBlock);

    if (g.move) {
#pragma unroll 1
        for (int p = 0; p < g.o.B; p++) {
            const long n_o = conf_count(g.o, p);
            if (n_o == 0) continue;                          // takes part in nothing
            const double *po = g.pack_o + (size_t)p * (size_t)g.Tpo * 4;
            const double *qo_all = g.blk_o + (size_t)p * (size_t)g.nblk_o * 4;
            if (g.cull && live) {                            // seeds: three rows of every segment, tested exactly
#pragma unroll 1
                for (int m = 0; m < S; m++) {
                    const long b0 = s_b[m], len = s_b[m + 1] - b0;
                    double best = conf_unkey(s_key[m * kSweepLanes + lane]);
#pragma unroll 1
                    for (int j = 0; j < 3; j++) {
                        const long i = b0 + (len * (2 * j + 1)) / 6;
                        const double c = pair_at(sfa, na, sfo, no, pa + (size_t)i * 4, po + (size_t)clampl(i + kq, 0, n_o - 1) * 4);
                        if (c < best) best = c;
                    }
                    s_key[m * kSweepLanes + lane] = conf_key(best);
                }
            }
            __syncthreads();
            int m_lo = 0;                                    // the segment of the block's first row (uniform)
#pragma unroll 1
            for (int blk = 0; blk < nblocks; blk++) {
                const long t0 = (long)blk * kConfBlock;
                const int hi = (int)(n - t0 < kConfBlock ? n - t0 : kConfBlock);
                while (s_b[m_lo + 1] <= t0) m_lo++;
                int m_hi = m_lo;
                while (s_b[m_hi + 1] < t0 + hi) m_hi++;
                if (g.cull) {
                    // A's block circle against every partner block the band's instants of this block lie in
                    double worst = -INFINITY;
                    if (live)
                        for (int m = m_lo; m <= m_hi; m++) {
                            const double v = conf_unkey(s_key[m * kSweepLanes + lane]);
                            worst = v > worst ? v : worst;
                        }
                    const double thr = wave_max(worst);
                    const long b0 = clampl(t0 + (long)k0 * q, 0, n_o - 1) / kConfBlock;
                    const long b1 = clampl(t0 + kConfBlock - 1 + (long)(k0 + nb - 1) * q, 0, n_o - 1) / kConfBlock;
                    if (!band_needs_block(g, radii, thr, qa_all + (size_t)blk * 4, qo_all, b0, b1, lane)) continue;
                }
                sweep_stage(stage_a, pa, t0, n, stage_o, po, t0 + (long)k0 * q, n_o, nq, lane);
                {
                    int m = m_lo;                            // the segment of the lane's row of the block
                    while (m < m_hi && s_b[m + 1] <= t0 + lane) m++;
                    s_seg_of[lane] = (unsigned char)m;
                }
                __syncthreads();
                int m_cur = m_lo;                            // the segment the walk is in (uniform)
                SweepQueue queue{sfa, sfo, stage_a, stage_o, s_queue, na, no, lane};
                // entry (tt, l): lane l's partner row of block row tt sits at stage slot tt + l q; the key of tt's segment;
                // the lane's minimum of the segment the walk is in
                const auto slot_of = [&](int tt, int l) { return tt + l * q; };
                const auto key_of = [&](int tt, int l) { return &s_key[s_seg_of[tt] * kSweepLanes + l]; };
                const auto own_min = [&]() { return conf_unkey(s_key[m_cur * kSweepLanes + lane]); };
                double best = own_min();
#pragma unroll 1
                for (int tt = 0; tt < hi; tt++) {
                    const int m = s_seg_of[tt];
                    if (m != m_cur) {                        // uniform: the walk passes a segment boundary
                        m_cur = m;
                        best = own_min();
                    }
                    bool cand = live;
                    if (cand && g.cull) {
                        const double2 a01 = *(const double2 *)(stage_a + tt * 4);
                        const double2 o01 = *(const double2 *)(stage_o + (size_t)(tt + off_o) * 4);
                        cand = !row_culled(g, radii, best, a01.x, a01.y, o01.x, o01.y);
                    }
                    queue.push(cand, tt, best, slot_of, key_of, own_min);
                }
                queue.close(best, slot_of, key_of, own_min);
            }
            // the tail: parked at row n - 1 against partner rows n + k q .. n_o - 1, each tested once per band
            const long j_lo = n + (long)k0 * q;
            if (j_lo < n_o) {
                const double *ra = pa + (size_t)(n - 1) * 4;
                const double ax = ra[0], ay = ra[1];
                unsigned long long *key = s_key + (S - 1) * kSweepLanes + lane;
#pragma unroll 1
                for (long j0 = j_lo; j0 < n_o; j0 += kSweepLanes) {
                    const long j = j0 + lane;
                    const double thr = wave_max(live ? conf_unkey(*key) : -INFINITY);
                    double c = INFINITY;
                    if (j < n_o) {
                        const double *ro = po + (size_t)j * 4;
                        const bool test = !g.cull || !row_culled(g, radii, thr, ax, ay, ro[0], ro[1]);
                        if (test) {
                            const double e = pair_at(sfa, na, sfo, no, ra, ro);
                            if (e == e) c = e;
                        }
                    }
#pragma unroll
                    for (int off = 1; off < kSweepLanes; off <<= 1) {    // c = the minimum over lanes lane .. 63
                        const double o = __shfl_down(c, off);
                        if (lane + off < kSweepLanes && o < c) c = o;
                    }
                    __syncthreads();
                    s_suf[lane] = c;
                    __syncthreads();
                    const long st = n + kq - j0;             // where the lane's range starts inside this chunk
                    if (live && st < kSweepLanes) {
                        const double v = s_suf[st > 0 ? st : 0];
                        if (v < conf_unkey(*key)) *key = conf_key(v);
                    }
                }
            }
            __syncthreads();
        }
        if (live)
            for (int m = 0; m < M; m++) {
                const double v = m < S ? conf_unkey(s_key[m * kSweepLanes + lane]) : INFINITY;
                g.move[out0 + (size_t)m * g.C] = v != INFINITY ? v : NAN;
            }
    }

    if (g.wait && live) {                                    // no barrier below
#pragma unroll 1
        for (int m = 0; m < M; m++) {
            double best = INFINITY;
            if (m < S) {
                const long b = s_b[m];
                const double *ra = pa + (size_t)(b > 0 ? b - 1 : 0) * 4;
                const double ax = ra[0], ay = ra[1];
#pragma unroll 1
                for (int p = 0; p < g.o.B; p++) {
                    const long n_o = conf_count(g.o, p);
                    if (n_o == 0) continue;
                    const double *po = g.pack_o + (size_t)p * (size_t)g.Tpo * 4;
#pragma unroll 1
                    for (long t = b + kq, te = t + q; t < te; t++) {
                        const double *ro = po + (size_t)(t < n_o - 1 ? t : n_o - 1) * 4;
                        const bool test = !g.cull || !row_culled(g, radii, best, ax, ay, ro[0], ro[1]);
                        if (test) {
                            const double c = pair_at(sfa, na, sfo, no, ra, ro);
                            if (c < best) best = c;          // false for NaN
                        }
                        if (t >= n_o - 1) break;             // the partner is parked: the instants behind repeat this pose
                    }
                }
            }
            g.wait[out0 + (size_t)m * g.C] = best != INFINITY ? best : NAN;
        }
    }
    if (gi == 0 && lane == 0 && g.n_seg) g.n_seg[r] = S;
}

// ---- the schedule of one routine from its tables -----------------------------------------------------------------------
// v | carries: v[k] |= v[k - 1] & p[k], within a 64-bit word; pp[k] = p[0] & .. & p[k] (a carry into bit 0 reaches bit k)
__device__ __forceinline__ void sched_chain(unsigned long long &v, unsigned long long p, unsigned long long &pp)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        v |= p & (v << s);
        p &= (p << s) | ((1ull << s) - 1ull);
    }
    pp = p;
}

__global__ __launch_bounds__(64) void k_schedule_solve(int M, int C, int q, double margin, const double *__restrict__ move,
                                                       const double *__restrict__ wait, const int *__restrict__ n_seg,
                                                       int *__restrict__ delay_rows, int *__restrict__ total_rows,
                                                       double *__restrict__ clearance)
{
    extern __shared__ unsigned long long s_bits[];           // F [M][nw], then ok(wait) [M][nw]
    const int r = blockIdx.x, lane = threadIdx.x;
    const int nw = (C + 63) / 64;
    unsigned long long *s_f = s_bits, *s_w = s_bits + (size_t)M * nw;
    int S = n_seg[r];
    S = S < 0 ? 0 : (S > M ? M : S);
    const double *mv = move + (size_t)r * (size_t)M * (size_t)C, *wt = wait + (size_t)r * (size_t)M * (size_t)C;
    const unsigned long long in_window = lane < nw ? (lane == nw - 1 && (C & 63) ? (1ull << (C & 63)) - 1ull : ~0ull) : 0ull;

    unsigned long long f = lane == 0 ? 1ull : 0ull;          // F_{-1}: cumulative delay 0 only
#pragma unroll 1
    for (int m = 0; m < S; m++) {
        unsigned long long okm = 0, okw = 0;                 // the lane's words of ok(move[m]), ok(wait[m])
#pragma unroll 1
        for (int w = 0; w < nw; w++) {
            const int kk = w * 64 + lane;
            const bool in = kk < C;
            const unsigned long long bm = __ballot(in && !(mv[(size_t)m * C + (in ? kk : 0)] < margin));
            const unsigned long long bw = __ballot(in && !(wt[(size_t)m * C + (in ? kk : 0)] < margin));
            if (w == lane) {
                okm = bm;
                okw = bw;
            }
        }
        // p[k] = ok(wait[m][k - 1]): the wait bits one up, across the words
        const unsigned long long below = __shfl_up(okw, 1);
        const unsigned long long p = ((okw << 1) | (lane > 0 ? below >> 63 : 0ull)) & in_window;
        unsigned long long gm = f, pp;
        sched_chain(gm, p, pp);
        // the carries between the words: the same recurrence on the words' top bits
        unsigned long long carry = __ballot((gm >> 63) & 1ull), through = __ballot((pp >> 63) & 1ull), unused;
        sched_chain(carry, through, unused);
        if (lane > 0 && ((carry >> (lane - 1)) & 1ull)) gm |= pp;
        f = gm & okm & in_window;
        if (lane < nw) {
            s_f[(size_t)m * nw + lane] = f;
            s_w[(size_t)m * nw + lane] = okw;
        }
    }
    __syncthreads();

    // backtrack: the smallest k_{S-1}; then, slot by slot downwards, the largest k_{m-1} that reaches k_m
    int kk = -1;
    if (S > 0) {
        const unsigned long long any = __ballot(f != 0ull);
        if (any) {
            const int w = __ffsll((long long)any) - 1;
            kk = w * 64 + __ffsll((long long)s_f[(size_t)(S - 1) * nw + w]) - 1;
        }
    }
    const bool have = kk >= 0;
    if (total_rows && lane == 0) total_rows[r] = have ? kk * q : -1;
    double best = INFINITY;
    if (have) {
#pragma unroll 1
        for (int m = S - 1; m >= 0; m--) {
            // lo: one behind the last blocked wait of slot m below kk; the bits of a word below kk
            const long rel = (long)kk - (long)lane * 64;
            const unsigned long long under = rel >= 64 ? ~0ull : (rel <= 0 ? 0ull : (1ull << rel) - 1ull);
            const unsigned long long blocked = lane < nw ? ~s_w[(size_t)m * nw + lane] & under : 0ull;
            const unsigned long long anyb = __ballot(blocked != 0ull);
            int lo = 0;
            if (anyb) {
                const int w = 63 - __clzll((long long)anyb);
                const long rw = (long)kk - (long)w * 64;
                const unsigned long long uw = rw >= 64 ? ~0ull : (1ull << rw) - 1ull;
                lo = w * 64 + 64 - __clzll((long long)(~s_w[(size_t)m * nw + w] & uw));
            }
            int prev = 0;                                    // k_{m-1}; k_{-1} = 0
            if (m > 0) {
                const long rl = (long)lo - (long)lane * 64, rh = (long)kk + 1 - (long)lane * 64;
                const unsigned long long from = rl <= 0 ? ~0ull : (rl >= 64 ? 0ull : ~((1ull << rl) - 1ull));
                const unsigned long long upto = rh >= 64 ? ~0ull : (rh <= 0 ? 0ull : (1ull << rh) - 1ull);
                const unsigned long long c = lane < nw ? s_f[(size_t)(m - 1) * nw + lane] & from & upto : 0ull;
                const unsigned long long anyc = __ballot(c != 0ull);  // never empty: F_m[kk] was derived from such a bit
                const int w = anyc ? 63 - __clzll((long long)anyc) : 0;
                const long rlw = (long)lo - (long)w * 64, rhw = (long)kk + 1 - (long)w * 64;
                const unsigned long long fw = rlw <= 0 ? ~0ull : (rlw >= 64 ? 0ull : ~((1ull << rlw) - 1ull));
                const unsigned long long uw = rhw >= 64 ? ~0ull : (rhw <= 0 ? 0ull : (1ull << rhw) - 1ull);
                const unsigned long long cw = s_f[(size_t)(m - 1) * nw + w] & fw & uw;
                prev = cw ? w * 64 + 63 - __clzll((long long)cw) : lo;
            }
            if (delay_rows && lane == 0) delay_rows[(size_t)r * M + m] = (kk - prev) * q;
            if (clearance) {
                for (int u = prev + lane; u < kk; u += 64) {
                    const double v = wt[(size_t)m * C + u];
                    if (v < best) best = v;
                }
                if (lane == 0) {
                    const double v = mv[(size_t)m * C + kk];
                    if (v < best) best = v;
                }
            }
            kk = prev;
        }
    }
    if (delay_rows)
        for (int m = (have ? S : 0) + lane; m < M; m += 64) delay_rows[(size_t)r * M + m] = have ? 0 : -1;
    if (clearance) {
        best = wave_min(best);
        if (lane == 0) clearance[r] = best != INFINITY ? best : NAN;
    }
}

}  // namespace vap

extern "C" {

int vap_schedule_tables(vap_ctx *ctx, int n_delays, int delay_step,
                        int R, long cap_a, const double *d_rows_a, const int *d_counts_a, int stride_a, int n_foot_a,
                        const double *h_foot_a, int M, const int *d_seg_start,
                        int Bo, long cap_o, const double *d_rows_o, const int *d_counts_o, int stride_o, int n_foot_o,
                        const double *h_foot_o,
                        double *d_move, double *d_wait, int *d_n_seg, uint32_t *d_flags)
{
    using namespace vap;
    const ConfInput a{R, cap_a, d_rows_a, d_counts_a, stride_a, n_foot_a, h_foot_a}, o{Bo, cap_o, d_rows_o, d_counts_o, stride_o, n_foot_o, h_foot_o};
    if (M < 1 || n_delays < 1 || delay_step < 1)
        return vap_fail(VAP_ERR_INVALID, "M, n_delays and delay_step must be >= 1 (got %d, %d, %d)", M, n_delays, delay_step);
    VAP_TRY(conf_check_shape("R", a, o));
    // no pairing and no margin here; without routines nothing of the partners is read
    VAP_TRY(conf_check_sides(a, o, R > 0 ? Bo : 0, false, 0.0, R > 0 && !d_seg_start, "null rows / counts / segment starts"));
    if (M > VAP_TIMELINE_MAX_LEGS) return vap_fail(VAP_ERR_UNSUPPORTED, "%d slots above VAP_TIMELINE_MAX_LEGS = %d", M, VAP_TIMELINE_MAX_LEGS);
    if (n_delays > VAP_SCHEDULE_MAX_DELAYS)
        return vap_fail(VAP_ERR_UNSUPPORTED, "%d delays above VAP_SCHEDULE_MAX_DELAYS = %d", n_delays, VAP_SCHEDULE_MAX_DELAYS);
    if ((long)(n_delays - 1) * delay_step > INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "a window of %d delays at step %d ends above %d rows", n_delays, delay_step, INT_MAX);
    if (cap_a > INT_MAX || cap_o > INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld above %d rows", cap_a > cap_o ? cap_a : cap_o, INT_MAX);
    const ConfHorizon ha = conf_horizon(cap_a), ho = conf_horizon(cap_o);
    const SweepBands bands = sweep_bands(n_delays, delay_step, (size_t)M * kSweepLanes * 8);
    const long grid = (long)R * bands.nbands, grid_pack = (long)R * ha.groups > (long)Bo * ho.groups ? (long)R * ha.groups : (long)Bo * ho.groups;
    if (grid > INT_MAX || grid_pack > INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "%d routines, %d partners, %d delays: too many workgroups for one launch", R, Bo, n_delays);
    VAP_TRY(vap_set_device(ctx));
    if (R == 0) return VAP_OK;
    if (!d_move && !d_wait && !d_n_seg && !d_flags) return VAP_OK;
    VAP_TRY(sweep_fits(ctx, bands, delay_step, kSchedStaticLds, "delays"));

    ConfFoot fa, fo;
    SchedArgs g;
    VAP_TRY(conf_pack_sides(ctx, a, o, 0, ha, ho, fa, fo, g));
    g.seg_start = d_seg_start;
    g.M = M;
    g.C = n_delays;
    g.q = delay_step;
    g.band = bands.band;
    g.nbands = bands.nbands;
    g.move = d_move;
    g.wait = d_wait;
    g.n_seg = d_n_seg;
    g.flags = d_flags;
    hipLaunchKernelGGL(k_schedule_sweep, dim3((unsigned)grid), dim3(kSweepLanes), bands.lds, ctx->stream, fa, fo, g);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

int vap_schedule_solve(vap_ctx *ctx, int R, int M, int n_delays, int delay_step, double margin, const double *d_move,
                       const double *d_wait, const int *d_n_seg, int *d_delay_rows, int *d_total_rows, double *d_clearance)
{
    using namespace vap;
    if (M < 1 || n_delays < 1 || delay_step < 1)
        return vap_fail(VAP_ERR_INVALID, "M, n_delays and delay_step must be >= 1 (got %d, %d, %d)", M, n_delays, delay_step);
    if (R < 0) return vap_fail(VAP_ERR_INVALID, "bad shape R=%d", R);
    if (!std::isfinite(margin)) return vap_fail(VAP_ERR_INVALID, "margin must be finite");
    if (R > 0 && (!d_move || !d_wait || !d_n_seg)) return vap_fail(VAP_ERR_INVALID, "null tables / segment counts");
    if (M > VAP_TIMELINE_MAX_LEGS) return vap_fail(VAP_ERR_UNSUPPORTED, "%d slots above VAP_TIMELINE_MAX_LEGS = %d", M, VAP_TIMELINE_MAX_LEGS);
    if (n_delays > VAP_SCHEDULE_MAX_DELAYS)
        return vap_fail(VAP_ERR_UNSUPPORTED, "%d delays above VAP_SCHEDULE_MAX_DELAYS = %d", n_delays, VAP_SCHEDULE_MAX_DELAYS);
    if ((long)(n_delays - 1) * delay_step > INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "a window of %d delays at step %d ends above %d rows", n_delays, delay_step, INT_MAX);
    VAP_TRY(vap_set_device(ctx));
    if (R == 0) return VAP_OK;
    if (!d_delay_rows && !d_total_rows && !d_clearance) return VAP_OK;
    const size_t lds = (size_t)2 * M * ((n_delays + 63) / 64) * 8;
    hipLaunchKernelGGL(k_schedule_solve, dim3((unsigned)R), dim3(64), lds, ctx->stream, M, n_delays, delay_step, margin, d_move, d_wait,
                       d_n_seg, d_delay_rows, d_total_rows, d_clearance);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
