// vap_conflict_shifts.hip — robot-to-robot clearance as a function of the start shift (vap_conflict_shifts).
//
// vap_footprint_conflicts answers for one shift_rows; a caller who asks "how long must I wait" needs a whole window of
// them.  This file sweeps the window in one pass over rows that are packed once.  Definitions: include/vap.h.
//
// Three steps on the context's stream:
//   pack     vap_conflict.hip's k_conflict_pack on each side's OWN rows (shift 0, a horizon of the side's capacity):
//            {cx, cy, cos, sin} per row and a bounding circle per 64 rows.  The same kernel on the same rows: every packed
//            value, and so every row clearance, is the existing call's number.
//   sweep    a workgroup (one wave) owns one A route and a band of up to 64 shifts, a lane per shift, and takes the
//            route's partners one after another.  Per pair it walks the instants t in blocks of 64, aligned to 64 so that
//            a block of instants is one packed block of A.  Instant t poses A at row t and O at row t - s, each index
//            clamped into its side's rows where the hold bits say so; the lane's examined instants are one interval
//            [tb, te) (vap.h), so the five pieces of the minimum (the diagonal and the four held edges) are one walk.
//            Instants at which BOTH indices are clamped repeat the pose pair of a neighbouring examined instant and are
//            never walked: the walk covers [0, n_a) and [s_lo, s_hi + n_o) only, which bounds it for any shift.
//              stage   the A block and the O band it meets, 64 + (band - 1) step rows, in LDS;
//              block   one test of A's block circle against the O blocks of the band, with the largest running minimum
//                      of the band, discards the block for all shifts at once;
//              rows    per (instant, shift) the bounding-circle bound against the lane's running minimum (the slack rule
//                      of vap_conflict.hip).  A skipped row's clearance exceeds the running minimum, so it could not have
//                      changed the table; "blocked" is read off the table, so the margin needs no threshold of its own;
//              exact   survivors are queued in LDS and tested 64 at a time, a lane per queued (instant, shift), whatever
//                      lanes they came from: neighbouring shifts rarely agree on which instants survive, and a wave that
//                      ran the exact pair whenever one lane needed it would run it almost always.  A result goes to its
//                      shift's running minimum with an integer LDS atomic-min on an order-preserving key: the minimum of
//                      a set does not depend on the order, so the outputs do not depend on scheduling.
//            The running minimum is seeded with four exactly tested instants spread over the lane's interval.
//            The lane writes the table entry, the band's blocked bits (one atomic OR of a word) and folds the pair into
//            the route's minimum and blocked bits.
//   finalise a thread per pair and per route scans its blocked bits in ascending order for first and safe.
//
// Scratch: the two packs, (Ba capP_a + Bo capP_o) x 32 B plus their block circles, and Ba (P + 1) ceil(n_shifts / 64)
// words of blocked bits.  Nothing grows with pairs x blocks x shifts.
//
// Kept here: the [tb, te) interval, the two runs of blocks, the seeds, the blocked bits, the finalise kernel.  The stage,
// the block test and the survivor queue are vap_band_sweep.h's; the row bound, the checks and the packing vap_conflict.h's.
#include "vap_band_sweep.h"

namespace vap {

// k_shift_sweep's static LDS: two footprints, the A block, the keys, the queue.  The staged O band follows it as dynamic
// LDS and is read 16 bytes at a time, so the static part must stay a multiple of 16.
constexpr size_t kShiftStaticLds = 2 * kFootMaxVerts * 8 * 8 + kConfBlock * 32 + kSweepLanes * 8 + kSweepQueue * 2;
static_assert(kShiftStaticLds % 16 == 0, "the dynamic LDS behind k_shift_sweep's statics must start 16-byte aligned");

struct ShiftArgs : ConfPacked {
    int matched, P, hold;
    long shift_lo;
    int step, n_shifts;
    const int *base;          // [Ba] or null
    int band, nbands, nwords; // shifts per workgroup (a power of two <= 64), bands per route, bit words per window
    double margin;
    double *table, *route_table;
    unsigned long long *pair_bits, *route_bits;   // null: not needed
};

__global__ __launch_bounds__(kSweepLanes) void k_shift_sweep(ConfFoot fa, ConfFoot fo, ShiftArgs g)
{
    __shared__ double sfa[kFootMaxVerts * 8], sfo[kFootMaxVerts * 8];
    __shared__ __attribute__((aligned(16))) double stage_a[kConfBlock * 4];
    __shared__ unsigned long long s_key[kSweepLanes];
    __shared__ unsigned short s_queue[kSweepQueue];
    extern __shared__ __attribute__((aligned(16))) double stage_o[];     // [64 + (band - 1) step][4]

    const int lane = threadIdx.x;
    sweep_load_feet(sfa, sfo, fa, fo, lane);
    const int ia = blockIdx.x / g.nbands, gi = blockIdx.x % g.nbands;
    const int k0 = gi * g.band, k = k0 + lane;
    const int nb = min(g.band, g.n_shifts - k0);             // live lanes of this band
    const bool live = lane < nb;
    const long n_a = conf_count(g.a, ia);
    const long s0 = g.shift_lo + (g.base ? (long)g.base[ia] : 0L);
    const long s_lo = s0 + (long)k0 * g.step, s_hi = s_lo + (long)(nb - 1) * g.step;
    const long s = s_lo + (long)(live ? lane : 0) * g.step;
    const int off_o = live ? (nb - 1 - lane) * g.step : 0;   // the lane's O row of instant tt sits at stage slot tt + off_o
    const int nq = kConfBlock + (nb - 1) * g.step;           // staged O rows
    const int na = fa.n, no = fo.n;
    const double radii = fa.R + fo.R;
    const double *pa = g.pack_a + (size_t)ia * (size_t)g.Tpa * 4;
    const double *qa_all = g.blk_a + (size_t)ia * (size_t)g.nblk_a * 4;
    __syncthreads();

    double rbest = INFINITY;
    bool rblocked = false;
#pragma unroll 1
    for (int p = 0; p < g.P; p++) {
        const int io = g.matched ? ia : p;
        const long n_o = conf_count(g.o, io);
        const size_t pair = (size_t)ia * (size_t)g.P + (size_t)p;
        if (!(n_a > 0 && n_o > 0)) {                         // an invalid pair: NaN, and no bits
            if (g.table && live) g.table[pair * (size_t)g.n_shifts + (size_t)k] = NAN;
            continue;
        }
        const double *po = g.pack_o + (size_t)io * (size_t)g.Tpo * 4;
        const double *qo_all = g.blk_o + (size_t)io * (size_t)g.nblk_o * 4;
        // the lane's examined instants [tb, te)
        long tb = s < 0 ? s : 0, te = n_a > n_o + s ? n_a : n_o + s;
        if (!(g.hold & VAP_HOLD_A_FIRST)) tb = tb > 0 ? tb : 0;
        if (!(g.hold & VAP_HOLD_A_LAST)) te = te < n_a ? te : n_a;
        if (!(g.hold & VAP_HOLD_O_FIRST)) tb = tb > s ? tb : s;
        if (!(g.hold & VAP_HOLD_O_LAST)) te = te < n_o + s ? te : n_o + s;
        const bool some = live && tb < te;
        const long T0 = wave_min(some ? tb : LONG_MAX), T1 = wave_max(some ? te : LONG_MIN);

        double best = INFINITY;
        if (some && g.cull) {
#pragma unroll 1
            for (int q = 0; q < 4; q++) {
                const long t = tb + ((te - tb) * (2 * q + 1)) / 8;
                const double c = pair_at(sfa, na, sfo, no, pa + (size_t)clampl(t, 0, n_a - 1) * 4, po + (size_t)clampl(t - s, 0, n_o - 1) * 4);
                if (c < best) best = c;
            }
        }
        s_key[lane] = conf_key(best);
        SweepQueue queue{sfa, sfo, stage_a, stage_o, s_queue, na, no, lane};
        // entry (tt, l): lane l's O row of instant tt sits at stage slot tt + (nb - 1 - l) step; the lane's own minimum
        const auto slot_of = [&](int tt, int l) { return tt + (nb - 1 - l) * g.step; };
        const auto key_of = [&](int, int l) { return &s_key[l]; };
        const auto own_min = [&]() { return conf_unkey(s_key[lane]); };

        // up to two runs of 64-instant blocks: A's own rows and the O band's own rows, inside what any lane examines
        long seg[2][2];
        int nseg = 0;
        if (T0 < T1) {
            const long x1 = T0 > 0 ? T0 : 0, y1 = T1 < n_a ? T1 : n_a;
            const long x2 = T0 > s_lo ? T0 : s_lo, y2 = T1 < s_hi + n_o ? T1 : s_hi + n_o;
            if (x1 < y1) { seg[nseg][0] = floordiv64(x1); seg[nseg][1] = floordiv64(y1 - 1); nseg++; }
            if (x2 < y2) { seg[nseg][0] = floordiv64(x2); seg[nseg][1] = floordiv64(y2 - 1); nseg++; }
            if (nseg == 2) {
                if (seg[1][0] < seg[0][0]) {
                    const long a0 = seg[0][0], a1 = seg[0][1];
                    seg[0][0] = seg[1][0]; seg[0][1] = seg[1][1];
                    seg[1][0] = a0; seg[1][1] = a1;
                }
                if (seg[1][0] <= seg[0][1]) {                // they share a block: one run
                    seg[0][1] = seg[0][1] > seg[1][1] ? seg[0][1] : seg[1][1];
                    nseg = 1;
                }
            }
        }
#pragma unroll 1
        for (int sg = 0; sg < nseg; sg++) {
#pragma unroll 1
            for (long m = seg[sg][0]; m <= seg[sg][1]; m++) {
                const long t0 = m * kConfBlock;
                const int lo_l = some ? (int)clampl(tb - t0, 0, kConfBlock) : 0, hi_l = some ? (int)clampl(te - t0, 0, kConfBlock) : 0;
                const bool mine = lo_l < hi_l;
                const int lo_u = wave_min(mine ? lo_l : kConfBlock), hi_u = wave_max(mine ? hi_l : 0);
                if (lo_u >= hi_u) continue;
                if (g.cull) {
                    // A's block circle against every O block the band's rows of this block lie in
                    const double thr = wave_max(mine ? best : -INFINITY);
                    const double *qa = qa_all + (size_t)clampl(m, 0, g.nblk_a - 1) * 4;
                    const long b0 = clampl(floordiv64(t0 - s_hi), 0, g.nblk_o - 1), b1 = clampl(floordiv64(t0 + kConfBlock - 1 - s_lo), 0, g.nblk_o - 1);
                    if (!band_needs_block(g, radii, thr, qa, qo_all, b0, b1, lane)) continue;
                }
                sweep_stage(stage_a, pa, t0, n_a, stage_o, po, t0 - s_hi, n_o, nq, lane);
                __syncthreads();
#pragma unroll 1
                for (int tt = lo_u; tt < hi_u; tt++) {
                    bool cand = tt >= lo_l && tt < hi_l;
                    if (cand && g.cull) {
                        const double2 a01 = *(const double2 *)(stage_a + tt * 4);
                        const double2 o01 = *(const double2 *)(stage_o + (size_t)(tt + off_o) * 4);
                        cand = !row_culled(g, radii, best, a01.x, a01.y, o01.x, o01.y);
                    }
                    queue.push(cand, tt, best, slot_of, key_of, own_min);
                }
                queue.close(best, slot_of, key_of, own_min);
            }
        }
        __syncthreads();
        best = conf_unkey(s_key[lane]);
        __syncthreads();                                     // s_key is rewritten for the next pair
        const bool have = some && best != INFINITY;          // a finite clearance was examined
        const bool blocked = have && best < g.margin;
        if (g.table && live) g.table[pair * (size_t)g.n_shifts + (size_t)k] = have ? best : NAN;
        if (g.pair_bits) {
            const unsigned long long w = __ballot(blocked);
            if (lane == 0 && w) atomicOr(g.pair_bits + pair * (size_t)g.nwords + (size_t)(k0 / 64), w << (k0 % 64));
        }
        if (have) {
            rbest = best < rbest ? best : rbest;
            rblocked = rblocked || blocked;
        }
    }
    if (g.route_table && live) g.route_table[(size_t)ia * (size_t)g.n_shifts + (size_t)k] = rbest != INFINITY ? rbest : NAN;
    if (g.route_bits) {
        const unsigned long long w = __ballot(live && rblocked);
        if (lane == 0 && w) atomicOr(g.route_bits + (size_t)ia * (size_t)g.nwords + (size_t)(k0 / 64), w << (k0 % 64));
    }
}

// first and safe of one window of blocked bits, in ascending order of the shift
__device__ __forceinline__ void shift_scan(const unsigned long long *bits, int n_shifts, int min_run, int scan, int &first, int &safe)
{
    int run = 0, up = -1, down = -1;
    safe = 0;
#pragma unroll 1
    for (int k = 0; k < n_shifts; k++) {
        if ((bits[k >> 6] >> (k & 63)) & 1ull) {
            run = 0;
            continue;
        }
        safe++;
        if (run < INT_MAX) run++;
        if (run >= min_run) {
            if (up < 0) up = k - (min_run - 1);
            down = k;
        }
    }
    first = scan > 0 ? up : down;
}

// threads 0 .. Ba P - 1: the pairs; the next Ba: the routes
__global__ __launch_bounds__(64) void k_shift_finalise(ShiftArgs g, int min_run, int scan, int *__restrict__ pair_first,
                                                       int *__restrict__ pair_safe, int *__restrict__ route_first,
                                                       int *__restrict__ route_safe)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x, n_pairs = (size_t)g.a.B * (size_t)g.P;
    if (i < n_pairs) {
        if (!pair_first && !pair_safe) return;
        const int ia = (int)(i / (size_t)g.P), io = g.matched ? ia : (int)(i % (size_t)g.P);
        int first = -1, safe = 0;
        if (conf_count(g.a, ia) > 0 && conf_count(g.o, io) > 0) shift_scan(g.pair_bits + i * (size_t)g.nwords, g.n_shifts, min_run, scan, first, safe);
        if (pair_first) pair_first[i] = first;
        if (pair_safe) pair_safe[i] = safe;
    } else if (i < n_pairs + (size_t)g.a.B) {
        if (!route_first && !route_safe) return;
        const int ia = (int)(i - n_pairs);
        int first = -1, safe = 0;
        if (conf_count(g.a, ia) > 0) shift_scan(g.route_bits + (size_t)ia * (size_t)g.nwords, g.n_shifts, min_run, scan, first, safe);
        if (route_first) route_first[ia] = first;
        if (route_safe) route_safe[ia] = safe;
    }
}

}  // namespace vap

extern "C" {

int vap_conflict_shifts(vap_ctx *ctx, int pairing, int hold, double margin, int shift_lo, int shift_step, int n_shifts,
                        const int *d_shift_base, int min_run, int scan,
                        int Ba, long cap_a, const double *d_rows_a, const int *d_counts_a, int stride_a, int n_foot_a,
                        const double *h_foot_a,
                        int Bo, long cap_o, const double *d_rows_o, const int *d_counts_o, int stride_o, int n_foot_o,
                        const double *h_foot_o,
                        double *d_table, int *d_pair_first, int *d_pair_safe,
                        double *d_route_table, int *d_route_first, int *d_route_safe)
{
    using namespace vap;
    const ConfInput a{Ba, cap_a, d_rows_a, d_counts_a, stride_a, n_foot_a, h_foot_a}, o{Bo, cap_o, d_rows_o, d_counts_o, stride_o, n_foot_o, h_foot_o};
    const bool matched = pairing == VAP_CONFLICT_MATCHED;
    if (pairing != VAP_CONFLICT_ALL_PAIRS && !matched) return vap_fail(VAP_ERR_INVALID, "unknown pairing %d", pairing);
    if (hold < 0 || hold > 15) return vap_fail(VAP_ERR_INVALID, "hold must be a mask of the four VAP_HOLD bits (got %d)", hold);
    if (n_shifts < 1 || shift_step < 1 || min_run < 1)
        return vap_fail(VAP_ERR_INVALID, "n_shifts, shift_step and min_run must be >= 1 (got %d, %d, %d)", n_shifts, shift_step, min_run);
    if (scan != 1 && scan != -1) return vap_fail(VAP_ERR_INVALID, "scan must be +1 or -1 (got %d)", scan);
    VAP_TRY(conf_check_shape("Ba", a, o));
    VAP_TRY(conf_check_sides(a, o, Bo, matched, margin, false, "null rows / counts"));
    if (n_shifts > VAP_CONFLICT_SHIFTS_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "%d shifts above VAP_CONFLICT_SHIFTS_MAX = %d", n_shifts, VAP_CONFLICT_SHIFTS_MAX);
    if (cap_a > INT_MAX || cap_o > INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld above %d rows", cap_a > cap_o ? cap_a : cap_o, INT_MAX);
    VAP_TRY(vap_set_device(ctx));
    if (Ba == 0 || Bo == 0) return VAP_OK;
    if (!d_table && !d_pair_first && !d_pair_safe && !d_route_table && !d_route_first && !d_route_safe) return VAP_OK;

    const ConfHorizon ha = conf_horizon(cap_a), ho = conf_horizon(cap_o);
    const SweepBands bands = sweep_bands(n_shifts, shift_step, 0);
    VAP_TRY(sweep_fits(ctx, bands, shift_step, kShiftStaticLds, "shifts"));
    const int nwords = (n_shifts + 63) / 64;
    const long grid = (long)Ba * bands.nbands, grid_pack = (long)Ba * ha.groups > (long)Bo * ho.groups ? (long)Ba * ha.groups : (long)Bo * ho.groups;
    const size_t P = matched ? 1 : (size_t)Bo, n_fin = (size_t)Ba * P + (size_t)Ba;
    if (grid > INT_MAX || grid_pack > INT_MAX || (n_fin + 63) / 64 > (size_t)INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "%d x %d routes, %d shifts: too many workgroups for one launch", Ba, Bo, n_shifts);

    ConfFoot fa, fo;
    ShiftArgs g;
    VAP_TRY(conf_pack_sides(ctx, a, o, 0, ha, ho, fa, fo, g));
    const bool want_pair = d_pair_first || d_pair_safe, want_route = d_route_first || d_route_safe;
    const size_t pair_words = want_pair ? (size_t)Ba * P * (size_t)nwords : 0, route_words = want_route ? (size_t)Ba * (size_t)nwords : 0;
    if (pair_words + route_words) {
        VAP_TRY(ctx->ensure(ctx->conf_part, (pair_words + route_words) * 8));
        HIP_TRY(hipMemsetAsync(ctx->conf_part.ptr, 0, (pair_words + route_words) * 8, ctx->stream));
    }
    g.matched = matched ? 1 : 0;
    g.P = (int)P;
    g.hold = hold;
    g.shift_lo = shift_lo;
    g.step = shift_step;
    g.n_shifts = n_shifts;
    g.base = d_shift_base;
    g.band = bands.band;
    g.nbands = bands.nbands;
    g.nwords = nwords;
    g.margin = margin;
    g.table = d_table;
    g.route_table = d_route_table;
    g.pair_bits = want_pair ? (unsigned long long *)ctx->conf_part.ptr : nullptr;
    g.route_bits = want_route ? (unsigned long long *)ctx->conf_part.ptr + pair_words : nullptr;

    hipLaunchKernelGGL(k_shift_sweep, dim3((unsigned)grid), dim3(kSweepLanes), bands.lds, ctx->stream, fa, fo, g);
    if (want_pair || want_route)
        hipLaunchKernelGGL(k_shift_finalise, dim3((unsigned)((n_fin + 63) / 64)), dim3(64), 0, ctx->stream, g, min_run, scan, d_pair_first,
                           d_pair_safe, d_route_first, d_route_safe);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
