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
#include "vap_conflict.h"

namespace vap {

constexpr int kShiftLanes = 64;                  // one wave: a lane per shift of the band
constexpr long kShiftStageRows = 1024;           // O rows staged at most (32 KB); the band halves until it fits
constexpr int kShiftQueue = 128;                 // ring of queued (instant, shift) survivors
// k_shift_sweep's static LDS: two footprints, the A block, the keys, the queue.  The staged O band follows it as dynamic
// LDS and is read 16 bytes at a time, so the static part must stay a multiple of 16.
constexpr size_t kShiftStaticLds = 2 * kFootMaxVerts * 8 * 8 + kConfBlock * 32 + kShiftLanes * 8 + kShiftQueue * 2;
static_assert(kShiftStaticLds % 16 == 0, "the dynamic LDS behind k_shift_sweep's statics must start 16-byte aligned");

struct ShiftArgs {
    const double *pack_a, *pack_o, *blk_a, *blk_o;
    ConfSide a, o;
    long Tpa, Tpo;            // packed rows per route
    int nblk_a, nblk_o;
    int matched, P, hold, cull;
    long shift_lo;
    int step, n_shifts;
    const int *base;          // [Ba] or null
    int band, nbands, nwords; // shifts per workgroup (a power of two <= 64), bands per route, bit words per window
    double margin, slack;
    double *table, *route_table;
    unsigned long long *pair_bits, *route_bits;   // null: not needed
};

__device__ __forceinline__ long floordiv64(long x) { return x >= 0 ? x / 64 : -((63 - x) / 64); }
__device__ __forceinline__ long clampl(long x, long lo, long hi) { return x < lo ? lo : (x > hi ? hi : x); }

// an order-preserving map of doubles (no NaN) to unsigned 64-bit keys, and back
__device__ __forceinline__ unsigned long long shift_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double shift_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

template <typename T>
__device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kShiftLanes) void k_shift_sweep(ConfFoot fa, ConfFoot fo, ShiftArgs g)
{
    __shared__ double sfa[kFootMaxVerts * 8], sfo[kFootMaxVerts * 8];
    __shared__ __attribute__((aligned(16))) double stage_a[kConfBlock * 4];
    __shared__ unsigned long long s_key[kShiftLanes];
    __shared__ unsigned short s_queue[kShiftQueue];
    extern __shared__ __attribute__((aligned(16))) double stage_o[];     // [64 + (band - 1) step][4]

    const int lane = threadIdx.x;
    sfa[lane] = fa.v[lane];
    sfa[lane + 64] = fa.v[lane + 64];
    sfo[lane] = fo.v[lane];
    sfo[lane + 64] = fo.v[lane + 64];
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
                const double *ra = pa + (size_t)clampl(t, 0, n_a - 1) * 4, *ro = po + (size_t)clampl(t - s, 0, n_o - 1) * 4;
                const double2 a01 = *(const double2 *)ra, a23 = *(const double2 *)(ra + 2);
                const double2 o01 = *(const double2 *)ro, o23 = *(const double2 *)(ro + 2);
                const double c = pair_clearance(sfa, na, sfo, no, a01.x, a01.y, a23.x, a23.y, o01.x, o01.y, o23.x, o23.y);
                if (c < best) best = c;
            }
        }
        s_key[lane] = shift_key(best);
        int qn = 0, head = 0;                                // the queue's fill and first entry (uniform)

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
                    const double ax = qa[0], ay = qa[1], ar = qa[2];
                    const long b0 = clampl(floordiv64(t0 - s_hi), 0, g.nblk_o - 1), b1 = clampl(floordiv64(t0 + kConfBlock - 1 - s_lo), 0, g.nblk_o - 1);
                    bool need = false;
#pragma unroll 1
                    for (long b = b0 + lane; b <= b1; b += kShiftLanes) {
                        const double *qo = qo_all + (size_t)b * 4;
                        const double ox = qo[0], oy = qo[1];
                        const double slack = g.slack + kCullSlack * (fabs(ax) + fabs(ay) + fabs(ox) + fabs(oy) + ar + qo[2]);
                        need = need || !conf_culled(thr + slack + radii + ar + qo[2], ox - ax, oy - ay);
                    }
                    if (!__any(need)) continue;
                }
                // stage: every lane has left the previous block's rows (a flush ends with a barrier)
                {
                    const double *src = pa + (size_t)clampl(t0 + lane, 0, n_a - 1) * 4;
                    *(double2 *)(stage_a + lane * 4) = *(const double2 *)src;
                    *(double2 *)(stage_a + lane * 4 + 2) = *(const double2 *)(src + 2);
                }
#pragma unroll 1
                for (int q = lane; q < nq; q += kShiftLanes) {
                    const double *src = po + (size_t)clampl(t0 - s_hi + q, 0, n_o - 1) * 4;
                    *(double2 *)(stage_o + (size_t)q * 4) = *(const double2 *)src;
                    *(double2 *)(stage_o + (size_t)q * 4 + 2) = *(const double2 *)(src + 2);
                }
                __syncthreads();
                // the exact pair of `n` queued survivors, a lane each; afterwards every lane's running minimum is current
                auto flush = [&](int n) {
                    __syncthreads();
                    if (lane < n) {
                        const int e = s_queue[(head + lane) & (kShiftQueue - 1)];
                        const int tt = e & 63, l = e >> 6;
                        const double *ra = stage_a + tt * 4, *ro = stage_o + (size_t)(tt + (nb - 1 - l) * g.step) * 4;
                        const double2 a01 = *(const double2 *)ra, a23 = *(const double2 *)(ra + 2);
                        const double2 o01 = *(const double2 *)ro, o23 = *(const double2 *)(ro + 2);
                        const double c = pair_clearance(sfa, na, sfo, no, a01.x, a01.y, a23.x, a23.y, o01.x, o01.y, o23.x, o23.y);
                        if (c == c) atomicMin(&s_key[l], shift_key(c));      // a NaN clearance takes part in nothing
                    }
                    __syncthreads();
                    best = shift_unkey(s_key[lane]);
                };
#pragma unroll 1
                for (int tt = lo_u; tt < hi_u; tt++) {
                    bool cand = tt >= lo_l && tt < hi_l;
                    if (cand && g.cull) {
                        const double2 a01 = *(const double2 *)(stage_a + tt * 4);
                        const double2 o01 = *(const double2 *)(stage_o + (size_t)(tt + off_o) * 4);
                        const double slack = g.slack + kCullSlack * (fabs(a01.x) + fabs(a01.y) + fabs(o01.x) + fabs(o01.y));
                        cand = !conf_culled(best + slack + radii, o01.x - a01.x, o01.y - a01.y);
                    }
                    const unsigned long long mask = __ballot(cand);
                    if (mask) {
                        if (cand) {
                            const int pos = head + qn + __popcll(mask & ((1ull << lane) - 1ull));
                            s_queue[pos & (kShiftQueue - 1)] = (unsigned short)(tt | (lane << 6));
                        }
                        qn += __popcll(mask);
                        if (qn >= kShiftLanes) {
                            flush(kShiftLanes);
                            head = (head + kShiftLanes) & (kShiftQueue - 1);
                            qn -= kShiftLanes;
                        }
                    }
                }
                flush(qn);                                   // the rows leave LDS with this block; also the barrier
                head = 0;
                qn = 0;
            }
        }
        __syncthreads();
        best = shift_unkey(s_key[lane]);
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
    if (pairing != VAP_CONFLICT_ALL_PAIRS && pairing != VAP_CONFLICT_MATCHED) return vap_fail(VAP_ERR_INVALID, "unknown pairing %d", pairing);
    if (hold < 0 || hold > 15) return vap_fail(VAP_ERR_INVALID, "hold must be a mask of the four VAP_HOLD bits (got %d)", hold);
    if (n_shifts < 1 || shift_step < 1 || min_run < 1)
        return vap_fail(VAP_ERR_INVALID, "n_shifts, shift_step and min_run must be >= 1 (got %d, %d, %d)", n_shifts, shift_step, min_run);
    if (scan != 1 && scan != -1) return vap_fail(VAP_ERR_INVALID, "scan must be +1 or -1 (got %d)", scan);
    if (Ba < 0 || Bo < 0 || cap_a < 0 || cap_o < 0)
        return vap_fail(VAP_ERR_INVALID, "bad shape Ba=%d cap_a=%ld Bo=%d cap_o=%ld", Ba, cap_a, Bo, cap_o);
    if (stride_a < 1 || stride_o < 1) return vap_fail(VAP_ERR_INVALID, "count strides must be >= 1 (got %d, %d)", stride_a, stride_o);
    if (pairing == VAP_CONFLICT_MATCHED && Ba != Bo) return vap_fail(VAP_ERR_INVALID, "matched pairing needs Ba == Bo (got %d, %d)", Ba, Bo);
    if ((Ba > 0 && (!d_counts_a || (cap_a > 0 && !d_rows_a))) || (Bo > 0 && (!d_counts_o || (cap_o > 0 && !d_rows_o))))
        return vap_fail(VAP_ERR_INVALID, "null rows / counts");
    if (!std::isfinite(margin)) return vap_fail(VAP_ERR_INVALID, "margin must be finite");
    if (!h_foot_a || !h_foot_o) return vap_fail(VAP_ERR_INVALID, "null footprint");
    VAP_TRY(check_convex(h_foot_a, n_foot_a, "footprint", 0));
    VAP_TRY(check_convex(h_foot_o, n_foot_o, "footprint", 1));
    if (n_shifts > VAP_CONFLICT_SHIFTS_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "%d shifts above VAP_CONFLICT_SHIFTS_MAX = %d", n_shifts, VAP_CONFLICT_SHIFTS_MAX);
    if (cap_a > INT_MAX || cap_o > INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld above %d rows", cap_a > cap_o ? cap_a : cap_o, INT_MAX);
    VAP_TRY(vap_set_device(ctx));
    if (Ba == 0 || Bo == 0) return VAP_OK;
    if (!d_table && !d_pair_first && !d_pair_safe && !d_route_table && !d_route_first && !d_route_safe) return VAP_OK;

    const bool matched = pairing == VAP_CONFLICT_MATCHED;
    const long nblk_a = cap_a > 0 ? (cap_a + kConfBlock - 1) / kConfBlock : 1, nblk_o = cap_o > 0 ? (cap_o + kConfBlock - 1) / kConfBlock : 1;
    const long Tpa = nblk_a * kConfBlock, Tpo = nblk_o * kConfBlock;
    const int groups_a = (int)((nblk_a + 3) / 4), groups_o = (int)((nblk_o + 3) / 4);
    // the band: the most shifts, a power of two, whose O rows fit the stage
    int band = kShiftLanes;
    while (band > 1 && kConfBlock + (long)(band - 1) * shift_step > kShiftStageRows) band /= 2;
    const int nbands = (n_shifts + band - 1) / band, nwords = (n_shifts + 63) / 64;
    const int nb_max = band < n_shifts ? band : n_shifts;
    const size_t lds = (size_t)(kConfBlock + (long)(nb_max - 1) * shift_step) * 32;
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) lds_max = 0;
    const size_t avail = lds_max > 0 && lds_max < 64 * 1024 ? (size_t)lds_max : (size_t)64 * 1024;
    if (lds + kShiftStaticLds > avail)
        return vap_fail(VAP_ERR_UNSUPPORTED, "a band of %d shifts at step %d needs %zu bytes of LDS; the device gives a workgroup %zu",
                        band, shift_step, lds + kShiftStaticLds, avail);
    const long grid = (long)Ba * nbands, grid_pack = (long)Ba * groups_a > (long)Bo * groups_o ? (long)Ba * groups_a : (long)Bo * groups_o;
    const size_t P = matched ? 1 : (size_t)Bo, n_fin = (size_t)Ba * P + (size_t)Ba;
    if (grid > INT_MAX || grid_pack > INT_MAX || (n_fin + 63) / 64 > (size_t)INT_MAX)
        return vap_fail(VAP_ERR_UNSUPPORTED, "%d x %d routes, %d shifts: too many workgroups for one launch", Ba, Bo, n_shifts);

    VAP_TRY(ctx->ensure(ctx->conf_pack_a, (size_t)Ba * (size_t)Tpa * 32));
    VAP_TRY(ctx->ensure(ctx->conf_pack_o, (size_t)Bo * (size_t)Tpo * 32));
    VAP_TRY(ctx->ensure(ctx->conf_blk_a, (size_t)Ba * (size_t)nblk_a * 32));
    VAP_TRY(ctx->ensure(ctx->conf_blk_o, (size_t)Bo * (size_t)nblk_o * 32));
    const bool want_pair = d_pair_first || d_pair_safe, want_route = d_route_first || d_route_safe;
    const size_t pair_words = want_pair ? (size_t)Ba * P * (size_t)nwords : 0, route_words = want_route ? (size_t)Ba * (size_t)nwords : 0;
    if (pair_words + route_words) {
        VAP_TRY(ctx->ensure(ctx->conf_part, (pair_words + route_words) * 8));
        HIP_TRY(hipMemsetAsync(ctx->conf_part.ptr, 0, (pair_words + route_words) * 8, ctx->stream));
    }

    ConfFoot fa, fo;
    conf_foot(h_foot_a, n_foot_a, fa);
    conf_foot(h_foot_o, n_foot_o, fo);
    ShiftArgs g;
    g.a = ConfSide{d_rows_a, d_counts_a, cap_a, stride_a, Ba, 0};
    g.o = ConfSide{d_rows_o, d_counts_o, cap_o, stride_o, Bo, 0};
    g.pack_a = (const double *)ctx->conf_pack_a.ptr;
    g.pack_o = (const double *)ctx->conf_pack_o.ptr;
    g.blk_a = (const double *)ctx->conf_blk_a.ptr;
    g.blk_o = (const double *)ctx->conf_blk_o.ptr;
    g.Tpa = Tpa;
    g.Tpo = Tpo;
    g.nblk_a = (int)nblk_a;
    g.nblk_o = (int)nblk_o;
    g.matched = matched ? 1 : 0;
    g.P = (int)P;
    g.hold = hold;
    g.cull = ctx->footprint_cull;
    g.shift_lo = shift_lo;
    g.step = shift_step;
    g.n_shifts = n_shifts;
    g.base = d_shift_base;
    g.band = band;
    g.nbands = nbands;
    g.nwords = nwords;
    g.margin = margin;
    g.slack = kCullSlack * (1.0 + fa.R + fo.R);
    g.table = d_table;
    g.route_table = d_route_table;
    g.pair_bits = want_pair ? (unsigned long long *)ctx->conf_part.ptr : nullptr;
    g.route_bits = want_route ? (unsigned long long *)ctx->conf_part.ptr + pair_words : nullptr;

    hipLaunchKernelGGL(k_conflict_pack, dim3((unsigned)((long)Ba * groups_a)), dim3(256), 0, ctx->stream, g.a, fa.cx, fa.cy, Tpa,
                       (int)nblk_a, groups_a, (double *)ctx->conf_pack_a.ptr, (double *)ctx->conf_blk_a.ptr);
    hipLaunchKernelGGL(k_conflict_pack, dim3((unsigned)((long)Bo * groups_o)), dim3(256), 0, ctx->stream, g.o, fo.cx, fo.cy, Tpo,
                       (int)nblk_o, groups_o, (double *)ctx->conf_pack_o.ptr, (double *)ctx->conf_blk_o.ptr);
    hipLaunchKernelGGL(k_shift_sweep, dim3((unsigned)grid), dim3(kShiftLanes), lds, ctx->stream, fa, fo, g);
    if (want_pair || want_route)
        hipLaunchKernelGGL(k_shift_finalise, dim3((unsigned)((n_fin + 63) / 64)), dim3(64), 0, ctx->stream, g, min_run, scan, d_pair_first,
                           d_pair_safe, d_route_first, d_route_safe);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
