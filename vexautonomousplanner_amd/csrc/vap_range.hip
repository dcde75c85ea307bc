// vap_range.hip — what a wall-facing distance sensor reads along time-domain rows (vap_range_readings; include/vap.h).
//
// A ray cast: per row and sensor the nearest intersection of one ray — from the sensor's mount point, along its beam, both
// posed with the row — with the field walls, the scene's convex polygons and circles, and the partners' posed footprints; the
// status of that reading (valid, out of window, too oblique, blocked by a partner ...); per route and sensor the rows per
// status and the smallest and largest valid range; per route and channel (each sensor, "x observable", "y observable") the
// valid rows and the longest run of rows without a valid reading.
//
//   k_range_rows<LDS>  a workgroup per tile of a route's rows (kRangeThreads rows a step, `iters` steps a tile), a lane per row:
//                      one sincos per row, then sensors x elements.  The element loops are uniform across the wave: the
//                      packed scene is read at wave-uniform addresses — from LDS when the whole block fits kRangeLdsDoubles
//                      (LDS = true), from the global block otherwise — and an element is skipped when no lane of the wave
//                      needs it (its bounding circle cannot hold a strictly nearer hit on any lane's ray).  An edge is
//                      decided from signs and products; the one division is paid by a hit that can still win.  Per-reading
//                      outputs are staged in LDS and written [row][sensor]-contiguous.  Per tile one record: counts per
//                      status (ballots), min / max valid range (wave shuffles, then LDS), and per channel the gap record
//                      (rows ok, leading run, trailing run, longest run, its first row) built from the waves' ballot masks.
//   k_range_finish     a workgroup of 64 per route: the tiles' records in row order.  The gap record's combine is associative,
//                      the counts are integers and the ranges a min / max, so the tiling cannot change a result.
// No float atomics; the integer atomics are LDS counters.  Two calls give the same bits, culling on and off too.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "vap_footprint.h"
#include "vap_raycast.h"

namespace vap {
namespace {

constexpr int kRangeThreads = 256;
constexpr int kRangeWaves = kRangeThreads / 64;
constexpr int kRangeMaxChan = kRangeMaxSens + 2;
constexpr int kRangeMaxPartners = 16;
constexpr int kRangeLdsDoubles = 2048;    // a packed scene of up to 16 KiB is staged in LDS, a larger one is read from global
constexpr int kRangePartInts = 128;       // per tile: counts [8][8], then the channels' records [10][5]
constexpr int kRangeChanAt = 64;
constexpr int kRangePartDbls = 16;        // per tile: min, max valid range [8][2]
constexpr int kRangeGridYMax = 65535;

// Packed block (fp64), vap_footprint.h's layouts: foot [n_foot_o][8] (the partners' footprint, body frame) | poly [n_poly][4] |
// pv [nv][8] | circ [n_circle][4].
struct RangeArgs {
    const double *rows;
    const int *counts;
    const double *scene;
    const double *rows_o;
    const int *counts_o;
    int stride, cap, b0, iters, tiles, n_sens;
    int n_dbl, o_poly, o_pv, o_circ;
    int n_poly, n_circle, n_foot_o, has_field, cull;
    int stride_o, cap_o, Bo, shift;
    double xmin, ymin, xmax, ymax, slack, foot_R;
    double sens[kRangeMaxSens][8];
    double *range, *cosi;
    int *code;
    double *part_d;
    int *part_i;
    int *status_counts;
    double *minmax;
    int *channels;
};

// Rows [row0, row0 + len) of one channel: rows ok, the not-ok runs at both ends (== len when no row is ok), the longest
// not-ok run and the first row of the earliest such run (-1: none).
struct Gap {
    int row0, len, n_ok, lead, trail, best, start;
};

// a, then b right behind it.  Associative; the earliest of equally long runs stays (a's, then the one across the seam).
__device__ inline Gap gap_combine(const Gap &a, const Gap &b)
{
    if (a.len == 0) return b;
    if (b.len == 0) return a;
    Gap c;
    c.row0 = a.row0;
    c.len = a.len + b.len;
    c.n_ok = a.n_ok + b.n_ok;
    c.lead = a.lead == a.len ? a.len + b.lead : a.lead;
    c.trail = b.trail == b.len ? b.len + a.trail : b.trail;
    c.best = a.best;
    c.start = a.start;
    const int mid = a.trail + b.lead;
    if (mid > c.best) { c.best = mid; c.start = a.row0 + a.len - a.trail; }
    if (b.best > c.best) { c.best = b.best; c.start = b.start; }
    return c;
}

// the record of rows row0 .. row0 + L - 1 (L in 1..64) from a wave's ballot of "ok", lane i = row row0 + i
__device__ inline Gap gap_of_mask(unsigned long long ok, int L, int row0)
{
    const unsigned long long low = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
    ok &= low;
    Gap g;
    g.row0 = row0;
    g.len = L;
    g.n_ok = __popcll(ok);
    if (ok == 0ull) {
        g.lead = g.trail = g.best = L;
        g.start = row0;
        return g;
    }
    g.lead = __ffsll((long long)ok) - 1;
    g.trail = L - 64 + __clzll((long long)ok);
    g.best = 0;
    g.start = -1;
    unsigned long long y = ~ok & low, last = 0ull;
    int k = 0;
    while (y) {             // after k rounds bit i is set iff rows i - k .. i are all not ok
        last = y;
        y &= y << 1;
        k++;
    }
    if (k) {
        g.best = k;
        g.start = row0 + (__ffsll((long long)last) - 1) - (k - 1);
    }
    return g;
}

// One reading: the ray from (ox, oy) along (ux, uy) at row r.  S: the packed block (LDS or global).
__device__ inline void cast_ray(const RangeArgs &g, const double *S, bool live, long r, double ox, double oy, double ux, double uy,
                                double &best, double &bcos, int &bface, int &bel)
{
    // 1-3. the wall, the polygons, the circles (vap_raycast.h)
    const double slack = ray_slack(g, ox, oy);
    cast_scene(g, S, live, ox, oy, ux, uy, slack, best, bcos, bface, bel);
    // 4. partners: partner o stands at its row clamp(r - shift, 0, n_o - 1); the ray goes into its body frame
#pragma unroll 1
    for (int o = 0; o < g.Bo; o++) {
        int n_o = g.counts_o[(size_t)o * g.stride_o];
        n_o = n_o < 0 ? 0 : (n_o > g.cap_o ? g.cap_o : n_o);
        if (n_o == 0) continue;
        long ro = r - (long)g.shift;
        ro = ro < 0 ? 0 : (ro > n_o - 1 ? n_o - 1 : ro);
        const double *P = g.rows_o + ((size_t)o * (size_t)g.cap_o + (size_t)ro) * 8;
        const double ph = P[4], px = P[6], py = P[7];
        if (g.cull && !__any(live && !ray_culled(ox, oy, ux, uy, best, slack, px, py, g.foot_R))) continue;
        // (sin and cos, not a second sincos: that call is not inlined here and its two results would go through scratch)
        const double s2 = sin(-ph), c2 = cos(-ph);
        const double dx = ox - px, dy = oy - py;
        const double qx = c2 * dx + s2 * dy, qy = c2 * dy - s2 * dx;
        const double vx = c2 * ux + s2 * uy, vy = c2 * uy - s2 * ux;
#pragma unroll 1
        for (int j = 0; j < g.n_foot_o; j++)
            edge_test(S + j * 8, qx, qy, vx, vy, j, g.n_poly + g.n_circle + o, best, bcos, bface, bel);
    }
}

template <bool LDS>
__global__ void __launch_bounds__(kRangeThreads) k_range_rows(RangeArgs g)
{
    extern __shared__ double s_dyn[];                          // [the packed block, if LDS][staged outputs, if asked for]
    __shared__ unsigned long long s_mask[kRangeWaves][kRangeMaxChan];
    __shared__ int s_cnt[kRangeMaxSens * 8];
    __shared__ double s_mm[kRangeWaves][kRangeMaxSens][2];
    const int b = g.b0 + blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ns = g.n_sens, nch = ns + 2;
    int n = g.counts[(size_t)b * g.stride];
    n = n < 0 ? 0 : (n > g.cap ? g.cap : n);
    const int tile_rows = g.iters * kRangeThreads;
    const int r_begin = blockIdx.x * tile_rows;
    const bool rows_out = g.range || g.cosi || g.code;
    if (r_begin >= n && !rows_out) return;                     // (the whole workgroup)
    const double *S = g.scene;
    double *stage = s_dyn;
    if (LDS) {
        if (r_begin < n)
            for (int i = t; i < g.n_dbl; i += kRangeThreads) s_dyn[i] = g.scene[i];
        S = s_dyn;
        stage = s_dyn + ((g.n_dbl + 1) & ~1);
    }
    double *st_range = stage, *st_cos = stage + kRangeThreads * ns;
    int *st_code = reinterpret_cast<int *>(stage + 2 * kRangeThreads * ns);
    if (t < kRangeMaxSens * 8) s_cnt[t] = 0;
    if (t < kRangeWaves * kRangeMaxSens * 2) (&s_mm[0][0][0])[t] = (t & 1) ? -INFINITY : INFINITY;
    Gap rec{0, 0, 0, 0, 0, 0, -1};                             // of channel t, in threads t < nch
    __syncthreads();
    for (int it = 0; it < g.iters; it++) {
        const int r0 = r_begin + it * kRangeThreads;
        if (r0 >= g.cap || (r0 >= n && !rows_out)) break;
        const int r = r0 + t;
        const bool live = r < n;
        if (r0 + wave * 64 < n) {                              // (the whole wave)
            double h = 0.0, x = 0.0, y = 0.0;
            if (live) {
                const double *row = g.rows + ((size_t)b * g.cap + r) * 8;
                h = row[4];
                x = row[6];
                y = row[7];
            }
            const bool bad = !(isfinite(h) && isfinite(x) && isfinite(y));
            double sn, c;
            sincos(-h, &sn, &c);
            bool xobs = false, yobs = false;
#pragma unroll 1
            for (int s = 0; s < ns; s++) {
                const double mx = g.sens[s][0], my = g.sens[s][1], bx = g.sens[s][2], by = g.sens[s][3];
                const double ox = x + (c * mx - sn * my), oy = y + (sn * mx + c * my);
                const double ux = c * bx - sn * by, uy = sn * bx + c * by;
                double best, bcos;
                int face, el;
                cast_ray(g, S, live && !bad, r, ox, oy, ux, uy, best, bcos, face, el);
                int status;
                if (bad) status = 6;
                else if (el == -2) status = 1;
                else if (el >= g.n_poly + g.n_circle) status = 5;
                else if (best < g.sens[s][4]) status = 2;
                else if (best > g.sens[s][5]) status = 3;
                else if (bcos < g.sens[s][6]) status = 4;
                else status = 0;
                if (bad || el == -2) { best = NAN; bcos = NAN; face = 0; el = -2; }
                const bool ok = live && status == 0;
                xobs |= ok && el == -1 && (face == 0 || face == 2);
                yobs |= ok && el == -1 && (face == 1 || face == 3);
                if (rows_out) {
                    st_range[t * ns + s] = best;
                    st_cos[t * ns + s] = bcos;
                    st_code[t * ns + s] = status | (face << 4) | ((el + 2) << 12);
                }
                const unsigned long long m_ok = __ballot(ok);
                for (int k = 0; k < 7; k++) {
                    const int cnt = __popcll(__ballot(live && status == k));
                    if (lane == 0 && cnt) atomicAdd(&s_cnt[s * 8 + k], cnt);
                }
                if (m_ok) {                                    // (the whole wave)
                    double lo = ok ? best : INFINITY, hi = ok ? best : -INFINITY;
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const double olo = __shfl_xor(lo, off), ohi = __shfl_xor(hi, off);
                        lo = olo < lo ? olo : lo;
                        hi = ohi > hi ? ohi : hi;
                    }
                    if (lane == 0) {
                        if (lo < s_mm[wave][s][0]) s_mm[wave][s][0] = lo;
                        if (hi > s_mm[wave][s][1]) s_mm[wave][s][1] = hi;
                    }
                }
                if (lane == 0) s_mask[wave][s] = m_ok;
            }
            const unsigned long long m_x = __ballot(xobs), m_y = __ballot(yobs);
            if (lane == 0) {
                s_mask[wave][ns] = m_x;
                s_mask[wave][ns + 1] = m_y;
            }
        }
        if (rows_out && !live) {                               // past the route's rows: NaN / -1 (past capacity: not written)
            for (int s = 0; s < ns; s++) {
                st_range[t * ns + s] = NAN;
                st_cos[t * ns + s] = NAN;
                st_code[t * ns + s] = -1;
            }
        }
        __syncthreads();
        if (rows_out) {
            const int nrow = g.cap - r0 < kRangeThreads ? g.cap - r0 : kRangeThreads;
            const int nval = nrow * ns;
            const size_t base = ((size_t)b * g.cap + r0) * ns;
            for (int i = t; i < nval; i += kRangeThreads) {
                if (g.range) g.range[base + i] = st_range[i];
                if (g.cosi) g.cosi[base + i] = st_cos[i];
                if (g.code) g.code[base + i] = st_code[i];
            }
        }
        if (t < nch) {
            for (int w = 0; w < kRangeWaves; w++) {
                const int w0 = r0 + w * 64;
                if (w0 >= n) break;
                rec = gap_combine(rec, gap_of_mask(s_mask[w][t], n - w0 < 64 ? n - w0 : 64, w0));
            }
        }
        __syncthreads();
    }
    if (r_begin >= n) return;
    const size_t p = (size_t)b * g.tiles + blockIdx.x;
    if (t < kRangeMaxSens * 8) g.part_i[p * kRangePartInts + t] = s_cnt[t];
    if (t < ns) {
        double lo = s_mm[0][t][0], hi = s_mm[0][t][1];
        for (int w = 1; w < kRangeWaves; w++) {
            lo = s_mm[w][t][0] < lo ? s_mm[w][t][0] : lo;
            hi = s_mm[w][t][1] > hi ? s_mm[w][t][1] : hi;
        }
        g.part_d[p * kRangePartDbls + t * 2] = lo;
        g.part_d[p * kRangePartDbls + t * 2 + 1] = hi;
    }
    if (t < nch) {
        int *o = g.part_i + p * kRangePartInts + kRangeChanAt + t * 5;
        o[0] = rec.n_ok;
        o[1] = rec.lead;
        o[2] = rec.trail;
        o[3] = rec.best;
        o[4] = rec.start;
    }
}

// A workgroup of 64 per route: the tiles' records in row order.
__global__ void __launch_bounds__(64) k_range_finish(RangeArgs g)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const int ns = g.n_sens, nch = ns + 2;
    int n = g.counts[(size_t)b * g.stride];
    n = n < 0 ? 0 : (n > g.cap ? g.cap : n);
    const int tile_rows = g.iters * kRangeThreads;
    const int nt = (int)(((long)n + tile_rows - 1) / tile_rows);
    const size_t p0 = (size_t)b * g.tiles;
    if (g.status_counts && t < ns * 8) {
        int sum = 0;
        for (int i = 0; i < nt; i++) sum += g.part_i[(p0 + i) * kRangePartInts + t];
        g.status_counts[(size_t)b * ns * 8 + t] = (t & 7) == 7 ? 0 : sum;
    }
    if (g.minmax && t < ns) {
        double lo = INFINITY, hi = -INFINITY;
        for (int i = 0; i < nt; i++) {
            const double l = g.part_d[(p0 + i) * kRangePartDbls + t * 2], h = g.part_d[(p0 + i) * kRangePartDbls + t * 2 + 1];
            lo = l < lo ? l : lo;
            hi = h > hi ? h : hi;
        }
        g.minmax[((size_t)b * ns + t) * 2] = lo == INFINITY ? NAN : lo;
        g.minmax[((size_t)b * ns + t) * 2 + 1] = hi == -INFINITY ? NAN : hi;
    }
    if (g.channels && t < nch) {
        Gap rec{0, 0, 0, 0, 0, 0, -1};
        for (int i = 0; i < nt; i++) {
            const int *q = g.part_i + (p0 + i) * kRangePartInts + kRangeChanAt + t * 5;
            const int r0 = i * tile_rows;
            rec = gap_combine(rec, Gap{r0, n - r0 < tile_rows ? n - r0 : tile_rows, q[0], q[1], q[2], q[3], q[4]});
        }
        int *o = g.channels + ((size_t)b * nch + t) * 5;
        o[0] = rec.n_ok;
        o[1] = rec.n_ok ? rec.lead : -1;
        o[2] = rec.n_ok ? rec.len - 1 - rec.trail : -1;
        o[3] = rec.best;
        o[4] = rec.best ? rec.start : -1;
    }
}

}  // namespace
}  // namespace vap

extern "C" {

int vap_range_readings(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride, int n_sens,
                       const double *h_sensors, const double *h_field, int n_poly, const int *h_poly_start, const double *h_poly_xy,
                       int n_circle, const double *h_circles, int Bo, long cap_o, const double *d_rows_o, const int *d_counts_o,
                       int stride_o, int n_foot_o, const double *h_foot_o, int shift_rows, double *d_range, double *d_cos_incidence,
                       int *d_code, int *d_status_counts, double *d_range_minmax, int *d_channels)
{
    using namespace vap;
    VAP_TRY(vap_set_device(ctx));
    if (B < 0 || capacity < 0) return vap_fail(VAP_ERR_INVALID, "bad shape B=%d capacity=%ld", B, capacity);
    if (capacity > INT_MAX - 2048) return vap_fail(VAP_ERR_UNSUPPORTED, "capacity %ld above %d rows", capacity, INT_MAX - 2048);
    if (counts_stride < 1) return vap_fail(VAP_ERR_INVALID, "counts_stride must be >= 1 (got %d)", counts_stride);
    if (B > 0 && (!d_counts || (capacity > 0 && !d_rows))) return vap_fail(VAP_ERR_INVALID, "null rows / counts");
    // the sensors
    if (n_sens < 1 || n_sens > kRangeMaxSens) return vap_fail(VAP_ERR_INVALID, "%d sensors (1..%d)", n_sens, kRangeMaxSens);
    VAP_TRY(check_sensor_rows(n_sens, h_sensors));
    // the scene
    double scale = 0.0;
    int nv = 0;
    VAP_TRY(check_scene(h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, scale, nv));
    // the partners
    if (Bo < 0 || cap_o < 0) return vap_fail(VAP_ERR_INVALID, "bad partner shape Bo=%d capacity=%ld", Bo, cap_o);
    if (Bo > kRangeMaxPartners) return vap_fail(VAP_ERR_UNSUPPORTED, "%d partners (at most %d)", Bo, kRangeMaxPartners);
    if (!d_rows_o || cap_o == 0) Bo = 0;
    if (Bo > 0) {
        if (cap_o > INT_MAX) return vap_fail(VAP_ERR_UNSUPPORTED, "partner capacity %ld above %d rows", cap_o, INT_MAX);
        if (stride_o < 1) return vap_fail(VAP_ERR_INVALID, "the partners' counts stride must be >= 1 (got %d)", stride_o);
        if (!d_counts_o || !h_foot_o) return vap_fail(VAP_ERR_INVALID, "null partner counts / footprint");
        VAP_TRY(check_convex(h_foot_o, n_foot_o, "partner footprint", 0));
    } else {
        n_foot_o = 0;
    }
    if (B == 0) return VAP_OK;

    RangeArgs g{};
    g.rows = d_rows;
    g.counts = d_counts;
    g.stride = counts_stride;
    g.cap = (int)capacity;
    g.n_sens = n_sens;
    std::memcpy(g.sens, h_sensors, (size_t)n_sens * 8 * sizeof(double));
    SceneLayout blk;                                   // the partners' footprint rows in front (vap_footprint.h)
    VAP_TRY(scene_block(ctx, n_foot_o, h_foot_o, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles, nv, blk));
    g.o_poly = blk.o_poly, g.o_pv = blk.o_pv, g.o_circ = blk.o_circ, g.n_dbl = blk.n_dbl;
    double far = 0.0;
    for (int i = 0; i < n_foot_o; i++) far = std::fmax(far, std::hypot(h_foot_o[2 * i], h_foot_o[2 * i + 1]));
    g.scene = (const double *)ctx->scene.ptr;
    g.n_poly = n_poly;
    g.n_circle = n_circle;
    g.n_foot_o = n_foot_o;
    g.has_field = h_field ? 1 : 0;
    if (h_field) g.xmin = h_field[0], g.ymin = h_field[1], g.xmax = h_field[2], g.ymax = h_field[3];
    g.foot_R = far;
    g.slack = kCullSlack * (1.0 + scale + far);
    g.cull = ctx->footprint_cull;
    g.rows_o = d_rows_o;
    g.counts_o = d_counts_o;
    g.stride_o = stride_o;
    g.cap_o = (int)cap_o;
    g.Bo = Bo;
    g.shift = shift_rows;
    g.range = d_range;
    g.cosi = d_cos_incidence;
    g.code = d_code;
    g.status_counts = d_status_counts;
    g.minmax = d_range_minmax;
    g.channels = d_channels;
    // tiles as vap_drive_audit's: four steps a tile once there are workgroups enough to fill the device, else one, so that one
    // long routine still spreads over the CUs
    const long tiles4 = (capacity + 4 * kRangeThreads - 1) / (4 * kRangeThreads);
    g.iters = (long)B * tiles4 >= 1024 ? 4 : 1;
    const long tile_rows = (long)g.iters * kRangeThreads;
    g.tiles = (int)((capacity + tile_rows - 1) / tile_rows);
    const size_t np = (size_t)B * (size_t)(g.tiles > 0 ? g.tiles : 1);
    const size_t dbl_bytes = np * kRangePartDbls * sizeof(double);
    VAP_TRY(ctx->ensure(ctx->range_part, dbl_bytes + np * kRangePartInts * sizeof(int)));
    g.part_d = (double *)ctx->range_part.ptr;
    g.part_i = (int *)((char *)ctx->range_part.ptr + dbl_bytes);

    const bool lds = g.n_dbl <= kRangeLdsDoubles;
    const bool rows_out = d_range || d_cos_incidence || d_code;
    const size_t dyn = (lds ? (size_t)((g.n_dbl + 1) & ~1) * sizeof(double) : 0) +
                       (rows_out ? (size_t)kRangeThreads * n_sens * (2 * sizeof(double) + sizeof(int)) : 0);
    if (g.tiles > 0) {
        for (int b0 = 0; b0 < B; b0 += kRangeGridYMax) {
            const int nb = B - b0 < kRangeGridYMax ? B - b0 : kRangeGridYMax;
            g.b0 = b0;
            if (lds) hipLaunchKernelGGL(k_range_rows<true>, dim3((unsigned)g.tiles, (unsigned)nb), dim3(kRangeThreads), dyn, ctx->stream, g);
            else hipLaunchKernelGGL(k_range_rows<false>, dim3((unsigned)g.tiles, (unsigned)nb), dim3(kRangeThreads), dyn, ctx->stream, g);
        }
    }
    if (d_status_counts || d_range_minmax || d_channels)
        hipLaunchKernelGGL(k_range_finish, dim3((unsigned)B), dim3(64), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    return VAP_OK;
}

}  // extern "C"
