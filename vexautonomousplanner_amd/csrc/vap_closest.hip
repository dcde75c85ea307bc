// vap_closest.hip — closest-point projection of query points onto fitted paths.
//
//   VAP_CLOSEST_GUI    PathWidget.find_closest_point_on_path (gui/path.py:658-727) reproduced exactly: a coarse pass of
//                      25*len(nodes)+1 percent steps, then 501 steps over +-2 % of the coarse winner, each step
//                      percent_to_parameter (SM:277-289, quirk Q6) + get_point_at_parameter (SM:204-215) + math.hypot,
//                      min_dist carried from the coarse pass into the fine one, strict '<' (the first index wins).
//   VAP_CLOSEST_EXACT  the global minimiser of |P(t) - q| over t in [0, W-1]: per segment the real roots of
//                      g(u) = (P(u) - q) . P'(u) (degree 9), isolated by sign variations of its Bernstein coefficients
//                      on dyadic subintervals and polished by safeguarded Newton, against the segment endpoints.
//
// One workgroup of four waves per (path, block of queries); a wave takes one query at a time and spreads its
// candidates (GUI) or the path's segments (EXACT) over its 64 lanes, then takes a wave argmin.  The path's spline
// table {parameters[-1], distance offset, parameter offset, first node} sits in LDS, its segment rows too when they
// fit.  Every point is evaluated the way k_route_eval / the batched samplers evaluate it (hermite_eval_ref after the
// SM:243-275 spline mapping), so a returned point equals vap_route_eval(order 0) at the returned parameter bit for bit.
#include <cmath>
#include <cstdint>

#include "vap_device.h"
#include "vap_ctx_state.h"

namespace vap {

constexpr int kClosestThreads = 256;
constexpr int kClosestWaves = kClosestThreads / 64;
constexpr int kClosestQueriesPerBlock = 4 * kClosestWaves;    // each wave takes 4 queries of its workgroup
constexpr int kClosestMaxQueryBlocks = 65535;                  // grid.y
constexpr int kClosestSegLdsBytes = 32 * 1024;                 // segment rows staged in LDS up to this size
constexpr int kExactMaxDepth = 30;                             // dyadic subdivision down to 2^-30 in local u
constexpr int kExactMaxIntervals = 512;                        // per segment and query (a safety bound, never met)

// One path as the kernel reads it.
struct ClosestPath {
    const double *seg;   // [W-1][12] segment rows (LDS or global)
    const double *sp;    // [n_spl][kSplineStride] in LDS
    const double *D;     // [n_spl][lut_n] partial distances of each spline's table (SM:448-454)
    int n_spl, lut_n, W;
    double total;
};

// SM:243-275 _map_parameter_to_spline (a split node belongs to the earlier spline) + QHS:221-251: route_eval's
// operations on the spline-table layout of the batched kernels.
__device__ __forceinline__ int closest_spline_of(const ClosestPath &p, double t)
{
    int si = p.n_spl - 1;
#pragma unroll 1
    for (int i = 0; i < p.n_spl - 1; i++)
        if (t <= p.sp[(i + 1) * kSplineStride + 3]) { si = i; break; }
    return si;
}
__device__ __forceinline__ void closest_eval(const ClosestPath &p, double t, int order, double &x, double &y)
{
    const int si = closest_spline_of(p, t);
    const int first = (int)p.sp[si * kSplineStride + 3];
    const int last = si + 1 < p.n_spl ? (int)p.sp[(si + 1) * kSplineStride + 3] : p.W - 1;
    hermite_eval_ref(p.seg + (size_t)first * 12, p.sp[si * kSplineStride + 0], last - first, order, t - (double)first, x, y);
}

// Arc length s at parameter t from the path's own table: the lerp of distance_to_time (SM:291-318) inverted between
// the two table parameters around t, so that distance_to_time(s) gives t back.
__device__ double closest_arc_length(const ClosestPath &p, double t)
{
    const int si = closest_spline_of(p, t);
    const int n = p.lut_n;
    const double tmax = p.sp[si * kSplineStride + 0], doff = p.sp[si * kSplineStride + 1], poff = p.sp[si * kSplineStride + 2];
    const double *D = p.D + (size_t)si * n;
    auto par = [&](int j) { return linspace_at(tmax, n, j) + poff; };
    if (!(t > par(0))) return D[0] + doff;
    if (t >= par(n - 1)) return D[n - 1] + doff;
    const double step = tmax / (double)(n - 1);
    int j = (int)ceil((t - poff) / step);
    j = j < 1 ? 1 : (j > n - 1 ? n - 1 : j);
#pragma unroll 1
    while (j > 1 && par(j - 1) >= t) j--;
#pragma unroll 1
    while (j < n - 1 && par(j) < t) j++;
    const double t0 = par(j - 1), t1 = par(j), d0 = D[j - 1] + doff, d1 = D[j] + doff;
    if (!(t1 > t0) || !(d1 > d0)) return d0;
    return d0 + (d1 - d0) * (t - t0) / (t1 - t0);
}

// percent_to_parameter (SM:277-289): min(max(len(nodes) * percent, 0), len(nodes) - 1), Python's min / max.
__device__ __forceinline__ double gui_parameter(int N, double percent)
{
    const double x = (double)N * percent;
    const double v = 0.0 > x ? 0.0 : x;
    const double hi = (double)(N - 1);
    return hi < v ? hi : v;
}

// (d, key) argmin over the wave: the smaller d, on equal d the smaller key.  Every lane ends with the result.
template <typename K>
__device__ __forceinline__ void wave_argmin(double &d, K &key)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(d, off);
        const K ok = __shfl_xor(key, off);
        if (od < d || (od == d && ok < key)) { d = od; key = ok; }
    }
}

// ---- EXACT mode: one segment -------------------------------------------------------------------------------------
// g(u) = (P(u) - q) . P'(u) in monomial form, g[0..9]
__device__ __forceinline__ void stationary_poly(const double *__restrict__ r, double qx, double qy, double g[10])
{
    double cx[6], cy[6];
    hermite_to_power(r[0], r[2], r[4], r[6], r[8], r[10], cx);
    hermite_to_power(r[1], r[3], r[5], r[7], r[9], r[11], cy);
    cx[0] -= qx;
    cy[0] -= qy;
#pragma unroll
    for (int k = 0; k < 10; k++) g[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 5; j++) g[i + j] += cx[i] * ((double)(j + 1) * cx[j + 1]) + cy[i] * ((double)(j + 1) * cy[j + 1]);
}
__device__ __forceinline__ double poly9(const double g[10], double u)
{
    double v = g[9];
#pragma unroll
    for (int k = 8; k >= 0; k--) v = fma(v, u, g[k]);
    return v;
}
__device__ __forceinline__ double poly9_d(const double g[10], double u)
{
    double v = 9.0 * g[9];
#pragma unroll
    for (int k = 8; k >= 1; k--) v = fma(v, u, (double)k * g[k]);
    return v;
}
// Sign variations of the Bernstein coefficients of g restricted to [a, a+h] (zeros skipped).  By Descartes' rule in the
// Bernstein basis the count bounds the roots in the interval and has their parity; 0 or 1 decides it.  `first` gets
// the sign of the first coefficient that is not zero: the sign of g just inside the interval's left end.
__device__ int bernstein_variations(const double g[10], double a, double h, int &first)
{
    double c[10];
#pragma unroll
    for (int k = 0; k < 10; k++) c[k] = g[k];
#pragma unroll
    for (int i = 0; i < 9; i++)             // Taylor shift: c(s) = g(a + s)
#pragma unroll
        for (int k = 8; k >= i; k--) c[k] = fma(a, c[k + 1], c[k]);
    double hp = 1.0;
#pragma unroll
    for (int k = 0; k < 10; k++) { c[k] *= hp; hp *= h; }   // c(h s)
    // b_i = sum_{k<=i} C(i,k) / C(9,k) c_k
    constexpr double binom9[10] = {1, 9, 36, 84, 126, 126, 84, 36, 9, 1};
    int var = 0;
    int last = 0;
    first = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        double b = 0.0, cik = 1.0;   // C(i, k)
#pragma unroll
        for (int k = 0; k <= i; k++) {
            b += cik / binom9[k] * c[k];
            cik = cik * (double)(i - k) / (double)(k + 1);
        }
        const int s = b > 0.0 ? 1 : (b < 0.0 ? -1 : 0);
        if (s != 0) {
            if (last != 0 && s != last) var++;
            if (last == 0) first = s;
            last = s;
        }
    }
    return var;
}
// The one root of g in [lo, hi]: Newton inside a bracket that bisection keeps shrinking.  Where g(lo) is exactly zero (a
// segment that starts at a cusp: P'(lo) = 0, and lo is a node the node pass has taken) the bracket's left sign is the
// one just inside: `first`, from the Bernstein coefficients of this same interval.  With the zero itself the bracket
// closed on lo and lost the root.  On a deeper interval the Taylor-shifted first coefficient and poly9(g, lo) round
// differently, so `first` may come from a tiny first coefficient that is not zero; it is still the sign just inside.
__device__ double bracketed_root(const double g[10], double lo, double hi, int first)
{
    double glo = poly9(g, lo);
    if (glo == 0.0) glo = (double)first;
    double x = 0.5 * (lo + hi);
#pragma unroll 1
    for (int it = 0; it < 80; it++) {
        const double gx = poly9(g, x);
        if (gx == 0.0) break;
        if ((gx < 0.0) == (glo < 0.0)) { lo = x; glo = gx; }
        else hi = x;
        const double dg = poly9_d(g, x);
        double xn = x - gx / dg;
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
        const double step = fabs(xn - x);
        x = xn;
        if (step <= 1e-16 || hi - lo <= 1e-16) break;
    }
    return x;
}

struct Best {
    double d, t;
};
__device__ __forceinline__ void consider(const ClosestPath &p, double qx, double qy, double t, Best &b)
{
    double x, y;
    closest_eval(p, t, 0, x, y);
    const double d = hypot(x - qx, y - qy);
    if (d < b.d || (d == b.d && t < b.t)) { b.d = d; b.t = t; }
}

// Distance from q to the bounding box of the segment's Bezier control points (the curve lies in their hull): a lower
// bound of the distance to the segment.
__device__ __forceinline__ double segment_lower_bound(const double *__restrict__ r, double qx, double qy)
{
    double lb2 = 0.0;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const double p0 = r[c], p1 = r[2 + c], d0 = r[4 + c], d1 = r[6 + c], e0 = r[8 + c], e1 = r[10 + c];
        const double b[6] = {p0, p0 + d0 / 5.0, p0 + 0.4 * d0 + e0 / 20.0, p1 - 0.4 * d1 + e1 / 20.0, p1 - d1 / 5.0, p1};
        double mn = b[0], mx = b[0];
#pragma unroll
        for (int i = 1; i < 6; i++) { mn = fmin(mn, b[i]); mx = fmax(mx, b[i]); }
        const double q = c == 0 ? qx : qy;
        const double o = q < mn ? mn - q : (q > mx ? q - mx : 0.0);
        lb2 += o * o;
    }
    return sqrt(lb2);
}

__device__ void exact_segment(const ClosestPath &p, int s, double qx, double qy, Best &b)
{
    const double *r = p.seg + (size_t)s * 12;
    double g[10];
    stationary_poly(r, qx, qy, g);
    const double base = (double)s;
    uint64_t idx = 0;
    int depth = 0;
#pragma unroll 1
    for (int n = 0; n < kExactMaxIntervals; n++) {
        const double h = ldexp(1.0, -depth);
        const double a = (double)idx * h;
        int first;
        const int var = bernstein_variations(g, a, h, first);
        if (var >= 2 && depth < kExactMaxDepth) {
            consider(p, qx, qy, base + (a + 0.5 * h), b);   // a root exactly at the split point is caught here
            idx <<= 1;
            depth++;
            continue;
        }
        if (var >= 1) consider(p, qx, qy, base + bracketed_root(g, a, a + h, first), b);
        while (depth > 0 && (idx & 1)) { idx >>= 1; depth--; }
        if (depth == 0) break;
        idx += 1;
    }
}

// ---- the kernel --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kClosestThreads) void k_closest(ClosestSrc src, int Q, int mode, int shared_queries,
                                                             const double *__restrict__ queries, double *__restrict__ o_t,
                                                             double *__restrict__ o_pt, double *__restrict__ o_d,
                                                             double *__restrict__ o_s, double *__restrict__ o_ct,
                                                             uint32_t *__restrict__ flags)
{
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    __shared__ int s_nspl;
    __shared__ double s_total;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int W = src.W, G = W - 1;
    const int NSmax = src.sptab ? src.NS : (src.r_tmax ? src.r_nspl : 1);
    double *s_sp = s_mem;
    double *s_seg = s_mem + (size_t)NSmax * kSplineStride;
    const double *gseg = src.seg + (size_t)b * G * 12;
    const bool seg_lds = src.seg_lds != 0;
    if (seg_lds)
        for (int i = tid; i < G * 12; i += kClosestThreads) s_seg[i] = gseg[i];
    if (src.sptab) {
        const int n = src.nspl[b];
        for (int i = tid; i < n * kSplineStride; i += kClosestThreads) s_sp[i] = src.sptab[(size_t)b * src.NS * kSplineStride + i];
        if (tid == 0) s_nspl = n;
    } else if (src.r_tmax) {
        for (int i = tid; i < src.r_nspl; i += kClosestThreads) {
            s_sp[i * kSplineStride + 0] = src.r_tmax[i];
            s_sp[i * kSplineStride + 1] = src.r_dist0[i];
            s_sp[i * kSplineStride + 2] = src.r_param0[i];
            s_sp[i * kSplineStride + 3] = (double)src.r_seg0[i];
        }
        if (tid == 0) s_nspl = src.r_nspl;
    } else if (tid == 0) {
        // a plain path: one spline, zero offsets; parameters[-1] exactly as the fit formed it (QHS:719-736, sequential
        // np.cumsum order of the chord lengths — segment rows 0 and 1 are the waypoints themselves)
        double cum = 0.0;
        for (int i = 0; i < G; i++) {
            const double *r = gseg + (size_t)i * 12;
            const double dx = r[2] - r[0], dy = r[3] - r[1];
            cum += sqrt(dx * dx + dy * dy);
        }
        s_sp[0] = (cum == 0.0) ? (double)G : cum * (double)G / cum;
        s_sp[1] = 0.0;
        s_sp[2] = 0.0;
        s_sp[3] = 0.0;
        s_nspl = 1;
    }
    __syncthreads();
    ClosestPath p;
    p.seg = seg_lds ? s_seg : gseg;
    p.sp = s_sp;
    p.n_spl = s_nspl;
    p.lut_n = src.lut_n;
    p.D = src.lut + (size_t)b * src.lut_stride;
    p.W = W;
    if (tid == 0) {
        const int l = p.n_spl - 1;
        s_total = p.D[(size_t)l * p.lut_n + p.lut_n - 1] + p.sp[l * kSplineStride + 1];   // SM:457-464's running sum
    }
    __syncthreads();
    p.total = s_total;
    const bool bad = flags && (flags[b] & 8u);              // VAP_FLAG_BAD_ROUTE from the profile call
    const bool empty = !(p.total > 0.0);                     // gui/path.py:670-679: no path / zero length
    if (empty && tid == 0 && flags && blockIdx.y == 0) atomicOr(&flags[b], VAP_FLAG_DEGENERATE_BIT);
    const int wave = tid >> 6, lane = tid & 63;
    const int q0 = blockIdx.y * kClosestQueriesPerBlock;
    const int q1 = q0 + kClosestQueriesPerBlock < Q ? q0 + kClosestQueriesPerBlock : Q;
#pragma unroll 1
    for (int q = q0 + wave; q < q1; q += kClosestWaves) {
        const size_t oi = (size_t)b * Q + q;
        const double *qp = queries + 2 * (shared_queries ? (size_t)q : oi);
        const double qx = qp[0], qy = qp[1];
        double t;
        if (bad || empty) {
            t = NAN;
        } else if (mode == VAP_CLOSEST_GUI) {
            const int nc = 25 * W;                 // num_steps = 25 * len(self.nodes)
            const double ncd = (double)nc;
            double bd = INFINITY;
            int bi = INT32_MAX;
#pragma unroll 1
            for (int i = lane; i <= nc; i += 64) {
                const double tc = gui_parameter(W, (double)i / ncd);
                double x, y;
                closest_eval(p, tc, 0, x, y);
                const double d = hypot(x - qx, y - qy);
                if (d < bd) { bd = d; bi = i; }
            }
            wave_argmin(bd, bi);
            const double cp = bi == INT32_MAX ? 0.0 : (double)bi / ncd;     // closest_percent
            const double lo = cp - 0.02, hi = cp + 0.02;
            const double start = lo > 0.0 ? lo : 0.0;                          // max(0.0, cp - 0.02)
            const double end = hi < 1.0 ? hi : 1.0;                            // min(1.0, cp + 0.02)
            const double step = (end - start) / 500;
            double fd = INFINITY;
            int fi = INT32_MAX;
#pragma unroll 1
            for (int i = lane; i <= 500; i += 64) {
                const double tf = gui_parameter(W, start + (double)i * step);
                double x, y;
                closest_eval(p, tf, 0, x, y);
                const double d = hypot(x - qx, y - qy);
                if (d < fd) { fd = d; fi = i; }
            }
            wave_argmin(fd, fi);
            if (fd < bd) t = gui_parameter(W, start + (double)fi * step);
            else t = bi == INT32_MAX ? 0.0 : gui_parameter(W, cp);
        } else {
            Best best{INFINITY, INFINITY};
#pragma unroll 1
            for (int k = lane; k < W; k += 64) consider(p, qx, qy, (double)k, best);   // the nodes: an upper bound
            wave_argmin(best.d, best.t);
            const double ub = best.d;
#pragma unroll 1
            for (int s = lane; s < G; s += 64) {
                const double lb = segment_lower_bound(p.seg + (size_t)s * 12, qx, qy);
                if (lb > ub * (1.0 + 1e-12) + 1e-12) continue;
                exact_segment(p, s, qx, qy, best);
            }
            wave_argmin(best.d, best.t);
            t = best.t;
        }
        if (lane == 0) {
            double x = NAN, y = NAN, d = NAN, s = NAN, ct = NAN;
            if (!(bad || empty)) {
                closest_eval(p, t, 0, x, y);
                d = hypot(x - qx, y - qy);
                double dx, dy;
                closest_eval(p, t, 1, dx, dy);
                const double cr = dx * (qy - y) - dy * (qx - x);
                ct = cr > 0.0 ? d : -d;
                if (o_s) s = closest_arc_length(p, t);
            }
            if (o_t) o_t[oi] = t;
            if (o_pt) { o_pt[2 * oi] = x; o_pt[2 * oi + 1] = y; }
            if (o_d) o_d[oi] = d;
            if (o_s) o_s[oi] = s;
            if (o_ct) o_ct[oi] = ct;
        }
    }
}

size_t closest_lds_bytes(const ClosestSrc &src, bool &seg_lds)
{
    const int NSmax = src.sptab ? src.NS : (src.r_tmax ? src.r_nspl : 1);
    const size_t sp = sizeof(double) * (size_t)NSmax * kSplineStride;
    const size_t sg = sizeof(double) * (size_t)(src.W - 1) * 12;
    seg_lds = sg <= (size_t)kClosestSegLdsBytes;
    return sp + (seg_lds ? sg : 0);
}

hipError_t launch_closest(hipStream_t st, ClosestSrc src, int B, int Q, int mode, int shared_queries, const double *queries,
                          double *t, double *pt, double *d, double *s, double *ct, uint32_t *flags)
{
    bool seg_lds = false;
    const size_t lds = closest_lds_bytes(src, seg_lds);
    src.seg_lds = seg_lds ? 1 : 0;
    // lds never exceeds the 64 KB any launch may have, so no larger limit is asked for: staged rows mean W <= 342 and at
    // most 341 splines (32 736 + 341 * 32 = 43 648 B); unstaged rows leave the spline table alone, at most
    // kMaxRouteWaypoints - 1 = 1499 rows of 32 B (47 968 B).  tests/test_closest_cpu.py pins the arithmetic.
    const dim3 grid(B, (Q + kClosestQueriesPerBlock - 1) / kClosestQueriesPerBlock);
    hipLaunchKernelGGL(k_closest, grid, dim3(kClosestThreads), lds, st, src, Q, mode, shared_queries, queries, t, pt, d, s, ct, flags);
    return hipGetLastError();
}

}  // namespace vap

extern "C" {

int vap_closest_points(vap_ctx *ctx, int B, int W, int Q, int mode, int shared_queries, const double *d_queries,
                       double *d_parameter, double *d_point, double *d_distance, double *d_arc_length, double *d_cross_track,
                       uint32_t *d_flags)
{
    VAP_TRY(vap_set_device(ctx));
    if (B < 1 || W < 2 || Q < 0) return vap_fail(VAP_ERR_INVALID, "bad shape B=%d W=%d Q=%d", B, W, Q);
    if (mode != VAP_CLOSEST_GUI && mode != VAP_CLOSEST_EXACT) return vap_fail(VAP_ERR_INVALID, "mode must be VAP_CLOSEST_GUI or VAP_CLOSEST_EXACT");
    VapTables t;
    VAP_TRY(vap_ctx_tables(ctx, B, W, false, t));
    if (Q == 0) return VAP_OK;
    if (!d_queries) return vap_fail(VAP_ERR_INVALID, "null query buffer");
    if ((Q + vap::kClosestQueriesPerBlock - 1) / vap::kClosestQueriesPerBlock > vap::kClosestMaxQueryBlocks)
        return vap_fail(VAP_ERR_UNSUPPORTED, "Q=%d queries per path exceed one launch (%d)", Q,
                        vap::kClosestMaxQueryBlocks * vap::kClosestQueriesPerBlock);
    vap::ClosestSrc src;
    src.W = W;
    src.seg = t.seg;
    src.lut = t.lut;
    src.lut_n = vap::kLutN;
    src.lut_stride = vap::kLutN;
    if (t.rt.sptab) {
        src.sptab = t.rt.sptab;
        src.nspl = t.rt.nspl;
        src.NS = t.rt.NS;
        src.lut_stride = (size_t)t.rt.NS * vap::kLutN;
    }
    HIP_TRY(vap::launch_closest(ctx->stream, src, B, Q, mode, shared_queries, d_queries, d_parameter, d_point, d_distance,
                                d_arc_length, d_cross_track, d_flags));
    return VAP_OK;
}

}  // extern "C"
