// vap_sample.hip — K3+K4, the sampler (gfx950 / CDNA4).
// ------------------------------------------------------------------------------------------------
// K3+K4: sampling.  grid = (tiles, B); a workgroup evaluates kSampleChunk consecutive samples of one
// path, each thread kSPT consecutive ones (so every output leaves as one 16-byte store per lane and
// the arc-length table is walked, not searched, after the thread's first sample).  The last thread's
// samples belong to the next tile: they only supply the neighbour for |dtheta| (rows that fit one pass,
// S <= kSampleChunk, need no such neighbour and are written by all threads).
// LDS: distance table + interval slopes (16 KB), the path's coefficient blocks when they fit
// (G <= kLdsCoefSegments; otherwise they are read through L1/L2, where a wavefront's consecutive
// samples hit one or two blocks), and a neighbour exchange of one record per thread.
// Arithmetic: parameter/index path, derivative evaluation and curvature in fp64 (DESIGN.md
// §Numerics); no fp64 division on the per-sample path.
// ------------------------------------------------------------------------------------------------
//
// Stage map: K1 fit -> K2 arc-length LUT -> K3+K4 sample -> K5 velocity pass.
// Data layout in HBM (B paths, W waypoints, G = W-1 segments, S sample capacity):
//   segments [B][G][6][2] fp64   reference row order (QHS:120-122)
//   power    [B][G][30]   fp64   monomial coefficients of P, P', P'' (x then y each; scratch)
//   lut      [B][1000]    fp64   cumulative trapezoid distances (SM:448-454)
//   meta     [B][4]       fp64   {param_last, total_length, dd, n_samples}
//   x,y,heading,curvature,dtheta,velocity [B][S]  fp32 or fp64, sample-major per path so that a
//   wavefront of consecutive samples reads/writes 256 (fp32) or 512 (fp64) contiguous bytes.
#include "vap_device.h"
#include "vap_kernels.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace vap {

static_assert(kCoefBlockDoubles == kCoefDoubles, "scratch sizing and block layout disagree");
static_assert(kGridRunBlockDoubles == kGridRunDoubles, "scratch sizing and run-table layout disagree");

// HI (fp32 outputs only): also write the curvature and |dtheta| rows in fp64 (ok64, odth64) for the fp64
// velocity recurrence behind fp32 outputs; the fp32 |dtheta| row is then optional (odth may be NULL).
//
// HALVES: a thread's kSPT samples go through the phases of the tile body kSPT / HALVES at a time.  HALVES = 2 keeps
// the fp64 derivative values, table entries and exchange values of two samples alive instead of four.  The instantiations
// it serves (fp32 rows with the fp64 side rows) fit 128 registers without a spill — 117; the four-wide form 120, once the
// fp32 position values are formed where the tile body says and not after the barrier — and are bound
// to four waves per SIMD (k_sample_waves; two paths per workgroup are held to three by their 44 KB of LDS whatever their
// registers).
// align_bits (launch_sample): bit 0 = the caller's rows take 16-byte stores (row length and row bases), bit 1 = the fp64
// side rows do.
constexpr int k_sample_waves(int halves, int ppb) { return halves == 2 && ppb == 1 ? 4 : 3; }
#ifdef VAP_SAMPLE_STATS   // developer build: in-kernel cycle shares per wave (costs scalar registers the kernel spills)
#define VAP_STATS_PARAM , long long *__restrict__ stats
#else
#define VAP_STATS_PARAM
#endif
template <typename OT, bool COEF_LDS, bool HI, int PPB = 1, int HALVES = 1>
__global__ __launch_bounds__(kSampleThreads, k_sample_waves(HALVES, PPB)) void k_sample(int B, int W, int S, int tile, int tiles_per_block, int align_bits,
                                                           const double *__restrict__ power,
                                                           const double *__restrict__ seg_rows,
                                                           const double *__restrict__ lut,
                                                           const double *__restrict__ slopes,
                                                           const double *__restrict__ meta,
                                                           const double *__restrict__ aux,
                                                           const double *__restrict__ runs,
                                                           OT *__restrict__ ox, OT *__restrict__ oy,
                                                           OT *__restrict__ oh, OT *__restrict__ ok,
                                                           OT *__restrict__ odth, double *__restrict__ ok64,
                                                           double *__restrict__ odth64 VAP_STATS_PARAM)
{
    static_assert(HALVES == 1 || HALVES == 2, "a thread's samples go through the phases all at once or in two halves");
    static_assert(!HI || sizeof(OT) == 4, "the fp64 side rows belong to the fp32 output mode");
    // PPB paths per workgroup (blockIdx.y * PPB + pp).  Rows that are one tile long (config 5: 1024 samples) leave a
    // workgroup as much time in staging — a chain of dependent memory round trips: meta, aux, tables, run table — as in
    // the tile itself; with PPB = 2 the loads of both paths are in flight together and the chain is paid once for two.
    extern __shared__ __attribute__((aligned(16))) double s_coef[];   // PPB * G * kCoefDoubles when COEF_LDS
    __shared__ double sD_all[PPB * kLutN], sWt_all[PPB * kLutN];
    // neighbour exchange, double-buffered by tile parity (one barrier per tile)
    // (one record per thread: one LDS address serves the four values; the entry past the last thread is read by the last
    // thread of a one-tile row, whose last sample has no neighbour, and never used)
    struct Neighbour { double dx, dy; OT th; int j; };
    __shared__ Neighbour s_nb[2][kSampleThreads + 1];
#ifdef VAP_SAMPLE_STATS
    const long long ts0 = stats ? __builtin_amdgcn_s_memtime() : 0;
#endif
    const int tid = threadIdx.x;
    const int G = W - 1;
    const int tile0 = blockIdx.x * tiles_per_block;
    if (tile0 * tile >= S) return;
    // tile == kSampleChunk: the whole row is one tile, so the last thread's last sample is the row's last
    // and needs no neighbour — every thread writes
    const bool writer = tile == kSampleChunk || tid < kSampleThreads - 1;
    // rows (and tile starts, multiples of kSPT) start 16-byte aligned: S % VW == 0 and the row bases, tested once per launch
    const bool aligned = (align_bits & 1) != 0;
    const bool aligned_hi = (align_bits & 2) != 0;   // the fp64 side rows: S even and their bases

    // per path: the scalars of its grid and tables
    int p_b[PPB], p_N[PPB], p_nruns[PPB];
    bool p_live[PPB];
    double p_tmax[PPB], p_total[PPB], p_dd[PPB], p_lstep[PPB], p_tstep[PPB], p_inv[PPB], p_sk[PPB];
    double run_touch = 0.0;
#pragma unroll
    for (int pp = 0; pp < PPB; pp++) {
        const int bq = blockIdx.y * PPB + pp;
        p_live[pp] = bq < B;
        const int b = p_live[pp] ? bq : B - 1;
        p_b[pp] = b;
        const double *m = meta + (size_t)b * kMetaStride;
        p_tmax[pp] = m[0]; p_total[pp] = m[1]; p_dd[pp] = m[2];
        p_N[pp] = (int)m[3];
        const double *ax = aux + (size_t)b * kAuxStride;
        p_lstep[pp] = ax[0]; p_tstep[pp] = ax[1]; p_inv[pp] = ax[2];
        p_nruns[pp] = (int)ax[3];
        // (touch the head of the run table now: its lookup below depends on meta / aux and would otherwise wait
        // for memory a second time)
        run_touch += runs[(size_t)b * kGridRunDoubles + (tid < 120 ? tid : 0)];
    }
    // (the last segment's end-tangent row d1 for the end tangent below: asked for now, with the meta loads — it depends on
    // the path's index alone — so that the one lane that uses it does not wait for memory once more)
    __shared__ double s_end[PPB][2];
    double end_d1x = 1.0, end_d1y = 1.0;
    {
        const int pp = tid < PPB ? tid : 0;
        if (seg_rows && tid < PPB && p_live[pp]) {
            end_d1x = seg_rows[((size_t)p_b[pp] * G + (G - 1)) * 12 + 6];
            end_d1y = seg_rows[((size_t)p_b[pp] * G + (G - 1)) * 12 + 7];
        }
    }
    // the paths' tables are staged once and serve every tile of this workgroup; all loads first
    {
        constexpr int ITER = 4;
        double vD[PPB][ITER], vW[PPB][ITER];
#pragma unroll
        for (int pp = 0; pp < PPB; pp++) {
            // (not a function of the path's sample count: the table loads then leave with the meta loads instead of a memory
            // round trip after them — the row is in bounds either way, p_b is clamped)
            const bool go = p_live[pp];
#pragma unroll
            for (int it = 0; it < ITER; it++) {
                const int i = tid + it * kSampleThreads;
                vD[pp][it] = (go && i < kLutN) ? lut[(size_t)p_b[pp] * kLutN + i] : 0.0;
                vW[pp][it] = (go && slopes && i < kLutN) ? slopes[(size_t)p_b[pp] * kLutN + i] : 0.0;
            }
        }
        static_assert(ITER * kSampleThreads >= kLutN, "one pass covers the table");
        // (here, between asking for the tables and using them: the lane's arithmetic runs while the workgroup waits for memory)
        // The table's last entry (read by the path's last sample only) sits at the end of the last segment, where the
        // reference's basis sum gives the end tangent exactly — a component that is an exact zero there (a path that ends
        // along an axis) keeps its sign into atan2 (SM:536) — while the power form leaves a residue of either sign: -pi for
        // +pi.  One lane per path evaluates the reference's form once; a component it puts at the zero level replaces the
        // power form's in that sample (NaN: keep the power form's, bit for bit what it always was — taking both components
        // from the reference's form on every path moves the last bits of an ordinary path's last heading and curvature, and with
        // them the rows pinned by tests/test_gpu_sample_rows.py).  seg_rows is NULL only where a caller has no segment rows.
#pragma unroll
        for (int pp = 0; pp < PPB; pp++) {
            if (tid == pp) {
                double rx = 1.0, ry = 1.0;
                // (P'(end) is the row d1 up to roundings and a parameter an ulp short of the end: only a path whose d1 has a
                // component near zero can have one at the zero level, and only it pays for the reference's basis sum)
                if (fabs(end_d1x) <= 1e-9 * fabs(end_d1y) || fabs(end_d1y) <= 1e-9 * fabs(end_d1x))
                    hermite_eval_ref(seg_rows + (size_t)p_b[pp] * G * 12, p_tmax[pp], G, 1, (double)(W - 1), rx, ry);
                s_end[pp][0] = fabs(rx) <= 1e-12 * fabs(ry) ? rx : __builtin_nan("");
                s_end[pp][1] = fabs(ry) <= 1e-12 * fabs(rx) ? ry : __builtin_nan("");
            }
        }
        if constexpr (COEF_LDS) {
#pragma unroll
            for (int pp = 0; pp < PPB; pp++)
                if (p_live[pp])     // (as the tables: not behind the meta loads)
                    lds_fill<4>(s_coef + (size_t)pp * G * kCoefDoubles, power + (size_t)p_b[pp] * G * kCoefDoubles, G * kCoefDoubles, tid,
                                kSampleThreads);
        }
#pragma unroll
        for (int pp = 0; pp < PPB; pp++) {
#pragma unroll
            for (int it = 0; it < ITER; it++) {
                const int i = tid + it * kSampleThreads;
                if (i < kLutN) {
                    sD_all[pp * kLutN + i] = vD[pp][it];
                    if (slopes) sWt_all[pp * kLutN + i] = vW[pp][it];
                }
            }
        }
    }
    // MPG:112-122 distance grid: the reference accumulates current_dist += dd.  A thread's first sample of a
    // tile comes from the path's run table (that sum in closed form, vap_device.h), the following ones by the
    // reference's own addition.
    auto grid_first_of = [&](const double *run_tab, double dd, int N, int n_runs, int kb0) {
        const int dd_exp = (__double2hiint(dd) >> 20) & 0x7ff;
        const int kf = kb0 < N - 1 ? kb0 : N - 1;
        // the run from the exponent of kf*dd: right except next to a binade boundary
        int r = 2 + 2 * (((__double2hiint((double)kf * dd) >> 20) & 0x7ff) - dd_exp);
        r = kf <= 0 ? 0 : r < 1 ? 1 : r;
        r = r > n_runs - 1 ? n_runs - 1 : r;
        const double *e = run_tab + 3 * r;
        int ka = (int)grid_run_k0(e, 0);
        const int kb = (int)grid_run_k0(e, 1);
        double sa = e[1], da = e[2];
        if (kf < ka || kf >= kb) {
            while ((int)grid_run_k0(run_tab, r + 1) <= kf) r++;                      // the end markers stop this
            while (r > 0 && (int)grid_run_k0(run_tab, r) > kf) r--;
            ka = (int)grid_run_k0(run_tab, r);
            sa = run_tab[3 * r + 1];
            da = run_tab[3 * r + 2];
        }
        return sa + (double)(kf - ka) * da;
    };
    // the first tile's lookup goes out together with the staging loads
#pragma unroll
    for (int pp = 0; pp < PPB; pp++)
        p_sk[pp] = (p_live[pp] && tile0 * tile < p_N[pp])
                       ? grid_first_of(runs + (size_t)p_b[pp] * kGridRunDoubles, p_dd[pp], p_N[pp], p_nruns[pp], tile0 * tile + tid * kSPT)
                       : 0.0;
    // Rows of one tile (PPB == 2 serves only those): a path's 1000 interval slopes would serve ~1000 samples once each, so a
    // sample forms the slope of ITS interval on the spot — the same expression, the same bits — and the slope array, its
    // 1000 divisions per path and a workgroup barrier go (config 5: staging is 45 % of a workgroup's life).
    constexpr bool kSlopeOnDemand = PPB == 2;
    if (!slopes && !kSlopeOnDemand) {
        // the interval slopes (t1 - t0)/(d1 - d0) of SM:311-317 from the staged distances — the expression k_lut uses, so
        // the same numbers, without 8 KB per path going to HBM and back (config 5: a fifth of the step's traffic)
        __syncthreads();
#pragma unroll
        for (int pp = 0; pp < PPB; pp++) {
            if (p_live[pp] && tile0 * tile < p_N[pp]) {
                const double *sDp = sD_all + pp * kLutN;
                for (int j = tid; j < kLutN; j += kSampleThreads) {
                    double w = 0.0;
                    if (j > 0) {
                        const double t0 = (double)(j - 1) * p_lstep[pp], t1 = (j == kLutN - 1) ? p_tmax[pp] : (double)j * p_lstep[pp];
                        w = div_inrange(t1 - t0, sDp[j] - sDp[j - 1]);
                    }
                    sWt_all[pp * kLutN + j] = w;
                }
            }
        }
    }
    __syncthreads();
    asm volatile("" ::"v"(run_touch));
#ifdef VAP_SAMPLE_STATS
    const long long ts1 = stats ? __builtin_amdgcn_s_memtime() : 0;
#endif
    const double end_param = (double)(W - 1);
    const int tab_n = W * kSamplesPerNode;
    int tiles_done = 0;   // parity of the neighbour exchange

#pragma unroll 1
    for (int pp = 0; pp < PPB; pp++) {
    // (the path's scalars again, from the scalar cache: carrying them through the tile loop as arrays indexed by pp
    // costs registers the tile body does not have)
    const int bq = blockIdx.y * PPB + pp;
    if (bq >= B) break;
    const int b = bq;
    const double *m = meta + (size_t)b * kMetaStride;
    const double t_max = m[0], total = m[1], dd = m[2];
    const int N = (int)m[3];
    const double *ax = aux + (size_t)b * kAuxStride;
    const double lstep = ax[0], tstep = ax[1], inv_tstep = ax[2];
    const int n_runs = (int)ax[3];
    const size_t row = (size_t)b * S;
    const double *sD = sD_all + pp * kLutN, *sWt = sWt_all + pp * kLutN;
    const double *pw = power + (size_t)b * G * kCoefDoubles;
    const double *coef = COEF_LDS ? s_coef + (size_t)pp * G * kCoefDoubles : pw;
    const double *run_tab = runs + (size_t)b * kGridRunDoubles;
    const double sk_first = PPB == 1 ? p_sk[0] : (pp == 0 ? p_sk[0] : p_sk[PPB - 1]);
    auto grid_first = [&](int kb0) { return grid_first_of(run_tab, dd, N, n_runs, kb0); };
    for (int tl = 0; tl < tiles_per_block; tl++) {
        const int k0 = (tile0 + tl) * tile;
        if (k0 >= S) break;
        const int kbase = k0 + tid * kSPT;
        auto store_vec = [&](OT *dst, const OT v[kSPT]) {
            if (!dst || !writer) return;
            if (aligned && kbase + kSPT <= S) {
                if constexpr (sizeof(OT) == 4) {
                    if constexpr (HI) {
                        // the caller's rows leave non-temporally: nothing on the device reads them again before the whole
                        // batch has been written, and the fp64 side rows the velocity kernel is about to read keep the
                        // cache (MALL) to themselves
                        using f4 = float __attribute__((ext_vector_type(4)));
                        f4 w = {v[0], v[1], v[2], v[3]};
                        __builtin_nontemporal_store(w, reinterpret_cast<f4 *>(dst + row + kbase));
                    } else {
                        *reinterpret_cast<float4 *>(dst + row + kbase) = make_float4(v[0], v[1], v[2], v[3]);
                    }
                } else {
                    *reinterpret_cast<double2 *>(dst + row + kbase) = make_double2(v[0], v[1]);
                    *reinterpret_cast<double2 *>(dst + row + kbase + 2) = make_double2(v[2], v[3]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < kSPT; i++)
                    if (kbase + i < S) dst[row + kbase + i] = v[i];
            }
        };
        auto store_hi = [&](double *dst, const double v[kSPT]) {   // rows of S doubles: 16-byte aligned when S is even
            if (!writer) return;
            if (aligned_hi && kbase + kSPT <= S) {
                *reinterpret_cast<double2 *>(dst + row + kbase) = make_double2(v[0], v[1]);
                *reinterpret_cast<double2 *>(dst + row + kbase + 2) = make_double2(v[2], v[3]);
            } else {
#pragma unroll
                for (int i = 0; i < kSPT; i++)
                    if (kbase + i < S) dst[row + kbase + i] = v[i];
            }
        };
        if (k0 >= N) {
            // past this path's grid (ragged dd mode): zero-fill so every output element is defined
            const OT z[kSPT] = {(OT)0, (OT)0, (OT)0, (OT)0};
            store_vec(ox, z); store_vec(oy, z); store_vec(oh, z); store_vec(ok, z); store_vec(odth, z);
            if constexpr (HI) {
                const double zd[kSPT] = {0.0, 0.0, 0.0, 0.0};
                store_hi(ok64, zd); store_hi(odth64, zd);
            }
            continue;
        }
        // interior tiles (every sample and its right-hand neighbour before the path's last sample, not the first tile, rows
        // 16-byte aligned): the same body without the end-of-path selects, chosen per tile — wave-uniform
        auto tile_body = [&](auto interior_tag) {
            constexpr bool INTERIOR = decltype(interior_tag)::value;
        constexpr int HS = kSPT / HALVES;   // samples that go through a phase side by side
        OT vx[kSPT], vy[kSPT], vh[kSPT], vk[kSPT], vd[kSPT];
        double vd64[HI ? kSPT : 1];
        [[maybe_unused]] double kap_even = 0.0;   // HI: the fp64 curvature row leaves in pairs as soon as a pair exists
        // MPG:112-122 distance grid: the reference accumulates current_dist += dd.  The thread's first
        // sample comes from the path's run table (that sum in closed form), the following ones by the
        // reference's own addition.  The wave's kSPT*64 consecutive samples almost always lie in one run,
        // or in three (a binade boundary: the old run, the boundary element, the new run).
        double sk = tl == 0 ? sk_first : grid_first(kbase);
        double d1x[kSPT], d1y[kSPT];
        int jjv[kSPT];
        int idx = 0;
        const int pb = tiles_done & 1;
        tiles_done++;
        // |heading[k+1] - heading[k]| of the reference's raw (un-unwrapped) atan2 values, for the thread's samples GA..GB:
        // each needs its right-hand neighbour's tangent, table entry and heading — the next sample of the thread, or, for
        // the thread's last sample, the next thread's first (the exchange: only after the tile's barrier)
        auto dtheta_range = [&](auto ga_tag, auto gb_tag) {
            constexpr int GA = decltype(ga_tag)::value, GB = decltype(gb_tag)::value, GN = GB - GA + 1;
            if constexpr (HI && sizeof(OT) == 4) {
                // the samples side by side, no branch per sample: the series for all of them, ONE rarely taken block
                // for samples outside its range, then the 2*pi multiples (the same operations as dtheta_f64)
                double dl[GN];
                bool act[GN], gen[GN];
                double nxv[GN], nyv[GN];
                OT nthv[GN];
                bool any_gen = false;
#pragma unroll
                for (int q = 0; q < GN; q++) {
                    const int i = GA + q;
                    const int k = kbase + i;
                    nxv[q] = (i + 1 < kSPT) ? d1x[(i + 1) % kSPT] : s_nb[pb][tid + 1].dx;
                    nyv[q] = (i + 1 < kSPT) ? d1y[(i + 1) % kSPT] : s_nb[pb][tid + 1].dy;
                    const int nj = (i + 1 < kSPT) ? jjv[(i + 1) % kSPT] : s_nb[pb][tid + 1].j;
                    nthv[q] = (i + 1 < kSPT) ? vh[(i + 1) % kSPT] : s_nb[pb][tid + 1].th;
                    act[q] = (INTERIOR || k < N - 1) && nj != jjv[i];
                    dl[q] = dtheta_f64_series(d1x[i], d1y[i], nxv[q], nyv[q], gen[q]);
                    gen[q] = gen[q] && act[q];
                    any_gen |= gen[q];
                }
                if (__builtin_expect(any_gen, 0)) {
#pragma unroll
                    for (int q = 0; q < GN; q++)
                        if (gen[q]) dl[q] = dtheta_f64_general(d1x[GA + q], d1y[GA + q], nxv[q], nyv[q]);
                }
#pragma unroll
                for (int q = 0; q < GN; q++) {
                    const int i = GA + q;
                    const double v = dtheta_f64_wrap(dl[q], vh[i], nthv[q]);
                    vd64[i] = act[q] ? v : vd64[i];   // (the fp32 row, where the staged API asks for it: rounded at the store)
                }
            } else {
#pragma unroll
                for (int i = GA; i <= GB; i++) {
                    const int k = kbase + i;
                    if (INTERIOR || k < N - 1) {
                        const double nx = (i + 1 < kSPT) ? d1x[(i + 1) % kSPT] : s_nb[pb][tid + 1].dx;
                        const double ny = (i + 1 < kSPT) ? d1y[(i + 1) % kSPT] : s_nb[pb][tid + 1].dy;
                        const int nj = (i + 1 < kSPT) ? jjv[(i + 1) % kSPT] : s_nb[pb][tid + 1].j;
                        const OT nth = (i + 1 < kSPT) ? vh[(i + 1) % kSPT] : s_nb[pb][tid + 1].th;
                        if constexpr (sizeof(OT) == 8) {
                            vd[i] = fabs(nth - vh[i]);
                        } else if constexpr (HI) {
                            if (nj != jjv[i]) vd64[i] = dtheta_f64(d1x[i], d1y[i], nx, ny, vh[i], nth);
                            vd[i] = (OT)vd64[i];   // (only stored when the staged API asked for the fp32 row as well)
                        } else {
                            if (nj != jjv[i]) vd[i] = dtheta_f32(d1x[i], d1y[i], nx, ny, vh[i], nth);
                        }
                    }
                }
            }
        };
#pragma unroll
        for (int h = 0; h < HALVES; h++) {
        const int g0 = h * HS;   // the half's first sample of the thread
        // Phase A, the samples' parameters and table entries side by side; the redo of a sample that sits a few ulps
        // from a decision point (rare) is ONE block after them instead of a divergent branch inside every sample
        double tA[HS], sA[HS];
        int idxA[HS];
        bool redo[HS], any_redo = false;
        // A1: distances and table entries.  The thread's first sample searches the table (fixed halvings, no loop); each
        // following one walks on from its predecessor's entry, which it passes at most once or twice where a table interval
        // is longer than dd (config 3: ~10 samples per interval) — two entries in one LDS read, two compare-and-selects.  A
        // sample that took both steps may have further to go: ONE rarely taken block after the side-by-side samples finishes
        // the walk (`while (idx < kLutN - 1 && sD[idx] < s) idx++`, the same entry in every case).
        bool walk_on[HS], any_walk = false;
#pragma unroll
        for (int i = 0; i < HS; i++) {
            const int g = g0 + i;
            const int k = INTERIOR ? kbase + g : (kbase + g < N - 1 ? kbase + g : N - 1);
            if (g > 0) sk = sk + dd;
            const double s = INTERIOR ? sk : ((k == N - 1) ? total : sk);
            walk_on[i] = false;
            if (g == 0) {
                idx = lut_search_left_fixed(sD, s);
                if constexpr (!INTERIOR) idx = idx < 1 ? 1 : idx;
            } else {   // (idx >= 1 already: the walk only moves on)
                const int i1 = idx + 1 < kLutN - 1 ? idx + 1 : kLutN - 1;
                const double a0 = sD[idx], a1 = sD[i1];
                const bool st1 = idx < kLutN - 1 && a0 < s;
                const bool st2 = st1 && idx + 1 < kLutN - 1 && a1 < s;
                idx += (int)st1 + (int)st2;
                walk_on[i] = st2;
                any_walk |= st2;
            }
            sA[i] = s;
            idxA[i] = idx;
        }
        if (__builtin_expect(any_walk, 0)) {
#pragma unroll
            for (int i = (g0 == 0 ? 1 : 0); i < HS; i++) {
                if (walk_on[i]) {
                    int ix = idxA[i];
                    while (ix < kLutN - 1 && sD[ix] < sA[i]) ix++;
                    idxA[i] = ix;
                }
            }
        }
        if constexpr (HALVES > 1) idx = idxA[HS - 1];   // the next half walks on from this half's last entry
        // A2: parameters and property-table entries
#pragma unroll
        for (int i = 0; i < HS; i++) {
            const double s = sA[i];
            const int idx = idxA[i];
            const double d0 = sD[idx - 1];
            const double t0 = (double)(idx - 1) * lstep;
            const bool exact = INTERIOR ? false : (s <= 0.0 || s >= total);
            double wslope;
            if (kSlopeOnDemand && !slopes) {
                const double t1 = (idx == kLutN - 1) ? t_max : (double)idx * lstep;
                wslope = div_inrange(t1 - t0, sD[idx] - d0);
            } else {
                wslope = sWt[idx];
            }
            double t = fma(wslope, s - d0, t0);
            if constexpr (!INTERIOR) t = s >= total ? end_param : t;
            bool near;
            jjv[g0 + i] = table_index_fast(t, tab_n, inv_tstep, near);
            tA[i] = t;
            redo[i] = near && !exact;
            any_redo |= redo[i];
        }
        if (__builtin_expect(any_redo, 0)) {
#pragma unroll
            for (int i = 0; i < HS; i++) {
                if (redo[i]) {   // the reference's own rounding (SM:311-317)
                    const int ix = idxA[i];
                    const double d0 = sD[ix - 1], t0 = (double)(ix - 1) * lstep;
                    const double t1 = (ix == kLutN - 1) ? t_max : (double)ix * lstep;
                    tA[i] = t0 + (t1 - t0) * (sA[i] - d0) / (sD[ix] - d0);
                    jjv[g0 + i] = table_index(tA[i], tab_n, end_param);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < HS; q++) {
            const int i = g0 + q;
            const double t = tA[q];
            const int jj = jjv[i];
            const double tp = (jj == tab_n - 1) ? end_param : (double)jj * tstep;
            double lt;
            int sg;
            normalize_inside(tp, G, lt, sg);
            const double *c = coef + sg * kCoefDoubles;
            double ex = horner4(c + kCoefD1, lt), ey = horner4(c + kCoefD1 + 5, lt);           // P'
            if constexpr (!INTERIOR) {
                if (__builtin_expect(jj == tab_n - 1, 0)) {   // the path's last sample (s_end: staged above; NaN = keep)
                    const double rx = s_end[pp][0], ry = s_end[pp][1];
                    ex = rx == rx ? rx : ex;
                    ey = ry == ry ? ry : ey;
                }
            }
            const double fx = horner3(c + kCoefD2, lt), fy = horner3(c + kCoefD2 + 4, lt);     // P''
            const double ss = fma(ex, ex, ey * ey);                               // SM:517
            const double num = fma(ex, fy, -(ey * fx));                           // SM:523
            // SM:526-527.  HI: straight-line, the curvature of every sample, then the select (kept from being sunk back into
            // a branch around P'' and the curvature, whose exec-mask bookkeeping costs more than it skips).  The other modes
            // keep the branch: speculated, the curvature costs them registers they do not have (fp64: 130 spills).
            double kap;
            if constexpr (HI) {
                double kc = curvature_of(num, ss);
                asm volatile("" : "+v"(kc));
                kap = (ss >= 1e-10) ? kc : 0.0;
            } else {
                kap = (ss >= 1e-10) ? curvature_of(num, ss) : 0.0;
            }
            vk[i] = (OT)kap;
            if constexpr (HI) {
                vd64[i] = 0.0;
                if ((i & 1) == 0) {
                    kap_even = kap;
                } else if (writer) {
                    const int ke = kbase + i - 1;
                    const double v0 = (INTERIOR || ke < N) ? kap_even : 0.0, v1 = (INTERIOR || ke + 1 < N) ? kap : 0.0;
                    if (INTERIOR || (aligned_hi && ke + 2 <= S)) {
                        *reinterpret_cast<double2 *>(ok64 + row + ke) = make_double2(v0, v1);
                    } else {
                        if (ke < S) ok64[row + ke] = v0;
                        if (ke + 1 < S) ok64[row + ke + 1] = v1;
                    }
                }
            }
            vh[i] = heading_of<OT>(ey, ex);                                       // SM:536
            d1x[i] = ex;
            d1y[i] = ey;
            // SM:204-215 get_point_at_parameter(t) at the sample's own parameter
            normalize_inside(t, G, lt, sg);
            c = coef + sg * kCoefDoubles;
            if constexpr (sizeof(OT) == 4) {
                const float *cf = reinterpret_cast<const float *>(c + kCoefPf);
                const float ltf = (float)lt;
                vx[i] = horner5f(cf, ltf);
                vy[i] = horner5f(cf + 6, ltf);
                // (formed here, not after the barrier where they are stored: until then the twelve coefficients and the
                // parameter would wait in registers in place of the two values)
                asm volatile("" : "+v"(vx[i]), "+v"(vy[i]));
            } else {
                vx[i] = horner5(c + kCoefP, lt);
                vy[i] = horner5(c + kCoefP + 6, lt);
            }
            vd[i] = (OT)0;
        }
        if (h == 0) {   // the thread's first sample is its left-hand neighbour's right-hand neighbour
            Neighbour *nb = &s_nb[pb][tid];
            nb->dx = d1x[0];
            nb->dy = d1y[0];
            nb->j = jjv[0];
            nb->th = vh[0];
        }
        if constexpr (HALVES == 2) {
            // the first half's samples but its last: their neighbours are at hand, and their tangents need not wait
            if (h == 0) dtheta_range(std::integral_constant<int, 0>{}, std::integral_constant<int, HS - 2>{});
        }
        }   // halves
        __syncthreads();
        if (writer) {
            // the rest: from the first half's last sample (its neighbour is the second half's first) to the thread's last
            dtheta_range(std::integral_constant<int, (HALVES == 2 ? HS - 1 : 0)>{}, std::integral_constant<int, kSPT - 1>{});
            if (!INTERIOR && k0 + kSampleChunk > N) {   // only the path's last tile has samples to blank
#pragma unroll
                for (int i = 0; i < kSPT; i++)
                    if (kbase + i >= N) {
                        vx[i] = vy[i] = vh[i] = vk[i] = vd[i] = (OT)0;
                        if constexpr (HI) vd64[i] = 0.0;
                    }
            }
            store_vec(ox, vx); store_vec(oy, vy); store_vec(oh, vh); store_vec(ok, vk);
            if constexpr (HI) store_hi(odth64, vd64);
            if constexpr (HI && sizeof(OT) == 4) {
                // vd64 is zero wherever the fp32 row is (samples without a right-hand neighbour, blanked samples): the
                // fp32 row is its rounding, formed only when there is a row to store
                if (odth) {
#pragma unroll
                    for (int i = 0; i < kSPT; i++) vd[i] = (OT)vd64[i];
                    store_vec(odth, vd);
                }
            } else {
                store_vec(odth, vd);
            }
        }
            };
        // (a path without a usable length — flagged VAP_FLAG_DEGENERATE, its table NaN from some entry on — still has N = S on
        // the fixed grid: it never takes the interior body, whose table search may answer entry 0 for it and then reads sD[-1])
        const bool interior = k0 > 0 && k0 + kSampleThreads * kSPT < N - 1 && aligned && aligned_hi && k0 + kSampleThreads * kSPT <= S &&
                              total > 0.0 && total < __builtin_inf();
        if (interior) tile_body(std::true_type{});
        else tile_body(std::false_type{});
    }
    }   // paths of this workgroup
#ifdef VAP_SAMPLE_STATS
    if (stats && (tid & 63) == 0) {
        long long *st = stats + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + (tid >> 6)) * 4;
        st[0] = ts1 - ts0;                                 // staging + barrier
        st[1] = __builtin_amdgcn_s_memtime() - ts1;        // all tiles
        st[2] = 0;
        st[3] = 0;
    }
#endif
}

hipError_t launch_sample(hipStream_t st, bool f64, int B, int W, int S, const double *pw, const double *lut,
                         const double *slopes, const double *meta, const double *aux, const double *runs, void *x,
                         void *y, void *h, void *k, void *dth, double *k64, double *dth64, const double *seg)
{
    const bool hi = !f64 && k64 && dth64;
    // one workgroup stages a path's tables once and walks tiles_per_block consecutive tiles; paths are
    // split over several workgroups only when the batch alone cannot fill the chip
    // a tile is kSampleTile samples (the last thread only feeds its neighbour's |dtheta|) unless the whole
    // row fits one workgroup pass (S <= kSampleChunk, e.g. 1024-sample rows), where no neighbour is needed
    const int tile = S <= kSampleChunk ? kSampleChunk : kSampleTile;
    const int n_tiles = (S + tile - 1) / tile;
    int split = (2048 + B - 1) / B;
    split = split < 1 ? 1 : (split > n_tiles ? n_tiles : split);
    const int tiles_per_block = (n_tiles + split - 1) / split;
    const bool in_lds = (W - 1) <= kLdsCoefSegments;
    // rows of one tile in large batches: two paths per workgroup (their staging loads in flight together)
    const int ppb = (n_tiles == 1 && B >= 8192 && in_lds && (W - 1) <= 16) ? 2 : 1;
    const dim3 grid((n_tiles + tiles_per_block - 1) / tiles_per_block, (B + ppb - 1) / ppb);
    const size_t lds = in_lds ? sizeof(double) * (size_t)ppb * (W - 1) * kCoefDoubles : 0;
    // 16-byte stores: the row length and the row bases, tested here once per launch (bit 0: the caller's rows, bit 1:
    // the fp64 side rows)
    const size_t vw = f64 ? 2 : 4;
    const uintptr_t bases = (uintptr_t)x | (uintptr_t)y | (uintptr_t)h | (uintptr_t)k | (uintptr_t)dth;
    const uintptr_t bases_hi = (uintptr_t)k64 | (uintptr_t)dth64;
    const int align_bits = (((size_t)S % vw) == 0 && (bases & 15) == 0 ? 1 : 0) | ((S & 1) == 0 && (bases_hi & 15) == 0 ? 2 : 0);
#ifdef VAP_SAMPLE_STATS
    // developer build (-DVAP_SAMPLE_STATS): VAP_SAMPLE_STATS=1 prints in-kernel cycle shares per wave (synchronises!)
    static const bool want_stats = getenv("VAP_SAMPLE_STATS") != nullptr;
    long long *stats = nullptr;
    const size_t n_waves = (size_t)grid.x * grid.y * 4;
    if (want_stats) (void)hipMalloc(&stats, n_waves * 4 * sizeof(long long));
#define VAP_STATS_ARG , stats
#else
#define VAP_STATS_ARG
#endif
#define VAP_SAMPLE(OT_, LDS_, HI_, PPB_, HALVES_)                                                                   \
    hipLaunchKernelGGL((k_sample<OT_, LDS_, HI_, PPB_, HALVES_>), grid, dim3(kSampleThreads), lds, st, B, W, S, tile, tiles_per_block, \
                       align_bits, pw, seg, lut, slopes, meta, aux, runs, (OT_ *)x, (OT_ *)y, (OT_ *)h, (OT_ *)k, (OT_ *)dth, k64,   \
                       dth64 VAP_STATS_ARG)
    // HALVES = 2 (four waves per SIMD) where the instantiation fits 128 registers without a spill
    if (ppb == 2) {
        if (f64) VAP_SAMPLE(double, true, false, 2, 1);
        else if (hi) VAP_SAMPLE(float, true, true, 2, 2);
        else VAP_SAMPLE(float, true, false, 2, 1);
    } else if (f64) { if (in_lds) VAP_SAMPLE(double, true, false, 1, 1); else VAP_SAMPLE(double, false, false, 1, 1); }
    else if (hi) { if (in_lds) VAP_SAMPLE(float, true, true, 1, 2); else VAP_SAMPLE(float, false, true, 1, 2); }
    else { if (in_lds) VAP_SAMPLE(float, true, false, 1, 1); else VAP_SAMPLE(float, false, false, 1, 1); }
#undef VAP_SAMPLE
#undef VAP_STATS_ARG
#ifdef VAP_SAMPLE_STATS
    if (stats) {
        std::vector<long long> h(n_waves * 4);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h.data(), stats, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
        (void)hipFree(stats);
        double sum[4] = {0, 0, 0, 0};
        for (size_t w = 0; w < n_waves; w++)
            for (int k = 0; k < 4; k++) sum[k] += (double)h[w * 4 + k];
        fprintf(stderr, "[sample grid %ux%u, %d tiles/block] per-wave mean ticks: stage %.0f tiles %.0f\n", grid.x,
                grid.y, tiles_per_block, sum[0] / n_waves, sum[1] / n_waves);
    }
#endif
    return hipGetLastError();
}

}  // namespace vap
