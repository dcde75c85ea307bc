// vap_band_sweep.h — the band sweep under vap_conflict_shifts (k_shift_sweep) and vap_schedule_tables (k_schedule_sweep).
//
// Both kernels give a workgroup of one wave one A route and a band of up to 64 window entries, a lane per entry, walk A's
// rows in blocks of 64 and let the lanes read one staged run of O rows, each from its own offset.  What the two walks do
// alike stands here once: sweep_load_feet (the footprints into LDS), band_needs_block (A's block circle against the O
// blocks the band meets), sweep_stage (the A block and the O band into LDS) and SweepQueue (the ring of survivors of the
// row bound, tested exactly 64 at a time whatever lanes they came from; a result lowers an integer key in LDS).  What
// differs is passed in: the O blocks and rows a band meets, the staged O slot of an entry, the key a result goes to and the
// key a lane reads its running minimum from.  Host: sweep_bands sizes the band and its LDS, sweep_fits refuses a band
// the device has no LDS for.
#pragma once
#include "vap_conflict.h"

namespace vap {

constexpr int kSweepLanes = 64;                  // one wave: a lane per window entry of the band
constexpr long kSweepStageRows = 1024;           // O rows staged at most (32 KB); the band halves until it fits
constexpr int kSweepQueue = 128;                 // ring of queued (row, lane) survivors

__device__ __forceinline__ void sweep_load_feet(double *sfa, double *sfo, const ConfFoot &fa, const ConfFoot &fo, int lane)
{
    sfa[lane] = fa.v[lane];
    sfa[lane + 64] = fa.v[lane + 64];
    sfo[lane] = fo.v[lane];
    sfo[lane + 64] = fo.v[lane + 64];
}

// Does any O block b0 .. b1 (circles at qo_all) come within `thr` of A's block circle qa?  Lanes stride the blocks.
__device__ __forceinline__ bool band_needs_block(const ConfPacked &g, double radii, double thr, const double *qa, const double *qo_all,
                                                 long b0, long b1, int lane)
{
    const double ax = qa[0], ay = qa[1], ar = qa[2];
    bool need = false;
#pragma unroll 1
    for (long b = b0 + lane; b <= b1; b += kSweepLanes) {
        const double *qo = qo_all + (size_t)b * 4;
        need = need || !block_culled(g, radii, thr, ax, ay, ar, qo[0], qo[1], qo[2]);
    }
    return __any(need);
}

// A's packed rows t0 .. t0 + 63 and O's rows o0 .. o0 + nq - 1, each index clamped into the side's own rows.  Every lane
// must have left the previous block's rows (SweepQueue::close ends with a barrier).
__device__ __forceinline__ void sweep_stage(double *stage_a, const double *pa, long t0, long n_a, double *stage_o, const double *po, long o0,
                                            long n_o, int nq, int lane)
{
    {
        const double *src = pa + (size_t)clampl(t0 + lane, 0, n_a - 1) * 4;
        *(double2 *)(stage_a + lane * 4) = *(const double2 *)src;
        *(double2 *)(stage_a + lane * 4 + 2) = *(const double2 *)(src + 2);
    }
#pragma unroll 1
    for (int i = lane; i < nq; i += kSweepLanes) {
        const double *src = po + (size_t)clampl(o0 + i, 0, n_o - 1) * 4;
        *(double2 *)(stage_o + (size_t)i * 4) = *(const double2 *)src;
        *(double2 *)(stage_o + (size_t)i * 4 + 2) = *(const double2 *)(src + 2);
    }
}

// The survivors of one pair's walk.  slot(tt, l): the staged O row of block row tt for lane l; key(tt, l): the key that
// entry's clearance lowers; mine(): the lane's running minimum, read back after the exact tests.
struct SweepQueue {
    const double *sfa, *sfo, *stage_a, *stage_o;
    unsigned short *ring;
    int na, no, lane;
    int qn = 0, head = 0;                        // the ring's fill and first entry (uniform)

    // the exact pair of `n` queued survivors, a lane each; afterwards every lane's running minimum is current
    template <class Slot, class Key, class Mine>
    __device__ __forceinline__ void flush(int n, double &best, Slot slot, Key key, Mine mine)
    {
        __syncthreads();
        if (lane < n) {
            const int e = ring[(head + lane) & (kSweepQueue - 1)];
            const int tt = e & 63, l = e >> 6;
            const double c = pair_at(sfa, na, sfo, no, stage_a + tt * 4, stage_o + (size_t)slot(tt, l) * 4);
            if (c == c) atomicMin(key(tt, l), conf_key(c));      // a NaN clearance takes part in nothing
        }
        __syncthreads();
        best = mine();
    }
    // block row tt of this lane has (cand) or has not passed the row bound; 64 waiting entries are tested at once
    template <class Slot, class Key, class Mine>
    __device__ __forceinline__ void push(bool cand, int tt, double &best, Slot slot, Key key, Mine mine)
    {
        const unsigned long long mask = __ballot(cand);
        if (!mask) return;
        if (cand) {
            const int pos = head + qn + __popcll(mask & ((1ull << lane) - 1ull));
            ring[pos & (kSweepQueue - 1)] = (unsigned short)(tt | (lane << 6));
        }
        qn += __popcll(mask);
        if (qn >= kSweepLanes) {
            flush(kSweepLanes, best, slot, key, mine);
            head = (head + kSweepLanes) & (kSweepQueue - 1);
            qn -= kSweepLanes;
        }
    }
    // the end of a block: the rows leave LDS with it; also the barrier in front of the next block's staging
    template <class Slot, class Key, class Mine>
    __device__ __forceinline__ void close(double &best, Slot slot, Key key, Mine mine)
    {
        flush(qn, best, slot, key, mine);
        head = 0;
        qn = 0;
    }
};

// ---- host ----------------------------------------------------------------------------------------------------------------
// The band of a window of n entries at `step` rows apart: the most entries, a power of two, whose O rows fit the stage.
struct SweepBands {
    int band, nbands, nb_max;     // entries per workgroup, workgroups per route, live lanes of the fullest band
    size_t lds;                   // dynamic LDS: the caller's keys, then the staged O band
};
static SweepBands sweep_bands(int n, int step, size_t key_bytes)
{
    SweepBands b;
    b.band = kSweepLanes;
    while (b.band > 1 && kConfBlock + (long)(b.band - 1) * step > kSweepStageRows) b.band /= 2;
    b.nbands = (n + b.band - 1) / b.band;
    b.nb_max = b.band < n ? b.band : n;
    b.lds = key_bytes + (size_t)(kConfBlock + (long)(b.nb_max - 1) * step) * 32;
    return b;
}
// refuses a band whose LDS, with the kernel's static_lds, is above what the device gives a workgroup; `entries` names the
// window's entries in the message.  Needs a context that vap_set_device has accepted.
static int sweep_fits(vap_ctx *ctx, const SweepBands &b, int step, size_t static_lds, const char *entries)
{
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) lds_max = 0;
    const size_t avail = lds_max > 0 && lds_max < 64 * 1024 ? (size_t)lds_max : (size_t)64 * 1024;
    if (b.lds + static_lds > avail)
        return vap_fail(VAP_ERR_UNSUPPORTED, "a band of %d %s at step %d needs %zu bytes of LDS; the device gives a workgroup %zu", b.band,
                        entries, step, b.lds + static_lds, avail);
    return VAP_OK;
}

}  // namespace vap
