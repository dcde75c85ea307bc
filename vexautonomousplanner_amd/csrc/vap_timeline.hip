// vap_timeline.hip — the legs of a routine chained into one timeline (vap_routine_timeline; definitions: include/vap.h).
//
// Per used slot m of a routine the output holds [turn m] [leg m] [dwell m]: the in-place turn from the heading in front to
// the leg's first heading (MPG:487-507 handle_turn over MPG:319-346; vap_turn.h), the leg's rows moved to their place in
// time and distance, and the rows of the dwell at its end.
//
//   k_routine_timeline   one workgroup of 256 threads per (routine, slot), so one routine still spreads over M CUs.  Every
//                        workgroup derives all of its routine's offsets itself: nothing waits across workgroups and there
//                        are no atomics beside the flag OR.
//     prologue   lanes 0 .. M-1 of wave 0 take one slot each: leg index, row count, the used columns of the first and
//                last row, the dwell.  A lane gets the last heading of the slot in front by a shuffle, and from it its
//                turn's row count.  The block sizes (integers) and the leg lengths (fp64) are then summed left to right,
//                slot after slot, every lane running the same sum on shuffled values; the lane of the workgroup's own slot
//                leaves what the body needs in LDS (one struct, 144 bytes).
//     body       thread 0 runs the turn's running sum and stores its rows: serial, because bit equality with the
//                reference's rectangle-rule sum is the point (about 90 rows for a half turn of the default robot at 10 ms).
//                Meanwhile waves 1-3 (all four without a turn) move the leg, four lanes per row and 16 bytes each,
//                consecutive lanes on consecutive pieces, as k_time_waits' row mover does; piece 0 adds the two offsets.
//                The dwell rows follow in the same 16-byte form.
#include <climits>
#include <cmath>
#include <cstdint>

#include "vap_kernels.h"
#include "vap_turn.h"

namespace vap {

constexpr int kTlThreads = 256;
constexpr int kTlRow = 8;   // time, position, velocity, acceleration, heading, angular velocity, x, y

struct TimelineSlot {       // what the body of one (routine, slot) workgroup needs
    long long o_turn, total;            // first output row of the turn block; rows of the whole routine
    double off, h_front, f_pos, f_x, f_y;   // position offset; heading, position and point of the row in front
    double first_h, first_x, first_y, last_h, last_x, last_y, last_pos;
    int n_turn, cnt, n_dwell, leg, bad, n_used, has_front;
};

__device__ inline int tl_sat(long long v) { return v < (long long)INT_MAX ? (int)v : INT_MAX; }

__global__ __launch_bounds__(kTlThreads) void k_routine_timeline(TimelineArgs a)
{
    __shared__ TimelineSlot s_slot;
    const int tid = threadIdx.x, M = a.M;
    const int r = blockIdx.x / M, mine = blockIdx.x - r * M;
    const double dt = a.dt;
    if (tid < 64) {                     // wave 0, all 64 lanes: the shuffles below need every one of them
        int n = a.n_legs ? a.n_legs[r] : M;
        n = n < 0 ? 0 : (n > M ? M : n);
        const bool used = tid < n;
        const double h0 = a.start_heading ? a.start_heading[r] : NAN;
        int leg = -1, cnt = 0, n_dwell = 0;
        double first_h = 0, first_x = 0, first_y = 0, last_h = 0, last_x = 0, last_y = 0, last_pos = 0;
        bool bad = false;
        if (used) {
            leg = a.leg[(size_t)r * M + tid];
            if (leg >= 0 && leg < a.L) {
                cnt = a.counts_in[(size_t)leg * a.counts_stride];
                cnt = cnt > a.cap_in ? a.cap_in : cnt;
            }
            if (cnt > 0) {
                const double *f = a.rows_in + (size_t)leg * a.cap_in * kTlRow;
                const double *l = f + (size_t)(cnt - 1) * kTlRow;
                first_h = f[4]; first_x = f[6]; first_y = f[7];
                last_pos = l[1]; last_h = l[4]; last_x = l[6]; last_y = l[7];
                bad = !(tl_heading_ok(first_h) && tl_finite(first_x) && tl_finite(first_y) && tl_heading_ok(last_h) &&
                        tl_finite(last_x) && tl_finite(last_y));
                const double w = a.dwell ? a.dwell[(size_t)r * M + tid] : 0.0;
                if (w > 0.0) {          // int(dwell / dt), k_time_waits' steps_of
                    const double q = w / dt;
                    n_dwell = q < (double)INT_MAX ? (int)q : INT_MAX;
                }
            } else {
                bad = true;
            }
        }
        if (tid == 0 && h0 == h0 && !tl_heading_ok(h0)) bad = true;
        const bool any_bad = __ballot(bad) != 0ull;
        // the heading in front: the last heading of the slot before, or the start heading (NaN: none)
        const double up = __shfl_up(last_h, 1);
        const double h_front = tid == 0 ? h0 : up;
        int n_turn = 0;
        if (used && !any_bad && h_front == h_front) {
            const double d = tl_wrap_delta(first_h - h_front);
            if (!(fabs(d) < a.turn_min)) n_turn = turn_profile(-d, a.max_vel, a.max_acc, a.track_width, dt).n;
        }
        // left to right over the slots: rows in front of every block, and the fp64 sum of the leg lengths in front
        long long o = 0, my_o = 0;
        double off = 0.0, my_off = 0.0;
        for (int k = 0; k < n; k++) {
            if (k == tid) { my_o = o; my_off = off; }
            o += (long long)__shfl(n_turn, k) + (long long)__shfl(cnt, k) + (long long)__shfl(n_dwell, k);
            off = off + __shfl(last_pos, k);
        }
        const double up_x = __shfl_up(last_x, 1), up_y = __shfl_up(last_y, 1);
        if (tid == mine) {
            TimelineSlot s;
            s.o_turn = my_o; s.total = any_bad ? 0 : o; s.off = my_off; s.h_front = h_front;
            s.has_front = tid > 0;
            // the row in front is the last row of the slot before (or of its dwell): its position is
            // last_pos + off of that slot, which is this slot's off
            s.f_pos = my_off;
            s.f_x = tid > 0 ? up_x : first_x; s.f_y = tid > 0 ? up_y : first_y;
            s.first_h = first_h; s.first_x = first_x; s.first_y = first_y;
            s.last_h = last_h; s.last_x = last_x; s.last_y = last_y; s.last_pos = last_pos;
            s.n_turn = n_turn; s.cnt = cnt; s.n_dwell = n_dwell; s.leg = leg; s.bad = any_bad; s.n_used = n;
            s_slot = s;
        }
    }
    __syncthreads();
    const TimelineSlot s = s_slot;
    const long long cap = a.cap_out;
    if (mine == 0 && tid == 0) {
        a.counts_out[2 * (size_t)r] = (int)(s.total < cap ? s.total : cap);
        a.counts_out[2 * (size_t)r + 1] = s.n_used;
        const uint32_t f = (s.bad ? 8u /* VAP_FLAG_BAD_ROUTE */ : 0u) | (s.total > cap ? 2u /* VAP_FLAG_TRUNCATED */ : 0u);
        if (a.flags && f) atomicOr(&a.flags[r], f);
    }
    int *map = a.map + ((size_t)r * M + mine) * 3;
    double *seam = a.seam + ((size_t)r * M + mine) * 3;
    if (s.bad || mine >= s.n_used) {    // a bad routine, or a slot behind the used ones: no rows
        if (tid < 3) { map[tid] = -1; seam[tid] = NAN; }
        return;
    }
    double *out = a.rows_out + (size_t)r * a.cap_out * kTlRow;
    const long long o_leg = s.o_turn + s.n_turn, o_dwell = o_leg + s.cnt;
    const bool turning = s.n_turn > 0;
    if (tid == 0) {
        map[0] = tl_sat(s.o_turn); map[1] = tl_sat(o_leg); map[2] = tl_sat(o_dwell);
        double h_end = s.h_front;
        if (turning) {                  // handle_turn, MPG:487-507: the heading profile is a running sum (as k_time_waits)
            const double h = s.h_front;
            const TurnProfile p = turn_profile(-tl_wrap_delta(s.first_h - h), a.max_vel, a.max_acc, a.track_width, dt);
            double accum = 0, prev_h = 0;
            for (int j = 0; j < s.n_turn; j++) {
                const double vel = turn_velocity(p, (double)j * dt);
                double hh = accum / p.half_tw * p.sign;
                const double raw = hh;
                accum += vel * dt;
                const double wv = j == 0 ? 0.0 : (raw - prev_h) / dt;   // differences of the UN-wrapped headings
                prev_h = raw;
                while (hh + h > M_PI) hh -= 2 * M_PI;
                while (hh + h < -M_PI) hh += 2 * M_PI;
                h_end = h + hh;
                const long long o = s.o_turn + j;
                if (o >= cap) continue;   // cut: the sum goes on, the seam needs its last heading
                double2 *w = reinterpret_cast<double2 *>(out + (size_t)o * kTlRow);
                w[0] = make_double2((double)o * dt, s.f_pos);
                w[1] = make_double2(0.0, 0.0);
                w[2] = make_double2(h_end, wv);
                w[3] = make_double2(s.f_x, s.f_y);
            }
        }
        seam[0] = s.h_front == s.h_front ? tl_wrap_delta(s.first_h - h_end) : NAN;
        seam[1] = s.has_front ? s.first_x - s.f_x : 0.0;
        seam[2] = s.has_front ? s.first_y - s.f_y : 0.0;
    }
    // the movers: waves 1-3 beside a turn, all four without one
    const int ct = turning ? tid - 64 : tid, nc = turning ? kTlThreads - 64 : kTlThreads;
    if (ct < 0) return;
    {
        const double *in = a.rows_in + (size_t)s.leg * a.cap_in * kTlRow;
        const double t_add = (double)o_leg * dt;
        const long long room = cap - o_leg, n_copy = room < s.cnt ? (room < 0 ? 0 : room) : s.cnt;
        for (long long idx = ct; idx < 4 * n_copy; idx += nc) {
            const long long i = idx >> 2;
            const int piece = (int)(idx & 3);
            double2 v = *reinterpret_cast<const double2 *>(in + (size_t)i * kTlRow + 2 * piece);
            if (piece == 0) { v.x = v.x + t_add; v.y = v.y + s.off; }
            *reinterpret_cast<double2 *>(out + (size_t)(o_leg + i) * kTlRow + 2 * piece) = v;
        }
    }
    {
        const long long room = cap - o_dwell, n_rows = room < s.n_dwell ? (room < 0 ? 0 : room) : s.n_dwell;
        const double pos = s.last_pos + s.off;
        for (long long idx = ct; idx < 4 * n_rows; idx += nc) {
            const long long o = o_dwell + (idx >> 2);
            const int piece = (int)(idx & 3);
            double2 v = make_double2(0.0, 0.0);
            if (piece == 0) v = make_double2((double)o * dt, pos);
            else if (piece == 2) v.x = s.last_h;
            else if (piece == 3) v = make_double2(s.last_x, s.last_y);
            *reinterpret_cast<double2 *>(out + (size_t)o * kTlRow + 2 * piece) = v;
        }
    }
}

hipError_t launch_routine_timeline(hipStream_t st, const TimelineArgs &a)
{
    hipLaunchKernelGGL(k_routine_timeline, dim3((unsigned)(a.R * a.M)), dim3(kTlThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace vap
