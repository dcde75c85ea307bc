// vap_turn.h — the in-place turn's wheel-speed profile, shared by the kernels that insert turn rows (k_time_waits,
// k_routine_timeline) or count them (k_plan_order_timed), and the timeline's tests of a leg's end rows.
#pragma once
#include <cmath>

namespace vap {

// MPG:319-346 motion_profile_angle over ODM:4-69 generate_trapezoidal_profile: the rows an in-place turn inserts
struct TurnProfile {
    double t_acc, vpeak, total_time, amax, half_tw, sign;
    int n;
};
__device__ inline TurnProfile turn_profile(double angle, double vmax, double amax, double tw, double dt)
{
    TurnProfile p;
    const double arc = fabs(angle) * tw / 2;
    p.t_acc = vmax / amax;
    const double d_acc = 0.5 * amax * (p.t_acc * p.t_acc);
    p.vpeak = vmax;
    if (2 * d_acc > arc) {
        p.t_acc = sqrt(arc / amax);
        p.vpeak = amax * p.t_acc;
        p.total_time = 2 * p.t_acc;
    } else {
        p.total_time = 2 * p.t_acc + (arc - 2 * d_acc) / p.vpeak;
    }
    p.amax = amax;
    p.half_tw = tw / 2;
    p.sign = angle > 0 ? -1.0 : 1.0;
    p.n = (int)ceil((p.total_time + dt) / dt);   // np.arange(0, total_time + dt, dt)
    return p;
}
__device__ inline double turn_velocity(const TurnProfile &p, double tt)
{
    if (tt <= p.t_acc) return p.amax * tt;
    if (tt <= p.total_time - p.t_acc) return p.vpeak;
    return p.vpeak - p.amax * (tt - (p.total_time - p.t_acc));
}

// what makes a leg's first or last row usable in a timeline, and the change of heading a turn covers: shared by
// k_routine_timeline and k_plan_order_timed, so that the order's rows are the timeline's
__device__ inline bool tl_heading_ok(double h) { return fabs(h) <= 2 * M_PI; }   // false for NaN and the infinities
__device__ inline bool tl_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }
__device__ inline double tl_wrap_delta(double d)
{
    if (d > M_PI) d -= 2 * M_PI;
    if (d <= -M_PI) d += 2 * M_PI;
    return d;
}

}  // namespace vap
