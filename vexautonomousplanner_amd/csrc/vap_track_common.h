// vap_track_common.h — what the follower rollouts share (vap_tracking.hip: RAMSETE; vap_pursuit.hip: pure pursuit):
// the angle wrap, sinc, and the fixed-order summary of a route's rollouts.
#pragma once
#include <cmath>

namespace vap {

constexpr int kTrackThreads = 256;
constexpr double kPi = 3.14159265358979323846;

// ((a + pi) mod 2 pi) - pi with the floored mod (MPG:560-562); fmod is exact
__device__ __forceinline__ double track_wrap(double a)
{
    double m = fmod(a + kPi, 2.0 * kPi);
    if (m < 0.0) m += 2.0 * kPi;
    return m - kPi;
}

__device__ __forceinline__ double track_sinc(double x, double sin_x)
{
    return fabs(x) < 1e-4 ? 1.0 - x * x / 6.0 : sin_x / x;
}

// wheel-speed saturation that keeps c_L : c_R (hence the curvature); true where the row is saturated
__device__ __forceinline__ bool track_saturate(double &cl, double &cr, double wmax)
{
    const double mx = fmax(fabs(cl), fabs(cr));
    if (mx > wmax) {
        const double scale = wmax / mx;
        cl *= scale;
        cr *= scale;
        return true;
    }
    return false;
}

// the plant of one rollout: the wheel gains, T * track_scale, the lag's a = 1 - exp(-h / tau); the pose, the actual wheel
// speeds and the distance travelled
struct TrackPlant {
    double gl = 1.0, gr = 1.0, tts = 1.0, a = 1.0;
    double x = 0.0, y = 0.0, phi = 0.0, wl = 0.0, wr = 0.0, dist = 0.0, vprev = 0.0;

    // the executed row r in the time-profile layout, four 16-byte stores
    __device__ __forceinline__ void write_row(double *erow, int r, double dt)
    {
        const double v = (gl * wl + gr * wr) / 2.0;
        const double om = (gr * wr - gl * wl) / tts;
        double2 *o = (double2 *)(erow + (size_t)r * 8);
        o[0] = make_double2((double)r * dt, dist);
        o[1] = make_double2(v, r > 0 ? (v - vprev) / dt : 0.0);
        o[2] = make_double2(-track_wrap(phi), -om);
        o[3] = make_double2(x, y);
        vprev = v;
    }

    // nsub substeps of h towards the commands: first-order wheel lag, then the exact arc
    __device__ __forceinline__ void advance(double cl, double cr, int nsub, double h)
    {
#pragma unroll 1
        for (int s = 0; s < nsub; s++) {
            wl += (cl - wl) * a;
            wr += (cr - wr) * a;
            const double v = (gl * wl + gr * wr) / 2.0;
            const double om = (gr * wr - gl * wl) / tts;
            const double u = om * h / 2.0;
            double sa, ca;
            sincos(phi + u, &sa, &ca);
            const double d = v * h * track_sinc(u, sin(u));
            x += d * ca;
            y += d * sa;
            phi += om * h;
            dist += fabs(d);
        }
    }
};

// a route's rollouts in ascending k: worst (a strictly larger error replaces: the smallest k stays), running sum, count
// above the tolerance.  `Args` carries the per-route output pointers worst, mean, worst_rollout, worst_row, n_exceeding.
struct TrackSummary {
    double worst = -INFINITY, sum = 0.0;
    int k = -1, row = -1, cnt = 0, nex = 0;
    __device__ void take(double e, int r, int kk, double tol)
    {
        if (r < 0) return;
        if (e > worst) { worst = e; k = kk; row = r; }
        sum += e;
        cnt++;
        nex += e > tol ? 1 : 0;
    }
    template <class Args>
    __device__ void store(const Args &g, int b) const
    {
        if (g.worst) g.worst[b] = cnt ? worst : NAN;
        if (g.mean) g.mean[b] = cnt ? sum / (double)cnt : NAN;
        if (g.worst_rollout) g.worst_rollout[b] = k;
        if (g.worst_row) g.worst_row[b] = row;
        if (g.n_exceeding) g.n_exceeding[b] = nex;
    }
};

}  // namespace vap
