"""Host replica of the kinematic recurrence of the time-domain resample (MPG:566-584), in plain Python fp64.

This is the reference of the bit comparisons in test_gpu_time.py: a statement-by-statement restatement of the loop of
generate_motion_profile that follows forward_backward_pass, with every division a true IEEE division and no fused
multiply-add (Python floats are IEEE doubles, each operation rounded once).  test_time_cpu.py pins it bit for bit on
the oracle's generate_motion_profile, which the golden vectors pin on the real reference.

It imports nothing from the package under test.
"""
import numpy as np

# int(wait_time / dt) where the quotient rounds just below an integer (the reference drops a row there, MPG:460, 510)
# and where it is exact.  Evaluated by Python; test_time_cpu.py asserts every entry, so the GPU tests' expectations
# do not come from the kernel.  A kernel that multiplied by the rounded 1/dt would give 7, 3, 3 at 0.05 and 0.1.
WAIT_EDGE_STEPS = {
    (0.29, 0.01): 28, (0.57, 0.01): 56, (0.58, 0.01): 57,
    (0.35, 0.05): 6, (0.15, 0.05): 2, (0.3, 0.1): 2,
    (0.07, 0.01): 7, (0.06, 0.02): 3,
}


def grid_index(x, dd, n):
    """The i in [-1, n-1] with i*dd <= x < (i+1)*dd, products as rounded: np.searchsorted(xs, x, side="right") - 1 over
    xs[i] = i*dd (MPG:366, 484) by bisection, as the oracle does it."""
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) // 2
        if not (x < float(mid) * dd):
            lo = mid + 1
        else:
            hi = mid
    return lo - 1


def lerp_grid(x, dd, ys, n):
    """MPG:349-386 over x_array[i] = i*dd: the end values outside the grid, a true division inside."""
    idx = grid_index(x, dd, n)
    if idx < 0:
        return ys[0]
    if idx >= n - 1:
        return ys[n - 1]
    x0, x1 = float(idx) * dd, float(idx + 1) * dd
    y0, y1 = ys[idx], ys[idx + 1]
    return y0 + (x - x0) * (y1 - y0) / (x1 - x0)


def _clip(x, lo, hi):
    # np.clip for ordered, non-NaN bounds: the lower bound first, then the upper one
    m = lo if x < lo else x
    return hi if m > hi else m


def integrate(velocity, total, dd, dt, max_acc, max_dec, capacity):
    """MPG:413-418, 523, 566-584 for one path.

    velocity   the distance-domain velocity row, sample i at i*dd (any float type; read as fp64)
    total      the path's arc length; dd the grid step; dt the time step
    capacity   rows at most: a path that needs more is cut there (``truncated``)
    Returns (rows, count, truncated): rows is (count, 5) fp64 = time, position, velocity, acceleration, target
    velocity of every time step.
    """
    ys = [float(v) for v in np.asarray(velocity, dtype=np.float64)]
    n = len(ys)
    dd, dt, total = float(dd), float(dt), float(total)
    max_acc, max_dec = float(max_acc), float(max_dec)
    current_time, current_pos = 0.0, 0.0
    current_vel = ys[0] if n else 0.0
    out = []
    truncated = False
    while current_pos < total:                                                  # MPG:523
        if len(out) >= capacity:
            truncated = True
            break
        target_vel = lerp_grid(current_pos, dd, ys, n)                          # MPG:568
        next_target_vel = lerp_grid(current_pos + dd, dd, ys, n)                # MPG:569
        target_vel = (target_vel + next_target_vel) / 2                         # MPG:570
        if not (target_vel > 0.001):
            target_vel = 0.001
        accel = _clip((target_vel - current_vel) / dt, -max_dec, max_acc)       # MPG:573-575
        current_vel = _clip(current_vel + accel * dt, 0.0, target_vel)          # MPG:579
        delta_pos = current_vel * dt + 0.5 * accel * dt * dt                    # MPG:580
        if current_vel <= 0.1:
            delta_pos = 0.1 * dt + 0.5 * accel * dt * dt                        # MPG:581-582
        current_pos += delta_pos
        out.append((current_time, current_pos, current_vel, accel, target_vel))
        current_time += dt                                                      # MPG:600
    rows = np.array(out, dtype=np.float64).reshape(len(out), 5)
    return rows, len(out), truncated
