"""The cases of the wait-schedule tests (vap_schedule_tables / vap_schedule_solve), shared by the CPU and the GPU tests.

``known``   1 ft squares at heading 0, margin 1/32 ft.  A drives y = 0 from x = -5 at 1/16 ft per row, 161 rows, slots at
            rows 0 and 64.  Partner 1 drives x = 0 from y = -5 at 1/16 ft per row, 161 rows: both reach the origin at row
            80.  Partner 2 drives x = -5 from y = 5 at 1/8 ft per row, 41 rows, and parks on A's start point.  Against
            partner 1 alone A waits at the start; with partner 2 it must leave the start before partner 2 arrives and wait
            out the crossing at row 64: an answer neither a start delay nor a single dwell gives.
``family``  seeded: straight drives through a point within 1 ft of the field centre, 0.05 (A) / 0.06 (partners) ft per row,
            a small random walk on top, a turning heading; R = 6, Bo = 3, capacities 160 / 130 (two and a half 64-row
            blocks), M = 4 with 1 - 4 used slots at random rows, junk behind the counts.
``random_tables``  tables no geometry would produce, entries from {0.5, -0.5, NaN}, for solve against brute.
"""
import numpy as np

UNIT = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])
KNOWN_MARGIN = 1.0 / 32.0
KNOWN_WINDOW = 48                     # C * q
# delay_rows by delay_step, partner 1 alone and both partners
KNOWN_ONE = {1: [33, 0], 2: [34, 0], 4: [36, 0]}
KNOWN_BOTH = {1: [15, 18], 2: [14, 20], 4: [12, 24]}
KNOWN_BOTH_CLEARANCE = 0.0625

FOOT = np.array([[-0.3, -0.25], [0.3, -0.25], [0.3, 0.25], [-0.3, 0.25]])      # 0.6 x 0.5 ft
FAMILY_MARGIN, FAMILY_C, FAMILY_Q = 0.1, 48, 2
FAMILY_SEEDS = range(6)
R, BO, CAP_A, CAP_O, M = 6, 3, 160, 130, 4


def known():
    """(rows_a (1, 161, 8), seg_start (1, 2), rows_o (2, 161, 8), counts_o (2,))."""
    t = np.arange(161, dtype=np.float64)
    a = np.zeros((1, 161, 8))
    o = np.zeros((2, 161, 8))
    a[0, :, 0] = o[:, :, 0] = 0.01 * t
    a[0, :, 6] = -5.0 + t / 16.0
    o[0, :, 7] = -5.0 + t / 16.0
    o[1, :41, 6] = -5.0
    o[1, :41, 7] = 5.0 - np.arange(41) / 8.0
    o[1, 41:, 1:] = np.nan                                     # behind the count
    return a, np.array([[0, 64]], dtype=np.int32), o, np.array([161, 41], dtype=np.int32)


def _drive(rng, cap, n, step):
    """One route of n rows: a straight drive through a point near the centre, a small random walk, a turning heading."""
    rows = np.zeros((cap, 8))
    through = rng.uniform(-1.0, 1.0, 2)
    ang = rng.uniform(0, 2 * np.pi)
    d = np.array([np.cos(ang), np.sin(ang)])
    at = rng.uniform(0.3, 0.7) * n                             # the row at which it passes the point
    t = np.arange(cap, dtype=np.float64)
    xy = through[None, :] + (t - at)[:, None] * step * d[None, :] + np.cumsum(rng.normal(0, 0.004, (cap, 2)), axis=0)
    rows[:, 0] = 0.01 * t
    rows[:, 4] = ang + rng.uniform(-0.01, 0.01) * t
    rows[:, 6:8] = xy
    return rows


def family(seed):
    """(rows_a (R, CAP_A, 8), counts_a (R,), seg_start (R, M), rows_o (BO, CAP_O, 8), counts_o (BO,))."""
    rng = np.random.default_rng(1000 + seed)
    counts_a = rng.integers(CAP_A // 2, CAP_A + 1, R).astype(np.int32)
    counts_o = rng.integers(CAP_O // 2, CAP_O + 1, BO).astype(np.int32)
    rows_a = np.stack([_drive(rng, CAP_A, counts_a[r], 0.05) for r in range(R)])
    rows_o = np.stack([_drive(rng, CAP_O, counts_o[b], 0.06) for b in range(BO)])
    seg = np.full((R, M), -1, dtype=np.int32)
    for r in range(R):
        S = int(rng.integers(1, M + 1))
        seg[r, :S] = np.concatenate([[0], np.sort(rng.choice(np.arange(1, counts_a[r]), S - 1, replace=False))])
    for rows, counts in ((rows_a, counts_a), (rows_o, counts_o)):
        for b in range(len(rows)):
            rows[b, counts[b]:, 1:] = rng.choice([np.nan, np.inf, 1e300, -3.0], size=rows[b, counts[b]:, 1:].shape)
    return rows_a, counts_a, seg, rows_o, counts_o


def random_tables(seed, n, max_s=3, max_c=6, m=None):
    """n cases (move (M, C), wait (M, C), S) with M = m or S .. max_s, entries from {0.5, -0.5, NaN}."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        S = int(rng.integers(0, max_s + 1))
        Mx = m if m is not None else int(rng.integers(max(S, 1), max_s + 1))
        S = min(S, Mx)
        C = int(rng.integers(1, max_c + 1))
        p_block = rng.uniform(0.1, 0.6)
        pick = lambda: rng.choice([0.5, -0.5, np.nan], size=(Mx, C), p=[0.85 - p_block, p_block, 0.15])
        out.append((pick(), pick(), S))
    return out


def classify(total):
    return "none" if total < 0 else ("zero" if total == 0 else "positive")


ROUTINE_DT, ROUTINE_MARGIN, ROUTINE_C, ROUTINE_Q = 0.02, 0.085, 128, 2
ROUTINE_FOOT = np.array([[-0.75, -0.75], [0.75, -0.75], [0.75, 0.75], [-0.75, 0.75]])


def _straight(n, start, heading, length, dt):
    """n rows at constant speed from ``start`` over ``length`` feet; the robot faces phi = -heading."""
    s = np.linspace(0.0, length, n)
    rows = np.zeros((n, 8))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4] = np.arange(n) * dt, s, length / ((n - 1) * dt), heading
    rows[:, 6], rows[:, 7] = start[0] + s * np.cos(-heading), start[1] + s * np.sin(-heading)
    return rows


def routine_scene():
    """Three legs for one routine and two partners, 1.5 ft squares, 20 ms rows.  Leg 0 drives +x from (-2, 0) to the
    origin, leg 1 -y to (0, -5), leg 2 +x to (2, -5).  Partner 0 crosses leg 1 at y = -2 along +x; partner 1 comes down
    x = -2 from y = 6 and parks on the routine's start point.  Returns (legs (3, 150, 8), counts (3,), partners
    (2, 306, 8), partner counts (2,))."""
    dt = ROUTINE_DT
    legs = [_straight(60, (-2.0, 0.0), 0.0, 2.0, dt), _straight(150, (0.0, 0.0), np.pi / 2, 5.0, dt),
            _straight(60, (0.0, -5.0), 0.0, 2.0, dt)]
    rows = np.full((3, 150, 8), np.nan)
    for i, l in enumerate(legs):
        rows[i, :len(l)] = l
    partners = np.full((2, 306, 8), np.nan)
    partners[0] = _straight(306, (-8.0, -2.0), 0.0, 16.0, dt)
    partners[1, :100] = _straight(100, (-2.0, 6.0), np.pi / 2, 6.0, dt)
    return rows, np.array([60, 150, 60], dtype=np.int32), partners, np.array([306, 100], dtype=np.int32)
