"""ctypes binding of libvap.so (include/vap.h).  The ONLY compute backend of this package.

There is no CPU fallback: if the shared library is missing or no HIP device is visible, every
entry point raises.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C vexautonomousplanner_amd/csrc``.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvap.so")

VAP_OK = 0
VAP_ERR_INVALID = -1
VAP_ERR_NO_DEVICE = -2
VAP_ERR_HIP = -3
VAP_ERR_UNFITTED = -4
VAP_ERR_CAPACITY = -5
VAP_ERR_UNSUPPORTED = -6
VAP_F32 = 0
VAP_F64 = 1
FLAG_DEGENERATE = 1
FLAG_TRUNCATED = 2
FLAG_NOCONVERGE = 4
FLAG_BAD_ROUTE = 8
PLAN_SNAPPED_START, PLAN_SNAPPED_GOAL, PLAN_NO_FREE, PLAN_UNREACHABLE, PLAN_VERTICES_TRUNCATED = 16, 32, 64, 128, 256
ORDER_INFEASIBLE = 512
FLAG_ILLCONDITIONED = 1024
PLAN_TRAVEL_MAX_POINTS, PLAN_ORDER_MAX_SITES = 16, 10
PLAN_ORDER_TIMED_MAX_SITES = 8
TIMELINE_MAX_LEGS = 32
T_FIT, T_LUT, T_SAMPLE, T_VELOCITY, T_TOTAL, T_COUNT = 0, 1, 2, 3, 4, 8
OPT_VELOCITY_KERNEL = 0
OPT_TIME_DOMAIN_RESIDUAL = 3
OPT_F32_RECURRENCE = 1
OPT_TIME_KERNEL = 4
OPT_FOOTPRINT_CULL = 5
OPT_CONDITIONING_SCRATCH_MB = 6
TIME_KERNEL_AUTO, TIME_KERNEL_LANE, TIME_KERNEL_QUAD, TIME_KERNEL_FUSED = 0, 1, 2, 3
RECURRENCE_F64, RECURRENCE_F32 = 0, 1
VELOCITY_AUTO, VELOCITY_SEQ_LITERAL, VELOCITY_SEQ_FAST, VELOCITY_RELAX = 0, 1, 2, 3
VELOCITY_RELAX_BLOCK, VELOCITY_RELAX_WAVE = 4, 5
VELOCITY_LANES, VELOCITY_LANES_16, VELOCITY_LANES_32, VELOCITY_LANES_64 = 6, 7, 8, 9
VELOCITY_RELAX_ROUNDS = 10
LUT_SAMPLES = 1000
SAMPLES_PER_NODE = 1000
CLOSEST_GUI, CLOSEST_EXACT = 0, 1
CLOSEST_MODES = {"gui": CLOSEST_GUI, "exact": CLOSEST_EXACT}
CONFLICT_ALL_PAIRS, CONFLICT_MATCHED = 0, 1
HOLD_A_FIRST, HOLD_A_LAST, HOLD_O_FIRST, HOLD_O_LAST = 1, 2, 4, 8
CONFLICT_SHIFTS_MAX = 4096
SCHEDULE_MAX_DELAYS = 4096
FOLLOWER_RAMSETE, FOLLOWER_PURSUIT = 0, 1
# vap_range_readings: a reading's status, and the limits
RANGE_VALID, RANGE_NONE, RANGE_NEAR, RANGE_FAR, RANGE_OBLIQUE, RANGE_BLOCKED, RANGE_BAD_POSE = 0, 1, 2, 3, 4, 5, 6
RANGE_MAX_SENSORS, RANGE_MAX_PARTNERS = 8, 16


def closest_mode(mode):
    """"gui" | "exact" (or VAP_CLOSEST_GUI / VAP_CLOSEST_EXACT) -> the C-ABI value."""
    if mode in (CLOSEST_GUI, CLOSEST_EXACT) and not isinstance(mode, bool):
        return int(mode)
    try:
        return CLOSEST_MODES[str(mode).lower()]
    except KeyError:
        raise ValueError(f"closest-point mode must be 'gui' or 'exact' (got {mode!r})") from None

# every symbol include/vap.h declares; tests check the library exports exactly these
EXPORTS = (
    "vap_version", "vap_status_string", "vap_last_error", "vap_device_count", "vap_ctx_create",
    "vap_ctx_destroy", "vap_ctx_set_stream", "vap_ctx_synchronize", "vap_ctx_set_option",
    "vap_ctx_set_timing",
    "vap_last_timing", "vap_fit", "vap_build_lut", "vap_sample", "vap_velocity_pass",
    "vap_time_profile", "vap_profile_batch", "vap_profile_batch_host", "vap_eval_host", "vap_basis_host", "vap_lookup_host",
    "vap_route_create", "vap_route_destroy", "vap_route_info", "vap_route_set_table_sizes", "vap_route_table_sizes", "vap_route_get_splines", "vap_route_eval",
    "vap_route_lookup", "vap_route_sample_count", "vap_route_forward_backward", "vap_route_motion_profile",
    "vap_grid_distances", "vap_route_limits", "vap_velocity_pass_limits", "vap_time_insert_waits", "vap_fit_ex",
    "vap_profile_routes", "vap_time_profile_routes", "vap_time_insert_events", "vap_limit_rows_dtype",
    "vap_closest_points", "vap_route_closest", "vap_footprint_clearance", "vap_footprint_conflicts",
    "vap_conflict_shifts", "vap_schedule_tables", "vap_schedule_solve",
    "vap_tracking_rollouts", "vap_pursuit_rollouts", "vap_rollout_clearance", "vap_rollout_conflicts", "vap_search_sample", "vap_search_update", "vap_plan_grid", "vap_plan_seeds",
    "vap_plan_occupancy", "vap_plan_seeds_occupied", "vap_plan_travel", "vap_plan_order",
    "vap_routine_timeline", "vap_plan_order_timed", "vap_velocity_conditioning",
    "vap_curve_caps", "vap_drive_audit", "vap_range_readings", "vap_odometry_rollouts",
)


class Constraints(C.Structure):
    """vap_constraints == motion_profile_generator.Constraints field order (MPG:14-21)."""
    _fields_ = [("max_vel", C.c_double), ("max_acc", C.c_double), ("max_dec", C.c_double),
                ("friction_coef", C.c_double), ("max_jerk", C.c_double), ("track_width", C.c_double)]


class FollowerStruct(C.Structure):
    """vap_follower (include/vap.h)."""
    _fields_ = [("track_width", C.c_double), ("b", C.c_double), ("zeta", C.c_double), ("wheel_speed_max", C.c_double),
                ("tolerance", C.c_double), ("n_substeps", C.c_int), ("settle_rows", C.c_int)]


class PursuitStruct(C.Structure):
    """vap_pursuit (include/vap.h)."""
    _fields_ = [("track_width", C.c_double), ("lookahead", C.c_double), ("min_speed", C.c_double), ("arrive_tolerance", C.c_double),
                ("wheel_speed_max", C.c_double), ("tolerance", C.c_double), ("n_substeps", C.c_int), ("settle_rows", C.c_int)]


class ResetRuleStruct(C.Structure):
    """vap_reset_rule (include/vap.h)."""
    _fields_ = [("gate", C.c_double), ("min_cos", C.c_double), ("gain", C.c_double), ("every", C.c_int)]


class SearchWeights(C.Structure):
    """vap_search_weights (include/vap.h)."""
    _fields_ = [("w_time", C.c_double), ("w_length", C.c_double), ("w_violation", C.c_double), ("infeasible_base", C.c_double),
                ("clearance_margin", C.c_double), ("conflict_margin", C.c_double), ("tracking_tolerance", C.c_double)]


class CurveLimitsStruct(C.Structure):
    """vap_curve_limits (include/vap.h)."""
    _fields_ = [("lateral_acc_max", C.c_double), ("angular_acc_max", C.c_double)]


class DriveLimitsStruct(C.Structure):
    """vap_drive_limits (include/vap.h)."""
    _fields_ = [("track_width", C.c_double), ("wheel_speed_max", C.c_double), ("wheel_acc_max", C.c_double),
                ("jerk_max", C.c_double), ("lateral_acc_max", C.c_double), ("angular_acc_max", C.c_double)]


ip = C.POINTER(C.c_int)


class RouteDesc(C.Structure):
    """vap_route_desc (include/vap.h)."""
    _fields_ = [("n_nodes", C.c_int), ("waypoints", C.POINTER(C.c_double)), ("is_reverse", C.POINTER(C.c_int)),
                ("turn", C.POINTER(C.c_double)), ("stop", C.POINTER(C.c_int)), ("wait_time", C.POINTER(C.c_double)),
                ("max_velocity", C.POINTER(C.c_double)), ("max_acceleration", C.POINTER(C.c_double)),
                ("tangent", C.POINTER(C.c_double)), ("magnitudes", C.POINTER(C.c_double)),
                ("n_actions", C.c_int), ("ap_t", C.POINTER(C.c_double)), ("ap_stop", C.POINTER(C.c_int)),
                ("ap_wait_time", C.POINTER(C.c_double)), ("ap_max_velocity", C.POINTER(C.c_double)),
                ("ap_max_acceleration", C.POINTER(C.c_double))]


class VapError(RuntimeError):
    def __init__(self, status, where, detail):
        self.status = status
        super().__init__(f"{where}: {detail} (vap_status {status})")


_lib = None
vp = C.c_void_p
dp = C.POINTER(C.c_double)
u32p = C.POINTER(C.c_uint32)


def lib():
    """Load libvap.so once.  Raises ImportError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `make -C vexautonomousplanner_amd/csrc`).  This package has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; load it FIRST so libvap.so binds to the same HIP
    # runtime instance as the tensors it is handed (two runtimes in one process do not share
    # devices or streams).  A plain C caller links libvap.so against /opt/rocm as usual.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.vap_version.restype = C.c_int
    L.vap_status_string.restype = C.c_char_p
    L.vap_status_string.argtypes = [C.c_int]
    L.vap_last_error.restype = C.c_char_p
    L.vap_device_count.restype = C.c_int
    L.vap_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.vap_ctx_destroy.argtypes = [vp]
    L.vap_ctx_set_stream.argtypes = [vp, vp]
    L.vap_ctx_synchronize.argtypes = [vp]
    L.vap_ctx_set_timing.argtypes = [vp, C.c_int]
    L.vap_ctx_set_option.argtypes = [vp, C.c_int, C.c_int]
    L.vap_last_timing.argtypes = [vp, C.POINTER(C.c_float)]
    L.vap_fit.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.vap_fit_ex.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [vp] * 13
    L.vap_build_lut.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.vap_sample.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp,
                             vp, vp, vp, vp, vp, vp]
    L.vap_velocity_pass.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(Constraints),
                                    C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]
    L.vap_profile_batch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp,
                                    C.POINTER(Constraints), C.c_double, C.c_double,
                                    vp, vp, vp, vp, vp, vp, vp]
    L.vap_profile_batch_host.argtypes = L.vap_profile_batch.argtypes
    L.vap_profile_routes.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, vp, vp, vp,
                                     C.POINTER(Constraints), C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
    L.vap_time_profile.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp,
                                   C.POINTER(Constraints), C.c_double, C.c_int, vp, vp, vp, vp]
    L.vap_route_limits.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 9 + [C.POINTER(Constraints), C.c_double] + [vp] * 6
    L.vap_velocity_pass_limits.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(Constraints), C.c_double, C.c_double,
                                           vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.vap_limit_rows_dtype.argtypes = [vp, C.c_int]
    L.vap_time_insert_waits.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double] + [vp] * 14
    L.vap_time_profile_routes.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(Constraints), C.c_double,
                                          C.c_int, vp, vp, vp, vp, vp]
    L.vap_time_insert_events.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(Constraints)] + [vp] * 14
    L.vap_eval_host.argtypes = [vp, C.c_int, dp, C.c_double, C.c_int, C.c_int, dp, dp]
    L.vap_basis_host.argtypes = [vp, C.c_int, C.c_int, dp, dp]
    L.vap_lookup_host.argtypes = [vp, C.c_int, dp, C.c_double, dp, C.c_int, C.c_int, dp, dp]
    lp = C.POINTER(C.c_long)
    L.vap_route_create.argtypes = [vp, C.POINTER(RouteDesc), C.POINTER(vp)]
    L.vap_route_destroy.argtypes = [vp]
    L.vap_route_info.argtypes = [vp, ip, dp]
    L.vap_route_set_table_sizes.argtypes = [vp, C.c_int, C.c_int]
    L.vap_route_table_sizes.argtypes = [vp, ip, ip]
    L.vap_route_get_splines.argtypes = [vp, ip, ip, dp, dp, dp, dp, dp]
    L.vap_route_eval.argtypes = [vp, C.c_int, C.c_int, dp, dp]
    L.vap_route_lookup.argtypes = [vp, C.c_int, C.c_int, dp, dp]
    L.vap_route_sample_count.argtypes = [vp, C.c_double, ip]
    L.vap_grid_distances.argtypes = [C.c_double, C.c_double, C.c_long, dp, C.POINTER(C.c_long)]
    L.vap_route_forward_backward.argtypes = [vp, C.POINTER(Constraints), C.c_double, C.c_double, C.c_double,
                                             C.c_int, ip, dp, dp, dp, dp, dp, dp]
    L.vap_route_motion_profile.argtypes = [vp, C.POINTER(Constraints), C.c_double, C.c_double, C.c_long, dp, lp,
                                           lp, ip, lp, ip]
    L.vap_closest_points.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 7
    L.vap_route_closest.argtypes = [vp, C.c_int, C.c_int, dp, dp]
    L.vap_footprint_clearance.argtypes = [vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_int, dp, dp, C.c_int, ip, dp,
                                          C.c_int, dp, C.c_double] + [vp] * 6
    side = [C.c_int, C.c_long, vp, vp, C.c_int, C.c_int, dp]
    L.vap_footprint_conflicts.argtypes = [vp, C.c_int, C.c_int, C.c_double] + side + side + [vp] * 8
    L.vap_conflict_shifts.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int] + side + side + \
        [vp] * 6
    L.vap_schedule_tables.argtypes = [vp, C.c_int, C.c_int] + side + [C.c_int, vp] + side + [vp] * 4
    L.vap_schedule_solve.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double] + [vp] * 6
    L.vap_tracking_rollouts.argtypes = [vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_double, C.POINTER(FollowerStruct), C.c_int,
                                        C.c_int, vp] + [vp] * 7 + [C.c_long, vp, vp]
    L.vap_pursuit_rollouts.argtypes = [vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_double, C.POINTER(PursuitStruct), C.c_int,
                                       C.c_int, vp] + [vp] * 9 + [C.c_long, vp, vp]
    L.vap_rollout_clearance.argtypes = [vp, C.c_int, vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, vp,
                                        C.c_int, dp, dp, C.c_int, ip, dp, C.c_int, dp, C.c_double] + [vp] * 18
    L.vap_rollout_conflicts.argtypes = [vp, C.c_int, vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_double, C.c_int, C.c_int, vp,
                                        C.c_int, dp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_int, dp, C.c_double, C.c_int, vp, vp] + \
        [vp] * 20
    L.vap_search_sample.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]
    L.vap_search_update.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_double] + [vp] * 5 + \
        [C.POINTER(SearchWeights), C.c_int, C.c_double, C.c_double, C.c_double] + [vp] * 10 + [C.c_int, C.c_uint32]
    scene = [dp, C.c_int, ip, dp, C.c_int, dp, C.c_double, C.c_double, C.c_double]   # field .. circles, cell, radius, margin
    L.vap_plan_grid.argtypes = [vp] + scene + [vp, vp, ip, ip]
    L.vap_plan_seeds.argtypes = [vp, C.c_int, C.c_int, vp, vp] + scene + [C.c_int] + [vp] * 6
    L.vap_plan_seeds_occupied.argtypes = [vp, C.c_int, C.c_int, vp, vp] + scene + [C.c_int] + [vp] * 3 + [vp] * 6
    L.vap_plan_occupancy.argtypes = [vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, C.c_double,
                                     C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, ip, ip]
    L.vap_plan_travel.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp] + scene + [C.c_int] + [vp] * 3 + [vp] * 4
    L.vap_plan_order.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.vap_routine_timeline.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(Constraints),
                                       C.c_double, vp, vp, C.c_int] + [vp] * 9
    L.vap_plan_order_timed.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(Constraints), C.c_double,
                                       vp, vp, C.c_int] + [vp] * 6 + [C.c_int] + [vp] * 7
    L.vap_velocity_conditioning.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(Constraints), C.c_double, C.c_double] + [vp] * 7 + \
        [C.c_int, C.c_double, C.c_uint64, C.c_uint32, C.c_double] + [vp] * 6
    L.vap_curve_caps.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(Constraints), C.POINTER(CurveLimitsStruct)] + [vp] * 5
    L.vap_drive_audit.argtypes = [vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_double, C.POINTER(DriveLimitsStruct)] + [vp] * 6
    L.vap_range_readings.argtypes = [vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_int, dp, dp, C.c_int, ip, dp, C.c_int, dp,
                                     C.c_int, C.c_long, vp, vp, C.c_int, C.c_int, dp, C.c_int] + [vp] * 6
    L.vap_odometry_rollouts.argtypes = [vp, C.c_int, C.c_long, vp, vp, C.c_int, C.c_double, C.POINTER(FollowerStruct), C.c_int,
                                        C.c_int, vp, C.c_int, vp, C.c_int, dp, C.POINTER(ResetRuleStruct), dp, C.c_int, ip, dp,
                                        C.c_int, dp] + [vp] * 7 + [C.c_long, vp, vp, vp]
    _lib = L
    return L


def check(status, where):
    if status != VAP_OK:
        L = lib()
        detail = L.vap_last_error().decode() or L.vap_status_string(status).decode()
        raise VapError(status, where, detail)


class Context:
    """One device + stream + scratch arena (vap_ctx).  Not thread-safe; make one per thread."""

    def __init__(self, device=0):
        self._L = lib()
        h = vp()
        check(self._L.vap_ctx_create(int(device), C.byref(h)), "vap_ctx_create")
        self.handle = h
        self.device = int(device)

    def close(self):
        if getattr(self, "handle", None):
            self._L.vap_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """stream_ptr: a hipStream_t as int (0 = HIP's default stream); None = the context's own stream."""
        arg = vp(-1 & 0xFFFFFFFFFFFFFFFF) if stream_ptr is None else vp(int(stream_ptr))
        check(self._L.vap_ctx_set_stream(self.handle, arg), "vap_ctx_set_stream")

    def synchronize(self):
        check(self._L.vap_ctx_synchronize(self.handle), "vap_ctx_synchronize")

    def set_option(self, option, value):
        check(self._L.vap_ctx_set_option(self.handle, int(option), int(value)), "vap_ctx_set_option")

    def set_timing(self, enabled=True):
        check(self._L.vap_ctx_set_timing(self.handle, int(bool(enabled))), "vap_ctx_set_timing")

    def last_timing(self):
        ms = (C.c_float * T_COUNT)()
        check(self._L.vap_last_timing(self.handle, ms), "vap_last_timing")
        return {"fit": ms[T_FIT], "lut": ms[T_LUT], "sample": ms[T_SAMPLE],
                "velocity": ms[T_VELOCITY], "total": ms[T_TOTAL]}


_default_ctx = {}


def default_context(device=0):
    """Process-wide context per device (what the single-path drop-in classes use)."""
    ctx = _default_ctx.get(device)
    if ctx is None or ctx.handle is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx


def make_constraints(c):
    """Accept a Constraints-like object (attributes) or a 6-sequence."""
    if isinstance(c, Constraints):
        return c
    if hasattr(c, "max_vel"):
        return Constraints(float(c.max_vel), float(c.max_acc), float(c.max_dec),
                           float(c.friction_coef), float(c.max_jerk), float(c.track_width))
    v = [float(x) for x in c]
    if len(v) != 6:
        raise ValueError("constraints need 6 values: max_vel,max_acc,max_dec,friction_coef,"
                         "max_jerk,track_width")
    return Constraints(*v)
