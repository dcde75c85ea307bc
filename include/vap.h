/* vap.h — C-ABI of libvap.so: MI355X-native batched trajectory generator.
 *
 * Drop-in boundary for the quintic-Hermite spline + 2-D motion-profile hot path of
 * RohitMovva/VexAutonomousPlanner.  The reference has no FFI of its own (it is pure Python); each
 * entry point below names the reference function(s) it replaces (file:line under the reference's
 * src/), and INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 *   QHS = splines/quintic_hermite_spline.py      SM = splines/spline_manager.py
 *   MPG = motion_profiling_v2/motion_profile_generator.py
 *
 * Conventions
 *   - plain C types only; every buffer is caller-owned; the library keeps no pointer after a call.
 *   - "d_" pointers are DEVICE (HBM) pointers valid on the context's device; "h_" pointers are host.
 *   - all entry points return 0 (VAP_OK) or a negative vap_status; none of them throws.
 *   - work is enqueued on the context's HIP stream (vap_ctx_set_stream); "_host" variants and
 *     vap_ctx_synchronize block, the device-pointer variants do not.
 *   - units: feet, seconds, radians.
 *
 * Precision (`vap_dtype`):
 *   VAP_F32  fp32 inputs/outputs.  Parameter/index arithmetic, derivative evaluation, curvature, heading
 *            differences and the velocity recurrence are carried in fp64 on the device (the reference's
 *            table/step-lookup quantisation, its finite-difference angular-acceleration term and the
 *            error amplification of its recurrence in tight curves are not reproducible to 1e-5
 *            otherwise); positions, headings and all stores are fp32.
 *            VAP_OPT_F32_RECURRENCE selects an all-fp32 recurrence instead.
 *   VAP_F64  fp64 inputs/outputs, all arithmetic fp64.  Not every operation is the reference's correctly rounded one:
 *            reciprocals, 1/sqrt and the final square root of a velocity come from the hardware estimates refined by
 *            Newton steps (within an ulp), the recurrence runs in its collapsed four-instruction form,
 *            and atan2 / pow are the device library's, not NumPy's.  Measured against the real reference: velocities
 *            <= 4.1e-11 on the curated fixtures, <= 4e-8 on 60 000 random shapes and robots, and 1.9e-6 on the worst case
 *            found (fixture big_w2048_p2: 2048 waypoints, 4e5 samples) — where the statement-by-statement sweep
 *            (VAP_VELOCITY_SEQ_LITERAL) gives the same 1.9e-6 and the fp64 CPU restatement itself is 7.9e-8 from the
 *            reference: the reference's own recurrence amplifies last-bit differences of its inputs by up to 1e9
 *            there.  The bound that holds for both dtypes on every path tried is north_star's 1e-5.
 *            vap_velocity_conditioning measures that amplification per path and names the paths in that regime.
 */
#ifndef VAP_H
#define VAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAP_VERSION 100

typedef enum {
    VAP_OK = 0,
    VAP_ERR_INVALID = -1,     /* bad argument (NULL, W < 2, S < 2, ...): reference returns False */
    VAP_ERR_NO_DEVICE = -2,   /* no usable HIP device: the product never falls back to the CPU */
    VAP_ERR_HIP = -3,         /* a HIP runtime call failed; vap_last_error() has the text */
    VAP_ERR_UNFITTED = -4,    /* evaluator called before fit/build (reference: ValueError) */
    VAP_ERR_CAPACITY = -5,    /* output capacity S too small for the requested grid */
    VAP_ERR_UNSUPPORTED = -6
} vap_status;

typedef enum { VAP_F32 = 0, VAP_F64 = 1 } vap_dtype;

/* MPG:14-21 Constraints dataclass, same field order. */
typedef struct {
    double max_vel, max_acc, max_dec, friction_coef, max_jerk, track_width;
} vap_constraints;

/* Per-path flag bits written to flags[b].
 *
 * A path flagged VAP_FLAG_DEGENERATE (two equal neighbouring waypoints, a path of zero length, a NaN or infinite
 * coordinate, coordinates whose squared distances overflow or underflow) lives in its batch on these terms, held by
 * tests/test_gpu_bad_paths.py:
 *   - its rows (x, y, heading, curvature, velocity, time-domain rows) are unspecified and may be non-finite; meta[0..2]
 *     may be NaN;
 *   - its meta[3] is an integer in [0, S] and its time-domain row count lies in [0, capacity_rows]: nothing is written
 *     outside the rows the caller gave it;
 *   - no other path's outputs or flags depend on it: the rows, meta and flags of every other path of the call are, bit for
 *     bit, those of the same batch with a good path in its place — in the fused and the staged calls, vap_profile_routes,
 *     fp32 / fp64 rows and the fp32 recurrence, every velocity kernel option but VAP_VELOCITY_RELAX_ROUNDS and the long-row
 *     look-back kernel (a row per launch group: no sharing), the three time-domain kernels, vap_time_insert_events,
 *     vap_route_limits + vap_velocity_pass_limits, vap_curve_caps, vap_velocity_conditioning and vap_closest_points;
 *   - vap_search_update reads its flag as cost +inf and ranks it behind every finite candidate. */
#define VAP_FLAG_DEGENERATE 1u /* zero-length segment or non-finite value met during fit/LUT */
#define VAP_FLAG_TRUNCATED 2u  /* grid needed more than S samples; the first S were produced */
#define VAP_FLAG_NOCONVERGE 4u /* velocity relaxation hit its round limit (never expected) */

/* Timing slots of vap_last_timing (milliseconds, HIP events on the context's stream). */
enum { VAP_T_FIT = 0, VAP_T_LUT = 1, VAP_T_SAMPLE = 2, VAP_T_VELOCITY = 3, VAP_T_TOTAL = 4,
       VAP_T_COUNT = 8 };

#define VAP_LUT_SAMPLES 1000      /* SM:427 min_samples */
#define VAP_SAMPLES_PER_NODE 1000 /* SM:477 samples_per_node */

typedef struct vap_ctx vap_ctx;

/* ---- context ------------------------------------------------------------------------------- */
int vap_version(void);
const char *vap_status_string(int status);
/* Thread-local text of the last failure in this thread ("" if none). */
const char *vap_last_error(void);
/* Number of HIP devices visible (0 when there is none; never initialises a context). */
int vap_device_count(void);
/* One context = one device + one stream + its scratch arena.  Not thread-safe; one per thread. */
int vap_ctx_create(int device, vap_ctx **out);
int vap_ctx_destroy(vap_ctx *ctx);
/* Run subsequent work on `hip_stream` (a hipStream_t, e.g. torch's current stream; NULL is HIP's
 * default stream).  VAP_STREAM_OWN selects the context's own non-blocking stream again (the initial
 * state). */
#define VAP_STREAM_OWN ((void *)(intptr_t)-1)
int vap_ctx_set_stream(vap_ctx *ctx, void *hip_stream);
int vap_ctx_synchronize(vap_ctx *ctx);
/* Tuning / test knobs.  VAP_OPT_VELOCITY_KERNEL selects the K5 implementation: AUTO (default) picks
 * the register-resident relaxation kernel when the row fits and the sequential sweep otherwise;
 * SEQ_LITERAL is the statement-by-statement form of MPG:188-311, SEQ_FAST the same sweep with the
 * collapsed limits (bit-identical to RELAX).  RELAX_BLOCK is the workgroup-per-path kernel RELAX uses;
 * RELAX_WAVE (fp32) walks each path with one wave in stream-ordered windows — exact as well, kept for
 * experiments (slower on MI355X for the sizes measured).  LANES (fp64 recurrence) is "a wavefront of paths": a
 * lane walks a path, 16-64 paths per workgroup, coefficients streamed through LDS by producer waves — every
 * sample evaluated once per direction, bit-identical to SEQ_FAST, any row length; AUTO picks it for batches of
 * 2048 paths and more.  LANES_16 / _32 / _64 force its group size (tests).  Rows too long for the register-resident
 * kernel (config 2) are cut into super-chunks whose interface states are handed on by look-back inside one launch per
 * direction; RELAX_ROUNDS forces the earlier form of that kernel (one launch per super-round, convergence checked
 * on the host) — the same rows bit for bit (tests). */
enum { VAP_OPT_VELOCITY_KERNEL = 0, VAP_OPT_F32_RECURRENCE = 1, /* 2: retired (sampling inside the velocity kernel, rounds 3-4) */
       VAP_OPT_TIME_DOMAIN_RESIDUAL = 3, VAP_OPT_TIME_KERNEL = 4, VAP_OPT_FOOTPRINT_CULL = 5,
       VAP_OPT_CONDITIONING_SCRATCH_MB = 6 };
enum { VAP_VELOCITY_AUTO = 0, VAP_VELOCITY_SEQ_LITERAL = 1, VAP_VELOCITY_SEQ_FAST = 2, VAP_VELOCITY_RELAX = 3,
       VAP_VELOCITY_RELAX_BLOCK = 4 /* workgroup per path */, VAP_VELOCITY_RELAX_WAVE = 5 /* wave per path, fp32 */,
       VAP_VELOCITY_LANES = 6 /* lane per path, fp64 recurrence */, VAP_VELOCITY_LANES_16 = 7, VAP_VELOCITY_LANES_32 = 8,
       VAP_VELOCITY_LANES_64 = 9, VAP_VELOCITY_RELAX_ROUNDS = 10 /* long rows: host-checked super-rounds */ };
/* VAP_OPT_F32_RECURRENCE: arithmetic of the forward/backward velocity recurrence in VAP_F32 calls.
 *   VAP_RECURRENCE_F64 (default): the sampling kernel keeps fp64 curvature / heading-difference rows in
 *     context scratch and the recurrence runs in fp64 on them; inputs and every output row stay fp32.  The
 *     reference's recurrence amplifies a rounding error by track_width*curvature/2 per step in curves tighter
 *     than 2/track_width, so only this mode holds 1e-5 against the reference on every path.
 *   VAP_RECURRENCE_F32: rows and recurrence in fp32 — faster, and within 1e-5 on ~98.6 % of config-3-shaped
 *     paths (worst sample 7e-5). */
enum { VAP_RECURRENCE_F64 = 0, VAP_RECURRENCE_F32 = 1 };
/* VAP_OPT_TIME_DOMAIN_RESIDUAL (1 = on, the default; 0 = off): VAP_F32 calls with the fp64 recurrence also leave, in
 * context scratch, what each stored fp32 velocity lost of the fp64 value (an fp32 residual row, 4 B per sample-point of
 * extra writes).  A following vap_time_profile / vap_time_profile_routes that is handed that velocity row integrates
 * row + residual (MPG:566-584) — the caller's row as it is at that moment plus a term below its own rounding — which
 * is what keeps fp32 time-domain rows within 1e-5 of the reference.  Callers that never go to the time domain (pure
 * distance-domain batches, e.g. candidate ranking) switch it off and save the traffic. */
/* VAP_OPT_TIME_KERNEL: the kinematic recurrence of vap_time_profile[_routes] (MPG:566-584).  LANE walks a path with one
 * lane; QUAD with four (one grid index, one velocity sample and one interpolation per lane instead of two, four and two,
 * the 64-byte row stored as four 16-byte pieces) — the same rows bit for bit, a shorter step.  AUTO (default) takes
 * QUAD while four lanes per path still leave at most one wavefront per SIMD (B <= 16384) and LANE above that.
 * FUSED: QUAD's recurrence and the geometry of the rows behind it in one workgroup of 16 plain paths (the geometry runs in
 * the shadow of the recurrence); AUTO takes it while that is at most one workgroup per CU (B <= 16 x CUs), and batches of
 * routes (vap_time_profile_routes) never do. */
enum { VAP_TIME_KERNEL_AUTO = 0, VAP_TIME_KERNEL_LANE = 1, VAP_TIME_KERNEL_QUAD = 2, VAP_TIME_KERNEL_FUSED = 3 };
/* VAP_OPT_FOOTPRINT_CULL (1 = on, the default; 0 = off): vap_footprint_clearance skips, per row, every element whose
 * bounding-circle lower bound exceeds the row's running minimum (plus a small slack).  A skipped element could not have
 * become the row's minimum, so every output is the same bit for bit either way; 0 tests every element (tests).
 * vap_footprint_conflicts: the same switch for its block and row bounds (0 tests every row of every pair exactly). */
/* VAP_OPT_CONDITIONING_SCRATCH_MB (1 .. 16384, default 512): the context scratch vap_velocity_conditioning may hold at a
 * time, in MiB.  The call cuts its batch into launches whose probe rows fit (one path's rows at the least); its outputs do
 * not depend on the cut. */
int vap_ctx_set_option(vap_ctx *ctx, int option, int value);
/* Enable/disable per-stage hipEvent timing (replaces the reference's time.time() log lines,
 * SM:587-594, MPG:398-411).  Off by default. */
int vap_ctx_set_timing(vap_ctx *ctx, int enabled);
int vap_last_timing(vap_ctx *ctx, float ms[VAP_T_COUNT]);

/* ---- staged device API (plain-node paths: one spline of W control points per path) ----------
 * Buffers, for a batch of B paths with W waypoints (G = W-1 segments) and sample capacity S:
 *   waypoints  [B][W][2]                 dtype
 *   segments   [B][G][6][2]   fp64       rows p0,p1,d0*L,d1*L,dd0*L^2,dd1*L^2 (QHS:92-122)
 *   lut        [B][1000]      fp64       lookup_table.distances (SM:448-454); parameters are
 *                                        j * param_last/999 (np.linspace) and are not stored
 *   meta       [B][4]         fp64       {parameters[-1] (QHS:736), total_length, dd, n_samples}
 *   x,y,heading,curvature,velocity [B][S] dtype
 */

/* QHS:30-138 fit + QHS:149-219 _compute_derivatives + QHS:719-736 _compute_parameters, batched;
 * also SM:42-172 build_path for plain nodes.  d_tangent_in/out: optional [B][W][2] fp64 per-node
 * tangent overrides (NaN = None; SM:65-77, QHS:102-115), or NULL. */
int vap_fit(vap_ctx *ctx, vap_dtype dt, int B, int W, const void *d_waypoints,
            const double *d_tangent_in, const double *d_tangent_out, double *d_segments,
            double *d_segment_lengths /* [B][G] fp64, QHS:84-85, may be NULL */, double *d_meta,
            uint32_t *d_flags);

/* vap_fit with the rest of QuinticHermiteSpline.fit's own inputs (QHS:30-138), for callers that use the spline
 * class directly as SM:57-168 does for the splines of a split route:
 *   d_first_derivatives / d_second_derivatives  [B][W][2] fp64: used only when BOTH are given (QHS:52-68: with
 *       one missing, _compute_derivatives overwrites both)
 *   d_starting_tangent / d_ending_tangent       [B][2] fp64, NaN row = not set: QHS:129-132 -> set_starting_tangent /
 *       set_ending_tangent (QHS:543-590) — both write into the LAST segment (quirk Q3) — and the 2-point special
 *       case of _compute_derivatives (QHS:170-172, 181-182: the chord stays un-normalised).
 *   d_first_out / d_second_out                  [B][W][2] fp64, optional: the first_derivatives / second_derivatives
 *       attributes the reference leaves behind (estimates or the caller's arrays, with the setters' writes to
 *       first_derivatives[0] / [-1], QHS:557, 582).
 * Any of the six may be NULL. */
int vap_fit_ex(vap_ctx *ctx, vap_dtype dt, int B, int W, const void *d_waypoints,
               const double *d_tangent_in, const double *d_tangent_out, const double *d_first_derivatives,
               const double *d_second_derivatives, const double *d_starting_tangent,
               const double *d_ending_tangent, double *d_segments, double *d_segment_lengths,
               double *d_first_out, double *d_second_out, double *d_meta, uint32_t *d_flags);

/* SM:426-475 build_lookup_table.  Fills lut and meta[1] (= get_total_arc_length, SM:320-330). */
int vap_build_lut(vap_ctx *ctx, int B, int W, const double *d_segments, double *d_lut,
                  double *d_meta, uint32_t *d_flags);

/* Distance grid + per-sample properties: MPG:112-176 (the sampling loop of forward_backward_pass)
 * with SM:291-318 distance_to_time, SM:477-580 (the curvature/heading table entry the reference's
 * step lookup selects, evaluated on demand — the 1000*W table is never materialised) and
 * SM:204-215 get_point_at_parameter.
 *   dd > 0 : reference grid: s_0 = 0, s_k = fl(s_(k-1) + dd) while s_k < L (the reference's
 *            accumulated current_dist += dd, rounding included), plus the end sample; n_samples varies
 *   dd <= 0: fixed grid of exactly S samples, the same accumulation with dd_b = L_b / (S - 1.5)
 * The accumulated sum is reproduced in closed form (per binade the rounded increment is a constant
 * number of ulps), so sample k needs no scan over its predecessors: vap_grid_distances shows it.
 * Writes meta[2], meta[3]; d_dtheta [B][S] (dtype) receives |heading[k+1]-heading[k]| for the
 * velocity pass (scratch; may be NULL only if the velocity pass is not wanted). */
int vap_sample(vap_ctx *ctx, vap_dtype dt, int B, int W, int S, double dd, const double *d_segments,
               const double *d_lut, double *d_meta, void *d_x, void *d_y, void *d_heading,
               void *d_curvature, void *d_dtheta, uint32_t *d_flags);

/* MPG:188-316 forward + backward pass.  d_velocity receives the final velocities (MPG:316).
 * As in the reference, max_dec does not take part: boundary_map always contains sample 0 (MPG:110), so
 * forward_backward_pass replaces it with max_acc before its first step (MPG:194-196) and decelerates
 * with max_acc; max_dec is used by the time loop only (vap_time_profile, vap_route_motion_profile).
 * d_vcap: optional [B][S] (vap_limit_rows_dtype) per-sample initial velocities — the `velocities` list the reference
 * starts from (MPG:121,127,153,172: node / action-point max_velocity, 0.01 at stops); NULL = the
 * plain-node default max_vel with start/end velocities at the ends.  Entry 0 and the end sample are
 * taken from start_vel / end_vel.  Rows that fit the register-resident relaxation kernel (20 480
 * samples fp32, 10 240 fp64) run there, longer ones in the one-lane sequential sweep.
 * d_dtheta NULL = the rows the last sampling call (vap_profile_batch / vap_profile_routes; vap_sample for VAP_F32
 * with VAP_RECURRENCE_F64 only — in the other modes its rows are the caller's) of this shape and dtype
 * left on the context; for VAP_F32 with VAP_RECURRENCE_F64 these are fp64 curvature AND |dtheta| rows
 * (d_curvature is then not read and may be NULL) and the recurrence runs in fp64.  With an explicit d_dtheta
 * the recurrence runs in `dt` on the caller's rows. */
int vap_velocity_pass(vap_ctx *ctx, vap_dtype dt, int B, int S, const vap_constraints *c,
                      double start_vel, double end_vel, const double *d_meta,
                      const void *d_curvature, const void *d_dtheta, const void *d_vcap,
                      void *d_velocity, uint32_t *d_flags);

/* Per-sample limits of forward_backward_pass (MPG:100-176, 194-196, 256-257) for B routes whose nodes and
 * action points carry max_velocity, max_acceleration and stop, on the distance grid of the last
 * vap_sample / vap_profile_batch call on this context (same B, W, S):
 *   d_vcap          the `velocities` list the pass starts from (running max_velocity, 0.01 at stops,
 *                   end_vel at the end sample)
 *   d_acc_forward   max_acc (= max_dec) in force for the forward step from each sample  (boundary_map /
 *   d_acc_backward  max_acc the backward sweep has in force for its step from each sample  max_accels,
 *   d_dec_backward  [B] max_dec of the backward sweep: what the forward sweep left behind   incl. their quirks)
 * A node (parameter = its index) or action point (parameter t) takes effect at the first loop sample whose
 * parameter has reached it (MPG:125, 141-145) — a node before an action point on the same sample, and an
 * action point that would fall on its predecessor's sample never does, nor do those after it (the
 * reference looks at one pending action point per sample).  The list is taken in the order given, never sorted:
 * one whose parameter lies behind its predecessor's sample is such a case.  An action point at t <= 0 never takes
 * effect (the previous parameter starts at 0 and must be below t, MPG:144) and blocks the rest of the list, as does
 * one at t >= W - 1 (every loop parameter is below it) or NaN; +inf is the padding.  Nodes are counted, not looked up:
 * the j-th loop step whose parameter wraps ((prev_t % 1) > (t % 1), MPG:124) carries node j's attributes, so where one
 * step of the grid passes two nodes (a segment shorter than dd) the later nodes take effect one node late and the
 * last of them never.  stop, max_velocity and max_acceleration of the LAST node are never read; of node 0 only
 * max_velocity and max_acceleration are (MPG:100-107), its stop is not.
 *   d_node_max_velocity / d_node_max_acceleration [B][W]  (<= 0: none; NULL array: none)  MPG:100-107, 129-137
 *   d_node_stop                                   [B][W]  int32 (NULL: none)              MPG:126-127
 *   d_action_t                                    [B][M]  in the list's order (see above); pad with +inf
 *   d_action_max_velocity / _max_acceleration / _stop [B][M]  (NULL arrays: none)         MPG:146-160
 *   d_vcap, d_acc_forward, d_acc_backward [B][S], d_dec_backward [B] out, of type vap_limit_rows_dtype(ctx, dt):
 *                                    the three acceleration outputs are optional as a set (routes that do not
 *                                    change max_acceleration need only d_vcap)
 *   d_node_sample [B][W], d_action_sample [B][M]  int32 out, optional: the sample at which each takes
 *                                    effect (node 0: 0; INT_MAX: never)
 * d_lut NULL = the table of the last vap_profile_batch / vap_profile_routes (same B, W; after vap_profile_routes
 * d_lut must be NULL).  Reverse / turn nodes are not covered here
 * (vap_route_* is the general single-route path); waits act in the time domain (vap_time_insert_waits).
 * The output rows need no alignment beyond that of their element type: a row address that is not 16-byte aligned is
 * written element by element. */
/* Type of the limit rows (d_vcap, d_acc_forward, d_acc_backward, d_dec_backward) for rows of type dt in this context:
 * the type of the recurrence they enter — VAP_F64 for fp64 rows and for fp32 rows in the default mode
 * (VAP_RECURRENCE_F64: the fp64 recurrence amplifies an fp32-rounded limit such as 13.9 ft/s^2 past 1e-5, MPG:194-196,
 * 256-257 / DESIGN.md section 3), VAP_F32 for fp32 rows with VAP_RECURRENCE_F32. */
int vap_limit_rows_dtype(vap_ctx *ctx, vap_dtype dt);

int vap_route_limits(vap_ctx *ctx, vap_dtype dt, int B, int W, int M, int S, const double *d_lut,
                     const double *d_meta, const double *d_node_max_velocity,
                     const double *d_node_max_acceleration, const int *d_node_stop, const double *d_action_t,
                     const double *d_action_max_velocity, const double *d_action_max_acceleration,
                     const int *d_action_stop, const vap_constraints *c, double end_vel, void *d_vcap,
                     void *d_acc_forward, void *d_acc_backward, void *d_dec_backward, int *d_node_sample,
                     int *d_action_sample);

/* vap_velocity_pass with the limit rows of vap_route_limits (the three acceleration arguments NULL, or
 * all set together with d_vcap).  With acceleration rows the register-resident kernel covers rows up to
 * 10 240 samples (fp32) / 4096 (fp64); longer rows take the sequential sweep. */
int vap_velocity_pass_limits(vap_ctx *ctx, vap_dtype dt, int B, int S, const vap_constraints *c,
                             double start_vel, double end_vel, const double *d_meta,
                             const void *d_curvature, const void *d_dtheta, const void *d_vcap,
                             const void *d_acc_forward, const void *d_acc_backward,
                             const void *d_dec_backward, void *d_velocity, uint32_t *d_flags);

/* How far a path's velocity recurrence amplifies a relative change of its inputs: MPG:188-311 is swept on the rows as they
 * are and on K copies whose curvature and heading differences are changed by a relative +-delta, and the largest relative
 * change of a squared velocity, divided by 2 delta, is the path's conditioning number.  cond x (relative noise of the rows)
 * predicts how far two correct implementations of the recurrence — this library and the reference, say — may differ on the
 * path: ~1 to ~300 on ordinary paths, 1e6 to 1e8 on fixture big_w2048_p2.  Where cond is large the
 * reference's own profile oscillates from sample to sample.
 *   rows      curvature, |dtheta|, d_vcap, the three acceleration rows and d_meta are those of vap_velocity_pass_limits,
 *             resolved by the same code: d_dtheta NULL = the rows the last sampling call left on the context, and so on.
 *             N = meta[b][3] (taken as 0 below 0 and as S above S), dd = meta[b][2].  fp32 rows are widened: all
 *             arithmetic is fp64 whatever `dt` is.
 *   probes    k = 0 is the rows as they are.  For k = 1 .. K: curvature'[j] = curvature[j] * (1 + s delta) and
 *             dtheta'[j] = dtheta[j] * (1 + s' delta), one rounded product each (1 + s delta is exact), with (s, s') from one
 *             Philox4x32-10 block x (vap_search_sample's generator) of counter (j, k, 0x434f4e44, first_path + b) and key
 *             (seed & 0xffffffff, seed >> 32): s = +1 if x[0] & 1 else -1, s' likewise from x[1].  d_vcap and the
 *             acceleration rows are not perturbed.
 *   sweeps    each probe is MPG:188-311 in u = v^2, statement by statement — the sweep of VAP_VELOCITY_SEQ_LITERAL, compiled
 *             from the same text — and gives U_k[j], the squared velocity of sample j after the backward sweep
 *             (U_k[N - 1] = end_vel^2).
 *   deviation r_k[j] = |U_k[j] - U_0[j]| / U_0[j] where U_0[j] > 0; where U_0[j] == 0: 0 if U_k[j] == 0, else +inf; NaN for
 *             any other U_0[j].  sens[j] = (max over k of r_k[j]) / (2 delta) for j < N and 0 for j >= N; cond[b] = max over
 *             j of sens[j].  Every maximum starts from 0.0 and is taken under a strict >, so a NaN never wins.  Among equal
 *             values the smallest j, then the smallest k, gives worst_sample / worst_probe; both are -1 when cond is 0.
 *             N < 2 gives cond 0.
 *   flag      d_flags[b] |= VAP_FLAG_ILLCONDITIONED iff cond[b] > cond_limit (+inf: never).  d_flags [B] is this call's own
 *             array (optional, OR-ed into): no call of the pipeline writes the bit, and a caller who wants it among a
 *             profile result's flags — where vap_search_update would read it as an infeasible candidate — puts it there.
 *   outputs   d_cond [B] fp64; d_worst_sample, d_worst_probe [B] int32, optional; d_sensitivity [B][S] fp64, optional;
 *             d_velocity [B][S] fp64, optional: the velocity of U_0[j] (the row vap_velocity_pass gives under
 *             VAP_VELOCITY_SEQ_LITERAL on fp64 rows, bit for bit), 0 for j >= N.
 * VAP_ERR_INVALID: K not in {1, 3, 7, 15}; delta not a power of two in [2^-48, 2^-20]; cond_limit NaN or <= 0; B < 0; with
 * B > 0 the argument errors of vap_velocity_pass_limits and a null d_cond.  These are checked before the context is touched;
 * B = 0 is a no-op.  The probes' forward rows, B (K + 1) S 8 bytes, live in context scratch: the batch is cut into
 * launches that stay under VAP_OPT_CONDITIONING_SCRATCH_MB.  Works on the context's stream and does not synchronise; no
 * atomics: two calls give the same bits, and path b's outputs depend on (seed, first_path + b, its rows) only — not on B
 * or on the cut. */
#define VAP_FLAG_ILLCONDITIONED 1024u
int vap_velocity_conditioning(vap_ctx *ctx, vap_dtype dt, int B, int S, const vap_constraints *c, double start_vel,
                              double end_vel, const double *d_meta, const void *d_curvature, const void *d_dtheta,
                              const void *d_vcap, const void *d_acc_forward, const void *d_acc_backward,
                              const void *d_dec_backward, int K, double delta, uint64_t seed, uint32_t first_path,
                              double cond_limit, double *d_cond, int *d_worst_sample, int *d_worst_probe, uint32_t *d_flags,
                              double *d_sensitivity, double *d_velocity);

/* MPG:413-628, the time-domain resample that generate_motion_profile runs after
 * forward_backward_pass, for B plain-node paths (no turn / wait / reverse nodes and no action points:
 * those insert rows — use vap_route_motion_profile).  One row per time step of `time_step` seconds
 * (0.01 in the reference, MPG:389):
 *   rows      [B][capacity_rows][8] fp64  {time, position, linear velocity, acceleration, heading,
 *                                          angular velocity, x, y}   (MPG:558-592)
 *   counts    [B][2] int                  {rows written, entries of nodes_map}
 *   nodes_map [B][W] int                  row index at which each node is passed (MPG:420, 527-529;
 *                                          quirk Q5: the last node is never recorded)
 * d_velocity is the [B][S] result of vap_velocity_pass / vap_profile_batch in `dt`; d_meta as above.
 * d_segments / d_lut may both be NULL: the tables this context built in its last vap_profile_batch
 * call (same B and W) are used; those of a vap_profile_routes call, max_splines = 1 included, are refused
 * (VAP_ERR_UNSUPPORTED: vap_time_profile_routes).  A path needing more than capacity_rows rows is cut there and
 * flagged VAP_FLAG_TRUNCATED. */
int vap_time_profile(vap_ctx *ctx, vap_dtype dt, int B, int W, int S, const double *d_segments,
                     const double *d_lut, const double *d_meta, const void *d_velocity,
                     const vap_constraints *c, double time_step, int capacity_rows, double *d_rows,
                     int *d_counts, int *d_nodes_map, uint32_t *d_flags);

/* Waits and action points in the time domain (MPG:457-476, 509-518, 543-553) on top of the rows of
 * vap_time_profile: a node or action point with wait_time inserts int(wait_time/time_step) rows (zero
 * position / velocity / acceleration / angular velocity, the last heading and point) where it is passed,
 * and every later row moves by as many rows and time steps; actions_map records the row count at which
 * each action point fires (the reference's own test, MPG:546-553: one that lands exactly on a row's
 * parameter, or shares a row interval with its predecessor, never fires and blocks the ones after it; so
 * does one at t <= 0, at t >= W - 1, NaN, or behind its predecessor in an unsorted list — the list is taken in
 * the order given, and what fires here is decided by the rows alone, not by the distance grid of
 * vap_route_limits).  The wait of node 0 comes before row 0 with node 0's own heading (MPG:459-476); the wait of
 * the last node is never inserted (the loop ends before it is passed).
 *   d_rows_in [B][capacity_in][8], d_counts_in [B][2], d_nodes_map_in [B][W]   from vap_time_profile
 *   d_node_wait   [B][W]  seconds (NULL: none)       d_action_t / d_action_wait [B][M] (pad t with +inf)
 *   d_rows_out    [B][capacity_out][8]  (must not alias d_rows_in)
 *   d_counts_out  [B][3] int32: rows, nodes_map entries, actions_map entries
 *   d_nodes_map_out [B][W], d_actions_map_out [B][M] int32
 * Segments / table NULL = those of the last vap_profile_batch.  Turn and reverse nodes are not covered
 * (vap_route_motion_profile).
 * A route that needs more than capacity_out rows is cut there and flagged VAP_FLAG_TRUNCATED (here and in
 * vap_time_insert_events): rows [0, capacity_out) are exactly those of a call with enough capacity, d_counts_out[b][0] =
 * capacity_out, and nothing is written at or behind row capacity_out.  d_nodes_map_out, d_actions_map_out and their
 * counts are NOT cut: they hold what a call with enough capacity gives, so an entry of a truncated route may name a
 * row >= capacity_out that does not exist; compare entries with d_counts_out[b][0] before indexing rows with them.
 * Limits (here and in vap_time_insert_events):
 *   d_rows_in and d_rows_out must be 16-byte aligned — the rows move 16 bytes at a time; any other pointer is refused
 *   with VAP_ERR_INVALID before anything is launched.
 *   The kernel keeps its event list and the node arrays in LDS: 44 W + 12 M + 16 bytes of dynamic LDS and one static
 *   word, 44 W + 12 M + 20 bytes in all.  Up to 64 KB that runs on every device (W = 1488 with M = 1); above, the sum
 *   has to fit what the device gives one workgroup (hipDeviceAttributeMaxSharedMemoryPerBlock: 160 KB on an MI355X, which
 *   covers W = 2048 with up to M = 6142 action points and every route vap_profile_routes accepts) and is put to the
 *   runtime first.  A request that does not fit or is not granted returns VAP_ERR_UNSUPPORTED — the message names W, M,
 *   the bytes needed and the bytes available — before anything is launched or written. */
int vap_time_insert_waits(vap_ctx *ctx, int B, int W, int M, int capacity_in, int capacity_out, double time_step,
                          const double *d_segments, const double *d_lut, const double *d_meta,
                          const double *d_rows_in, const int *d_counts_in, const int *d_nodes_map_in,
                          const double *d_node_wait, const double *d_action_t, const double *d_action_wait,
                          double *d_rows_out, int *d_counts_out, int *d_nodes_map_out, int *d_actions_map_out,
                          uint32_t *d_flags);

/* vap_time_profile on the tables this context holds from its last vap_profile_batch / vap_profile_routes call, with
 * the reversed state of routes (MPG:431-433, 540-541): d_node_reverse [B][W] int32 (NULL: none); rows made while an
 * odd number of reverse nodes (node 0's flag included) has been passed carry heading - pi (before the wrap and the
 * sign, MPG:555-563) and negated velocity and acceleration (MPG:587-589).  Rows as vap_time_profile. */
int vap_time_profile_routes(vap_ctx *ctx, vap_dtype dt, int B, int W, int S, const double *d_meta,
                            const void *d_velocity, const vap_constraints *c, double time_step, int capacity_rows,
                            const int *d_node_reverse, double *d_rows, int *d_counts, int *d_nodes_map,
                            uint32_t *d_flags);

/* vap_time_insert_waits plus in-place turns (MPG:487-507 handle_turn over MPG:319-346 motion_profile_angle and
 * one_dim_mp_generator.py:4-69): a node with turn != 0 inserts, where it is passed and before its wait, the rows of a
 * trapezoidal heading profile of max_vel / max_acc on an arc of |turn| * track_width / 2 (zero velocity, the last
 * position and point, headings continuing from the last row, wrapped).  On the context's own tables (plain batch or
 * routes).  d_node_turn [B][W] degrees, d_node_reverse [B][W] (only node 0's wait heading reads it, MPG:463-464);
 * either may be NULL.  A turn at node 0 raises in the reference (quirk Q4): VAP_FLAG_BAD_ROUTE. */
int vap_time_insert_events(vap_ctx *ctx, int B, int W, int M, int capacity_in, int capacity_out, double time_step,
                           const vap_constraints *c, const double *d_meta, const double *d_rows_in,
                           const int *d_counts_in, const int *d_nodes_map_in, const double *d_node_wait,
                           const double *d_node_turn, const int *d_node_reverse, const double *d_action_t,
                           const double *d_action_wait, double *d_rows_out, int *d_counts_out, int *d_nodes_map_out,
                           int *d_actions_map_out, uint32_t *d_flags);

/* ---- fused hot path ------------------------------------------------------------------------ */

/* rebuild_tables (SM:582-594) + forward_backward_pass (MPG:70-316) for B plain-node paths, inputs
 * and outputs resident in HBM.  Any output pointer may be NULL except d_velocity.
 * d_meta: optional [B][4] fp64 (see above); d_flags: optional [B]. */
int vap_profile_batch(vap_ctx *ctx, vap_dtype dt, int B, int W, int S, double dd,
                      const void *d_waypoints, const vap_constraints *c, double start_vel,
                      double end_vel, void *d_x, void *d_y, void *d_heading, void *d_curvature,
                      void *d_velocity, double *d_meta, uint32_t *d_flags);

/* The same for B routes whose reverse / turn nodes cut them into several splines (SM:42-172 build_path for a whole
 * batch): fit with split tangents (SM:84-158) and the tangent setters' quirk (QHS:543-590), one 1000-entry table per
 * spline concatenated with running offsets (SM:436-464), distance -> parameter over that table and parameter ->
 * (spline, local parameter) with a split node belonging to the earlier spline (SM:243-275), then the plain velocity
 * pass — forward_backward_pass treats reverse / turn nodes like any other node (MPG:112-176).
 *   max_splines            upper bound of the splines of any route of the batch (1 + its reverse / turn nodes among
 *                          nodes 1..W-2); table scratch is sized by it
 *   d_node_reverse [B][W]  int32 is_reverse_node, d_node_turn [B][W] degrees (NULL arrays: none)
 *   d_node_tangent [B][W][2] fp64 (NaN row = None) with d_node_magnitudes [B][W][2] {incoming, outgoing} (SM:65-77)
 *   d_spline_counts [B]    int32 out, optional: splines per route
 * A route with a reverse / turn attribute on its LAST node (IndexError in the reference, SM:97) or with more
 * splines than max_splines is flagged VAP_FLAG_BAD_ROUTE; its rows are undefined.  Afterwards the context holds the
 * batch's tables: vap_route_limits + vap_velocity_pass_limits apply node / action-point limits as for plain paths.
 * The time domain of such a batch: vap_time_profile_routes, vap_time_insert_events.
 * The per-sample output rows of a batch with max_splines > 1 need no alignment beyond that of their element type (a row
 * address that is not 16-byte aligned is written element by element). */
#define VAP_FLAG_BAD_ROUTE 8u
int vap_profile_routes(vap_ctx *ctx, vap_dtype dt, int B, int W, int S, double dd, int max_splines,
                       const void *d_waypoints, const int *d_node_reverse, const double *d_node_turn,
                       const double *d_node_tangent, const double *d_node_magnitudes, const vap_constraints *c,
                       double start_vel, double end_vel, void *d_x, void *d_y, void *d_heading, void *d_curvature,
                       void *d_velocity, double *d_meta, uint32_t *d_flags, int *d_spline_counts);

/* Same with host buffers (allocates device scratch in the context arena, copies in and out,
 * synchronises).  This is what a single-path GUI call uses. */
int vap_profile_batch_host(vap_ctx *ctx, vap_dtype dt, int B, int W, int S, double dd,
                           const void *h_waypoints, const vap_constraints *c, double start_vel,
                           double end_vel, void *h_x, void *h_y, void *h_heading,
                           void *h_curvature, void *h_velocity, double *h_meta,
                           uint32_t *h_flags);

/* ---- scalar / vector evaluators on a fitted path (host buffers) -----------------------------
 * SM:204-241 get_point / get_derivative / get_second_derivative _at_parameter for n parameters of
 * path 0 of a (1,G,6,2) segment block held on the host.  order = 0,1,2.  out [n][2] fp64. */
int vap_eval_host(vap_ctx *ctx, int W, const double *h_segments, double param_last, int order,
                  int n, const double *h_t, double *h_out);

/* QHS:288-322 _get_basis_functions (order 0), QHS:324-363 _get_basis_derivatives (1), QHS:365-416
 * _get_basis_second_derivatives (2), QHS:418-469 _get_basis_third_derivatives (3) at n local parameters
 * (0..1 inside a segment): out [n][6] fp64 = [H0..H5] of that order, the reference's association order. */
int vap_basis_host(vap_ctx *ctx, int order, int n, const double *h_t, double *h_out);

/* SM:291-318 distance_to_time for n distances; SM:332-346 get_heading / get_curvature (table step
 * lookup) for n parameters.  what: 0 = distance_to_time, 1 = curvature, 2 = heading. */
int vap_lookup_host(vap_ctx *ctx, int W, const double *h_segments, double param_last,
                    const double *h_lut, int what, int n, const double *h_in, double *h_out);

/* ---- one general route (reverse / turn nodes, per-node limits, action points), fp64 -------------
 * The completeness path behind the drop-in classes: everything generate_motion_profile needs for a
 * GUI route, on the device.  Host buffers in, host buffers out; sizes are GUI-sized. */

/* Node / action-point attributes the path code reads (gui/node.py:17-51, gui/action_point.py:16-41).
 * Any attribute array may be NULL (= the GUI defaults: False / 0 / None). */
typedef struct {
    int n_nodes;                    /* W */
    const double *waypoints;        /* [W][2] feet */
    const int *is_reverse;          /* [W] */
    const double *turn;             /* [W] degrees */
    const int *stop;                /* [W] */
    const double *wait_time;        /* [W] seconds */
    const double *max_velocity;     /* [W] 0 = unset */
    const double *max_acceleration; /* [W] 0 = unset */
    const double *tangent;          /* [W][2], NaN row = None */
    const double *magnitudes;       /* [W][2] incoming, outgoing */
    int n_actions;                  /* M */
    const double *ap_t;             /* [M] path parameter */
    const int *ap_stop;
    const double *ap_wait_time, *ap_max_velocity, *ap_max_acceleration;
} vap_route_desc;

typedef struct vap_route vap_route;

/* SM:42-172 build_path (splits at reverse / turn nodes, SM:84-158 split tangents), QHS:30-219 fit per
 * spline (quirk Q3 kept), SM:426-475 lookup table.  VAP_ERR_INVALID where the reference returns
 * False or raises (fewer than 2 nodes; reverse/turn attribute on the last node). */
int vap_route_create(vap_ctx *ctx, const vap_route_desc *desc, vap_route **out);
int vap_route_destroy(vap_route *route);
/* number of splines and lookup_table.total_length (SM:320-330) */
int vap_route_info(vap_route *route, int *n_splines, double *total_length);
/* build_lookup_table(min_samples = lut_samples) and precompute_path_properties(samples_per_node) with sizes other than
 * the defaults every caller in the reference uses (1000 / 1000; SM:426-427, 477): rebuilds the route's arc-length
 * table with lut_samples entries per spline (np.linspace, trapezoid increments, np.cumsum — same operations, same
 * order) and makes the step lookup of get_heading / get_curvature (SM:550-580) read a table of
 * samples_per_node * len(nodes) entries.  Every later call on the route (lookups, forward_backward, motion_profile)
 * uses the new tables.  VAP_ERR_INVALID for lut_samples < 2 (the reference indexes local_params[1], SM:444). */
int vap_route_set_table_sizes(vap_route *route, int lut_samples, int samples_per_node);
int vap_route_table_sizes(vap_route *route, int *lut_samples, int *samples_per_node);
/* Per-spline results for the host mirrors of the drop-in classes; any pointer may be NULL.
 * start/npts/param_last [n_splines]; segments [(W-1)][6][2]; segment_lengths [W-1];
 * lut_distances / lut_parameters [n_splines*1000] = PathLookupTable (SM:466-475). */
int vap_route_get_splines(vap_route *route, int *h_start, int *h_npts, double *h_param_last, double *h_segments,
                          double *h_segment_lengths, double *h_lut_distances, double *h_lut_parameters);
/* SM:204-241 at n global parameters; order 0/1/2; out [n][2]. */
int vap_route_eval(vap_route *route, int order, int n, const double *h_t, double *h_out);
/* what: 0 = SM:291-318 distance_to_time, 1 = SM:340-346 get_curvature, 2 = SM:332-338 get_heading. */
int vap_route_lookup(vap_route *route, int what, int n, const double *h_in, double *h_out);
/* Samples forward_backward_pass produces for spacing dd (MPG:112-122, 172-175). */
int vap_route_sample_count(vap_route *route, double dd, int *n_out);
/* Host only, no device needed: the distance grid of MPG:112-122 for a path of length total_length
 * from the closed form the kernels use (csrc/vap_device.h build_grid_runs / grid_s).  Writes
 * s_k for k < min(*n_out, capacity) into h_s (may be NULL) and the loop count — the number of k with
 * s_k < total_length, i.e. n_samples - 1 — into *n_out.  Bit-identical to the reference's running sum. */
int vap_grid_distances(double dd, double total_length, long capacity, double *h_s, long *n_out);
/* MPG:70-316 with node / action-point limits (MPG:100-163) and boundary_map (MPG:194-196, 256-257).
 * Outputs (capacity each, any may be NULL): parameter t, x, y, heading, curvature, velocity. */
int vap_route_forward_backward(vap_route *route, const vap_constraints *c, double dd, double start_vel,
                               double end_vel, int capacity, int *n_out, double *h_t, double *h_x, double *h_y,
                               double *h_heading, double *h_curvature, double *h_velocity);
/* MPG:389-628 incl. in-place turns (MPG:319-346, one_dim_mp_generator.py:4-69) and waits.
 * rows [capacity_rows][8] = {time, position, linear_vel, acceleration, heading, angular_vel, x, y};
 * nodes_map (capacity W+1) / actions_map (capacity M+1) receive row indices (MPG:420, 528, 550).
 * VAP_ERR_CAPACITY if more rows are needed; VAP_ERR_INVALID where the reference raises (turn at node 0). */
int vap_route_motion_profile(vap_route *route, const vap_constraints *c, double dt, double dd, long capacity_rows,
                             double *h_rows, long *n_rows, long *h_nodes_map, int *n_nodes_map,
                             long *h_actions_map, int *n_actions_map);

/* ---- closest point on a path (gui/path.py:658-727 PathWidget.find_closest_point_on_path) -------------
 * VAP_CLOSEST_GUI: the GUI's own search, reproduced exactly — a coarse pass over percent = i / (25 * len(nodes)),
 *   i = 0..25*len(nodes), then 501 steps over [max(0, cp - 0.02), min(1, cp + 0.02)] around the coarse winner's percent
 *   cp, each step percent_to_parameter (SM:277-289, quirk Q6) + get_point_at_parameter (SM:204-215) + hypot; min_dist
 *   carries over into the fine pass and '<' is strict, so the first index at the minimum wins.
 * VAP_CLOSEST_EXACT: the global minimiser of |P(t) - q| over t in [0, W-1], across every spline of a route (per segment
 *   the roots of (P - q) . P', isolated by Bernstein sign variations, against the segment endpoints); on an exact tie
 *   the smallest parameter wins.
 * Outputs per query (fp64, any pointer may be NULL): parameter t; point P(t) [2] (= vap_route_eval order 0 at t, bit
 * for bit); distance |q - P(t)|; arc_length s at t from the path's own lookup table (the inverse of distance_to_time's
 * lerp, SM:291-318); cross_track = +distance when q lies left of P'(t) (cross(P', q - P) > 0), -distance otherwise.
 * A path of zero length (the GUI's early return, gui/path.py:670-679) gets NaN outputs. */
#define VAP_CLOSEST_GUI 0
#define VAP_CLOSEST_EXACT 1
/* gui/path.py:658-727 for the context's last vap_profile_batch / vap_profile_routes batch (same B and W).
 *   d_queries   [B][Q][2] feet, or [Q][2] for every path with shared_queries != 0
 *   d_parameter, d_distance, d_arc_length, d_cross_track [B][Q]; d_point [B][Q][2]
 *   d_flags     [B], optional, in / out: the profile call's flags — a path flagged VAP_FLAG_BAD_ROUTE gets NaN outputs;
 *               a path of zero length gets NaN outputs and VAP_FLAG_DEGENERATE.
 * Q = 0 is a no-op. */
int vap_closest_points(vap_ctx *ctx, int B, int W, int Q, int mode, int shared_queries, const double *d_queries,
                       double *d_parameter, double *d_point, double *d_distance, double *d_arc_length,
                       double *d_cross_track, uint32_t *d_flags);
/* gui/path.py:658-727 on one route, host buffers: one copy each way and one launch.  h_queries [n][2] feet;
 * h_out [n][6] = t, x, y, distance, arc_length, cross_track (NaN rows for a route of zero length). */
int vap_route_closest(vap_route *route, int mode, int n, const double *h_queries, double *h_out);

/* ---- robot-footprint clearance of time-domain rows --------------------------------------------------------------
 * Is a batch of trajectories drivable: does the robot's body stay on the field and off the field elements at every row?
 * The reference only previews the footprint (gui/path.py:764-809 PathWidget.draw_rect: the robot rectangle rotated to the
 * path direction, robot.width / robot.length in inches from config.yaml, gui/settings_widget.py:101-107); it never
 * checks it.  Units: feet, in the rows' own frame (the GUI's field frame: origin at the field centre, y down the image).
 *
 *   rows      d_rows [B][capacity][8] fp64 = {time, position, velocity, acceleration, heading, angular_vel, x, y} as
 *             vap_time_profile[_routes] / vap_time_insert_events write them; only rows r < d_counts[b * counts_stride]
 *             exist (counts_stride = 2 for the time-profile counts, 3 for the event-insertion counts; a count outside
 *             [0, capacity] is clamped to it).  The kernel reads columns 4, 6 and 7 only.
 *   pose      position (x, y); body angle phi = -heading.  The reference writes heading = -wrap(atan2(dy, dx) - pi *
 *             reversed) (MPG:555-563), so phi is the direction the robot's front faces: the direction of travel on
 *             forward segments, its opposite on reversed ones, the turning heading on in-place turn rows.  A body-frame
 *             point v sits at (x, y) + R(phi) v, R(phi) = [[cos, -sin], [sin, cos]].
 *   footprint h_footprint [n_foot][2], body frame (+x = the robot's front), convex, counter-clockwise, 3..16 vertices.
 *   scene     shared by every route of the call:
 *             h_field  [4] = xmin, ymin, xmax, ymax (NULL = no walls);
 *             polygons h_poly_xy [h_poly_start[n_poly]][2], polygon i = vertices h_poly_start[i] .. h_poly_start[i+1]-1,
 *                      convex, counter-clockwise, 3..16 vertices each (h_poly_start[0] = 0);
 *             circles  h_circles [n_circle][3] = cx, cy, r (r > 0).
 *             Collinear or duplicate vertices, clockwise or non-convex polygons, a non-positive radius, an empty or
 *             non-finite box: VAP_ERR_INVALID.  More than 256 polygons, 4096 polygon vertices or 256 circles:
 *             VAP_ERR_UNSUPPORTED.  The scene is host memory; it is validated and uploaded once per call.
 *   clearance of a row against one element, signed (negative = contact):
 *             wall     min over footprint vertices p of min(p.x - xmin, xmax - p.x, p.y - ymin, ymax - p.y);
 *             polygon  separated: the Euclidean distance (min of the vertex-to-edge distances both ways); overlapping:
 *                      minus the smallest projection overlap over the edge normals of both polygons (the separating-axis
 *                      test); touching gives 0;
 *             circle   the signed distance from the centre to the footprint polygon (positive outside), minus r.
 *             Element ids: the wall -1, polygons 0..n_poly-1, circles n_poly..n_poly+n_circle-1.  A row's clearance is the
 *             minimum over every element; on an exact tie the smallest id wins.
 *   outputs   per route [B], any pointer may be NULL: d_min_clearance (minimum over the route's rows), d_min_row (the first
 *             row at that minimum), d_min_element (the element at that row), d_first_row (the first row with clearance <
 *             margin, or -1), d_n_below (rows with clearance < margin).  A route without rows gets NaN, -1, -1, -1, 0.
 *             d_row_clearance [B][capacity] (optional): each row's clearance, NaN from counts[b] on.
 *   NaN       a row with a NaN in its pose (heading, x or y) has a NaN clearance and takes part in nothing: no minimum, no
 *             first row, no count; a route without a finite clearance gets the outputs of a route without rows.  Infinite
 *             coordinates are undefined.
 * The check is discrete at the rows' dt: motion between two rows is not swept.  A caller who wants a guard band passes
 * margin > 0 (one 10 ms row moves at most max_vel * dt, 0.04 ft at 4 ft/s).  B = 0 is a no-op. */
int vap_footprint_clearance(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                            int n_foot, const double *h_footprint, const double *h_field, int n_poly, const int *h_poly_start,
                            const double *h_poly_xy, int n_circle, const double *h_circles, double margin,
                            double *d_row_clearance, double *d_min_clearance, int *d_min_row, int *d_min_element,
                            int *d_first_row, int *d_n_below);

/* ---- robot-to-robot clearance between two batches of time-domain rows ---------------------------------------------
 * Which of my candidates get along with my partner's routine?  vap_footprint_clearance treats the field as empty of other
 * robots; this call poses two footprints, one per side, at the same instants and takes the clearance between them.
 *
 *   sides     A: d_rows_a [Ba][cap_a][8], d_counts_a with stride_a, footprint h_foot_a [n_foot_a][2];
 *             O ("others"): d_rows_o [Bo][cap_o][8], d_counts_o with stride_o, footprint h_foot_o [n_foot_o][2].
 *             Rows, counts (clamped to [0, capacity]) and the pose are vap_footprint_clearance's: only columns 4, 6, 7 are
 *             read; position (x, y), body angle phi = -heading.  Both row sets must be on the same time step (the caller
 *             guarantees it): row r of both sides is the same instant.  The two sides may be the same buffers (all pairs
 *             inside one batch; the diagonal is then a robot against itself, for the caller to ignore).
 *   shift     shift_rows (any sign): side O starts that many rows later.  With n_a, n_o the row counts,
 *               pose_a(r) = row min(r, n_a - 1) of a,   pose_o(r) = row clamp(r - shift_rows, 0, n_o - 1) of o:
 *             a robot that has not started, or has finished, stays on the field at its first or last pose.  A pair is
 *             examined at rows r = 0 .. T - 1, T = max(n_a, n_o + shift_rows, 1).
 *   clearance of a pair at a row: the polygon clearance above between the two posed footprints — separated: the Euclidean
 *             distance; overlapping: minus the smallest projection overlap over the edge normals of both; touching: 0.
 *             Symmetric in the two sides.  It saturates at minus the narrower footprint's extent once one projection
 *             contains the other, so deep overlaps tie exactly over many rows.  A row where either pose has a NaN
 *             (heading, x or y) has a NaN clearance and takes part in nothing; a pair without a finite clearance gets
 *             the outputs of an invalid pair.  Infinite coordinates are undefined.
 *   pairing  VAP_CONFLICT_ALL_PAIRS: every (a, o), P = Bo.  VAP_CONFLICT_MATCHED: Ba == Bo, pairs (i, i) only, P = 1.
 *   outputs   per pair [Ba][P], any pointer may be NULL: d_pair_clearance (the minimum over the pair's rows), d_pair_row
 *             (the first row at that minimum), d_pair_first_row (the first row with clearance < margin, or -1).  A pair
 *             with n_a == 0 or n_o == 0 gets NaN, -1, -1 and takes part in nothing below.
 *             per A route [Ba], any pointer may be NULL: d_min_clearance (the minimum over its pairs), d_min_other (the
 *             smallest o at that minimum), d_min_row (that pair's row), d_n_conflicts (pairs whose minimum is below
 *             margin), d_first_row (the earliest pair first row >= 0, or -1).  A route without a valid pair gets NaN, -1,
 *             -1, 0, -1.
 * Footprints are host memory, validated as vap_footprint_clearance validates its footprint (VAP_ERR_INVALID).  MATCHED
 * with Ba != Bo, a null row or count pointer with B > 0, a negative capacity: VAP_ERR_INVALID.  A capacity, or a horizon
 * max(cap_a, cap_o + shift_rows) rounded up to 64 rows, above INT_MAX: VAP_ERR_UNSUPPORTED.  Ba = 0 or Bo = 0 is a no-op.
 * Works on the context's stream and does not synchronise.  Context scratch grows with (Ba + Bo) x horizon x 32 B and with
 * Ba x ceil(Bo / 16), never with Ba x Bo.  Outputs do not depend on scheduling: two calls on the same inputs give the same
 * bits.  VAP_OPT_FOOTPRINT_CULL governs culling here too (block and row bounding circles before the exact pair); outputs
 * are bit for bit the same either way.  Discrete at the rows' dt like the static check: pass margin > 0 for a guard band. */
enum { VAP_CONFLICT_ALL_PAIRS = 0, VAP_CONFLICT_MATCHED = 1 };
int vap_footprint_conflicts(vap_ctx *ctx, int pairing, int shift_rows, double margin,
                            int Ba, long cap_a, const double *d_rows_a, const int *d_counts_a, int stride_a, int n_foot_a,
                            const double *h_foot_a,
                            int Bo, long cap_o, const double *d_rows_o, const int *d_counts_o, int stride_o, int n_foot_o,
                            const double *h_foot_o,
                            double *d_pair_clearance, int *d_pair_row, int *d_pair_first_row,
                            double *d_min_clearance, int *d_min_other, int *d_min_row, int *d_n_conflicts, int *d_first_row);

/* ---- robot-to-robot clearance over a window of start shifts -------------------------------------------------------
 * How long must I wait at this site, or how late must my partner start, for the two of us not to meet?  The call above
 * answers for ONE shift_rows; this one returns, for every pair of routes, the clearance as a function of the start shift
 * over a whole window, in one pass over rows that are packed once, and the first shift at which a route clears every other
 * robot for a run of consecutive shifts.
 *
 *   sides, rows, counts, strides, footprints, pose (phi = -heading, columns 4, 6, 7), the polygon clearance, pairing
 *             (VAP_CONFLICT_ALL_PAIRS: P = Bo; VAP_CONFLICT_MATCHED: P = 1) and footprint validation are
 *             vap_footprint_conflicts' own.
 *   shifts    window entry k = 0 .. n_shifts - 1 of A route a stands for the shift
 *               s = shift_lo + base[a] + k * shift_step,   computed in 64 bits;
 *             d_shift_base is a device int32 [Ba], or NULL for 0; shift_step >= 1.  As above, s is how many rows later
 *             side O starts; a negative s means that A starts |s| rows after O.
 *   instants  a valid pair (n_a > 0 and n_o > 0) at shift s is examined at t = min(0, s) .. max(n_a, n_o + s) - 1.  At
 *             instant t, A's row is i = t and O's row is j = t - s.  An index outside its side's rows is treated by the
 *             four bits of hold:
 *               VAP_HOLD_A_FIRST (1)  i < 0 becomes 0          VAP_HOLD_A_LAST (2)  i >= n_a becomes n_a - 1
 *               VAP_HOLD_O_FIRST (4)  j < 0 becomes 0          VAP_HOLD_O_LAST (8)  j >= n_o becomes n_o - 1
 *             With a bit clear, an instant that needs it is not examined.  hold = 14 is exactly vap_footprint_conflicts'
 *             horizon and parking: the table entry is then that call's d_pair_clearance at shift_rows = s, the same number.
 *   table     d_table [Ba][P][n_shifts]: the smallest clearance over the examined instants.  A NaN clearance takes part
 *             in nothing; the entry is NaN when no finite clearance was examined, and for an invalid pair.
 *   blocked   shift k of a pair is blocked iff table < margin (NaN never blocks).
 *             d_pair_safe [Ba][P]: the number of unblocked k; 0 for an invalid pair.
 *             d_pair_first [Ba][P]: scan = +1: the smallest k such that k .. k + min_run - 1 all lie in the window and
 *             are unblocked; scan = -1: the largest k such that k - min_run + 1 .. k do; -1 when there is none, and for
 *             an invalid pair.  min_run >= 1.
 *   per route shift k of route a is blocked iff any valid pair of a is blocked at k.  d_route_table [Ba][n_shifts]: the
 *             minimum over its valid pairs' table entries (NaN ignored; NaN if there is none); d_route_first [Ba] and
 *             d_route_safe [Ba] follow the pair rules.  A route with n_a = 0 gets NaN, -1, 0.  A route with rows but no
 *             valid pair is blocked nowhere: first = 0 (scan +1) or n_shifts - 1 (scan -1) when min_run <= n_shifts, and
 *             safe = n_shifts.
 * Every output pointer may be NULL.  n_shifts < 1, shift_step < 1, min_run < 1, scan not +-1, hold outside 0..15, MATCHED
 * with Ba != Bo, null rows or counts with B > 0, a negative capacity, a bad footprint: VAP_ERR_INVALID.  n_shifts above
 * VAP_CONFLICT_SHIFTS_MAX, a capacity above INT_MAX: VAP_ERR_UNSUPPORTED.  Arguments are checked before the context is
 * touched.  Ba = 0 or Bo = 0 is a no-op.  Works on the context's stream and does not synchronise.  Context scratch grows
 * with (Ba cap_a + Bo cap_o) x 32 B (capacities rounded up to 64 rows) and with Ba (P + 1) n_shifts bits, never with pairs
 * x rows or pairs x blocks x shifts.  Two calls on the same inputs give the same bits.  VAP_OPT_FOOTPRINT_CULL governs culling
 * (block and row bounding circles before the exact pair); outputs are the same numbers either way.  Discrete at the rows'
 * dt like the call above.  The row at which a minimum falls is not returned: call vap_footprint_conflicts at that shift. */
enum { VAP_HOLD_A_FIRST = 1, VAP_HOLD_A_LAST = 2, VAP_HOLD_O_FIRST = 4, VAP_HOLD_O_LAST = 8 };
#define VAP_CONFLICT_SHIFTS_MAX 4096
int vap_conflict_shifts(vap_ctx *ctx, int pairing, int hold, double margin, int shift_lo, int shift_step, int n_shifts,
                        const int *d_shift_base, int min_run, int scan,
                        int Ba, long cap_a, const double *d_rows_a, const int *d_counts_a, int stride_a, int n_foot_a,
                        const double *h_foot_a,
                        int Bo, long cap_o, const double *d_rows_o, const int *d_counts_o, int stride_o, int n_foot_o,
                        const double *h_foot_o,
                        double *d_table, int *d_pair_first, int *d_pair_safe,
                        double *d_route_table, int *d_route_first, int *d_route_safe);

/* ---- closed-loop tracking rollouts of time-domain rows -----------------------------------------------------------
 * How far does the robot stray from a route when it DRIVES it?  The two clearance calls judge the nominal rows; the robot
 * feeds those rows (t, x, y, heading, v, omega: the columns trajectory_io.py writes into routes.h) to a path follower.
 * This call rolls a differential-drive robot with a RAMSETE follower along every route of a batch, K times per route under
 * K perturbation records, and returns the tracking error and, on request, the EXECUTED rows in the time-profile layout, so
 * that both clearance calls accept them unchanged.  fp64 throughout.
 *
 *   rows      d_rows [B][capacity][8], d_counts with counts_stride as vap_footprint_clearance (n = the count clamped to
 *             [0, capacity]); columns 2, 4, 5, 6 and 7 are read.
 *   reference at row r: (x_r, y_r) = columns 6, 7; phi_r = -column 4; v_r = column 2; omega_r = -column 5 (the body rate:
 *             MPG:576 writes angular_vel = -v * curvature beside the negated heading).  For the settle rows r >= n the
 *             reference is row n - 1's pose with v_r = omega_r = 0.
 *   follower  vap_follower: track_width T (ft), RAMSETE gains b and zeta, the wheel speed limit (ft/s), the tolerance the
 *             route summary counts against (ft), n_substeps integration steps per row, settle_rows extra rows at the end.
 *   perturb   d_perturb [B][K][8], or [K][8] for every route with shared_perturb != 0; a record is {dx, dy, dphi,
 *             gain_left, gain_right, track_scale, tau, reserved}: a start offset, a gain on each wheel's actual speed, a
 *             factor on the effective track width, and the time constant (s) of a first-order lag between commanded and
 *             actual wheel speed.  The undisturbed record is {0, 0, 0, 1, 1, 1, 0, 0}.
 *   state     x, y, phi (unwrapped) and the actual wheel speeds w_L, w_R.  Start: (x_0 + dx, y_0 + dy, phi_0 + dphi),
 *             w_L = v_0 - omega_0 T / 2, w_R = v_0 + omega_0 T / 2.
 *   step      r = 0 .. n + settle_rows - 1, in this order:
 *             1. errors: (e_x, e_y) = R(-phi) (p_r - p); e_phi = wrap(phi_r - phi), wrap(a) = ((a + pi) mod 2 pi) - pi
 *                with the floored mod (MPG:560-562); e_pos = hypot(e_x, e_y).
 *             2. statistics: the maximum e_pos and the first row that strictly exceeds the running maximum; the maxima
 *                of |e_y| and |e_phi|.
 *             3. executed row r (if requested): time = r * time_step; position = the distance travelled so far (the sum
 *                of |d| below); velocity v = (g_L w_L + g_R w_R) / 2, the actual body speed; acceleration = (v - v of
 *                the previous row) / time_step, 0 at row 0; heading = -wrap(phi); angular velocity = -omega, omega =
 *                (g_R w_R - g_L w_L) / (T track_scale); x; y.
 *             4. control (RAMSETE): k = 2 zeta sqrt(omega_r^2 + b v_r^2); v_c = v_r cos e_phi + k e_x;
 *                omega_c = omega_r + k e_phi + b v_r sinc(e_phi) e_y; c_L = v_c - omega_c T / 2, c_R = v_c + omega_c T / 2.
 *             5. saturation: m = max(|c_L|, |c_R|); if m > wheel_speed_max both are scaled by wheel_speed_max / m (the
 *                ratio c_L : c_R, hence the curvature, is kept) and the row counts as saturated.
 *             6. n_substeps substeps of h = time_step / n_substeps: w += (c - w) a for each wheel, a = 1 - exp(-h / tau)
 *                (a = 1 for tau = 0); v and omega as in 3; the exact arc: u = omega h / 2, d = v h sinc(u),
 *                p += d (cos(phi + u), sin(phi + u)), phi += omega h.  sinc(x) = 1 - x^2 / 6 for |x| < 1e-4, else sin x / x.
 *             After the last step: the final position error |p_(n-1) - p| and heading error |wrap(phi_(n-1) - phi)|.
 *   outputs   any pointer may be NULL.
 *             per rollout: d_stats [B][K][6] = {max e_pos, max |e_y|, max |e_phi|, final position error, final heading
 *             error, 0}; d_stat_rows [B][K][2] = {row of max e_pos, saturated rows}.
 *             per route [B]: d_worst (the largest max e_pos over k; the smallest k on a tie), d_worst_rollout and
 *             d_worst_row (that k and its row), d_mean (the mean of max e_pos, summed in ascending k), d_n_exceeding
 *             (rollouts whose max e_pos is above f->tolerance).
 *             executed rows: d_exec_rows [B * K][cap_exec][8], rollout (b, k) at b * K + k, rows 0 .. n + settle_rows - 1
 *             (the rest is left as it was); d_exec_counts [B * K][2] = {n + settle_rows, 0}, so counts_stride = 2 works in
 *             both clearance calls.  cap_exec < capacity + settle_rows: VAP_ERR_INVALID.
 *   edges     a route with n = 0: NaN / -1 / 0 in every output of its rollouts and of the route, executed count 0.  A
 *             rollout whose record has a non-finite entry, a gain <= 0, track_scale <= 0 or tau < 0 is invalid: NaN / -1,
 *             no executed rows (count 0), no part in the route's summary (a route without a valid rollout: NaN, NaN, -1,
 *             -1, 0).
 *   alignment d_rows, d_perturb, d_stats and d_exec_rows must be 16-byte aligned (they are read and written two doubles
 *             at a time); hipMalloc's and torch's allocations are.  A misaligned one: VAP_ERR_INVALID.
 * VAP_ERR_INVALID: a non-positive (or non-finite) track_width, b, zeta, wheel_speed_max or time_step; n_substeps outside
 * 1..16; settle_rows outside 0..10000; K outside 1..4096; a null rows, counts or perturbation pointer with B > 0.  The
 * arguments are checked before the context is touched.  B = 0 is a no-op.  Works on the context's stream and does not
 * synchronise.  Two calls on the same inputs give the same bits: every reduction has a fixed order, no float atomics. */
typedef struct {
    double track_width, b, zeta, wheel_speed_max, tolerance;
    int n_substeps, settle_rows;
} vap_follower;
int vap_tracking_rollouts(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                          double time_step, const vap_follower *f, int K, int shared_perturb, const double *d_perturb,
                          double *d_stats, int *d_stat_rows, double *d_worst, double *d_mean, int *d_worst_rollout,
                          int *d_worst_row, int *d_n_exceeding, long cap_exec, double *d_exec_rows, int *d_exec_counts);

/* ---- closed-loop rollouts under a pure-pursuit follower ------------------------------------------------------------
 * The same question as vap_tracking_rollouts for the follower most teams run.  Pure pursuit is indexed by where the robot
 * is on the path, not by the clock: it reads the polyline of the rows and their speeds and steers for a goal one lookahead
 * further along it.  Layout conventions, perturbation records, the plant (lag, exact arc), saturation, the executed rows
 * and the per-route summary are vap_tracking_rollouts'; what differs is stated here.  fp64 throughout.
 *
 *   path      of a route with n rows (the count clamped to [0, capacity]): points P_i = columns 6, 7 and speeds v_i =
 *             column 2, i = 0 .. n - 1.  Columns 1, 4 and 5 are not read, except row 0's columns 4 and 5 for the start
 *             state.  Segment i = 0 .. n - 2: s_i = P_(i+1) - P_i, len_i = sqrt(s_x^2 + s_y^2); cumulative chord length
 *             c_0 = 0, c_(i+1) = c_i + len_i summed strictly in index order.  Segments without length (wait rows, in-place
 *             turns) are legal and passed over.  u_end = s_i / len_i of the last segment with len_i > 0, (1, 0) if none.
 *             Every norm below is sqrt(dx^2 + dy^2).
 *   status    d_route_status [B], a bit mask over rows 0 .. n - 1, written before the rollouts: bit 0 a row with v_i < 0,
 *             bit 1 a non-finite x, y or v.  A route with a non-zero status is treated as a route with n = 0.
 *   NOT EXECUTED BY THIS FOLLOWER: reverse legs (status bit 0), and in-place turns and dwells (their rows have no
 *             length: the robot drives on, it neither stops to wait nor turns on the spot).
 *   follower  vap_pursuit: track_width T (ft), lookahead (ft), min_speed (ft/s: the commanded speed never falls below
 *             it before arrival), arrive_tolerance (ft), the wheel speed limit (ft/s), the tolerance the route summary
 *             counts against (ft), n_substeps, settle_rows.
 *   perturb   vap_tracking_rollouts' record {dx, dy, dphi, gain_left, gain_right, track_scale, tau, lookahead} and its
 *             validity rule; slot 7 is the ROLLOUT'S LOOKAHEAD L: 0 means f->lookahead, > 0 is L in feet, < 0 or
 *             non-finite makes the record invalid.  So K can span perturbations x lookaheads.
 *   state     the pose and wheels start as in vap_tracking_rollouts: (x_0 + dx, y_0 + dy, -heading_0 + dphi), wheels
 *             from v_0 and omega_0 = -column 5 of row 0.  Besides: ic = 0 (closest segment), il = 0 (lookahead segment),
 *             arrived = -1.
 *   step      r = 0 .. n + settle_rows - 1, in this order:
 *             1. closest point (n >= 2).  For a segment i: t_i = clamp(((p - P_i) . s_i) / (s_i . s_i), 0, 1), 0 if
 *                s_i . s_i == 0; q_i = P_i + t_i s_i; D_i = |p - q_i|^2.  While ic < n - 2 and D_(ic+1) <= D_ic: ic += 1.
 *                Then e_ct = sqrt(D_ic), v_t = v_ic + t (v_(ic+1) - v_ic), s_c = c_ic + t len_ic, at_end = (ic == n - 2
 *                and t == 1).  n = 1: e_ct = |p - P_0|, v_t = v_0, at_end.
 *             2. statistics: the maximum e_ct and the first step that strictly exceeds the running maximum.
 *             3. executed row r (if requested): vap_tracking_rollouts' step 3.
 *             4. arrival: if arrived < 0 and (at_end or |P_(n-1) - p| <= arrive_tolerance): arrived = r.  From that step
 *                on c_L = c_R = 0.
 *             5. while not arrived: s* = s_c + L; il = max(il, ic); while il < n - 2 and c_(il+1) < s*: il += 1.  If
 *                s* >= c_(n-1) the goal is G = P_(n-1) + (s* - c_(n-1)) u_end (the path prolonged along its last
 *                tangent); otherwise f = clamp((s* - c_il) / len_il, 0, 1), 0 if len_il == 0, and G = P_il + f s_il.
 *                l_y = -sin(phi) (G_x - x) + cos(phi) (G_y - y); a2 = |G - p|^2; kappa = 2 l_y / a2, 0 if a2 == 0;
 *                sp = max(v_t, min_speed); c_L = sp - sp kappa T / 2, c_R = sp + sp kappa T / 2.
 *             6. saturation and 7. substeps: vap_tracking_rollouts' steps 5 and 6.
 *             After the last step: the final position error |P_(n-1) - p|.
 *   outputs   any pointer may be NULL.
 *             per rollout: d_stats [B][K][6] = {max e_ct, final position error, arrival time = arrived * time_step (NaN
 *             if it never arrived), the rollout's lookahead, 0, 0}; d_stat_rows [B][K][4] = {step of max e_ct, saturated
 *             rows, arrived step (-1 if never), final ic}.
 *             per route [B]: d_worst, d_worst_rollout, d_worst_row, d_mean, d_n_exceeding as vap_tracking_rollouts over
 *             max e_ct; d_n_unfinished (valid rollouts with arrived < 0); d_route_status.
 *             executed rows: d_exec_rows, d_exec_counts and cap_exec exactly as vap_tracking_rollouts.
 *   edges     n = 0, a non-zero status and an invalid record: NaN in all six stats, -1 in all four stat rows, executed
 *             count 0, no part in the route's summary (a route without a valid rollout: NaN, NaN, -1, -1, 0, 0).
 *   alignment as vap_tracking_rollouts: d_rows, d_perturb, d_stats, d_exec_rows 16-byte aligned, else VAP_ERR_INVALID.
 * VAP_ERR_INVALID: a non-positive (or non-finite) track_width, lookahead, wheel_speed_max or time_step; a negative (or
 * non-finite) min_speed or arrive_tolerance; a NaN tolerance; n_substeps outside 1..16; settle_rows outside 0..10000; K
 * outside 1..4096; a null rows, counts or perturbation pointer with B > 0; cap_exec below capacity + settle_rows.  The
 * arguments are checked before the context is touched.  B = 0 is a no-op.  Works on the context's stream and does not
 * synchronise.  Two calls on the same inputs give the same bits: every reduction has a fixed order, no float atomics. */
typedef struct {
    double track_width, lookahead, min_speed, arrive_tolerance, wheel_speed_max, tolerance;
    int n_substeps, settle_rows;
} vap_pursuit;
int vap_pursuit_rollouts(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                         double time_step, const vap_pursuit *f, int K, int shared_perturb, const double *d_perturb,
                         double *d_stats, int *d_stat_rows, double *d_worst, double *d_mean, int *d_worst_rollout,
                         int *d_worst_row, int *d_n_exceeding, int *d_n_unfinished, int *d_route_status, long cap_exec,
                         double *d_exec_rows, int *d_exec_counts);

/* ---- scene clearance of the disturbed rollouts ---------------------------------------------------------------------
 * Does the robot still miss the post when it starts an inch off, one side runs 3 % weak and the drive lags?  The rollout
 * calls above can write every executed row (d_exec_rows) and vap_footprint_clearance can read them back: B x K x rows x
 * 64 bytes through memory for five numbers per rollout.  This call runs the K rollouts per route of either follower and
 * takes the scene clearance of every executed row while it is still on the chip.  No executed rows are written.
 *
 *   follower  follower_kind = VAP_FOLLOWER_RAMSETE with `follower` a const vap_follower *, or VAP_FOLLOWER_PURSUIT with a
 *             const vap_pursuit *.
 *   rollouts  d_rows, d_counts, counts_stride, time_step, K, shared_perturb, d_perturb and the follower outputs d_stats,
 *             d_stat_rows ([B][K][2] for RAMSETE, [B][K][4] for pure pursuit), d_worst, d_mean, d_worst_rollout, d_worst_row,
 *             d_n_exceeding, and for pure pursuit d_n_unfinished and d_route_status: exactly as vap_tracking_rollouts /
 *             vap_pursuit_rollouts take and write them for the same inputs, bit for bit.  d_n_unfinished and d_route_status
 *             must be NULL with VAP_FOLLOWER_RAMSETE (VAP_ERR_INVALID).
 *   scene     n_foot, h_footprint, h_field, n_poly, h_poly_start, h_poly_xy, n_circle, h_circles and margin exactly as
 *             vap_footprint_clearance takes them: the same validation, limits and errors, the same element ids.
 *   pose      of executed row r: what step 3 of vap_tracking_rollouts would store, heading = -wrap(phi), x, y.  The
 *             footprint is posed at the body angle -heading = wrap(phi), not at the unwrapped phi (the two differ in
 *             the last bits of sin and cos once |phi| > pi).
 *   outputs   any pointer may be NULL.
 *             per rollout: d_clearance [B][K]; d_clear_rows [B][K][4] = {the first row at the minimum, the element at it,
 *             the first row with clearance < margin or -1, the rows with clearance < margin}.  DEFINITION: the five
 *             numbers vap_footprint_clearance returns (d_min_clearance, d_min_row, d_min_element, d_first_row, d_n_below)
 *             for route b * K + k of that follower's d_exec_rows / d_exec_counts with the same scene, footprint and margin
 *             and counts_stride = 2 — over executed rows 0 .. n + settle_rows - 1, bit for bit.  The reduction over a
 *             rollout's rows is that call's: a strictly smaller clearance replaces (the first row stays on a tie), a NaN
 *             clearance never replaces.  A rollout without executed rows (n = 0, an invalid record, a non-zero pursuit
 *             status) gets NaN, -1, -1, -1, 0.
 *             per route [B], over the route's valid rollouts (those with a minimum row >= 0) in ascending k:
 *             d_worst_clearance (the smallest per-rollout clearance; the smallest k on a tie), d_worst_clear_rollout,
 *             d_worst_clear_row, d_worst_clear_element (that k, its row and its element), d_mean_clearance (one running
 *             sum divided by the count), d_n_colliding (valid rollouts with clearance < margin), d_n_clear_valid (the valid
 *             rollouts: n_colliding / n_clear_valid is the collision share).  A route without a valid rollout gets NaN,
 *             -1, -1, -1, NaN, 0, 0.
 *   alignment d_rows, d_perturb and d_stats 16-byte aligned as in the rollout calls, else VAP_ERR_INVALID.
 * The check is discrete at time_step, as vap_footprint_clearance is: motion between two rows is not swept.
 * VAP_OPT_FOOTPRINT_CULL governs culling; on and off give the same bits.  Every reduction has a fixed order and there are
 * no float atomics: two calls on the same inputs give the same bits.
 * VAP_ERR_INVALID: a follower_kind other than the two; a null follower; every follower, time_step, K (outside 1..4096),
 * shape, stride and null-pointer error of the follower's own call; a non-finite margin; a null, clockwise, non-convex or
 * degenerate footprint; every scene error of vap_footprint_clearance.  VAP_ERR_UNSUPPORTED: that call's scene limits (256
 * polygons, 4096 polygon vertices, 256 circles); capacity + settle_rows above INT_MAX; too many workgroups for one launch.
 * The host arguments are checked before the context is touched.  B = 0 is a no-op.  Works on the context's stream and does
 * not synchronise.  Context scratch: the packed scene, pure pursuit's status words, and for K > 256 the B x K partials of
 * the summaries; it never grows with rows x K. */
enum { VAP_FOLLOWER_RAMSETE = 0, VAP_FOLLOWER_PURSUIT = 1 };
int vap_rollout_clearance(vap_ctx *ctx, int follower_kind, const void *follower, int B, long capacity, const double *d_rows,
                          const int *d_counts, int counts_stride, double time_step, int K, int shared_perturb,
                          const double *d_perturb, int n_foot, const double *h_footprint, const double *h_field, int n_poly,
                          const int *h_poly_start, const double *h_poly_xy, int n_circle, const double *h_circles, double margin,
                          double *d_stats, int *d_stat_rows, double *d_worst, double *d_mean, int *d_worst_rollout,
                          int *d_worst_row, int *d_n_exceeding, int *d_n_unfinished, int *d_route_status, double *d_clearance,
                          int *d_clear_rows, double *d_worst_clearance, int *d_worst_clear_rollout, int *d_worst_clear_row,
                          int *d_worst_clear_element, double *d_mean_clearance, int *d_n_colliding, int *d_n_clear_valid);

/* ---- clearance of the disturbed rollouts to the partner's routines --------------------------------------------------
 * Does a disturbed run still miss my partner?  vap_rollout_clearance answers for the scene; this call answers for the other
 * robots.  The rollout calls can write every executed row and vap_footprint_conflicts can read them back, once per distinct
 * start shift; this call runs the K rollouts per route of either follower and takes, for every executed row while it is on
 * the chip, the clearance to every partner route at the same instant.  No executed rows are written, and side A is never
 * packed.
 *
 *   follower, rollouts   follower_kind, follower, B, capacity, d_rows, d_counts, counts_stride, time_step, K, shared_perturb,
 *             d_perturb and the follower outputs d_stats .. d_route_status: exactly as vap_rollout_clearance takes and
 *             writes them (the follower's plain call, bit for bit; d_n_unfinished and d_route_status NULL with
 *             VAP_FOLLOWER_RAMSETE; the same 16-byte alignment rule).
 *   sides     n_foot_a, h_foot_a: my robot's footprint.  Side O ("others"): Bo, cap_o, d_rows_o, d_counts_o, stride_o,
 *             n_foot_o, h_foot_o, and margin, as vap_footprint_conflicts names and validates them.  Bo is 1 ..
 *             VAP_ROLLOUT_CONFLICT_OTHERS_MAX: Bo = 0 is VAP_ERR_INVALID, above the limit VAP_ERR_UNSUPPORTED.
 *   shifts    shift_rows (host), d_route_shift [B] or NULL for 0, d_rollout_shift [K] (shared by all routes) or NULL for 0.
 *             For rollout (b, k) side O starts s = shift_rows + route_shift[b] + rollout_shift[k] rows late, summed in 64
 *             bits.  shift_rows must lie within +-2^24, else VAP_ERR_INVALID; each device entry is CLAMPED into +-2^24
 *             before the sum.
 *   DEFINITION  Let E be that follower's d_exec_rows / d_exec_counts (route b * K + k, counts_stride 2, capacity capacity +
 *             settle_rows).  For rollout (b, k) with its shift s, one call vap_footprint_conflicts(VAP_CONFLICT_ALL_PAIRS,
 *             shift_rows = s, margin, Ba = 1: that executed route, h_foot_a; side O as given) defines, bit for bit:
 *             per pair (optional): d_pair_clearance [B][K][Bo] = that call's d_pair_clearance[o]; d_pair_rows [B][K][Bo][2] =
 *             its d_pair_row[o], d_pair_first_row[o].
 *             per rollout: d_conflict [B][K] = its d_min_clearance; d_conflict_rows [B][K][4] = its d_min_other, d_min_row,
 *             d_n_conflicts, d_first_row (the other at the minimum, its row, the pairs below the margin, the earliest
 *             first row or -1).
 *             Everything vap_footprint_conflicts defines is inherited: pose columns 4, 6, 7 and body angle -heading
 *             (here: what step 3 of the rollout would store, heading = -wrap(phi)); the horizon T = max(n_a, n_o + s, 1)
 *             with n_a the rollout's executed count; parking at the first or last pose; a NaN pose takes part in nothing;
 *             an invalid pair (n_a = 0 or n_o = 0) gives NaN, -1, -1; a strictly smaller clearance replaces, the first row
 *             stays on a tie; the smallest o wins on a tie across pairs.  A rollout without executed rows (n = 0, an
 *             invalid record, a non-zero pursuit status) gets the outputs of a route without a valid pair: NaN, -1, -1,
 *             0, -1, and NaN, -1, -1 per pair.
 *             per route [B], over the route's valid rollouts (conflict row >= 0) in ascending k: d_worst_conflict (the
 *             smallest per-rollout value; the smallest k on a tie), d_worst_conflict_rollout, d_worst_conflict_other,
 *             d_worst_conflict_row (that k, its other and its row), d_mean_conflict (one running sum divided by the
 *             count), d_n_conflicting (valid rollouts below the margin), d_n_conflict_valid.  A route without a valid
 *             rollout gets NaN, -1, -1, -1, NaN, 0, 0.
 *             Every output pointer may be NULL.
 * The check is discrete at time_step.  VAP_OPT_FOOTPRINT_CULL governs culling (the row's bounding circles before the exact
 * pair); on and off give the same bits.  Every reduction has a fixed order and there are no float atomics: two calls on
 * the same inputs give the same bits.
 * VAP_ERR_INVALID: every error of the follower's own call; Bo < 1; shift_rows beyond +-2^24; a negative cap_o; stride_o <
 * 1; null rows or counts of side O with B > 0; a non-finite margin; a null, clockwise, non-convex or degenerate footprint.
 * VAP_ERR_UNSUPPORTED: Bo above the limit; capacity + settle_rows or cap_o so large that a row index n + 3 * 2^24 could
 * pass INT_MAX; too many workgroups for one launch; more LDS than the device gives a workgroup (4 KiB per partner route
 * beside the kernel's own; the message has the byte count).  The host arguments are checked before the context is touched.
 * B = 0 is a no-op.  Works on the context's stream and does not synchronise.  Context scratch: side O's packed rows (Bo x
 * cap_o x 32 B), pure pursuit's status words, and for K > 256 the B x K partials of the summaries; it never grows with
 * rows x K. */
#define VAP_ROLLOUT_CONFLICT_OTHERS_MAX 16
int vap_rollout_conflicts(vap_ctx *ctx, int follower_kind, const void *follower, int B, long capacity, const double *d_rows,
                          const int *d_counts, int counts_stride, double time_step, int K, int shared_perturb,
                          const double *d_perturb, int n_foot_a, const double *h_foot_a, int Bo, long cap_o, const double *d_rows_o,
                          const int *d_counts_o, int stride_o, int n_foot_o, const double *h_foot_o, double margin, int shift_rows,
                          const int *d_route_shift, const int *d_rollout_shift, double *d_stats, int *d_stat_rows, double *d_worst,
                          double *d_mean, int *d_worst_rollout, int *d_worst_row, int *d_n_exceeding, int *d_n_unfinished,
                          int *d_route_status, double *d_pair_clearance, int *d_pair_rows, double *d_conflict, int *d_conflict_rows,
                          double *d_worst_conflict, int *d_worst_conflict_rollout, int *d_worst_conflict_other,
                          int *d_worst_conflict_row, double *d_mean_conflict, int *d_n_conflicting, int *d_n_conflict_valid);

/* ---- cross-entropy route search over batches of candidate trajectories --------------------------------------------
 * The calls above judge candidate routes; these two make the candidates and act on the verdicts, so that a search
 *   sample -> vap_profile_batch -> vap_time_profile -> vap_footprint_clearance [-> conflicts, rollouts] -> update
 * runs on the device with no result read on the host.  R routes ("problems") are refined at a time, N candidates each;
 * candidate (r, n) is route r * N + n of the batch B = R * N the evaluation calls see.  Plain-node paths only.
 *
 * vap_search_sample writes d_waypoints [R * N][W][2] in dt (the input of vap_profile_batch) from d_mean and d_sigma
 * [R][W][2] fp64:
 *   candidate 0   the best route so far, d_best_waypoints [R][W][2] in dt, where d_best_cost[r] is finite (both pointers
 *                 non-NULL); otherwise the mean rounded to dt.
 *   candidate n   coordinate = mean + sigma * z in fp64 (a product, a sum), rounded once to dt; where sigma == 0 the
 *                 coordinate is the mean itself (pinned).  (z_x, z_y) of waypoint w come from one Philox4x32-10 block with
 *                 counter (n, w, iteration, first_problem + r) and key (seed & 0xffffffff, seed >> 32): u1 = (x0 + 0.5) *
 *                 2^-32, u2 = (x1 + 0.5) * 2^-32, rho = sqrt(-2 ln u1), z_x = rho cos(2 pi u2), z_y = rho sin(2 pi u2), with
 *                 2 pi = 6.283185307179586; x2 and x3 are unused.  A candidate depends on (seed, iteration, first_problem
 *                 + r, n, w) only, not on R, N or the launch.
 * VAP_ERR_INVALID: N outside 1..4096, W < 2, a null mean, sigma or output, a misaligned pointer (mean, sigma: 16 bytes;
 * waypoints: a pair of dt); VAP_ERR_UNSUPPORTED: W above 2048 or R * N above INT_MAX.
 *
 * vap_search_update scores the N candidates of each problem, ranks them, refits mean and sigma to the elites and keeps
 * the best route so far.  One workgroup per problem; every sum has a fixed order and there are no float atomics, so two
 * calls on the same inputs give the same bits.
 *   terms      per candidate [B], any pointer may be NULL: d_counts with counts_stride (the count c of vap_time_profile;
 *              duration = c * time_step), d_meta [B][4] (length = meta[b][1]), d_flags, d_clearance (the route's minimum of
 *              vap_footprint_clearance), d_conflict_clearance (of vap_footprint_conflicts), d_tracking_worst (d_worst of
 *              vap_tracking_rollouts).
 *   cost       violation = max(0, clearance_margin - clearance) + max(0, conflict_margin - conflict) + max(0, tracking_worst
 *              - tracking_tolerance) over the terms given, summed in this order from 0;
 *              cost = w_time * duration + w_length * length; if violation > 0: cost = cost + (infeasible_base +
 *              w_violation * violation).  cost = +inf if flags != 0, c <= 0, the length or one of the three terms is NaN
 *              (the violation is then NaN) or the sum is NaN.  So a feasible candidate beats every infeasible one, and
 *              among infeasible ones the smaller violation wins.
 *   rank       d_order [R][N]: the problem's candidate indices by (cost, index) ascending; d_cost, d_violation [B];
 *              d_n_feasible [R]: candidates with a finite cost and violation == 0.
 *   refit      (d_mean != NULL; d_sigma then too) the elites are the first min(E, finite-cost candidates) of the order.
 *              Per coordinate j with sigma > 0: m = (sum of the elites' values in rank order, as stored in dt and widened
 *              to fp64) / count; var = (sum of (value - m)^2 in rank order) / count; mean = (1 - alpha) * mean + alpha * m;
 *              sigma = min(max(sqrt((1 - alpha) * (sigma * sigma) + alpha * var), sigma_min), sigma_max).  A coordinate
 *              with sigma == 0 is pinned: its mean and sigma keep their bits.  Without a finite-cost candidate nothing
 *              changes.  With d_mean == NULL the call only scores and ranks.
 *   best       (d_best_cost != NULL, in/out [R], +inf before the first call) if the first candidate of the order has a
 *              finite cost strictly below d_best_cost[r]: d_best_cost[r] = it, d_best_waypoints [R][W][2] (dt) = its
 *              waypoints, d_best_terms [R][4] = {duration, length, violation, candidate index}.  d_history
 *              [R][history_stride] receives d_best_cost[r] after this step at column iteration.
 * VAP_ERR_INVALID: N, W as above; E outside 1..N, alpha outside [0, 1], sigma_min < 0 or above sigma_max (with d_mean); a
 * negative or non-finite weight, a non-finite margin or tolerance; counts without a positive time_step; best waypoints,
 * terms or history without d_best_cost; iteration >= history_stride.  R = 0 is a no-op.  Both calls work on the context's
 * stream and do not synchronise. */
typedef struct {
    double w_time, w_length, w_violation, infeasible_base, clearance_margin, conflict_margin, tracking_tolerance;
} vap_search_weights;
int vap_search_sample(vap_ctx *ctx, int dt, int R, int N, int W, const double *d_mean, const double *d_sigma,
                      const void *d_best_waypoints, const double *d_best_cost, uint64_t seed, uint32_t iteration,
                      uint32_t first_problem, void *d_waypoints);
int vap_search_update(vap_ctx *ctx, int dt, int R, int N, int W, const void *d_waypoints, const int *d_counts, int counts_stride,
                      double time_step, const double *d_meta, const uint32_t *d_flags, const double *d_clearance,
                      const double *d_conflict_clearance, const double *d_tracking_worst, const vap_search_weights *weights,
                      int E, double alpha, double sigma_min, double sigma_max, double *d_mean, double *d_sigma, double *d_cost,
                      double *d_violation, int *d_order, int *d_n_feasible, double *d_best_cost, void *d_best_waypoints,
                      double *d_best_terms, double *d_history, int history_stride, uint32_t iteration);

/* ---- seed routes through a scene, on a grid ----------------------------------------------------------------------------
 * vap_search_* refine a route that is already roughly right; these two calls find one.  The robot is a disc of radius
 * `radius` (feet); the scene is vap_footprint_clearance's (h_field, polygons, circles: the same validation, limits and
 * status codes), and a field box is required (h_field == NULL: VAP_ERR_INVALID).  Everything below is decided by integer
 * comparisons or by comparisons of single IEEE additions, so the outputs do not depend on scheduling: two calls give the
 * same bits, and a heap Dijkstra doing the same additions gives the same distance field bit for bit.  No FMA anywhere.
 *
 *   grid      nx = ceil((xmax - xmin) / cell), ny = ceil((ymax - ymin) / cell); cell (i, j), index j * nx + i, has its centre
 *             at (xmin + (i + 0.5) * cell, ymin + (j + 0.5) * cell); a point lies in cell i = clamp(floor((x - xmin) / cell),
 *             0, nx - 1), j likewise.  The last column or row may reach past the box when the quotient is no integer.
 *   clearance of a cell centre p, the minimum of
 *             wall     min(p.x - xmin, xmax - p.x, p.y - ymin, ymax - p.y);
 *             polygon  with edges a -> b, e = b - a, |e| = sqrt(e.x e.x + e.y e.y): s = ((p - a) x e) / |e|, the outward
 *                      signed distance to the edge's line.  If the largest s is > 0: the smallest point-to-segment
 *                      distance, sqrt of the smallest dx dx + dy dy with (dx, dy) = (p - a) - t e, t = ((p - a) . e) *
 *                      (1 / (e.x e.x + e.y e.y)) clamped to [0, 1]; else the largest s (<= 0, inside);
 *             circle   sqrt(dx dx + dy dy) - r;
 *             minus radius.  A cell is FREE iff clearance >= margin.
 *   distance  per problem, from the goal's cell, over the eight moves (di, dj) in this order: (1,0) (0,1) (-1,0) (0,-1)
 *             (1,1) (-1,1) (-1,-1) (1,-1); an axis move costs w = cell, a diagonal one w = cell * 1.4142135623730951.  A
 *             move between two free cells is allowed; a diagonal one also needs the two axis cells it passes between to
 *             be free (no corner is cut).  d[goal cell] = 0, d[v] = min over allowed moves v -> u of fl(d[u] + w): the
 *             unique fixed point.  Cells that are not free, or not reached, have +inf.
 *   snapping  if the start's or the goal's own cell is not free, the free cell nearest to the point is used: smallest
 *             dx dx + dy dy from the point to the cell centre, the lowest index on a tie (a robot parked against a wall is
 *             the usual start, and a disc of the circumscribed radius does not fit there).  VAP_PLAN_SNAPPED_START /
 *             VAP_PLAN_SNAPPED_GOAL say so.
 *   trace     from the (snapped) start cell, step to the allowed neighbour with the smallest fl(d[u] + w), the first in the
 *             move order on a tie (strict <), until d = 0.
 *   pull      over the traced cells c_0 .. c_(n-1): anchor a = 0; take the largest b > a with c_b visible from c_a, or
 *             a + 1 if none beyond it is; emit c_b; a = b.  c_b is visible from c_a = (i0, j0) when, with (dx, dy) the index
 *             difference, every cell (i, j) of the two cells' bounding box with 2 |(i - i0) dy - (j - j0) dx| <= |dx| + |dy|
 *             is free (the supercover of the segment between the centres; integers only).
 *   vertices  the start, the centres of the emitted cells but the last, the goal: c_0's centre is replaced by the exact
 *             start and the goal cell's by the exact goal; [start, goal] when both share a cell.  Visibility holds between
 *             centres, so the first and last segment may be off by up to half a cell (more after snapping): these are
 *             SEEDS for the search, not checked routes.
 *   waypoints l_m = sqrt(dx dx + dy dy) of segment m, c_0 = 0, c_(m+1) = c_m + l_m in order, L = the last c.  Waypoint k =
 *             1 .. W-2 lies at arc s = (k * L) / (W - 1) on the first segment m with c_(m+1) >= s and l_m > 0, at a + ((s -
 *             c_m) / l_m) * (b - a) (the goal if there is none: L = 0).  Waypoints 0 and W-1 are the start's and the goal's
 *             own bits.  fp64.
 *   failures  a non-finite start or goal (VAP_FLAG_DEGENERATE), no free cell at all (VAP_PLAN_NO_FREE), a start whose d is
 *             +inf (VAP_PLAN_UNREACHABLE): NaN waypoints and vertices, length +inf, n_vertices 0 (and, for the first two, a
 *             distance field of +inf; the unreachable start's field is the goal's own).  The relaxation stops
 *             after a sweep that changes nothing and after nx * ny sweeps at the latest, the trace after nx * ny cells; a
 *             shortest path has fewer edges, so valid input never gets there (VAP_FLAG_NOCONVERGE if it does).
 *
 * vap_plan_grid writes d_clearance [ny][nx] fp64 and d_free [ny][nx] bytes (1 = free); either may be NULL, and with both
 * NULL the call only checks its arguments and reports nx, ny (host ints, either may be NULL) without a context.
 * vap_plan_seeds plans R problems, d_starts / d_goals [R][2] fp64 on the device, one workgroup per problem at a time with
 * the distance field in LDS: d_waypoints [R][W][2]; optional (NULL to skip) d_length [R], d_flags [R], d_n_vertices [R]
 * (all vertices, also beyond max_vertices), d_vertices [R][max_vertices][2] (the first max_vertices, NaN behind the last;
 * more vertices than that set VAP_PLAN_VERTICES_TRUNCATED, only when this output is asked for; the waypoints always use
 * every vertex), d_distance [R][ny][nx].
 * VAP_ERR_INVALID: cell <= 0, radius < 0, a non-finite cell, radius or margin, no field box, a bad scene, W < 2, R < 0, a
 * null start, goal or waypoint pointer with R > 0, max_vertices < 2 with d_vertices.  VAP_ERR_UNSUPPORTED: nx * ny above
 * 16384, W above 2048, the scene's limits, a device whose LDS cannot hold the grid.  The arguments are checked before the
 * context is touched.  R = 0 is a no-op.  Both work on the context's stream and do not synchronise; the scene is host
 * memory, uploaded once per call. */
#define VAP_PLAN_SNAPPED_START 16u
#define VAP_PLAN_SNAPPED_GOAL 32u
#define VAP_PLAN_NO_FREE 64u
#define VAP_PLAN_UNREACHABLE 128u
#define VAP_PLAN_VERTICES_TRUNCATED 256u
int vap_plan_grid(vap_ctx *ctx, const double *h_field, int n_poly, const int *h_poly_start, const double *h_poly_xy, int n_circle,
                  const double *h_circles, double cell, double radius, double margin, double *d_clearance, uint8_t *d_free,
                  int *nx_out, int *ny_out);
int vap_plan_seeds(vap_ctx *ctx, int R, int W, const double *d_starts, const double *d_goals, const double *h_field, int n_poly,
                   const int *h_poly_start, const double *h_poly_xy, int n_circle, const double *h_circles, double cell,
                   double radius, double margin, int max_vertices, double *d_waypoints, double *d_length, uint32_t *d_flags,
                   int *d_n_vertices, double *d_vertices, double *d_distance);

/* ---- routes rasterised onto the planner's grid; seeds round a partner's routine -------------------------------------------
 * vap_plan_seeds plans through the static scene and does not know that another robot drives there.  vap_plan_occupancy
 * turns a batch of time-domain rows (a partner's routine, or my own candidates) into per-cell occupancy on vap_plan_grid's
 * grid: which cell centres a disc of `radius` cannot stand on while the routes' footprints pass, and when.
 * vap_plan_seeds_occupied plans with that occupancy blocked, per problem and within a time window.  The reference poses a
 * footprint in one place only (gui/path.py:764-809 PathWidget.draw_rect) and never rasterises it.
 *
 *   rows      d_rows [B][capacity][8], d_counts, counts_stride: vap_footprint_clearance's (a count outside [0, capacity] is
 *             clamped to it; columns 4, 6 and 7 are read).  n_b = the clamped count of route b.
 *   footprint h_footprint [n_foot][2], body frame, convex, counter-clockwise, 3..16 vertices: vap_footprint_clearance's
 *             validation.
 *   grid      vap_plan_grid's, from h_field (required) and cell: nx, ny, the cell centres, nx * ny <= 16384.
 *   pose      row r of a route: vertex v of the footprint at (x, y) + R(phi) v, phi = -heading, R(phi) = [[cos, -sin],
 *             [sin, cos]], computed as x + (cos * v.x - sin * v.y), y + (sin * v.x + cos * v.y) in fp64, once per row.
 *   clearance of cell centre p against that row: vap_plan_grid's polygon formula applied to the posed vertices (edges
 *             a -> b between consecutive posed vertices, e = b - a, |e| = sqrt(e.x e.x + e.y e.y), s = ((p - a) x e) / |e|;
 *             largest s > 0: sqrt of the smallest point-to-segment dx dx + dy dy, t = ((p - a) . e) * (1 / (e.x e.x +
 *             e.y e.y)) clamped to [0, 1]; else the largest s), minus radius.  The row COVERS the cell iff clearance <
 *             margin: a cell is covered exactly when vap_plan_grid with the posed footprint as a scene polygon would not
 *             call it free on the polygon's account.  A row with a non-finite pose covers nothing and takes no part in
 *             the minimum; nor does a row with a COLLAPSED pose: one so large (|x| or |y| beyond about 2^53 times the
 *             footprint's size) that some posed edge has e.x e.x + e.y e.y equal to zero, or not finite.  No FMA.
 *   instants  row r stands at instant r + shift_rows (any sign).
 *   outputs   per cell [ny][nx], over all B routes, any pointer may be NULL:
 *             d_first  int32, the smallest covering instant; INT_MAX if never covered;
 *             d_last   int32, the largest covering instant; INT_MIN if never covered;
 *             d_count  int32, the number of covering (route, row) pairs;
 *             d_min_clearance  fp64, the minimum of the clearance over every existing row of every route (covering or
 *                      not); +inf without rows.
 *   holds     hold_last != 0: a cell covered by row n_b - 1 of a route gets last = INT_MAX (the robot stays where its
 *             routine ends, vap_footprint_conflicts' convention).  hold_first != 0: a cell covered by row 0 gets first =
 *             INT_MIN (it stands there before it starts).  Holds do not change d_count.
 *   B = 0, capacity = 0 or counts of 0 write the never-covered values.  With every output NULL the call only checks its
 *   arguments and reports nx, ny (host ints, either may be NULL) without a context.
 * VAP_ERR_INVALID: B < 0, capacity < 0, counts_stride < 1, a null row or count pointer with B > 0, a bad footprint, no field
 * box, an empty or non-finite box, cell <= 0, radius < 0, a non-finite cell, radius or margin.  VAP_ERR_UNSUPPORTED: nx * ny
 * above 16384; a capacity of INT_MAX rows or more; a shift_rows with which an instant could reach INT_MIN or INT_MAX (the
 * hold values).  The arguments are checked before the context is touched.  Works on the context's stream and does not
 * synchronise.  The outputs do not depend on scheduling: integer min, max and add and a minimum over the doubles' ordered
 * bit patterns merge the routes, so two calls give the same bits, and B routes in one call give the elementwise min / max /
 * sum / min of B calls.  VAP_OPT_FOOTPRINT_CULL governs culling here too (a box per 64 rows, a circle per row); outputs are
 * bit for bit the same either way.  Discrete at the rows' dt: pass margin > 0 for a guard band.
 *
 * vap_plan_seeds_occupied is vap_plan_seeds with three more inputs: d_occ_first, d_occ_last [ny][nx] int32 (device; what
 * vap_plan_occupancy wrote for the same field and cell) and d_windows [R][2] int32 = (t0, t1) per problem (device; NULL:
 * every instant, (INT_MIN, INT_MAX)).  For problem r a cell is FREE iff it is free in the static scene and NOT
 * (t0 < t1 and first < t1 and last >= t0): the window [t0, t1) meets [first, last].  [first, last] is the hull of the visits:
 * a cell visited twice counts as blocked in between, which is conservative.  A window with t1 <= t0 is empty and blocks
 * nothing.  Everything after the free mask (no free cell, distance, snapping, trace, pull, vertices, waypoints, flags,
 * limits) is vap_plan_seeds' definition with this mask.  With both occupancy pointers NULL the call IS vap_plan_seeds, bit
 * for bit (d_windows is ignored); exactly one of them NULL is VAP_ERR_INVALID. */
int vap_plan_occupancy(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride, int n_foot,
                       const double *h_footprint, const double *h_field, double cell, double radius, double margin, int shift_rows,
                       int hold_first, int hold_last, int *d_first, int *d_last, int *d_count, double *d_min_clearance, int *nx_out,
                       int *ny_out);
int vap_plan_seeds_occupied(vap_ctx *ctx, int R, int W, const double *d_starts, const double *d_goals, const double *h_field,
                            int n_poly, const int *h_poly_start, const double *h_poly_xy, int n_circle, const double *h_circles,
                            double cell, double radius, double margin, int max_vertices, const int *d_occ_first,
                            const int *d_occ_last, const int *d_windows, double *d_waypoints, double *d_length, uint32_t *d_flags,
                            int *d_n_vertices, double *d_vertices, double *d_distance);

/* ---- a routine's travel matrix and its visiting order -----------------------------------------------------------------------
 * A routine is a start and a handful of sites, not one (start, goal) pair.  vap_plan_travel plans every ordered pair of P
 * points of a problem at the price of P distance fields; vap_plan_order finds the cheapest order to visit the sites in from
 * any cost matrix (the travel matrix, or what the caller made of it on the device: seconds, dwell times, forbidden legs).
 * The reference keeps a routine as a hand-ordered list of nodes (gui/path.py) and has neither.
 *
 * vap_plan_travel: d_points [R][P][2] fp64 on the device, 2 <= P <= 16; the scene, cell, radius and margin of vap_plan_seeds;
 * d_occ_first, d_occ_last, d_windows [R][2] of vap_plan_seeds_occupied (both occupancy pointers NULL: the static scene;
 * problem r's one window holds for all its pairs).  For a != b, entry (r, a, b) of every output IS what vap_plan_seeds (or,
 * with an occupancy, vap_plan_seeds_occupied) gives for start = point a, goal = point b of problem r, bit for bit: its
 * snapping, trace, pull, vertices, waypoints, flags and failures (vap_plan_seeds without its vertex output: max_vertices is
 * accepted and cuts nothing, VAP_PLAN_VERTICES_TRUNCATED is never set).  The diagonal (r, b, b) has travel 0, flags 0,
 * n_vertices 0 and every waypoint equal to point b's own bits, whatever they are.  The matrix is NOT symmetric: the trace
 * breaks ties by move order, so (a, b) and (b, a) may take different cells; nothing is mirrored.  The field of goal b is
 * relaxed once and serves every start, which is all that distinguishes this call from P (P - 1) problems of vap_plan_seeds.
 *   d_travel      [R][P][P] fp64, the pulled polyline's length (vap_plan_seeds' d_length), +inf on failure; required
 *   d_flags       [R][P][P] uint32, d_n_vertices [R][P][P] int32, d_waypoints [R][P][P][W][2] fp64: each may be NULL; W is
 *                 read only with d_waypoints
 * VAP_ERR_INVALID: vap_plan_seeds' scene, cell, radius and margin errors, exactly one occupancy pointer NULL, P < 2, R < 0, a
 * null point or travel pointer with R > 0, W < 2 with d_waypoints.  VAP_ERR_UNSUPPORTED: P > 16, nx * ny above 16384, W above
 * 2048 with d_waypoints, R * P above INT_MAX, a device whose LDS cannot hold the grid.  The arguments are checked before the
 * context is touched.  R = 0 is a no-op.  Works on the context's stream and does not synchronise; two calls give the same bits.
 *
 * vap_plan_order: d_cost [R][P][P] fp64 on the device, c[a][b] the cost of going from point a to point b; point 0 is where
 * the routine starts, points 1 .. M = P - 1 are the sites, 1 <= M <= 10; the diagonal and column 0 are not read.  An entry
 * that is NaN or -inf counts as +inf (a forbidden leg).
 *   end       -1: the routine may end at any site; 1 .. M: it ends at that site.
 *   before    d_before [R][P] uint32 or NULL: bit j - 1 of before[k] says site j must have been visited before site k.
 *             Entry 0 and bits >= M are ignored.
 *   f         over site sets S (bit j - 1 = site j): f[{j}][j] = c[0][j] if before[j] = 0, else +inf.  For j in S, |S| > 1:
 *             if before[j] is a subset of S \ {j}, f[S][j] = the minimum over i in S \ {j}, taken in increasing i under a
 *             strict <, of fl(f[S \ {j}][i] + c[i][j]), and the parent of (S, j) is the i that won; otherwise +inf.
 *   last      with F the full set: `end` if given, else the j with the smallest f[F][j], the lowest j on a tie.
 *   outputs   d_total [R] = f[F][last]; d_order [R][M] int32, the sites in visiting order, from `last` back along the
 *             parents; d_flags [R] uint32, optional.  A total of +inf (every leg forbidden, a precedence cycle, an `end`
 *             that something must follow) is infeasible: order all -1, total +inf, VAP_ORDER_INFEASIBLE.
 * fl(x + c) is monotone in x, so the total is the smallest left-to-right sum c[0][o1] + c[o1][o2] + ... over all admissible
 * permutations, bit for bit; only the choice among equal totals rests on the two tie rules.  One workgroup per problem at a
 * time with f in LDS (2^M * M * 8 bytes).  VAP_ERR_INVALID: P < 2, R < 0, end outside {-1, 1 .. M}, a null cost, order or
 * total pointer with R > 0.  VAP_ERR_UNSUPPORTED: P > 11.  The arguments are checked before the context is touched.  R = 0 is a
 * no-op.  Works on the context's stream and does not synchronise; no atomics: two calls give the same bits. */
#define VAP_ORDER_INFEASIBLE 512u
#define VAP_PLAN_TRAVEL_MAX_POINTS 16
#define VAP_PLAN_ORDER_MAX_SITES 10
int vap_plan_travel(vap_ctx *ctx, int R, int P, int W, const double *d_points, const double *h_field, int n_poly,
                    const int *h_poly_start, const double *h_poly_xy, int n_circle, const double *h_circles, double cell,
                    double radius, double margin, int max_vertices, const int *d_occ_first, const int *d_occ_last,
                    const int *d_windows, double *d_travel, uint32_t *d_flags, int *d_n_vertices, double *d_waypoints);
int vap_plan_order(vap_ctx *ctx, int R, int P, const double *d_cost, int end, const uint32_t *d_before, int *d_order, double *d_total,
                   uint32_t *d_flags);

/* ---- a routine's legs chained into one timeline ------------------------------------------------------------------------------
 * vap_plan_order gives a visiting order and the route search refines each leg by itself, every leg profiled from its own
 * time zero.  vap_routine_timeline puts the legs back together: for every used slot m of routine r the output holds, in this
 * order, [turn m] [leg m] [dwell m], all in the 8-column rows of vap_time_profile and on one time step, so the result goes
 * where the rows of vap_time_profile go (vap_footprint_clearance, vap_footprint_conflicts, vap_tracking_rollouts,
 * vap_plan_occupancy).  The reference chains nothing: a routine is one hand-made path there; the turn is its own
 * (MPG:319-346 motion_profile_angle over one_dim_mp_generator.py:4-69, inserted as MPG:487-507 handle_turn does).
 *   inputs    d_rows_in [L][capacity_in][8], d_counts_in [L * counts_stride] (entry l * counts_stride = rows of leg l; a count
 *             above capacity_in counts as capacity_in): L legs on the device.  d_leg [R][M] int32: the leg driven in slot m;
 *             a leg may serve several slots and routines.  d_n_legs [R] int32 or NULL (= M): slots used, clamped to 0 .. M.
 *             d_dwell [R][M] seconds at the end of slot m or NULL; d_start_heading [R] or NULL: the heading the robot stands
 *             at before slot 0 (NaN: none).  1 <= M <= 32.
 *   turn      from the heading h of the output row in front (slot 0: the start heading; none: no turn block) to the heading
 *             of leg m's first row: D = first - h; if D > pi, D -= 2 pi; if D <= -pi, D += 2 pi.  |D| < turn_min: no rows.
 *             Otherwise the rows of handle_turn for angle = -D radians with c->max_vel, max_acc, track_width: n =
 *             ceil((total_time + dt) / dt) rows; row j has heading h + wrapped(sum_{i<j} v(i dt) dt / (track_width / 2) * sign)
 *             (the running sum taken left to right) and angular velocity (difference of the UN-wrapped sums) / dt, 0 in
 *             row 0; linear velocity and acceleration 0; position, x, y of the row in front (slot 0: position 0 and the
 *             point of leg 0's first row).
 *   leg       the leg's rows, with time = in_time + (double)s * dt (s = the block's first output row, vap_time_insert_waits'
 *             convention) and position = in_position + off_m, off_0 = 0, off_{m+1} = off_m + (last position of leg m), summed
 *             left to right.  The other six columns are copied.
 *   dwell     int(dwell / dt) rows (NaN or <= 0: none; saturating at INT_MAX): velocity, acceleration, angular velocity 0;
 *             heading, x, y, position of the row in front.  Every inserted row (turn or dwell) at output row o has time
 *             (double)o * dt.
 *   outputs   d_rows_out [R][capacity_out][8] (must not alias d_rows_in); d_counts_out [R][2] = {rows, slots used}; d_map
 *             [R][M][3] = the first output row of slot m's turn, leg and dwell block (saturating at INT_MAX; -1 for an unused
 *             slot): site m is reached at map[r][m][2] * dt, and the routine takes rows * dt; d_seam [R][M][3] = {heading of
 *             leg m's first row minus the heading of the last turn row (of the row in front without a turn), wrapped as D; x
 *             and y of leg m's first row minus those of the row in front}: the rectangle-rule sum does not land on the angle
 *             (6.8e-7 rad for a quarter turn of the default robot at 10 ms), and the x, y gap is what a planner has to keep
 *             small.  Without a row in front the x, y entries are 0, and the heading entry is NaN unless a start heading was
 *             given.  d_flags [R] or NULL: bits are OR-ed in.
 *   failures  a routine with a used slot whose leg index is outside [0, L), whose leg has no rows, or whose first-row or
 *             last-row x or y is not finite or heading is not within [-2 pi, 2 pi] (the rows of vap_time_profile keep
 *             [-pi, pi]), or with such a start heading: VAP_FLAG_BAD_ROUTE, 0 rows, map -1, seam NaN, and none of its rows
 *             is written.  Truncation is vap_time_insert_events': rows [0, capacity_out) are exactly those of a call with
 *             enough capacity, nothing is written at or behind capacity_out, the count is capacity_out, VAP_FLAG_TRUNCATED;
 *             d_map and d_seam are NOT cut.
 * One workgroup per (routine, slot); each derives its routine's offsets itself.  VAP_ERR_INVALID: M < 1, R < 0, L < 0, a negative
 * capacity, counts_stride < 1, a time_step that is not positive and finite, a turn_min that is negative or not finite, null
 * constraints or a max_vel, max_acc or track_width that is not positive and finite, a null leg, count, map, seam or row
 * pointer with R > 0, d_rows_out == d_rows_in, a row pointer that is not 16-byte aligned (hipMalloc's and torch's allocations
 * are).  VAP_ERR_UNSUPPORTED: M > 32, R * M above INT_MAX, a full turn of more than
 * 2^20 rows.  The arguments are checked before the context is touched.  R = 0 is a no-op.  Works on the context's stream and
 * does not synchronise; no atomics beside the flag OR: two calls give the same bits. */
#define VAP_TIMELINE_MAX_LEGS 32
int vap_routine_timeline(vap_ctx *ctx, int R, int M, int L, int capacity_in, int capacity_out, double time_step,
                         const vap_constraints *c, double turn_min, const double *d_rows_in, const int *d_counts_in,
                         int counts_stride, const int *d_leg, const int *d_n_legs, const double *d_dwell,
                         const double *d_start_heading, double *d_rows_out, int *d_counts_out, int *d_map, double *d_seam,
                         uint32_t *d_flags);

/* ---- a routine's visiting order by the clock ----------------------------------------------------------------------------------
 * vap_plan_order orders the sites by any P x P cost, which cannot carry what a routine's time is made of: a routine lasts
 * rows * dt, and its rows are, slot by slot, the rows of the turn on the spot (which depend on the heading the robot arrives
 * with, so on the leg before), the leg's own rows and int(dwell / dt).  vap_plan_order_timed runs Held-Karp over (site set,
 * last site, site before it) on exactly these integers, read from the legs' time-domain rows, so that its total for an order
 * IS, bit for bit, the row count vap_routine_timeline gives for that order; optionally it selects the subset of sites worth
 * the most under a row budget.  The reference has neither (a routine is a hand-ordered list of nodes, gui/path.py).
 *   points    point 0 is the start, points 1 .. M = P - 1 are the sites, 1 <= M <= 8 (VAP_PLAN_ORDER_TIMED_MAX_SITES): the
 *             table is 2^M * M * M int32 plus a parent byte each, 80 KiB of LDS at M = 8; at M = 9 it would be 166 KB and
 *             leaves the LDS, so P > 9 is VAP_ERR_UNSUPPORTED.
 *   legs      d_rows [L][capacity][8], d_counts [L * counts_stride] (entry l * counts_stride = rows of leg l): L legs on the
 *             device, exactly as vap_routine_timeline takes them, all on the time step `time_step`.  d_leg [R][P][P] int32:
 *             the leg from point a to point b of problem r; column 0 and the diagonal are never read.  A leg is USABLE iff
 *             its index is in [0, L), d_leg_flags (uint32 [L], may be NULL) is 0 for it, c = min(count, capacity) > 0, and
 *             its first and last row pass the timeline's own test: heading (column 4) within [-2 pi, 2 pi], x and y (columns
 *             6, 7) finite.  Every other leg is forbidden.  For a usable leg n(a, b) = c, hf(a, b) = the heading of row 0,
 *             hl(a, b) = the heading of row c - 1.
 *   turn      turn(h_front, h_first) is 0 rows when h_front is NaN.  Otherwise D = h_first - h_front; if D > pi, D -= 2 pi;
 *             if D <= -pi, D += 2 pi; |D| < turn_min: 0 rows, else the n = ceil((total_time + dt) / dt) rows of the
 *             timeline's turn for angle = -D with c->max_vel, max_acc, track_width (compiled from the same text).
 *   dwell     d_dwell [R][P] seconds at SITE j, or NULL; entry 0 is unused.  w(j) = int(dwell / dt) for a dwell > 0,
 *             saturating at INT_MAX, else 0.
 *   rows      of a sequence s_1 .. s_k of distinct sites, s_0 = 0:
 *               sum over m = 1 .. k of [ turn(h_{m-1}, hf(s_{m-1}, s_m)) + n(s_{m-1}, s_m) + w(s_m) ],
 *             h_0 = d_start_heading[r] (NULL or NaN: none), h_m = hl(s_{m-1}, s_m); arrival_m = the rows in front of slot m
 *             + its turn + its leg, the timeline's map[r][m - 1][2].  Summed in 64 bits; a sequence of INT_MAX rows or more
 *             is inadmissible.  A start heading outside [-2 pi, 2 pi] makes the problem infeasible (the empty sequence
 *             included), as it makes a routine bad.
 *   admissible  every leg of the sequence is usable; for every visited k every site of before[k] is visited earlier
 *             (d_before [R][P] uint32 or NULL, the masks of vap_plan_order; entry 0 and bits >= M are ignored); if end >= 1
 *             the sequence ends at `end` (so the empty sequence is then not admissible); end = -1: it may end anywhere.
 *   full mode (d_budget_rows == NULL): k = M and the fewest rows win; among equals the sequence that is smallest read
 *             BACKWARDS: the lowest last site, then the lowest site before it, and so on.  (The table's minimum over (last,
 *             previous) in lexicographic order and the lowest parent under a strict < at every step back give exactly this;
 *             the costs are integers, nothing is rounded.)
 *   budget mode (d_budget_rows [R] int32; negative counts as 0): over all admissible sequences of any k >= 0 with rows <=
 *             budget: the largest value(S), then the fewest rows, then the smallest S as an integer (bit j - 1 = site j),
 *             then the backwards rule.  value(S) is the fp64 sum of d_value[r][j] over the sites of S in ascending j,
 *             starting from 0.0; d_value [R][P] or NULL (1 each; entry 0 unused); an entry that is NaN, negative or infinite
 *             counts as 0.  With every value positive and an ample budget the result equals full mode's.
 *   outputs   d_order [R][M] int32: the visited sites in order, then -1; d_n_visited [R] int32; d_rows_total [R] int32;
 *             d_arrival_rows [R][M] int32, -1 behind the visited slots; d_value_total [R] fp64 (full mode: value of the full
 *             set); d_flags [R] uint32, optional, written (not OR-ed).  No admissible sequence: order and arrival -1,
 *             n_visited 0, rows_total -1, value NaN, VAP_ORDER_INFEASIBLE.
 * One workgroup per problem at a time with the table in LDS.  VAP_ERR_INVALID: P < 2, R < 0, L < 0, a negative capacity,
 * counts_stride < 1, end outside {-1, 1 .. M}, a null leg or order / n_visited / rows_total / arrival_rows / value_total pointer
 * with R > 0, a null row or count pointer with R > 0 and L > 0 (rows: and capacity > 0), and every time step, turn_min and
 * constraints vap_routine_timeline refuses, its rule that a full turn may not exceed 2^20 rows included.  VAP_ERR_UNSUPPORTED:
 * P > 9.  The arguments are checked before the context is touched.  R = 0 is a no-op.  Works on the context's stream and does
 * not synchronise; no atomics: two calls give the same bytes. */
#define VAP_PLAN_ORDER_TIMED_MAX_SITES 8
int vap_plan_order_timed(vap_ctx *ctx, int R, int P, int L, int capacity, double time_step, const vap_constraints *c,
                         double turn_min, const double *d_rows, const int *d_counts, int counts_stride, const int *d_leg,
                         const uint32_t *d_leg_flags, const double *d_dwell, const double *d_start_heading, const double *d_value,
                         const int *d_budget_rows, int end, const uint32_t *d_before, int *d_order, int *d_n_visited,
                         int *d_rows_total, int *d_arrival_rows, double *d_value_total, uint32_t *d_flags);

/* ---- drive limits: curve caps for the velocity pass, and an audit of time-domain rows -------------------------------------------
 * vap_constraints carries friction_coef and max_jerk, and forward_backward_pass reads neither; the reference also computes
 * curvature_derivs (MPG:178-186) for a curvature-rate cap, limit_velocity_by_ang_accel (MPG:41-50), that it comments out of
 * both sweeps (MPG:215-220, 276-281), and the wheel speeds (MPG:594-599) and wheel accelerations (MPG:612-616) of every
 * time-domain row, which it drops on return.  The two calls below use them; no other entry point changes.
 *
 * vap_curve_caps writes, per sample, min(incoming cap, lateral cap, curvature-rate cap) into a row that
 * vap_velocity_pass_limits takes as d_vcap.
 *   rows      N = meta[b][3] (taken as 0 below 0 and as S above S), dd = meta[b][2], as vap_velocity_conditioning.
 *             d_curvature [B][S] in `dt`, or NULL for VAP_F32 with VAP_RECURRENCE_F64: the fp64 rows the last sampling call
 *             of this shape left on the context (VAP_ERR_INVALID where it holds none).  d_vcap_in / d_vcap_out [B][S] of type
 *             vap_limit_rows_dtype(ctx, dt); d_vcap_in NULL = c->max_vel everywhere; the two may be the same row (in place,
 *             e.g. behind vap_route_limits).  Row addresses that are not 16-byte aligned are moved element by element.
 *   arithmetic  fp64 on widened inputs, IEEE divisions and square roots, no contraction; an fp32 result is rounded to nearest.
 *   lateral   cap_lat = sqrt(A / |k|) where |k| > 0, else +inf; A = lateral_acc_max (ft/s^2; friction_coef * g).
 *   rate      dk_0 = (k_1 + k_0) / dd, dk_(N-1) = (k_(N-1) + k_(N-2)) / dd, dk_i = (k_(i+1) - k_(i-1)) / (2 dd) between.  The
 *             two PLUS signs are the reference's own (MPG:180, 182; a quirk: the ends hold a mean curvature over dd / 2, not
 *             a difference) and are kept.  cap_ang = max_vel if |dk| < 1e-9, else min(sqrt(alpha / |dk|), max_vel), the left
 *             operand unless the right is strictly smaller (MPG:45-50); alpha = angular_acc_max (rad/s^2; the reference's
 *             max_angular_accel is 2 max_acc / track_width, MPG:82).  N < 2, or alpha = +inf, gives no cap (+inf).
 *   output    out_i = min(in_i, cap_lat, cap_ang) for i < N in Python's order: in_i, unless cap_lat is strictly smaller, then
 *             that, unless cap_ang is strictly smaller.  A NaN curvature gives out_i = NaN (the velocity pass flags such a
 *             path).  Samples i >= N receive in_i.  The velocity pass takes entry 0 and the end sample from start_vel / end_vel.
 *   count     d_n_bound [B][2] int32, optional: the samples i < N with cap_lat < in_i, and with cap_ang < in_i (integer
 *             atomics: deterministic).
 * VAP_ERR_INVALID, before the context is touched: a limit that is NaN or <= 0 (+inf switches a cap off), a non-finite max_vel or
 * track_width, a null meta, limits, constraints or output pointer with B > 0.  B = 0 is a no-op.  Works on the context's stream
 * and does not synchronise. */
typedef struct {
    double lateral_acc_max; /* ft/s^2;  +inf = off */
    double angular_acc_max; /* rad/s^2; +inf = off */
} vap_curve_limits;
int vap_curve_caps(vap_ctx *ctx, vap_dtype dt, int B, int S, const vap_constraints *c, const vap_curve_limits *lim,
                   const double *d_meta, const void *d_curvature, const void *d_vcap_in, void *d_vcap_out, int *d_n_bound);

/* vap_drive_audit: what the drivetrain has to do to follow time-domain rows.  d_rows [B][capacity][8] in the layout of
 * vap_time_profile (any producer of it: vap_time_profile[_routes], vap_time_insert_waits / _events, vap_routine_timeline, the
 * rollouts' executed rows); n = d_counts[b * counts_stride] clamped to [0, capacity].  Only column 2 (v) and column 5 (omega)
 * are read.  With T = track_width and h = time_step, for row r < n, every operation fp64 and IEEE, in this order:
 *   wL = v - (omega T) / 2, wR = v + (omega T) / 2            MPG:594-599, get_wheel_trajectory (MPG:641-642)
 *   aL = (wL_r - wL_(r-1)) / h, aR likewise                   MPG:612-616 — but a wheel before row 0 stands still (0.0): the
 *                                                             reference's i = 0 wraps to index -1, the LAST row; not kept
 *   b = (v_r - v_(r-1)) / h, j = (b_r - b_(r-1)) / h          v_(-1) = b_(-1) = 0
 *   l = v omega,  g = (omega_r - omega_(r-1)) / h             omega_(-1) = 0
 * and the audited quantities q0 = max(|wL|, |wR|), q1 = max(|aL|, |aR|), q2 = |j|, q3 = |l|, q4 = |g|, with the limits
 * wheel_speed_max, wheel_acc_max, jerk_max, lateral_acc_max, angular_acc_max in that order.
 *   outputs (any may be NULL)
 *     d_peak [B][5] fp64         the maximum of each q over the route's rows
 *     d_peak_row [B][5] int32    the first row attaining it
 *     d_n_over [B][5] int32      the rows with q strictly above its limit (+inf: never)
 *     d_first_over [B][5] int32  the first such row, or -1
 *     d_route_status [B] int32   bit 1 (value 2): a non-finite v or omega among rows 0 .. n - 1 (vap_pursuit_rollouts'
 *                                convention); such a route is treated as a route with n = 0
 *     d_wheel_rows [B][capacity][8] fp64  {wL, wR, aL, aR, b, j, l, g}, signed, for rows below n; nothing is written at or
 *                                above n
 *   n = 0 gives NaN peaks, -1 rows and 0 counts.  A q that is NaN (finite inputs can only give one by overflow) neither becomes
 *   a peak nor counts.
 * d_rows and d_wheel_rows must be 16-byte aligned.  The peaks are reduced as (value, row) pairs under one total order (the
 * larger value, then the lower row) and the counts as integers, so the result does not depend on how the rows are tiled; no
 * float atomics: two calls give the same bits.
 * VAP_ERR_INVALID, before the context is touched: a track_width or time_step that is not positive and finite, a limit that is
 * NaN or negative, a null rows, counts or limits pointer with B > 0, a misaligned pointer, B < 0, capacity < 0,
 * counts_stride < 1.  B = 0 is a no-op.  Works on the context's stream and does not synchronise. */
typedef struct {
    double track_width, wheel_speed_max, wheel_acc_max, jerk_max, lateral_acc_max, angular_acc_max;
} vap_drive_limits;
int vap_drive_audit(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                    double time_step, const vap_drive_limits *lim, double *d_peak, int *d_peak_row, int *d_n_over,
                    int *d_first_over, int *d_route_status, double *d_wheel_rows);

/* ---- range-sensor readings of time-domain rows against the scene ---------------------------------------------------
 * Everything above takes the pose for known.  On a robot it comes from dead reckoning, and the usual cure is a wall-facing
 * distance sensor that resets one coordinate when it sees a wall it can trust.  This call says what such a sensor would read
 * at every row, and where along a route a reset is possible at all.  Units: feet, the rows' own frame.  The whole call is fp64.
 *
 *   rows      d_rows [B][capacity][8], d_counts with counts_stride, exactly as vap_footprint_clearance takes them (counts
 *             clamped to [0, capacity]; only columns 4, 6, 7 are read).  Pose p = (x, y), phi = -heading, a body point v sits
 *             at p + R(phi) v.
 *   scene     h_field (or NULL), polygons, circles: vap_footprint_clearance's, the same validation, limits and status codes.
 *   sensors   h_sensors [n_sens][8] = {mx, my, ux, uy, r_min, r_max, min_cos, 0}, n_sens 1..8: the mount point in the body
 *             frame (ft); the beam direction as a body-frame unit vector, |hypot(ux, uy) - 1| <= 1e-12 (the caller gives it,
 *             nothing is renormalised); the valid window 0 <= r_min <= r_max (ft); min_cos in [0, 1], the smallest accepted
 *             cosine of the incidence angle.
 *   partners  optional (Bo = 0, cap_o = 0 or NULL rows: none): d_rows_o [Bo][cap_o][8], d_counts_o with stride_o, one footprint
 *             h_foot_o [n_foot_o][2] (convex, counter-clockwise, 3..16 vertices), shift_rows.  Bo <= 16.  Every route of the call
 *             sees every partner; partner o at row r stands at its own row clamp(r - shift_rows, 0, n_o - 1)
 *             (vap_footprint_conflicts' parking); a partner without rows is absent.  Both sides are on the same time step (the
 *             caller guarantees it).
 *   reading   (row r, sensor s).  The beam is a single ray: it has no cone, the robot's own body is not seen, and motion
 *             between rows is not swept.  With c, s = cos phi, sin phi taken once per row: origin o = p + R(phi)(mx, my),
 *             direction u = (c ux - s uy, s ux + c uy).  Candidates in this order; a later one replaces the best only on a
 *             strictly smaller t, so the first in this order wins a tie:
 *             1. wall, element -1: only with a field and only if o lies inside or on the box.  For u.x > 0 t = (xmax - o.x) /
 *                u.x, for u.x < 0 t = (xmin - o.x) / u.x, likewise in y; the smaller wins, on a tie the x side.  face = 0 xmin,
 *                1 ymin, 2 xmax, 3 ymax; cos_inc = |u.x| or |u.y|.
 *             2. polygons k = 0 .. n_poly - 1, element k, edges j ascending, face = j.  For the edge a -> a + e: den = u x e
 *                (0: no candidate), t = ((a - o) x e) / den, w = ((a - o) x u) / den; a candidate if t >= 0 and 0 <= w <= 1;
 *                cos_inc = |u . n|, n the edge's unit normal.  Any edge counts: an origin inside a polygon reads the distance
 *                to its way out.
 *             3. circles, element n_poly + k, face 0.  d = o - centre, b = d . u, q = d . d - r^2, disc = b^2 - q (< 0: no
 *                candidate); t = -b - sqrt(disc), if that is < 0 t = -b + sqrt(disc), if still < 0 no candidate; cos_inc =
 *                |u . (o + t u - centre)| / r.
 *             4. partners, element n_poly + n_circle + o: the posed footprint's edges as a polygon's, face = edge index.
 *             A comparison with a NaN is false: NaN candidates take part in nothing.
 *   status    in priority order: 6 bad pose (non-finite x, y or heading), 1 no candidate, 5 the nearest is a partner (blocked),
 *             2 t < r_min, 3 t > r_max, 4 cos_inc < min_cos, 0 valid.
 *   outputs   any pointer may be NULL (nothing is written for it).
 *             per reading [B][capacity][n_sens]: d_range (t wherever a candidate exists, whatever the status; NaN for status
 *             1 and 6 and for rows >= count), d_cos_incidence (the same NaN rule), d_code (int32) = status | face << 4 |
 *             (element + 2) << 12, the element field 0 when there is none; -1 for rows >= count.
 *             per route and sensor: d_status_counts [B][n_sens][8] (rows per status 0..6, slot 7 = 0), d_range_minmax
 *             [B][n_sens][2] (smallest and largest valid range, NaN if none).
 *             per route and channel: d_channels [B][n_sens + 2][5] = {n_ok, first_ok, last_ok, gap_rows, gap_row}.  Channel
 *             s < n_sens: sensor s valid at this row; channel n_sens: some sensor valid on a wall face 0 or 2 (x observable);
 *             channel n_sens + 1: the same for faces 1 or 3 (y observable).  gap_rows: the longest run of consecutive rows of
 *             [0, n) that are not ok, leading and trailing runs included (0 if every row is ok, n if none is); gap_row: the
 *             first row of the earliest longest run, -1 when gap_rows = 0.  A route with n = 0 gets 0 counts, NaN and
 *             {0, -1, -1, 0, -1}.
 * VAP_ERR_INVALID: n_sens outside 1..8, a non-finite sensor entry or one outside the bounds above, a null rows or counts
 * pointer with B > 0, a bad shape or stride, a partner footprint that vap_footprint_clearance would refuse, every scene error
 * of that call.  VAP_ERR_UNSUPPORTED: its scene limits, more than 16 partners, a capacity above INT_MAX - 2048.  B = 0 is a
 * no-op.  No pointer has an alignment requirement beyond its type's.  VAP_OPT_FOOTPRINT_CULL governs culling (an element is
 * skipped only when its bounding circle, with the rounding slack of vap_footprint_clearance, cannot hold a strictly nearer hit);
 * on and off give the same bits.  Every summary is an integer or a min / max, and the gap is combined with an associative
 * record, so the result does not depend on how the rows are tiled; no float atomics: two calls on the same inputs give the same
 * bits.  Works on the context's stream and does not synchronise. */
int vap_range_readings(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride, int n_sens,
                       const double *h_sensors, const double *h_field, int n_poly, const int *h_poly_start, const double *h_poly_xy,
                       int n_circle, const double *h_circles, int Bo, long cap_o, const double *d_rows_o, const int *d_counts_o,
                       int stride_o, int n_foot_o, const double *h_foot_o, int shift_rows, double *d_range, double *d_cos_incidence,
                       int *d_code, int *d_status_counts, double *d_range_minmax, int *d_channels);

/* ---- odometry rollouts: the follower steers on a dead-reckoned pose with range resets -----------------------------------
 * vap_tracking_rollouts feeds the follower the true pose and vap_range_readings says what a sensor reads along given rows.
 * This call closes the loop: the RAMSETE follower of vap_tracking_rollouts steers on an ESTIMATE of the pose, the estimate
 * drifts with encoder and gyro errors, and it is pulled back whenever a range reading passes a gate.  "With these sensors the
 * robot ends within x ft of the goal."  fp64 throughout.
 *
 *   rows, counts, follower, perturbation records, the plant, saturation, substeps and settle rows: vap_tracking_rollouts'.
 *   sensors   h_sensors [n_sens][8] and the scene (h_field .. h_circles): vap_range_readings', the same validation and limits.
 *             There are no partners.  n_sens may be 0 (pure dead reckoning); the sensors, the scene and the rule may then be NULL.
 *   odometry  d_odometry [B][K][8], or [K][8] with shared_odometry != 0; a record is {enc_left, enc_right, heading_scale,
 *             heading_drift (rad/s), range_scale, range_bias (ft), 0, 0}; the ideal record is {1, 1, 1, 0, 1, 0, 0, 0}.  A record
 *             with a non-finite entry, enc_* <= 0, heading_scale <= 0 or range_scale <= 0 is invalid, and its rollout is treated
 *             as one with an invalid perturbation record.
 *   rule      vap_reset_rule {gate (ft), min_cos, gain, every}.
 *   state     the true plant as in vap_tracking_rollouts (row 0's pose plus (dx, dy, dphi)).  The estimate (xh, yh, phih) starts
 *             at row 0's pose exactly: the robot believes it was placed where the plan starts.
 *   step      r = 0 .. n + settle_rows - 1, in this order:
 *             1. resets, only if n_sens > 0 and r % every == 0; sensors s ascending, each sees the estimate as the earlier
 *                ones left it.  (a) The true reading is what vap_range_readings gives for executed row r: pose heading =
 *                -wrap(phi), x, y; candidates 1-3 of that call; the same status rules.  Only status 0 yields a reading,
 *                z = range_scale t + range_bias; any other status leaves the estimate alone and counts nowhere.  (b) The expected
 *                reading is taken from the estimate against the walls only: oh = ph + R(phih)(mx, my), uh = R(phih)(ux, uy), cos
 *                and sin of phih taken once per row; rule 1 of vap_range_readings gives th, a face and cosh; no candidate without
 *                a field or with oh outside the box.  The reset is accepted iff there is a wall candidate, cosh >= min_cos and
 *                |z - th| <= gate (a NaN comparison is false); otherwise it is rejected.  (c) Accepted, faces 0 and 2:
 *                xh += gain (th - z) uh.x; faces 1 and 3: yh += gain (th - z) uh.y.  phih is never reset.
 *             2. errors: the control errors are step 1 of vap_tracking_rollouts with (ph, phih) in place of the pose; the true
 *                errors e_x, e_y, e_phi, e_pos the same with the true pose; e_est = hypot(xh - x, yh - y), e_estphi =
 *                |wrap(phih - phi)|.
 *             3. statistics on the true errors as vap_tracking_rollouts' step 2, plus the maxima of e_est and e_estphi.
 *             4. executed row r (if requested): vap_tracking_rollouts' step 3.  Estimate row r (if requested):
 *                {-wrap(phih), xh, yh, (double) mask}, bit s of mask set when sensor s was accepted at this row.
 *             5. RAMSETE with the control errors.  6. saturation: unchanged.
 *             7. n_substeps substeps, each the plant's substep and then the estimate's from the wheel speeds and omega the plant
 *                just used, in exactly these operations: vh = (enc_left (g_L w_L) + enc_right (g_R w_R)) / 2;
 *                D = (heading_scale omega) h + heading_drift h; uh = D / 2; dh = vh h sinc(uh);
 *                ph += dh (cos(phih + uh), sin(phih + uh)); phih += D.  With the ideal record and a zero start offset the
 *                estimate equals the true pose bit for bit, and the call equals vap_tracking_rollouts.
 *             After the last step: vap_tracking_rollouts' final errors of the true pose, and the final e_est.
 *   outputs   any pointer may be NULL.  d_stats [B][K][8] = {max e_pos, max |e_y|, max |e_phi|, final position error, final
 *             heading error, max e_est, max e_estphi, final e_est}; d_stat_rows [B][K][4] = {row of max e_pos, saturated rows,
 *             resets accepted, resets rejected}; the five per-route outputs as vap_tracking_rollouts over the max e_pos column,
 *             in the same fixed order; d_exec_rows, d_exec_counts and cap_exec exactly as there (both clearance calls and
 *             vap_range_readings take them); d_est_rows [B * K][cap_exec][4].  Edges (n = 0, invalid records, a route without
 *             a valid rollout) as there: NaN / -1 / 0.
 * VAP_ERR_INVALID, before the context is touched: everything vap_tracking_rollouts and the sensor and scene checks of
 * vap_range_readings refuse; n_sens outside 0..8; a negative or non-finite gate; min_cos or gain outside [0, 1]; every outside
 * 1..10000; a null rule or sensors pointer with n_sens > 0; a null odometry pointer with B > 0; a d_odometry or d_est_rows that
 * is not 16-byte aligned.  VAP_ERR_UNSUPPORTED: the scene limits of vap_range_readings.  B = 0 is a no-op.
 * VAP_OPT_FOOTPRINT_CULL governs the cull of the true ray, on and off give the same bits.  Works on the context's stream and
 * does not synchronise.  Two calls on the same inputs give the same bits: no float atomics. */
typedef struct {
    double gate, min_cos, gain;
    int every;
} vap_reset_rule;
int vap_odometry_rollouts(vap_ctx *ctx, int B, long capacity, const double *d_rows, const int *d_counts, int counts_stride,
                          double time_step, const vap_follower *f, int K, int shared_perturb, const double *d_perturb,
                          int shared_odometry, const double *d_odometry, int n_sens, const double *h_sensors,
                          const vap_reset_rule *rule, const double *h_field, int n_poly, const int *h_poly_start,
                          const double *h_poly_xy, int n_circle, const double *h_circles, double *d_stats, int *d_stat_rows,
                          double *d_worst, double *d_mean, int *d_worst_rollout, int *d_worst_row, int *d_n_exceeding,
                          long cap_exec, double *d_exec_rows, int *d_exec_counts, double *d_est_rows);

/* ---- a routine's waits against its partners, every slot at once ------------------------------------------------------------
 * vap_conflict_shifts delays a whole route, and a caller can delay everything from one slot on.  Neither says "leave the start
 * before the partner parks on it, then wait at site 1 until the crossing is free".  A chained routine stands still at every
 * slot boundary, so a wait there is free: these two calls return, per routine, how many rows to wait in front of every slot
 * so that the whole routine clears every partner and finishes as early as possible.
 *   side A    R routines: d_rows_a [R][cap_a][8], d_counts_a with stride_a, the footprint and the pose (columns 4, 6, 7, phi =
 *             -heading) as vap_footprint_conflicts reads them; n = the count clamped to 0 .. cap_a.  d_seg_start [R][M] int32, 1
 *             <= M <= VAP_TIMELINE_MAX_LEGS: entry m is the first row of segment m (vap_routine_timeline's d_map[r][m][0]); a
 *             negative entry is an unused slot.  With S the number of used slots, b_0 .. b_{S-1} their entries and b_S = n,
 *             segment m is rows [b_m, b_{m+1}).  A routine with n > 0 and S >= 1 is bad unless b_0 == 0, the starts ascend
 *             strictly, b_{S-1} < n and no used slot stands behind an unused one: VAP_FLAG_BAD_ROUTE is OR-ed into d_flags,
 *             n_seg = 0, NaN tables.  A routine with n = 0 or S = 0 gets n_seg = 0 and NaN tables without a flag.
 *   side O    Bo partners: rows, counts, stride and footprint as in vap_conflict_shifts.  At instant t a partner stands at its
 *             row clamp(t, 0, n_o - 1); one with n_o == 0 takes part in nothing.  Every routine is taken against every
 *             partner.  The clearance of a pose pair is vap_footprint_conflicts'; a NaN clearance takes part in nothing.
 *   delays    n_delays = C (1 .. VAP_SCHEDULE_MAX_DELAYS) cumulative delays k = 0 .. C - 1 of k * delay_step rows, delay_step =
 *             q >= 1; (C - 1) q must not exceed INT_MAX.
 *   tables    d_move, d_wait [R][M][C] fp64; an unused slot's entries are NaN.
 *             move[m][k]: the smallest clearance over the partners and the rows i in [b_m, b_{m+1}) of A's row i against the
 *             partner's pose at instant i + k q.  For the last used segment also A parked at row n - 1 at the instants n + k q
 *             .. n_o - 1 of each partner (VAP_HOLD_A_LAST of the calls above).
 *             wait[m][u]: the smallest clearance of the hold pose, A's row max(b_m - 1, 0), at the instants b_m + u q .. b_m +
 *             (u + 1) q - 1.
 *             An entry is NaN when nothing finite was examined.  An entry is blocked iff it is < margin; NaN never blocks.
 *             The tables are a composition of vap_conflict_shifts' table: move[m] is that call on the segment's rows as a
 *             route of their own at the shifts -(b_m + k q) with hold 12 (14 for the last used segment), wait[m][u] the
 *             minimum of q entries of the one-row route of the hold pose at hold 12 — the same numbers.
 *   schedule  indices 0 <= k_0 <= .. <= k_{S-1} < C with move[m][k_m] unblocked for every m and wait[m][u] unblocked for
 *             every k_{m-1} <= u < k_m (k_{-1} = 0).  The answer has the smallest k_{S-1}; among those, from m = S - 2 down to
 *             0, the largest k_m: the waits happen as early in the routine as the partners allow.
 *   outputs   d_delay_rows [R][M] int32: d_0 = k_0 q, d_m = (k_m - k_{m-1}) q rows to wait in front of slot m; 0 for unused
 *             slots; -1 in EVERY slot when the window holds no schedule or n_seg == 0.  d_total_rows [R]: k_{S-1} q or -1.
 *             d_clearance [R]: the smallest finite table entry the schedule uses (its moves and its waits), or NaN.  A
 *             routine with rows and no valid partner is blocked nowhere: all zeros.
 * vap_schedule_tables packs both sides as vap_conflict_shifts does and sweeps: one wave per (routine, band of up to 64 delays),
 * one walk over the routine's rows per partner.  Any of d_move, d_wait, d_n_seg [R], d_flags [R] may be NULL.  Context scratch
 * is the two packs, (R cap_a + Bo cap_o) x 32 B with capacities rounded up to 64 rows; nothing grows with R x M x C beside the
 * two tables.  VAP_OPT_FOOTPRINT_CULL governs culling; on and off, and two calls, give the same bits.
 * vap_schedule_solve is the search alone, on any tables the caller hands it: F_{-1} = {0}; G_m[k] = F_{m-1}[k] or (G_m[k - 1]
 * and wait[m][k - 1] unblocked); F_m[k] = move[m][k] unblocked and G_m[k]; one wave per routine, bit-packed in LDS.  d_n_seg
 * [R] is S per routine (clamped to 0 .. M); any of the three outputs may be NULL.  Integers only: two calls give the same bits.
 * VAP_ERR_INVALID: M, n_delays or delay_step < 1, a negative R, Bo or capacity, a count stride < 1, a margin that is not
 * finite, a bad footprint, null rows, counts, segment starts or (solve) tables or d_n_seg with R > 0.  VAP_ERR_UNSUPPORTED: M
 * above VAP_TIMELINE_MAX_LEGS, n_delays above VAP_SCHEDULE_MAX_DELAYS, (C - 1) q or a capacity above INT_MAX, more workgroups
 * than one launch takes.  Arguments are checked before the context is touched.  R = 0 is a no-op; Bo = 0 is valid (NaN tables,
 * so an all-zero schedule for a routine with rows).  Both work on the context's stream and do not synchronise. */
#define VAP_SCHEDULE_MAX_DELAYS 4096
int vap_schedule_tables(vap_ctx *ctx, int n_delays, int delay_step,
                        int R, long cap_a, const double *d_rows_a, const int *d_counts_a, int stride_a, int n_foot_a,
                        const double *h_foot_a, int M, const int *d_seg_start,
                        int Bo, long cap_o, const double *d_rows_o, const int *d_counts_o, int stride_o, int n_foot_o,
                        const double *h_foot_o,
                        double *d_move, double *d_wait, int *d_n_seg, uint32_t *d_flags);
int vap_schedule_solve(vap_ctx *ctx, int R, int M, int n_delays, int delay_step, double margin, const double *d_move,
                       const double *d_wait, const int *d_n_seg, int *d_delay_rows, int *d_total_rows, double *d_clearance);

#ifdef __cplusplus
}
#endif
#endif /* VAP_H */
