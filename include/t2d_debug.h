/* t2d_debug.h -- test and measurement hooks of the MI355X-native batched tactics2d step.
 *
 * NOT part of the product ABI.  libt2d_hip.so (include/t2d.h) exports none of these; they exist only in
 * libt2d_hip_debug.so = the same sources built with -DT2D_DEBUG_HOOKS (python -m tactics2d_amd.build --debug-lib), which
 * exports everything t2d.h declares plus what is declared here.  Loaded by tests/, bench.py's closed_loop leg and scripts/
 * through tactics2d_amd/debug.py; no product module imports that.  The reference's operator API has no counterpart of any of
 * this (fault injection, a delayed collective, a stand-in policy, placement maps): they are how the build is TESTED.
 *
 * The -DT2D_DEBUG_HOOKS build differs from the product in exactly: these entry points, tactics2d_amd/csrc/t2d_loop.hip, the
 * math probe (tactics2d_amd/csrc/t2d_math_probe.hip and t2d_math_probe_table.hip, which compile t2d_math.h once more and touch
 * no product kernel), the geometry probe (t2d_geom_probe.hip: t2d_geom_dev.h once more, likewise), the wave-scan probe (a one-wave
 * kernel at the end of t2d_collide.hip that calls the step kernel's wave_excl_scan), and two reads inside the step kernel (the placement map of a single launch, the fault word of a chained one).
 */
#ifndef T2D_DEBUG_H_
#define T2D_DEBUG_H_
#include "t2d.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Placement of the step launch: entry b = logical workgroup (the envs [g * epb, (g + 1) * epb), epb = 256 / padded
 * max_agents unless the geometry budget narrowed it) | wave rotation 0..3 << 16 that physical workgroup b steps.  Must be a
 * permutation of the launch's workgroups; NULL / 0 restores the identity.  Results never depend on it -- the hardware
 * places workgroup b on XCD b mod 8 and its waves on fixed SIMDs, so the map only decides which envs share a SIMD and
 * which XCD gets the expensive ones.  Reset by every t2d_set_*_geometry.  Host memory.                                  */
int t2d_debug_set_step_placement(t2d_pool* pool, const uint32_t* map_host, int32_t n_workgroups);

/* Test hook: the CHAIN launches of t2d_step_n enqueued from now on break ONE hand-off on purpose -- workgroup 1 posts its step
 * 1 with a foreign XCC id (kind 1: what a consumer on another XCD would see) or not at all (kind 2: its consumer's bounded
 * wait runs out after ~0.2 s); kind 3: it posts its step 0 with a foreign XCC id, so that the failure is on record while the
 * fragment's first step is still being dispatched (a grid larger than the device holds: the checkpoint must still be complete);
 * 0 = off.  Needs a pool of >= 2 step workgroups and fragments of >= 3 steps to have any effect. */
int t2d_debug_chain_fault(t2d_pool* pool, int32_t kind);

/* Test hook: occupies the pool's gather stream for `microseconds` (one idle wave), so that the gathers enqueued after it
 * start late -- what a slow peer does to the collective.  tests/test_gpu_dist.py uses it to check that a step about to
 * overwrite a record slot really waits for the gather that still has to read it.                                       */
int t2d_debug_delay_gather(t2d_pool* pool, int32_t microseconds);

/* Which instantiation of the step / event kernel the LAST launch of this process took: its template arguments as written at the
 * launch site in tactics2d_amd/csrc/t2d_collide.hip, e.g. "(true, 1, false, true)" = the chained fused step, fast integrator.
 * tests/test_gpu_forms.py drives one recipe per launch site and holds the set it sees against the list in the source file
 * (DESIGN.md 4.2c).  Not thread-safe; a static string.                                                                    */
const char* t2d_debug_last_step_kernel(void);
/* ... and its SHAPE: 64 = the twin of that form with envs of 64 participants, four per workgroup, compiled in (the plain step and
 * the plain chained step of such pools take it: DESIGN.md 4.2c), 0 = the generic instantiation, which reads its shape from the
 * launch.  t2d_debug_set_step_shape64(pool, 0) keeps a pool on the generic instantiations (1: back to the default), so that tests
 * and measurements can hold the two against each other on one pool: same results, bit for bit (tests/test_gpu_shape64.py). */
int t2d_debug_last_step_shape(void);
int t2d_debug_set_step_shape64(t2d_pool* pool, int32_t on);

/* ---- the closed loop (measurement / test helpers; tactics2d_amd/csrc/t2d_loop.hip) -----------------------------------------
 * The reference's callers run  action = policy(obs); obs, reward, ... = env.step(action)  (envs/parking.py:219-256 inside the
 * tutorial's training loop).  On the device that is: a policy kernel that reads the state the previous step left behind and
 * writes an [N, 2] (steering, accel) tensor -> t2d_step reading it in place (t2d_bind_actions_strided) -> the policy again,
 * with no host synchronisation; the envs cut into groups -- one pool and one stream each -- so that one group's policy,
 * start-up and tail overlap the other groups' busy middle (env groups: tactics2d_amd/pipeline.py, t2d_step_groups).
 *   t2d_debug_feedback_policy   a STAND-IN policy, one launch: per participant accel = clip(k_speed (v_target - speed), -3, 2),
 *                               steering = k_steer sin(0.05 x + 0.08 y + heading); act_out_dev = f32 [N][2] (steering, accel).
 *   t2d_debug_closed_loop_*     n iterations of (that policy, t2d_step) per group enqueued by ONE host call -- launcher 0: from
 *                               the calling thread, round the groups step by step; 1: one host thread per group; 2: one captured
 *                               hipGraph per group holding graph_steps iterations, replayed (a replay rewrites the record-ring
 *                               slots of the capture: pick graph_steps = a multiple of T2D_RECORD_RING, or read T2D_F_STATUS /
 *                               T2D_F_REWARD).  create binds each pool's actions to its act_out_dev[g]; run returns when
 *                               everything is enqueued (t2d_sync / stream synchronisation waits for it); results are those of
 *                               the same policy and t2d_step calls on one pool holding all the envs. */
typedef struct t2d_closed_loop t2d_closed_loop;
int t2d_debug_feedback_policy(t2d_pool* pool, float* act_out_dev, float v_target, float k_speed, float k_steer, void* hip_stream);
int t2d_debug_closed_loop_create(t2d_pool* const* pools, void* const* hip_streams, float* const* act_out_dev, int32_t n_groups,
                                 int32_t interval_ms, int32_t launcher, int32_t graph_steps, t2d_closed_loop** out);
int t2d_debug_closed_loop_run(t2d_closed_loop* loop, int32_t n_steps);
int t2d_debug_closed_loop_destroy(t2d_closed_loop* loop);

/* ---- the device math primitives, one at a time (tactics2d_amd/csrc/t2d_math_probe.hip; tests/test_gpu_math.py) ------------------
 * Evaluates ONE function of tactics2d_amd/csrc/t2d_math.h over host arrays on device `device_id`, compiled with the product's
 * flags.  fn = T2D_MATH_*; a_host / b_host = n inputs each (b_host is read by the two-argument functions only and may be NULL
 * otherwise); out_host = outputs(fn) * n doubles, PLANAR: output j of element i at out_host[j * n + i].
 *     fn                  inputs                     outputs
 *     SINCOS              a = x                      sin, cos                       sincos_det
 *     SINCOS_SMALL        a = x, |x| <= 0.78         sin, cos                       sincos_det_small (no reduction)
 *     SINCOS_STEER        a = x                      sin, cos                       sincos_det_steer (wave-uniform shortcut)
 *     SINCOS_STEER_AND    a = steering, b = heading  sin a, cos a, sin b, cos b     sincos_det_steer_and
 *     TAN, ATAN           a = x                      one                            tan_det, atan_det
 *     ATAN2               a = y, b = x               one                            atan2_det
 *     MOD_TWO_PI, LOG, EXP  a = x                    one                            mod_two_pi, log_det, exp_det
 *     POW                 a = x, b = y               one                            pow_det(x, y)
 *     FRESNEL             a = x                      S, C                           fresnel_det (fn 12: 11 stays unassigned,
 *                                                                                   tests/test_gpu_math.py sends it as the unknown one)
 * Element i is computed by lane i % 64 of wave i / 64 in workgroups of 256, and the lanes past n leave before any wave-level
 * operation: the caller decides which inputs share a wave (the __ballot shortcuts of the steer variants).
 * table = 1 runs the same function compiled with T2D_TRIG_TABLE (constants from __constant__ tables, as t2d_collide.hip compiles
 * the header): SINCOS .. ATAN2 only.  Synchronous; uses the device's default stream.
 * Errors (the text: t2d_last_error(NULL)): T2D_ERR_INVALID for an unknown fn, table outside {0, 1} or = 1 for a function without
 * a table variant, n outside [1, T2D_MATH_MAX_N], a null array, an unknown device; T2D_ERR_HIP for a failing runtime call.   */
enum {
    T2D_MATH_SINCOS = 0, T2D_MATH_SINCOS_SMALL = 1, T2D_MATH_SINCOS_STEER = 2, T2D_MATH_SINCOS_STEER_AND = 3, T2D_MATH_TAN = 4,
    T2D_MATH_ATAN = 5, T2D_MATH_ATAN2 = 6, T2D_MATH_MOD_TWO_PI = 7, T2D_MATH_LOG = 8, T2D_MATH_EXP = 9, T2D_MATH_POW = 10,
    T2D_MATH_FRESNEL = 12
};
#define T2D_MATH_MAX_N 16777216
int t2d_debug_math(int32_t device_id, int32_t fn, int32_t table, int64_t n, const double* a_host, const double* b_host,
                   double* out_host);

/* ---- the step kernel's slot hand-out (wave_excl_scan, tactics2d_amd/csrc/t2d_collide.hip; tests/test_gpu_wave_scan.py) -----------
 * compact_and_process gives every lane of a wave its first queue slot as the exclusive prefix sum of the lanes' candidate counts,
 * computed in registers.  This runs that very function on n_waves waves, one per vector of 64 counts: cnt_host = int32
 * [n_waves][64] (lane l of wave w holds cnt_host[64 w + l]); off_host = int32 [n_waves][64], the sum of the lanes below; total_host
 * = int32 [n_waves], the sum of all 64.  Synchronous; uses the device's default stream.
 * Errors (the text: t2d_last_error(NULL)): T2D_ERR_INVALID for n_waves outside [1, T2D_WAVE_SCAN_MAX_WAVES], a null array, an
 * unknown device; T2D_ERR_HIP for a failing runtime call.                                                                     */
#define T2D_WAVE_SCAN_MAX_WAVES 65536
int t2d_debug_wave_scan(int32_t device_id, int32_t n_waves, const int32_t* cnt_host, int32_t* off_host, int32_t* total_host);

/* ---- the device geometry predicates, one at a time (tactics2d_amd/csrc/t2d_geom_probe.hip; tests/test_gpu_geom.py) --------------
 * Evaluates ONE predicate of tactics2d_amd/csrc/t2d_geom_dev.h over host arrays on device `device_id`, compiled with the product's
 * flags.  Everything is fp64, so that a test can place vertices closer to each other than fp32 poses allow, and PLANAR: component j
 * of element i at a_host[j * n + i] (b_host, out_host alike).  A quad is 8 components x0 y0 .. x3 y3, counter-clockwise; a triangle
 * repeats vertex 0 as its fourth (what load_quad_f32 does).  Integer results come back as doubles.
 *     fn                          a (components)       b (components)        outputs
 *     SAT_QUADS                   quad A (8)           quad B (8)            0 / 1                  sat_quads(A, B)
 *     RECT_PAIR_FILTER            rectangle A (8)      rectangle B (8)       0 / 1 / 2              rect_pair_filter(A, B)
 *     RECT_VS_CONVEX_FILTER       rectangle A (8)      convex B (8)          0 / 1 / 2              rect_vs_convex_filter(A, B)
 *     POINT_IN_QUAD               quad B (8)           point x y (2)         0 / 1                  point_in_quad(B, x, y)
 *     SEG_DIST2                   p q c (6)            -- (may be NULL)      the double             seg_dist2(p, q, c)
 *     PIECE_MEETS_QUAD_INTERIOR   quad P (8)           piece ax ay bx by (4) 0 / 1                  piece_meets_quad_interior(P, a, b)
 *     IOU_TERMS                   quad A (8)           quad B (8)            10: the eight clipped_edge_term values in the order
 *                                 quad_iou (t2d_collide.hip) forms and sums them -- s0..s3 = A's edges clipped to closed B (not
 *                                 strict), s4..s7 = B's edges clipped to A (strict), origin A[0] --, then quad_area2(A), quad_area2(B)
 * Element i is computed by lane i % 64 of wave i / 64 in workgroups of 256.  Synchronous; uses the device's default stream.  The
 * outputs are filled with 0xff bytes before the launch: an element the kernel did not write reads as that NaN.
 * Errors (the text: t2d_last_error(NULL)): T2D_ERR_INVALID for an unknown fn, n outside [1, T2D_GEOM_MAX_N], a null array (b_host of
 * SEG_DIST2 excepted), an unknown device; T2D_ERR_HIP for a failing runtime call.                                                  */
enum {
    T2D_GEOM_SAT_QUADS = 0, T2D_GEOM_RECT_PAIR_FILTER = 1, T2D_GEOM_RECT_VS_CONVEX_FILTER = 2, T2D_GEOM_POINT_IN_QUAD = 3,
    T2D_GEOM_SEG_DIST2 = 4, T2D_GEOM_PIECE_MEETS_QUAD_INTERIOR = 5, T2D_GEOM_IOU_TERMS = 6
};
#define T2D_GEOM_MAX_N 65536
int t2d_debug_geom(int32_t device_id, int32_t fn, int64_t n, const double* a_host, const double* b_host, double* out_host);

/* ---- memory bookkeeping (tactics2d_amd/csrc/t2d_devbuf.h; tests/test_gpu_lifetime.py) ------------------------------------------
 * What the library (this copy of it: every pool, trajectory and probe call of the process) holds right now: out = {device bytes,
 * device blocks, pinned host bytes, pinned host blocks}.  Every allocation of the library goes through one owning buffer type
 * that keeps these four counts, so a pool that is destroyed must bring them back to what they were before it was created.   */
int t2d_debug_memory(int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* T2D_DEBUG_H_ */
