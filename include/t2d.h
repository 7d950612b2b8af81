/*
 * t2d.h -- C ABI of libt2d_hip.so: the MI355X-native batched env.step() hot path
 * for tactics2d (physics integrators + collision / out-of-bound / off-lane events).
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain
 * pointers / ints / sizes, returns an int status (0 = T2D_OK) and never throws.
 * No torch types appear here; PyTorch only ever sees the raw device pointers
 * returned by t2d_get_field().
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * the tactics2d repository root, v0.1.9rc3):
 *
 *   t2d_set_param_table   <- SingleTrackKinematics.__init__  physics/single_track_kinematics.py:62-124
 *                            SingleTrackDynamics.__init__    physics/single_track_dynamics.py:58-138
 *                            PointMass.__init__              physics/point_mass.py:33-81
 *                            Vehicle/Cyclist/Pedestrian templates participant/element/participant_template.py:42-257
 *   t2d_reset             <- ParticipantBase.reset / Trajectory.add_state   participant/trajectory/trajectory.py:115-149
 *                            _ParkingScenarioManager.reset   envs/parking.py:397-441
 *   t2d_integrate         <- PhysicsModelBase.step           physics/physics_model_base.py:28
 *                            SingleTrackKinematics.step/_step physics/single_track_kinematics.py:126-198
 *                            SingleTrackDynamics.step/_step  physics/single_track_dynamics.py:140-251
 *                            PointMass.step/_step_newton     physics/point_mass.py:83-175,209-232
 *   t2d_set_static_geometry <- StaticCollision.reset         traffic/event_detection/collision.py:45-46
 *                            OutBound.reset                  traffic/event_detection/out_bound.py:50-65
 *   t2d_set_lane_geometry <- OffLane.reset                   traffic/event_detection/off_lane.py:19-20
 *   t2d_collide           <- Vehicle.get_pose                participant/element/vehicle.py:263-281
 *                            StaticCollision.update          traffic/event_detection/collision.py:37-43
 *                            DynamicCollision.update         traffic/event_detection/collision.py:18-25 (intended semantics)
 *                            OutBound.update                 traffic/event_detection/out_bound.py:37-48
 *                            OffLane.update                  traffic/event_detection/off_lane.py:16-17 (stub; build-defined:
 *                                                            not union(lane polygons).contains(pose), the predicate of
 *                                                            out_bound.py:37-48 applied to the lanes)
 *   t2d_snapshot/restore  <- ParkingEnv.reset / _ParkingScenarioManager.reset       envs/parking.py:262-298,397-441
 *   t2d_set_target_areas  <- Arrival.reset                traffic/event_detection/arrival.py:49-51
 *                            Arrival.update / NoAction.update (IoU)   arrival.py:32-47, no_action.py:32-53
 *   t2d_lidar_config/scan <- SingleLineLidar.__init__ / _scan_obstacles    sensor/lidar.py:33-57,128-221
 *   t2d_lidar_scan_all    <- the same scan bound to every participant (bind_id)  sensor/lidar.py:29,98-221
 *   t2d_check_status      <- _ParkingScenarioManager.check_status           envs/parking.py:361-392
 *   t2d_step              <- _ParkingScenarioManager.update + check_status  envs/parking.py:352-392
 *                            ParkingEnv.step terminated/truncated/reward    envs/parking.py:219-256,148-161
 *                            TimeExceed.update               traffic/event_detection/time_exceed.py:26-33
 *   t2d_traj_* /          <- Trajectory.add_state / get_state / history_states  participant/trajectory/trajectory.py:115-188
 *   t2d_verify_states        PhysicsModelBase.verify_states  physics/physics_model_base.py:53-73
 *                            ParticipantBase._verify_trajectory  participant/element/participant_base.py:120-131
 *   t2d_set_routes* /     <- OffRoute.reset / update             traffic/event_detection/off_route.py:24-51
 *   t2d_off_route            Trajectory.get_trace (trace routes)  participant/trajectory/trajectory.py:151-168
 *   t2d_dubins_paths /    <- Dubins.get_all_path / get_path / get_curve  interpolator/dubins.py:240-331
 *   t2d_curve_lines /        DubinsPath.get_curve_line :28-104; ReedsSheppPath.get_curve_line  interpolator/reeds_shepp.py:46-139
 *   t2d_curve_routes         Circle.get_arc  geometry/circle.py:106-139 (the curve written into the routes above)
 *   t2d_spline_curves /   <- Bezier.get_curve / BSpline.get_curve / CubicSpline.get_curve  interpolator/bezier.py, b_spline.py,
 *   t2d_spline_routes        cubic_spline.py over interpolator/cpp_interpolator/src/{bezier,b_spline,cubic_spline}.cpp
 *   t2d_grid_dijkstra     <- Dijkstra.plan / plan_graph  search/dijkstra.py:24-394 over grid_to_csr  search/graph_utils.py:10-150
 *   t2d_grid_astar        <- AStar.plan / plan_graph  search/a_star.py:23-404 over the same graph
 *   t2d_hybrid_astar      <- HybridAStar.plan  search/hybrid_a_star.py:58-172 with create_grid_collision_checker  tests/test_search.py:128-191
 *   t2d_sample_plan       <- RRT.plan  search/rrt.py:74-164; RRTStar.plan / _choose_parent  search/rrt_star.py:22-201;
 *                            RRTConnect.plan  search/rrt_connect.py:72-206, with the same collision checker
 *   t2d_prm_plan          <- PRM.plan  search/prm.py:52-344, with the same collision checker
 *   t2d_set_tracks /      <- _RacingScenarioManager._locate_agent / check_status  envs/racing.py:261-301, 339-369
 *   t2d_track_progress       RacingEnv._get_rewards                envs/racing.py:121-139
 *   t2d_generate_tracks / <- RacingTrackGenerator.generate         map/generator/generate_racing_track.py (random stream: build-defined)
 *   t2d_set_tracks_generated / t2d_tracks_regenerate   RacingEnv.reset: a new track per episode   envs/racing.py:374-383
 *   t2d_step_host         <- ParkingEnv.step as its caller sees it: host action in, host 5-tuple out
 *                            envs/parking.py:219-256, _get_infos / _get_relative_pose :190-217
 *
 * Threading: one host thread per pool.  t2d_integrate / t2d_collide / t2d_step are
 * asynchronous on the supplied hipStream_t (passed as void*; NULL = the null stream).
 * Nothing synchronises implicitly except t2d_download / t2d_upload / t2d_reset /
 * t2d_sync / the t2d_set_* calls (which copy from host memory), and those wait for THIS
 * pool's work only -- the streams it was launched on since the last such call plus its own
 * internal streams -- never for the whole device: other pools (env groups) and a policy
 * running on other streams keep going.
 *
 * Non-finite values.  The integrators follow the reference: np.clip(nan, lo, hi) is nan (single_track_kinematics.py:192-193),
 * np.clip(+-inf) the bound, np.mod(+-inf, 2 pi) nan -- a NaN action or state makes the participant's state NaN exactly where
 * numpy would (tests/golden/nonfinite.npz, made by importing the reference).  What the reference leaves to GEOS is BUILD-DEFINED
 * here: a participant whose pose (x, y or heading) is not finite takes no part in event detection -- its flags are 0 and nobody
 * collides with it --, its IoU events are not evaluated (T2D_F_IOU = NaN), as a lidar ego it sees nothing (+inf on every beam)
 * and as a lidar obstacle it is skipped; an IDM participant with a non-finite pose leads nobody (comparisons with NaN are
 * false).  Nothing hangs and no other participant's result changes (tests/test_gpu_nonfinite.py).  t2d_step_host rejects
 * non-finite actions when given an action box (T2D_ERR_ACTION), as `action_space.contains` does.
 *
 * Ownership: the pool owns every device buffer.  Host pointers passed in are read
 * during the call and never retained.  Device pointers handed out by t2d_get_field
 * stay valid until t2d_destroy.
 */
#ifndef T2D_H_
#define T2D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2D_ABI_VERSION 13

/* ---- status codes --------------------------------------------------------------- */
#define T2D_OK            0
#define T2D_ERR_INVALID   1   /* bad argument (null, out of range, inconsistent sizes)   */
#define T2D_ERR_HIP       2   /* a HIP runtime call failed; see t2d_last_error           */
#define T2D_ERR_NOMEM     3
#define T2D_ERR_STATE     4   /* call order violated (e.g. step before param table)      */
#define T2D_ERR_GEOMETRY  5   /* polygon not convex / degenerate / too many vertices     */
#define T2D_ERR_ACTION    6   /* t2d_step_host: an action outside the caller's action box (InvalidAction, envs/parking.py:235-236); nothing was stepped */

/* ---- physics model ids (column T2D_P_MODEL of a parameter row) --------------------- */
#define T2D_MODEL_KINEMATICS 0   /* SingleTrackKinematics */
#define T2D_MODEL_DYNAMICS   1   /* SingleTrackDynamics   */
#define T2D_MODEL_POINTMASS  2   /* PointMass, newton back-end */
#define T2D_MODEL_POINTMASS_EULER 4   /* PointMass, euler back-end (point_mass.py:177-207, backend="euler"): vx, vy AND heading are state
                                       * (the clipped speed is re-projected onto the previous sub-step's heading).  A rare,
                                       * selectable second back-end: integrated by the side kernel that also takes
                                       * T2D_MODEL_DRIFT (one launch ahead of the step launch; such pools are not chained) */
#define T2D_MODEL_DRIFT      3   /* SingleTrackDrift (Pacejka tyres, default Tire constants); extra state
                                  * T2D_F_OMEGA_F / T2D_F_OMEGA_R; integrated by its own kernel */
#define T2D_MODEL_REPLAY     5   /* no physics: the state at env time t is row t of a recorded trajectory (t2d_replay_bind);
                                  * the row carries shape, length and width only (the participant takes part in events, lidar
                                  * scans and leader searches); range, mass and sub-step columns are ignored.  Written by a
                                  * launch of its own ahead of the step launch, like T2D_MODEL_DRIFT (such pools are not chained) */

/* ---- shape kinds (column T2D_P_SHAPE) ---------------------------------------------- */
#define T2D_SHAPE_OBB    0   /* Vehicle / Cyclist / Other: length x width box             */
#define T2D_SHAPE_CIRCLE 1   /* Pedestrian: (centre, radius = width / 2)                  */

/* ---- parameter-table row: T2D_PARAM_COLS doubles per participant type ---------------
 * Ranges are ALREADY normalised by the host exactly like the reference constructors
 * (A.1 in SURVEY.md); an unbounded range has its bit cleared in T2D_P_RANGE_FLAGS.  */
enum {
    T2D_P_MODEL = 0,       /* T2D_MODEL_*                                   */
    T2D_P_LF = 1,
    T2D_P_LR = 2,
    T2D_P_WB = 3,          /* lf + lr, summed on the host like the reference */
    T2D_P_STEER_LO = 4,
    T2D_P_STEER_HI = 5,
    T2D_P_SPEED_LO = 6,
    T2D_P_SPEED_HI = 7,
    T2D_P_ACCEL_LO = 8,
    T2D_P_ACCEL_HI = 9,
    T2D_P_RANGE_FLAGS = 10, /* bit0 steer bounded, bit1 speed bounded, bit2 accel bounded */
    T2D_P_MASS = 11,
    T2D_P_MASS_HEIGHT = 12,
    T2D_P_MU = 13,
    T2D_P_IZ = 14,
    T2D_P_CF = 15,
    T2D_P_CR = 16,
    T2D_P_DELTA_T_MS = 17,  /* integer-valued: sub-step in ms (reference _DELTA_T = 5)  */
    T2D_P_SHAPE = 18,       /* T2D_SHAPE_*                                              */
    T2D_P_LENGTH = 19,      /* OBB length (m)                                           */
    T2D_P_WIDTH = 20,       /* OBB width (m); circle radius = width / 2                 */
    T2D_P_RESERVED0 = 21,
    T2D_P_RESERVED1 = 22,
    T2D_P_RESERVED2 = 23,
    T2D_PARAM_COLS = 24,
    /* T2D_MODEL_DRIFT rows reuse four columns the other models leave alone: */
    T2D_P_DRIFT_TSB = 15,    /* T_sb, brake-torque split   (single_track_drift.py:102) */
    T2D_P_DRIFT_TSE = 16,    /* T_se, engine-torque split  (:103)                      */
    T2D_P_DRIFT_RADIUS = 22, /* effective wheel radius (m) (:101)                      */
    T2D_P_DRIFT_IYW = 23,    /* wheel inertia I_yw         (:106)                      */
    /* ... and rows of the other models carry two DERIVED values there, written by the library (whatever the caller put
     * into the reserved columns is ignored): */
    T2D_P_DT_S = 22,         /* (double)delta_t_ms / 1000: the Euler sub-step in seconds (_step's `dt`)            */
    T2D_P_SUBSTEPS = 23      /* (interval_ms / delta_t_ms) * 65536 + interval_ms % delta_t_ms for the interval of the
                              * launch in flight (a 32-thread kernel refreshes it when the interval changes)        */
};
#define T2D_RANGE_STEER 1
#define T2D_RANGE_SPEED 2
#define T2D_RANGE_ACCEL 4
#define T2D_MAX_TYPES 32

/* ---- pool fields (t2d_get_field / t2d_download / t2d_upload) ------------------------
 * Per-participant fields hold N = n_env * max_agents elements, env-major
 * (index = env * max_agents + agent).  Per-env fields hold n_env elements.         */
enum {
    T2D_F_X = 0,        /* f32[N]  env-local x (m)                                   */
    T2D_F_Y = 1,        /* f32[N]                                                    */
    T2D_F_HEADING = 2,  /* f32[N]  stored heading, np.mod(phi, 2*pi)                 */
    T2D_F_SPEED = 3,    /* f32[N]  signed scalar speed                               */
    T2D_F_VX = 4,       /* f32[N]  written by kinematics / point-mass only           */
    T2D_F_VY = 5,       /* f32[N]                                                    */
    T2D_F_ACT0 = 6,     /* f32[N]  accel (vehicles) | ax (point mass)                */
    T2D_F_ACT1 = 7,     /* f32[N]  steer (vehicles) | ay (point mass)                */
    T2D_F_IDS = 8,      /* u32[N]  model_id | type_id<<8 | active<<16                */
    T2D_F_FLAGS = 9,    /* u32[N]  event bits, see T2D_FLAG_*                        */
    T2D_F_APPLIED0 = 10,/* f32[N]  clipped accel actually applied (State.accel)      */
    T2D_F_APPLIED1 = 11,/* f32[N]  clipped steer actually applied                    */
    T2D_F_ENV_FLAGS = 12,  /* u32[E]  OR of the participants' flags                  */
    T2D_F_CNT_STEP = 13,   /* i32[E]  ScenarioManager.cnt_step                       */
    T2D_F_FRAME_MS = 14,   /* i32[E]  State.frame of the env (ms)                    */
    T2D_F_STATUS = 15,     /* u8[E*4] scenario_status, traffic_status, terminated, truncated */
    T2D_F_REWARD = 16,     /* f32[E]                                                  */
    T2D_F_RECORD = 17,     /* u32[T2D_RECORD_RING][E][2] packed per-env result records {reward bits, status
                              word}, a ring: t2d_step number k (0-based since create) writes slot
                              k % T2D_RECORD_RING, so a collective can ship the records of the last K
                              steps in one message while the following steps already run          */
    T2D_F_IOU = 18,        /* f32[E]  IoU(ego pose, target) of the last step; NaN = not evaluated (None) */
    T2D_F_CNT_NO_ACTION = 19, /* i32[E] NoAction.cnt_no_action                          */
    T2D_F_LIDAR = 20,      /* f32[E][n_beams] last t2d_lidar_scan into the pool's own buffer (size set by
                              t2d_lidar_config; +inf = no return)                                 */
    T2D_F_LEADER = 21,     /* i32[N]  agent index (inside the env) of the IDM leader chosen by the last
                            *         t2d_idm_actions, -1 = none / participant not IDM-controlled   */
    T2D_F_OMEGA_F = 22,    /* f32[N]  SingleTrackDrift front wheel angular speed (rad/s); 0 after t2d_reset */
    T2D_F_OMEGA_R = 23,    /* f32[N]  rear wheel                                                        */
    T2D_F_COUNT = 24
};

/* ---- per-participant / per-env event bits ------------------------------------------- */
#define T2D_FLAG_COLLISION_DYNAMIC 1u   /* OBB/circle intersects another active participant */
#define T2D_FLAG_COLLISION_STATIC  2u   /* intersects a static polygon (StaticCollision)    */
#define T2D_FLAG_OUT_BOUND         4u   /* not boundary.contains(pose)  (OutBound)          */
#define T2D_FLAG_OFF_LANE          8u   /* not union(lanes).contains(pose); build-defined, DESIGN.md */

/* ---- ScenarioStatus / TrafficStatus values: traffic/status.py:10-61 ----------------- */
#define T2D_TRAFFIC_NO_ACTION_QUIRK 5  /* parking.py:373 stores ScenarioStatus.NO_ACTION (5) in traffic_status */
#define T2D_SCENARIO_NORMAL        1
#define T2D_SCENARIO_COMPLETED     2
#define T2D_SCENARIO_TIME_EXCEEDED 3
#define T2D_SCENARIO_OUT_BOUND     4
#define T2D_SCENARIO_NO_ACTION     5
#define T2D_SCENARIO_FAILED        6
#define T2D_TRAFFIC_NORMAL            1
#define T2D_TRAFFIC_COLLISION_STATIC  3
#define T2D_TRAFFIC_COLLISION_DYNAMIC 4
#define T2D_TRAFFIC_OFF_LANE          6

/* ---- geometry limits ----------------------------------------------------------------- */
#define T2D_MAX_POLY_VERTS 8      /* static / lane polygons: convex, 3..8 vertices (5..8: evaluated as a fan of quads) */
#define T2D_RECORD_RING 64      /* slots of the per-env result-record ring (T2D_F_RECORD): two gather fragments of 32 steps */
#define T2D_MAX_AGENTS 256        /* participants per env                                 */

/* ---- status / reward configuration (t2d_set_status_config) --------------------------- */
typedef struct t2d_status_config {
    int32_t max_step;            /* TimeExceed.max_step; <= 0 disables (time_exceed.py:20) */
    int32_t ego_index;           /* agent whose flags drive the env status (0)            */
    int32_t check_dynamic;       /* include participant-participant collision in status   */
    int32_t check_off_lane;      /* include build-defined off-lane in status              */
    float reward_collision;      /* -5  envs/parking.py:151-152                           */
    float reward_time_exceed;    /* -1  envs/parking.py:153-157                           */
    float reward_out_bound;      /* -5  envs/parking.py:158-159                           */
    float reward_completed;      /* +5  envs/parking.py:160-161                           */
    float time_penalty_scale;    /* 0.001: -tanh(cnt_step / max_step) * scale  :163       */
    /* ---- IoU events of the ego (scope rows f1), all off by default ------------------------- */
    int32_t check_arrival;       /* Arrival.update arrival.py:32-47: IoU(pose, target) >= threshold
                                    -> COMPLETED (needs t2d_set_target_areas)               */
    int32_t check_no_action;     /* NoAction.update no_action.py:32-53: IoU(pose, last pose) >
                                    no_action_iou on more than no_action_max_step checks    */
    int32_t no_action_max_step;  /* 100  envs/parking.py:344                                   */
    int32_t shaped_reward;       /* IoU gain + distance-to-target gain of _get_reward :163-188 */
    float arrival_threshold;     /* 0.95  arrival.py:22                                        */
    float no_action_iou;         /* 0.999 no_action.py:47                                      */
    float dist_reward_scale;     /* 0.1   envs/parking.py:187                                  */
} t2d_status_config;

typedef struct t2d_pool t2d_pool;

/* Error text of the most recent failing call on this pool (owned by the pool), or of the
 * most recent failing t2d_create when pool == NULL (thread-local).                      */
const char* t2d_last_error(const t2d_pool* pool);
int t2d_abi_version(void);

/* Create a pool of n_env environments x max_agents participants on HIP device device_id.
 * All state starts zeroed and inactive.                                                  */
int t2d_create(int32_t n_env, int32_t max_agents, int32_t device_id, t2d_pool** out_pool);
int t2d_destroy(t2d_pool* pool);

/* rows: n_types rows of row_stride doubles (row_stride >= T2D_PARAM_COLS), host memory.  */
int t2d_set_param_table(t2d_pool* pool, const double* rows, int32_t n_types, int32_t row_stride);

/* Static obstacle polygons + map boundary, CSR, host memory, env-local fp32 coordinates.
 *   env_poly_offsets  [n_env + 1]  polygons of env e are [off[e], off[e+1])
 *   poly_vert_offsets [n_poly + 1] vertices of polygon p are [off[p], off[p+1])
 *   verts_xy          [2 * n_vert] interleaved x,y
 *   boundary          [4 * n_env]  xmin, xmax, ymin, ymax (OutBound tuple order) or NULL
 *   boundary_valid    [n_env]      0 = "boundary is None" -> never out of bound; NULL = all valid
 * Polygons must be convex with 3..T2D_MAX_POLY_VERTS vertices; either winding accepted.  A polygon of
 * 5..8 vertices is evaluated as its fan of quads (v0 v1 v2 v3), (v0 v3 v4 v5), (v0 v5 v6 v7): the union is the
 * polygon, `intersects` is the OR over the parts; the lidar scans the undivided ring.
 * Size: the step kernels keep the static + lane parts of one workgroup's envs in ONE packed LDS record of at most 32 KiB
 * (t2d_geometry_budget says what a scene needs).  A scene beyond that -- a reference map of hundreds of lanelets,
 * map/element/map.py:242-329 answers its proximity queries with an STRtree -- is NOT refused: t2d_set_static_geometry /
 * t2d_set_lane_geometry keep its parts in global memory behind one uniform grid per env (the HBM grid tier,
 * tactics2d_amd/csrc/t2d_mapgrid.hip), and t2d_step / t2d_step_n run as t2d_integrate -> a map-events launch -> the event + status
 * launch (t2d_step_form: T2D_FORM_UNFUSED): the same flags, statuses and rewards at any map size, about three launches per step
 * instead of one.  (Not for generated parking scenes: their capacity layout is fixed.)              */
int t2d_set_static_geometry(t2d_pool* pool, const int32_t* env_poly_offsets,
                            const int32_t* poly_vert_offsets, const float* verts_xy,
                            const float* boundary, const uint8_t* boundary_valid);

/* Lane polygons for the build-defined off-lane flag; same CSR convention.  Envs with no
 * lane polygons never raise T2D_FLAG_OFF_LANE (== the reference stub).  The flag is
 * `not union(lanes).contains(pose)`: the boundary of the union of each env's lanes is extracted
 * here, once (lanes that abut must share their vertices exactly, or overlap: a sliver between two
 * almost-collinear edges is a real gap of the union).                                      */
int t2d_set_lane_geometry(t2d_pool* pool, const int32_t* env_lane_offsets,
                          const int32_t* lane_vert_offsets, const float* verts_xy);

int t2d_set_status_config(t2d_pool* pool, const t2d_status_config* cfg);

/* Target parking areas for Arrival and the reward shaping (Arrival.reset arrival.py:49-51,
 * _ParkingScenarioManager.target_area envs/parking.py:399-401): one quadrilateral per env,
 * target_xy[n_env][4][2] fp32 (either winding, convex); centroid[n_env][2] = its area centroid
 * (`target_area.geometry.centroid`) or NULL to have it computed.  NULL target_xy removes them.
 * Host memory.  (Re)initialises the per-env min-distance-to-target from the current state.    */
int t2d_set_target_areas(t2d_pool* pool, const float* target_xy, const float* centroid);

/* (Re)initialise participants.  All arrays are host memory with N = n_env*max_agents
 * elements; env_mask (n_env bytes, NULL = every env) selects which envs are written.
 * vx / vy may be NULL (then vx = speed*cos(heading), vy = speed*sin(heading) in fp64,
 * rounded to fp32 -- State.velocity, participant/trajectory/state.py:152-169).
 * Resets cnt_step, frame, status, reward and flags of the selected envs.                */
int t2d_reset(t2d_pool* pool, const uint8_t* env_mask, const float* x, const float* y,
              const float* heading, const float* speed, const float* vx, const float* vy,
              const uint8_t* type_id, const uint8_t* active);

/* Zero-copy actions: make the integrator read ACT0/ACT1 from caller-owned DEVICE memory (e.g. a
 * policy's output tensor, N floats each) instead of the pool's own buffers.  NULL, NULL rebinds
 * the pool's buffers.  The caller keeps the memory alive and orders its writes on the stream;
 * the library only ever READS it (IDM-controlled participants take their action from the pool's
 * own ACT0/ACT1 fields, where t2d_idm_actions writes).  t2d_upload of ACT0 / ACT1 ends a binding:
 * uploaded actions are the actions from then on.                                                */
int t2d_bind_actions(t2d_pool* pool, const float* act0_dev, const float* act1_dev);
/* The same with a stride: participant i's actions are act0_dev[i * stride] and act1_dev[i * stride] (stride in
 * elements, >= 1).  A policy's [N, 2] output in the reference's (steering, accel) layout (envs/parking.py:130-139)
 * binds as act0 = out + 1, act1 = out, stride = 2 -- no copy kernels between the policy and the step.              */
int t2d_bind_actions_strided(t2d_pool* pool, const float* act0_dev, const float* act1_dev, int32_t stride);
/* Optional guard for bound memory: n_elements = how many float elements may be read from act0_dev and from act1_dev (0 = not
 * declared, the default after every t2d_bind_actions[_strided]; the library cannot see the size of caller-owned memory).  With a
 * declared extent, t2d_step_n refuses (T2D_ERR_INVALID) a fragment whose last step would read beyond it -- participant N - 1 of
 * step n_steps - 1 reads element (N - 1) * stride + (n_steps - 1) * act_step_stride -- instead of faulting on the device.
 * T2D_ERR_STATE while the pool reads its own ACT0 / ACT1 fields; T2D_ERR_INVALID if one action set does not fit.
 * (The reference has no counterpart: its actions are Python tuples, envs/parking.py:239.)                                      */
int t2d_set_action_extent(t2d_pool* pool, int64_t n_elements);

/* Physics only: one PhysicsModelBase.step(interval_ms) for every active participant,
 * actions taken from fields ACT0/ACT1.                                                  */
int t2d_integrate(t2d_pool* pool, int32_t interval_ms, void* hip_stream);
#define T2D_MAX_INTERVAL_MS 32767   /* interval_ms of every stepping call: 1 .. 32767 (the sub-step count travels in 15 bits) */
/* Events only: recompute FLAGS / ENV_FLAGS from the current poses.                      */
int t2d_collide(t2d_pool* pool, void* hip_stream);
/* ScenarioManager.check_status alone (envs/parking.py:361-392): events + the status / reward /
 * counter epilogue on the current poses (what t2d_step runs after the integrator).         */
int t2d_check_status(t2d_pool* pool, int32_t interval_ms, void* hip_stream);
/* ScenarioManager.update + check_status: integrate, collide, status/reward epilogue.  By default
 * ONE fused launch (the participant is integrated in registers and its new pose feeds the event
 * phases directly); t2d_set_fused_step(pool, 0) selects the two-kernel form, whose results are
 * bit-identical.  kernel_id 2 of t2d_profile_read times the fused launch.                   */
int t2d_step(t2d_pool* pool, int32_t interval_ms, void* hip_stream);
int t2d_set_fused_step(t2d_pool* pool, int32_t on);
/* Pools with ONE participant per env (ParkingEnv, BASELINE config 2) whose parameter table holds box-shaped types only
 * and that have no lane geometry take their fused step with one WAVE per env instead of one lane per participant (the
 * quads of the lot, the constraints of the two IoUs spread over the wave's lanes: ~2.5x faster at 4096 envs).  Same
 * arithmetic, same results bit for bit -- with ONE exception: the single-ego kernel always ITERATES a kinematic step, so on
 * pools large enough for the general kernel to resum it (integrator variant 1 at >= 131072 participants on an MI355X, or
 * variant 3: t2d_set_integrator_variant) the two agree to the series' truncation (< 1e-9 m; the last bit of the fp32 state may
 * differ), and bit for bit again under variants 0 and 2.  On by default, t2d_set_ego_kernel(pool, 0) keeps the pool on the
 * general kernel. */
int t2d_set_ego_kernel(t2d_pool* pool, int32_t on);
/* One step of n pools in a single call -- env groups on separate streams (independent environments cut into
 * groups whose launches overlap: one group's start-up latency and tail hide behind the others' busy middle,
 * DESIGN.md "Env groups").  For i in [0, n): if act0 / act1 are non-NULL, t2d_bind_actions(pools[i],
 * act0[i], act1[i]); then t2d_step(pools[i], interval_ms, hip_streams[i]).  Exists because at ~6 us of GPU
 * time per group and step, one host call per pool and per step is what limits the rate.  With n > 1 the step
 * kernels are also told that launches overlap, which turns their wave priorities round (a launch that has the GPU
 * to itself serves the waves that are behind first, overlapping launches the waves that are about to retire:
 * DESIGN.md 4.2); pools stepped on different streams through separate t2d_step calls keep the single-launch rule.
 * Returns the first error (its message is on that pool).                                                 */
int t2d_step_groups(t2d_pool* const* pools, const float* const* act0_dev, const float* const* act1_dev,
                    void* const* hip_streams, int32_t n, int32_t interval_ms);

/* n_steps consecutive t2d_step's enqueued by ONE call -- a rollout fragment on resident actions (the loop of
 * envs/parking.py:219-256 without a host round trip per step).  Step k reads participant i's action at
 * act[i * stride + k * act_step_stride] of the bound (or the pool's own) action arrays: act_step_stride = 0 repeats one
 * action set (frame skip), n_env * max_agents * stride walks an action ring laid out [n_steps][N].  Results are exactly
 * those of n_steps t2d_step calls; per-step rewards / statuses are in the record ring (T2D_F_RECORD), the participant
 * fields hold the last step's values.
 * How: pools whose step is the fused kernel alone (no drift / regenerated scenes; installed IDM controllers are run by the
 * step launch itself, here as in t2d_step, for envs of 2..64 participants) get ONE launch
 * holding all the steps.  Large pools: workgroup (g, k) takes step k of the envs of workgroup g and is ordered after workgroup
 * (g, k - 1) by a per-workgroup word in device memory (kept inside one XCD's L2, the placement checked: DESIGN.md 4.10) -- no
 * launch boundary between steps, so the start-up of step k + 1 overlaps the tail of step k.  Small pools: every workgroup
 * loops over the steps itself, and where a step's workgroups number at most the device's CUs a second set of waves per
 * workgroup integrates step k + 1 while the first checks the events of step k (t2d_step_form tells which).
 * Failure (never observed; forced by tests with t2d_debug_chain_fault): every wait is bounded, and a chained hand-off checks
 * that producer and consumer share an XCD.  A workgroup whose hand-off fails records the failure and goes on (never a hang):
 * what it and everything enqueued behind it on the device computes from then on -- state, flags, records, a t2d_gather of those
 * records, a lidar scan -- is INVALID until the host has noticed: the first t2d_sync / t2d_download / t2d_step_n after it
 * returns T2D_ERR_STATE -- once -- and the pool goes on with ordinary launches (t2d_set_step_chaining re-enables chaining).
 * CHAIN forms: the pool has then been rolled back to the state and step count (t2d_step_count) it had when the failed fragment
 * began -- every chained fragment checkpoints what it starts from -- so the caller re-issues its steps from there; the pure
 * outputs (flags, status, reward, records, vx / vy of the single-track models, the applied action) are rewritten by the next step.  LOOP forms (a wait inside a workgroup ran out): the state is
 * undefined, t2d_reset / t2d_restore(mode 0) / uploads make the pool usable again.
 * act_step_stride > 0 needs an action ring bound with t2d_bind_actions[_strided] (n_steps * act_step_stride elements beyond
 * the last participant's first action); the pool's own ACT0 / ACT1 fields hold one set: T2D_ERR_INVALID otherwise.
 * Other pools, and every pool after
 * t2d_set_step_chaining(pool, 0, *), take n_steps ordinary launches -- and t2d_step its plainest form: installed IDM
 * controllers as a launch of their own (on = 1: automatic, the default; 2 / 3 / 4 pin the chained
 * form / the plain loop / the loop with integrator but without lane waves -- measurements and tests).  priority_rule: wave priorities inside a chained launch
 * (1, default: the rule for overlapping work; 0: the single-launch rule).  kernel_id 7 in t2d_profile_read
 * (one "launch" = one chained launch of up to T2D_RECORD_RING steps).                                                    */
int t2d_step_n(t2d_pool* pool, int32_t interval_ms, int32_t n_steps, int64_t act_step_stride, void* hip_stream);
int t2d_set_step_chaining(t2d_pool* pool, int32_t on, int32_t priority_rule);
/* Small pools of envs with 33..64 participants (at most 4 x the device's CUs envs, no IoU events): the fused step gives every
 * env a workgroup of its own and runs its event stages on four waves side by side (pairs / static polygons / two halves of the
 * lane polygons) instead of one wave walking through all of them -- same arithmetic, same results, a shorter dependent
 * chain per env.  Only pools whose envs carry static obstacles AND lanes take it (a pool with nothing to run side by side is
 * slower that way).  On by default (t2d_step and t2d_step_n alike); 0 keeps one wave per env.                              */
int t2d_set_split_step(t2d_pool* pool, int32_t on);
/* Which form of the step kernel a call with n_steps steps takes on this pool now (diagnostics, tests, bench lines):        */
enum {
    T2D_FORM_UNFUSED = 0,     /* separate integrate + check_status launches, or helper kernels around the fused step */
    T2D_FORM_STEP = 1,        /* one fused launch per step, one wave per env (or per 2..64 small envs)                 */
    T2D_FORM_STEP_SPLIT = 2,  /* one fused launch per step, one workgroup per env                                      */
    T2D_FORM_EGO = 3,         /* single-ego kernel, one launch per step                                                */
    T2D_FORM_EGO_LOOP = 4,    /* single-ego kernel, the lanes loop over the steps                                      */
    T2D_FORM_CHAIN = 5,       /* one launch of (workgroup, step) workgroups ordered by counters                        */
    T2D_FORM_CHAIN_SPLIT = 6, /* the same with one workgroup per env                                                   */
    T2D_FORM_LOOP = 7,        /* resident workgroups loop over the steps                                               */
    T2D_FORM_LOOP_PIPE = 8,   /* ... with integrator waves running one step ahead of the event waves                   */
    T2D_FORM_EGO_LOOP_PIPE = 9 /* the single-ego kernel's loop with integrator waves                                  */
};
int t2d_step_form(t2d_pool* pool, int32_t n_steps);   /* a T2D_FORM_* value; -1: null pool */

/* Zero-copy device pointer of a field (for wrapping as a torch tensor).                 */
int t2d_get_field(t2d_pool* pool, int32_t field_id, void** dev_ptr, size_t* nbytes);
/* Synchronous host<->device copies of a whole field (parity tests, small envs).         */
int t2d_download(t2d_pool* pool, int32_t field_id, void* host_dst, size_t nbytes);
int t2d_upload(t2d_pool* pool, int32_t field_id, const void* host_src, size_t nbytes);
/* Waits for THIS pool's work only: the streams it was launched on since the last such call (up to four are tracked; more
 * distinct streams, or a tracked stream that has been destroyed in the meantime, make the call fall back to a device-wide
 * synchronise) plus the pool's own internal streams.  The set-up calls and the two copies above wait the same way.       */
int t2d_sync(t2d_pool* pool);

/* ---- the Gym-API host path: host actions in, ONE packed host frame out ------------------------------------------------
 * What the reference's caller gets from ParkingEnv.step (envs/parking.py:219-256) is host values: the observation, the reward,
 * terminated / truncated and the info dict of _get_infos (:203-217: lidar, state, target area / heading, the two statuses and
 * the relative pose of _get_relative_pose :190-201).  t2d_step_host is that call for every env of the pool: it takes the
 * actions from HOST memory, runs t2d_step (and, when the frame carries a lidar section, t2d_lidar_scan writing straight into
 * the frame), packs everything the 5-tuple needs of the ego of every env into one contiguous FRAME and brings it to pinned host
 * memory with one asynchronous copy and one stream synchronisation -- instead of one blocking copy per field.
 *   t2d_frame_config   chooses the sections (T2D_FRAME_*), allocates the device frame and n_host_frames (1..T2D_MAX_HOST_FRAMES)
 *                      pinned host frames, and fills
 *                      *layout with the byte offsets of the sections inside a frame (-1 = section absent).  Asking for the
 *                      configuration already in place keeps the frames (and what a caller still holds of them); a DIFFERENT one
 *                      frees them: views of earlier frames are invalid from then on, as after t2d_destroy, and a pool whose
 *                      actions are the ones t2d_step_host last staged reads its OWN action fields (T2D_F_ACT0 / ACT1) again
 *                      until the next t2d_step_host / t2d_bind_actions / upload.  Call it again after
 *                      t2d_lidar_config changed the beam count.  T2D_FRAME_ZEROCOPY: no copy commands at all -- the step kernel
 *                      reads the actions from mapped host memory and the pack / lidar kernels write the mapped host frame
 *                      (lowest latency for small pools; a large pool's 8 B per participant would cross PCIe inside the step).
 *   t2d_set_target_headings  target_heading of every env (envs/parking.py:401), host fp64 [n_env]; generated scenes
 *                      (t2d_parking_scenes) bring their own.  Without it diff_heading is NaN.
 *   t2d_step_host      actions_host = f32 [n_env * max_agents][2] in the reference's action layout (steering, accel)
 *                      (envs/parking.py:239; a point mass: (ay, ax)), or NULL = the actions already in / bound to the pool.
 *                      Ends any t2d_bind_actions binding (the pool reads a buffer of its own from then on).  Returns with
 *                      *frame_host pointing at the filled host frame: frame_index (0 .. n_host_frames - 1) names the pinned
 *                      frame to fill -- a caller that hands the frame's memory on (numpy views) picks one nobody holds any
 *                      more, and no copy is needed -- or -1 = the frames in turn.  Reports a failed scene regeneration like
 *                      t2d_sync does.
 *                      action_box = {steering lo, steering hi, accel lo, accel hi} or NULL: `action_space.contains(action)`
 *                      of envs/parking.py:235-236 for every row, checked while the actions are staged (closed bounds, a NaN
 *                      is outside) -- T2D_ERR_ACTION, nothing stepped AND nothing staged (the verdict precedes the copy: the
 *                      actions of the last accepted call stay in place), the message names the first offending row.
 *   t2d_host_action_buffer  the pool's own pinned staging buffer, f32 [n_env * max_agents][2] (valid until the next
 *                      t2d_frame_config): a caller that writes its actions THERE and passes that pointer to t2d_step_host saves the
 *                      staging copy (2 MB per step at 4096 x 64: ~ 70 us of host memcpy); the box check still reads every row.
 *   t2d_frame_fetch    the frame of the CURRENT state without stepping (what reset() returns; the lidar section is scanned
 *                      from the current poses).
 * Frame sections (E = n_env; every offset a multiple of 256 B):
 *   header     u32 [16]: {step count (low half), scene-regeneration error word, 0 ...}
 *   obs        f32 [E][6]   x, y, heading, speed, vx, vy of the ego (vx / vy as stored: see T2D_F_VX)
 *   rel        f64 [E][3]   diff_position, diff_angle, diff_heading of _get_relative_pose: |centroid - (x, y)|,
 *                           atan2(cy - y, cx - x) - heading, target_heading - heading, in fp64 from the stored fp32 state
 *                           (NaN without target areas / headings)
 *   reward     f32 [E]      status  u8 [E][4]   iou f32 [E]   frame_ms i32 [E]   cnt_step i32 [E]
 *   episode    i32 [E]      generated scenes: episode number of the env (0 otherwise)
 *   target     f32 [E][8] + f64 [E] target_heading   (T2D_FRAME_TARGET: the target area the env is in NOW; generated scenes)
 *   lidar      f32 [E][n_beams]                      (T2D_FRAME_LIDAR)                                                      */
#define T2D_FRAME_LIDAR    1u
#define T2D_FRAME_TARGET   2u
#define T2D_FRAME_ZEROCOPY 4u
#define T2D_MAX_HOST_FRAMES 16
typedef struct t2d_frame_layout {
    int64_t bytes;          /* size of one frame */
    int64_t off_obs, off_rel, off_reward, off_status, off_iou, off_frame_ms, off_cnt_step, off_episode;
    int64_t off_target, off_target_heading, off_lidar;   /* -1 = absent */
    int32_t n_env, n_beams;
} t2d_frame_layout;
int t2d_frame_config(t2d_pool* pool, uint32_t sections, int32_t n_host_frames, t2d_frame_layout* layout);
int t2d_set_target_headings(t2d_pool* pool, const double* heading_host);
int t2d_step_host(t2d_pool* pool, const float* actions_host, const float* action_box, int32_t interval_ms, void* hip_stream,
                  int32_t frame_index, const void** frame_host);
int t2d_frame_fetch(t2d_pool* pool, void* hip_stream, int32_t frame_index, const void** frame_host);
int t2d_host_action_buffer(t2d_pool* pool, float** actions_host);

/* Episode-start snapshot for device-side (auto-)reset -- the vector-env counterpart of
 * ParkingEnv.reset (envs/parking.py:262-298) without a host round trip.
 * t2d_snapshot copies the current participant state (x, y, heading, speed, vx, vy, ids) into a
 * pool-owned device snapshot.  t2d_restore (asynchronous on the stream) writes it back and
 * clears cnt_step / frame / status / reward / flags:
 *   mode 0: every env;  mode 1: only envs whose status says terminated or truncated.       */
int t2d_snapshot(t2d_pool* pool);
int t2d_restore(t2d_pool* pool, int32_t mode, void* hip_stream);
/* Vector-env auto-reset fused into t2d_step: an env whose status comes out terminated or truncated
 * is put back to the snapshot at the end of the same launch (state, ids, cnt_step, frame).  Its
 * status / reward / flags keep the terminal step's values until the next step overwrites them, as
 * Gym vector envs report them.  Needs a snapshot.                                                */
int t2d_set_auto_reset(t2d_pool* pool, int32_t on);

/* Single-line lidar of the ego of every env (SingleLineLidar, sensor/lidar.py:33-221, as configured by
 * ParkingEnv envs/parking.py:303-304,422-431: 360 beams, 20 m): distance to the nearest obstacle edge
 * along n_beams rays at angles linspace(0, 2 pi, n_beams, endpoint=False) in the ego frame; +inf = no
 * return.  Obstacles = the static polygons of t2d_set_static_geometry and, when include_participants,
 * the boxes of the other active participants.  beam_sin / beam_cos: host arrays [n_beams] with the sin /
 * cos of those angles (numpy), or NULL to have the library compute them with libm.
 * t2d_lidar_scan writes fp32 [n_env][n_beams] to out_dev (caller-owned device memory, e.g. the policy's
 * observation tensor) or, when NULL, to the pool's T2D_F_LIDAR buffer.  kernel_id 3 in t2d_profile_read.
 * The scan of every participant instead of the ego alone: t2d_lidar_scan_all below.                     */
int t2d_lidar_config(t2d_pool* pool, int32_t n_beams, float max_range, int32_t include_participants,
                     const double* beam_sin, const double* beam_cos);
int t2d_lidar_scan(t2d_pool* pool, float* out_dev, void* hip_stream);

/* The same scan with EVERY participant of every env as the sensor, in one launch (SingleLineLidar bound to any
 * participant: sensor/lidar.py:29 `bind_id`, :98-126 the rings in that participant's frame, :128-221 the scan).
 * Row (e, j) is what t2d_lidar_scan gives for env e with status_config.ego_index = j, bit for bit: obstacles =
 * the static polygons and, when include_participants, the boxes of the OTHER active participants (k != j).
 * Rows of inactive participants and of participants whose x, y or heading is not finite are all +inf; a
 * circle-shaped participant (pedestrian) is a sensor like any other and, as above, no obstacle.
 * Uses the configuration of t2d_lidar_config (beams, range, include_participants, beam tables); ignores
 * status_config.ego_index and never touches the status configuration.
 * t2d_lidar_scan_all writes fp32 [n_env][max_agents][n_beams] to out_dev (caller-owned device memory, e.g. a
 * multi-agent policy's observation tensor) or, when NULL, to a buffer of the pool's own, allocated on first
 * use and again after t2d_lidar_config changed the beam count.  One launch, asynchronous on hip_stream, no
 * host synchronisation: enqueued behind t2d_step / t2d_step_n on the same stream it sees that step's poses.
 * T2D_ERR_STATE / T2D_ERR_GEOMETRY as t2d_lidar_scan.  kernel_id 8 in t2d_profile_read.
 * t2d_lidar_all_buffer: pointer and size (n_env * max_agents * n_beams * 4 bytes) of the pool's own buffer;
 * T2D_ERR_STATE before the first NULL-destination scan (and after a new beam count until the next one). */
int t2d_lidar_scan_all(t2d_pool* pool, float* out_dev, void* hip_stream);
int t2d_lidar_all_buffer(t2d_pool* pool, void** dev_ptr, size_t* nbytes);

/* On-device scripted agents: IDM car following (IDMController, controller/idm_controller.py:33-157).
 * ctrl_rows: host array [n_ctrl][row_stride >= T2D_IDM_COLS] of fp64 parameter sets -- the constructor
 * arguments of idm_controller.py:33-57 (`configure` :143-157 = calling t2d_set_idm again) plus the two
 * columns of the build-defined leader rule; ctrl_id: host array [n_env * max_agents], index of the
 * participant's parameter set or T2D_IDM_NONE (its action stays whatever the caller supplied).
 * A refused call changes nothing in the pool (the three t2d_set_* of the scripted agents share one order: host arguments,
 * quiesce, the pool's state, new device memory, and only then the exchange).  n_ctrl = 0 uninstalls and frees the installation's
 * device memory.  t2d_idm_actions = IDMController.step :59-93 for every controlled participant:
 * acceleration (np.clip-ed to [-comfortable_deceleration, max_acceleration]) -> the pool's T2D_F_ACT0, steering
 * 0.0 -> T2D_F_ACT1 (always the pool's own fields: memory bound with t2d_bind_actions is never written; controlled
 * participants are integrated from the pool's fields, the others from the bound memory), leader index ->
 * T2D_F_LEADER.  The reference takes `leading_state` from its caller; here the leader is the nearest active
 * participant ahead (0 < longitudinal offset <= horizon along the own heading) inside the own corridor
 * (|lateral offset| <= lane_half_width), lowest index on ties; none -> free-flow branch.  Distance is
 * centre to centre (np.hypot), as in :111-113.  While installed, t2d_step, t2d_step_n and t2d_integrate run it
 * first: t2d_integrate as a launch of its own on the same stream (kernel_id 4 in t2d_profile_read); the step launches
 * -- for envs of 2..64 participants without IoU events -- in their own front, same leaders and accelerations
 * (t2d_set_step_chaining(pool, 0, *) keeps the separate launch there as well).                */
enum t2d_idm_col {
    T2D_IDM_DESIRED_SPEED = 0,
    T2D_IDM_TIME_HEADWAY = 1,
    T2D_IDM_MIN_SPACING = 2,
    T2D_IDM_MAX_ACCEL = 3,
    T2D_IDM_COMF_DECEL = 4,
    T2D_IDM_DELTA = 5,
    T2D_IDM_LANE_HALF_WIDTH = 6, /* build-defined leader rule */
    T2D_IDM_HORIZON = 7,         /* build-defined: look-ahead (m), may be +inf */
    T2D_IDM_COLS = 8
};
#define T2D_IDM_NONE 255
/* values of forced_leader_dev[i] (device array [n_env * max_agents], or NULL = search everywhere): the
 * reference's calling convention `step(ego_state, leading_state)` -- an agent index inside the env (an
 * inactive or out-of-range index counts as no leader), T2D_IDM_LEADER_FREE = `leading_state=None`,
 * T2D_IDM_LEADER_SEARCH = apply the leader rule above.                                               */
#define T2D_IDM_LEADER_FREE (-1)
#define T2D_IDM_LEADER_SEARCH (-2)
int t2d_set_idm(t2d_pool* pool, const double* ctrl_rows, int32_t n_ctrl, int32_t row_stride,
                const uint8_t* ctrl_id);
int t2d_idm_actions(t2d_pool* pool, const int32_t* forced_leader_dev, void* hip_stream);

/* verify_state -- the reference's "very rough check" of a state transition (SingleTrackKinematics.verify_state
 * physics/single_track_kinematics.py:200-250, SingleTrackDynamics.verify_state single_track_dynamics.py:253-306,
 * PointMass.verify_state point_mass.py:234-259; called by ParticipantBase._verify_state participant_base.py:107-118).
 * last_state = the pool's current state, candidate = four device arrays [n_env * max_agents] (x, y, heading, speed);
 * valid_dev[i] = 1 where the reference returns True (also for inactive participants and interval_ms = 0).
 * Quirks kept: any unbounded range -> True; x / y are tested with strict inequalities against an unsorted range. */
int t2d_verify_state(t2d_pool* pool, const float* x_dev, const float* y_dev, const float* heading_dev,
                     const float* speed_dev, int32_t interval_ms, uint8_t* valid_dev, void* hip_stream);

/* Device-resident trajectories -- the reference's per-participant Trajectory (participant/trajectory/trajectory.py:12-188)
 * for a whole pool, kept on the device, and PhysicsModelBase.verify_states (physics/physics_model_base.py:53-73; called by
 * ParticipantBase._verify_trajectory participant_base.py:120-131) over it in one launch.
 *
 * A t2d_traj is bound to one pool: its N (= n_env * max_agents), its device, and -- read at t2d_verify_states time -- its
 * participants' ids (type, model, active) and its parameter table.  It holds T2D_TRAJ_COLS fp32 columns (x, y, heading, speed,
 * vx, vy: what the pool stores), each laid out [capacity][N]: slot s is row s of every column.  The library never grows or
 * wraps a buffer: which frame lives in which slot, and growth (a bigger t2d_traj + t2d_traj_copy), are the caller's.
 * Destroy a trajectory before its pool.
 *
 *   t2d_traj_record   slot <- the pool's current state: one stream-ordered launch, no host sync.  A record enqueued on the
 *                     step's stream after t2d_step sees that step's state.  (The intermediate states of a t2d_step_n fragment are
 *                     not recorded: record at fragment ends, or step one launch at a time.)
 *   t2d_traj_write    slot <- cols_host, 6 x N fp32 (x, y, heading, speed, vx, vy), e.g. a host BatchedState; synchronous.
 *   t2d_traj_read     cols_host (6 x N) <- slot; waits for the pool's work first (as t2d_download does).
 *   t2d_traj_column   zero-copy device pointer of column `col` ([capacity][N] fp32), valid until t2d_traj_destroy.
 *   t2d_traj_copy     slots [0, n_slots) of src -> dst (same N and device; capacities may differ), stream-ordered.
 *   t2d_verify_states valid_dev[i] (uint8, N) = 1 exactly when the reference's verify_states returns True for participant i's
 *                     trajectory of n_frames frames, frame k held in slot slot_host[k]: frame k >= 1 is checked against frame 0
 *                     with interval interval_ms_host[k] (fp64 ms, dt = interval / 1000; entry 0 is unused).  The check is
 *                     t2d_verify_state's, row by row (model ids 2 and 4: the point-mass acceleration test; single-track rows with
 *                     all three range flags: the heading / speed / x / y box; True for interval 0).  Inactive participants and
 *                     one-frame trajectories get 1.  One launch on hip_stream; the host arrays are read during the call.
 *
 * Reference quirks kept (the caller computes the intervals as the reference does):
 *   - last_state is never advanced (physics_model_base.py:65-71): every frame is checked against the FIRST frame, not its
 *     predecessor -- a trajectory the model itself stepped usually fails after frame 1, and a jump passes if it stays within
 *     one interval's reach of frame 0;
 *   - a stable-frequency trajectory's interval is 1000 / fps (a float: 33.333... ms at 30 fps), not the stamp difference; an
 *     uneven one uses frame_k - frame_0;
 *   - t2d_verify_state's own quirks: an unbounded range passes, x / y are strict inequalities against an unsorted range.
 *
 * Errors: T2D_ERR_INVALID for a null pointer, a slot at or past capacity, n_frames < 1, col outside [0, T2D_TRAJ_COLS),
 * capacity < 1, or t2d_traj_copy between trajectories of another N / device or of more slots than either holds;
 * T2D_ERR_STATE (t2d_traj_record, t2d_verify_states) for a pool without a parameter table or without a t2d_reset.  The
 * message is the bound pool's t2d_last_error.                                                                            */
#define T2D_TRAJ_COLS 6
typedef struct t2d_traj t2d_traj;
int t2d_traj_create(t2d_pool* pool, int32_t capacity, t2d_traj** out_traj);
int t2d_traj_destroy(t2d_traj* traj);
int t2d_traj_record(t2d_traj* traj, int32_t slot, void* hip_stream);
int t2d_traj_write(t2d_traj* traj, int32_t slot, const float* cols_host);
int t2d_traj_read(t2d_traj* traj, int32_t slot, float* cols_host);
int t2d_traj_column(t2d_traj* traj, int32_t col, void** dev_ptr, size_t* nbytes);
int t2d_traj_copy(t2d_traj* dst, const t2d_traj* src, int32_t n_slots, void* hip_stream);
int t2d_verify_states(t2d_traj* traj, int32_t n_frames, const int32_t* slot_host, const double* interval_ms_host,
                      uint8_t* valid_dev, void* hip_stream);

/* Replayed participants -- ParticipantBase.is_active / get_state(frame) (participant/element/participant_base.py:166-203) and
 * ScenarioManager.get_active_participants(frame) (traffic/scenario_manager.py:83-94) inside the device step: a participant
 * whose parameter row has model T2D_MODEL_REPLAY takes its state from a recorded trajectory instead of a physics model.
 *
 * Source: a t2d_traj whose slot k holds the states of time stamp t0_ms + k * period_ms, k in [0, n_slots).  It may belong to
 * another pool of the same max_agents and device (a library pool that is never stepped) with n_src_env envs.  Source
 * participant j is present in slots [first_slot[j], last_slot[j]] (first > last: never).
 * Binding: env e of `pool` shows source env src_env[e] (NULL: e itself, needs n_src_env == n_env) at stamp
 * T2D_F_FRAME_MS[e] + offset_ms[e] (NULL: 0); agent a of the env is agent a of the source env.
 *
 * A step to interval i (t2d_integrate, t2d_step, every step of t2d_step_n and t2d_step_host) runs ONE launch ahead of the step
 * launch, after the IDM controllers and the drift side kernel: for every participant whose type row has model 5, with
 * F = frame_ms[e] + i + offset_ms[e] and k = (F - t0_ms) / period_ms: where first_slot[j] <= k <= last_slot[j] and k < n_slots
 * the six state columns become slot k of the source, bit for bit, and the active byte of T2D_F_IDS becomes 1 (the model
 * byte 5); elsewhere the active byte becomes 0 and the state is left as it is.  The events, the lidar and the leader
 * search of that step see the new state.  There is no interpolation: the host refuses (T2D_ERR_INVALID, nothing stepped)
 * an interval, an offset or a t0_ms that is not a multiple of period_ms.  t2d_collide and t2d_check_status do not advance
 * it.  t2d_step_form reports T2D_FORM_UNFUSED for a pool with a model-5 row; a pool without one takes the launches it took.
 *
 *   t2d_replay_bind   all host arrays are read during the call ([n_env]: src_env, offset_ms; [n_src_env * max_agents]:
 *                     first_slot, last_slot, NULL = 0 .. n_slots - 1).  src == NULL unbinds.  A new binding replaces the old.
 *   t2d_replay_apply  the same write for the envs' CURRENT stamp (F = frame_ms[e] + offset_ms[e]), advancing nothing: after
 *                     t2d_reset and before t2d_snapshot it puts the replayed participants where the recording has them at
 *                     episode start (an auto-reset then restores that state and the ids with the snapshot).
 *
 * Errors: T2D_ERR_INVALID for a source of another max_agents or device, src_env outside [0, n_src_env), NULL src_env with
 * n_src_env != n_env, n_slots outside [1, capacity], period_ms < 1, t0_ms or an offset off the grid, a window slot outside
 * [0, n_slots) (first > last is legal), and -- at step time -- an interval off the grid; T2D_ERR_STATE for stepping (or
 * t2d_replay_apply on) a pool whose table holds a model-5 row without a binding, and for t2d_traj_destroy of a trajectory
 * that is still bound (unbind, or destroy the stepped pool, first).  A failed t2d_replay_bind leaves the previous binding. */
int t2d_replay_bind(t2d_pool* pool, const t2d_traj* src, int32_t n_slots, int32_t t0_ms, int32_t period_ms,
                    const int32_t* src_env, const int32_t* offset_ms, const int32_t* first_slot, const int32_t* last_slot);
int t2d_replay_apply(t2d_pool* pool, void* hip_stream);

/* Off-route detection -- OffRoute.update (traffic/event_detection/off_route.py:24-34: `route.distance(location) > threshold`,
 * location = the participant's centre point, route = a LineString) for every participant of every env in ONE launch.
 *
 * Per participant i with position (x, y) (the pool's fp32 columns), a route (a polyline of n >= 2 fp32 vertices, env-local
 * coordinates) and a threshold (fp32), everything widened to fp64, one rounding per operation, per segment A -> B:
 *   ux = Bx - Ax, uy = By - Ay, wx = Px - Ax, wy = Py - Ay, L2 = ux ux + uy uy, t = wx ux + wy uy;
 *   t <= 0: d2 = wx wx + wy wy;  else t >= L2: vx = Px - Bx, vy = Py - By, d2 = vx vx + vy vy;  else c = wx uy - wy ux,
 *   d2 = (c c) / L2   (a zero-length segment has t = 0 and takes the first branch);
 * d2min = the minimum over the segments in vertex order (strict <: the first minimum wins), d = sqrt(d2min) (IEEE),
 * off = d > (double)threshold (strict, as the reference), distance = (float)d.  A negative threshold makes every finite
 * distance "off", a NaN threshold none (both as in the reference).
 * BUILD-DEFINED (the reference raises, or cannot build such a LineString; a batched call cannot raise per lane): no route for
 * the participant (route_of = -1), an inactive participant (active byte of T2D_F_IDS), a non-finite x or y, or a trace route
 * whose window holds fewer than two slots: off = 0, distance = NaN.  A pedestrian is a point like everyone else: the centre,
 * never the shape.  PARITY UNPINNED against the reference's engine (GEOS is not available to this build): the arithmetic is
 * pinned against exact rational arithmetic (tests/route_ref.py).
 *
 * One kind of routes is installed at a time; installing one replaces the other.  All host arrays are read during the call.
 *   t2d_set_routes          map routes, shared between envs.  A route SET is a list of polylines, CSR like
 *                           t2d_set_static_geometry: routes of set s are [set_route_offsets[s], set_route_offsets[s + 1]),
 *                           vertices of route r are [route_vert_offsets[r], route_vert_offsets[r + 1]) of verts_xy (interleaved
 *                           x, y).  set_of_env[e] picks the set env e uses (NULL: set 0 for every env -- 4096 envs on one map
 *                           hold one copy of it); route_of[i] = index of participant i's route inside its env's set, -1 = none
 *                           (NULL: none for everybody); threshold[i] (NULL: 0 for everybody).  n_sets = 0 or NULL offsets
 *                           clear the routes (of either kind).  A set holds at most T2D_MAX_ROUTE_SET_VERTS vertices (the
 *                           kernel stages the env's set in LDS): T2D_ERR_GEOMETRY beyond, the message names limit and set.
 *   t2d_set_route_assignment  route_of / threshold alone (either may be NULL = unchanged): a new episode on the same map
 *                           re-uploads no geometry.  For trace routes route_of is the source agent index (below).
 *   t2d_set_routes_from_traj  trace routes, straight from a recorded trajectory: the route of participant (e, a) is the
 *                           polyline through the (x, y) of source participant (src_env[e], route_of[i]) in slots
 *                           first_slot .. last_slot of traj (Trajectory.get_trace(frame_range),
 *                           participant/trajectory/trajectory.py:151-168: every recorded stamp in the window, in order).
 *                           route_of NULL: the own agent index a; -1: none.  src_env NULL: e itself (needs as many source
 *                           envs as envs); first_slot / last_slot [N_src], NULL = 0 .. n_slots - 1, first > last is legal
 *                           (= no route).  The source follows t2d_replay_bind's rules (same max_agents and device, possibly
 *                           another pool).  NO VERTEX IS COPIED: the kernel reads the trajectory's own x and y columns, so
 *                           re-recording a bound slot changes the route, and the trajectory must outlive the binding
 *                           (t2d_traj_destroy of a bound one: T2D_ERR_STATE, as for replay; t2d_set_routes(pool, 0, ...) or
 *                           t2d_destroy of the pool releases it).
 *   t2d_off_route           one launch, asynchronous on hip_stream, reads the pool's current state, writes distance f32[N]
 *                           and verdict u8[N] to caller-owned device memory; a NULL output goes to a buffer of the pool's own
 *                           (t2d_off_route_buffers; allocated on first use).  Reads the status configuration nowhere and
 *                           changes no pool field, flag bit, status or reward.  kernel_id 9 in t2d_profile_read.  No stepping
 *                           call launches it.
 * Errors, before anything is enqueued and leaving the previous routes installed: T2D_ERR_INVALID for non-monotone offsets, a
 * route of fewer than two vertices, set_of_env / route_of / src_env out of range, n_slots outside [1, capacity], a window slot
 * outside [0, n_slots), a source of another max_agents or device; T2D_ERR_GEOMETRY for a set beyond T2D_MAX_ROUTE_SET_VERTS;
 * T2D_ERR_STATE for t2d_off_route without routes, without a parameter table or without a t2d_reset, for
 * t2d_set_route_assignment without routes, and for t2d_off_route_buffers before the first use of the pool's own buffers.  */
#define T2D_MAX_ROUTE_SET_VERTS 4096   /* vertices of one route set (64 routes x 64 vertices: 32 KiB of LDS as fp32 pairs) */
int t2d_set_routes(t2d_pool* pool, int32_t n_sets, const int32_t* set_route_offsets, const int32_t* route_vert_offsets,
                   const float* verts_xy, const int32_t* set_of_env, const int32_t* route_of, const float* threshold);
int t2d_set_route_assignment(t2d_pool* pool, const int32_t* route_of, const float* threshold);
int t2d_set_routes_from_traj(t2d_pool* pool, const t2d_traj* traj, int32_t n_slots, const int32_t* src_env,
                             const int32_t* first_slot, const int32_t* last_slot, const int32_t* route_of,
                             const float* threshold);
int t2d_off_route(t2d_pool* pool, float* dist_out_dev, uint8_t* off_out_dev, void* hip_stream);
int t2d_off_route_buffers(t2d_pool* pool, void** dist_dev, void** off_dev, size_t* n_elements);

/* Racing tile progress -- _RacingScenarioManager._locate_agent (envs/racing.py:261-301), check_status (:339-369) and
 * RacingEnv._get_rewards (:121-139) for every env in ONE launch behind the step launch.
 *
 * A TRACK is a ring of n_tile lane tiles, tile i's successor is (i + 1) % n_tile (what RacingTrackGenerator._get_tiles builds,
 * map/generator/generate_racing_track.py:160-198), each tile four fp32 vertices in the order of Lane.geometry
 * (map/element/lane.py:125-128: the left side, then the right side reversed).  Lane.geometry is a LinearRing, so the
 * reference's `tile_shape.intersects(pose) or tile_shape.contains(pose)` is true exactly when one of the tile's four EDGES
 * meets the closed box of the car: a car wholly inside a tile touches nothing.  The predicate is stated in
 * tactics2d_amd/csrc/t2d_track_dev.h (fp64 from the fp32 inputs, one rounding per operation, the box = Vehicle.get_pose with
 * the event kernels' expressions) and again in tests/track_ref.py; like every geometric predicate here it is pinned against
 * exact rational arithmetic, not against GEOS.  It needs no convexity of the tile.  An ego that is inactive, not box-shaped
 * or whose pose is not finite touches nothing (build-defined).
 *
 * The march (racing.py:271-288): starting at tile_visiting it walks the successors once round the ring, collects the FIRST
 * contiguous run of touched tiles and stops at the first untouched tile after the run has begun.  With offsets counted from
 * tile_visiting the run is [j0, j1).  If it is not empty, tile_visiting becomes its last tile, the run is marked visited,
 * and so is the GAP in front of it, under one of two rules:
 *   T2D_TRACK_RULE_REFERENCE  the reference exactly (racing.py:292-301): the gap loop starts at the successor of tile_visiting
 *                             and stops at the first member of the run, i.e. offsets [1, j0) -- and when the run is
 *                             [tile_visiting] alone it never meets a member until it has gone all the way round: EVERY tile is
 *                             marked and the lap is complete (the reference's degenerate case, kept bit for bit; so does a car
 *                             that touches only the tile behind it).  max_advance is ignored.
 *   T2D_TRACK_RULE_FORWARD    BUILD-DEFINED: the same predicate and the same march, but (a) only tile_visiting and its first
 *                             max_advance successors are looked at (0 = the whole ring), and (b) the gap is the tiles strictly
 *                             between tile_visiting and the run's first tile -- empty when the run starts at tile_visiting or at
 *                             its successor.  Nothing else differs.  With it a lap completes when the car has driven it.
 *
 * Status and reward, per env, from what the step launch left in T2D_F_STATUS / T2D_F_FLAGS / T2D_F_CNT_STEP (nothing is
 * recomputed; the order of the first three checks is ParkingEnv's, so the pool's bytes already decide them; configure the pool
 * with check_no_action = 1, no_action_max_step = 100 and no arrival for the reference's racing checklist), first match wins:
 *   pool scenario TIME_EXCEEDED            -> scenario TIME_EXCEEDED (3), reward -1
 *   pool traffic  T2D_TRAFFIC_NO_ACTION_QUIRK -> traffic 5 (racing.py:351 stores ScenarioStatus.NO_ACTION in traffic_status, so
 *                                             _get_rewards gives this step the RUNNING reward, not -1), truncated
 *   pool scenario OUT_BOUND                -> traffic 4 (racing.py:356 stores ScenarioStatus.OUT_BOUND there), reward -5
 *   check_off_road and T2D_FLAG_OFF_LANE of the ego -> traffic T2D_TRAFFIC_OFF_LANE (6), reward -5.  BUILD-DEFINED: the
 *                                             reference's OffLane.update is a stub and TrafficStatus.OFF_ROAD does not exist
 *   every tile visited                     -> scenario COMPLETED, reward (n_tile - 0.1 cnt_step) / n_tile * 100, terminated
 *   otherwise                              running reward -0.1 cnt_step + 0.1 num_visited
 * in fp64 in the reference's order, stored as fp32; truncated = not terminated and (scenario != NORMAL or traffic != NORMAL).
 *
 *   t2d_set_tracks       n_sets tracks shared between envs, CSR like t2d_set_routes: tiles of track s are
 *                        [set_tile_offsets[s], set_tile_offsets[s + 1]) of tiles_xy ([n_tile][4][2] fp32, host memory);
 *                        3 <= n_tile <= T2D_MAX_TRACK_TILES (beyond: T2D_ERR_GEOMETRY; the visited mask is
 *                        T2D_MAX_TRACK_TILES / 32 words per env); set_of_env[e] picks env e's track (NULL: track 0); ego_index =
 *                        the agent that drives; rule, max_advance, check_off_road as above.  Every env starts as after
 *                        t2d_track_reset.  n_sets = 0 or NULL offsets remove the tracks.
 *   t2d_track_reset      envs with env_mask[e] != 0 (NULL: all): only tile 0 visited, tile_visiting = 0 (_reset_map,
 *                        racing.py:303-312), status NORMAL.
 *   t2d_track_upload     the same from the caller's values (an episode resumed in the middle of a lap): tile_visiting i32[E],
 *                        mask u32[E][T2D_MAX_TRACK_TILES / 32] (bit t % 32 of word t / 32 = tile t); entries of unselected envs
 *                        are ignored.  A tile_visiting outside the env's ring or mask bits beyond n_tile: T2D_ERR_INVALID.
 *   t2d_track_progress   one launch, asynchronous on hip_stream.  Results go to buffers of the track's own
 *                        (t2d_track_buffers: tile_visiting i32[E], num_visited i32[E], mask, status u8[E][4] in the layout of
 *                        T2D_F_STATUS, reward f32[E]); write_status != 0 also stores status and reward into T2D_F_STATUS /
 *                        T2D_F_REWARD, so that t2d_restore(pool, 1, stream) puts finished racing episodes back.  An env whose
 *                        OWN status buffer says terminated or truncated from the previous launch starts this launch from the
 *                        progress state t2d_track_reset / t2d_track_upload last gave it (the library keeps that copy as
 *                        t2d_snapshot keeps the pool's), whatever write_status was.  kernel_id 10 in t2d_profile_read.  No
 *                        stepping call launches it, it changes no other pool field, and t2d_set_auto_reset is not involved.
 * Errors: T2D_ERR_INVALID for a null pool / array, n_tile < 3, non-monotone offsets, set_of_env / ego_index / rule out of
 * range, max_advance < 0; T2D_ERR_GEOMETRY for a track beyond T2D_MAX_TRACK_TILES or a non-finite vertex; T2D_ERR_STATE for
 * t2d_track_reset / _upload / _progress / _buffers without tracks and for t2d_track_progress without a parameter table or
 * a t2d_reset.  A failing call leaves the installed tracks and their state as they were.                                   */
#define T2D_MAX_TRACK_TILES 2048      /* tiles of one track: four times the largest ring the reference's generator was seen to make */
#define T2D_TRACK_RULE_REFERENCE 0
#define T2D_TRACK_RULE_FORWARD 1
int t2d_set_tracks(t2d_pool* pool, int32_t n_sets, const int32_t* set_tile_offsets, const float* tiles_xy,
                   const int32_t* set_of_env, int32_t ego_index, int32_t rule, int32_t max_advance, int32_t check_off_road);
int t2d_track_reset(t2d_pool* pool, const uint8_t* env_mask);
int t2d_track_upload(t2d_pool* pool, const uint8_t* env_mask, const int32_t* tile_visiting, const uint32_t* mask);
int t2d_track_progress(t2d_pool* pool, int32_t write_status, void* hip_stream);
int t2d_track_buffers(t2d_pool* pool, void** tile_visiting_dev, void** num_visited_dev, void** mask_dev, void** status_dev,
                      void** reward_dev, size_t* n_env);

/* Racing tracks generated on the device (kernel: tactics2d_amd/csrc/t2d_trackgen.hip) -- RacingTrackGenerator.generate
 * (map/generator/generate_racing_track.py) as the host class tactics2d_amd/generator.py::RacingTrackGenerator restates it, for
 * many tracks in one launch, and RacingEnv.reset's "a new track for every episode" (envs/racing.py:374-383) without the host.
 *
 * THE STREAM.  Like the parking generator the build draws from a counter stream of its own, not numpy's MT19937: splitmix64,
 * the top 53 bits of each output as a uniform u in [0, 1) (tactics2d_amd/csrc/t2d_rng.h).  With fin() the splitmix64 finaliser
 * (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31; all modulo 2^64), ATTEMPT a
 * OF TRACK t draws from the stream whose state before its first draw is
 *     fin(fin(seed + (t + 1) * T2D_TRACKGEN_KEY_TRACK) + (a + 1) * T2D_TRACKGEN_KEY_ATTEMPT)
 * and draw k (k = 0 first) of a stream in state s is u = (fin(s + (k + 1) * 0x9E3779B97F4A7C15) >> 11) * 2^-53.
 * randint(10, 20) is 10 + floor(10 u), uniform(a, b) is a + (b - a) u, and within an attempt the draws are asked for in the
 * order RacingTrackGenerator._get_checkpoints asks numpy for them: n; n noises; n radii; then per pass and turn t1, t2 and,
 * for a rejected turn, the radius step and the angle step.
 * THE RULE.  An attempt succeeds as in the reference: all n turns glued within 100 passes AND the angles still sorted (a turn
 * whose three points are collinear, |denominator| < 1e-10, where the reference raises, fails its attempt).  THE TRACK IS THE
 * ONE MADE FROM THE SUCCESSFUL ATTEMPT WITH THE LOWEST INDEX; attempts 0 .. T2D_TRACKGEN_MAX_ATTEMPTS - 1 are tried (one in
 * six succeeds: 0.83^128 = 4e-11).  The kernel runs T2D_TRACKGEN_ROUND consecutive attempts side by side; the result does not
 * depend on that, on the launch or on how a batch is split: track first_track + i of one call is track i of a call that
 * starts there.  A track that hits the cap (T2D_TRACKGEN_CAPPED) or has more than T2D_MAX_TRACK_TILES tiles
 * (T2D_TRACKGEN_OVERFLOW) comes back FLAGGED, without tiles, and is never installed.
 * THE BUILD restates the host class step by step in fp64, one rounding per operation, trigonometry = the deterministic
 * sincos / atan2 / mod 2 pi of t2d_math.h: _circle_radius, the control points of the accepted pass, _get_start_point (with
 * its Frobenius-norm measure of a straight, and "the first of the three longest that is < 200, else the third"), _bezier2
 * (50 points per turn), _Polyline.length as a running sum in segment order, n_tile = ceil(length / 10), _get_tiles (a point at
 * distance d lies on the first segment k with before[k] + seg[k] > d), the shift to the centre of the fp64 bounding box of
 * the tile vertices, rounding to fp32, RacingTrack.start_pose from the shifted fp64 start line (car_length = the ego's
 * length; heading reduced to [0, 2 pi)) and the boundary (floor min x, ceil max x, floor min y, ceil max y) over the fp32
 * tile vertices and the fp32 shifted centre-line points.  np.linalg.norm sums in an order BLAS chooses; here the norm of 2
 * numbers is sqrt(a*a + b*b) and of 4 numbers sqrt(((a*a + b*b) + c*c) + d*d).  tests/trackgen_ref.py states all of this in
 * Python; the kernel agrees with it bit for bit, and it agrees with the host class (fed the same draws) to one fp32 ulp.
 * PARITY with the reference: by construction different in the random stream, the attempt cap and the norms' summation order.
 *
 *   t2d_generate_tracks  the stand-alone batch generator (no pool), one launch, asynchronous on hip_stream.  Every output is
 *                        DEVICE memory, one record per track, tiles in the CAPACITY LAYOUT: tiles f32 [n_tracks]
 *                        [T2D_MAX_TRACK_TILES][4][2] (64 KiB per track; only the first n_tile records of a track are written),
 *                        n_tile / n_checkpoint / attempt i32 [n_tracks] (attempt = index of the accepted attempt, -1 at the
 *                        cap), start_pose f64 [n_tracks][3], start_line f32 [n_tracks][2][2], boundary f32 [n_tracks][4],
 *                        flags u32 [n_tracks].  Of a flagged track only flags, attempt, n_checkpoint and n_tile (0 at the
 *                        cap, the refused count beyond the capacity) are written.  tiles, start_line and boundary are written
 *                        with 16-byte vector stores: these three pointers must be 16-byte aligned (hipMalloc's are), and
 *                        T2D_ERR_INVALID is returned for one that is not.
 *   t2d_set_tracks_generated  generates n_sets tracks (streams first_track .. first_track + n_sets - 1) INTO the pool and
 *                        installs them as t2d_set_tracks would: the tiles are the pool's track sets in the capacity layout,
 *                        with a per-set tile count the progress launch and the camera's track layer read (host-uploaded tracks
 *                        fill the same array); each env's out-bound boundary, the ego's start pose in the state columns and in
 *                        the episode snapshot (speed 0) and the progress state as after t2d_track_reset are installed too, all
 *                        on the device.  Needs a parameter table, t2d_reset, t2d_snapshot and a boundary array
 *                        (t2d_set_static_geometry) to write into.  Synchronous, as t2d_set_tracks is; reads n_tile back (so that
 *                        t2d_track_upload keeps validating).  check_off_road is not supported with generated tracks: the
 *                        function has no such argument, so there is nothing for it to refuse with T2D_ERR_INVALID -- the refusal
 *                        is the binding's (ParticipantPool.set_tracks_generated(check_off_road=True) and VecRacingEnv raise
 *                        ValueError), and the progress launch runs as with check_off_road = 0.  Any flagged track: T2D_ERR_GEOMETRY, the message names it, nothing is installed.
 *                        regenerate = 1 needs n_sets == n_env, the identity set_of_env (or NULL then) and track_stride >=
 *                        n_env (T2D_ERR_INVALID otherwise).
 *   t2d_tracks_regenerate  ONE launch, asynchronous, for between t2d_track_progress(write_status = 1) and t2d_restore(pool, 1):
 *                        every env whose track status says terminated or truncated moves on to its next episode k (its count
 *                        goes up by one): the track of stream first_track + e + k * track_stride is generated IN PLACE into
 *                        the env's slot, and its tile count, its boundary and the start pose in the snapshot replace the old
 *                        ones; the restore launch that follows starts the episode there.  Terminal status and reward stay
 *                        readable.  An env whose new track is flagged keeps its old track, and the pool's sticky error word is
 *                        raised: the next t2d_sync / t2d_download reports T2D_ERR_STATE once.  Its episode count does NOT go
 *                        up then, so its next finish asks for the same stream and is flagged again: such an env stays on its old
 *                        track until t2d_set_tracks_generated re-keys it (about 4e-11 per track at the cap).  Workgroups of envs that did not
 *                        finish exit on their first load.  T2D_ERR_STATE unless t2d_set_tracks_generated(regenerate = 1)
 *                        preceded it.  kernel_id 12 in t2d_profile_read.  No stepping call launches it.                        */
#define T2D_TRACKGEN_MAX_ATTEMPTS 128
#define T2D_TRACKGEN_ROUND 16
#define T2D_TRACKGEN_CAPPED 1u
#define T2D_TRACKGEN_OVERFLOW 2u
#define T2D_TRACKGEN_KEY_TRACK 0xD1B54A32D192ED03ull
#define T2D_TRACKGEN_KEY_ATTEMPT 0x8CB92BA72F3D8DD7ull
#define T2D_PROFILE_TRACKGEN 12
int t2d_generate_tracks(int32_t device_id, int32_t n_tracks, uint64_t seed, int64_t first_track, double car_length,
                        float* tiles_dev, int32_t* n_tile_dev, int32_t* n_checkpoint_dev, int32_t* attempt_dev,
                        double* start_pose_dev, float* start_line_dev, float* boundary_dev, uint32_t* flags_dev, void* hip_stream);
int t2d_set_tracks_generated(t2d_pool* pool, int32_t n_sets, uint64_t seed, int64_t first_track, int64_t track_stride,
                             double car_length, const int32_t* set_of_env, int32_t ego_index, int32_t rule, int32_t max_advance, int32_t regenerate);
int t2d_tracks_regenerate(t2d_pool* pool, void* hip_stream);
/* device pointers of the generated tracks' records (n_sets of each, layouts as t2d_generate_tracks'; valid until the tracks
 * are replaced): T2D_ERR_STATE without generated tracks                                                                     */
int t2d_generated_track_buffers(t2d_pool* pool, void** tiles_dev, void** n_tile_dev, void** n_checkpoint_dev, void** attempt_dev,
                                void** start_pose_dev, void** start_line_dev, void** boundary_dev, void** episode_dev,
                                size_t* n_sets);

/* Reeds-Shepp curves and the parking tutorial's planner on the device.
 *
 * The curve family is ReedsShepp of interpolator/reeds_shepp.py: get_all_path (:495-527) normalises the goal into the start
 * frame in units of the radius and returns T2D_RS_SLOTS = 48 slots in a fixed order -- _CSC 0-7 (:207-257), _CCC 8-19
 * (:259-312), _CCCC 20-27 (:314-374), _CCSC 28-43 (:376-449), _CCSCC 44-47 (:451-493) -- each None or a ReedsSheppPath
 * whose `segments`, `signs` and `length` are those of :19-44.  get_path (:529-558) keeps the LAST of several equal shortest
 * lengths; the tutorial's planner pops a heap of (length, index) and so takes the LOWEST index.
 *   t2d_rs_slot_info  the constants of one slot, host only (no device needed): letters[5] +1 L / -1 R / 0 S, signs[5] the
 *                     `signs` of its paths, zero padded both; n_seg; curve_type 0 CSC, 1 CCC, 2 CCCC, 3 CCSC, 4 CCSCC.
 *   t2d_rs_paths      get_all_path for n independent queries in ONE launch, asynchronous on hip_stream, no pool:
 *                     start_dev / goal_dev f64 [n][3] (x, y, heading; device memory) and one radius ->
 *                     valid_dev u64 [n] (bit s: slot s is a path), segments_dev f64 [n][48][5] (signs[i] * segments[i], in
 *                     units of the radius, zero padded, all zero for None), length_dev f64 [n][48] (metres, +inf for None),
 *                     shortest_dev i32 [n][2]: get_path's slot, then the lowest-index shortest one (-1: no slot is a
 *                     path, as for a query that is not finite).  T2D_ERR_INVALID for radius <= 0 (ReedsShepp.__init__
 *                     :153-156 raises ValueError), n < 0 or a null pointer: nothing is launched.
 *
 * The planner is cell 9 of docs/tutorial/train_parking_demo.ipynb for the ego of every env, one launch:
 *   get_rs_path          both poses shifted to the rear axle (ego: the state columns; goal: the mean of the target quad's
 *                        four vertices and the target heading, read from the device copies of t2d_set_target_areas /
 *                        t2d_set_target_headings or of the generated scenes); no plan beyond threshold_distance;
 *                        candidates in ascending (length, slot) up to length_ratio x the shortest; the first whose
 *                        swept box crosses no obstacle edge is the plan.
 *   construct_obstacles  the scan clipped to [0, max_range] (+inf: max_range), minus distance_tolerance, floored at
 *                        vehicle_base[k]; point k at angle k * pi / n_beams * 2, shifted by center_shift in x; n_beams edges
 *                        joining consecutive points in a closed chain; edges that touch the box at the goal are dropped.
 *   is_traj_valid        the LINES of the box's four edges against the line of every chain edge; a hit is an intersection
 *                        point within both edges' coordinate ranges +- edge_tolerance; parallel lines never hit.
 * BUILD-DEFINED: (1) sampling -- segment i of a path is checked at the arc lengths k * sample_step, k = 0 .. ceil(len_i /
 * sample_step), the last one clipped to len_i, so every segment's start and end pose is checked (the reference's arcs come
 * from its compiled Circle.get_arc, omit their end point and take their yaw from a linspace); a path of more than
 * T2D_RS_MAX_POSES poses is not checked: status T2D_RS_UNCHECKED, the plan stops there.  (2) the goal box of
 * construct_obstacles stands at the goal IN THE FRAME OF THE CHAIN (the ego's rear axle); the notebook passes the world-frame
 * pose there, which is that frame only for an ego at the origin.  (3) all arithmetic is fp64 on the fp32 scan values (numpy
 * keeps `lidar_obs - distance_tolerance` in fp32).  (4) a NaN scan value gives T2D_RS_UNCHECKED for that env.
 *   t2d_rs_config   cfg: see t2d_rs_params (all finite; radius, half_length, half_width, sample_step > 0, length_ratio >= 1,
 *                   the others >= 0; T2D_ERR_INVALID otherwise).  vehicle_base_host: n_beams floats (RSPlanner.
 *                   init_vehicle_base: the distance from the box centre to the box outline along each beam), or NULL: computed
 *                   from half_length / half_width.  Needs t2d_lidar_config (T2D_ERR_STATE) with at most T2D_RS_MAX_BEAMS beams
 *                   (T2D_ERR_INVALID); takes its beam count and range.  Allocates the pool's own plan records.
 *                   The chain is built at the angles k * 2 pi / n_beams: a lidar configured with beam tables that are not
 *                   those angles (to 1e-9 in sin and cos) is refused with T2D_ERR_STATE, here and in t2d_rs_plan.
 *   t2d_rs_plan     one launch, asynchronous on hip_stream, no host synchronisation: behind t2d_step + t2d_lidar_scan on the
 *                   same stream it plans from that step's poses and scan.  lidar_dev: f32 [n_env][n_beams] device memory, or
 *                   NULL = the pool's T2D_F_LIDAR buffer.  out_dev: t2d_rs_plan_record [n_env] (8-byte aligned), or NULL =
 *                   the pool's own records.  T2D_ERR_STATE before t2d_rs_config, after the lidar's beam count changed,
 *                   before t2d_reset, and without target areas and headings.  kernel_id T2D_PROFILE_RS_PLAN in t2d_profile_read.
 *   t2d_rs_plan_buffers  pointer and size in bytes of the pool's own records; T2D_ERR_STATE before t2d_rs_config.
 * Rows that cannot plan: an inactive ego, or a pose / target that is not finite: T2D_RS_NO_TARGET.                      */
#define T2D_RS_SLOTS 48
#define T2D_RS_MAX_SEGMENTS 5
#define T2D_RS_MAX_POSES 1024
#define T2D_RS_MAX_BEAMS 1024
#define T2D_RS_NO_TARGET 0   /* the ego is inactive, or its pose or the target is not finite */
#define T2D_RS_FAR 1         /* the goal is farther than threshold_distance */
#define T2D_RS_FOUND 2
#define T2D_RS_NONE_FREE 3   /* every candidate within length_ratio x the shortest crosses an obstacle edge */
#define T2D_RS_UNCHECKED 4   /* a NaN in the scan (slot -1), or the candidate `slot` has more than T2D_RS_MAX_POSES poses */
#define T2D_PROFILE_RS_PLAN 13
typedef struct t2d_rs_params {
    double radius;              /* wheel_base / tan(steer_ratio * steer_hi) */
    double center_shift;        /* length / 2 - rear_overhang: box centre ahead of the rear axle */
    double half_length, half_width;
    double distance_tolerance;  /* 0.05 */
    double threshold_distance;  /* lidar_range - 5 */
    double sample_step;         /* 0.1 */
    double length_ratio;        /* 2 */
    double edge_tolerance;      /* 1e-4 */
} t2d_rs_params;
typedef struct t2d_rs_plan_record {   /* 96 bytes */
    int32_t status;             /* T2D_RS_* */
    int32_t slot;               /* the chosen slot (T2D_RS_FOUND), the unchecked one, or -1 */
    int32_t n_seg;              /* segments of that slot, else 0 */
    int32_t n_visited;          /* candidates visited */
    int32_t steer[T2D_RS_MAX_SEGMENTS];   /* per segment +1 L / -1 R / 0 S */
    int32_t reserved;
    double distance[T2D_RS_MAX_SEGMENTS]; /* per segment the signed distance in metres (what RSAgent.calculate_target_points consumes) */
    double length;              /* of the chosen slot, NaN without one */
    double shortest;            /* the shortest candidate's length, NaN for NO_TARGET / FAR */
} t2d_rs_plan_record;
int t2d_rs_slot_info(int32_t slot, int8_t* letters, int8_t* signs, int32_t* n_seg, int32_t* curve_type);
int t2d_rs_paths(int32_t device_id, int32_t n, double radius, const double* start_dev, const double* goal_dev, uint64_t* valid_dev,
                 double* segments_dev, double* length_dev, int32_t* shortest_dev, void* hip_stream);
int t2d_rs_config(t2d_pool* pool, const t2d_rs_params* cfg, const float* vehicle_base_host);
int t2d_rs_plan(t2d_pool* pool, const float* lidar_dev, t2d_rs_plan_record* out_dev, void* hip_stream);
int t2d_rs_plan_buffers(t2d_pool* pool, void** dev_ptr, size_t* nbytes);

/* Dubins paths and sampled curve lines on the device -- interpolator/dubins.py (Dubins :107-331, DubinsPath :14-104),
 * ReedsSheppPath.get_curve_line (interpolator/reeds_shepp.py:46-139) and Circle.get_arc (geometry/circle.py:106-139).
 *
 * Dubins.get_all_path (:240-273) returns six slots in a fixed order, LRL, RLR, LSL, RSL, RSR, LSR: None or a DubinsPath with
 * segments (t, p, q) in units of the radius and length = |segments|.sum() * radius; theta = atan2(dy, dx), d = |delta| / radius,
 * alpha / beta = mod(heading - theta, 2 pi); a CSC word is None for a negative discriminant, a CCC word for |discriminant| > 1.
 * get_path (:275-304) keeps the LAST of several equal shortest lengths.  _LRL (:216-231) computes t = mod(-alpha + tmp + p / 2)
 * where the family's form has -alpha - tmp + p / 2: the curve of slot 0 misses the goal.  lrl_rule 0 keeps it
 * as written; lrl_rule 1, BUILD-DEFINED, corrects that sign and changes nothing else.
 *   t2d_dubins_slot_info  the letters of one slot, host only: letters[3] +1 L / -1 R / 0 S.
 *   t2d_dubins_paths      get_all_path for n independent queries in ONE launch, asynchronous on hip_stream, no pool:
 *                         start_dev / goal_dev f64 [n][3] (x, y, heading) -> valid_dev u8 [n] (bit s: slot s is a path),
 *                         segments_dev f64 [n][6][3] (zero for None), length_dev f64 [n][6] (metres, +inf for None),
 *                         shortest_dev i32 [n][2]: get_path's slot, then the lowest-index shortest one; -1: no slot is a path,
 *                         which is also the BUILD-DEFINED answer to a query that is not finite.  T2D_ERR_INVALID for
 *                         radius <= 0 (Dubins.__init__ :126-128 raises ValueError), n < 0, an lrl_rule other than 0 / 1 or a
 *                         null pointer: nothing is launched.
 *
 * A curve line is the point list of get_curve_line: the word walked segment by segment from the start pose.
 *   arcs       centre = point + r (cos(h +- pi/2), sin(h +- pi/2)), + for L; start angle h + pi/2 for R, h - pi/2 for L; points
 *              centre + r (cos a_k, sin a_k), a_k = a0 + k ((a0 + delta) - a0), delta = -+step / r, as many as numpy's arange
 *              gives, ceil((stop - start) / delta) in fp64: the arc's END POINT IS NOT among them; yaw = linspace(h, h_end,
 *              count), which does reach the end heading.  Clockwise: Dubins: the letter is R; Reeds-Shepp: (R and forward) or
 *              (L and backward).
 *   straights  linspace from the point to the end point, end included (the next segment's first point repeats it);
 *              max(1, ceil(L / step)) points for Dubins, max(2, ceil(L / step)) for Reeds-Shepp.
 *   tiny       |length| < 1e-15: the single point.  An arc of 0 points is [point] for Dubins; for Reeds-Shepp an arc of fewer
 *              than 2 points is [point, end_point] with yaw [h, h_end].
 * One word per curve, 48 bytes: f64 seg[5] (signed lengths in units of the radius; under T2D_CURVE_RS the sign is the
 * reference's `forward`; under T2D_CURVE_DUBINS |seg| is read, as DubinsPath.get_curve_line does, so a negative length drives
 * forward), i8 letter[5] (+1 L / -1 R / 0 S), i8 n_seg, 2 bytes of padding.
 * BUILD-DEFINED: a word of 0 segments (or of more than T2D_RS_MAX_SEGMENTS), or a start or segment that is not finite, gives
 * count 0 and nothing else written; a curve of more than max_points points writes its first max_points and count holds the
 * FULL count (saturating at INT32_MAX; a single segment's count at 2^30).
 *   t2d_curve_lines   n curves in ONE launch, asynchronous on hip_stream, no pool: words_dev [n] (8-byte aligned), start_dev
 *                     f64 [n][3], rule T2D_CURVE_DUBINS / T2D_CURVE_RS -> xy_dev f64 [n][max_points][2] (16-byte aligned),
 *                     yaw_dev f64 [n][max_points], count_dev i32 [n], end_dev f64 [n][3] (next_point / next_heading after the
 *                     last segment).  T2D_ERR_INVALID for radius, step_size or max_points <= 0, n < 0, another rule, a null or
 *                     misaligned pointer: nothing is launched.
 *   t2d_curve_routes  the same sampler, curve e for env e, written as fp32 vertices INTO the installed route sets' own device
 *                     storage: route `route` of env e's set, whose vertex count is the capacity.  count c == 0: the route is
 *                     left untouched; c <= capacity: vertices k < c are the points, vertices k >= c the curve's END POINT (the
 *                     route reaches the goal although the arcs omit it; zero-length segments are defined by every consumer);
 *                     c > capacity: the first `capacity` points.  count_dev i32 [n_env] (may be NULL) = c in every case.
 *                     t2d_off_route, t2d_pid_actions and t2d_pursuit_actions see the curve in their next launch on the stream.
 *                     Offsets, assignment and thresholds are untouched.  T2D_ERR_STATE unless route sets are the installed
 *                     kind, no two envs share a set and every env's set has a route `route`; T2D_ERR_INVALID as above, for
 *                     route < 0 and for a count_dev that is not 4-byte aligned (every INVALID before every STATE; the three
 *                     route writers share these checks and their order): nothing is launched.
 *                     kernel_id T2D_PROFILE_CURVE_ROUTES in t2d_profile_read.
 *   t2d_route_vertices  the installed route sets' vertex storage, f32 [n_vertices][2] in the order of t2d_set_routes' verts_xy
 *                     (what t2d_curve_routes writes into and the three consumers read); valid until the routes are replaced or
 *                     cleared.  The memory is writable: a caller that writes through it edits the routes the consumers read and
 *                     orders those writes against their launches itself.  T2D_ERR_STATE unless route sets are the installed kind;
 *                     T2D_ERR_INVALID for a null output.                                    */
#define T2D_DUBINS_SLOTS 6
#define T2D_CURVE_WORD_BYTES 48
#define T2D_CURVE_DUBINS 0
#define T2D_CURVE_RS 1
#define T2D_PROFILE_CURVE_ROUTES 17
int t2d_dubins_slot_info(int32_t slot, int8_t* letters);
int t2d_dubins_paths(int32_t device_id, int32_t n, double radius, const double* start_dev, const double* goal_dev, int32_t lrl_rule,
                     uint8_t* valid_dev, double* segments_dev, double* length_dev, int32_t* shortest_dev, void* hip_stream);
int t2d_curve_lines(int32_t device_id, int32_t n, const void* words_dev, const double* start_dev, double radius, double step_size,
                    int32_t rule, int32_t max_points, double* xy_dev, double* yaw_dev, int32_t* count_dev, double* end_dev,
                    void* hip_stream);
int t2d_curve_routes(t2d_pool* pool, const void* words_dev, const double* start_dev, double radius, double step_size, int32_t rule,
                     int32_t route, int32_t* count_dev, void* hip_stream);
int t2d_route_vertices(t2d_pool* pool, void** verts_dev, size_t* n_vertices);

/* Bezier, B-spline and cubic spline curves on the device -- interpolator/bezier.py, b_spline.py, cubic_spline.py and the compiled
 * module behind them, interpolator/cpp_interpolator/src/{bezier,b_spline,cubic_spline}.cpp, restated operation by operation in
 * fp64 (+ - * / and comparisons only, every sum in the reference's order: tests/spline_ref.py).
 *   Bezier     N control points, n_interpolation >= 2 points: binomials b[k] = b[k-1] * (N-k) / k, t = i * (1 / (n-1)), powers by
 *              repeated multiplication, terms b[k] * (1-t)^(N-1-k) * t^k accumulated from k = 0 upward.
 *   B-spline   n_interpolation >= 1 points at u = u_start + j * ((u_end - u_start) / n_interpolation), j < n_interpolation,
 *              u_start = knots[degree], u_end = knots[n_ctrl]: THE END OF THE CURVE IS NEVER SAMPLED.  The basis is the triangular
 *              table of basis_function: degree 0 is half-open (k[idx] <= u < k[idx+1], 0 at the last knot), a term with a zero
 *              denominator is 0, and the point is the sum over ALL control points in order.  knots_dev NULL: the Python
 *              default, np.linspace(0, 1, n_ctrl + degree + 1), computed on the device as i * (1 / (num - 1)), the last one 1.
 *   cubic      y as a function of strictly increasing x, (n_ctrl-1) * n_interpolation + 1 points.  Inside a segment the abscissa
 *              is ACCUMULATED, xi += h / (n_interpolation-1): the last sample of a segment only approximates the next knot, the
 *              next segment starts on the knot itself (a near-duplicate vertex), and the last control point is appended
 *              exactly.  Natural and Clamped: the Thomas recursion.  NotAKnot: BandedSolve as written (pivot from at most two
 *              rows below, strict >, columns i .. i+2 only); with THREE control points its matrix is singular: where the
 *              elimination cancels exactly (equal spacing always, most other rows) it returns m = 0 and the curve is the
 *              polyline through the points; where a rounding residue is left, that residue is the last pivot and the curve is
 *              what it gives -- the reference's either way.  derivs_dev is read under T2D_SPLINE_CLAMPED only.
 * BUILD-DEFINED, per row: count 0 and nothing else written where n_ctrl is below the family's minimum (Bezier 2, cubic 3,
 * B-spline degree + 1) or above max_ctrl, where the x of a cubic row is not strictly increasing, where knots decrease, or where
 * a control point, knot or (Clamped) derivative the row reads is not finite.  One bad row touches only its own outputs.  A curve
 * of more than max_points points writes its first max_points and count holds the FULL count (saturating at INT32_MAX).
 *   t2d_spline_curves  n curves of ONE family in ONE launch, asynchronous on hip_stream, no pool: kind T2D_SPLINE_*; ctrl_dev
 *                      f64 [n][max_ctrl][2] (16-byte aligned), n_ctrl_dev i32 [n] (row e uses its first n_ctrl[e] points),
 *                      n_interpolation; B-spline: degree and knots_dev f64 [n][max_ctrl + degree + 1] (row e uses its first
 *                      n_ctrl[e] + degree + 1) or NULL; cubic: boundary_type T2D_SPLINE_NATURAL / _CLAMPED / _NOT_A_KNOT and
 *                      derivs_dev f64 [n][2] or NULL (0, 0) -> xy_dev f64 [n][max_points][2] (16-byte aligned), count_dev i32
 *                      [n].  Arguments of another family are ignored.  T2D_ERR_INVALID, nothing launched: n < 0, max_points
 *                      <= 0, another kind or boundary type, n_interpolation below the family's minimum (2, 1, 2), degree < 0
 *                      or > T2D_SPLINE_MAX_DEGREE, max_ctrl < 1 or > T2D_SPLINE_MAX_CTRL, a null or misaligned pointer.
 *   t2d_spline_routes  the same sampler, curve e for env e (n = n_env), written as fp32 vertices into route `route` of env e's
 *                      installed set under the rules of t2d_curve_routes: the route's vertex count is the capacity; count c ==
 *                      0 leaves the route untouched; c <= capacity: vertices k >= c repeat the curve's LAST WRITTEN POINT -- for
 *                      a B-spline that is its last SAMPLE, not the curve's end --; c > capacity: the first `capacity` points.
 *                      count_dev i32 [n_env] (may be NULL) = c.  T2D_ERR_STATE unless route sets are the installed kind, no
 *                      two envs share a set and every env's set has a route `route`; T2D_ERR_INVALID as above and for route
 *                      < 0.  kernel_id T2D_PROFILE_SPLINE_ROUTES in t2d_profile_read.
 * T2D_SPLINE_CURVES_PER_BLOCK curves share a workgroup (one wave each; the per-curve working set, 10 KB for a cubic spline, lives
 * in LDS, which is what the two caps bound).                                                                              */
#define T2D_SPLINE_BEZIER 0
#define T2D_SPLINE_BSPLINE 1
#define T2D_SPLINE_CUBIC 2
#define T2D_SPLINE_NATURAL 1
#define T2D_SPLINE_CLAMPED 2
#define T2D_SPLINE_NOT_A_KNOT 3
#define T2D_SPLINE_MAX_CTRL 32
#define T2D_SPLINE_MAX_DEGREE 5
#define T2D_SPLINE_CURVES_PER_BLOCK 4
#define T2D_PROFILE_SPLINE_ROUTES 18
int t2d_spline_curves(int32_t device_id, int32_t n, int32_t kind, const double* ctrl_dev, const int32_t* n_ctrl_dev, int32_t max_ctrl,
                      int32_t n_interpolation, int32_t degree, const double* knots_dev, int32_t boundary_type, const double* derivs_dev,
                      int32_t max_points, double* xy_dev, int32_t* count_dev, void* hip_stream);
int t2d_spline_routes(t2d_pool* pool, int32_t kind, const double* ctrl_dev, const int32_t* n_ctrl_dev, int32_t max_ctrl,
                      int32_t n_interpolation, int32_t degree, const double* knots_dev, int32_t boundary_type, const double* derivs_dev,
                      int32_t route, int32_t* count_dev, void* hip_stream);

/* Spiral and ParamPoly3 curves and the plan-view reference line of an OpenDRIVE road on the device -- interpolator/spiral.py,
 * interpolator/param_poly3.py and, of map/parser/parse_xodr.py, _sample_line / _sample_spiral / _sample_arc / _sample_poly3 /
 * _sample_param_poly3 / _sample_geometry and the head of load_road (pts_arr, s_arr, kappa_arr), restated operation by operation in
 * fp64 with the library's own sincos and its own Fresnel integrals (tests/road_ref.py).  One wave handles one
 * curve or road, T2D_ROAD_CURVES_PER_BLOCK of them share a workgroup, a lane stores one 16-byte [x, y].
 *   Spiral      n_interpolation >= 1 points at np.linspace(0, length, n).  gamma == 0 and start_curvature == 0: the line;
 *               gamma == 0: the arc by its sin / cos differences; otherwise a (C(t) + i S(t)) exp(i theta_0), a = sqrt(pi /
 *               |gamma|), t = s sqrt(|gamma| / pi), theta_0 = heading - k0^2 / (2 gamma).  AS WRITTEN (T2D_SPIRAL_REFERENCE) this
 *               is the Euler spiral only for k0 == 0 and gamma > 0: |gamma| scales, nothing mirrors, and theta_0 is shifted but the
 *               Fresnel argument is not.  T2D_SPIRAL_STANDARD (build-defined) is the clothoid of heading(s) = heading + k0 s +
 *               gamma s^2 / 2, through the shifted argument t = (s + k0 / gamma) sqrt(|gamma| / pi) and the mirror for gamma < 0;
 *               its line and arc branches are the same.
 *   ParamPoly3  max(2, int(length / 0.1)) points (an fp64 division, truncated) at p = np.linspace(0, p_max, n), p_max = length
 *               under p_range 1 (arcLength) and 1 under p_range 0 (normalized); u, v = a + b p + c p^2 + d p^3 summed left to right
 *               with p^2 = p p and p^3 = (p p) p (numpy's p ** 3 goes through pow: at most an ulp away); [x, y] = (u cos + v
 *               (-sin), u sin + v cos) + start.
 *   plan view   per road up to max_geom records of T2D_PLANVIEW_RECORD_BYTES: i32 kind (T2D_GEOM_*), i32 p_range, f64 s, x, y, hdg,
 *               length, f64 par[8] = spiral {curvStart, curvEnd}, arc {curvature}, poly3 {a, b, c, d}, paramPoly3 {aU, bU, cU, dU,
 *               aV, bV, cV, dV}.  Geometries are sampled in order: line and poly3 max(2, int(length / 0.1) + 1) points (a line of
 *               length <= 0: one); spiral Spiral's 100 points with curvature linspace(curvStart, curvEnd, 100) (length < 1e-6:
 *               one point); arc |curvature| < 1e-9: the line sampler, with curvature 0; otherwise the circle by its tangent and
 *               np.arange at 0.1 m of arc, WHICH NEVER SAMPLES THE ARC'S END; poly3 and paramPoly3 with their analytic curvature
 *               (speed ** 1.5 as speed sqrt(speed)).  A geometry's last point is dropped if it equals the one before it; its s is
 *               linspace(s, s + length, points left).  Over the concatenation, point k is kept if k == 0 or its distance
 *               sqrt(dx dx + dy dy) to RAW point k - 1 (kept or not) is > 0.02.  A road of fewer than 2 kept points has no line:
 *               count 0.  AS WRITTEN, a spiral shorter than about 1.98 m (99 steps of 0.02) loses every point but its first.
 * BUILD-DEFINED, per row: count 0 and nothing else written where a value the row reads is not finite (the par entries of its
 * kinds only), a length is < 0, a kind or a paramPoly3's p_range is unknown, n_geom is outside [1, max_geom], or the road has more
 * than T2D_PLANVIEW_MAX_RAW raw points.  One bad row touches only its own outputs.  A curve or line of more than max_points points
 * writes its first max_points and count holds the FULL count.
 *   t2d_spiral_curves       n spirals in ONE launch, asynchronous on hip_stream, no pool: par_dev f64 [n][6] = {length, x0, y0,
 *                           heading, start_curvature, gamma} -> xy_dev f64 [n][max_points][2] (16-byte aligned), count_dev i32 [n].
 *   t2d_param_poly3_curves  par_dev f64 [n][12] = {length, x0, y0, heading, aU, bU, cU, dU, aV, bV, cV, dV}, p_range_dev i32 [n].
 *   t2d_planview_lines      rec_dev [n][max_geom] records, n_geom_dev i32 [n] -> xy_dev f64 [n][max_points][2], s_dev and kappa_dev
 *                           f64 [n][max_points] (either may be NULL), count_dev i32 [n].
 *                           T2D_ERR_INVALID, nothing launched, for all three: n < 0, max_points <= 0, n_interpolation < 1, another
 *                           rule, max_geom outside [1, T2D_PLANVIEW_MAX_GEOM], a null or misaligned pointer.
 *   t2d_planview_routes     the same chain, road e for env e (n = n_env), written as fp32 vertices into route `route` of env e's
 *                           installed set under the rules of t2d_curve_routes.  A set holds 4096 vertices and a road has ten raw
 *                           points per metre, hence stride >= 1: the vertices are kept points 0, stride, 2 stride, ... and ALWAYS
 *                           the last kept point; count c = the number of vertices that gives.  The route's vertex count is the
 *                           capacity; c == 0 leaves the route untouched; c <= capacity: vertices k >= c repeat the last kept point;
 *                           c > capacity: the first `capacity` of them.  count_dev i32 [n_env] (may be NULL).  T2D_ERR_STATE
 *                           unless route sets are the installed kind, no two envs share a set and every env's set has a route
 *                           `route`; T2D_ERR_INVALID as above and for stride < 1 or route < 0.  kernel_id
 *                           T2D_PROFILE_PLANVIEW_ROUTES in t2d_profile_read.                                                    */
#define T2D_SPIRAL_REFERENCE 0
#define T2D_SPIRAL_STANDARD 1
#define T2D_GEOM_LINE 0
#define T2D_GEOM_SPIRAL 1
#define T2D_GEOM_ARC 2
#define T2D_GEOM_POLY3 3
#define T2D_GEOM_PARAM_POLY3 4
#define T2D_PLANVIEW_RECORD_BYTES 112
#define T2D_PLANVIEW_MAX_GEOM 64
#define T2D_PLANVIEW_MAX_RAW 1048576
#define T2D_ROAD_CURVES_PER_BLOCK 4
enum { T2D_PROFILE_PLANVIEW_ROUTES = 19 };   /* (the kernel ids after 18 are enumerators) */
int t2d_spiral_curves(int32_t device_id, int32_t n, const double* par_dev, int32_t n_interpolation, int32_t rule, int32_t max_points,
                      double* xy_dev, int32_t* count_dev, void* hip_stream);
int t2d_param_poly3_curves(int32_t device_id, int32_t n, const double* par_dev, const int32_t* p_range_dev, int32_t max_points,
                           double* xy_dev, int32_t* count_dev, void* hip_stream);
int t2d_planview_lines(int32_t device_id, int32_t n, const void* rec_dev, const int32_t* n_geom_dev, int32_t max_geom, int32_t rule,
                       int32_t max_points, double* xy_dev, double* s_dev, double* kappa_dev, int32_t* count_dev, void* hip_stream);
int t2d_planview_routes(t2d_pool* pool, const void* rec_dev, const int32_t* n_geom_dev, int32_t max_geom, int32_t rule, int32_t stride,
                        int32_t route, int32_t* count_dev, void* hip_stream);

/* A polyline the caller already has on the device -- a planner's path -- as a route: the fourth writer beside t2d_curve_routes,
 * t2d_spline_routes and t2d_planview_routes, under their rules (T2D_ERR_STATE unless route sets are the installed kind, no two envs
 * share a set and every env's set has a route `route`; asynchronous on hip_stream).
 *   points_dev  f64 [n_env][max_pts][cols], cols >= 2: x and y are the first two columns (t2d_hybrid_astar's path with its heading
 *               column and t2d_sample_plan's path both go in as they are); counts_dev i32 [n_env]: a planner's path_len as it is
 *   The used length is min(counts[e], max_pts).  Vertex k of the route is the fp32 rounding of point k; vertices past the used
 *   length repeat the last used point; a route of fewer vertices than that takes the first `capacity` points.  A row whose count
 *   is <= 0, or one with a coordinate among the points it would write that is not finite once rounded to fp32, leaves its route
 *   as it is.  count_dev i32 [n_env] (may be NULL): the used length, 0 for a row left as it is.
 * T2D_ERR_INVALID, nothing launched: a null or misaligned pointer, max_pts < 1, cols < 2, route < 0.  kernel_id
 * T2D_PROFILE_POLYLINE_ROUTES in t2d_profile_read.                                                                              */
enum { T2D_PROFILE_POLYLINE_ROUTES = 20 };
int t2d_polyline_routes(t2d_pool* pool, const double* points_dev, const int32_t* counts_dev, int32_t max_pts, int32_t cols,
                        int32_t route, int32_t* count_dev, void* hip_stream);

/* Shortest paths over weighted obstacle grids on the device -- search/dijkstra.py (Dijkstra.plan, Dijkstra.plan_graph) over the
 * graph of search/graph_utils.py: grid_to_csr, for n independent grids in ONE launch, asynchronous on hip_stream, no pool
 * (tests/grid_search_ref.py).  One workgroup solves one grid with its weights and its field in LDS.
 *   weight_dev  f64 [n][max_cells]: grid e is its first H * W entries, row-major; +inf or NaN marks an obstacle
 *   hw_dev      i32 [n][2]: H and W of grid e (a ragged batch); source_dev / target_dev i32 [n]: cells row * W + col;
 *               target -1 asks for the field alone
 *   connectivity 4 or 8; diagonal_cost_multiplier: finite, >= 0
 *   edges       never stored: between two neighbouring free cells (w[a] + w[b]) / 2.0, times the multiplier for a diagonal, fp64,
 *               one rounding per operation -- grid_to_csr's expression.  An edge of weight EXACTLY 0 is no edge: the reference
 *               walks graph[i].nonzero(), which drops stored zeros (two neighbouring cells of cost 0 are not connected).
 *   g_dev       f64 [n][max_cells]: the cost-to-go field from the source, +inf in obstacles and unreached cells; BIT-EQUAL to the
 *               reference's g_score where that has closed the cell (it is the fixed point of g[v] = min_u fl(g[u] + e(u, v))
 *               whatever the order of relaxation).  Entries past H * W are not written.
 *   path_dev    i32 [n][max_path]: the cells from source to target, -1 past the end; path_len_dev i32 [n]: the path's FULL
 *               length in cells (> max_path: T2D_GRID_TRUNCATED, the first max_path cells are written); the reference's path in
 *               every case: the predecessor of v is the neighbour u with fl(g[u] + e(u, v)) == g[v] and the smallest (g[u], u),
 *               which is the order the reference's heap of (g, index) tuples closes nodes in.
 *   status_dev  i32 [n]: T2D_GRID_*; sweeps_dev i32 [n]: the relaxation rounds the grid took.
 * BUILD-DEFINED, per row, touching only that row: T2D_GRID_INVALID (field +inf over H * W, no path, 0 sweeps) where H or W is
 * not positive or H * W is above max_cells, where source or target is out of range or an obstacle (also when
 * target == source, where the reference returns the one-point path before it looks at the grid), or where a weight is negative.  max_iter is not modelled:
 * the kernel always finishes, after at most H * W rounds.  Where a sum absorbs an edge (fl(g + e) == g) the candidates are
 * further restricted to (g[u], u) < (g[v], v), and a chain that does not reach the source gives T2D_GRID_NO_PATH.
 * T2D_ERR_GEOMETRY, nothing launched: max_cells above T2D_GRID_MAX_CELLS, the cap of the LDS form (two fp64 planes of 32 KiB,
 * two workgroups per CU).  T2D_ERR_INVALID, nothing launched: n < 0, max_cells < 1, max_path < 0, another connectivity, a
 * multiplier that is negative or not finite, a null or misaligned pointer (path_dev may be NULL when max_path is 0).          */
#define T2D_GRID_FOUND 0
#define T2D_GRID_NO_PATH 1
#define T2D_GRID_TRUNCATED 2
#define T2D_GRID_INVALID 3
#define T2D_GRID_FIELD_ONLY 4
#define T2D_GRID_MAX_CELLS 4096
int t2d_grid_dijkstra(int32_t device_id, int32_t n, const double* weight_dev, const int32_t* hw_dev, const int32_t* source_dev,
                      const int32_t* target_dev, int32_t max_cells, int32_t connectivity, double diagonal_cost_multiplier,
                      int32_t max_path, double* g_dev, int32_t* path_dev, int32_t* path_len_dev, int32_t* status_dev,
                      int32_t* sweeps_dev, void* hip_stream);

/* Grid A* on the device -- search/a_star.py: AStar.plan_graph (:279-404; AStar.plan :23-276 is the same loop) over the graph of
 * search/graph_utils.py: grid_to_csr, for n independent queries in ONE launch, asynchronous on hip_stream, no pool
 * (tests/astar_ref.py).  One wave runs one query.  The rule is the reference's, decision for decision: pop the
 * open entry with the smallest (f, cell); a popped entry whose cell is closed costs one iteration and does nothing else; close
 * the cell, test it against the target; relax every neighbour that is not closed with fl(g[cur] + e(cur, nb)), e being
 * t2d_grid_dijkstra's edge expression (an edge of weight exactly 0 is no edge): a STRICTLY smaller sum sets came_from, g and
 * f = fl(g + fl(heuristic_scale * h)) and pushes (f, nb); the loop runs while the open set is not empty and i < max_iter.
 *   weight_dev, hw_dev, source_dev, target_dev, max_cells, connectivity, diagonal_cost_multiplier, max_path: t2d_grid_dijkstra's
 *                layout and meaning; a target is required (no field-only call)
 *   heuristic_kind  one per launch; fp64, one rounding per operation, dx = x - hx, dy = y - hy for the cell (x, y) = (col, row):
 *                T2D_ASTAR_H_ZERO 0; T2D_ASTAR_H_EUCLIDEAN sqrt(dx dx + dy dy) (correctly rounded); T2D_ASTAR_H_MANHATTAN
 *                |dx| + |dy|; T2D_ASTAR_H_OCTILE hi + (diagonal_cost_multiplier - 1.0) * lo with hi / lo the larger / smaller of
 *                |dx|, |dy|; T2D_ASTAR_H_TABLE h_dev f64 [n][max_cells], one value per cell, the caller's
 *   htarget_dev  f64 [n][2]: the point (hx, hy) in cell units the built-in kinds measure against -- NOT the target cell: AStar.plan
 *                measures against the unrounded target.  May be NULL for ZERO and TABLE; h_dev may be NULL unless TABLE.
 *   heuristic_scale  f = g + heuristic_scale * h; the product is always formed (exact at 1.0): weighted A*
 *   max_iter     the reference's; a value <= 0 pops nothing
 *   cell_size, origin_x / origin_y: path_xy only, as in t2d_hybrid_astar
 *   workspace_dev, workspace_bytes: at least t2d_grid_astar_workspace_bytes(n, max_cells, connectivity) bytes, 16-byte aligned,
 *                contents irrelevant before and after: per cell the f of each push (one per neighbour), scale * h, g, came_from
 *   path_dev     i32 [n][max_path]: the cells from source to target, -1 past the end; path_len_dev i32 [n]: the FULL length
 *                (0 without a path); path_xy_dev f64 [n][max_path][2] or NULL: origin + (col, row) * cell_size, NaN past the end
 *                (t2d_polyline_routes takes it as it is)
 *   status_dev   i32 [n]: T2D_GRID_FOUND, _NO_PATH (the open set ran empty), _MAX_ITER (i reached max_iter with entries left),
 *                _TRUNCATED (the path is longer than max_path; its first max_path cells are written), _INVALID
 *   iterations_dev i32 [n]: the reference's i when it returns (the final pop of a found target is not counted, stale pops are);
 *                expanded_dev i32 [n]: the closed cells
 *   g_dev f64 / closed_dev u8 / parent_dev i32 [n][max_cells], each may be NULL: g_score, closed and came_from (-1: none) as they
 *                stand at termination -- the state of the reference's last callback; tentative g of open cells included, +inf
 *                where a cell was never reached.  Entries past H * W are not written.
 * There is NO overflow status: a neighbour pushes a cell only when it closes, and closes once, so a cell never holds more than
 * `connectivity` entries; the workspace has room for exactly that.
 * BUILD-DEFINED, per row, touching only that row: T2D_GRID_INVALID (g +inf, nothing closed, no parent over H * W, no path, 0
 * iterations) where H or W is not positive or H * W is above max_cells (then nothing of g / closed / parent is written), where
 * source or target is out of range or an obstacle, where a weight is negative, where h of a cell of the grid is NaN or -inf
 * or heuristic_scale * h is NaN (0 * inf), where htarget is not finite (built-in kinds), where heuristic_scale is negative or
 * not finite (every row).  +inf in a table is legal: such entries order by cell.  source == target is searched like any
 * query: the first pop finds it (path of one cell, 0 iterations, 1 closed cell); AStar.plan answers it before any launch.
 * T2D_ERR_GEOMETRY, nothing launched: max_cells above T2D_GRID_MAX_CELLS (one fp64 key, a closed bit and a counter byte per
 * cell in LDS: 36.5 KiB at the cap).  T2D_ERR_INVALID, nothing launched: n < 0, max_cells < 1, max_path < 0, another
 * connectivity, a multiplier that is negative or not finite, an unknown heuristic_kind, cell_size not in 1e-150 .. 1e150, an
 * origin that is not finite, a null or misaligned pointer (path_dev may be NULL when max_path is 0), a workspace smaller than
 * t2d_grid_astar_workspace_bytes (which returns -1 for arguments out of range).                                                */
#define T2D_GRID_MAX_ITER 5
#define T2D_ASTAR_H_ZERO 0
#define T2D_ASTAR_H_EUCLIDEAN 1
#define T2D_ASTAR_H_MANHATTAN 2
#define T2D_ASTAR_H_OCTILE 3
#define T2D_ASTAR_H_TABLE 4
int64_t t2d_grid_astar_workspace_bytes(int32_t n, int32_t max_cells, int32_t connectivity);
int t2d_grid_astar(int32_t device_id, int32_t n, const double* weight_dev, const int32_t* hw_dev, const int32_t* source_dev,
                   const int32_t* target_dev, int32_t max_cells, int32_t connectivity, double diagonal_cost_multiplier,
                   int32_t heuristic_kind, const double* htarget_dev, const double* h_dev, double heuristic_scale, int32_t max_iter,
                   int32_t max_path, double cell_size, double origin_x, double origin_y, void* workspace_dev, int64_t workspace_bytes,
                   int32_t* path_dev, int32_t* path_len_dev, double* path_xy_dev, int32_t* status_dev, int32_t* iterations_dev,
                   int32_t* expanded_dev, double* g_dev, uint8_t* closed_dev, int32_t* parent_dev, void* hip_stream);

/* Hybrid A* on the device -- search/hybrid_a_star.py: HybridAStar.plan (:58-172) for n independent queries in ONE launch,
 * asynchronous on hip_stream, no pool (tests/hybrid_astar_ref.py).  One wave runs one query: the pops are the
 * reference's (the smallest (f, node index) of the open entries, every pop expands, no closed set), the primitives are taken in
 * the order of `delta`, the prune against the cost grid is sequential (an earlier primitive of the same expansion wins its cell).
 *   weight_dev   f64 [n][max_cells], hw_dev i32 [n][2]: the obstacle grids in t2d_grid_dijkstra's layout; a cell that is +inf or
 *                NaN is an obstacle: the CLOSED square of side cell_size centred at origin + (col, row) * cell_size.  A segment
 *                collides when the slab test of the reference's own checker (tests/test_search.py: create_grid_collision_checker,
 *                its 1e-9 degenerate-axis branches, its divisions and its t_min <= t_max) passes for an obstacle; it is evaluated
 *                over the cells whose centre lies in the segment's bounding box grown by 1.5 cells, which gives the full loop's answer.
 *   start_dev / target_dev f64 [n][3]: x, y, heading; boundary_dev f64 [n][4]: x_min, x_max, y_min, y_max
 *   delta_dev    f64 [n_steer]: tan(steer) / wheelbase * step_size per steering angle, computed by the CALLER with its libm (tan
 *                never runs on the device); n_steer 1 .. T2D_HYBRID_MAX_STEER
 *   step_size    xy_res = step_size * 0.5, heading_res = pi / 8 (16 heading cells), x_cells = int((x_max - x_min) / xy_res) + 1;
 *                state_to_grid truncates, its heading is heading mod 2 pi as Python computes it, its index clamped to 15
 *   max_iter     pops before T2D_HYBRID_MAX_ITER; max_nodes: the nodes a query may append (its share of the workspace)
 *   workspace_dev, workspace_bytes: at least t2d_hybrid_astar_workspace_bytes(n, max_nodes) bytes, 16-byte aligned, contents
 *                irrelevant before and after: per query the nodes (40 bytes each) and the cost grid (1 MiB)
 *   path_dev     f64 [n][max_path][3]: the states from start to goal, NaN past the end (all NaN without a path); headings are NOT
 *                reduced to [0, 2 pi) -- neither are the reference's; path_len_dev i32 [n]: the FULL length (0 without a path)
 *   status_dev   i32 [n]: T2D_HYBRID_*; iterations_dev i32 [n]: the pops; nodes_dev i32 [n]: the nodes appended, the start included
 * cos / sin are the deterministic sincos of this library (the reference's libm differs in the last bit of some results): the
 * kernel equals tests/hybrid_astar_ref.py bit for bit, and that equals the reference on its recorded fixture.
 * The goal test is the reference's: |x - tx| < xy_res, |y - ty| < xy_res, |heading - t_heading| < heading_res, strict, on the
 * UNNORMALISED heading (a state that has turned through a full circle is not at the goal).  The start is neither
 * collision-checked nor bounds-checked, as there.  velocity is unused there and absent here.
 * BUILD-DEFINED, per row, touching only that row: T2D_HYBRID_INVALID where a pose, the boundary or a delta is not finite (x, y and
 * the boundary above 1e150, a heading or a delta above 1e9 in magnitude count as not finite), where x_min >= x_max or
 * y_min >= y_max, where the start's state_to_grid cell lies outside the cost grid (the reference raises IndexError or wraps a
 * negative index), where H or W is not positive or H * W is above max_cells.  T2D_HYBRID_OVERFLOW -- no path reported, never a
 * wrong one -- where an expansion would need more than max_nodes nodes, more than T2D_HYBRID_MAX_OPEN open entries (LDS), a depth
 * of 65535 (the cost grid holds a node's depth in 16 bits: g is the running sum of `depth` copies of step_size, strictly
 * increasing, so the comparison of depths is the comparison of costs), or where x_cells * y_cells is above
 * T2D_HYBRID_MAX_XY_CELLS.  T2D_HYBRID_TRUNCATED: the path is longer than max_path, its first max_path states are written.
 * T2D_ERR_INVALID, nothing launched: n < 0, max_cells < 1, max_path < 0, max_nodes < 1, n_steer outside 1 .. 16, step_size or
 * cell_size not in 1e-150 .. 1e150 (so <= 0, NaN and inf), an origin that is not finite, a null or misaligned pointer (path_dev
 * may be NULL when max_path is 0), a workspace smaller than t2d_hybrid_astar_workspace_bytes (which returns -1 for n < 0 or
 * max_nodes < 1).                                                                                                             */
#define T2D_HYBRID_FOUND 0
#define T2D_HYBRID_NO_PATH 1
#define T2D_HYBRID_MAX_ITER 2
#define T2D_HYBRID_TRUNCATED 3
#define T2D_HYBRID_OVERFLOW 4
#define T2D_HYBRID_INVALID 5
#define T2D_HYBRID_MAX_OPEN 2048
#define T2D_HYBRID_MAX_XY_CELLS 32768
#define T2D_HYBRID_MAX_STEER 16
int64_t t2d_hybrid_astar_workspace_bytes(int32_t n, int32_t max_nodes);
int t2d_hybrid_astar(int32_t device_id, int32_t n, const double* weight_dev, const int32_t* hw_dev, int32_t max_cells,
                     const double* start_dev, const double* target_dev, const double* boundary_dev, const double* delta_dev,
                     int32_t n_steer, double step_size, double cell_size, double origin_x, double origin_y, int32_t max_iter,
                     int32_t max_nodes, int32_t max_path, void* workspace_dev, int64_t workspace_bytes, double* path_dev,
                     int32_t* path_len_dev, int32_t* status_dev, int32_t* iterations_dev, int32_t* nodes_dev, void* hip_stream);

/* Sampling planners on the device -- search/rrt.py: RRT.plan (:74-164), search/rrt_star.py: RRTStar.plan (:88-201) with
 * _choose_parent (:22-37), search/rrt_connect.py: RRTConnect.plan (:72-206) -- for n independent queries of ONE kind in ONE launch,
 * asynchronous on hip_stream, no pool (tests/sample_plan_ref.py).  One wave runs one query.  Every iteration
 * draws rx, ry, takes the tree's node nearest to them (the FIRST minimum of dx dx + dy dy), steers (the sample itself where
 * sqrt(dx dx + dy dy) < extension_step, else nearest + extension_step * d / dist), goes on to the next iteration unless the new
 * point lies in the closed boundary and the segment nearest -> new is free, and appends.  np.hypot and np.linalg.norm are
 * sqrt(dx dx + dy dy) here; fp64, one rounding per operation.
 *   T2D_SAMPLE_RRT          after an append: where sqrt(|new - target|^2) < extension_step and the segment new -> target is free,
 *                           the target is appended and the search ends.  The path is the walk from the start to the LAST node
 *                           appended IN EVERY CASE (rrt.py:147): when max_iter runs out it is not empty, whatever the docstring says.
 *   T2D_SAMPLE_RRT_STAR     the parent is the smallest (cost, index) among the nodes within `radius` (d2 <= radius * radius) whose
 *                           segment to the new point is free, taken only where its cost is STRICTLY below the nearest node's;
 *                           every other node within the radius whose segment is free and whose cost exceeds the new node's cost
 *                           plus the distance is given the new node as parent and that cost; its descendants KEEP their costs.
 *                           The tree's coordinates are RRT's for the same draws.  The end and the path are RRT's.
 *   T2D_SAMPLE_RRT_CONNECT  tree a from the start, tree b from the target; even iterations extend a, odd ones b (the draw is taken
 *                           in both); after an append ONE segment, new -> the node of the other tree nearest to it, is tested: free,
 *                           the path is a's walk followed by b's walk reversed.  max_iter: no path.
 *   weight_dev, hw_dev, max_cells, cell_size, origin_x / origin_y: the obstacle grids and the collision test of t2d_hybrid_astar
 *   start_dev / target_dev f64 [n][2]; boundary_dev f64 [n][4]: x_min, x_max, y_min, y_max
 *   seed_dev     u64 [n]: draw k of query e is the top 53 bits of splitmix64's finaliser of seed[e] + (k + 1) * 0x9E3779B97F4A7C15
 *                as a uniform u in [0, 1) (the stream of t2d_generate_tracks); iteration i takes rx = x_min + (x_max - x_min) * u
 *                from draw 2 i and ry from draw 2 i + 1, whether or not it appends: np.random.uniform's formula on the build's stream
 *   max_iter     iterations before T2D_SAMPLE_MAX_ITER; max_nodes: the nodes of a query, both trees of RRT-Connect together
 *   workspace_dev, workspace_bytes: at least t2d_sample_plan_workspace_bytes(n, max_nodes) bytes, 16-byte aligned.  It holds the
 *                TREES, an output: query e's row starts at e * (workspace bytes / n) and holds x, y f64 [max_nodes][2], then cost
 *                f64 [max_nodes] (RRT* only, else not written), then parent i32 [max_nodes] (an index within the node's own tree,
 *                -1 for a root).  Tree a's node i is entry i; RRT-Connect's tree b's node j is entry max_nodes - 1 - j.
 *   path_dev     f64 [n][max_path][2], NaN past the end; path_len_dev i32 [n]: the FULL length
 *   status_dev   i32 [n]: T2D_SAMPLE_*; iterations_dev i32 [n]: the loop iterations begun; nodes_dev i32 [n][2]: the nodes of tree a
 *                and of tree b (0 for the other two kinds)
 * The start is neither bounds- nor collision-checked, as in the reference.  callback is not modelled.
 * BUILD-DEFINED, per row, touching only that row: T2D_SAMPLE_INVALID (no node, no path) where a coordinate of the start, the target
 * or the boundary is not finite (above 1e150 in magnitude counts as not finite), where H or W is not positive or H * W is above
 * max_cells.  A boundary with min > max is NOT invalid: as in the reference no new point lies in it, and the row ends with
 * T2D_SAMPLE_MAX_ITER.  T2D_SAMPLE_OVERFLOW -- no path reported, never a wrong one -- where an append would exceed max_nodes.
 * T2D_SAMPLE_TRUNCATED: a path was found and is longer than max_path, its first max_path points are written; the walk of a
 * T2D_SAMPLE_MAX_ITER row is cut the same way and keeps its status (path_len > max_path tells).  The first
 * T2D_SAMPLE_LDS_NODES nodes' coordinates are also kept in LDS (for RRT-Connect half of them per tree); nothing depends on it.
 * T2D_ERR_INVALID, nothing launched: an unknown kind, n < 0, max_cells < 1, max_path < 0, max_nodes < 1, max_iter < 0,
 * extension_step or cell_size not in 1e-150 .. 1e150 (so <= 0, NaN and inf), a radius that is negative or NaN, an origin that is
 * not finite, a null or misaligned pointer (path_dev may be NULL when max_path is 0), a workspace smaller than
 * t2d_sample_plan_workspace_bytes (which returns -1 for n < 0 or max_nodes < 1).                                               */
#define T2D_SAMPLE_RRT 0
#define T2D_SAMPLE_RRT_STAR 1
#define T2D_SAMPLE_RRT_CONNECT 2
#define T2D_SAMPLE_FOUND 0
#define T2D_SAMPLE_MAX_ITER 1
#define T2D_SAMPLE_TRUNCATED 2
#define T2D_SAMPLE_OVERFLOW 3
#define T2D_SAMPLE_INVALID 4
#define T2D_SAMPLE_LDS_NODES 512
int64_t t2d_sample_plan_workspace_bytes(int32_t n, int32_t max_nodes);
int t2d_sample_plan(int32_t device_id, int32_t n, int32_t kind, const double* weight_dev, const int32_t* hw_dev, int32_t max_cells,
                    const double* start_dev, const double* target_dev, const double* boundary_dev, const uint64_t* seed_dev,
                    double extension_step, double radius, double cell_size, double origin_x, double origin_y, int32_t max_iter,
                    int32_t max_nodes, int32_t max_path, void* workspace_dev, int64_t workspace_bytes, double* path_dev,
                    int32_t* path_len_dev, int32_t* status_dev, int32_t* iterations_dev, int32_t* nodes_dev, void* hip_stream);

/* Probabilistic roadmaps on the device -- search/prm.py: PRM.plan (:52-344) -- for n independent queries in ONE launch, asynchronous
 * on hip_stream, no pool (tests/prm_ref.py).  One workgroup runs one query; fp64, one rounding per operation.
 *   nodes        node 0 is the start, node 1 the target, node 2 + s is (x_min + (x_max - x_min) * u(2 s), y_min + (y_max - y_min) *
 *                u(2 s + 1)) with u(k) draw k of the row's stream (seed_dev as t2d_sample_plan takes it).  N = n_samples + 2 <=
 *                T2D_PRM_MAX_NODES.  A sample is NOT collision-checked, as in the reference: a node inside an obstacle stays, isolated.
 *   neighbours   connection_radius == 0: of node i the min(k_nearest + 1, N) smallest dx dx + dy dy in the order (d2, index), i
 *                itself dropped, ascending.  connection_radius > 0: every j != i with sqrt(d2) <= connection_radius in ascending j;
 *                a node with more than max_degree of them makes the row T2D_PRM_OVERFLOW.  Only j > i becomes a candidate edge: an
 *                edge exists because j is near i, not because i is near j (the reference's asymmetry, restated).
 *   edges        a candidate whose segment touches no obstacle cell (the collision test of t2d_hybrid_astar) is an edge of cost
 *                sqrt(dx dx + dy dy) of nodes[i] - nodes[j]; the list is ordered by i, within i in the neighbour order.
 *   search       g[0] = 0, g[v] = min(g[v], fl(g[u] + w)) over both directions of every edge until nothing changes: every sweep
 *                reads the field of the sweep before it, sweeps_dev counts them, the last one -- which changes nothing -- included.
 *                The predecessor of v is the u with the smallest (g[u], u) among the neighbours with fl(g[u] + w) == g[v] and
 *                g[u] < g[v] -- or, at equal g (an edge of cost 0 between coincident nodes), u given its value in an earlier
 *                sweep than v, so that every walk ends at the start; the path is the walk back from node 1.
 *   workspace_dev, workspace_bytes: at least t2d_prm_plan_workspace_bytes(n, n_samples, k) bytes, 16-byte aligned, k being k_nearest
 *                or, in radius mode, max_degree.  It holds the ROADMAP, an output: with K = min(k, N - 1) and E = N * K, query e's
 *                row starts at e * (workspace bytes / n) and holds the nodes f64 [N][2], dist f64 [N] (the cost from the start to
 *                every node, +inf where not connected), edge_cost f64 [E], edge_ij i32 [E][2] (the first n_edges entries of each
 *                are written), then scratch i32 [E].
 *   path_dev     f64 [n][max_path][2] from the start to the target, NaN past the end; path_len_dev i32 [n]: the FULL length
 *   status_dev   i32 [n]: T2D_PRM_*; n_edges_dev i32 [n]; sweeps_dev i32 [n]
 * callback and max_iter are not modelled: the search is always finished.
 * BUILD-DEFINED, per row, touching only that row: T2D_PRM_INVALID (nothing of the roadmap written, no path) where a coordinate of
 * the start, the target or the boundary is not finite (above 1e150 in magnitude counts as not finite), where x_min >= x_max or
 * y_min >= y_max, where the start or the target lies outside the closed boundary grown by 1e-9, where H or W is not positive or
 * H * W is above max_cells -- the cases in which the reference raises.  T2D_PRM_OVERFLOW (the nodes written, no edge, no path):
 * radius mode only.  T2D_PRM_NO_PATH: the roadmap does not connect start and target; dist is written.  T2D_PRM_TRUNCATED:
 * path_len > max_path, the first max_path points are written.  Among exactly coincident nodes the smaller index is the nearer.
 * T2D_ERR_INVALID, nothing launched: n < 0, max_cells < 1, max_path < 0, n_samples outside 1 .. T2D_PRM_MAX_NODES - 2, a
 * connection_radius that is negative, NaN or infinite, k_nearest outside 1 .. T2D_PRM_MAX_K in k-nearest mode, max_degree < 1 in
 * radius mode, cell_size not in 1e-150 .. 1e150, an origin that is not finite, a null or misaligned pointer (path_dev may be NULL
 * when max_path is 0), a workspace smaller than t2d_prm_plan_workspace_bytes (which returns -1 for arguments out of range).     */
#define T2D_PRM_FOUND 0
#define T2D_PRM_NO_PATH 1
#define T2D_PRM_TRUNCATED 2
#define T2D_PRM_OVERFLOW 3
#define T2D_PRM_INVALID 4
#define T2D_PRM_MAX_NODES 1024
#define T2D_PRM_MAX_K 16
int64_t t2d_prm_plan_workspace_bytes(int32_t n, int32_t n_samples, int32_t k_or_degree);
int t2d_prm_plan(int32_t device_id, int32_t n, const double* weight_dev, const int32_t* hw_dev, int32_t max_cells,
                 const double* start_dev, const double* target_dev, const double* boundary_dev, const uint64_t* seed_dev,
                 int32_t n_samples, int32_t k_nearest, double connection_radius, int32_t max_degree, double cell_size,
                 double origin_x, double origin_y, int32_t max_path, void* workspace_dev, int64_t workspace_bytes, double* path_dev,
                 int32_t* path_len_dev, int32_t* status_dev, int32_t* n_edges_dev, int32_t* sweeps_dev, void* hip_stream);

/* The occupancy grid of every env's CURRENT scene, in the layout t2d_grid_dijkstra, t2d_hybrid_astar and t2d_sample_plan read in
 * place: ONE launch, asynchronous on hip_stream (enqueued behind a step on the same stream it sees that step).  The reference has no
 * counterpart; the rule is build-defined (tests/occupancy_ref.py).
 *   window      shared by the batch: H x W cells; cell (row, col) is the CLOSED square of side cell_size centred at
 *               (origin_x + col * cell_size, origin_y + row * cell_size)
 *   rule        a cell is OCCUPIED iff the Euclidean distance between it and some listed obstacle, as a closed filled set, is
 *               <= inflate (0: touches or overlaps; containment either way counts).  fp64 on the fp32 scene data, no division; a cell
 *               at a distance <= inflate is always occupied, an occupied cell lies within inflate + 2^-42 * (the largest
 *               coordinate in play) -- rounding can only add cells.
 *   listed      the env's static rings (t2d_set_static_geometry, undivided; the live quads of a generated scene) and, with
 *               include_participants, every ACTIVE participant except slot exclude_slot (-1: none excepted): its oriented box
 *               T2D_P_LENGTH x T2D_P_WIDTH about its pose, corners centre +- L/2 (c, s) +- W/2 (-s, c) with the library's deterministic
 *               (s, c) of the heading, or, for T2D_SHAPE_CIRCLE, the disc of radius width / 2
 *   weight_dev  f64 [n_env][H * W] row-major: free_weight (finite, >= 0) in free cells, +inf in occupied ones; mask_dev u8
 *               [n_env][H][W]: 1 = occupied.  Either may be NULL, not both.  hw_dev i32 [n_env][2] (may be NULL): (H, W);
 *               status_dev i32 [n_env] (may be NULL): T2D_OCC_*
 *   format      0, or T2D_OCC_FORMAT_NAIVE: every cell tests every listed element (the measurement yardstick; the same grid)
 * BUILD-DEFINED, per row, touching only that row: a listed participant whose x, y or heading is not finite makes the row
 * T2D_OCC_INVALID and EVERY cell of it an obstacle; an inactive participant and a ring of fewer than 3 vertices are ignored.
 * T2D_ERR_INVALID, nothing launched: H or W < 1 (or more tiles than a launch holds), cell_size outside 1e-150 .. 1e150, inflate
 * outside 0 .. 1e150, an origin that is not finite, a free_weight that is negative or not finite, exclude_slot outside
 * -1 .. max_agents - 1, an unknown format bit, both outputs NULL, weight_dev not 16-byte or another pointer not 4-byte aligned.
 * T2D_ERR_STATE: include_participants before t2d_set_param_table and t2d_reset.  H * W is not capped by T2D_GRID_MAX_CELLS.
 * kernel_id T2D_PROFILE_OCCUPANCY in t2d_profile_read.                                                                          */
#define T2D_OCC_OK 0
#define T2D_OCC_INVALID 1
#define T2D_OCC_FORMAT_NAIVE 1
enum { T2D_PROFILE_OCCUPANCY = 21 };
int t2d_occupancy_grid(t2d_pool* pool, int32_t H, int32_t W, double cell_size, double origin_x, double origin_y, double inflate,
                       int32_t include_participants, int32_t exclude_slot, double free_weight, double* weight_dev, uint8_t* mask_dev,
                       int32_t* hw_dev, int32_t* status_dev, int32_t format, void* hip_stream);

/* Following a Reeds-Shepp plan: the parking tutorial's RSAgent (docs/tutorial/train_parking_demo.ipynb cell 17) with the
 * PIDController and rear_center_coord of cell 14, for the ego of every env, in ONE launch in front of the step launch.  It takes
 * over the action row of an env while a path is being executed and leaves the policy's row alone otherwise.
 *
 * State per env, struct-of-arrays in pool-owned device memory (one array per field, contiguous over envs): the adopted
 * segments (at most T2D_RS_MAX_SEGMENTS: steer +1 / 0 / -1, signed distance, target point x / y / yaw, arc centre, start
 * point) with the index of the head, the last distance_to_go (+inf: none), and prev_error / integral / target of the velocity,
 * acceleration and steer controller.  One call does for env e, in this order:
 *   1. episode end = agent.reset(): if the env's status word left by the last step says terminated or truncated (the
 *      condition of t2d_restore(mode 1) and of the fused auto-reset, which keeps that status readable until the next step),
 *      path, last distance and the controllers' prev_error / integral are cleared.
 *   2. adopt = RSAgent.plan -> calculate_target_points: if no path is held and the env's plan record reads T2D_RS_FOUND with
 *      1 .. T2D_RS_MAX_SEGMENTS segments, the target points are chained over steer[i] / distance[i] from the ego's pose moved to
 *      the rear axle by dr, with the notebook's three branches as written.  While a path is held the record is not read.
 *   3. act = RSAgent.get_action: distance_to_go d to the head's target; the head is popped if d < reach_radius or (last < d and
 *      d < rising_radius), once per call (last := +inf on a pop, else d); nothing left: the action is (0, 0) and the path is
 *      finished.  Otherwise velocity PID on -d * sign(distance) clipped to +-max_speed, acceleration PID on the speed clipped to
 *      +-max_acceleration, arc or line error + yaw_weight * wrapped yaw error, steer PID, steer * steer_ratio + delta clipped to
 *      +-1; the normalised action is (target_steer, target_a / max_acceleration).  Controller state survives pops and a path's
 *      end; only 1. clears it.
 *   4. the action row (steering, accel): executing -> the normalised action through the tutorial wrapper's _preprocess_action for
 *      the symmetric box (+-steer_bound, +-accel_bound) in fp32 and in its order (round to fp32, clip to +-1,
 *      * (high - low) / 2 + (high + low) / 2); otherwise the policy's row, bit for bit.
 * All arithmetic is fp64 on the pool's fp32 state columns, with the library's own sincos / atan2.
 * BUILD-DEFINED: (a) a non-finite x / y / heading / speed of an active ego, or a computed action that is not finite (the
 * notebook's zero-length S segment divides 0 by 0 when it is the head), drops the env's path, raises T2D_RS_FOLLOW_DROPPED and
 * passes the policy's row through; the controllers keep the state they had before that call: a NaN never reaches the step from
 * here.  (b) an inactive ego neither adopts nor acts.  (c) there is no timeout: a follower that never reaches its target keeps
 * executing until the episode ends, as the notebook's does; t2d_rs_follow_reset with a mask drops paths.
 *   t2d_rs_follow_config   all values finite; radius, max_speed, max_acceleration, reach_radius, rising_radius, steer_bound,
 *                          accel_bound > 0 (T2D_ERR_INVALID otherwise); T2D_ERR_STATE before t2d_rs_config.  Allocates and clears
 *                          the state and the pool's own records.
 *   t2d_rs_follow          one launch, asynchronous on hip_stream, no host synchronisation.  plan_dev: t2d_rs_plan_record [n_env]
 *                          or NULL = the pool's own plan records; act_in_dev / act_out_dev: f32 [n_env][2] (steering, accel),
 *                          may be the same memory; act_in_dev NULL = zeros; out_dev: t2d_rs_follow_record [n_env] (8-byte
 *                          aligned) or NULL = the pool's own.  T2D_ERR_STATE before t2d_rs_follow_config or t2d_reset,
 *                          T2D_ERR_INVALID without act_out_dev.  kernel_id T2D_PROFILE_RS_FOLLOW in t2d_profile_read.
 *   t2d_rs_follow_reset    agent.reset() for the envs whose mask byte (device memory) is non-zero, NULL = all; asynchronous on
 *                          hip_stream.  A t2d_reset without a mask and t2d_parking_scenes do the same for every env.
 *   t2d_rs_follow_buffers  pointer and size in bytes of the pool's own records.                                          */
#define T2D_RS_FOLLOW_ADOPTED 1u       /* a plan was adopted in this call */
#define T2D_RS_FOLLOW_POP_REACHED 2u   /* the head was popped: d < reach_radius */
#define T2D_RS_FOLLOW_POP_RISING 4u    /* the head was popped: last < d < rising_radius */
#define T2D_RS_FOLLOW_FINISHED 8u      /* the last segment was popped: the action is (0, 0) */
#define T2D_RS_FOLLOW_RESET 16u        /* the episode ended in the last step: agent.reset() */
#define T2D_RS_FOLLOW_DROPPED 32u      /* non-finite input or result: the path was dropped */
#define T2D_PROFILE_RS_FOLLOW 14
typedef struct t2d_rs_follow_params {
    double radius;                  /* execute_radius: the planner's radius */
    double dr;                      /* rear axle behind the centre: the planner's center_shift */
    double steer_ratio;             /* 0.98 */
    double max_speed;               /* 0.5 */
    double max_acceleration;        /* 2.0 */
    double kp_v, ki_v, kd_v;        /* velocity controller: 0.8, 0, 0 */
    double kp_a, ki_a, kd_a;        /* acceleration controller: 2.0, 0, 0 */
    double kp_s, ki_s, kd_s;        /* steer controller: 5.0, 0, 0 */
    double yaw_weight;              /* 0.5 */
    double reach_radius;            /* 0.02 */
    double rising_radius;           /* 0.1 */
    double steer_bound, accel_bound;   /* the env's action box, rounded to fp32: 0.524, 2.0 */
} t2d_rs_follow_params;
typedef struct t2d_rs_follow_record {   /* 48 bytes */
    int32_t executing;              /* segments left after the call */
    int32_t segment;                /* index of the head within the adopted plan, -1 without a path */
    uint32_t events;                /* T2D_RS_FOLLOW_* of this call */
    int32_t steps;                  /* calls that acted on the path since its adoption, this one included */
    double action[2];               /* the normalised action (steer, accel), NaN when the policy's row went through */
    double distance_to_go;          /* to the head's target (to the last popped one in a finishing call), else NaN */
    double total_error;             /* what the steer controller saw, else NaN */
} t2d_rs_follow_record;
int t2d_rs_follow_config(t2d_pool* pool, const t2d_rs_follow_params* cfg);
int t2d_rs_follow(t2d_pool* pool, const t2d_rs_plan_record* plan_dev, const float* act_in_dev, float* act_out_dev,
                  t2d_rs_follow_record* out_dev, void* hip_stream);
int t2d_rs_follow_reset(t2d_pool* pool, const uint8_t* mask_dev, void* hip_stream);
int t2d_rs_follow_buffers(t2d_pool* pool, void** records_dev, size_t* nbytes);

/* Lane-keeping scripted traffic: the reference's PIDController (controller/pid_controller.py:15-470) for every controlled
 * participant of every env in ONE launch in front of the step launch.  The reference leaves cross_track_error, target_heading
 * and target_speed to its caller and ships no caller; here the caller is the build: the error is MEASURED against the
 * participant's installed route (t2d_set_routes).  The action rows it writes reach the step through t2d_bind_actions_strided,
 * as t2d_rs_follow's do; no stepping call launches the kernel, and a PID-controlled participant is not an IDM-controlled one.
 *
 * The law (the reference's, operation by operation in fp64; one rounding per operation):
 *   _compute_pid(error, state, kp, ki, kd, limits)   :159-234
 *       p = kp * error; raw = (error - prev_error) / dt (0.0 unless dt > 0); derivative = alpha * raw + (1 - alpha) *
 *       prev_derivative; out = p + kd * derivative; with limits: out beyond one of them is set to it and counts as saturated;
 *       integral += error * dt, or integral *= 0.99 when saturated; out += ki * integral; with limits: np.clip(out, min, max).
 *       New state: (integral, error, derivative).
 *   lateral (lat_mode != 0)   :333-375   error = the wrapped heading error atan2(sin(e), cos(e)), e = target_heading - heading
 *       (lat_mode 1; target_heading takes precedence over cross_track_error) or the cross-track error (lat_mode 2);
 *       _compute_pid WITHOUT limits (so anti-windup never acts on this side); lat_mode 2: steering = out * (2.0 / wheel_base),
 *       and with wheel_base <= 0 the steering is 0.0 although the lateral state has been updated already (the reference catches
 *       its own ValueError; in its "lateral" mode it re-raises -- here that participant's steering is 0.0 too and
 *       T2D_PID_BAD_WHEEL_BASE is raised); steering = np.clip(steering, -max_steering, max_steering).  lat_mode 0: steering 0.0.
 *   longitudinal, after the lateral side   :378-404   lon_mode 0: acceleration 0.0 (control_mode "lateral"); 1: _compute_pid on
 *       target_speed - speed with limits (min_accel, max_accel), clipped again; 2: the IDM law of t2d_set_idm row idm_row[i] with
 *       the leader rule of t2d_idm_actions (same operations, same bits); 3: the caller's acceleration (act_in) passed through.
 *   ("combined" = lat_mode 1 or 2 with lon_mode 1; "lateral" = lon_mode 0; "longitudinal" = lat_mode 0 with lon_mode 1.)
 *
 * The measurement (BUILD-DEFINED; tests/pid_ref.py restates it in numpy).  Position = the participant's centre (x, y), as in
 * t2d_off_route.  Over the segments A -> B of the participant's route in vertex order, zero-length segments skipped:
 * u = B - A, w = P - A, L2 = u.u, t = w.u; d2 = |w|^2 if t <= 0, |P - B|^2 if t >= L2, else (wx uy - wy ux)^2 / L2 -- the
 * arithmetic of t2d_off_route -- and the first strict minimum wins.  d = sqrt(d2min) (the bits of t2d_off_route's distance
 * before its fp32 cast); c = wx uy - wy ux of the winning segment; cross_track_error = +d if c > 0, -d if c < 0, else 0.0
 * (positive: the route lies to the LEFT of the vehicle along the direction of travel, so positive steering closes it);
 * target_heading = atan2(uy, ux) of the winning segment (the library's own atan2).  T2D_PID_ROUTE_END is raised, and nothing
 * else changes, when the winning segment is the route's last non-degenerate one and t >= L2 there (the nearest point is the
 * route's last vertex).  route_of = -1, or a route of zero-length segments only, is NO ROUTE: the reference's combined-mode
 * fallback -- steering 0.0, lateral state untouched -- with T2D_PID_NO_ROUTE.  A non-finite x / y / heading / speed (or
 * target_speed under lon_mode 1), or a non-finite steering or acceleration: the state stays as it was, the caller's row goes
 * through bit for bit and T2D_PID_NONFINITE is raised.  Inactive or uncontrolled participants: the caller's row, bit for bit.
 * Episode end (t2d_rs_follow's rule): an env whose status left by the last step says terminated or truncated has the state of
 * all its participants cleared (controller.reset()) at the start of the call, T2D_PID_RESET.
 *
 *   t2d_set_pid      ctrl_rows: host [n_ctrl][row_stride >= T2D_PID_COLS] fp64, 1 <= n_ctrl <= 254, validated as the
 *                    constructor validates (:87-102: dt <= 0, max_steering <= 0, max_accel <= 0, min_accel >= 0, max_accel <=
 *                    min_accel, alpha <= 0 or > 1 are refused; lat_mode in 0..2, lon_mode in 0..3).  wheel_base NaN = lf + lr of
 *                    the participant's type row.  ctrl_id u8[N] (T2D_PID_NONE: uncontrolled), target_speed f32[N] (NULL: zeros),
 *                    idm_row i32[N] (NULL: row 0; read under lon_mode 2 only).  T2D_ERR_INVALID for a participant that is IDM-
 *                    controlled as well (t2d_set_idm refuses the same afterwards), for one that is pursuit-controlled
 *                    (t2d_set_pursuit; t2d_set_idm refuses that too) and for an idm_row outside the installed rows;
 *                    T2D_ERR_STATE for lon_mode 2 without installed IDM rows.  A refused call changes nothing.  Clears the state
 *                    of every participant.  n_ctrl = 0 uninstalls and frees the installation's device memory, the pool's own
 *                    records included.
 *   t2d_pid_actions  one launch, asynchronous on hip_stream.  act_in_dev / act_out_dev: f32 [N][2] rows (steering, accel), may be
 *                    the same memory; act_in_dev is never written, NULL = zeros.  Controlled rows receive the fp32 rounding of the
 *                    fp64 action.  record_dev: t2d_pid_record [N] (8-byte aligned) or NULL = the pool's own.  T2D_ERR_STATE
 *                    before t2d_set_pid or t2d_reset, when no route set is installed although a row has lat_mode != 0, when trace
 *                    routes are the installed kind, and when a row has lon_mode 2 and the IDM rows it was installed against are
 *                    gone; T2D_ERR_INVALID without act_out_dev.  kernel_id T2D_PROFILE_PID in t2d_profile_read.
 *   t2d_pid_reset    controller.reset() for the envs whose mask byte (device memory) is non-zero, NULL = all; asynchronous.  A
 *                    t2d_reset without a mask does the same for every env.
 *   t2d_pid_state    the six fp64 state words of every participant, host array [N][6] in the order of T2D_PID_S_*: write = 0
 *                    reads them (after the pool's work), write != 0 replaces them.
 *   t2d_pid_buffers  pointer and size in bytes of the pool's own records, valid until the next t2d_set_pid (which replaces or
 *                    frees them).                                                                                             */
enum {
    T2D_PID_DT = 0,
    T2D_PID_KP_LAT = 1,
    T2D_PID_KI_LAT = 2,
    T2D_PID_KD_LAT = 3,
    T2D_PID_MAX_STEERING = 4,
    T2D_PID_KP_LON = 5,
    T2D_PID_KI_LON = 6,
    T2D_PID_KD_LON = 7,
    T2D_PID_MAX_ACCEL = 8,
    T2D_PID_MIN_ACCEL = 9,
    T2D_PID_ALPHA = 10,      /* derivative_filter_alpha */
    T2D_PID_LAT_MODE = 11,   /* build column: 0 none, 1 target_heading, 2 cross_track_error */
    T2D_PID_LON_MODE = 12,   /* build column: 0 acceleration 0.0, 1 PID on target_speed, 2 IDM law, 3 caller's acceleration */
    T2D_PID_WHEEL_BASE = 13, /* build column: the wheel_base kwarg; NaN = lf + lr of the type row */
    T2D_PID_COLS = 14
};
enum {
    T2D_PID_S_LAT_INTEGRAL = 0,
    T2D_PID_S_LAT_PREV_ERROR = 1,
    T2D_PID_S_LAT_PREV_DERIVATIVE = 2,
    T2D_PID_S_LON_INTEGRAL = 3,
    T2D_PID_S_LON_PREV_ERROR = 4,
    T2D_PID_S_LON_PREV_DERIVATIVE = 5,
    T2D_PID_STATE_WORDS = 6
};
#define T2D_PID_NONE 255
#define T2D_PID_ROUTE_END 1u    /* the nearest point of the route is its last vertex */
#define T2D_PID_NONFINITE 2u    /* non-finite input or result: state kept, the caller's row passed through */
#define T2D_PID_RESET 4u        /* the episode ended in the last step: controller.reset() */
#define T2D_PID_NO_ROUTE 8u     /* lat_mode != 0 without a route: steering 0.0, lateral state untouched */
#define T2D_PID_BAD_WHEEL_BASE 16u /* cross-track mode with wheel_base <= 0: lateral state updated, steering 0.0 */
#define T2D_PID_SATURATED 32u   /* the longitudinal PID saturated without its integral term (leaky integration) */
#define T2D_PROFILE_PID 15
typedef struct t2d_pid_record {     /* 48 bytes */
    double cross_track;             /* the measured cross_track_error (m), NaN without a measurement */
    double lat_error;               /* what the lateral PID saw (lat_mode 1: the wrapped heading error), NaN when it did not run */
    int32_t segment;                /* index of the winning segment within the route, -1 without a measurement */
    int32_t leader;                 /* lon_mode 2: agent index of the chosen leader, else -1 */
    uint32_t events;                /* T2D_PID_* of this call */
    uint32_t reserved;              /* 0 */
    double action[2];               /* the applied (steering, accel) in fp64, NaN when the caller's row went through */
} t2d_pid_record;
int t2d_set_pid(t2d_pool* pool, const double* ctrl_rows, int32_t n_ctrl, int32_t row_stride, const uint8_t* ctrl_id,
                const float* target_speed, const int32_t* idm_row);
int t2d_pid_actions(t2d_pool* pool, const float* act_in_dev, float* act_out_dev, t2d_pid_record* record_dev, void* hip_stream);
int t2d_pid_reset(t2d_pool* pool, const uint8_t* env_mask_dev, void* hip_stream);
int t2d_pid_state(t2d_pool* pool, double* state_host, int32_t write);
int t2d_pid_buffers(t2d_pool* pool, void** records_dev, size_t* nbytes);

/* Path-following scripted traffic: the reference's PurePursuitController (controller/pure_pursuit_controller.py:16-98) and
 * AccelerationController (controller/acceleration_controller.py:14-145; cruise and adaptive cruise, ACC) for every controlled
 * participant of every env in ONE launch in front of the step launch.  Both are stateless: there is no _reset, no _state and no
 * episode-end rule.  The rows written reach the step through t2d_bind_actions_strided, as t2d_pid_actions' do; no stepping
 * call launches the kernel; a participant has ONE of the IDM, PID and pursuit controllers.
 *
 * The law (the reference's, operation by operation in fp64; one rounding per operation; np.clip = two selects):
 *   cruise   :73-93    accel = (target_speed - speed) / kp   -- it DIVIDES by kp --;  accel = clip(accel, accel_last -
 *       accel_change_rate * delta_t, accel_last + accel_change_rate * delta_t); accel = clip(accel, min_accel, max_accel).
 *       accel_last = ego_state.accel = T2D_F_APPLIED0 of the participant, which is 0.0 after a reset (the reference's State
 *       holds None there and its arithmetic raises).  A reset is every episode start: t2d_reset (the selected envs) and
 *       t2d_restore write 0.0 into T2D_F_APPLIED0 / 1; after a step that restarts finished envs in its own launch
 *       (t2d_set_auto_reset, regenerated scenes) the column is left as it is and the call reads 0.0 for an env whose
 *       T2D_F_CNT_STEP is 0, until t2d_upload(T2D_F_APPLIED0) or t2d_integrate writes the column again.
 *       NOT the reference's State.accel property as it stands: that returns the NORM of the acceleration vector (accel *
 *       cos(heading), accel * sin(heading)) and is never negative, although both laws clip around it and down to min_accel < 0.
 *       Here accel_last and front.accel are the signed scalars the pool stores, and the fixture that pins the laws
 *       (tests/golden/make_pursuit.py) overrides that one property to hand the signed scalar out.
 *   ACC      :95-124   distance_front = hypot(dx, dy) to the leader; distance_target = clip(speed * interval + 5.0, 7.0, 80.0);
 *       relative_target_speed = (distance_target - distance_front) / kp; relative_accel = (relative_target_speed -
 *       (v_front - v)) / kp; accel = front.accel - relative_accel; then the same two clips.  front.accel / front.speed =
 *       T2D_F_APPLIED0 / T2D_F_SPEED of the leader; the leader is the one t2d_idm_actions' rule finds with this row's
 *       LANE_HALF_WIDTH and HORIZON (no IDM rows needed).  No leader: cruise, with T2D_PURSUIT_NO_LEADER.
 *       (speed_factor is set by update_driving_style and never read by the reference; it has no column.)
 *   pure pursuit  :53-98   pre_aiming_distance = max(speed * interval, min_pre_aiming_distance); pre_aiming_point = the
 *       waypoints interpolated at that distance; angle = atan2(dy, dx) to it, distance = sqrt(dy * dy + dx * dx);
 *       steering = atan(2.0 * wheel_base * sin(angle - heading) / distance).  No steering clip.
 *   sin, atan2 and atan are the library's own deterministic functions, hypot is sqrt(dx * dx + dy * dy).
 *
 * The waypoints (BUILD-DEFINED; tests/pursuit_ref.py restates them in numpy).  The reference interpolates from the START of
 * whatever line string its caller hands over (its source carries a "TODO: set an automatic reference point catcher").  Here
 * the line string is the rest of the participant's route from its projection onward.  Position = the participant's centre.
 * The projection is t2d_pid_actions' measurement exactly (same segment arithmetic, first strict minimum, zero-length segments
 * skipped; the record's cross-track error has the PID record's bits).  On the winning segment A -> B, u = B - A, w = P - A,
 * t = w.u clamped to [0, L2]: the start point is Q = A + u * (tc / L2).  The walk then covers rem = pre_aiming_distance
 * forward: per segment, v = (the segment's end) - cur, L = sqrt(vx * vx + vy * vy); if rem <= L and L > 0 the target is
 * cur + v * (rem / L); otherwise rem -= L, cur = the segment's end, and the walk goes on.  An open route that ends first gives
 * its last vertex (what shapely's interpolate gives beyond the length) with T2D_PURSUIT_ROUTE_END.  A route whose first and
 * last vertices are equal bit for bit is CLOSED: the walk continues from its first segment (T2D_PURSUIT_WRAPPED once it visits
 * one) and visits at most as many segments as the route has, the winning one first: a look-ahead longer than that ends at the
 * winning segment's start vertex with T2D_PURSUIT_ROUTE_END.  route_of = -1, or a route of zero-length segments only, is NO
 * ROUTE: steering 0.0 with T2D_PURSUIT_NO_ROUTE.
 *
 * Non-finite values.  A non-finite x, y, heading, speed or stored accel, or a non-finite target_speed under lon_mode 0 / 1,
 * passes the caller's row through bit for bit with T2D_PURSUIT_NONFINITE; so does a non-finite resulting steering or
 * acceleration (a look-ahead point that coincides with the position while the heading equals the bearing gives 0 / 0; kp = 0
 * is not refused, as the reference does not refuse it, and the IEEE result decides).  +-inf that the clips or atan make finite
 * is kept.  Inactive or uncontrolled participants: the caller's row, bit for bit.
 *
 *   t2d_set_pursuit      ctrl_rows: host [n_ctrl][row_stride >= T2D_PURSUIT_COLS] fp64, 1 <= n_ctrl <= 254; refused
 *                        (T2D_ERR_INVALID): min_pre_aiming <= 0 (the constructor's refusal), a non-finite column (wheel_base
 *                        may be NaN = lf + lr of the participant's type row, horizon may be +inf), lat_mode outside 0..1,
 *                        lon_mode outside 0..2, a negative or NaN target_speed of a controlled participant (the constructor's
 *                        refusal; +inf passes and is a non-finite input of the call), a ctrl_id without a row, a participant
 *                        that is IDM- or PID-controlled (t2d_set_idm and t2d_set_pid refuse the same afterwards).  ctrl_id
 *                        u8[N] (T2D_PURSUIT_NONE: uncontrolled), target_speed f32[N] (NULL: zeros).  A refused call changes
 *                        nothing.  n_ctrl = 0 uninstalls and frees the installation's device memory, the pool's own
 *                        records included.
 *   t2d_pursuit_actions  one launch, asynchronous on hip_stream.  act_in_dev / act_out_dev: f32 [N][2] rows (steering, accel),
 *                        may be the same memory; act_in_dev is never written, NULL = zeros.  Controlled rows receive the fp32
 *                        rounding of the fp64 action.  record_dev: t2d_pursuit_record [N] (8-byte aligned) or NULL = the
 *                        pool's own.  T2D_ERR_STATE before t2d_set_pursuit or t2d_reset, when a row has lat_mode 1 and no
 *                        route set is installed, when trace routes are the installed kind, and when a row has lon_mode 0 / 1
 *                        while t2d_set_outputs has switched T2D_OUT_APPLIED off (accel_last would be stale);
 *                        T2D_ERR_INVALID without act_out_dev.  kernel_id T2D_PROFILE_PURSUIT in t2d_profile_read.
 *   t2d_pursuit_buffers  pointer and size in bytes of the pool's own records, valid until the next t2d_set_pursuit (which
 *                        replaces or frees them).                                                                           */
enum {
    T2D_PURSUIT_MIN_PRE_AIMING = 0,    /* PurePursuitController.min_pre_aiming_distance */
    T2D_PURSUIT_INTERVAL_LAT = 1,      /* PurePursuitController.interval */
    T2D_PURSUIT_KP = 2,                /* AccelerationController.kp (a divisor) */
    T2D_PURSUIT_ACCEL_CHANGE_RATE = 3,
    T2D_PURSUIT_MAX_ACCEL = 4,
    T2D_PURSUIT_MIN_ACCEL = 5,
    T2D_PURSUIT_INTERVAL_LON = 6,      /* AccelerationController.interval */
    T2D_PURSUIT_DELTA_T = 7,
    T2D_PURSUIT_LAT_MODE = 8,          /* build column: 0 steering 0.0 (AccelerationController.step), 1 pure pursuit */
    T2D_PURSUIT_LON_MODE = 9,          /* build column: 0 cruise, 1 ACC behind the leader (cruise without one), 2 caller's accel */
    T2D_PURSUIT_WHEEL_BASE = 10,       /* build column: the wheel_base argument; NaN = lf + lr of the type row */
    T2D_PURSUIT_LANE_HALF_WIDTH = 11,  /* build columns: the leader rule's corridor and horizon (t2d_set_idm's) */
    T2D_PURSUIT_HORIZON = 12,
    T2D_PURSUIT_COLS = 13
};
#define T2D_PURSUIT_NONE 255
#define T2D_PURSUIT_ROUTE_END 1u   /* the walk ran out of route: the target is where it stopped */
#define T2D_PURSUIT_NONFINITE 2u   /* non-finite input or result: the caller's row passed through */
#define T2D_PURSUIT_WRAPPED 4u     /* the walk went over the seam of a closed route */
#define T2D_PURSUIT_NO_ROUTE 8u    /* lat_mode 1 without a route: steering 0.0 */
#define T2D_PURSUIT_NO_LEADER 16u  /* lon_mode 1 without a leader: cruise */
#define T2D_PROFILE_PURSUIT 16
typedef struct t2d_pursuit_record { /* 72 bytes */
    double point[2];                /* the look-ahead point (x, y), NaN without a walk */
    double pre_aiming_distance;     /* max(speed * interval, min_pre_aiming_distance), NaN when lat_mode 1 did not run */
    double distance;                /* from the position to the look-ahead point, NaN without a walk */
    double cross_track;             /* signed cross-track error of the projection (the PID record's bits), NaN without one */
    int32_t segment;                /* the projection's segment within the route, -1 without one */
    int32_t target_segment;         /* the segment the look-ahead point lies on, -1 without a walk */
    int32_t leader;                 /* lon_mode 1: agent index of the chosen leader, else -1 */
    uint32_t events;                /* T2D_PURSUIT_* of this call */
    double action[2];               /* the applied (steering, accel) in fp64, NaN when the caller's row went through */
} t2d_pursuit_record;
int t2d_set_pursuit(t2d_pool* pool, const double* ctrl_rows, int32_t n_ctrl, int32_t row_stride, const uint8_t* ctrl_id,
                    const float* target_speed);
int t2d_pursuit_actions(t2d_pool* pool, const float* act_in_dev, float* act_out_dev, t2d_pursuit_record* record_dev,
                        void* hip_stream);
int t2d_pursuit_buffers(t2d_pool* pool, void** records_dev, size_t* nbytes);

/* BEV camera -- the top-down semantic image both reference envs declare as their observation (Box(0, 255, (200, 200, 3),
 * uint8), envs/racing.py:102, envs/parking.py:130), for every env in ONE launch behind the step launch.
 *
 * What the reference defines, and this follows (sensor/camera.py, renderer/matplotlib_renderer.py, matplotlib_config.py):
 *   view window   _calculate_bounds: x in [sx - left, sx + right], y in [sy - back, sy + front] around the sensor ("front" is
 *                 +y of the view); auto_scale then widens the short side, about the centre, to the image's aspect ratio
 *                 height / width.
 *   transform     _transform_to_camera_view: v = R(+camera_yaw) (p - sensor) + sensor.  heading_up != 0 takes camera_yaw =
 *                 pi / 2 - heading of the bound participant (it points to the front); heading_up = 0 is north-up, camera_yaw = 0.
 *   style         _resolve_style gives every class its colour and z-order; elements of equal z are drawn in the order
 *                 BEVCamera lists them: areas (the parking target, then the obstacles), lanes, then the participants by slot,
 *                 each body followed by its heading triangle (midpoints of edges 0-1, 1-2 and 3-0 of the body ring).  A
 *                 pedestrian (T2D_SHAPE_CIRCLE) is a disc of radius width / 2 and has no triangle.  Inactive participants are
 *                 not listed.  The defaults below are the reference's resolved values for its envs' objects: a `medium_car`
 *                 Vehicle and an `adult_male` Pedestrian resolve to z-order 1 (their type names are not in DEFAULT_ORDER), so a
 *                 car's body is drawn UNDER the lane it drives on and only its heading triangle (z 7) shows there.
 *   culling       _in_perception_range (distance <= 1.5 x the largest range) never changes a pixel: the farthest corner of
 *                 the window is at most sqrt(2) x the largest range from the sensor.  Not implemented.
 * BUILD-DEFINED, the raster: the image is exactly the view window; pixel (row r, col c) of the height x width image is the
 * class of the topmost element that contains the CENTRE of the pixel; row 0 is at the front edge.  Containment is even-odd
 * crossing on the caller's undivided ring (racing tiles may be non-convex), dx^2 + dy^2 <= r^2 for discs.  No anti-aliasing,
 * no outline strokes; road lines (whose widths are in points) are not drawn.  fp32 throughout: a pixel whose centre is
 * within about 1e-4 m of an edge may fall on either side.  A bound participant whose pose is not finite gives an all-
 * background image.
 *
 *   t2d_camera_config      width x height pixels (each 1 .. T2D_CAMERA_MAX_SIDE), the perception range (left, right, front,
 *                          back; metres, finite, left + right > 0, front + back > 0), bind_slot = the participant slot the
 *                          camera follows, heading_up, layers = T2D_CAMERA_LAYER_* bits, format = T2D_CAMERA_FORMAT_CLASS,
 *                          _RGB or both (| T2D_CAMERA_FORMAT_NAIVE: the measurement yardstick in which every pixel tests
 *                          every element; same image).  Allocates the library's own images.  width = 0 removes the camera.
 *   t2d_camera_set_palette rgb u8[n_class][3], n_class <= T2D_CAMERA_N_CLASS: the colour of classes 0 .. n_class - 1.
 *   t2d_camera_set_style   class_of_type u8[T2D_MAX_TYPES] (NULL: T2D_SHAPE_OBB rows are vehicles, T2D_SHAPE_CIRCLE rows
 *                          pedestrians; T2D_CAMERA_CLASS_BACKGROUND = participants of that row are not drawn, what the
 *                          reference does with an `Obstacle` participant) and z_of_class u8[T2D_CAMERA_N_CLASS] (NULL: the
 *                          defaults), 1 .. 255.
 *   t2d_camera_render      one launch, asynchronous on hip_stream, of the pool's current state.  out_class_dev / out_rgb_dev:
 *                          device memory u8[n_env][height][width] / u8[n_env][height][width][3], 4-byte aligned; with both
 *                          NULL the configured formats go to the library's own images.  kernel_id 11 in t2d_profile_read.  No
 *                          stepping call launches it and it changes no pool field.
 *   t2d_camera_buffers     the library's own images (NULL for a format that was not configured) and their sizes in bytes.
 * Errors: T2D_ERR_INVALID for a null pool, a size / range / slot / layer / format / class out of range; T2D_ERR_STATE for
 * t2d_camera_set_palette / _set_style / _render / _buffers without a configured camera, for t2d_camera_render without a
 * parameter table or a t2d_reset, and for a rendered layer whose geometry was never set (T2D_CAMERA_LAYER_STATIC without
 * static geometry or generated scenes, _LANES without lane geometry, _TRACKS without t2d_set_tracks, _TARGET without target
 * areas); T2D_ERR_NOMEM when the images cannot be allocated.                                                                 */
#define T2D_CAMERA_MAX_SIDE 4096
#define T2D_CAMERA_LAYER_STATIC 1
#define T2D_CAMERA_LAYER_LANES 2
#define T2D_CAMERA_LAYER_TRACKS 4
#define T2D_CAMERA_LAYER_TARGET 8
#define T2D_CAMERA_LAYER_PARTICIPANTS 16
#define T2D_CAMERA_LAYER_ARROWS 32      /* the heading triangles (needs T2D_CAMERA_LAYER_PARTICIPANTS) */
#define T2D_CAMERA_LAYER_ALL 63
#define T2D_CAMERA_FORMAT_CLASS 1
#define T2D_CAMERA_FORMAT_RGB 2
#define T2D_CAMERA_FORMAT_NAIVE 4
#define T2D_CAMERA_CLASS_BACKGROUND 0   /* the figure's white (255, 255, 255) */
#define T2D_CAMERA_CLASS_LANE 1         /* z 3, (47, 53, 66) */
#define T2D_CAMERA_CLASS_OBSTACLE 2     /* z 5, (178, 190, 195) */
#define T2D_CAMERA_CLASS_TARGET 3       /* z 1, (238, 118, 110) */
#define T2D_CAMERA_CLASS_VEHICLE 4      /* z 1, (43, 203, 186) */
#define T2D_CAMERA_CLASS_CYCLIST 5      /* z 6, (253, 150, 68) */
#define T2D_CAMERA_CLASS_PEDESTRIAN 6   /* z 1, (69, 170, 242) */
#define T2D_CAMERA_CLASS_HEADING_ARROW 7 /* z 7, (47, 53, 66) */
#define T2D_CAMERA_N_CLASS 8
#define T2D_PROFILE_CAMERA 11
int t2d_camera_config(t2d_pool* pool, int32_t width, int32_t height, float left, float right, float front, float back,
                      int32_t bind_slot, int32_t heading_up, uint32_t layers, uint32_t format);
int t2d_camera_set_palette(t2d_pool* pool, const uint8_t* rgb, int32_t n_class);
int t2d_camera_set_style(t2d_pool* pool, const uint8_t* class_of_type, const uint8_t* z_of_class);
int t2d_camera_render(t2d_pool* pool, void* out_class_dev, void* out_rgb_dev, void* hip_stream);
int t2d_camera_buffers(t2d_pool* pool, void** class_dev, void** rgb_dev, size_t* class_bytes, size_t* rgb_bytes);

/* Reset-time scene synthesis: ParkingLotGenerator.generate
 * (map/generator/generate_parking_lot.py:239-444) for n_env independent scenes, one lane per scene, on `device_id`.
 * PARITY UNPINNED against the reference: it draws from numpy's global MT19937 stream and evaluates its predicates in
 * shapely (neither available to this build), so the kernel follows the reference's distributions, draw order, control
 * flow and predicates (closed `intersects`, `distance`, `contains`) on a counter-based stream of its own
 * (oracle/t2d_oracle.c: t2do_generate_parking states it; the two agree bit for bit).  Scene e uses stream
 * (seed, first_env + e): a sharded job generates the same scenes whatever the number of ranks.
 * Outputs are HOST arrays (the call synchronises): quads [n_env][T2D_GEN_MAX_QUADS][4][2] fp32 obstacle quads in
 * Map.areas order (same id replaces: map.py:444-453), quad_id their reference ids (-1 = unused slot), n_quads,
 * start [n_env][3] = x, y, heading (fp64, heading not wrapped: +pi when flipped, :409-419), target [n_env][4][2],
 * target_heading (fp64), boundary [n_env][4] = xmin, xmax, ymin, ymax (:436-440), info = T2D_GEN_* bits |
 * obstacle attempts << 8 | start attempts << 16.  The reference's rejection loops are unbounded; here an env whose
 * loop hits the cap is returned with T2D_GEN_UNVERIFIED / T2D_GEN_START_UNVERIFIED set, never silently.        */
#define T2D_GEN_MAX_QUADS 12
#define T2D_GEN_MAX_ATTEMPTS 8
#define T2D_GEN_MAX_START_ATTEMPTS 64
#define T2D_GEN_BAY 0x01u              /* mode == "bay" (else "parallel") */
#define T2D_GEN_UNVERIFIED 0x02u       /* _verify_obstacles still False after T2D_GEN_MAX_ATTEMPTS */
#define T2D_GEN_START_UNVERIFIED 0x04u /* _verify_start_state still False after T2D_GEN_MAX_START_ATTEMPTS */
#define T2D_GEN_NONCONVEX 0x08u        /* an obstacle quad is not convex (the event kernels need convex polygons) */
#define T2D_GEN_OVERFLOW 0x10u         /* more than T2D_GEN_MAX_QUADS distinct ids / obstacle list full */
#define T2D_GEN_START_FLIPPED 0x20u
#define T2D_GEN_TARGET_FLIPPED 0x40u
int t2d_generate_parking(int32_t device_id, uint64_t seed, int64_t first_env, int32_t n_env, double type_proportion,
                         double vehicle_length, double vehicle_width, float* quads, int32_t* quad_id,
                         int32_t* n_quads, double* start, float* target, double* target_heading, float* boundary,
                         uint32_t* info);

/* The same generator writing straight into a pool (one participant per env, SingleTrackKinematics/Dynamics/PointMass
 * agent of type 0): every env's obstacles, boundary, target area (+ area centroid), start pose, episode snapshot and
 * IoU / shaping state are produced and installed by one launch -- what t2d_set_static_geometry + t2d_set_target_areas
 * + t2d_reset + t2d_snapshot do for host-described scenes, with nothing crossing PCIe (envs/parking.py:397-441).
 * Call after t2d_set_param_table / t2d_set_status_config.  Scene of (env e, episode k) = stream
 * first_env + e + k * env_stride (env_stride = total envs of the job).  regenerate != 0: every later t2d_step /
 * t2d_check_status is followed, on the same stream, by a launch that gives each env whose episode just ended
 * (terminated | truncated) the scene of its next episode -- the reference's reset() per episode -- while the terminal
 * status / reward stay readable until the next step; kernel_id 6 in t2d_profile_read.  regenerate = 1: the scenes of
 * the next 16 episodes of every env are kept staged in HBM and topped up every 8 steps on a stream owned by the pool
 * (a scene is a ~46 us single-lane chain), so the step's stream only copies: sixteen lanes per finished env, in the
 * epilogue of the ego step kernel itself when that is the pool's step (no launch behind it, no kernel_id 6 then),
 * else in a launch of their own.  The shortest episode the status rules allow is two steps, the ring holds sixteen and
 * the step stream waits for the refill before last: an env cannot outrun its ring.  Should one ever find its slot
 * unstaged it keeps its lot, and the next t2d_sync / t2d_download / t2d_step_n returns T2D_ERR_STATE (once; call
 * t2d_parking_scenes again) -- results never depend on timing.  regenerate = 2: no staging,
 * scenes are generated on the step's stream.  Geometry lives in a
 * fixed-capacity layout (T2D_GEN_MAX_QUADS polygon slots per env); t2d_set_static_geometry leaves this mode.
 * t2d_get_parking_scenes copies the current scenes (arrays as in t2d_generate_parking, any pointer may be NULL) and
 * the per-env episode numbers to the host.                                                                         */
int t2d_parking_scenes(t2d_pool* pool, uint64_t seed, int64_t first_env, int64_t env_stride, double type_proportion,
                       double vehicle_length, double vehicle_width, int32_t regenerate);
int t2d_get_parking_scenes(t2d_pool* pool, float* quads, int32_t* quad_id, int32_t* n_quads, double* start,
                           float* target, double* target_heading, float* boundary, uint32_t* info, int32_t* episode);

/* Kernel variants: 0 = exact (library-grade fp64 trig every sub-step), 1 = fast (default: SingleTrackKinematics steps whose
 * speed stays inside its bounds are RESUMMED -- the Euler sum of the step's sub-steps evaluated as a series instead of
 * iterated, truncation < 1e-9 m --, everything else advances cos / sin by a rotation recurrence), 2 = fast with the kinematic
 * steps iterated as well (rounds 1-4's form; A/B measurements and tests).  Pools of fewer than two waves per SIMD of the device
 * (< 131072 participants on an MI355X) iterate under variant 1 too -- a lone wave is a latency chain the series' table fetch
 * lengthens --; 3 = variant 1 with the series whatever the pool size (tests).  The single-ego kernel (t2d_set_ego_kernel) and
 * the looping forms of t2d_step_n (pools of <= 2 workgroups per CU) iterate under every variant.  All satisfy the 1e-5
 * contract; see DESIGN.md. */
int t2d_set_integrator_variant(t2d_pool* pool, int32_t variant);

/* Which pure OUTPUT columns the integrators store.  The reference's step() returns a State carrying vx / vy and the
 * applied (clipped) action beside the pose (single_track_kinematics.py:169-198); on the step path nothing reads them back:
 * vx / vy of the single-track models are v cos / v sin of the new heading and T2D_F_APPLIED0/1 the clipped action.  A
 * rollout that does not consume them leaves 16 B per participant and step unwritten (a quarter of the step's HBM writes).
 * Default T2D_OUT_ALL (the reference's State).  A point mass's vx / vy are state and are stored whatever the mask says;
 * with a bit cleared the column keeps its last stored values.                                                          */
#define T2D_OUT_VELOCITY 1u   /* T2D_F_VX / T2D_F_VY of SingleTrackKinematics participants */
#define T2D_OUT_APPLIED 2u    /* T2D_F_APPLIED0 / T2D_F_APPLIED1 */
#define T2D_OUT_ALL 3u
int t2d_set_outputs(t2d_pool* pool, uint32_t mask);

/* Per-kernel timing with HIP events recorded on the launch stream around each kernel.
 * kernel_id: 0 = integrate, 1 = collide(+status), 2 = fused step, 3 = lidar, 4 = idm, 5 = drift, 6 = scene regeneration,
 * 7 = chained steps (t2d_step_n), 8 = lidar of every participant (t2d_lidar_scan_all), 9 = off-route (t2d_off_route),
 * 10 = racing tile progress (t2d_track_progress), 11 = BEV camera (t2d_camera_render), 12 = racing track regeneration
 * (t2d_tracks_regenerate), 13 = Reeds-Shepp planner (t2d_rs_plan), 14 = Reeds-Shepp path follower (t2d_rs_follow),
 * 15 = lane-keeping PID controllers (t2d_pid_actions), 16 = pure pursuit and cruise / ACC controllers (t2d_pursuit_actions),
 * 17 = curve lines into the route sets (t2d_curve_routes), 18 = spline curves into the route sets (t2d_spline_routes),
 * 19 = plan-view reference lines into the route sets (t2d_planview_routes), 20 = a caller's polylines into the route sets
 * (t2d_polyline_routes), 21 = the occupancy grid of every env (t2d_occupancy_grid).  */
int t2d_profile_enable(t2d_pool* pool, int32_t on);
int t2d_profile_read(t2d_pool* pool, int32_t kernel_id, double* total_ms, int64_t* launches);

/* ---- multi-GPU: environments shard across ranks, one process per GPU, no data-path collective.  The only
 * exchange is an all-gather of the 8-byte per-env result records {reward bits, status word} -- RCCL over xGMI, issued
 * from here, reading the record ring (T2D_F_RECORD) in place.
 *   t2d_comm_unique_id  ncclGetUniqueId: rank 0 calls it and ships the 128 bytes to the other ranks by whatever the
 *                       launcher offers (a torch.distributed store, MPI, a file): that bootstrap is the host's business.
 *   t2d_comm_init       ncclCommInitRank on the pool's device (collective over the ranks).  world = 1 with id = NULL
 *                       needs no RCCL at all.  RCCL is opened with dlopen here, not linked.
 *   t2d_gather          all-gather of the records of the LAST n_steps steps (n_steps divides T2D_RECORD_RING and the
 *                       number of steps taken so far) into out_dev = u32 [world][n_steps][n_env][2], caller-owned device
 *                       memory.  nccl_comm = an ncclComm_t of the caller's, or NULL = the pool's own.  Ordered after
 *                       what is enqueued on hip_stream (the steps' stream) and run on a stream of the pool's own, so the
 *                       following steps do not wait for it; a later step that is about to overwrite a slot a gather
 *                       still reads waits for that gather first (event wait on the step's stream, inside t2d_step).
 *   t2d_gather_wait     makes hip_stream wait for every gather issued so far (block_host = 0), or blocks the host until
 *                       they are done (block_host != 0); out_dev may be read after that.                              */
#define T2D_COMM_ID_BYTES 128
int t2d_comm_unique_id(uint8_t* id_out);
int t2d_comm_init(t2d_pool* pool, const uint8_t* id, int32_t rank, int32_t world);
int t2d_gather(t2d_pool* pool, void* nccl_comm, int32_t n_steps, void* out_dev, void* hip_stream);
/* What the pool's communicator is: native_rccl = 1 when t2d_comm_init created an RCCL communicator (0: none, or the
 * RCCL-free world of one), world / rank read back FROM that communicator (ncclCommCount / ncclCommUserRank) -- the proof
 * a multi-GPU run can print that RCCL saw N ranks.  Any pointer may be NULL.                                        */
int t2d_comm_info(t2d_pool* pool, int32_t* native_rccl, int32_t* world, int32_t* rank);
/* t2d_step / t2d_check_status calls so far (t2d_step_n counts n): the step count t2d_gather's n_steps must divide, and the
 * record-ring slot of the next step (count % T2D_RECORD_RING).  -1 for a null pool.                                   */
int64_t t2d_step_count(const t2d_pool* pool);
int t2d_gather_wait(t2d_pool* pool, void* hip_stream, int32_t block_host);

/* Capacity planning: resident workgroups per CU of the fused step kernel with this pool's geometry, its LDS bytes per
 * workgroup (static tables + the workgroup's geometry record), and (may be NULL) the bytes of packed geometry records
 * the workgroups of one step launch stage into LDS.  The 4096 x 64 metric launch is one wave-round of 1024 workgroups
 * on 256 CUs and needs 4; a scene whose record grows past the LDS budget halves the rate.                          */
int t2d_step_occupancy(t2d_pool* pool, int32_t* blocks_per_cu, int64_t* lds_bytes,
                       int64_t* geometry_bytes_per_launch);

/* A hipStreamNonBlocking stream created by the library (priority as hipStreamCreateWithPriority: 0 default, negative
 * higher) -- for hosts that step env groups on streams of their own (t2d_step_groups) without another HIP binding.      */
int t2d_stream_create(int32_t device_id, int32_t priority, void** out_stream);
int t2d_stream_destroy(void* stream);

/* Host-only (no device is touched): the rectangles t2d_set_lane_geometry finds inside the union of each env's lane polygons
 * -- the certificate behind the step kernel's off-lane short cut (a pose whose box lies in one of them is contained in the
 * union).  out = f32 [n_env][T2D_SAFE_RECTS][4] (xmin, xmax, ymin, ymax); unused slots hold (+inf, -inf, +inf, -inf).
 * Same CSR arguments as t2d_set_lane_geometry.  Lets a caller (and the CPU tests) hold the certificate against its own
 * predicate (map/element/map.py:242-329 answers the same "what is near this pose" question with an STRtree).            */
#define T2D_SAFE_RECTS 4
int t2d_lane_safe_rects(int32_t n_env, const int32_t* env_lane_offsets, const int32_t* lane_vert_offsets,
                        const float* verts_xy, float* out);

/* Host-only (no device is touched): the LDS budget of a scene before it is installed.  The step kernels keep the static and
 * lane geometry of one workgroup's envs in ONE packed record of at most 32 KiB; t2d_set_static_geometry / t2d_set_lane_geometry
 * narrow the workgroup down to one wave (64 / padded max_agents envs) before they move the scene to the HBM grid tier.  This call runs
 * the same preparation (convexity checks, fans of quads for 5..8-gons, the boundary pieces of each env's lane union) on host
 * CSR arrays (as in t2d_set_*_geometry; either pair may be NULL) and reports the dwords the fullest such workgroup needs and
 * the budget (8192): what tactics2d_amd/mapgeom.py uses to say how many lane / obstacle polygons of a reference map
 * (map/element/lane.py:125-130, map/element/area.py) an env can carry.                                                      */
int t2d_geometry_budget(int32_t n_env, int32_t max_agents, const int32_t* env_poly_offsets, const int32_t* poly_vert_offsets,
                        const float* poly_xy, const int32_t* env_lane_offsets, const int32_t* lane_vert_offsets,
                        const float* lane_xy, int32_t* dwords_needed, int32_t* dwords_budget, int32_t* envs_per_workgroup);

/* Test and measurement hooks (fault injection, a gather delay, a stand-in policy and closed-loop runner, placement maps) are
 * NOT part of this library: include/t2d_debug.h, exported only by libt2d_hip_debug.so (the same sources built with
 * -DT2D_DEBUG_HOOKS), which tests/, bench.py's closed_loop leg and scripts/ load.                                          */

#ifdef __cplusplus
}
#endif
#endif /* T2D_H_ */
