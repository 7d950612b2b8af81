// t2d_pool.h -- internal layout of a participant pool (host + device views).
//
// Data layout in HBM (the field arrays are allocated once in t2d_create, every other buffer by the call that configures its
// subsystem; hipMalloc aligns all of them to 256 B):
//   per participant, N = n_env * max_agents, env-major (idx = env * A + agent), one
//   contiguous array per field (Struct-of-Arrays) so a wave64 touching 64 consecutive
//   participants issues one 256-B coalesced transaction per field:
//     x, y, heading, speed, vx, vy, act0, act1, applied0, applied1 : f32[N]
//     ids, flags                                                   : u32[N]
//   per env: env_flags u32[E], cnt_step i32[E], frame_ms i32[E], status u8[4E], reward f32[E]
//   parameter table: fp64, TRANSPOSED [T2D_PARAM_COLS][T2D_MAX_TYPES] so that lanes reading
//     column c for different type ids hit consecutive LDS banks after staging
//   static / lane geometry: CSR offsets + fp64 CCW vertices + per-polygon AABB (fp64)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/t2d.h"
#include "t2d_devbuf.h"

namespace t2d {

// Packed geometry record of one collide workgroup (EPB consecutive envs), all dwords, kind k =
// 0 static obstacles / 1 lanes:
//   pstart[k][EPB+1]   first polygon of each env inside the record (int)
//   vstart[k][MP_k+1]  first vertex of each polygon inside the record (int)
//   aabb[k][MP_k]      xmin, xmax, ymin, ymax (fp32, exact: vertices are fp32)
//   xy[k][MV_k]        CCW vertices x, y (fp32)
//   bstart[MP_1+1]     lanes only: first boundary piece of each lane polygon inside the record (int)
//   bnd[MB][4]         lanes only: boundary pieces of the union of the env's lanes, fp64 Ax, Ay, Bx, By (16-B aligned),
//                      grouped by the lane polygon whose edge they are part of (off-lane = not union.contains(pose))
//   safe[EPB][kSafeRects]  lanes only: axis-aligned rectangles (xmin, xmax, ymin, ymax, fp32) known to lie inside the
//                      union of the env's lanes (a rectangular lane, or several that abut exactly, shrunk by 0.1 mm): a
//                      pose whose box lies in one of them is contained in the union -- certified without the polygon tests.
//                      Unused slots hold the empty box (+inf, -inf, +inf, -inf)
// MP_k / MV_k / MB = largest polygon / vertex / piece count of any workgroup; stride is a multiple of 4
// dwords so records are copied to LDS with 16-B loads.
struct GeoLayout {
    int32_t stride;          // dwords per record (0 when there is no geometry)
    int32_t epb;             // environments per collide workgroup
    int32_t has[2];
    int32_t off_pstart[2], off_vstart[2], off_aabb[2], off_xy[2];  // dword offsets
    int32_t off_bstart, off_bnd;                                   // lanes: boundary pieces of the union (dword offsets)
    int32_t off_safe;                                              // lanes: rectangles inside the union (dword offset)
};
constexpr int kSafeRects = 4;   // per env
constexpr int kKinDegree = 4;   // resummed kinematics: polynomials of degree 4 in a^2 (truncation < 2e-10 m at |a| <= 0.5)
enum { KIN_Q0 = 0, KIN_Q4, KIN_Q2, KIN_Q6, KIN_R4, KIN_R8, KIN_R2, KIN_R6 };

// Maps beyond the step kernel's LDS record: one uniform grid per env in HBM (t2d_mapgrid.hip)
constexpr float kGridMargin = 1e-2f;   // parts are registered, and poses looked up, with boxes widened by this much (m)
struct MapGridEnv {
    float x0, y0, inv_cell;   // cell (ix, iy) covers [x0 + ix / inv_cell, ...) x [y0 + iy / inv_cell, ...)
    int32_t nx, ny, cell_off; // the env's cells are cell_start[cell_off + iy * nx + ix]
    int32_t has_lanes, pad;
};
// One registration of a part in a cell: the part's vertices INLINE (padded to four the way load_quad_f32 pads: a triangle repeats its
// first vertex), its boundary pieces' range and the first cell of the part's own cell range -- so a pose that meets the part through
// several cells evaluates it once (in the first cell both ranges share) and the walk is cell -> record, one dependent load.
struct MapItem {
    float xy[8];
    int32_t bnd0, bnd1;       // lane parts: pieces [bnd0, bnd1) of MapGridView::bnd (static parts: 0, 0)
    uint32_t cell_lo;         // ix0 | iy0 << 16 of the cells the part is registered in
    uint32_t kind;            // 0 static, 1 lane
};
static_assert(sizeof(MapItem) == 48, "three 16-byte loads per record");
struct MapGridView {
    const MapGridEnv* env;        // [E]
    const int32_t* cell_start;    // CSR over all cells of all envs (+ 1)
    const MapItem* items;         // per cell: the parts whose (widened) box overlaps it
    const double* bnd;            // boundary pieces of the envs' lane unions, 4 doubles each
};

// What kernels receive by value.
struct LidarView;
struct SceneView;
struct PoolView {
    int32_t n_env, A, N;
    // (sits in the padding behind N, in the cache line every kernel reads when it starts: asked for in the middle of a lone
    // wave's step it is a scalar-cache hit, not a miss of its own -- 512 x 32 envs one launch per step: 12.2 -> 12.7 us
    // with the word further down)  the sub-step count the resummation table below was built for; 0: none
    int32_t kin_n;
    float *x, *y, *heading, *speed, *vx, *vy, *applied0, *applied1;
    const float *act0, *act1;   // the pool's own action fields, or caller-owned device memory (t2d_bind_actions): read only
    int32_t act_stride;         // participant i's actions are act0[i * act_stride], act1[i * act_stride] (1 unless bound strided)
    // IDM agents while caller actions are bound: controlled lanes (idm_ctrl[i] != T2D_IDM_NONE) take their action from the
    // pool's own fields, where the idm kernel writes -- never into the caller's memory.  Null otherwise.
    const uint8_t* idm_ctrl;
    const float *own_act0, *own_act1;
    float *omega_f, *omega_r;  // SingleTrackDrift wheel speeds
    uint32_t *ids, *flags, *env_flags;
    int32_t *cnt_step, *frame_ms;
    uint8_t* status;
    float* reward;
    uint2* record;  // this step's slot of the ring of {reward bits, status word} records
    const double* params;  // [T2D_PARAM_COLS][T2D_MAX_TYPES]
    int32_t n_types;
    // static + lane geometry: one fixed-stride packed record per collide workgroup (see GeoLayout)
    const uint32_t* geo;           // [n_blocks * stride] dwords or null
    GeoLayout geo_layout;
    const float* boundary;         // [4*E] or null
    const uint8_t* boundary_valid; // [E] or null
    // IoU events of the ego (Arrival / NoAction) and reward shaping state, per env
    const double* target_xy;   // [E][8] CCW target quad, or null
    const double* target_c;    // [E][2] its area centroid
    double* last_pose;         // [E][8] pose seen by the previous NoAction.update
    uint8_t* last_valid;       // [E]
    int32_t* cnt_na;           // [E] NoAction.cnt_no_action
    double* max_iou;           // [E] ParkingEnv._max_iou
    double* min_dist;          // [E] ParkingEnv._min_dist_to_target
    const double* snap_min_dist;  // [E] value at the snapshot (episode start)
    const double* time_penalty;   // [max_step + 1] -tanh(cnt / max_step) * time_penalty_scale (host libm), or null
    float* iou;                // [E] last IoU(pose, target), NaN = None
    const float* snap[6];      // episode-start snapshot (x, y, heading, speed, vx, vy) or null
    const uint32_t* snap_ids;
    const float* snap_omega[2];  // wheel speeds at the snapshot; null unless a drift type is present
    int32_t auto_reset;        // t2d_step restores finished envs in its epilogue
    // T2D_OUT_* : which pure OUTPUT columns the integrators store (t2d_set_outputs).  vx / vy of the single-track models and
    // the applied (clipped) action are derived from the state and the action -- nothing on the step path reads them back;
    // a point mass's vx / vy are state and always stored.
    int32_t out_mask;
    // 0: the step launch has the GPU to itself (one wave-round): waves that are BEHIND go first, so that a SIMD's four
    // waves finish together.  1: launches of several pools overlap (t2d_step_groups): waves past the integrator go first,
    // so that workgroups retire and the next launch's can start.  See the priority note in t2d_collide.hip.
    int32_t overlapped;
    // step launch: physical workgroup -> (logical workgroup | wave rotation << 16), or null = identity (t2d_set_step_placement)
    const uint32_t* wgmap;
    // Chained multi-step launch (t2d_step_n; collide_kernel<..., CHAIN>): ONE launch of n_steps x chain_wgs workgroups,
    // workgroup (x = g, y = k) takes step k of the envs of workgroup g and first waits until chain_done[g] == chain_base + k
    // (set by the workgroup that took step k - 1 of the same envs).  Null for the plain one-step launch.
    unsigned long long* chain_done;   // [chain_wgs] {steps of its envs completed so far (a count that only ever grows), XCC id}
    uint32_t* chain_err;        // 1: a workgroup's wait ran out, 2: its predecessor ran on another XCD (never expected; the host checks)
    uint32_t chain_base;        // what chain_done[] holds when this launch starts
    int32_t chain_real_wgs;     // workgroups that own envs; the grid's x extent is rounded up to a multiple of 8
    int32_t split_step;         // the step launch gives every env a workgroup of its own (SPLIT form, small pools of 64-agent envs)
    int32_t loop_steps;         // > 0: the LOOP form -- every workgroup walks through this many steps itself (small pools)
    int32_t pipe_step;          // LOOP form with integrator waves running a step ahead of the event waves (PIPE)
    int32_t chain_k;            // > 1: the chained form with workgroups that take chain_k (= loop_steps) consecutive steps each
    int64_t chain_act_step;     // elements between the action sets of consecutive steps (0: the same actions every step)
    uint2* record_ring;         // the whole ring of per-env result records; step k writes slot (record_slot0 + k) % ring
    int32_t record_slot0;
    // CHAIN launches: what the state was when the fragment started, written by the workgroups of its step 0 from the values
    // they load anyway -- [x | y | heading | speed | vx | vy | ids] of N words each, then cnt_step / frame_ms of n_env words
    // each.  A fragment whose hand-off fails (chain_err) is rolled back to it by the host: t2d_step_n never leaves a pool
    // on stale results (see t2d_api.hip quiesce).  ckpt_tag travels into chain_err[1] with the error: which fragment.
    uint32_t* ckpt;
    uint32_t ckpt_tag;
    uint32_t chain_fault;       // test hook (t2d_debug_chain_fault): 1 = a producer posts a foreign XCC id, 2 = one never posts
    // t2d_step_n on a pool with installed IDM controllers (PIPE form): the integrator waves run the controller ahead of every
    // step themselves (t2d_idm_dev.h) -- its rows, every participant's controller id, and the places t2d_idm_actions writes
    const double* idm_rows;
    const uint8_t* idm_ctrl_all;
    int32_t* idm_leader;
    float *idm_act0_own, *idm_act1_own;
    int32_t idm_n_ctrl;
    const SceneView* regen;   // ego step kernel, regenerating pool: the device copy of the pool's SceneView, else null
    double interval_s;        // (double)interval_ms / 1000 of this launch (PointMass's dt), divided once by the host
    // SingleTrackKinematics, fast variant: the Euler sum of a step RESUMMED instead of iterated (t2d_integrate_dev.h
    // resum_kinematics).  kin_n = the sub-step count the table below was built for (0: none; lanes whose type has another
    // count keep the recurrence loop); kin_coef[i][p] = coefficient of a^(2 i) of polynomial p (KIN_Q0 ...), each the moment
    // of the centred sub-step index it multiplies, divided by its factorial, times the sign / the 1/2, 1/6 of its b-term;
    // kin_geo = {m, M, m - 1/2, m (m - 1) / 2, M^2 / 2, m + 1, (m + 1)^2 / 2, n} with m = (n - 1) / 2, M = n / 2.  Computed by
    // the host (long double) whenever the interval changes; read by the kernels as scalar loads from their argument block.
    double kin_coef[kKinDegree + 1][8];
    double kin_geo[8];
    // pools whose static + lane geometry lives in the HBM grid tier (t2d_mapgrid.hip): the per-participant verdicts
    // (T2D_FLAG_COLLISION_STATIC | T2D_FLAG_OFF_LANE) of t2d_mapgrid.hip's two launches, OR-ed into the flags by the event kernel; else null
    const uint32_t* map_flags;
    unsigned long long* dbg;  // phase cycle accumulators (profiling builds with -DT2D_TIMING only)
    double cell;      // spatial-hash cell edge (m) >= max circum-diameter * 1.001
    double inv_cell;
};

// Lidar inputs (t2d_lidar.hip): plain per-env CSR of the static obstacle rings + beam tables.
struct LidarView {
    const int32_t* env_vert_off;  // [E+1] vertex range of env e, or null (no static obstacles)
    const int32_t* env_vert_cnt;  // null, or [E] vertices in use when envs own fixed-capacity ranges (generated scenes)
    const float* xy;              // [V][4] one record per polygon EDGE: x1, y1, x2, y2 (vertex v -> next vertex of its ring)
    // [V] per edge: index (0..15) of its ring among its env's rings when the ring may take part in the occlusion culling of
    // the scan (CCW, convex, every interior angle with sin >= 0.05, <= 16 rings and <= 48 edges in the env), else 0xff; or null
    const uint8_t* edge_meta;
    const double* beam_pre;       // [n_beams][6] per beam: a = sin, b = -cos of linspace(0, 2pi, n, endpoint=False)[k]
                                  // (lidar.py:161-162) and the four slack-widened bounds of its end point (x hi / lo, y hi / lo)
    double max_range;
    int32_t n_beams, include_participants, ego_index, max_static_verts;
    int32_t max_slots;  // LDS edge slots per env: max_static_verts + 4 * max_agents (when participants are scanned)
    int32_t queue_len;  // (set by launch_lidar) candidates per wave and compaction round
};

// Device-side ParkingLotGenerator (t2d_generate.hip): stream parameters, the per-scene output arrays and -- when the
// scenes are installed in a pool -- the places t2d_set_static_geometry / t2d_set_target_areas / t2d_reset /
// t2d_snapshot would have written: every env owns T2D_GEN_MAX_QUADS polygon slots of 4 vertices.
struct SceneArrays {  // one record per scene, the layout of t2d_generate_parking's outputs
    float* quads; int32_t* quad_id; int32_t* n_quads; double* start; float* target; double* target_heading;
    float* boundary; uint32_t* info;
};
struct SceneView {
    uint64_t seed;
    int64_t first_env, env_stride;  // scene of (env e, episode k) = stream first_env + e + k * env_stride
    double type_proportion, len, wid;
    SceneArrays live;     // [n_env] the scenes the envs are in
    SceneArrays staged;   // [n_env * ring] scenes of coming episodes (episode k of env e in slot k % ring), or nulls
    int32_t ring;         // staged scenes per env (0 = none: regeneration generates on the step's stream)
    int32_t* staged_ep;   // [n_env * ring] episode number held by each staged slot (-1 = empty)
    uint2* refill_list;   // [n_env * ring] {staged slot, episode to generate for it} found by a refill's scan; refill_count[0] of them
    uint32_t* refill_count;
    int32_t* episode;     // [n_env]
    uint32_t* geo;        // the pool's geometry records (capacity layout)
    GeoLayout gl;
    float* lidar_xy; int32_t* lidar_cnt;
    uint8_t* lidar_meta;  // [n_env][4 * T2D_GEN_MAX_QUADS] per edge: its ring's slot when the ring may take part in the scan's occlusion culling, else 0xff
    uint32_t* commit_err; // sticky: an env whose episode ended found no staged scene (scene_commit_kernel)
    float* boundary; double* target_xy; double* target_c;
    float* snap[6]; uint32_t* snap_ids; uint32_t ids_word;
    double* snap_min_dist;
};

// IDM controllers (t2d_idm.hip): parameter sets + one controller id per participant.
struct IdmView {
    const double* rows;      // [n_ctrl][T2D_IDM_COLS]
    const uint8_t* ctrl_id;  // [N] index into rows, T2D_IDM_NONE = action left to the caller
    int32_t* leader;         // [N] out: agent index of the chosen leader inside the env, -1 = none
    int32_t n_ctrl;
};

// The Gym-API host frame (t2d_step_host): where the pack kernel writes what ParkingEnv.step hands its caller, one frame per
// step -- `out` is the device frame (then copied to pinned host memory) or the mapped host frame itself (T2D_FRAME_ZEROCOPY).
struct FrameView {
    char* out;
    t2d_frame_layout lay;
    const double* target_heading;   // [E] or null (diff_heading = NaN)
    const float* target_quads;      // [E][8] scene mode: the live target areas; else null
    const int32_t* episode;         // [E] scene mode, else null
    const uint32_t* commit_err;     // scene regeneration's sticky error word, or null
    uint32_t step_count;
    int32_t ego_index;
};

// Replayed participants (T2D_MODEL_REPLAY; replay_kernel in t2d_history.hip): what a binding holds on the device.  The four
// arrays share one allocation, each starting on a 16-byte boundary.
struct ReplaySpec {
    const float* src;            // the source trajectory's buffer, [T2D_TRAJ_COLS][capacity][N_src]
    const int32_t* src_env;      // [n_env]
    const int32_t* offset_ms;    // [n_env]
    const int32_t* first_slot;   // [N_src]
    const int32_t* last_slot;    // [N_src]
    uint32_t type_mask;          // bit t: row t of the parameter table has model T2D_MODEL_REPLAY (set at launch time)
    int32_t capacity, N_src, n_slots, t0_ms, period_ms;
};

// Off-route detector (t2d_route.hip): what an installed kind of routes holds on the device.  kind 1 = route sets (polylines
// in CSR form, shared between envs), kind 2 = trace routes read out of a recorded trajectory's own x / y columns.
struct RouteView {
    int32_t kind;                    // 0 none, 1 sets, 2 traces
    int32_t lds_bytes;               // sets: dynamic LDS of the launch (the largest set's vertices + route offsets)
    const int32_t* route_of;         // [N] sets: route inside the env's set; traces: agent index of the source participant; -1 none
    const float* threshold;          // [N]
    const int32_t* set_of_env;       // [E] sets
    const int32_t* set_route_start;  // [n_sets + 1] first route of each set
    const int32_t* route_vert_off;   // [n_route + 1] first vertex of each route
    const float* verts;              // [n_vert][2]
    const float *tx, *ty;            // traces: the source trajectory's x and y columns, [capacity][N_src]
    const int32_t *src_env, *first_slot, *last_slot;   // traces: [E], [N_src], [N_src]
    int32_t N_src;
    int32_t log2_group;              // traces: 1 << log2_group lanes per participant (0: one lane each)
};

// Racing tile progress (t2d_track.hip): the installed track sets, the per-env progress state and the copy of it that
// t2d_track_reset / t2d_track_upload last gave each env (where an env whose episode ended starts again).
struct TrackView {
    int32_t installed, ego_index, rule, max_advance, check_off_road, pad;
    const float* tiles;            // [n_tile of all sets][4][2] ring vertices, 32-byte records
    const int32_t* set_start;      // [n_sets + 1] first tile of each set (generated tracks: set * T2D_MAX_TRACK_TILES, the capacity layout)
    const int32_t* n_tile;         // [n_sets] tiles of each set's ring (what lies beyond them in a generated set's slot is never read)
    const int32_t* set_of_env;     // [E]
    int32_t *visiting, *num_visited;   // [E]
    uint32_t* mask;                // [E][T2D_MAX_TRACK_TILES / 32] bit t of an env: tile t visited
    uint8_t* status;               // [E][4] in the layout of T2D_F_STATUS
    float* reward;                 // [E]
    const int32_t* start_visiting; // [E]
    const uint32_t* start_mask;    // [E][T2D_MAX_TRACK_TILES / 32]
};

// The device track generator (t2d_trackgen.hip).  Track t of a launch is the track of the counter stream (seed, first_track +
// t [+ episode * track_stride]); its record goes to slot t of the arrays below, tiles in the capacity layout.
struct TrackGenView {
    uint64_t seed;
    int64_t first_track, track_stride;
    double car_length;             // the start pose puts the nose of a car of this length on the start line
    float* tiles;                  // [n][T2D_MAX_TRACK_TILES][4][2]
    int32_t *n_tile, *n_checkpoint, *attempt;   // [n]
    double* start_pose;            // [n][3] x, y, heading in [0, 2 pi)
    float* start_line;             // [n][2][2]
    float* boundary;               // [n][4] xmin, xmax, ymin, ymax
    uint32_t* flags;               // [n] T2D_TRACKGEN_*
    // installed tracks only (t2d_set_tracks_generated / t2d_tracks_regenerate)
    const uint8_t* status;         // [E][4] the progress launch's status: who finished
    int32_t* episode;              // [E] episodes each env has finished
    uint32_t* err;                 // sticky: a regenerated track came back flagged (its env kept the old one)
    float* env_boundary;           // [E][4] the pool's out-bound boundary
    float* snap[6];                // the episode snapshot
    int32_t ego_index, A;
};

// BEV camera (t2d_camera.hip): the window, the style tables and the camera's own device copy of the caller's static and lane
// rings (kind 0 / 1; undivided, as the lidar scans them) -- or, in scene mode, the generated scenes' live quads.
struct CameraView {
    int32_t configured, width, height, bind_slot, heading_up;
    uint32_t layers, format;
    float ux0, uy1, px_w, px_h;          // camera frame, offsets from the sensor: left edge, front edge; pixel size (m)
    const int32_t* env_poly_off[2];      // [E + 1] or null
    const int32_t* poly_vert_off[2];     // [P + 1]
    const float* poly_xy[2];             // [V][2]
    const float* scene_quads;            // scene mode: [E][T2D_GEN_MAX_QUADS][4][2], else null
    const int32_t *scene_quad_id, *scene_n_quads;
    uint32_t palette[T2D_CAMERA_N_CLASS];   // r | g << 8 | b << 16
    uint8_t z_of_class[T2D_CAMERA_N_CLASS];
    uint8_t class_of_type[T2D_MAX_TYPES];
};

// Occupancy grid (t2d_occupancy.hip): the window shared by the batch and the listing of the static rings -- the camera's device
// copy of the caller's rings (kind 0), or, in scene mode, the generated scenes' live quads.
struct OccView {
    int32_t H, W, include_participants, exclude_slot;
    double cell_size, origin_x, origin_y, inflate, free_weight;
    double mwin;                         // the window's magnitude: what the guard of an element is at least taken of
    const int32_t* env_poly_off;         // [E + 1] or null
    const int32_t* poly_vert_off;        // [P + 1]
    const float* poly_xy;                // [V][2]
    const float* scene_quads;            // scene mode: [E][T2D_GEN_MAX_QUADS][4][2], else null
    const int32_t *scene_quad_id, *scene_n_quads;
};

// The Reeds-Shepp planner (t2d_rs.hip): the configuration of t2d_rs_config and where a plan launch reads the target from.
struct RsPlanView {
    t2d_rs_params cfg;
    double lidar_range;            // the scan is clipped to it (t2d_lidar_config's max_range)
    const double* beam_tab;        // [n_beams][3] cos, sin of k * pi / n_beams * 2 and vehicle_base[k]
    const double* target_xy;       // [E][8] the pool's target quads, or
    const float* target_quads;     // [E][8] the generated scenes' live ones (then target_xy is not read)
    const double* target_heading;  // [E]
    int32_t n_beams, ego_index;
};

// The Reeds-Shepp path follower (t2d_rs_follow.hip): its configuration and its struct-of-arrays state, row r of a table = n_env
// consecutive values.  f64 rows: the last distance_to_go; target / prev_error / integral of the velocity, acceleration and steer
// controller; per segment its signed distance, target x / y / yaw, arc centre x / y (NaN on a line) and start x / y.  i32 rows:
// segments of the adopted plan, index of the head (executing: head < n_seg), calls since adoption, per segment the steer sign.
constexpr int kRfLast = 0, kRfPid = 1, kRfSeg = 10, kRfSegFields = 8, kRfF64Rows = kRfSeg + kRfSegFields * T2D_RS_MAX_SEGMENTS;
constexpr int kRfNSeg = 0, kRfHead = 1, kRfSteps = 2, kRfSteer = 3, kRfI32Rows = kRfSteer + T2D_RS_MAX_SEGMENTS;
struct RsFollowView {
    t2d_rs_follow_params cfg;
    double* f64;      // [kRfF64Rows][n_env]
    int32_t* i32;     // [kRfI32Rows][n_env]
    int32_t ego_index;
};

// Lane-keeping PID controllers (t2d_pid.hip): parameter sets, the per-participant assignment and the controllers' state,
// struct-of-arrays -- word w of participant i is state[w * N + i] -- so a wave's loads and stores of one word coalesce.
struct PidView {
    const double* rows;          // [n_ctrl][T2D_PID_COLS]
    const uint8_t* ctrl_id;      // [N] index into rows, T2D_PID_NONE = the caller's row goes through
    const float* target_speed;   // [N]
    const int32_t* idm_row;      // [N] row of idm_rows (lon_mode 2)
    double* state;               // [T2D_PID_STATE_WORDS][N]
    const double* idm_rows;      // [n_idm][T2D_IDM_COLS] the installed IDM parameter sets, or null
    int32_t n_ctrl, n_idm;
    int32_t stage_xy;            // some row has lon_mode 2: the env's (x, y, speed) go through LDS for the leader rule
};

// Pure pursuit and cruise / ACC controllers (t2d_pursuit.hip): parameter sets and the per-participant assignment.  Stateless.
struct PursuitView {
    const double* rows;          // [n_ctrl][T2D_PURSUIT_COLS]
    const uint8_t* ctrl_id;      // [N] index into rows, T2D_PURSUIT_NONE = the caller's row goes through
    const float* target_speed;   // [N]
    int32_t n_ctrl;
    int32_t stage_xy;            // some row has lon_mode 1: the env's (x, y, speed, applied accel) go through LDS for the leader
    int32_t episode_gate;        // a step that restarts finished envs wrote T2D_F_APPLIED0 last: an env at cnt_step 0 reads 0.0
};

// What one family of scripted action sources keeps in the pool: whether it is installed, the view its launch takes, the owners
// the view borrows from, the host's copy of the assignment (the one-controller-per-participant rule reads it) and what the
// installed rows imply for a call.  clear() is the uninstall: flags and view back to nothing, every block freed.
inline hipError_t first_error(std::initializer_list<hipError_t> es) {
    for (hipError_t e : es)
        if (e != hipSuccess) return e;
    return hipSuccess;
}
struct IdmFamily {
    bool on = false;
    IdmView view{};
    DevBuf<double> d_rows;
    DevBuf<uint8_t> d_ctrl;
    std::vector<uint8_t> ctrl_host;
    hipError_t clear() {
        on = false;
        view = IdmView{};
        ctrl_host.clear();
        return first_error({d_rows.reset(), d_ctrl.reset()});
    }
};
struct PidFamily {
    bool on = false;
    PidView view{};
    DevBuf<double> d_rows, d_state;
    DevBuf<uint8_t> d_ctrl;
    DevBuf<float> d_target;
    DevBuf<int32_t> d_idm_row;
    DevBuf<t2d_pid_record> d_rec;   // the pool's own records (a NULL record_dev)
    std::vector<uint8_t> ctrl_host;
    bool any_lat = false;           // some installed row has lat_mode != 0: a call needs route sets
    int idm_rows_needed = 0;        // lon_mode 2: 1 + the largest idm_row in use (0: no such participant)
    hipError_t clear() {
        on = any_lat = false;
        idm_rows_needed = 0;
        view = PidView{};
        ctrl_host.clear();
        return first_error({d_rows.reset(), d_state.reset(), d_ctrl.reset(), d_target.reset(), d_idm_row.reset(), d_rec.reset()});
    }
};
struct PursuitFamily {
    bool on = false;
    PursuitView view{};
    DevBuf<double> d_rows;
    DevBuf<uint8_t> d_ctrl;
    DevBuf<float> d_target;
    DevBuf<t2d_pursuit_record> d_rec;   // the pool's own records (a NULL record_dev)
    std::vector<uint8_t> ctrl_host;
    bool any_lat = false;    // some installed row has lat_mode 1: a call needs route sets
    bool any_last = false;   // some installed row has lon_mode 0 / 1: a call reads T2D_F_APPLIED0 (T2D_OUT_APPLIED)
    hipError_t clear() {
        on = any_lat = any_last = false;
        view = PursuitView{};
        ctrl_host.clear();
        return first_error({d_rows.reset(), d_ctrl.reset(), d_target.reset(), d_rec.reset()});
    }
};

constexpr int kIdsModelShift = 0;
constexpr int kIdsTypeShift = 8;
constexpr int kIdsActiveShift = 16;

}  // namespace t2d

struct t2d_pool {
    t2d::PoolView v{};
    int device = 0;
    bool have_params = false;
    bool have_reset = false;
    int integrator_variant = 1;
    bool kin_resum = true;   // fast variant: resummed kinematic steps (t2d_set_integrator_variant(pool, 2) keeps the recurrence loop)
    bool kin_resum_forced = false;   // ... also on pools too small to fill the GPU (variant 3: tests)
    bool fused_step = true;  // t2d_step = one launch (integrate + events + status)
    bool ego_kernel = true;  // single-ego pools step with one wave per env (t2d_ego.hip) when they qualify
    bool all_boxes = false;  // every row of the parameter table is T2D_SHAPE_OBB
    t2d_status_config status_cfg{};
    std::string err;
    double host_params[T2D_MAX_TYPES][T2D_PARAM_COLS]{};
    // Ownership: every DevBuf / PinBuf member below owns its block and frees it when the pool is deleted (or when a setter
    // resets / replaces it); the view structs next to them hold plain pointers borrowed from these owners.  The scripted
    // action sources keep theirs together (IdmFamily / PidFamily / PursuitFamily): their setters stage new blocks in locals
    // and move them in when nothing can fail any more, and an uninstall frees them (clear()).
    t2d::DevBuf<> field_buf[T2D_F_COUNT];
    void* field_ptr[T2D_F_COUNT]{};   // t2d_get_field's lookup table: field_buf[f].get()
    size_t field_bytes[T2D_F_COUNT]{};
    t2d::DevBuf<double> d_params;
    t2d::DevBuf<uint32_t> d_geo;
    // the HBM grid tier of maps too large for the LDS record (rebuild_geo): device copies of the parts + the grid
    bool grid_tier = false;
    t2d::MapGridView mapgrid{};
    t2d::DevBuf<t2d::MapGridEnv> d_grid_env;
    t2d::DevBuf<int32_t> d_grid_cell_start;
    t2d::DevBuf<t2d::MapItem> d_grid_items;
    t2d::DevBuf<uint32_t> d_map_flags;
    t2d::DevBuf<> d_grid_seg;   // t2d_mapgrid.hip: one segment per sixteen participants (poses, verdict bits, the queue of pairs to decide)
    t2d::DevBuf<double> d_grid_bnd;
    t2d::DevBuf<float> d_boundary;
    t2d::DevBuf<uint8_t> d_boundary_valid;
    // host copies of the CCW-normalised CSR geometry, kind 0 static / 1 lanes
    struct HostGeo {
        bool present = false;
        // polygons as the EVENT kernels see them: CCW, and every polygon with 5..8 vertices replaced by its fan of
        // quads (v0 v1 v2 v3), (v0 v3 v4 v5), (v0 v5 v6 v7) (last part a triangle for odd counts): the union is the
        // polygon, so `intersects` / point-in tests are the OR over the parts, and the kernels only ever meet 3- and
        // 4-vertex polygons (fan_parts in oracle/t2d_oracle.c states the same)
        std::vector<int32_t> env_off, vert_off;
        std::vector<float> xy, aabb;
        // the caller's rings, CCW, undivided: what the lidar scans (a fan's inner diagonals are not walls)
        std::vector<int32_t> ring_env_off, ring_vert_off;
        std::vector<float> ring_xy;
        // lanes only: boundary pieces of the union of each env's lanes, CSR per lane polygon (build_lane_boundary)
        std::vector<int32_t> bnd_off;
        std::vector<double> bnd;
        // lanes only: per env kSafeRects rectangles inside the union of its lanes (build_safe_rects), 4 floats each
        std::vector<float> safe;
    } hgeo[2];
    t2d::DevBuf<double> d_target_xy, d_target_c, d_last_pose, d_max_iou, d_min_dist, d_snap_min_dist;
    t2d::DevBuf<uint8_t> d_last_valid;
    bool have_target = false;
    // lidar (row f2)
    bool lidar_on = false;
    bool lidar_regular = true;   // the configured beams are linspace(0, 2 pi, n_beams, endpoint=False) to 1e-9 (t2d_rs_config needs that)
    t2d::LidarView lidar{};
    t2d::DevBuf<int32_t> d_lidar_env_off;
    t2d::DevBuf<uint8_t> d_lidar_meta;
    t2d::DevBuf<float> d_lidar_xy;
    t2d::DevBuf<float> d_lidar_all;   // [n_env][max_agents][n_beams]: the pool's own destination of t2d_lidar_scan_all (first use)
    t2d::DevBuf<double> d_beam_sin;
    t2d::DevBuf<double> d_time_penalty;
    bool has_drift = false;   // a T2D_MODEL_DRIFT row is in the parameter table
    // replayed participants (t2d_replay_bind): rows of model T2D_MODEL_REPLAY, the bound source and the device arrays of the binding
    uint32_t replay_types = 0;         // bit t: row t of the parameter table has model T2D_MODEL_REPLAY
    struct t2d_traj* replay_src = nullptr;   // null: no binding
    t2d::ReplaySpec replay{};
    t2d::DevBuf<int32_t> d_replay_meta;
    // off-route detector (t2d_set_routes / t2d_set_routes_from_traj): the installed routes, the assignment arrays and the pool's
    // own result buffers (first NULL-destination t2d_off_route)
    t2d::RouteView route{};
    struct t2d_traj* route_src = nullptr;   // trace routes: the bound trajectory
    t2d::DevBuf<> d_route_geo;           // sets: verts | set_of_env | set_route_start | route_vert_off; traces: src_env | first | last
    t2d::DevBuf<int32_t> d_route_of;
    t2d::DevBuf<float> d_route_thr;
    t2d::DevBuf<float> d_route_dist;
    t2d::DevBuf<uint8_t> d_route_off;
    std::vector<int32_t> route_limit;       // [E] exclusive upper bound of route_of in env e (routes of its set / max_agents)
    int32_t route_n_vert = 0;               // sets: vertices of all sets together (t2d_route_vertices)
    int32_t route_min_limit = 0;            // sets: the smallest route_limit (t2d_curve_routes: every env's set has route r < this)
    bool route_sets_distinct = false;       // sets: no two envs use the same set (t2d_curve_routes writes one curve per env)
    // racing tile progress (t2d_set_tracks): one allocation behind every pointer of the view; n_tile of each env's track
    t2d::TrackView track{};
    t2d::DevBuf<> d_track;
    std::vector<int32_t> track_n_tile;      // [E]
    t2d::TrackGenView trackgen{};           // generated tracks (t2d_set_tracks_generated); tiles == nullptr: host-uploaded ones
    int trackgen_sets = 0;
    bool trackgen_regen = false;            // t2d_tracks_regenerate is allowed
    bool trackgen_used = false;             // a regenerate launch since the last host synchronisation (its sticky word is read then)
    bool trackgen_failed = false;
    // BEV camera (t2d_camera_config): the view, the library's own images, the device copy of the rings (one allocation) and
    // the geometry generation it was made of (geo_gen counts every change of the host rings / the scene mode)
    t2d::CameraView camera{};
    t2d::DevBuf<uint8_t> d_cam_class, d_cam_rgb;
    t2d::DevBuf<> d_cam_geo;
    long long geo_gen = 0, cam_geo_gen = -1;
    bool cam_type_default = true;   // class_of_type follows the parameter table's shapes
    t2d::DevBuf<float> d_snap_omega[2];
    // scripted action sources (t2d_set_idm / t2d_set_pid / t2d_set_pursuit; the structs above)
    t2d::IdmFamily idm;
    t2d::PidFamily pid;
    t2d::PursuitFamily pursuit;
    t2d::DevBuf<float> d_snap[6];     // x, y, heading, speed, vx, vy at episode start
    t2d::DevBuf<uint32_t> d_snap_ids;
    t2d::DevBuf<uint32_t> d_wgmap;   // step-launch placement (t2d_debug_set_step_placement)
    bool have_snapshot = false;
    bool auto_reset = false;
    // A status step that may have restarted envs in its epilogue (auto-reset, regenerated scenes) wrote T2D_F_APPLIED0 last:
    // the column of an env at cnt_step 0 is then the ended episode's.  t2d_upload of the column and t2d_integrate end it.
    bool applied_spans_restart = false;
    // generated parking scenes (row f4): capacity-layout geometry owned by the device
    bool scene_mode = false, scene_regen = false;
    t2d::SceneView scene{};
    t2d::DevBuf<> d_scene_arrays;   // one allocation behind scene.live / scene.staged / scene.episode
    hipStream_t scene_stream = nullptr;   // staged scenes are refilled here, off the step's stream
    hipEvent_t ev_scene_commit = nullptr, ev_scene_refill = nullptr;
    bool scene_refill_pending = false;
    bool scene_commit_failed = false;
    bool scene_committed_in_step = false;   // the last step launch was the ego kernel with the commit in its epilogue
    t2d::DevBuf<t2d::SceneView> d_scene_view;
    bool scene_commit_used = false;   // a commit launch since the last host synchronisation (its sticky error word is read then)
    t2d::DevBuf<int32_t> d_lidar_cnt;
    long long step_count = 0;  // t2d_step calls so far (selects the record ring slot)
    int derived_interval = -1; // the interval_ms column T2D_P_SUBSTEPS of the device table was derived for (-1: none yet)
    // chained multi-step launches (t2d_step_n): per-workgroup step counters + one error word behind them
    t2d::DevBuf<unsigned long long> d_chain;   // chain_slots words, then the error word
    int chain_slots = 0;
    uint32_t chain_count = 0;      // what every counter holds once the launches enqueued so far have run
    bool chain_steps = true;       // t2d_set_step_chaining(pool, 0, *): t2d_step_n falls back to one launch per step
    bool chain_loop = true;        // small pools take the LOOP form (t2d_set_step_chaining(pool, 2, *): never)
    bool chain_pipe2 = true;       // ... and lane waves (PIPE = 2) where the pool has lane polygons
    bool chain_pipe = true;        // small pools: the LOOP form carries integrator waves that run a step ahead (PIPE)
    bool split_steps = true;       // small pools of 64-agent envs step with one env per workgroup (t2d_set_split_step)
    bool chain_priority = true;    // wave priorities of a chained launch: 1 = the rule for overlapping work (PoolView::overlapped)
    bool chain_used = false, chain_failed = false;
    // a failed chained launch (chain_err: 1 = a bounded wait ran out, 2 = producer and consumer of a hand-off on different
    // XCDs): reported ONCE by the next t2d_sync / t2d_download / t2d_step_n; chaining stays off for the pool afterwards.
    // CHAIN-form fragments carry a checkpoint of the state they started from (PoolView::ckpt): the pool is rolled back to it,
    // step count included, and goes on from there with plain launches.
    int chain_err_code = 0;
    bool chain_rolled_back = false;
    long long chain_rollback_step = 0;
    t2d::DevBuf<uint32_t> d_ckpt;
    bool ckpt_armed = false;       // every multi-step launch since the last quiesce was a CHAIN launch with a checkpoint
    uint32_t chain_sig = 0;        // shape (workgroups, split) of the last CHAIN launch whose counters d_chain holds; 0 = none
    uint32_t chain_fault = 0;      // t2d_debug_chain_fault
    bool shape64 = true;           // the plain forms may take their W64 twin (t2d_debug_set_step_shape64 turns it off)
    uint32_t types_used = 0;       // bit t: some active participant has type t (t2d_reset) -- or may have: every path that writes
                                   // ids on the device ORs in what it writes (t2d_restore, an armed auto-reset, t2d_parking_scenes)
    uint32_t snap_types = 0;       // bit t: some active participant of the snapshot has type t (t2d_snapshot, t2d_parking_scenes)
    int chain_depth = 1;           // steps per workgroup of the chained form of large pools (T2D_CHAIN_DEPTH in the environment)
    int device_cus = 0;            // compute units of the pool's device (read once)
    // result gather (the one collective of the path): RCCL communicator + a stream of its own, so that the steps that
    // follow a fragment do not wait for its all-gather; slot_event[k] != null = a gather that reads record slot k was
    // enqueued and the step about to overwrite that slot must wait for it first
    void* comm = nullptr;          // ncclComm_t created by t2d_comm_init (null: none / world of one)
    int comm_rank = 0, comm_world = 1;
    hipStream_t gather_stream = nullptr;
    hipEvent_t ev_frag_ready = nullptr;
    hipEvent_t ev_gather[T2D_RECORD_RING]{};
    hipEvent_t slot_event[T2D_RECORD_RING]{};
    hipEvent_t last_gather = nullptr;
    // streams with work of this pool possibly in flight (what the set-up calls / t2d_sync wait for)
    static constexpr int kMaxLiveStreams = 4;
    hipStream_t live_streams[kMaxLiveStreams]{};
    int n_live_streams = 0;
    bool live_overflow = false;
    // the Gym-API host frame (t2d_frame_config / t2d_step_host)
    uint32_t frame_sections = 0;
    t2d_frame_layout frame_layout{};
    t2d::DevBuf<char> d_frame;        // device frame (copy mode)
    t2d::PinBuf<char> h_frame[T2D_MAX_HOST_FRAMES];   // pinned (and mapped) host frames
    int n_host_frames = 0, frame_turn = 0;
    t2d::PinBuf<float> h_actions;       // pinned (and mapped) staging of the host actions, [N][2]
    t2d::DevBuf<float> d_actions;       // device copy of them (copy mode)
    bool act_in_frame = false;        // v.act0 / v.act1 point into d_actions / the mapped h_actions (set by t2d_step_host)
    int64_t act_extent = 0;       // elements readable behind each bound action pointer (t2d_set_action_extent; 0 = not declared)
    t2d::DevBuf<double> d_target_heading;
    // Reeds-Shepp planner (t2d_rs_config): the view, its beam table and the pool's own plan records
    bool rs_on = false;
    t2d::RsPlanView rs{};
    t2d::DevBuf<double> d_rs_beam_tab;
    t2d::DevBuf<t2d_rs_plan_record> d_rs_plan;
    // Reeds-Shepp path follower (t2d_rs_follow_config): the view, its state tables and the pool's own records
    bool rs_follow_on = false;
    t2d::RsFollowView rs_follow{};
    t2d::DevBuf<double> d_rs_follow_f64;     // what rs_follow.f64 / .i32 borrow
    t2d::DevBuf<int32_t> d_rs_follow_i32;
    t2d::DevBuf<t2d_rs_follow_record> d_rs_follow_rec;
    // profiling
    t2d::DevBuf<unsigned long long> d_dbg;   // what v.dbg borrows (-DT2D_TIMING builds)
    bool profiling = false;
    static constexpr int kMaxProfSteps = 4096;
    hipEvent_t* prof_events = nullptr;  // 2 events per recorded launch
    int prof_kernel[2 * kMaxProfSteps]{};
    int prof_count = 0;
};

// kernel launchers (defined in t2d_integrate.hip / t2d_collide.hip)
namespace t2d {
hipError_t launch_integrate(const PoolView& v, int interval_ms, int variant, bool allow_wide, int only_model, hipStream_t s);
// column T2D_P_SUBSTEPS of the device table for `interval_ms` (rows of the drift model keep their own column 23)
hipError_t launch_derive(double* params, int n_types, int interval_ms, hipStream_t s);
// (shape64: the plan's StepPlan::w64 -- the plain fused step takes its instantiation with the shape of 64-wide envs compiled in)
hipError_t launch_collide(const PoolView& v, const t2d_status_config& cfg, bool with_status,
                          int interval_ms, int fuse_variant, hipStream_t s, bool shape64 = false);
// n_steps fused steps in one launch (v.chain_* set by the caller); see PoolView::chain_done
hipError_t launch_step_chain(const PoolView& v, const t2d_status_config& cfg, int interval_ms, int variant, int n_steps,
                             hipStream_t s, bool shape64 = false);
hipError_t launch_ego_step(const PoolView& v, const t2d_status_config& cfg, int interval_ms, int variant, hipStream_t s);
hipError_t step_occupancy(const PoolView& v, int* blocks_per_cu, size_t* lds_bytes);
hipError_t launch_lidar(const PoolView& v, const LidarView& lv, float* out, hipStream_t s);
hipError_t launch_lidar_all(const PoolView& v, const LidarView& lv, float* out, hipStream_t s);
hipError_t launch_drift(const PoolView& v, int interval_ms, hipStream_t s);
hipError_t launch_verify(const PoolView& v, const float* x, const float* y, const float* heading, const float* speed,
                         int interval_ms, uint8_t* valid, hipStream_t s);
// device-resident trajectories (t2d_history.hip): slot `slot` of a [T2D_TRAJ_COLS][capacity][N] buffer <- the pool's state;
// verify_states of the frames slot_dev[0..n_frames) against frame 0 (stable: every interval_dev[k >= 1] is the same value)
hipError_t launch_traj_record(const PoolView& v, float* buf, int capacity, int slot, hipStream_t s);
hipError_t launch_verify_states(const PoolView& v, const float* buf, int capacity, const int32_t* slot_dev,
                                const double* interval_dev, int n_frames, int stable, uint8_t* valid, hipStream_t s);
// replayed participants: state and active byte at stamp frame_ms + step_ms + offset (step_ms = 0: the envs' current stamp)
hipError_t launch_replay(const PoolView& v, const ReplaySpec& r, int step_ms, hipStream_t s);
// off-route detector (t2d_route.hip): distance (f32) and verdict (u8) of every participant against its route
hipError_t launch_off_route(const PoolView& v, const RouteView& rv, float* dist, uint8_t* off, hipStream_t s);
// curve lines into the route sets (t2d_curve.hip): curve e -> the fp32 vertices of route `route` of env e's set
hipError_t launch_curve_routes(const PoolView& v, const RouteView& rv, const void* words, const double* start, double radius,
                               double step, int rule, int route, int32_t* count, hipStream_t s);
// a caller's polyline per env (t2d_curve.hip): the first min(counts[e], max_pts) points [max_pts][cols] -> the same vertices
hipError_t launch_polyline_routes(const PoolView& v, const RouteView& rv, const double* points, const int32_t* counts, int max_pts,
                                  int cols, int route, int32_t* count, hipStream_t s);
// spline curves (t2d_spline.hip): what is wrong with a launch's arguments (null: nothing), and curve e -> the fp32 vertices of
// route `route` of env e's set
const char* spline_args_error(int kind, const double* ctrl, const int32_t* n_ctrl, int max_ctrl, int n_interp, int degree,
                              const double* knots, int boundary, const double* derivs);
hipError_t launch_spline_routes(const PoolView& v, const RouteView& rv, int kind, const double* ctrl, const int32_t* n_ctrl,
                                int max_ctrl, int n_interp, int degree, const double* knots, int boundary, const double* derivs,
                                int route, int32_t* count, hipStream_t s);
// plan-view reference lines (t2d_road.hip): what is wrong with a launch's arguments (null: nothing), and road e -> the fp32
// vertices of route `route` of env e's set
const char* planview_args_error(const void* rec, const int32_t* n_geom, int max_geom, int rule);
hipError_t launch_planview_routes(const PoolView& v, const RouteView& rv, const void* rec, const int32_t* n_geom, int max_geom, int rule,
                                  int stride, int route, int32_t* count, hipStream_t s);
// racing tile progress (t2d_track.hip): march, visited mask, status and reward of every env
hipError_t launch_track_progress(const PoolView& v, const TrackView& tv, int write_status, hipStream_t s);
hipError_t launch_trackgen(const TrackGenView& g, int n, int mode, hipStream_t s);
hipError_t launch_track_install(const PoolView& v, const TrackGenView& g, const int32_t* set_of_env, hipStream_t s);
// BEV camera (t2d_camera.hip): the class and / or RGB image of every env (null: not written); naive = every pixel tests every element
hipError_t launch_camera(const PoolView& v, const CameraView& cv, const TrackView& tv, uint8_t* out_class, uint8_t* out_rgb, int naive,
                         hipStream_t s);
// occupancy grid (t2d_occupancy.hip): weights and / or mask of every env (null: not written); naive = every cell tests every element
hipError_t launch_occupancy(const PoolView& v, const OccView& ov, double* weight, uint8_t* mask, int32_t* hw, int32_t* status, int naive,
                            hipStream_t s);
// Reeds-Shepp planner (t2d_rs.hip): one plan record per env from the scan [n_env][n_beams]
hipError_t launch_rs_plan(const PoolView& v, const RsPlanView& rv, const float* scan, t2d_rs_plan_record* out, hipStream_t s);
// Reeds-Shepp path follower (t2d_rs_follow.hip): one action row and one record per env; agent.reset() for the masked envs (null: all)
hipError_t launch_rs_follow(const PoolView& v, const RsFollowView& fv, const t2d_rs_plan_record* plan, const float* act_in,
                            float* act_out, t2d_rs_follow_record* out, hipStream_t s);
hipError_t launch_rs_follow_reset(const PoolView& v, const RsFollowView& fv, const uint8_t* mask, hipStream_t s);
// lane-keeping PID controllers (t2d_pid.hip): one action row and one record per participant; controller.reset() for the masked
// envs (null: all)
hipError_t launch_pid(const PoolView& v, const PidView& cv, const RouteView& rv, const float* act_in, float* act_out,
                      t2d_pid_record* out, hipStream_t s);
hipError_t launch_pid_reset(const PoolView& v, const PidView& cv, const uint8_t* mask, hipStream_t s);
// pure pursuit and cruise / ACC controllers (t2d_pursuit.hip): one action row and one record per participant
hipError_t launch_pursuit(const PoolView& v, const PursuitView& cv, const RouteView& rv, const float* act_in, float* act_out,
                          t2d_pursuit_record* out, hipStream_t s);
hipError_t launch_idm(const PoolView& v, const IdmView& iv, const int32_t* forced_leader, float* act0_own, float* act1_own,
                      hipStream_t s);
hipError_t launch_restore(const PoolView& v, const float* const* snap, const uint32_t* snap_ids, int mode,
                          hipStream_t s);
hipError_t launch_spin(long long ticks_100mhz, hipStream_t s);
size_t map_segment_bytes(int n_participants);   // the walk -> decisions hand-over buffer of launch_map_events
hipError_t launch_map_events(const PoolView& v, const MapGridView& mg, void* segments, uint32_t* out, hipStream_t s);
#ifdef T2D_DEBUG_HOOKS
int last_collide_shape();           // 64: that launch took the W64 twin of its form (envs of 64, four per workgroup compiled in); 0: the generic one
const char* last_collide_form();   // template arguments of the collide_kernel instantiation the last launch took (t2d_collide.hip)
// the step kernel's wave_excl_scan on n_waves waves of 64 counts each (t2d_collide.hip): out_dev = per wave 64 offsets + the total
hipError_t launch_wave_scan_probe(const int32_t* cnt_dev, int32_t* out_dev, int n_waves);
#endif
hipError_t launch_frame_pack(const PoolView& v, const FrameView& fv, hipStream_t s);
// note that work of this pool was enqueued on `s` by code outside t2d_api.hip (a replayed graph): t2d_sync waits for it
void pool_touch(t2d_pool* p, hipStream_t s);
hipError_t launch_parking_scenes(const PoolView& v, const SceneView& sv, int n_env, int mode, hipStream_t s);
hipError_t launch_scene_refill(const SceneView& sv, int n_env, hipStream_t s);
// regenerate = 1: envs whose episode just ended take the scene staged for their next one, sixteen lanes per env
hipError_t launch_scene_commit(const PoolView& v, const SceneView& sv, int n_env, hipStream_t s);
}  // namespace t2d
