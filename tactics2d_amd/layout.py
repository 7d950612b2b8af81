"""Numeric constants of the C ABI (include/t2d.h), mirrored for the Python host side.
tests/test_layout.py parses the header and checks that the two agree."""
ABI_VERSION = 13   # T2D_ABI_VERSION: _ffi.lib() refuses a libt2d_hip.so built from another header
# parameter-row columns
P_MODEL, P_LF, P_LR, P_WB = 0, 1, 2, 3
P_STEER_LO, P_STEER_HI, P_SPEED_LO, P_SPEED_HI, P_ACCEL_LO, P_ACCEL_HI = 4, 5, 6, 7, 8, 9
P_RANGE_FLAGS, P_MASS, P_MASS_HEIGHT, P_MU, P_IZ, P_CF, P_CR = 10, 11, 12, 13, 14, 15, 16
P_DELTA_T_MS, P_SHAPE, P_LENGTH, P_WIDTH = 17, 18, 19, 20
PARAM_COLS = 24
MAX_TYPES = 32
RANGE_STEER, RANGE_SPEED, RANGE_ACCEL = 1, 2, 4
MODEL_KINEMATICS, MODEL_DYNAMICS, MODEL_POINTMASS, MODEL_DRIFT, MODEL_POINTMASS_EULER = 0, 1, 2, 3, 4
MODEL_REPLAY = 5   # no physics: the state comes out of a recorded trajectory (t2d_replay_bind)
P_DRIFT_TSB, P_DRIFT_TSE, P_DRIFT_RADIUS, P_DRIFT_IYW = 15, 16, 22, 23   # SingleTrackDrift rows only
P_DT_S, P_SUBSTEPS = 22, 23   # rows of the other models: derived by the library (sub-step in s, sub-step counts of the launch)
MAX_INTERVAL_MS = 32767
SHAPE_OBB, SHAPE_CIRCLE = 0, 1
# fields
F_X, F_Y, F_HEADING, F_SPEED, F_VX, F_VY, F_ACT0, F_ACT1, F_IDS, F_FLAGS = range(10)
F_APPLIED0, F_APPLIED1, F_ENV_FLAGS, F_CNT_STEP, F_FRAME_MS, F_STATUS, F_REWARD = range(10, 17)
F_RECORD = 17
F_IOU = 18
F_CNT_NO_ACTION = 19
F_LIDAR = 20
F_LEADER = 21
F_OMEGA_F, F_OMEGA_R = 22, 23
F_COUNT = 24
FIELD_DTYPES = {
    F_X: "float32", F_Y: "float32", F_HEADING: "float32", F_SPEED: "float32", F_VX: "float32",
    F_VY: "float32", F_ACT0: "float32", F_ACT1: "float32", F_IDS: "uint32", F_FLAGS: "uint32",
    F_APPLIED0: "float32", F_APPLIED1: "float32", F_ENV_FLAGS: "uint32", F_CNT_STEP: "int32",
    F_FRAME_MS: "int32", F_STATUS: "uint8", F_REWARD: "float32", F_RECORD: "uint32", F_IOU: "float32", F_CNT_NO_ACTION: "int32", F_LIDAR: "float32",
    F_LEADER: "int32", F_OMEGA_F: "float32", F_OMEGA_R: "float32",
}
PER_ENV_FIELDS = (F_ENV_FLAGS, F_CNT_STEP, F_FRAME_MS, F_STATUS, F_REWARD, F_RECORD, F_IOU, F_CNT_NO_ACTION, F_LIDAR)
# event bits
FLAG_COLLISION_DYNAMIC, FLAG_COLLISION_STATIC, FLAG_OUT_BOUND, FLAG_OFF_LANE = 1, 2, 4, 8
RECORD_RING = 64
OUT_VELOCITY, OUT_APPLIED, OUT_ALL = 1, 2, 3
SAFE_RECTS = 4
MAX_POLY_VERTS = 8
MAX_AGENTS = 256
MAX_ROUTE_SET_VERTS = 4096   # T2D_MAX_ROUTE_SET_VERTS: vertices of one route set (t2d_set_routes)
PROFILE_OFF_ROUTE = 9        # kernel id of t2d_off_route in t2d_profile_read
MAX_TRACK_TILES = 2048       # T2D_MAX_TRACK_TILES: tiles of one racing track (t2d_set_tracks); the visited mask is 64 words per env
TRACK_MASK_WORDS = MAX_TRACK_TILES // 32
TRACK_RULE_REFERENCE, TRACK_RULE_FORWARD = 0, 1   # T2D_TRACK_RULE_*
PROFILE_TRACK_PROGRESS = 10  # kernel id of t2d_track_progress in t2d_profile_read
# BEV camera (t2d_camera_config): layer bits, formats, classes
CAMERA_MAX_SIDE = 4096
CAMERA_LAYER_STATIC, CAMERA_LAYER_LANES, CAMERA_LAYER_TRACKS, CAMERA_LAYER_TARGET = 1, 2, 4, 8
CAMERA_LAYER_PARTICIPANTS, CAMERA_LAYER_ARROWS, CAMERA_LAYER_ALL = 16, 32, 63
CAMERA_FORMAT_CLASS, CAMERA_FORMAT_RGB, CAMERA_FORMAT_NAIVE = 1, 2, 4
CAMERA_CLASS_BACKGROUND, CAMERA_CLASS_LANE, CAMERA_CLASS_OBSTACLE, CAMERA_CLASS_TARGET = 0, 1, 2, 3
CAMERA_CLASS_VEHICLE, CAMERA_CLASS_CYCLIST, CAMERA_CLASS_PEDESTRIAN, CAMERA_CLASS_HEADING_ARROW = 4, 5, 6, 7
CAMERA_N_CLASS = 8
PROFILE_CAMERA = 11          # kernel id of t2d_camera_render in t2d_profile_read
# Reeds-Shepp curves and planner (t2d_rs_paths / t2d_rs_plan): sizes, the plan's status values, the record's size in bytes
RS_SLOTS, RS_MAX_SEGMENTS, RS_MAX_POSES, RS_MAX_BEAMS = 48, 5, 1024, 1024
RS_NO_TARGET, RS_FAR, RS_FOUND, RS_NONE_FREE, RS_UNCHECKED = range(5)
RS_RECORD_BYTES = 96
# the records as columns of their int32 ("<i4") and float64 ("<f8") views: field -> (view, column or columns of that view)
RS_RECORD_FIELDS = {"status": ("<i4", 0), "slot": ("<i4", 1), "n_seg": ("<i4", 2), "n_visited": ("<i4", 3), "steer": ("<i4", slice(4, 9)),
                    "distance": ("<f8", slice(5, 10)), "length": ("<f8", 10), "shortest": ("<f8", 11)}
PROFILE_RS_PLAN = 13         # kernel id of t2d_rs_plan in t2d_profile_read
# Dubins paths and sampled curve lines (t2d_dubins_paths / t2d_curve_lines / t2d_curve_routes): slots, the word record's size
# in bytes (f64 seg[5], i8 letter[5], i8 n_seg, 2 bytes of padding), the sampling rules, the kernel id
DUBINS_SLOTS = 6
CURVE_WORD_BYTES = 48
CURVE_DUBINS, CURVE_RS = 0, 1
PROFILE_CURVE_ROUTES = 17
# Bezier, B-spline and cubic spline curves (t2d_spline_curves / t2d_spline_routes): the families, the cubic spline's boundary
# types, the caps of a launch, the curves that share a workgroup, the kernel id
SPLINE_BEZIER, SPLINE_BSPLINE, SPLINE_CUBIC = 0, 1, 2
SPLINE_NATURAL, SPLINE_CLAMPED, SPLINE_NOT_A_KNOT = 1, 2, 3
SPLINE_MAX_CTRL, SPLINE_MAX_DEGREE = 32, 5
SPLINE_CURVES_PER_BLOCK = 4
PROFILE_SPLINE_ROUTES = 18
# Spiral and ParamPoly3 curves and plan-view reference lines (t2d_spiral_curves / t2d_param_poly3_curves / t2d_planview_lines /
# t2d_planview_routes): the spiral rules, the geometry kinds and pRange codes of a plan-view record, the record's size in bytes
# (i32 kind, i32 p_range, f64 s, x, y, hdg, length, f64 par[8]), the caps, the curves that share a workgroup, the kernel id
SPIRAL_REFERENCE, SPIRAL_STANDARD = 0, 1
GEOM_LINE, GEOM_SPIRAL, GEOM_ARC, GEOM_POLY3, GEOM_PARAM_POLY3 = range(5)
P_RANGE_NORMALIZED, P_RANGE_ARC_LENGTH = 0, 1
PLANVIEW_RECORD_BYTES = 112
PLANVIEW_MAX_GEOM, PLANVIEW_MAX_RAW = 64, 1 << 20
ROAD_CURVES_PER_BLOCK = 4
PROFILE_PLANVIEW_ROUTES = 19
# Grid shortest paths (t2d_grid_dijkstra): the status of a row, the cap on the cells of one grid (two fp64 planes in LDS)
GRID_FOUND, GRID_NO_PATH, GRID_TRUNCATED, GRID_INVALID, GRID_FIELD_ONLY = range(5)
GRID_MAX_CELLS = 4096
# Grid A* (t2d_grid_astar): the status it adds to GRID_*, the heuristic kinds of a launch
GRID_MAX_ITER = 5
ASTAR_H_ZERO, ASTAR_H_EUCLIDEAN, ASTAR_H_MANHATTAN, ASTAR_H_OCTILE, ASTAR_H_TABLE = range(5)
# Hybrid A* (t2d_hybrid_astar): the status of a row; the caps of one query: open entries (LDS), x_cells * y_cells of its cost grid
# (16 headings of 2 bytes each in the workspace), steering angles
HYBRID_FOUND, HYBRID_NO_PATH, HYBRID_MAX_ITER, HYBRID_TRUNCATED, HYBRID_OVERFLOW, HYBRID_INVALID = range(6)
HYBRID_MAX_OPEN = 2048
HYBRID_MAX_XY_CELLS = 32768
HYBRID_MAX_STEER = 16
# Sampling planners (t2d_sample_plan): the kinds, the status of a row, the nodes whose coordinates a query keeps in LDS, the bytes
# of one node in the workspace (x, y f64; cost f64; parent i32; a query's row is rounded up to 256 bytes); the kernel id of
# t2d_polyline_routes
SAMPLE_RRT, SAMPLE_RRT_STAR, SAMPLE_RRT_CONNECT = range(3)
SAMPLE_FOUND, SAMPLE_MAX_ITER, SAMPLE_TRUNCATED, SAMPLE_OVERFLOW, SAMPLE_INVALID = range(5)
SAMPLE_LDS_NODES = 512
SAMPLE_NODE_BYTES = 28
PROFILE_POLYLINE_ROUTES = 20
# Probabilistic roadmaps (t2d_prm_plan): the status of a row; the caps of one query: nodes (start, target and samples; x, y, two
# planes of g and two words each in LDS), k_nearest (a sorted list in registers)
PRM_FOUND, PRM_NO_PATH, PRM_TRUNCATED, PRM_OVERFLOW, PRM_INVALID = range(5)
PRM_MAX_NODES = 1024
PRM_MAX_K = 16
# Occupancy grid (t2d_occupancy_grid): the status of a row, the format bit of the measurement yardstick, the kernel id
OCC_OK, OCC_INVALID = range(2)
OCC_FORMAT_NAIVE = 1
PROFILE_OCCUPANCY = 21
# Reeds-Shepp path follower (t2d_rs_follow): the record's size in bytes, its event bits, the kernel id
RS_FOLLOW_RECORD_BYTES = 48
RS_FOLLOW_RECORD_FIELDS = {"executing": ("<i4", 0), "segment": ("<i4", 1), "events": ("<i4", 2), "steps": ("<i4", 3),
                           "action": ("<f8", slice(2, 4)), "distance_to_go": ("<f8", 4), "total_error": ("<f8", 5)}
RS_FOLLOW_ADOPTED, RS_FOLLOW_POP_REACHED, RS_FOLLOW_POP_RISING, RS_FOLLOW_FINISHED, RS_FOLLOW_RESET, RS_FOLLOW_DROPPED = \
    1, 2, 4, 8, 16, 32
PROFILE_RS_FOLLOW = 14
# IDM controller parameter sets (t2d_set_idm)
IDM_DESIRED_SPEED, IDM_TIME_HEADWAY, IDM_MIN_SPACING, IDM_MAX_ACCEL, IDM_COMF_DECEL, IDM_DELTA = range(6)
IDM_LANE_HALF_WIDTH, IDM_HORIZON = 6, 7
IDM_COLS = 8
IDM_NONE = 255
IDM_LEADER_FREE, IDM_LEADER_SEARCH = -1, -2
# lane-keeping PID controllers (t2d_set_pid / t2d_pid_actions): parameter-row columns, state words, event bits, the record's
# size in bytes, the kernel id
PID_DT, PID_KP_LAT, PID_KI_LAT, PID_KD_LAT, PID_MAX_STEERING, PID_KP_LON, PID_KI_LON, PID_KD_LON = range(8)
PID_MAX_ACCEL, PID_MIN_ACCEL, PID_ALPHA, PID_LAT_MODE, PID_LON_MODE, PID_WHEEL_BASE = range(8, 14)
PID_COLS = 14
PID_LAT_NONE, PID_LAT_HEADING, PID_LAT_CROSS_TRACK = 0, 1, 2     # values of the lat_mode column
PID_LON_ZERO, PID_LON_SPEED, PID_LON_IDM, PID_LON_CALLER = 0, 1, 2, 3   # values of the lon_mode column
PID_STATE_WORDS = 6   # lat integral, prev_error, prev_derivative, then the same three of the longitudinal side
PID_NONE = 255
PID_ROUTE_END, PID_NONFINITE, PID_RESET, PID_NO_ROUTE, PID_BAD_WHEEL_BASE, PID_SATURATED = 1, 2, 4, 8, 16, 32
PID_RECORD_BYTES = 48
PID_RECORD_FIELDS = {"cross_track": ("<f8", 0), "lat_error": ("<f8", 1), "segment": ("<i4", 4), "leader": ("<i4", 5), "events": ("<i4", 6),
                     "action": ("<f8", slice(4, 6))}
PROFILE_PID = 15
# pure pursuit and cruise / ACC controllers (t2d_set_pursuit / t2d_pursuit_actions): parameter-row columns, mode values, event
# bits, the record's size in bytes, the kernel id
PURSUIT_MIN_PRE_AIMING, PURSUIT_INTERVAL_LAT, PURSUIT_KP, PURSUIT_ACCEL_CHANGE_RATE, PURSUIT_MAX_ACCEL, PURSUIT_MIN_ACCEL = range(6)
PURSUIT_INTERVAL_LON, PURSUIT_DELTA_T, PURSUIT_LAT_MODE, PURSUIT_LON_MODE, PURSUIT_WHEEL_BASE = range(6, 11)
PURSUIT_LANE_HALF_WIDTH, PURSUIT_HORIZON = 11, 12
PURSUIT_COLS = 13
PURSUIT_LAT_NONE, PURSUIT_LAT_PURE_PURSUIT = 0, 1                      # values of the lat_mode column
PURSUIT_LON_CRUISE, PURSUIT_LON_ACC, PURSUIT_LON_CALLER = 0, 1, 2      # values of the lon_mode column
PURSUIT_NONE = 255
PURSUIT_ROUTE_END, PURSUIT_NONFINITE, PURSUIT_WRAPPED, PURSUIT_NO_ROUTE, PURSUIT_NO_LEADER = 1, 2, 4, 8, 16
PURSUIT_RECORD_BYTES = 72
PURSUIT_RECORD_FIELDS = {"point": ("<f8", slice(0, 2)), "pre_aiming_distance": ("<f8", 2), "distance": ("<f8", 3), "cross_track": ("<f8", 4),
                         "segment": ("<i4", 10), "target_segment": ("<i4", 11), "leader": ("<i4", 12), "events": ("<i4", 13),
                         "action": ("<f8", slice(7, 9))}
PROFILE_PURSUIT = 16
# host-frame sections (t2d_frame_config)
FRAME_LIDAR, FRAME_TARGET, FRAME_ZEROCOPY = 1, 2, 4
# device-resident trajectories (t2d_traj_*): column order of a slot
TRAJ_COLS = 6
TRAJ_X, TRAJ_Y, TRAJ_HEADING, TRAJ_SPEED, TRAJ_VX, TRAJ_VY = range(6)
