"""Reference restatement of the racing tile progress (test infrastructure; the definition is include/t2d.h, "Racing tile
progress", and DESIGN.md 4.13).

Statements of `_RacingScenarioManager._locate_agent` / `check_status` and `RacingEnv._get_rewards` (envs/racing.py:261-301,
339-369, 121-139):

  * `touch` / `touch_many`: the touch predicate in fp64, in the kernel's operation order (tactics2d_amd/csrc/t2d_track_dev.h).
    Every numpy operation is ONE IEEE rounding (numpy never contracts a product and a sum), so verdicts are comparable with the
    kernel's (built with -ffp-contract=off) bit for bit.
  * `touch_exact`: the same question -- does one of the ring's four edges meet the closed box? -- on fractions.Fraction, by
    another route (the edge clipped against the box's four half-planes), so that the two do not share a mistake.
  * `Progress.step`: the march, gap filling, status and reward vectorised over envs (what the GPU tests compare with).  Its
    reference rule is held against records of the reference's own `_locate_agent` run on scripted touch patterns
    (tests/golden/racing_progress.npz, march_*), its build-defined forward rule against `locate_forward`, a direct statement.

The car's box is Vehicle.get_pose with the event kernels' expressions: `box` goes through the C oracle (t2do_ego_poses: the
deterministic sincos, which numpy cannot restate for want of an fma).
"""
import ctypes as C
from fractions import Fraction

import numpy as np

F64 = np.float64
MAX_TILES = 2048
WORDS = MAX_TILES // 32
RULE_REFERENCE, RULE_FORWARD = 0, 1
# traffic/status.py:10-61 (and the two ScenarioStatus values the reference stores in traffic_status)
NORMAL, COMPLETED, TIME_EXCEEDED, OUT_BOUND, NO_ACTION, OFF_LANE = 1, 2, 3, 4, 5, 6


# ------------------------------------------------------------------------------------------------------------ the box
def boxes(oracle, rows, type_id, x, y, heading):
    """(pose float64 [n, 4, 2], boxed bool [n]) of n egos: t2do_pose_obb with the deterministic trig for box-shaped types
    with a finite pose, as the event kernels state it"""
    n = len(x)
    rows = np.ascontiguousarray(rows, np.float64)
    pose = np.zeros((n, 8)); xy = np.zeros((n, 2)); is_obb = np.zeros(n, np.uint8)
    g = oracle.lib().t2do_ego_poses
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
    g.argtypes = [f64p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, u8p, C.c_int, f64p, f64p, u8p]
    g(rows, rows.shape[1], n, 1, 0, np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32),
      np.ascontiguousarray(heading, np.float32), np.ascontiguousarray(type_id, np.uint8), 0, pose.reshape(-1), xy.reshape(-1), is_obb)
    return pose.reshape(n, 4, 2), is_obb.astype(bool)


# ------------------------------------------------------------------------------------------------ the predicate, fp64
def touch_many(Q, V):
    """Q float64 [m, 4, 2] boxes (CCW), V float64 [m, 4, 2] tile rings -> bool [m]: an edge of the ring meets the closed box.
    side[k][v] = (Q[k+1] - Q[k]) x (V[v] - Q[k]) < 0: vertex v strictly outside box edge k;  s[i][k] = (V[i+1] - V[i]) x
    (Q[k] - V[i]): the box strictly on one side of edge i when all four share a strict sign."""
    Q = np.asarray(Q, F64); V = np.asarray(V, F64)
    Qn = np.roll(Q, -1, axis=1)
    ex = (Qn[:, :, 0] - Q[:, :, 0])[:, :, None]; ey = (Qn[:, :, 1] - Q[:, :, 1])[:, :, None]          # [m, k, 1]
    rx = V[:, None, :, 0] - Q[:, :, None, 0]; ry = V[:, None, :, 1] - Q[:, :, None, 1]                # [m, k, v]
    out = (ex * ry - ey * rx) < 0.0                                                                    # [m, k, v]
    Vn = np.roll(V, -1, axis=1)
    dx = (Vn[:, :, 0] - V[:, :, 0])[:, :, None]; dy = (Vn[:, :, 1] - V[:, :, 1])[:, :, None]          # [m, i, 1]
    wx = Q[:, None, :, 0] - V[:, :, None, 0]; wy = Q[:, None, :, 1] - V[:, :, None, 1]                # [m, i, k]
    s = dx * wy - dy * wx
    one_side = (s > 0.0).all(axis=2) | (s < 0.0).all(axis=2)                                           # [m, i]
    both_out = (out & np.roll(out, -1, axis=2)).any(axis=1)                                            # [m, i]: vertices i and i + 1
    return (~(both_out | one_side)).any(axis=1)


def touch(Q, V):
    return bool(touch_many(np.asarray(Q, F64)[None], np.asarray(V, F64)[None])[0])


# ---------------------------------------------------------------------------------------------- the predicate, exact
def _fr(a):
    return [[Fraction(float(c)) for c in p] for p in a]


def touch_exact(Q, V):
    """The same verdict on exact rationals, by clipping: edge P0 + t (P1 - P0), t in [0, 1], cut by the four closed
    half-planes of the (CCW) box; the edge meets the box when an interval of t is left."""
    Q, V = _fr(Q), _fr(V)
    for i in range(4):
        p0, p1 = V[i], V[(i + 1) % 4]
        d = (p1[0] - p0[0], p1[1] - p0[1])
        lo, hi, ok = Fraction(0), Fraction(1), True
        for k in range(4):
            a, b = Q[k], Q[(k + 1) % 4]
            e = (b[0] - a[0], b[1] - a[1])
            f0 = e[0] * (p0[1] - a[1]) - e[1] * (p0[0] - a[0])   # >= 0: inside edge k
            g = e[0] * d[1] - e[1] * d[0]                         # f(t) = f0 + t g
            if g == 0:
                if f0 < 0:
                    ok = False
            elif g > 0:
                lo = max(lo, -f0 / g)
            else:
                hi = min(hi, -f0 / g)
            if not ok or lo > hi:
                ok = False
                break
        if ok:
            return True
    return False


# ----------------------------------------------------------------------------------------- the forward rule, directly
def locate_forward(touched, tile_visiting, visited, max_advance):
    """the forward rule stated directly: offsets from tile_visiting, the run [j0, j1) inside the window, the gap (0, j0)"""
    n = len(touched)
    visited = list(visited)
    looked = n if max_advance <= 0 or max_advance >= n else max_advance + 1
    offs = [touched[(tile_visiting + j) % n] for j in range(looked)]
    if not any(offs):
        return [], tile_visiting, visited
    j0 = offs.index(True)
    j1 = j0
    while j1 < looked and offs[j1]:
        j1 += 1
    for j in list(range(1, j0)) + list(range(j0, j1)):
        visited[(tile_visiting + j) % n] = True
    return [(tile_visiting + j) % n for j in range(j0, j1)], (tile_visiting + j1 - 1) % n, visited


# ------------------------------------------------------------------------------------------ status and reward, scalar
def status_reward(pool_scen, pool_traf, off_lane, check_off_road, all_visited, n_tile, cnt_step, num_visited):
    """check_status (racing.py:339-369) decided by the pool's status bytes, then _get_rewards (:121-139) in Python floats
    (fp64, the reference's expressions) -> (scenario, traffic, terminated, truncated, float32 reward)"""
    scen = traf = NORMAL
    if pool_scen == TIME_EXCEEDED:
        scen = TIME_EXCEEDED
    elif pool_traf == NO_ACTION:
        traf = NO_ACTION
    elif pool_scen == OUT_BOUND:
        traf = OUT_BOUND
    elif check_off_road and off_lane:
        traf = OFF_LANE
    elif all_visited:
        scen = COMPLETED
    if scen == TIME_EXCEEDED:            # (scenario_status is never NO_ACTION: racing.py:351 puts it into traffic_status)
        reward = -1
    elif traf == OUT_BOUND or traf == OFF_LANE:
        reward = -5
    elif scen == COMPLETED:
        reward = (n_tile - 0.1 * cnt_step) / n_tile * 100
    else:
        time_penalty = -0.1 * cnt_step
        tile_reward = 0.1 * num_visited
        reward = time_penalty + tile_reward
    terminated = scen == COMPLETED
    truncated = not terminated and (scen != NORMAL or traf != NORMAL)
    return scen, traf, terminated, truncated, np.float32(reward)


# --------------------------------------------------------------------------------------------- every env at once
def pack(visited):
    """bool [E, <= MAX_TILES] -> uint32 [E, WORDS]"""
    v = np.zeros((visited.shape[0], MAX_TILES), bool)
    v[:, :visited.shape[1]] = visited
    return np.ascontiguousarray(np.packbits(v, axis=1, bitorder="little")).view("<u4")


class Progress:
    """The state t2d_set_tracks / t2d_track_reset / t2d_track_upload / t2d_track_progress keep, for E envs.
    tracks: list of float32 [n_tile, 4, 2]; set_of_env int [E]."""

    PREFILTER_MARGIN = 1.0   # m; see touched()

    def __init__(self, tracks, set_of_env, rule, max_advance, check_off_road=False):
        self.tracks = [np.asarray(t, np.float32).reshape(-1, 4, 2) for t in tracks]
        self.set_of_env = np.asarray(set_of_env, np.int64)
        self.E = len(self.set_of_env)
        self.n_tile = np.array([len(self.tracks[s]) for s in self.set_of_env])
        self.T = int(max(len(t) for t in self.tracks))
        self.rule, self.max_advance, self.check_off_road = rule, int(max_advance), bool(check_off_road)
        # padded per-set tables: vertices (fp64, exact) and bounding boxes
        S = len(self.tracks)
        self.V = np.zeros((S, self.T, 4, 2))
        for s, t in enumerate(self.tracks):
            self.V[s, :len(t)] = t.astype(F64)
        self.lo = self.V.min(axis=2); self.hi = self.V.max(axis=2)          # [S, T, 2]
        self.valid = np.arange(self.T)[None, :] < np.array([len(t) for t in self.tracks])[:, None]
        self.visiting = np.zeros(self.E, np.int64)
        self.visited = np.zeros((self.E, self.T), bool)
        self.status = np.zeros((self.E, 4), np.uint8)
        self.reward = np.zeros(self.E, np.float32)
        self.reset()

    # -- t2d_track_reset / t2d_track_upload
    def reset(self, env_mask=None):
        v = np.zeros((self.E, self.T), bool); v[:, 0] = True
        self.upload(np.zeros(self.E, np.int64), v, env_mask)

    def upload(self, visiting, visited, env_mask=None):
        m = np.ones(self.E, bool) if env_mask is None else np.asarray(env_mask, bool)
        self.visiting[m] = np.asarray(visiting)[m]
        self.visited[m] = np.asarray(visited, bool)[m, :self.T]
        self.status[m] = (NORMAL, NORMAL, 0, 0)
        self.reward[m] = 0
        if not hasattr(self, "start_visiting"):
            self.start_visiting, self.start_visited = self.visiting.copy(), self.visited.copy()
        self.start_visiting[m] = self.visiting[m]
        self.start_visited[m] = self.visited[m]

    @property
    def num_visited(self):
        return self.visited.sum(axis=1).astype(np.int32)

    def mask(self):
        return pack(self.visited)

    # -- the predicate for every (env, tile)
    def touched(self, Q, boxed):
        """bool [E, T].  The exact predicate is evaluated on the pairs whose bounding boxes come within PREFILTER_MARGIN of
        each other; a tile further away than that cannot touch (the predicate's rounding errors are of the order of
        1e-13 m at these coordinates), so the result is the predicate's on every pair."""
        s = self.set_of_env
        qlo, qhi = Q.min(axis=1), Q.max(axis=1)                               # [E, 2]
        m = self.PREFILTER_MARGIN
        near = ((self.lo[s] <= (qhi + m)[:, None, :]) & (self.hi[s] >= (qlo - m)[:, None, :])).all(axis=2)
        near &= self.valid[s] & np.asarray(boxed, bool)[:, None]
        e, t = np.nonzero(near)
        out = np.zeros((self.E, self.T), bool)
        if len(e):
            out[e, t] = touch_many(Q[e], self.V[s[e], t])
        return out

    # -- t2d_track_progress
    def step(self, Q, boxed, pool_status, ego_flags, cnt_step, touched=None):
        """One launch.  Q float64 [E, 4, 2], boxed bool [E] (boxes()); pool_status uint8 [E, 4], ego_flags uint32 [E],
        cnt_step int [E]: T2D_F_STATUS, the ego's T2D_F_FLAGS and T2D_F_CNT_STEP as the step left them.
        Returns the run as (j0, j1) offset arrays (j0 = -1: empty)."""
        E, T, n = self.E, self.T, self.n_tile
        restart = (self.status[:, 2] | self.status[:, 3]) != 0
        self.visiting[restart] = self.start_visiting[restart]
        self.visited[restart] = self.start_visited[restart]
        if touched is None:
            touched = self.touched(Q, boxed)
        whole = (self.rule == RULE_REFERENCE) | (self.max_advance <= 0) | (self.max_advance >= n)
        limit = np.where(whole, n, self.max_advance + 1)
        j = np.arange(T + 1)[None, :]
        tile = (self.visiting[:, None] + j) % n[:, None]
        hit = np.take_along_axis(touched, np.minimum(tile, T - 1), axis=1) & (j < limit[:, None])      # [E, T + 1]
        any_hit = hit.any(axis=1)
        j0 = np.where(any_hit, hit.argmax(axis=1), -1)
        miss_after = ~hit & (j > j0[:, None])
        j1 = np.where(any_hit, miss_after.argmax(axis=1), -1)      # (column `limit` <= T is always a miss)
        all_ = (self.rule == RULE_REFERENCE) & (j0 == 0) & (j1 == 1)
        lo = np.where(j0 == 0, 0, 1)
        a = (self.visiting + lo) % n
        length = np.where(all_, n, j1 - lo)
        t = np.arange(T)[None, :]
        d = (t - a[:, None]) % n[:, None]
        mark = any_hit[:, None] & (d < length[:, None]) & (t < n[:, None])
        self.visited |= mark
        self.visiting = np.where(any_hit, (self.visiting + j1 - 1) % n, self.visiting)
        nv = self.num_visited
        for e in range(E):
            sc, tr, te, tu, rw = status_reward(int(pool_status[e, 0]), int(pool_status[e, 1]), bool(int(ego_flags[e]) & 8),
                                               self.check_off_road, int(nv[e]) == int(n[e]), int(n[e]), int(cnt_step[e]), int(nv[e]))
            self.status[e] = (sc, tr, te, tu)
            self.reward[e] = rw
        return j0, j1


# ------------------------------------------------------------------------------------------------------ hand-made cases
def kats():
    """(name, box float64 [4, 2] CCW, tile float32 [4, 2], touches) where every operation of the predicate is exact.
    The box is the unit-ish square [0, 4] x [0, 2]."""
    Q = np.array([[4.0, 0.0], [4.0, 2.0], [0.0, 2.0], [0.0, 0.0]])
    up = np.nextafter(np.float32(4.0), np.float32(5.0))          # one fp32 ulp right of the box's x = 4 side
    f = np.float32
    return [
        ("edge through the box", Q, f([[-1, 1], [5, 1], [5, 9], [-1, 9]]), True),
        ("edge inside the box", Q, f([[1, 0.5], [3, 0.5], [3, 9], [1, 9]]), True),
        ("box wholly inside the tile: touches nothing", Q, f([[-1, -1], [5, -1], [5, 3], [-1, 3]]), False),
        ("tile vertex on a box edge", Q, f([[4, 1], [6, 0], [7, 3], [6, 4]]), True),
        ("box vertex on a tile edge", Q, f([[3, 3], [5, 1], [8, 1], [8, 3]]), True),
        ("collinear overlap with a box side", Q, f([[4, 1], [4, 5], [6, 5], [6, 1]]), True),
        ("collinear with a box side, beyond it", Q, f([[4, 3], [4, 5], [6, 5], [6, 3]]), False),
        ("touching corner", Q, f([[4, 2], [6, 3], [7, 5], [5, 5]]), True),
        ("a miss by one ulp", Q, f([[up, -1], [up, 3], [6, 3], [6, -1]]), False),
        ("a hit at the ulp below", Q, f([[4, -1], [4, 3], [6, 3], [6, -1]]), True),
        ("non-convex tile", Q, f([[-2, -2], [6, -2], [2, 1], [6, 4]]), True),
        ("clockwise ring", Q, f([[-1, 9], [5, 9], [5, 1], [-1, 1]]), True),
        ("far away", Q, f([[10, 10], [12, 10], [12, 12], [10, 12]]), False),
    ]


def random_cases(n, seed):
    """boxes of a medium car at racing coordinates against quadrilaterals of tile size nearby: roughly half touch, and a share
    is made nearly degenerate (a tile vertex put on a box edge up to fp32 rounding)"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        c = rng.uniform(-780, 780, 2)
        h = rng.uniform(0, 2 * np.pi)
        hl, hw = 0.5 * 4.284, 0.5 * 1.799
        R = np.array([[np.cos(h), -np.sin(h)], [np.sin(h), np.cos(h)]])
        Q = (np.array([[hl, -hw], [hl, hw], [-hl, hw], [-hl, -hw]]) @ R.T + c).astype(F64)
        tc = c + rng.uniform(-9, 9, 2)
        th = rng.uniform(0, 2 * np.pi)
        Rt = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        V = (np.array([[-5, 2.5], [5, 2.5], [5, -2.5], [-5, -2.5]]) * rng.uniform(0.2, 1.2, (4, 2)) @ Rt.T + tc)
        if k % 4 == 0:   # a vertex on a box edge, up to the fp32 rounding of its coordinates
            s = rng.uniform(0, 1)
            i = rng.integers(4)
            V[rng.integers(4)] = Q[i] + s * (Q[(i + 1) % 4] - Q[i])
        yield Q, V.astype(np.float32)
