"""Scenes that SATURATE the step kernel's per-wave candidate queues (tactics2d_amd/csrc/t2d_collide.hip: compact_and_process, kQueueCap
entries per wave and round) and its box sweeps -- test infrastructure for tests/test_saturation_scenes.py (preconditions, CPU) and
tests/test_gpu_saturation.py.  The random scenes of tests/test_gpu_collide.py stay below the capacity in every wave (its docstring
has the counts); here a wave has several times the capacity in candidates and only a few of them are contacts, each of which alone
decides some participant's flag: a queue entry that is lost, in any round, shows as a wrong flag.

Participants sit at heading 0 (exact sine and cosine) on dyadic coordinates within |x|, |y| <= 16 m.

    needle_scene     one type, a 4.0 x 0.05 m box.  An env is a stack of needles in y, pitch 9/128 m, agent -> slot a random permutation;
                     every bounding circle (R = 2.0002 m) meets nearly every other, so a wave of A_pad-agent envs has 64 / A_pad x
                     A (A - 1) / 2 candidate pairs.  Contacts: the upper needle of disjoint adjacent slot pairs is lowered by 1/32 m into
                     its partner (gaps elsewhere: 0.02 m and more) -- a contacting pair is the only contact of both its members.
                     grid=True (A_pad 128 / 256: the LDS hash grid): successive slots alternate between x = -1/64 and +1/64, the two cell
                     columns either side of x = 0, and the stack runs through several cell rows (cell edge 4.005 m).  Where a cell row
                     ends inside the stack the pair across it is made a contact: with the columns alternating it crosses diagonally, in
                     every other env the upper slot repeats its partner's column and the pair crosses in y alone.
    slat_scene       K thin quads at 45 degrees, 17 / sqrt(2) = 12.02 m long, stacked along their normal, listed in a random order per
                     env, as static obstacles or as lanes; participants are 0.125 m boxes near the middle of the stack.  In the rotated
                     coordinates u = y - x, v = x + y (dyadic u, v give dyadic x, y) a slat is [u_k - t, u_k + t] x [-8.5, 8.5] with
                     u_k a multiple of the pitch 45/64 (0.4972 m along the normal: half a metre to the nearest dyadic in u), and a box
                     is u_c -+ 0.125.  Half thickness t: static 3/64 (0.0663 m thick), lane 17/64 (0.3757 m), overlapping lanes 51/128
                     (0.5635 m: neighbours share a strip 3/32 wide in u).  A box meets the axis-aligned boxes of the ~24 slats within
                     8.6 of it in u, touches at most one static slat and lies in at most two lanes.
    combined_scene   needles, static slats and lane slats in one env (the launch forms of t2d_step_n).

Every builder returns the dict of helpers.random_scene plus
    witness   bool [N]: the participants whose flag (`bit`) is meant to be set -- worked out here in exact dyadic arithmetic, not by the
              oracle (combined_scene: uint32 [N], the three flags as a word)
    bit       the flag bit(s) the scene is about
Counting (what the preconditions assert):
    wave_lower_bounds(sc)   per wave of the kernel (64 consecutive lanes of env_local * A_pad + agent), a LOWER bound on the candidates
                            its broad phases must accept, per call of compact_and_process (one per 64-box chunk of a polygon list)
    sole_witnesses(sc)      queue entries that alone decide some participant's flag
"""
import os
import re

import numpy as np

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDLE = (4.0, 0.05)
NEEDLE_PITCH = 9.0 / 128          # 0.0703125: a gap of 0.0203 m between neighbours
NEEDLE_DROP = 1.0 / 32            # the upper needle of a contact pair comes down by this: 0.0109 m deep in its partner
BOX = 0.125
T_NEEDLE, T_BOX, T_DISC = 0, 1, 2
U_PITCH = 45.0 / 64               # slat pitch in u = y - x
V_HALF = 8.5                      # slats reach v = x + y = -+ 8.5
T_STATIC, T_LANE, T_LANE_OVERLAP = 3.0 / 64, 17.0 / 64, 51.0 / 128
F_DYNAMIC, F_STATIC, F_OFF_LANE = 1, 2, 8
# a static quad far from every participant: it gives the lane scenes the static stage without which a 64-agent pool does not take
# the one-workgroup-per-env form (plan_step's split wants both stages)
DECOY = np.float32([[14.0, -15.0], [15.0, -15.0], [15.0, -14.0], [14.0, -14.0]])


def queue_cap():
    """kQueueCap as the kernel's source has it"""
    src = open(os.path.join(ROOT, "tactics2d_amd", "csrc", "t2d_collide.hip")).read()
    m = re.search(r"constexpr\s+int\s+kQueueCap\s*=\s*(\d+)\s*;", src)
    assert m, "constexpr int kQueueCap not found in t2d_collide.hip"
    return int(m.group(1))


def rows():
    """needle, 0.125 m box, and a disc nobody uses (a type table with a disc keeps one-agent pools on the general step kernel)"""
    out = []
    for (L_, W_) in (NEEDLE, (BOX, BOX)):
        r = np.zeros(24); r[0] = 0; r[1] = 1.2; r[2] = 1.3; r[3] = 2.5; r[17] = 5; r[18] = 0; r[19] = L_; r[20] = W_
        out.append(r)
    r = np.zeros(24); r[0] = 2; r[17] = 5; r[18] = 1; r[19] = BOX; r[20] = BOX
    out.append(r)
    return np.array(out)


def cell_edge():
    """the hash grid's cell edge for this type table (t2d_set_param_table: 1.001 x the largest circum-diameter + 1 mm)"""
    return float(np.hypot(*NEEDLE)) * 1.001 + 1e-3


def _scene(n_env, A, x, y, tid, active, witness, bit, **kw):
    N = n_env * A
    sc = dict(rows=rows(), n_env=n_env, A=A, x=np.float32(x).reshape(N), y=np.float32(y).reshape(N), heading=np.zeros(N, np.float32),
              type_id=np.uint8(tid).reshape(N), active=np.uint8(active).reshape(N), static=None, lanes=None, boundary=None,
              boundary_valid=None, witness=np.asarray(witness, bool).reshape(N), bit=bit)
    sc.update(kw)
    assert np.array_equal(np.float64(sc["x"]), np.float64(x).reshape(N)) and np.array_equal(np.float64(sc["y"]), np.float64(y).reshape(N)), \
        "positions must be exact in fp32"
    return sc


# ------------------------------------------------------------------------------------------------------------------- needles
def _needle_stack(rng, n, grid, env, shift, cx=0.0, cy=0.0):
    """(x, y, contact) of the n slots of one stack, bottom to top; contact[s]: slot s is the upper needle of a contact pair (s - 1, s)"""
    s = np.arange(n)
    y = cy + (s - (n - 1) / 2.0) * NEEDLE_PITCH
    x = np.full(n, cx)
    forced = np.zeros(n, bool)
    if grid:
        x = cx + np.where(s % 2 == 0, -1.0, 1.0) / 64
        row = np.floor(np.float64(np.float32(y + shift[1])) / cell_edge())
        low = np.floor(np.float64(np.float32(y - NEEDLE_DROP + shift[1])) / cell_edge())
        # slot t starts a new cell row, and still does once lowered: (t - 1, t) becomes a contact
        for t in np.flatnonzero((row[1:] != row[:-1]) & (low[1:] != row[:-1])) + 1:
            forced[t] = True
            if env % 2 == 0:
                x[t] = x[t - 1]                                # same column: the contact crosses in y alone
    # a free adjacent pair becomes a contact with probability q: q / (1 + q) contacts a needle, flag share 2 q / (1 + q) = 0.47.  On the
    # grid 0.62: a needle of a 200-stack has ~48 candidate partners above it, and its contacts are to stay past 0.5 % of them
    q = 0.45 if grid else 0.31
    contact = np.zeros(n, bool)
    taken = np.zeros(n + 1, bool)
    for t in np.flatnonzero(forced):
        contact[t] = True; taken[t - 1] = taken[t] = True
    t = 1
    while t < n:
        if not taken[t - 1] and not taken[t] and rng.random() < q:
            contact[t] = True; taken[t - 1] = taken[t] = True
            t += 2
        else:
            t += 1
    y = y - NEEDLE_DROP * contact
    return x, y, contact


def needle_scene(n_env, A, seed=0, inactive=0, grid=False, shift=(0.0, 0.0)):
    """inactive: that many agents of every env (chosen at random) are inactive: parked lanes among full ones.  shift: added to every
    position (the hash grid's cells are global)"""
    rng = np.random.default_rng([seed, n_env, A, inactive, int(grid)])
    x = np.zeros((n_env, A)); y = np.zeros((n_env, A)); active = np.ones((n_env, A), np.uint8); wit = np.zeros((n_env, A), bool)
    partner = np.full((n_env, A), -1)
    n = A - inactive
    for e in range(n_env):
        perm = rng.permutation(A)               # perm[slot] = agent; the last `inactive` of them sit out
        xs, ys, contact = _needle_stack(rng, n, grid, e, shift)
        ag = perm[:n]
        x[e, ag], y[e, ag] = xs, ys
        active[e, perm[n:]] = 0
        up = np.flatnonzero(contact)
        wit[e, ag[up]] = wit[e, ag[up - 1]] = True
        partner[e, ag[up]], partner[e, ag[up - 1]] = ag[up - 1], ag[up]
    return _scene(n_env, A, x + shift[0], y + shift[1], np.full((n_env, A), T_NEEDLE), active, wit, F_DYNAMIC, partner=partner.reshape(-1),
                  kind="needles")


# --------------------------------------------------------------------------------------------------------------------- slats
def _slat(u, t):
    """the quad [u - t, u + t] x [-V_HALF, V_HALF] of the (u, v) plane in x = (v - u) / 2, y = (v + u) / 2, counter-clockwise"""
    uv = np.array([[u - t, -V_HALF], [u - t, V_HALF], [u + t, V_HALF], [u + t, -V_HALF]])
    return np.float32(np.stack([(uv[:, 1] - uv[:, 0]) / 2, (uv[:, 1] + uv[:, 0]) / 2], 1))


def _box_uv(rng, n, K_slots, u0):
    """u, v of n boxes: u on the 1/64 grid over the middle 20 % of a stack of K_slots slats centred on u0 (one pitch at the least, so
    that boxes lie on and between slats), v on the 1/32 grid within -+ 45/64 (0.5 m along the slats)"""
    span = max(0.2 * K_slots * U_PITCH, U_PITCH)
    half = int(round(span * 64 / 2))
    u = u0 + rng.integers(-half, half + 1, n) / 64.0
    v = rng.integers(-22, 23, n) / 32.0
    return u, v


def _static_witness(u_box, u_slats):
    """a box u_c -+ BOX meets the closed slat u_k -+ t: |u_c - u_k| <= t + BOX (exact in dyadic arithmetic; touching counts)"""
    d = np.abs(u_box[:, None] - np.asarray(u_slats)[None, :])
    return d <= T_STATIC + BOX


def _lane_terms(u_box, u_slats, t):
    """per (box, slat): centre in the slat; a piece of the union's outline that is part of the slat runs through the open box"""
    u_slats = np.asarray(u_slats, np.float64)
    lo, hi = u_slats - t, u_slats + t
    inside = (u_box[:, None] >= lo[None, :]) & (u_box[:, None] <= hi[None, :])
    # an end of a slat is on the union's outline unless another slat covers it (closed: dyadic ends never coincide here)
    def exposed(p):
        return ~((p[:, None] >= lo[None, :]) & (p[:, None] <= hi[None, :]) & ~np.eye(len(u_slats), dtype=bool)).any(1)
    cut = np.zeros_like(inside)
    for ends, ex in ((lo, exposed(lo)), (hi, exposed(hi))):
        cut |= ex[None, :] & (np.abs(u_box[:, None] - ends[None, :]) < BOX)
    return inside, cut


def _off_lane(inside, cut, keep=None):
    if keep is not None:
        inside, cut = inside & keep, cut & keep
    return ~(inside.any(1) & ~cut.any(1))


def slat_scene(n_env, A, K, stage, seed=0):
    """stage: "static", "lane" or "lane_overlap" (thicker slats of which a random three in four are there: neighbours overlap, and
    boxes straddle the shared strip -- inside the union and inside neither slat alone -- or stand in a gap)"""
    rng = np.random.default_rng([seed, n_env, A, K, ("static", "lane", "lane_overlap").index(stage)])
    x = np.zeros((n_env, A)); y = np.zeros((n_env, A)); wit = np.zeros((n_env, A), bool)
    polys, us = [], []
    for e in range(n_env):
        if stage == "lane_overlap":
            slots = K + max(1, K // 3)
            k = np.sort(rng.choice(slots, K, replace=False))
        else:
            slots, k = K, np.arange(K)
        u_sl = (k - (slots - 1) / 2.0) * U_PITCH
        u_sl = u_sl[rng.permutation(K)]                    # listed in a random order
        u, v = _box_uv(rng, A, slots, 0.0)
        x[e], y[e] = (v - u) / 2, (v + u) / 2
        t = {"static": T_STATIC, "lane": T_LANE, "lane_overlap": T_LANE_OVERLAP}[stage]
        polys.append([_slat(q, t) for q in u_sl])
        us.append(u_sl)
        wit[e] = _static_witness(u, u_sl).any(1) if stage == "static" else _off_lane(*_lane_terms(u, u_sl, t))
    csr = H.to_csr(polys)
    kw = dict(static=csr) if stage == "static" else dict(lanes=csr, static=H.to_csr([[DECOY]] * n_env))
    return _scene(n_env, A, x, y, np.full((n_env, A), T_BOX), np.ones((n_env, A)), wit, F_STATIC if stage == "static" else F_OFF_LANE,
                  slat_u=us, slat_t=t, kind=stage, **kw)


# ------------------------------------------------------------------------------------------------------------------ combined
K_COMBINED_STATIC = 24
K_COMBINED_LANE = {64: 33, 16: 28}     # (16: fewer lanes under the needles, which bring candidates and no sole witness)
U0_BOXES = 2.8125                 # the boxes' place: the middle of the static stack
NEEDLES_AT = (5.0, -5.0)          # u = -10: the stack occupies u in [-13.7, -6.3], the static slats start at u = -5.3


def combined_needles(A):
    """needles per env: 44 of 64 (946 pairs a wave; 20 boxes x 24 slats is what remains for the static stage), 13 of 16"""
    return {64: 44, 16: 13}[A]


def combined_scene(n_env, A, seed=0):
    """needles round (5, -5), clear of the static slats and across the lower lane slats (off-lane, all of them); boxes round the
    middle of the static stack; the lane stack reaches from the needles to the boxes.  witness / bit: the three flags together"""
    rng = np.random.default_rng([seed, n_env, A, 4])
    nn = combined_needles(A)
    x = np.zeros((n_env, A)); y = np.zeros((n_env, A)); tid = np.zeros((n_env, A), np.uint8); wit = np.zeros((n_env, A), np.uint32)
    partner = np.full((n_env, A), -1)
    st, ln, us_s, us_l = [], [], [], []
    u_static = U0_BOXES + (np.arange(K_COMBINED_STATIC) - (K_COMBINED_STATIC - 1) / 2.0) * U_PITCH
    K_l = K_COMBINED_LANE[A]
    u_lane = u_static[-1] - np.arange(K_l) * U_PITCH + 15.0 / 64     # (off the static slats' centres)
    for e in range(n_env):
        perm = rng.permutation(A)
        ag, bx = perm[:nn], perm[nn:]
        xs, ys, contact = _needle_stack(rng, nn, False, e, (0.0, 0.0), *NEEDLES_AT)
        x[e, ag], y[e, ag] = xs, ys
        up = np.flatnonzero(contact)
        wit[e, ag[up]] |= F_DYNAMIC; wit[e, ag[up - 1]] |= F_DYNAMIC
        partner[e, ag[up]], partner[e, ag[up - 1]] = ag[up - 1], ag[up]
        wit[e, ag] |= F_OFF_LANE
        u, v = _box_uv(rng, len(bx), K_COMBINED_STATIC, U0_BOXES)
        x[e, bx], y[e, bx] = (v - u) / 2, (v + u) / 2
        tid[e, bx] = T_BOX
        touch = (np.abs(x[e, bx][:, None] - x[e, bx][None, :]) <= BOX) & (np.abs(y[e, bx][:, None] - y[e, bx][None, :]) <= BOX)
        wit[e, bx] |= np.where((touch & ~np.eye(len(bx), dtype=bool)).any(1), F_DYNAMIC, 0).astype(np.uint32)   # (boxes on boxes)
        us, ul = u_static[rng.permutation(K_COMBINED_STATIC)], u_lane[rng.permutation(K_l)]
        wit[e, bx] |= np.where(_static_witness(u, us).any(1), F_STATIC, 0).astype(np.uint32)
        wit[e, bx] |= np.where(_off_lane(*_lane_terms(u, ul, T_LANE)), F_OFF_LANE, 0).astype(np.uint32)
        st.append([_slat(q, T_STATIC) for q in us]); ln.append([_slat(q, T_LANE) for q in ul])
        us_s.append(us); us_l.append(ul)
    sc = _scene(n_env, A, x, y, tid, np.ones((n_env, A)), np.zeros((n_env, A)), F_DYNAMIC | F_STATIC | F_OFF_LANE, static=H.to_csr(st),
                lanes=H.to_csr(ln), partner=partner.reshape(-1), kind="combined", slat_u_static=us_s, slat_u_lane=us_l)
    sc["witness"] = wit.reshape(-1)       # (here: the flag word, not a mask)
    return sc


def tiled(sc, times):
    """the scene's envs repeated `times` times (a pool large enough for the chained form, with the oracle's answer for the first copy)"""
    out = dict(sc)
    out["n_env"] = sc["n_env"] * times
    for k in ("x", "y", "heading", "type_id", "active"):
        out[k] = np.tile(sc[k], times)
    for k in ("static", "lanes"):
        if sc[k] is not None:
            eo, vo, xy = sc[k]
            P, V = eo[-1], vo[-1]
            out[k] = (np.concatenate([[0]] + [eo[1:] + c * P for c in range(times)]).astype(np.int32),
                      np.concatenate([[0]] + [vo[1:] + c * V for c in range(times)]).astype(np.int32), np.tile(xy, (times, 1)))
    return out


# ------------------------------------------------------------------------------------------------------------------ counting
def a_pad(A):
    """lanes per env: A rounded up to a power of two, two at the least (launch_collide)"""
    p = 2
    while p < A:
        p *= 2
    return p


def geometry_fits(sc):
    """mapgeom.geometry_budget of the scene: whether its static and lane geometry stays on the LDS record, and the envs per
    workgroup of one wave (their lanes are env_local * A_pad + agent) -- the library's own answer, no device is touched.  (A pool
    may put two or four such waves in a workgroup: the envs of a wave stay the same.)"""
    from tactics2d_amd import mapgeom
    return mapgeom.geometry_budget(sc["n_env"], sc["A"], sc["static"], sc["lanes"])


def envs_per_workgroup(sc):
    return geometry_fits(sc)["envs_per_workgroup"]


def _pose_boxes(sc):
    half = sc["rows"][sc["type_id"], 19:21] / 2
    x, y = np.float64(sc["x"]), np.float64(sc["y"])
    return x - half[:, 0], x + half[:, 0], y - half[:, 1], y + half[:, 1]


def _poly_boxes(csr):
    eo, vo, xy = csr
    xy = np.float64(xy)
    mins = np.minimum.reduceat(xy, vo[:-1], 0); maxs = np.maximum.reduceat(xy, vo[:-1], 0)
    return eo, mins[:, 0], maxs[:, 0], mins[:, 1], maxs[:, 1]


N_CHUNKS = 3     # 64-box chunks of the longest polygon list here (K = 130)


def candidate_lower_bounds(sc, split=False):
    """per participant: pairs[i] = partners j > i (same env) whose centre lies within R_i + R_j - 1 mm (the kernel's circles carry
    5 mm each: it must accept these), and per polygon stage [N, N_CHUNKS]: the polygons whose box overlaps the exact pose box by
    1 mm or more in both axes (the kernel's pose box is rounded outwards), by the 64-box chunk of the env's list they are in --
    sweep_stage compacts and works off one chunk at a time, so a chunk is what one call of compact_and_process sees.  split: the
    one-workgroup-per-env form, whose lane stage runs on two waves, each with the first / second half of the env's lane list and
    a queue of its own: [N, 2 * N_CHUNKS], the chunks of the first half, then of the second.  Inactive participants count nothing."""
    n_env, A = sc["n_env"], sc["A"]
    act = sc["active"].reshape(n_env, A).astype(bool)
    R = (0.5 * np.hypot(sc["rows"][:, 19], sc["rows"][:, 20]))[sc["type_id"]].reshape(n_env, A)
    x, y = np.float64(sc["x"]).reshape(n_env, A), np.float64(sc["y"]).reshape(n_env, A)
    d = np.hypot(x[:, :, None] - x[:, None, :], y[:, :, None] - y[:, None, :])
    near = (d <= R[:, :, None] + R[:, None, :] - 1e-3) & act[:, :, None] & act[:, None, :]
    out = dict(pairs=np.triu(near, 1).sum(2).reshape(-1))
    lo_x, hi_x, lo_y, hi_y = (q.reshape(n_env, A) for q in _pose_boxes(sc))
    for name, key in (("static", "static"), ("lanes", "lanes")):
        halves = split and name == "lanes"
        cnt = np.zeros((n_env, A, (2 if halves else 1) * N_CHUNKS), int)
        if sc[key] is not None:
            eo, pxl, pxh, pyl, pyh = _poly_boxes(sc[key])
            for e in range(n_env):
                s = slice(eo[e], eo[e + 1])
                ox = np.minimum(hi_x[e][:, None], pxh[s][None, :]) - np.maximum(lo_x[e][:, None], pxl[s][None, :])
                oy = np.minimum(hi_y[e][:, None], pyh[s][None, :]) - np.maximum(lo_y[e][:, None], pyl[s][None, :])
                meet = (ox >= 1e-3) & (oy >= 1e-3) & act[e][:, None]
                q = np.arange(eo[e + 1] - eo[e])
                chunk = q // 64
                if halves:      # (collide_kernel: mid = p0 + ((p1 - p0 + 1) >> 1))
                    mid = (len(q) + 1) // 2
                    chunk = np.where(q < mid, q // 64, N_CHUNKS + (q - mid) // 64)
                for c in np.unique(chunk):
                    cnt[e, :, c] = meet[:, chunk == c].sum(1)
        out[name] = cnt.reshape(n_env * A, -1)
    return out


def wave_lower_bounds(sc, epb=None, split=False):
    """dict stage -> per wave of the launch, the bound on the entries of its BUSIEST call of compact_and_process (pairs: the one
    call; polygon stages: the fullest 64-box chunk, see candidate_lower_bounds), stage + "_all" -> per wave, all its calls
    together, and `full`: the waves that hold as many participants as any wave of the launch does (64 where A is a power of two; 48
    at A = 48, the env's 16 idle lanes beside them; 32 at A = 1, whose envs take two lanes each; at A = 100 the first wave of each
    env, not the one with its last 36)"""
    n_env, A = sc["n_env"], sc["A"]
    P = a_pad(A)
    epb = envs_per_workgroup(sc) if epb is None else epb
    per = candidate_lower_bounds(sc, split)
    env = np.repeat(np.arange(n_env), A); agent = np.tile(np.arange(A), n_env)
    lane = (env % epb) * P + agent
    waves_per_wg = max(1, (epb * P + 63) // 64)
    wave = (env // epb) * waves_per_wg + lane // 64
    n_waves = ((n_env + epb - 1) // epb) * waves_per_wg
    out = {}
    for k, v in per.items():
        calls = np.stack([np.bincount(wave, weights=c, minlength=n_waves) for c in v.reshape(len(wave), -1).T], 1).astype(int)
        out[k], out[k + "_all"] = calls.max(1), calls.sum(1)
    held = np.bincount(wave, minlength=n_waves)
    out["full"] = held == held.max()
    out["epb"] = epb
    return out


def sole_witnesses(sc):
    """dict stage -> number of queue entries whose loss alone changes some participant's flag.  Pairs: every contact pair (it is the only
    contact of both members).  Static: a box touches at most one slat (t + BOX < pitch / 2): every touching (box, slat).  Lanes:
    (box, slat) entries without which the box's verdict turns -- the centre's only slat of a contained box (a box cut by the
    outline, or with its centre in no lane, stays off-lane whatever is lost)."""
    out = {}
    A = sc["A"]
    if "partner" in sc:
        out["pairs"] = int((sc["partner"] >= 0).sum()) // 2
    kind = sc["kind"]
    if kind in ("static", "combined"):
        n = 0
        for e, us in enumerate(sc["slat_u"] if kind == "static" else sc["slat_u_static"]):
            sel = np.flatnonzero(sc["type_id"][e * A:(e + 1) * A] == T_BOX) + e * A
            u = sc["y"][sel].astype(np.float64) - sc["x"][sel].astype(np.float64)
            hit = _static_witness(u, us)
            assert hit.sum(1).max(initial=0) <= 1
            n += int(hit.sum())
        out["static"] = n
    if kind in ("lane", "lane_overlap", "combined"):
        n = 0
        t = sc["slat_t"] if kind != "combined" else T_LANE
        for e, ul in enumerate(sc["slat_u"] if kind != "combined" else sc["slat_u_lane"]):
            sel = np.flatnonzero(sc["type_id"][e * A:(e + 1) * A] == T_BOX) + e * A
            u = sc["y"][sel].astype(np.float64) - sc["x"][sel].astype(np.float64)
            inside, cut = _lane_terms(u, ul, t)
            base = _off_lane(inside, cut)
            for p in np.flatnonzero((inside | cut).any(0)):
                keep = np.ones(len(ul), bool); keep[p] = False
                n += int((_off_lane(inside, cut, keep[None, :]) != base).sum())
        out["lanes"] = n
    return out


# --------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """one scene at one shape.  expect: stage -> m: in every full wave the lower bound on the entries of the stage's busiest call of
    compact_and_process is >= m x the queue capacity (m > 0: the largest whole multiple the construction guarantees) or below the
    capacity (m = 0); below: stage -> m: ... and stays under m x the capacity; split_expect: the same for the lane stage's busiest
    call in the one-workgroup-per-env form (half the lane list per wave); stages that are not named are counted and reported
    only.  stages: the stages the scene is about -- their
    flag share must lie in [0.2, 0.8] and their sole witnesses number >= 1000 and >= 0.5 % of the bound over the case's seeds.
    runs: what tests/test_gpu_saturation.py puts the case through."""

    def __init__(self, name, build, seeds, expect, stages, has_lanes=False, runs=("collide", "step"), below=None, split_expect=None):
        self.name, self.build, self.seeds, self.expect, self.stages, self.has_lanes, self.runs = name, build, seeds, expect, stages, has_lanes, runs
        self.below, self.split_expect = below or {}, split_expect

    def scene(self, seed):
        key = (self.name, seed)
        if key not in _cache:
            _cache[key] = self.build(seed)
        return _cache[key]

    def flags_of(self, sc):
        """the witnesses as a flag word under the scene's bits"""
        return sc["witness"].astype(np.uint32) * (sc["bit"] if sc["witness"].dtype == bool else 1)

    def __repr__(self):
        return self.name


_cache = {}
SLAT_KS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 130)
SLAT_SHAPES = ((1024, 1), (256, 4), (64, 16), (64, 64), (16, 100))
# The K that fit the 32 KiB LDS record at each shape (mapgeom.geometry_budget; a wave of one-agent envs carries 32 records, of
# four-agent envs 16, of 16-agent envs 4).  Dropped because they do not fit -- static: K >= 31 at A = 1, K >= 63 at A = 4; lanes (32 B
# per outline piece on top of the vertices): K >= 5 at A = 1, K >= 31 at A = 4, K >= 63 at A = 16.
SLAT_FITS = {"static": {1: (1, 3, 4, 5), 4: (1, 3, 4, 5, 31, 32, 33), 16: SLAT_KS, 64: SLAT_KS, 100: SLAT_KS},
             "lane": {1: (1, 3, 4), 4: (1, 3, 4, 5), 16: (1, 3, 4, 5, 31, 32, 33), 64: SLAT_KS, 100: SLAT_KS},
             "lane_overlap": {16: (4, 33), 64: (4, 33, 65), 100: (4, 33, 65)}}
# one case per stage that must NOT fit (it would run on the HBM grid tier, which tests/test_gpu_mapgrid.py covers): not run here
SLAT_DOES_NOT_FIT = (("static", 256, 4, 63), ("lane", 256, 4, 31))
SEEDS = (0, 1, 2)


def _slat_expect(K, stage):
    """whole capacities in the busiest call of a wave of 64 boxes.  K <= 4: 64 K entries, below the capacity; K = 5: 320, past it
    by 32 (not asserted).  K >= 31: 23 to 24 slats in reach of every box, ~1500 entries in one chunk (K <= 64): five capacities;
    K = 65 leaves one slat to a second chunk, at worst 64 entries fewer: four; K = 130 spreads the slats in reach over two chunks
    of 64 and one of 2: the fuller has (23 - 2) / 2 of them or more, 11 x 64 = 704: two.  Overlapping lanes: three slats in four
    are there, ~18 in reach, 905 and more counted: three."""
    if K <= 5:
        return 0 if K <= 4 else None
    if stage == "lane_overlap":
        return 3
    return 5 if K <= 64 else (4 if K == 65 else 2)


def _slat_split_expect(K, stage):
    """64 x 64 lane scenes step with one workgroup per env, the lane list halved between two waves: each call sees half the slats
    in reach -- 12 x 64 = 768, two capacities (K = 130: the fuller chunk of a half, the same) -- overlapping lanes ~9 x 64: one"""
    return None if K <= 5 else (1 if stage == "lane_overlap" else 2)


def _cases():
    out = []
    for (n, A, kw, m, seeds, tag) in (
            (64, 64, {}, 6, SEEDS, ""),                            # 2016 pairs less the 28 more than 56 slots apart: 1988, seven rounds
            (64, 48, {}, 3, SEEDS, ""), (64, 32, {}, 3, SEEDS, ""),     # 1128 pairs; 2 x 496
            (64, 16, {}, 1, (0, 1, 2, 3, 4), ""),                  # 4 x 120 pairs is all such a wave holds: exactly the second round
            (64, 8, {}, 0, tuple(range(10)), "_control"),          # 8 x 28 = 224 pairs: one round
            (64, 64, dict(inactive=32), 1, SEEDS, "_half_inactive")):   # 32 needles an env: 496 pairs, two rounds, 32 parked lanes
        out.append(Case(f"needles{tag}_{n}x{A}", lambda s, n=n, A=A, kw=kw: needle_scene(n, A, s, **kw), seeds, dict(pairs=m), ("pairs",),
                        below=dict(pairs=2) if m == 1 else None))
    for (n, A) in ((16, 100), (8, 200)):
        for shift, tag in (((0.0, 0.0), ""), (GRID_SHIFT, "_shifted")):
            out.append(Case(f"needles_grid{tag}_{n}x{A}", lambda s, n=n, A=A, shift=shift: needle_scene(n, A, s, grid=True, shift=shift),
                            (0, 1, 2, 3, 4), {}, ("pairs",)))
    for stage in ("static", "lane", "lane_overlap"):
        for (n, A) in SLAT_SHAPES:
            for K in SLAT_FITS[stage].get(A, ()):
                st = "static" if stage == "static" else "lanes"
                m = _slat_expect(K, stage)
                out.append(Case(f"slats_{stage}_{n}x{A}_K{K}", lambda s, n=n, A=A, K=K, stage=stage: slat_scene(n, A, K, stage, s), SEEDS,
                                {} if m is None else {st: m}, (st,), has_lanes=stage != "static",
                                split_expect=_slat_split_expect(K, stage) if st == "lanes" and A == 64 else None))
    # 64 lanes cannot carry three capacities in all three stages at once: the multiples below are the largest whole ones each
    # stage reaches.  44 needles + 20 boxes: 946 needle pairs (3 x); the boxes see 24 static slats each and the needles the six
    # nearest them: 708, 2.4 x the capacity, all that fits beside 44 needles (a needle clear of the slats has at most seven static
    # boxes in reach) (2 x, under 3 x); lanes 20 x 24 + 44 x 14 = 1100 and more (3 x; halved between the lane waves of the split
    # form: 1 x).  13 needles + 3 boxes: 4 x 78 pairs, the second round (1 x, under 2 x); statics 4 x (3 x 24 + 13 x 6) = 600 less
    # the slats a box near the stack's end does not reach: 575 counted, a hair under 2 x (1 x, under 3 x); 28 lanes of which a
    # needle has nine or ten in reach: 2.7 x (2 x, under 3 x)
    out.append(Case("combined_64x64", lambda s: combined_scene(64, 64, s), SEEDS, dict(pairs=3, static=2, lanes=3), ("pairs", "static", "lanes"),
                    has_lanes=True, runs=("collide", "step", "step_n"), below=dict(static=3), split_expect=1))
    out.append(Case("combined_64x16", lambda s: combined_scene(64, 16, s), tuple(range(14)), dict(pairs=1, static=1, lanes=2),
                    ("pairs", "static", "lanes"), has_lanes=True, runs=("collide", "step", "step_n"), below=dict(pairs=2, static=3, lanes=3)))
    return out


# The second variant of the grid scenes stands 2 km from the origin, moved by (-1000, +2000) m: the pitch 9/128, the drop 1/32 and the columns
# -+ 1/64 are multiples of 2^-8, the fp32 ulp at 2000 m is 2^-13 -- nothing is lost and the oracle's flags equal the witnesses there
# (asserted with every other case), so the shift is used as it stands.
GRID_SHIFT = (-1000.0, 2000.0)
CASES = _cases()
