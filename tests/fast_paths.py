"""Which arithmetic the `fast` integrators take, wave by wave -- a numpy restatement of the path predicates of
tactics2d_amd/csrc/t2d_integrate_dev.h -- and scenes built wave by wave so that every path is reached on purpose.

The fast code chooses per WAVE (by __ballot): a lane's result depends on the 63 lanes next to it.  `wave_paths` names the
path of every group of 64 consecutive participants (integrate_kernel: lane i = participant i; the fused step of an
(n / 64, 64) pool: one env per wave); the single-ego kernel's wave is four consecutive envs (group=4).

Kinematics (step_kinematics<1>), the order of the tests in the kernel:
    resummed     every lane `lane_resum`                                            (:268-289, needs kin_n > 0)
    linear/tiny  every lane `lane_linear`, every amax <= kEpsTiny: rotate_tiny     (:290-295)
    linear/small every lane `lane_linear`, some amax > kEpsTiny: rotate_small      (:296-299)
    piecewise    every lane linear or crossing a bound inside the step             (:327-378)
    plain        the sub_step loop                                                 (:380)
Dynamics (step_dynamics<1>):
    always_fast/* every lane `always_fast`: no |v| >= 0.1 test, two sub-steps per trip   (:478-515)
    general/*     the general loop                                                       (:522-558)
    */tiny        rotate_tiny in every sub-step (the whole wave below kEpsTiny)          (:503, :555)
    */small       some sub-step takes rotate_small, none re-seeds
    */reseed      some lane beyond kEpsMax in some sub-step: sincos_det(phi + beta)      (:505, :557)
"""
from dataclasses import dataclass, field

import numpy as np

from tactics2d_amd import layout as L

K_EPS_MAX = 0.1        # integ::kEpsMax (:32)
K_EPS_TINY = 0.01      # integ::kEpsTiny (:33)
K_RESUM_AMAX = 0.5     # integ::kResumAmax (:97)
K_RESUM_BMAX = 5e-3    # integ::kResumBmax (:98)
V_FAST = 0.1000001     # the always_fast threshold (:480)
INT_MAX = 0x7fffffff

KIN_PATHS = ("resummed", "linear/tiny", "linear/small", "piecewise", "plain")
DYN_PATHS = tuple(f"{loop}/{rot}" for loop in ("always_fast", "general") for rot in ("tiny", "small", "reseed"))

# margins of the scenes: every lane at least 20 % clear of the thresholds that define its class
EPS_TINY_IN = 0.008     # tiny: |eps| <= 0.008          (kEpsTiny 0.01)
EPS_SMALL_LO = 0.015    # small: 0.015 <= |eps| <= 0.08 (kEpsTiny 0.01, kEpsMax 0.1)
EPS_SMALL_HI = 0.08
EPS_RESEED = 0.15       # re-seed: |eps| >= 0.15        (kEpsMax 0.1)
V_HIGH = 0.12           # always_fast lanes: |v| >= 0.12 at both ends of the step (threshold 0.1)
V_LOW = 0.08            # low-speed lanes: |v| <= 0.08 in every sub-step
V_SCENE_MIN = 0.7       # slowest tyre-branch lane of the dynamics scenes (below ~0.67 m/s the reference's explicit Euler is unstable)


def _clipped_action(rows, tid, action):
    """the applied action: fp32 input, clipped in fp64 where the row's range flag says so (:176-178, :397-399)"""
    r = rows[tid]
    fl = r[:, L.P_RANGE_FLAGS].astype(int)
    a = np.float64(np.float32(action[:, 0]))
    d = np.float64(np.float32(action[:, 1]))
    a = np.where(fl & L.RANGE_ACCEL, np.clip(a, r[:, L.P_ACCEL_LO], r[:, L.P_ACCEL_HI]), a)
    d = np.where(fl & L.RANGE_STEER, np.clip(d, r[:, L.P_STEER_LO], r[:, L.P_STEER_HI]), d)
    return a, d


def _substeps(rows, tid, interval):
    dt_ms = rows[tid, L.P_DELTA_T_MS].astype(int)
    return dt_ms / 1000.0, interval // dt_ms, interval % dt_ms


# --------------------------------------------------------------------------- kinematics
def kin_lanes(rows, tid, state, action, interval, kin_n=0):
    """The per-lane predicates of step_kinematics<1> (:247-338), by the kernel's names."""
    rows = np.asarray(rows, np.float64)
    tid = np.asarray(tid).astype(int)
    r = rows[tid]
    accel, delta = _clipped_action(rows, tid, action)
    v = np.float64(np.float32(state[:, 3]))
    clip_v = (r[:, L.P_RANGE_FLAGS].astype(int) & L.RANGE_SPEED) != 0
    vlo, vhi = r[:, L.P_SPEED_LO], r[:, L.P_SPEED_HI]
    dt, n, rem = _substeps(rows, tid, interval)
    t = r[:, L.P_LR] / r[:, L.P_WB] * np.tan(delta)                       # tan(beta) (:219)
    kk = np.tan(delta) / r[:, L.P_WB] / np.sqrt(1 + t * t)                # d(phi)/dt = v kk (:225)
    ah, kh = accel * dt, kk * dt                                          # (:247)
    pinned = clip_v & (((v == vhi) & (ah >= 0)) | ((v == vlo) & (ah <= 0)))          # (:257)
    ah_l = np.where(pinned, 0.0, ah)
    v_end = v + n * ah_l
    eps0, eps_end, dlt = v * kh, v_end * kh, ah_l * kh                    # (:260)
    in_range = (v >= vlo) & (v <= vhi)
    lane_linear = (~clip_v | (in_range & (v_end >= vlo) & (v_end <= vhi))) & (np.abs(eps0) <= K_EPS_MAX) & (np.abs(eps_end) <= K_EPS_MAX)   # (:261)
    m, M = (n - 1) / 2.0, n / 2.0                                         # kin_geo (t2d_api.hip kinematics_resum_table)
    ra = (dlt * (m - 0.5) + eps0) * M                                     # (:272)
    rb = dlt * M * M / 2                                                  # (:273)
    lane_resum = lane_linear & (kin_n > 0) & (n == kin_n) & (np.abs(ra) <= K_RESUM_AMAX) & (np.abs(rb) <= K_RESUM_BMAX)   # (:274)
    amax = np.maximum(np.abs(eps0), np.abs(eps_end))                      # (:292)
    inside = clip_v & ~pinned & in_range                                  # (:327)
    v_unc = v + n * ah
    crossing = inside & ((v_unc > vhi) | (v_unc < vlo))                   # (:329)
    vB = np.where(v_unc > vhi, vhi, vlo)                                  # (:330)
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = np.ceil((vB - v) / ah)                                       # (:333-334)
    kstar = np.where(crossing, np.clip(np.nan_to_num(tc, nan=1.0, posinf=1e6, neginf=1.0), 1, 1000000), INT_MAX).astype(np.int64)   # (:335)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_cross = np.where(crossing, (vB - v) / ah, np.nan)
    epsB = vB * kh
    lane_piecewise = lane_linear | (crossing & (np.abs(eps0) <= K_EPS_MAX) & (np.abs(epsB) <= K_EPS_MAX))   # (:338)
    return dict(pinned=pinned, lane_linear=lane_linear, lane_resum=lane_resum, crossing=crossing, kstar=kstar, t_cross=t_cross,
                lane_piecewise=lane_piecewise, amax=amax, eps0=eps0, eps_end=eps_end, epsB=epsB, vB=vB, ra=ra, rb=rb, n=n, rem=rem,
                in_range=in_range | ~clip_v, clip_v=clip_v, v_end=v_end)


def kin_wave_path(k, sl):
    """the path of the wave whose lanes are k[...][sl] -- the kernel's if / else chain (:278, :290, :293, :339)"""
    if k["lane_resum"][sl].all():
        return "resummed"
    if k["lane_linear"][sl].all():
        return "linear/tiny" if (k["amax"][sl] <= K_EPS_TINY).all() else "linear/small"
    if k["lane_piecewise"][sl].all():
        return "piecewise"
    return "plain"


# --------------------------------------------------------------------------- dynamics
def dyn_replay(rows, tid, state, action, interval):
    """The recurrence of SingleTrackDynamics._step (single_track_dynamics.py:140-229; step_dynamics :439-467) in fp64, every
    lane at once: final heading (unwrapped) and speed, |eps| = |(d_phi + d_beta) dt| of every sub-step (NaN beyond the
    lane's own count), the speed before every sub-step, and the `always_fast` predicate (:478-480)."""
    rows = np.asarray(rows, np.float64)
    tid = np.asarray(tid).astype(int)
    r = rows[tid]
    accel, delta = _clipped_action(rows, tid, action)
    phi = np.float64(np.float32(state[:, 2]))
    v = np.float64(np.float32(state[:, 3]))
    v0 = v.copy()
    clip_v = (r[:, L.P_RANGE_FLAGS].astype(int) & L.RANGE_SPEED) != 0
    vlo = np.where(clip_v, r[:, L.P_SPEED_LO], -np.inf)
    vhi = np.where(clip_v, r[:, L.P_SPEED_HI], np.inf)
    lf, lr, wb = r[:, L.P_LF], r[:, L.P_LR], r[:, L.P_WB]
    mass, hcg, mu, Iz, cf, cr = (r[:, c] for c in (L.P_MASS, L.P_MASS_HEIGHT, L.P_MU, L.P_IZ, L.P_CF, L.P_CR))
    dt, n, _ = _substeps(rows, tid, interval)
    g = 9.81
    ff, fr = (g * lr - accel * hcg) / wb, (g * lf + accel * hcg) / wb
    tand = np.tan(delta)
    d_phi, beta = v / wb * tand, np.arctan(lr / lf * tand)
    nmax = int(n.max())
    eps = np.full((len(tid), nmax), np.nan)
    vs_hist = np.full((len(tid), nmax), np.nan)
    for k in range(nmax):
        on = k < n
        vs_hist[on, k] = v[on]
        av = np.abs(v)
        vs = np.where(av > 1e-6, v, np.where(v >= 0, 1e-6, -1e-6))
        dd_phi = mu * mass / Iz * (lf * cf * ff * delta + (lr * cr * fr - lf * cf * ff) * beta - (lf * lf * cf * ff + lr * lr * cr * fr) * d_phi / vs)
        d_beta_hi = mu / vs * (cf * ff * delta - (cr * fr + cf * ff) * beta + (lr * cr * fr - lf * cf * ff) * d_phi / vs) - d_phi
        d_beta_lo = lr / (1 + tand * lr / wb) ** 2 / wb / np.cos(delta) ** 2 * delta
        hi = av >= 0.1
        d_beta = np.where(hi, d_beta_hi, d_beta_lo)
        d_phi_n = np.where(hi, d_phi + dd_phi * dt, d_phi + v * np.cos(beta) / wb * tand * dt)
        v_n = np.clip(v + accel * dt, vlo, vhi)
        e = (d_phi_n + d_beta) * dt
        eps[on, k] = np.abs(e[on])
        d_phi = np.where(on, d_phi_n, d_phi)
        phi = np.where(on, phi + d_phi_n * dt, phi)
        beta = np.where(on, beta + d_beta * dt, beta)
        v = np.where(on, v_n, v)
    v_fin = np.clip(v0 + n * (accel * dt), vlo, vhi)
    always_fast = ((v0 >= V_FAST) & (v_fin >= V_FAST)) | ((v0 <= -V_FAST) & (v_fin <= -V_FAST))
    return dict(phi=phi, v=v, eps=eps, v_sub=vs_hist, n=n, always_fast=always_fast, v_fin=v_fin)


def dyn_wave_path(d, sl):
    """The path of the wave whose lanes are d[...][sl].  Lanes run their own trip counts (delta_t is a type parameter), so a
    wave-uniform test sees the lanes still in the loop: in the general loop (:522) sub-step j of every lane with n > j;
    in the always_fast loop (:509-513) the paired sub-steps j < 2 (n // 2) together, then the odd tails of the lanes with an
    odd count together, each at its own last sub-step."""
    eps, n = d["eps"][sl], d["n"][sl]
    af = bool(d["always_fast"][sl].all())
    groups = []
    for j in range(eps.shape[1]):
        on = (2 * (n // 2) > j) if af else (n > j)
        if on.any():
            groups.append(eps[on, j])
    if af and (n % 2 == 1).any():
        odd = n % 2 == 1
        groups.append(eps[odd, n[odd] - 1])
    worst = np.array([g.max() for g in groups])
    rot = "reseed" if (worst > K_EPS_MAX).any() else ("small" if (worst > K_EPS_TINY).any() else "tiny")
    return ("always_fast/" if af else "general/") + rot


def wave_paths(model, rows, tid, state, action, interval, group=64, kin_n=0):
    """The path every group of `group` consecutive participants takes: a list of names of KIN_PATHS / DYN_PATHS.  kin_n: the
    sub-step count the pool's resummation table was built for (0: none -- variant fast_iterated, and fast on pools that do
    not fill the GPU; fast_resummed: interval // delta_t of the table's first kinematic row)."""
    n = len(tid)
    if model == "kin":
        k = kin_lanes(rows, tid, state, action, interval, kin_n)
        return [kin_wave_path(k, slice(i, min(i + group, n))) for i in range(0, n, group)]
    d = dyn_replay(rows, tid, state, action, interval)
    return [dyn_wave_path(d, slice(i, min(i + group, n))) for i in range(0, n, group)]


def by_path_order(model, rows, tid, state, action, interval):
    """A permutation that sorts cases into waves of one path class each: lanes by the slowest path they would force on
    their wave, then by their largest sub-step angle."""
    if model == "kin":
        k = kin_lanes(rows, tid, state, action, interval)
        cls = np.where(k["lane_linear"], 0, np.where(k["lane_piecewise"], 1, 2))
        key2 = np.where(cls == 1, k["kstar"].astype(np.float64), k["amax"])
    else:
        d = dyn_replay(rows, tid, state, action, interval)
        cls = np.where(d["always_fast"], 0, 1)
        with np.errstate(invalid="ignore"):
            key2 = np.nanmax(d["eps"], axis=1)
        key2 = np.nan_to_num(key2, nan=np.inf, posinf=np.inf)
    return np.lexsort((key2, cls))


# --------------------------------------------------------------------------- scenes
@dataclass
class Scene:
    """One pool's worth of cases, 64 per wave: labels[w] is what wave w was built to be, want[w] the path it must take (None:
    an edge wave, whose path may fall either way -- only the error bound is asserted)."""
    model: str
    rows: np.ndarray
    tid: np.ndarray
    state: np.ndarray
    action: np.ndarray
    interval: int
    labels: list = field(default_factory=list)
    want: list = field(default_factory=list)

    @property
    def n(self):
        return len(self.tid)


KIN_TIMINGS = [(100, 5), (50, 3), (9, 5), (100, 7), (35, 5)]
KIN_RANGES = [(-0.5, 0.5), (0.0, 1.2), (0.5, 7.0), (-7.0, 7.0), (0.0, 20.0), (2.0, 30.0)]   # test_fast_kinematics_speed_clipping_paths
T_TINY = 6      # the row of a toy vehicle (wheel base 0.1 m, speed unbounded): sub-step angles beyond kEpsMax at walking speed
T_EXACT = 7     # rows 7..14: bounds placed an exact number of updates away from a start speed (the near-integer wave)
T_OTHER = 15    # the parking row with delta_t + 1: linear lanes the resummation table was not built for


def _parking_row():
    import helpers as H
    k = [q for q in H.load_json("physics_kats.json") if q["ctor"] == "parking" and q["model"] == "kinematics"][0]
    return np.array(k["row"], np.float64)


def _kin_rows(delta_t, n_steps):
    rows = []
    for lo, hi in KIN_RANGES:
        r = _parking_row()
        r[L.P_SPEED_LO], r[L.P_SPEED_HI] = lo, hi
        r[L.P_RANGE_FLAGS] = int(r[L.P_RANGE_FLAGS]) | L.RANGE_SPEED
        r[L.P_ACCEL_LO], r[L.P_ACCEL_HI] = -6.0, 6.0
        r[L.P_DELTA_T_MS] = delta_t
        rows.append(r)
    r = rows[0].copy()
    r[L.P_LF], r[L.P_LR], r[L.P_WB] = 0.04, 0.06, 0.1
    r[L.P_RANGE_FLAGS] = int(r[L.P_RANGE_FLAGS]) & ~L.RANGE_SPEED
    rows.append(r)
    # near-integer rows: the bound is fl(v0 + j ah) in fp64, so that (vB - v0) / ah is j to ~1e-14
    exact = []
    dt = delta_t / 1000.0
    js = [1, 2, n_steps // 2 + 1, n_steps]
    for up in (True, False):
        for j in js:
            j = min(max(j, 1), n_steps)
            v0 = float(np.float32(0.8125 if up else 2.71875))
            acc = float(np.float32(1.7 if up else -2.3))
            r = rows[2].copy()                                   # range (0.5, 7)
            r[L.P_SPEED_HI if up else L.P_SPEED_LO] = v0 + j * (acc * dt)
            rows.append(r)
            exact.append((v0, acc, j))
    r = rows[3].copy()
    other = delta_t + 1 if n_steps * (delta_t + 1) > 0 and (n_steps * delta_t + delta_t - 1) // (delta_t + 1) != n_steps else delta_t - 2
    r[L.P_DELTA_T_MS] = other
    rows.append(r)
    return np.array(rows), exact


def kin_scene(interval, delta_t):
    """The kinematic scene of one (interval, delta_t): see the module docstring and the issue's list -- linear waves (tiny and
    small), pinned waves, one crossing wave per kstar and bound, a mixed and a near-integer wave, spoiler waves."""
    rng = np.random.default_rng(1000 * interval + delta_t)
    n_steps = interval // delta_t
    dt = delta_t / 1000.0
    rows, exact = _kin_rows(delta_t, n_steps)
    W = 64
    tids, vs, accs, steers, labels, want = [], [], [], [], [], []
    kh_gentle = np.tan(0.3) / 2.637 * dt         # an upper bound of |kh| of the parking row at |steer| <= 0.3 (cos(beta) <= 1)
    gentle = lambda: rng.uniform(-0.3, 0.3, W)

    def add(label, path, tid, v, acc, steer=None):
        tids.append(np.broadcast_to(np.asarray(tid), (W,)).astype(np.uint8))
        vs.append(np.float32(np.broadcast_to(v, (W,))))
        accs.append(np.float32(np.broadcast_to(acc, (W,))))
        steers.append(np.float32(rng.uniform(-0.6, 0.6, W) if steer is None else np.broadcast_to(steer, (W,))))
        labels.append(label)
        want.append(path)

    def lo_hi(tid):
        return rows[tid, L.P_SPEED_LO], rows[tid, L.P_SPEED_HI]

    def linear_inside(tid):
        """speed and acceleration with v and v + n ah well inside the range (never on a bound)"""
        lo, hi = lo_hi(tid)
        span = hi - lo
        acc = rng.uniform(-6, 6, W) * rng.choice([0.0, 0.05, 1.0], W)
        dv = n_steps * acc * dt + acc * (interval % delta_t) / 1000.0
        room = span - np.abs(dv)
        acc = np.where(room < 0.4 * span, 0.0, acc)
        dv = np.where(room < 0.4 * span, 0.0, dv)
        u = rng.uniform(0.1, 0.9, W)
        v_lo = lo - np.minimum(dv, 0) + 0.05 * span
        v_hi = hi - np.maximum(dv, 0) - 0.05 * span
        return v_lo + u * (v_hi - v_lo), acc

    def crossing(tid, up, kstar):
        """lanes that reach the bound in update kstar: t = (vB - v) / ah in [kstar - 0.8, kstar - 0.2]"""
        lo, hi = lo_hi(tid)
        t = kstar - rng.uniform(0.2, 0.8, np.shape(tid))
        amag = rng.uniform(0.5, 6.0, np.shape(tid))
        amag = np.float64(np.float32(np.minimum(amag, 0.9 * (hi - lo) / (t * dt))))
        acc = amag if up else -amag
        vB = hi if up else lo
        return vB - acc * dt * t, acc

    # ---- linear waves
    for rep in range(2):
        tid = rng.integers(0, 4, W)                                      # |v| <= 7, |steer| <= 0.3: amax <= 7 kh < kEpsTiny
        v, acc = linear_inside(tid)
        assert 7.0 * kh_gentle <= EPS_TINY_IN
        add("linear/tiny", "linear/tiny", tid, v, acc, gentle())
    for rep in range(2):
        # range (2, 30) at 20..29 m/s and full lock: eps0 = v kh in (kEpsTiny, kEpsMax] for at least the lanes steering hard
        tid = np.full(W, 5)
        acc = rng.uniform(-2, 2, W)
        v = rng.uniform(21.0, 28.0, W)
        steer = rng.choice([-1, 1], W) * rng.uniform(0.45, 0.6, W)
        small_ok = 21.0 * (np.tan(0.45) / 2.637 * dt) * 0.93 >= 1.2 * K_EPS_TINY     # (cos(beta) >= 0.93 at full lock)
        if small_ok:
            add("linear/small", "linear/small", tid, v, acc, steer)
        else:   # short sub-steps (delta_t 3): the parking row stays tiny below 30 m/s -- the toy vehicle turns fast enough
            v = rng.uniform(1.5, 2.5, W) * rng.choice([-1, 1], W)           # eps0 = v kh in 0.016 .. 0.04
            add("linear/small", "linear/small", np.full(W, T_TINY), v, rng.uniform(-1, 1, W), rng.choice([-1, 1], W) * rng.uniform(0.35, 0.5, W))
    # ---- pinned on a bound, the acceleration pushing outwards (or zero, of either sign)
    for rep in range(3):
        tid = rng.choice([0, 2, 3], W)                                   # (bounds that fp32 holds exactly: not 1.2)
        lo, hi = lo_hi(tid)
        up = rng.random(W) < 0.5
        mag = rng.uniform(0.1, 6.0, W) * rng.choice([0.0, 1.0, 1.0], W)
        acc = np.where(up, mag, -mag)                                    # (0.0 and -0.0 both occur)
        v = np.where(up, hi, lo)
        steer = gentle()
        path = "linear/tiny"
        if rep == 1:                                                     # v == vlo == 0 with ah < 0, and ah == +-0
            tid = rng.choice([1, 4], W)
            v = np.zeros(W)
            acc = np.where(np.arange(W) % 4 == 0, 0.0, np.where(np.arange(W) % 4 == 1, -0.0, -rng.uniform(0.1, 6.0, W)))
        if rep == 2:                                                     # pinned on 20 and 30 m/s at full lock: rotate_small
            if delta_t < 5:
                continue
            tid = rng.choice([4, 5], W)
            v, acc = rows[tid, L.P_SPEED_HI], rng.uniform(0.0, 6.0, W)
            steer = rng.choice([-1, 1], W) * rng.uniform(0.45, 0.6, W)
            path = "linear/small"
        add("pinned", path, tid, v, acc, steer)
    # ---- crossing waves: one per kstar and bound
    for up in (True, False):
        for ks in range(1, n_steps + 1):
            tid = rng.integers(0, 6, W)
            v, acc = crossing(tid, up, ks)
            add(f"cross/{'hi' if up else 'lo'}/kstar={ks}", "piecewise", tid, v, acc)
        # lanes whose kstar differ, and lanes that do not cross at all
        tid = rng.integers(0, 6, W)
        ks = rng.integers(1, n_steps + 1, W)
        v, acc = crossing(tid, up, ks)
        vl, al = linear_inside(tid)
        lin = np.arange(W) % 3 == 0
        add(f"cross/{'hi' if up else 'lo'}/mixed", "piecewise", tid, np.where(lin, vl, v), np.where(lin, al, acc))
    # ---- (vB - v) / ah within 1e-12 of an integer: the crossing sub-step may fall either way
    which = np.arange(W) % len(exact)
    add("cross/near-integer", None, T_EXACT + which, [exact[i][0] for i in which], [exact[i][1] for i in which])
    # ---- spoiler waves: 63 lanes of a class and one lane that forces the next slower path
    tid = rng.integers(0, 4, W)
    v, acc = linear_inside(tid)
    tid[17], v[17], acc[17] = 0, 0.5 + 0.2, 1.0                           # outside its range: plain loop
    add("spoiler/linear+outside", "plain", tid, v, acc)
    tid = rng.integers(0, 4, W)
    v, acc = linear_inside(tid)
    steer = rng.uniform(-0.6, 0.6, W)
    tid[40], v[40], acc[40], steer[40] = T_TINY, 0.15 / (5.0 * dt), 0.0, 0.5   # eps0 = v kh ~ 0.15 > kEpsMax: plain loop
    add("spoiler/linear+eps0", "plain", tid, v, acc, steer)
    tid = rng.integers(0, 4, W)
    v, acc = linear_inside(tid)
    c_v, c_a = crossing(tid, True, np.full(W, max(1, n_steps // 2)))
    v[5], acc[5] = c_v[5], c_a[5]                                        # one crossing lane: piecewise
    add("spoiler/linear+crossing", "piecewise", tid, v, acc)
    tid = rng.integers(0, 6, W)
    v, acc = crossing(tid, False, rng.integers(1, n_steps + 1, W))
    tid[63], v[63], acc[63] = 2, 0.5 - 0.25, -1.0                         # outside its range: plain loop
    add("spoiler/crossing+outside", "plain", tid, v, acc)
    tid = rng.integers(0, 4, W)
    v, acc = linear_inside(tid)
    steer = gentle()
    tid[9], v[9], acc[9] = T_OTHER, 0.1, 0.5                              # linear, of another sub-step count: the series' spoiler
    add("spoiler/resum+n", "linear/tiny", tid, v, acc, steer)

    n = W * len(labels)
    state = np.stack([rng.uniform(-0.01, 0.01, n), rng.uniform(-0.01, 0.01, n), rng.uniform(0, 0.2, n), np.concatenate(vs)], 1).astype(np.float32)
    action = np.stack([np.concatenate(accs), np.concatenate(steers)], 1).astype(np.float32)
    return Scene("kin", rows, np.concatenate(tids), state, action, interval, labels, want)


DYN_INTERVALS = [100, 50, 35, 9]


def _dyn_rows():
    """rows 0 (delta_t 5) and 2 (delta_t 3) of dyn_random.npz, each with its speed range and with none"""
    import helpers as H
    base = H.load_npz("dyn_random.npz")["rows"]
    rows = [base[0].copy(), base[2].copy(), base[0].copy(), base[2].copy()]
    for r in rows[2:]:
        r[L.P_RANGE_FLAGS] = int(r[L.P_RANGE_FLAGS]) & ~L.RANGE_SPEED
    return np.array(rows)


def dyn_scene(interval):
    """The dynamics scene of one interval.  Lanes alternate between delta_t 5 and 3 and between the bounded and the unbounded
    speed range, so the trip counts differ inside every wave.  Candidates are drawn at random, replayed, and kept where they
    fall at least 20 % clear of the thresholds of the class their wave needs."""
    rng = np.random.default_rng(77 + interval)
    rows = _dyn_rows()
    W = 64
    N = 60000

    def draw(vlo, vhi, steer, acc=(-4.0, 3.0), sign=True, tid=None):
        t = rng.integers(0, 4, N) if tid is None else np.full(N, tid)
        v = rng.uniform(vlo, vhi, N) * (rng.choice([-1, 1], N) if sign else 1)
        st = np.stack([np.zeros(N), np.zeros(N), np.zeros(N), v], 1).astype(np.float32)
        ac = np.stack([rng.uniform(*acc, N), rng.uniform(-steer, steer, N)], 1).astype(np.float32)
        return t, st, ac, dyn_replay(rows, t, st, ac, interval)

    parts, labels, want = [], [], []

    def add(label, path, tid, st, ac, pick):
        assert len(pick) == W, (label, len(pick))
        parts.append((tid[pick], st[pick], ac[pick]))
        labels.append(label)
        want.append(path)

    def fast_ok(d, v0):
        return d["always_fast"] & (np.abs(v0) >= V_HIGH) & (np.abs(d["v_fin"]) >= V_HIGH)

    # eps = (d_phi + d_beta) dt is the lateral-force term mu / v (...) dt: large at LOW speed and hard steering, largest in the
    # first sub-steps (the slip angle's transient).  One broad draw, speeds log-uniform, classified by the largest angle.
    def draw_log(vlo, vhi, steer, acc=(-4.0, 3.0)):
        t = rng.integers(0, 4, N)
        v = np.exp(rng.uniform(np.log(vlo), np.log(vhi), N))
        st = np.stack([np.zeros(N), np.zeros(N), np.zeros(N), v], 1).astype(np.float32)
        ac = np.stack([rng.uniform(*acc, N), rng.uniform(-steer, steer, N)], 1).astype(np.float32)
        return t, st, ac, dyn_replay(rows, t, st, ac, interval)

    t, st, ac, d = draw_log(V_SCENE_MIN, 40.0, 0.5)
    mx = np.nanmax(d["eps"], 1)
    good = fast_ok(d, st[:, 3])
    tiny = np.nonzero(good & (mx <= EPS_TINY_IN))[0]
    ok = np.nonzero(good & (mx >= EPS_SMALL_LO) & (mx <= EPS_SMALL_HI))[0]
    big = np.nonzero(good & (mx >= EPS_RESEED) & (mx <= 0.6))[0]
    # ---- always_fast, every sub-step tiny (one wave of them reversing at 5 .. 12 m/s)
    for rep in range(2):
        add("always_fast/tiny", "always_fast/tiny", t, st, ac, tiny[rep * W:(rep + 1) * W])
    tn, stn, acn, dn = draw(5.0, 12.0, 0.1)
    okn = np.nonzero(fast_ok(dn, stn[:, 3]) & (np.nanmax(dn["eps"], 1) <= EPS_TINY_IN))[0]
    add("always_fast/tiny", "always_fast/tiny", tn, stn, acn, okn[:W])
    # ---- always_fast, some sub-steps small: every lane's largest angle in the small band, or half the lanes'
    add("always_fast/small", "always_fast/small", t, st, ac, ok[:W])
    add("always_fast/small", "always_fast/small", t, st, ac, ok[W:2 * W])
    add("always_fast/small-half", "always_fast/small", t, st, ac, np.concatenate([ok[2 * W:2 * W + 32], tiny[2 * W:2 * W + 32]]))
    # ---- always_fast, some lane beyond kEpsMax
    for rep in range(2):
        pick = np.concatenate([ok[(3 + rep) * W:(3 + rep) * W + W - 8], big[8 * rep:8 * rep + 8]])
        add("always_fast/reseed", "always_fast/reseed", t, st, ac, rng.permutation(pick))
    # ---- the general loop: every lane below 0.1 m/s for the whole step (tiny), and half such lanes, half turning fast (small)
    tl, stl, acl, dl = draw(0.0, 0.06, 0.5, acc=(-0.15, 0.15))
    low = np.nonzero((np.nanmax(np.abs(dl["v_sub"]), 1) <= V_LOW) & (np.abs(dl["v_fin"]) <= V_LOW) & (np.nanmax(dl["eps"], 1) <= EPS_TINY_IN))[0]
    for rep in range(2):
        add("general/tiny", "general/tiny", tl, stl, acl, low[rep * W:(rep + 1) * W])
    for rep in range(2):
        pick_s, pick_l = ok[(5 + rep) * W:(5 + rep) * W + 32], low[(2 + rep) * 32 + 64:(2 + rep) * 32 + 96]
        tid = np.concatenate([t[pick_s], tl[pick_l]])
        s_ = np.concatenate([st[pick_s], stl[pick_l]])
        a_ = np.concatenate([ac[pick_s], acl[pick_l]])
        p = rng.permutation(W)
        parts.append((tid[p], s_[p], a_[p]))
        labels.append("general/small")
        want.append("general/small")
    # ---- edge waves (the path may fall either way; the bound holds on both)
    f = lambda a: np.float32(a)
    sgn = np.where(np.arange(W) % 2 == 0, 1.0, -1.0)
    # Rows 4..9: the same vehicle on SOFT tyres (cf = cr = 1 instead of 20.89).  With the stock stiffness the reference's explicit
    # Euler multiplies a yaw-rate error by 1 - 1.34 / v per 5 ms sub-step -- by -12 at 0.1 m/s, 1e21 over a step: no bound can be
    # asserted there (helpers.SENS_CHAOTIC).  The speed thresholds under test do not depend on the tyres.
    soft = np.concatenate([rows, rows[:2]])
    soft[:, L.P_CF] = soft[:, L.P_CR] = 1.0
    soft[4, L.P_SPEED_LO], soft[5, L.P_SPEED_LO] = 0.1000002, 0.12
    rows_all = np.concatenate([rows, soft])
    tid_e = 4 + (np.arange(W) // 2 % 4).astype(int)
    dts = rows_all[tid_e, L.P_DELTA_T_MS] / 1000.0
    ns = interval // rows_all[tid_e, L.P_DELTA_T_MS].astype(int)
    thr = np.float32(V_FAST)                                                    # the first fp32 at or above the threshold ...
    thr = np.float64(thr if float(thr) >= V_FAST else np.nextafter(thr, np.float32(1)))
    ulp = np.float64(np.spacing(np.float32(V_FAST)))
    near = thr + ulp * rng.integers(-3, 4, W)                                   # ... and up to three fp32 either side of it
    steer_e = rng.uniform(-0.02, 0.02, W)

    def edge(label, v0, acc, tid=tid_e, steer=steer_e):
        z = np.zeros(W)
        parts.append((np.asarray(tid), np.stack([z, z, z, v0], 1).astype(np.float32), np.stack([acc, steer], 1).astype(np.float32)))
        labels.append(label)
        want.append(None)

    # v0 on either side of +-0.1000001, the speed rising away from it
    above = thr + ulp * rng.integers(0, 4, W)                                   # on the threshold and up to three fp32 above it
    edge("edge/v0", sgn * near, sgn * rng.uniform(0.5, 2.0, W))
    edge("edge/v0-above", sgn * above, sgn * rng.uniform(0.5, 2.0, W))
    # v_fin on either side of +-0.1000001: the step brakes from 0.1 + n |ah| + (a few 1e-7)
    acc_f = f(rng.uniform(0.2, 1.0, W))
    edge("edge/v_fin", sgn * (near + ns * (np.float64(acc_f) * dts)), -sgn * acc_f)
    edge("edge/v_fin-above", sgn * (above + ns * (np.float64(acc_f) * dts)), -sgn * acc_f)
    # v_fin clamped onto a bound just above 0.1: rows 8, 9, whose lower bound is 0.1000002 / 0.12, braking into it
    clamp_tid = 8 + (np.arange(W) % 2)
    edge("edge/v_fin-clamped", rng.uniform(0.13, 0.2, W), -rng.uniform(2.0, 4.0, W), tid=clamp_tid)
    # braking through 0.1 inside the step: the branch switches mid-step
    k_sw = np.maximum(1, (ns * rng.uniform(0.3, 0.7, W)).astype(int))
    acc_b = f(-rng.uniform(0.3, 0.9, W))
    v_b = 0.1 - (k_sw - 0.5) * (np.float64(acc_b) * dts)
    edge("edge/brake-through-0.1", v_b, acc_b)
    # one lane below 0.1 m/s in an otherwise always_fast wave: the general loop for all 64
    pick = ok[7 * W:8 * W].copy()
    tid = t[pick].copy(); s_ = st[pick].copy(); a_ = ac[pick].copy()
    tid[31], s_[31], a_[31] = 0, [0, 0, 0, 0.05], [0.0, 0.1]
    parts.append((tid, s_, a_)); labels.append("spoiler/always_fast+slow"); want.append("general/small")
    pick = np.nonzero(fast_ok(d, st[:, 3]) & (mx <= EPS_TINY_IN))[0]
    if len(pick) >= W:
        tid = t[pick[:W]].copy(); s_ = st[pick[:W]].copy(); a_ = ac[pick[:W]].copy()
        tid[12], s_[12], a_[12] = 1, [0, 0, 0, -0.04], [0.0, -0.2]
        parts.append((tid, s_, a_)); labels.append("spoiler/always_fast+slow"); want.append("general/tiny")

    tid = np.concatenate([p[0] for p in parts]).astype(np.uint8)
    state = np.concatenate([p[1] for p in parts]).astype(np.float32)
    action = np.concatenate([p[2] for p in parts]).astype(np.float32)
    n = len(tid)
    state[:, 0], state[:, 1], state[:, 2] = rng.uniform(-0.01, 0.01, n), rng.uniform(-0.01, 0.01, n), rng.uniform(0, 0.2, n)
    return Scene("dyn", rows_all, tid, state, action, interval, labels, want)


# --------------------------------------------------------------------------- inputs of tests that predate the path model
def clipping_cases(interval, delta_t):
    """The 6000 random cases of test_gpu_physics.py::test_fast_kinematics_speed_clipping_paths, in the order drawn: on a
    bound, inside, about to cross, outside the range -- mixed lane by lane."""
    import helpers as H
    rng = np.random.default_rng(42 + interval)
    k = [q for q in H.load_json("physics_kats.json") if q["ctor"] == "parking" and q["model"] == "kinematics"][0]
    rows = []
    for lo, hi in KIN_RANGES:
        r = np.array(k["row"], np.float64)
        r[L.P_SPEED_LO], r[L.P_SPEED_HI] = lo, hi
        r[L.P_RANGE_FLAGS] = int(r[L.P_RANGE_FLAGS]) | 2
        r[L.P_ACCEL_LO], r[L.P_ACCEL_HI] = -6.0, 6.0
        r[L.P_DELTA_T_MS] = delta_t
        rows.append(r)
    rows = np.array(rows)
    n = 6000
    tid = rng.integers(0, len(KIN_RANGES), n).astype(np.uint8)
    lo = rows[tid, L.P_SPEED_LO]; hi = rows[tid, L.P_SPEED_HI]
    mode = rng.integers(0, 5, n)
    u = rng.random(n)
    v = np.where(mode == 0, lo, np.where(mode == 1, hi, lo + u * (hi - lo)))          # on a bound / inside
    v = np.where(mode == 3, np.where(u < 0.5, hi - 0.02 * u, lo + 0.02 * u), v)       # about to cross
    v = np.where(mode == 4, np.where(u < 0.5, hi + 0.3 * u, lo - 0.3 * u), v)         # outside (plain loop)
    st = np.stack([rng.uniform(-200, 200, n), rng.uniform(-200, 200, n), rng.uniform(-7, 7, n), v], 1).astype(np.float32)
    act = np.stack([rng.uniform(-6, 6, n), rng.uniform(-0.6, 0.6, n)], 1).astype(np.float32)
    act[rng.random(n) < 0.1, 0] = 0.0
    return rows, tid, st, act
