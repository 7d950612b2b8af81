"""Every scene of tests/reuse_scenes.py can fail: the reference applied to a configuration gives an answer that differs from the
same reference applied to the configuration, or the stale state, before it.  The floors are conditions on the scenes, met by the
references alone (the C oracle, pursuit_ref, route_ref); tests/test_gpu_reuse.py then holds the device to the same references.
No GPU is touched here."""
import numpy as np
import pytest

import reuse_scenes as RS


def _controlled(C):
    return (C["pursuit"][1] != 255) & (C["active"] != 0)


def _accel_last_matters(oracle, C_hist, C_new):
    """share of C_new's pursuit-controlled participants whose pursuit_ref action differs between accel_last = 0 and accel_last =
    what the oracle chain applied in the last step of C_hist's episode (what T2D_F_APPLIED0 still holds)"""
    _, applied, _ = RS.episode(oracle, C_hist)
    st = RS.state_of(C_new)
    n = len(st)
    zero = RS.pursuit_want(oracle, C_new, st, np.zeros(n, np.float32))
    stale = RS.pursuit_want(oracle, C_new, st, applied[-1])
    on = _controlled(C_new)
    assert on.sum() >= (3 if C_new["A"] > 1 else 1) * C_new["n_env"] // 2 and np.isfinite(zero["action"][on]).all()
    return float((zero["action"][on, 1] != stale["action"][on, 1]).mean()), zero


def test_second_reset_and_masked_reset_depend_on_accel_last(oracle):
    C1, C2 = RS.traffic(0), RS.second_reset()
    share, zero = _accel_last_matters(oracle, C1, C2)
    assert share >= 0.5, share
    on = _controlled(C2)
    assert (zero["leader"][on] >= 0).any() and (zero["leader"][on] < 0).any()        # ACC behind a leader, and cruise
    # the second reset is another episode: poses, the active pattern and the type ids all change
    assert (C1["x"] != C2["x"]).all() and (C1["active"] != C2["active"]).any() and (C1["type_id"] != C2["type_id"]).any()
    mask, Cm = RS.masked(C1, C2)
    assert mask.tolist() == [1, 0, 0, 1, 0]
    share, _ = _accel_last_matters(oracle, C1, Cm)
    sel = np.repeat(mask, C1["A"]).astype(bool)
    assert (Cm["x"][sel] == C2["x"][sel]).all() and (Cm["x"][~sel] == C1["x"][~sel]).all()
    st = RS.state_of(Cm)
    _, applied, _ = RS.episode(oracle, C1)
    zero = RS.pursuit_want(oracle, Cm, st, np.zeros(len(st), np.float32))
    stale = RS.pursuit_want(oracle, Cm, st, applied[-1])
    on = _controlled(Cm) & sel
    assert (zero["action"][on, 1] != stale["action"][on, 1]).mean() >= 0.5


@pytest.mark.parametrize("form", ["step", "unfused", "ego", "step_split"])
def test_restored_episodes_depend_on_accel_last(oracle, form):
    C = RS.traffic(3, max_step=4, stuck_env=1, **RS.RESTORE_FORMS[form])
    share, _ = _accel_last_matters(oracle, C, C)        # (the new episode starts from the snapshot: the same poses)
    assert share >= 0.5, share
    # env 1's ego stands in its static square from the first step on; nobody else has a verdict in the first step
    states, _, _ = RS.episode(oracle, C, 1)
    flags, env_flags = RS.collide_want(oracle, C, states[1][:, 0], states[1][:, 1], states[1][:, 2])
    assert flags[C["A"]] & 2 and env_flags.tolist() == [0, 2, 0, 0, 0]


@pytest.mark.parametrize("kind", RS.GEO_KINDS)
@pytest.mark.parametrize("shape", RS.GEO_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry_rungs_change_the_flags(oracle, shape, kind):
    ladder = RS.geometry_ladder(shape, kind)
    assert [s for s, _ in ladder] == ["small", "mid", "big", "small", "none"]
    prev = None
    for stage, C in ladder:
        flags, _ = RS.collide_want(oracle, C)
        if prev is not None:
            assert (flags != prev).mean() >= 0.10, (stage, float((flags != prev).mean()))
        prev = flags
        if stage == "none":
            assert C["static"] is None and C["lanes"] is None and not flags.any()
            continue
        b = RS._budget(C, C["static"], C["lanes"])
        assert b["tier"] == ("hbm_grid" if stage == "big" else "lds_record"), (stage, b)
        if stage == "mid":
            assert 0.5 * b["dwords_budget"] < b["dwords_needed"] <= b["dwords_budget"]
        for csr in (C["static"], C["lanes"]):
            if csr is not None:
                per_env = np.diff(csr[0])
                assert per_env[RS.NO_POLYGON_ENV] == 0 and len(set(per_env.tolist())) > 1       # the maps differ, one is empty
        if kind == "full":
            assert np.diff(C["static"][0])[RS.NO_LANE_ENV] > 0 and np.diff(C["lanes"][0])[RS.NO_LANE_ENV] == 0
        if stage == "big":
            assert C["x"][1] > RS.FAR_AWAY and C["active"][1]
            if kind != "static":
                assert flags[1] & 8                                                             # off-lane by the oracle
            if kind != "lanes":
                assert RS.segment_pairs(oracle, C) > RS.MAP_QUEUE                               # the first 64-participant segment
                assert 64 // C["A"] >= 8 or C["n_env"] * C["A"] < 64                            # ... spans several envs


def test_table_ladders(oracle):
    from tactics2d_amd import layout as L
    lad = RS.table_ladders()
    boxes, disc, _ = [C for _, C, _ in lad["circle_row"]]
    assert (boxes["rows"][:, L.P_SHAPE] == L.SHAPE_OBB).all() and (disc["rows"][:, L.P_SHAPE] != L.SHAPE_OBB).any() and boxes["A"] == 1
    plain, drift, _ = [C for _, C, _ in lad["drift_row"]]
    assert (drift["rows"][:, L.P_MODEL] == L.MODEL_DRIFT).sum() == 1 and not (plain["rows"][:, L.P_MODEL] == L.MODEL_DRIFT).any()
    table, long_, _ = [C for _, C, _ in lad["long_vehicles"]]
    diam = lambda C: np.hypot(C["rows"][:, L.P_LENGTH], C["rows"][:, L.P_WIDTH]).max()
    assert diam(long_) >= 2.5 * diam(table) and table["A"] > 64
    f0, f1 = RS.collide_want(oracle, table)[0], RS.collide_want(oracle, long_)[0]
    assert (f0 != f1).any() and (f1 & 1).sum() > (f0 & 1).sum()                                  # its cars now reach their neighbours


def test_lidar_rungs_change_the_scan(oracle):
    prev = None
    for stage, C in RS.lidar_ladder():
        scan = RS.lidar_want(oracle, C)
        assert 0.05 < np.isfinite(scan).mean() < 0.95
        if prev is not None:
            assert RS.beams_differing(prev, scan) >= 0.10, (stage, RS.beams_differing(prev, scan))
        prev = scan


def test_route_rungs_change_the_verdicts(oracle):
    prev, n_vert = None, []
    for stage, C in RS.route_ladder():
        _, off, _ = RS.off_route_want(C)
        on = C["active"] != 0
        assert 0.1 < off[on].mean() < 0.9
        if prev is not None:
            assert (off != prev).mean() >= 0.10, (stage, float((off != prev).mean()))
        prev = off
        n_vert.append(sum(len(r) for s in C["routes"]["sets"] for r in s))
        want = RS.pursuit_want(oracle, C, RS.state_of(C), np.zeros(len(on), np.float32))
        assert not (want["events"][_controlled(C)] & (8 | 2)).any()                              # nobody without a route, nothing non-finite
    assert n_vert[1] < n_vert[0] < n_vert[2] and n_vert[3] == n_vert[0]


def test_the_chain_moves_everybody_and_the_fields_not_compared_are_listed(oracle):
    C = RS.traffic(0)
    states, applied, rows = RS.episode(oracle, C)
    on = C["active"] != 0
    assert (states[-1][on, 0] != states[0][on, 0]).all() and (applied[-1][on] != 0).mean() > 0.9 and (applied[0] == 0).all()
    assert set(RS.NOT_COMPARED) == {"step_count", "record_slot", "profile"}


def test_status_stages_change_the_statuses(oracle):
    C = RS.status_scene()
    flags, _ = RS.collide_want(oracle, C)
    prev = None
    for cfg in (C["status"],) + RS.STATUS_STAGES:
        cnt, frame = np.full(C["n_env"], 3, np.int32), np.full(C["n_env"], 300, np.int32)
        st, rw = oracle.status(oracle.make_config(**cfg), C["n_env"], C["A"], flags, 100, cnt, frame)
        if prev is not None:
            assert (st != prev).any(1).sum() >= 2, (st.tolist(), prev.tolist())      # two envs and more get another status word
        prev = st
    assert RS.STATUS_STAGES[1]["max_step"] < 3 and (prev[:, 3] == 1).all()           # below cnt_step: every env is truncated


def test_the_map_queue_constant_is_the_kernel_s():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tactics2d_amd", "csrc", "t2d_mapgrid.hip")).read()
    block = int(re.search(r"constexpr int kMapBlock = (\d+);", src).group(1))
    lanes = int(re.search(r"#define T2D_MAP_LANES (\d+)", src).group(1))
    assert re.search(r"constexpr int kMapPerBlock = kMapBlock / kMapLanes;", src)
    per = int(re.search(r"constexpr int kMapQueue = (\d+) \* kMapPerBlock;", src).group(1))
    assert per * block // lanes == RS.MAP_QUEUE and block // lanes == 64


def test_the_narrowing_rung_fits_at_eight_envs_per_workgroup_only(oracle):
    ladder = RS.narrowing_ladder()
    assert [s for s, _ in ladder] == ["small", "mid", "small", "none"]
    prev = None
    for stage, C in ladder:
        flags, _ = RS.collide_want(oracle, C)
        if prev is not None:
            assert (flags != prev).mean() >= 0.10, stage
        prev = flags
        if stage == "none":
            continue
        b = RS._budget(C, C["static"], C["lanes"])
        assert b["tier"] == "lds_record" and b["envs_per_workgroup"] == 8
        # the record of 16 envs holds the polygons of two records of 8: more than the budget for G_mid, far less for G_small
        if stage == "mid":
            assert 0.6 * b["dwords_budget"] < b["dwords_needed"] <= b["dwords_budget"]
        else:
            assert 2 * b["dwords_needed"] < 0.5 * b["dwords_budget"]


def test_camera_rungs_change_the_image():
    prev = None
    for stage, sc, size, cls_of, pal in RS.camera_ladder():
        cls, rgb = RS.camera_want(sc, size, cls_of, pal)
        assert cls.shape == (5, size[1], size[0]) and len(np.unique(cls)) >= 3
        if prev is not None:
            assert RS.pixels_differing(prev, rgb) >= 0.10, (stage, RS.pixels_differing(prev, rgb))
        prev = rgb


def test_track_rungs_change_the_progress(oracle):
    prev = None
    for stage, sc in RS.track_ladder():
        visiting, visited = RS.track_want(oracle, sc)
        if prev is not None:      # a tile and more of difference in every env
            assert ((np.abs(visiting - prev[0]) >= 1) | (np.abs(visited - prev[1]) >= 1)).all(), (stage, visiting, prev)
        prev = (visiting, visited)


def test_target_stages_change_status_or_reward(oracle):
    C = RS.status_scene()
    flags, _ = RS.collide_want(oracle, C)
    xy = np.stack([C["x"][3::C["A"]], C["y"][3::C["A"]]], 1)
    prev = None
    for stage, target in RS.target_stages(C):
        ep = oracle.EpisodeState(C["n_env"], target, None, xy) if target is not None else oracle.EpisodeState(C["n_env"])
        cnt, frame = np.zeros(C["n_env"], np.int32), np.zeros(C["n_env"], np.int32)
        x = C["x"].copy(); x[3::C["A"]] += 0.5       # the ego has moved half a metre towards the first bay
        st, rw, iou = oracle.status_ex(oracle.make_config(**RS.TARGET_STATUS), C["A"], flags, 100, cnt, frame, C["rows"], x, C["y"],
                                       C["heading"], C["type_id"], ep)
        if prev is not None:
            assert ((rw != prev[1]) | (st != prev[0]).any(1)).mean() >= 0.5, (stage, rw, prev[1])
        prev = (st, rw)
