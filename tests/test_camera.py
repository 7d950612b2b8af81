"""The BEV camera without a GPU: the definition (tests/camera_ref.py) against the reference renderer's own output
(tests/golden/camera.npz, made by tests/golden/make_camera.py), the product's style table and rules against what the reference's
functions gave, and the wiring of the new C ABI."""
import json
import os
import re

import numpy as np
import pytest

import camera_ref as R
from tactics2d_amd import layout as L, sensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FX = np.load(os.path.join(GOLD, "camera.npz"))
STYLE = json.load(open(os.path.join(GOLD, "camera_style.json")))
N_SCENE = len(FX["scene_name"])

BAND_PIXELS = 2.0      # output pixels around element edges left out of the colour comparison (the renderer is anti-aliased)
BAND_MAX_SHARE = 0.15  # of a scene's pixels
CHANNEL_TOL = 2


def fixture_elements(s):
    """the listing of scene s in the world frame, as camera_ref elements -- participants' body-frame geometry taken to the world
    the way MatplotlibRenderer._update_polygon does (shape @ R(rotation).T + position)"""
    out = []
    for k in range(FX["scene_elem_off"][s], FX["scene_elem_off"][s + 1]):
        if not FX["elem_drawn"][k]:   # (an id the renderer already held: make_camera.py parking_map)
            continue
        cls, z = int(FX["elem_class"][k]), int(FX["elem_z"][k])
        if FX["elem_shape"][k]:
            out.append(dict(kind="circle", cls=cls, z=z, centre=FX["elem_pos"][k], r=float(FX["elem_radius"][k])))
        else:
            g = FX["elem_xy"][FX["elem_vert_off"][k]:FX["elem_vert_off"][k + 1]]
            c, sn = np.cos(FX["elem_rot"][k]), np.sin(FX["elem_rot"][k])
            out.append(dict(kind="polygon", cls=cls, z=z, xy=g @ np.array([[c, -sn], [sn, c]]).T + FX["elem_pos"][k]))
    return out


def test_the_fixture_has_the_scenes_the_issue_names():
    names = [str(n) for n in FX["scene_name"]]
    assert N_SCENE >= 12
    assert sum(n.startswith("racing") for n in names) >= 4 and "racing_seed2_non_convex_tile" in names
    assert sum(n.startswith("parking") for n in names) >= 2
    assert any((FX["wsize"][s][0] != FX["wsize"][s][1]) for s in range(N_SCENE))
    ped = L.CAMERA_CLASS_PEDESTRIAN
    assert any(ped in FX["elem_class"][FX["scene_elem_off"][s]:FX["scene_elem_off"][s + 1]] and
               (FX["scene_elem_off"][s + 1] - FX["scene_elem_off"][s]) > 10 for s in range(N_SCENE))
    assert os.path.getsize(os.path.join(GOLD, "camera.npz")) < 512 * 1024


@pytest.mark.parametrize("s", range(N_SCENE))
def test_definition_reproduces_the_reference_renderer_away_from_edges(s):
    """camera_ref == the reference's colours within 2 per channel at every pixel farther than two output pixels from any element
    edge; that band may take at most 15 % of the scene."""
    W, H = (int(v) for v in FX["wsize"][s])
    win = (FX["xlim"][s][0], FX["xlim"][s][1], FX["ylim"][s][0], FX["ylim"][s][1])
    pix = max((win[1] - win[0]) / W, (win[3] - win[2]) / H)
    cls, dist = R.render(fixture_elements(s), (W, H), win, FX["sensor"][s], float(FX["yaw"][s]), dist_cap=BAND_PIXELS * pix + 0.1)
    keep = dist > BAND_PIXELS * pix
    share = 1.0 - keep.mean()
    palette = np.array([STYLE["style"][n]["rgb"] for n in STYLE["class_names"]], np.int32)
    diff = np.abs(palette[cls] - FX[f"rgb_{s}"].astype(np.int32)).max(axis=-1)
    bad = (diff > CHANNEL_TOL) & keep
    print(f"{FX['scene_name'][s]}: band {100 * share:.2f} % of {W * H} px, {int(bad.sum())} differ outside, "
          f"{int(((diff > CHANNEL_TOL) & ~keep).sum())} inside")
    assert share <= BAND_MAX_SHARE
    assert not bad.any()
    assert len(np.unique(cls)) >= 2   # (the scene is not empty)


def test_the_racing_fixture_scene_shows_the_non_convex_tile():
    s = [str(n) for n in FX["scene_name"]].index("racing_seed2_non_convex_tile")
    def convex(g):
        e = np.roll(g, -1, axis=0) - g
        cr = e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0]
        return not ((cr > 1e-9).any() and (cr < -1e-9).any())
    lanes = [el for el in fixture_elements(s) if el["cls"] == L.CAMERA_CLASS_LANE]
    assert any(not convex(el["xy"]) for el in lanes)


def test_the_reference_draws_the_parking_target_only_without_the_back_wall():
    """the quirk the build does NOT reproduce: the target shares the back wall's element id"""
    names = [str(n) for n in FX["scene_name"]]
    seen = {}
    for s, n in enumerate(names):
        if n.startswith("parking"):
            k = slice(FX["scene_elem_off"][s], FX["scene_elem_off"][s + 1])
            t = FX["elem_class"][k] == L.CAMERA_CLASS_TARGET
            seen[n] = (int(t.sum()), int(FX["elem_drawn"][k][t].sum()))
    assert sorted(seen.values()) == [(0, 0), (1, 0), (1, 1), (1, 1)]
    assert FX["elem_drawn"].sum() == len(FX["elem_drawn"]) - 1


# ------------------------------------------------------------------------------------------------------------ style
def test_product_style_table_equals_the_reference():
    assert list(sensor.CLASS_NAMES) == STYLE["class_names"] == list(R.CLASS_NAMES)
    for k, name in enumerate(sensor.CLASS_NAMES):
        assert list(sensor.STYLE[name][0]) == STYLE["style"][name]["rgb"], name
        assert sensor.STYLE[name][1] == STYLE["style"][name]["z"] == R.Z_ORDER[k], name
        assert list(sensor.PALETTE[k]) == STYLE["style"][name]["rgb"] and sensor.Z_ORDER[k] == STYLE["style"][name]["z"]
    # every element of every scene resolved to its class's entry
    for k in range(len(FX["elem_class"])):
        name = STYLE["class_names"][FX["elem_class"][k]]
        assert list(FX["elem_rgb"][k]) == STYLE["style"][name]["rgb"] and FX["elem_z"][k] == STYLE["style"][name]["z"]


def test_library_defaults_equal_the_style_table():
    """the defaults compiled into the library (kCamRgb / kCamZ in t2d_api.hip) and documented in the header"""
    src = open(os.path.join(ROOT, "tactics2d_amd", "csrc", "t2d_api.hip")).read()
    rgb = re.search(r"kCamRgb\[T2D_CAMERA_N_CLASS\]\[3\] = \{(.*?)\};", src, re.S).group(1)
    assert [int(v) for v in re.findall(r"\d+", rgb)] == sensor.PALETTE.ravel().tolist()
    z = re.search(r"kCamZ\[T2D_CAMERA_N_CLASS\] = \{(.*?)\};", src, re.S).group(1)
    assert [int(v) for v in re.findall(r"\d+", z)] == sensor.Z_ORDER.tolist()
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    for k, name in enumerate(sensor.CLASS_NAMES):
        c = {"target_area": "TARGET"}.get(name, name.upper())
        m = re.search(rf"#define T2D_CAMERA_CLASS_{c} (\d+)\s+/\*(.*?)\*/", header)
        assert int(m.group(1)) == k
        if k:
            assert f"z {sensor.Z_ORDER[k]}, ({', '.join(str(v) for v in sensor.PALETTE[k])})" in m.group(2), name


# ------------------------------------------------------------------------------------------------------------ rules
def test_heading_up_convention_is_the_reference_functions():
    """_transform_to_camera_view rotates about the sensor by +camera_yaw; an agent of heading h points to the front for pi/2 - h"""
    for h, front in zip(FX["probe_heading"], FX["probe_front"]):
        np.testing.assert_allclose(front, [0.0, 1.0], atol=1e-12)
        yaw = sensor.camera_yaw(h)
        assert yaw == R.camera_yaw(h) == np.pi / 2 - h
        np.testing.assert_allclose(R.to_camera_view([np.cos(h), np.sin(h)], (0.0, 0.0), yaw), front, atol=1e-12)
    y = FX["probe_yaw"].item()
    np.testing.assert_allclose(FX["probe_rot"], [np.cos(y), np.sin(y)], atol=1e-15)
    np.testing.assert_allclose(R.to_camera_view([1.0, 0.0], (0.0, 0.0), y), FX["probe_rot"], atol=1e-15)
    assert sensor.camera_yaw(1.3, heading_up=False) == 0.0
    for s in range(N_SCENE):
        assert FX["yaw"][s] in (0.0, np.pi / 2 - FX["heading"][s])


def test_window_and_aspect_rules_are_the_reference_functions():
    seen_wide = seen_tall = False
    for s in range(N_SCENE):
        W, H = (int(v) for v in FX["wsize"][s])
        pr = tuple(FX["prange"][s])
        win = R.window(pr, (W, H), FX["sensor"][s])
        np.testing.assert_allclose(win, [*FX["xlim"][s], *FX["ylim"][s]], rtol=0, atol=1e-12)
        rel = sensor.view_window(pr, (W, H))
        sx, sy = FX["sensor"][s]
        np.testing.assert_allclose([rel[0] + sx, rel[1] + sx, rel[2] + sy, rel[3] + sy], win, rtol=0, atol=1e-9)
        np.testing.assert_allclose((win[3] - win[2]) / (win[1] - win[0]), H / W, rtol=1e-12)   # the aspect rule
        seen_wide |= (win[1] - win[0]) > pr[0] + pr[1] + 1e-9
        seen_tall |= (win[3] - win[2]) > pr[2] + pr[3] + 1e-9
    assert seen_wide and seen_tall   # both branches of auto_scale were pinned
    assert sensor.perception_range_4(25.0) == tuple(FX["scalar_range"]) == sensor.perception_range_4(25)
    assert sensor.perception_range_4((1, 2, 3, 4)) == (1.0, 2.0, 3.0, 4.0)
    with pytest.raises(ValueError):
        sensor.perception_range_4((1, 2, 3))


def test_participant_shapes_are_the_reference_listing():
    """body ring and heading triangle as BEVCamera._get_participants listed them (body frame), circle for a pedestrian"""
    n_arrow = 0
    for k in range(len(FX["elem_class"])):
        cls = int(FX["elem_class"][k])
        g = FX["elem_xy"][FX["elem_vert_off"][k]:FX["elem_vert_off"][k + 1]]
        if cls in (L.CAMERA_CLASS_VEHICLE, L.CAMERA_CLASS_CYCLIST):
            length, width = 2 * g[0][0], 2 * g[1][1]
            ring, tri = R.body_ring(0.0, 0.0, 0.0, length, width)
            np.testing.assert_allclose(ring, g, atol=1e-12)
            assert int(FX["elem_class"][k + 1]) == L.CAMERA_CLASS_HEADING_ARROW      # each body is followed by its triangle
            t = FX["elem_xy"][FX["elem_vert_off"][k + 1]:FX["elem_vert_off"][k + 2]]
            np.testing.assert_allclose(tri, t, atol=1e-12)
            np.testing.assert_array_equal(FX["elem_pos"][k], FX["elem_pos"][k + 1])
            n_arrow += 1
        elif cls == L.CAMERA_CLASS_PEDESTRIAN:
            assert FX["elem_shape"][k] == 1 and FX["elem_radius"][k] > 0
    assert n_arrow > 20
    # listing order: map elements before participants, in every scene
    part = {L.CAMERA_CLASS_VEHICLE, L.CAMERA_CLASS_CYCLIST, L.CAMERA_CLASS_PEDESTRIAN, L.CAMERA_CLASS_HEADING_ARROW}
    for s in range(N_SCENE):
        c = [int(v) in part for v in FX["elem_class"][FX["scene_elem_off"][s]:FX["scene_elem_off"][s + 1]]]
        assert c == sorted(c)


def test_elements_builds_the_reference_listing_order():
    els = R.elements(target=np.zeros((4, 2)), static=[np.ones((4, 2))], lanes=[np.ones((3, 2))], tiles=[np.ones((4, 2))],
                     participants=[(0, 0, 0, R.SHAPE_OBB, 4, 2, 1, R.VEHICLE), (0, 0, 0, R.SHAPE_OBB, 4, 2, 0, R.VEHICLE),
                                   (1, 1, 0, R.SHAPE_CIRCLE, 0.8, 0.8, 1, R.PEDESTRIAN), (1, 1, 0, R.SHAPE_OBB, 2, 1, 1, R.BACKGROUND)])
    assert [e["cls"] for e in els] == [R.TARGET, R.OBSTACLE, R.LANE, R.LANE, R.VEHICLE, R.ARROW, R.PEDESTRIAN]
    assert els[-1]["r"] == 0.4


def test_topmost_is_largest_z_then_latest_listing():
    sq = lambda x0, x1: np.array([[x0, -1], [x1, -1], [x1, 1], [x0, 1]], float)
    els = [dict(kind="polygon", cls=R.OBSTACLE, z=5, xy=sq(-1, 0.5)), dict(kind="polygon", cls=R.LANE, z=3, xy=sq(-0.5, 1)),
           dict(kind="polygon", cls=R.VEHICLE, z=1, xy=sq(-2, 2)), dict(kind="polygon", cls=R.TARGET, z=1, xy=sq(1.2, 2))]
    cls, _ = R.render(els, (8, 2), (-2, 2, -0.5, 0.5), (0.0, 0.0), 0.0)
    assert cls[0].tolist() == [R.VEHICLE, R.VEHICLE, R.OBSTACLE, R.OBSTACLE, R.OBSTACLE, R.LANE, R.TARGET, R.TARGET]


# ----------------------------------------------------------------------------------------------------------- wiring
def test_header_ffi_and_layout_agree():
    from tactics2d_amd import _ffi
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {n: int(v) for n, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    assert vals["T2D_ABI_VERSION"] == 13 == L.ABI_VERSION
    cam = {n: v for n, v in vals.items() if n.startswith("T2D_CAMERA_")}
    assert len(cam) >= 20
    for n, v in cam.items():
        assert getattr(L, n[len("T2D_"):]) == v, n
    assert L.PROFILE_CAMERA == vals["T2D_PROFILE_CAMERA"]
    assert L.CAMERA_N_CLASS == len(sensor.CLASS_NAMES)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(t2d_camera_[a-z_]+)\s*\(", text))
    assert declared == {"t2d_camera_config", "t2d_camera_set_palette", "t2d_camera_set_style", "t2d_camera_render", "t2d_camera_buffers"}
    for n in declared:
        assert n in _ffi.SYMBOLS
        args = re.search(rf"\b{n}\s*\((.*?)\);", text, re.S).group(1)
        assert len(_ffi.SYMBOLS[n][1]) == args.count(",") + 1, n


def test_envs_declare_the_reference_observation_space():
    """constructing the envs needs a device; the declared space and the argument check do not"""
    from tactics2d_amd import envs
    sp = envs._camera_space()
    assert sp.shape == (200, 200, 3) and sp.dtype == np.uint8 and sp.low.min() == 0 and sp.high.max() == 255
    with pytest.raises(ValueError):
        envs._check_observation("lidar")
