"""Sensors on the accelerated path.

`BEVCamera` mirrors (tactics2d v0.1.9rc3) sensor/camera.py `BEVCamera` + renderer/matplotlib_renderer.py for the part a policy
consumes: the top-down semantic image of every env, one launch (t2d_camera_render), device-resident.  The view window, the
camera transform, the classes' colours and z-orders and the participant shapes are the reference's; the raster -- the class of
the topmost element under each pixel CENTRE, no anti-aliasing, no outline strokes, no road lines -- is build-defined
(DESIGN.md 4.14).

The style table below restates what MatplotlibRenderer._resolve_style gives the objects of the reference's envs
(tests/golden/camera_style.json pins it).  Note the z-order of `vehicle` and `pedestrian`: the type names of the reference's
templates ("medium_car", "adult_male") are not keys of DEFAULT_ORDER and their colours are hex strings, so _resolve_style falls
back to z-order 1 -- a car's body lies UNDER the lane it drives on, only its heading triangle shows there.
"""
import numpy as np

from . import layout as L

# class id -> name, in the order of T2D_CAMERA_CLASS_*
CLASS_NAMES = ("background", "lane", "obstacle", "target_area", "vehicle", "cyclist", "pedestrian", "heading_arrow")
# name -> (rgb, z-order); background is the figure's white
STYLE = {
    "background": ((255, 255, 255), 0),
    "lane": ((0x2F, 0x35, 0x42), 3),           # subtype "road" -> DEFAULT_COLOR "black"
    "obstacle": ((0xB2, 0xBE, 0xC3), 5),       # type_ "obstacle" -> "gray"
    "target_area": ((0xEE, 0x76, 0x6E), 1),    # ParkingLotGenerator._target_color; "target_area" has no z-order entry
    "vehicle": ((0x2B, 0xCB, 0xBA), 1),        # Vehicle._default_color; type_ "medium_car" has no z-order entry
    "cyclist": ((0xFD, 0x96, 0x44), 6),        # Cyclist._default_color; type_ "cyclist"
    "pedestrian": ((0x45, 0xAA, 0xF2), 1),     # Pedestrian._default_color; type_ "adult_male" has no z-order entry
    "heading_arrow": ((0x2F, 0x35, 0x42), 7),  # "black"
}
PALETTE = np.array([STYLE[n][0] for n in CLASS_NAMES], np.uint8)
Z_ORDER = np.array([STYLE[n][1] for n in CLASS_NAMES], np.uint8)


def perception_range_4(perception_range):
    """SensorBase.__init__ (sensor/sensor_base.py:47-59): a scalar is the range in all four directions (left, right, front,
    back).  (None -- the whole map -- needs a map boundary and is not supported here.)"""
    if perception_range is None:
        raise ValueError("perception_range=None (the whole map) is not supported: give (left, right, front, back)")
    if isinstance(perception_range, (int, float)):
        return (float(perception_range),) * 4
    r = tuple(float(v) for v in perception_range)
    if len(r) != 4:
        raise ValueError("perception_range must be a scalar or (left, right, front, back)")
    return r


def view_window(perception_range, window_size):
    """The view window as offsets from the sensor, (x_min, x_max, y_min, y_max): MatplotlibRenderer._calculate_bounds, then
    auto_scale widens the short side about the centre to the image's aspect ratio height / width
    (renderer/matplotlib_renderer.py:137-232).  window_size = (width, height) in pixels."""
    left, right, front, back = perception_range_4(perception_range)
    x0, x1, y0, y1 = -left, right, -back, front
    ww, wh = x1 - x0, y1 - y0
    cx, cy = (x0 + x1) / 2, (y0 + y1) / 2
    res_aspect = window_size[1] / window_size[0]
    if wh / ww > res_aspect:
        nw, nh = wh / res_aspect, wh
    else:
        nw, nh = ww, ww * res_aspect
    return cx - nw / 2, cx + nw / 2, cy - nh / 2, cy + nh / 2


def camera_yaw(heading, heading_up=True):
    """The camera_yaw handed to _transform_to_camera_view (which rotates the scene about the sensor by +camera_yaw): an agent
    of heading h points to the front (+y of the view) for pi / 2 - h; north-up is 0."""
    return np.pi / 2 - heading if heading_up else 0.0 * heading


class BEVCamera:
    """The BEV camera of every env of a ParticipantPool.

        cam = BEVCamera(pool, (30, 30, 50, 10))      # racing's range; window_size = (width, height) = (200, 200)
        views = cam.render(stream)                   # {"image": u8 [n_env, H, W, 3], "image_class": u8 [n_env, H, W]}

    render() launches once and returns zero-copy torch views of the library's own images: they change with the next render()
    and are valid until the camera is configured again or the pool is closed.  layers: names out of LAYERS -- a layer whose
    geometry the pool does not have makes render() raise (ERR_STATE), so name the ones the scene has.  palette / class_names
    are exposed; set_palette() changes colours.  naive=True selects the measurement yardstick (same image)."""

    LAYERS = dict(static=L.CAMERA_LAYER_STATIC, lanes=L.CAMERA_LAYER_LANES, tracks=L.CAMERA_LAYER_TRACKS,
                  target=L.CAMERA_LAYER_TARGET, participants=L.CAMERA_LAYER_PARTICIPANTS, arrows=L.CAMERA_LAYER_ARROWS)
    class_names = CLASS_NAMES

    def __init__(self, pool, perception_range, window_size=(200, 200), bind_id=0, heading_up=True, layers=("participants", "arrows"),
                 rgb=True, classes=True, naive=False):
        self.pool = pool
        self.perception_range = perception_range_4(perception_range)
        self.window_size = (int(window_size[0]), int(window_size[1]))
        self.bind_id, self.heading_up = int(bind_id), bool(heading_up)
        mask = 0
        for name in layers:
            if name not in self.LAYERS:
                raise ValueError(f"unknown layer {name!r}")
            mask |= self.LAYERS[name]
        fmt = (L.CAMERA_FORMAT_RGB if rgb else 0) | (L.CAMERA_FORMAT_CLASS if classes else 0) | (L.CAMERA_FORMAT_NAIVE if naive else 0)
        self.layers, self.format = mask, fmt
        pool.camera_config(self.window_size[0], self.window_size[1], self.perception_range, self.bind_id, self.heading_up, mask, fmt)
        # (the library keeps palette and style over a reconfiguration: a new camera object starts from the reference's)
        pool.camera_set_palette(PALETTE)
        pool.camera_set_style(None, None)
        self.palette = PALETTE.copy()
        self._views = None

    @property
    def window(self):
        """(x_min, x_max, y_min, y_max) of the view, offsets from the sensor in the camera frame."""
        return view_window(self.perception_range, self.window_size)

    def set_palette(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        self.pool.camera_set_palette(rgb)
        self.palette[:len(rgb)] = rgb

    def set_style(self, class_of_type=None, z_of_class=None):
        self.pool.camera_set_style(class_of_type, z_of_class)

    def render(self, stream=None):
        self.pool.camera_render(stream)
        if self._views is None:
            self._views = self.pool.camera_views()
        return dict(self._views)

    def render_numpy(self):
        """render(), then the images as numpy arrays (synchronises)."""
        v = self.render()
        self.pool.sync()
        return {k: t.cpu().numpy() for k, t in v.items()}
