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


def parking_window(vehicle_size=(5.3, 2.5)):
    """(x_min, x_max, y_min, y_max) of the window every lot of the device-side ParkingLotGenerator lies in, whatever its seed
    (DESIGN.md 4.24), from the generator's own constants.  y: the back wall is at most 1.5 m deep below y = 0; the perturbed
    vehicles behind the start range stay in a box (+ 0.5 m of perturbation) that ends at y_max + slot_len + 8 with
    y_max <= 2 R + 2.4 (R: half the vehicle's diagonal; the side vehicles sit at most 1.6 m above their own lower extent) and
    slot_len <= 7.  x: the back wall and that box are 30 m wide about x = 0; the outermost side vehicle's centre lies at most
    next + max(1.6, thr + 0.8) + n_more (next + 0.8) from it (parallel lots: next = length, thr = length / 4, n_more = 2; bay
    lots: next = width, thr = 0.85, n_more = 3) and reaches R further.  Rounded outwards to whole metres."""
    ln, wd = float(vehicle_size[0]), float(vehicle_size[1])
    r = 0.5 * float(np.hypot(ln, wd))
    side = max(ln + max(1.6, 0.25 * ln + 0.8) + 2 * (ln + 0.8), wd + max(1.6, 0.85 + 0.8) + 3 * (wd + 0.8))
    half = float(np.ceil(max(15.0 + 0.5, side + r)))
    return -half, half, -2.0, float(np.ceil(2 * r + 17.4 + 0.5))


class OccupancyGrid:
    """The occupancy grid of every env of a ParticipantPool (t2d_occupancy_grid), beside BEVCamera: what the grid
    planners of `search` read in place.

        grid = OccupancyGrid(pool, 64, 64, 0.5, inflate=1.2)      # H x W cells of 0.5 m, obstacles grown by 1.2 m
        v = grid.render(stream)                                   # {"occupancy": f64 [n_env, H, W], "occupancy_mask": u8 [n_env, H, W], ...}
        out = HybridAStar.plan_batch(starts, targets, boundaries, v["occupancy"], **grid.planner_kwargs())

    The object owns its buffers: render() launches once and returns the same tensors every time (they change with the next
    render()).  origin: the centre of cell (0, 0); None centres the window on parking_window(vehicle_size), the window the lots of
    the device-side ParkingLotGenerator share.  exclude_slot None: the pool's ego index; naive=True: the measurement yardstick."""

    def __init__(self, pool, H, W, cell_size, origin=None, inflate=0.0, include_participants=False, exclude_slot=None,
                 free_weight=1.0, naive=False, vehicle_size=(5.3, 2.5)):
        import torch
        self.pool, self.H, self.W, self.cell_size = pool, int(H), int(W), float(cell_size)
        if origin is None:
            x0, x1, y0, y1 = parking_window(vehicle_size)
            origin = (0.5 * (x0 + x1) - 0.5 * (self.W - 1) * self.cell_size, 0.5 * (y0 + y1) - 0.5 * (self.H - 1) * self.cell_size)
        self.origin = (float(origin[0]), float(origin[1]))
        self.inflate, self.include_participants, self.exclude_slot = float(inflate), bool(include_participants), exclude_slot
        self.free_weight, self.naive = float(free_weight), bool(naive)
        dev = torch.device("cuda", pool.device_id)
        self.weight = torch.empty((pool.n_env, self.H, self.W), dtype=torch.float64, device=dev)
        self.mask = torch.empty((pool.n_env, self.H, self.W), dtype=torch.uint8, device=dev)
        self.hw = torch.empty((pool.n_env, 2), dtype=torch.int32, device=dev)
        self.status = torch.empty(pool.n_env, dtype=torch.int32, device=dev)
        if self.exclude_slot is None:
            self.exclude_slot = pool.status_config.ego_index if hasattr(pool, "status_config") else 0
        self._device = dev

    def planner_kwargs(self):
        """cell_size and origin as HybridAStar.plan_batch / RRT.plan_batch take them: they cannot disagree with the grid"""
        return dict(cell_size=self.cell_size, origin=self.origin)

    def render(self, stream=None):
        """One launch into the object's own tensors, asynchronous on `stream` (None: torch's current stream); returns them."""
        import torch
        p = self.pool
        st = stream if stream is not None else torch.cuda.current_stream(self._device).cuda_stream
        p._ck(p._lib.t2d_occupancy_grid(p._h, self.H, self.W, self.cell_size, self.origin[0], self.origin[1], self.inflate,
                                        int(self.include_participants), int(self.exclude_slot), self.free_weight, self.weight.data_ptr(),
                                        self.mask.data_ptr(), self.hw.data_ptr(), self.status.data_ptr(),
                                        L.OCC_FORMAT_NAIVE if self.naive else 0, st))
        return dict(occupancy=self.weight, occupancy_mask=self.mask, occupancy_hw=self.hw, occupancy_status=self.status)
