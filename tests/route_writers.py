"""What the GPU tests of the three route writers share (t2d_curve_routes in test_gpu_curve_lines.py, t2d_spline_routes in
test_gpu_splines.py, t2d_planview_routes in test_gpu_road.py, and the gate of all three in test_gpu_route_writers.py): a pool of
vehicles to install route sets into, the placeholder route a writer overwrites, and the off-route reading of a pool."""
import numpy as np

N_ENV, A = 8, 4


def route_pool(x, y, heading, speed, n_env=N_ENV, agents=A):
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, full_type_table
    from tactics2d_amd.pool import ParticipantPool
    rows, names = full_type_table()
    ty = names.index(list(VEHICLE_TEMPLATE)[0] + ":kin")
    pool = ParticipantPool(n_env, agents)
    pool.set_param_table(rows)
    pool.set_status_config(max_step=100000)
    pool.reset(x, y, heading, speed, np.full(n_env * agents, ty, np.uint8))
    return pool


def placeholder(cap, e, x0=500.0):
    """`cap` vertices on a line that lies nowhere near the curves, another line for every env"""
    t = np.linspace(0.0, 95.0, cap, dtype=np.float32)
    return np.stack([x0 + t, 300.0 + 10.0 * e + 0.0 * t], 1).astype(np.float32)


def off_route(pool):
    dist, _ = pool.off_route_host()
    return dist.copy(), pool.off_route_all()[1].copy()
