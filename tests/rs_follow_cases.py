"""The follower fixture (tests/golden/rs_follow.npz, see make_rs_follow.py) as sequences, and the specification run over them."""
import functools
import os

import numpy as np

import helpers as H
import rs_follow_ref as F

N_LOOPS = 24   # sequences 0 .. 23 are the reference's closed loops (default gains); the synthetic ones follow


@functools.lru_cache(None)
def fixture():
    with np.load(os.path.join(H.GOLD, "rs_follow.npz")) as z:
        return {k: z[k] for k in z.files}


def params(g, gains=0):
    t = g["gain_table"][gains]
    return F.Params(float(g["radius"].reshape(-1)[0]), float(g["dr"].reshape(-1)[0]), kp_v=t[0], ki_v=t[1], kd_v=t[2], kp_a=t[3], ki_a=t[4], kd_a=t[5], kp_s=t[6],
                    ki_s=t[7], kd_s=t[8])


def plan_of(g, k):
    """(steer, distance) of plan table row k, None for -1"""
    if k < 0:
        return None
    n = int(g["plan_n"][k])
    return g["plan_steer"][k, :n], g["plan_distance"][k, :n]


def sequence(g, q):
    return range(int(g["off"][q]), int(g["off"][q + 1]))
