"""Which launch every pool of a fixed list of recipes takes: tests/golden/step_forms.json.

    python tests/golden/make_step_forms.py [OUT.json]

For each recipe -- a scene of tests/test_gpu_forms.py (+ a parking pool of 4112 envs: 257 workgroups of the single-ego kernel, one
past the 256 compute units) crossed with the switches that move a pool between the forms of DESIGN.md 4.2c -- the file holds
what t2d_step_form names for calls of 1 and of 4 steps, and the template arguments of the collide_kernel instantiation that
pool.step(100) and pool.step_n(4, 100) really launched (tactics2d_amd.debug.last_step_kernel; "(false, -1, false)" = none: the
single-ego kernel, see `_Primer`).  The forms depend on the device's compute units, so their number is recorded as well.

Only the public Python API and tactics2d_amd.debug are used: the script runs unchanged on any commit, and the committed file
was written by the commit BEFORE the host's form decision moved into csrc/t2d_step_plan.h.  tests/test_gpu_step_plan.py
replays the recipes and wants every entry back: a change that moves a pool to another launch has to regenerate this file, in
the open.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_forms.json")

DEFAULT = dict(variant="fast", idm=False, chaining=1, split=1, ego_kernel=1, fused=1, auto_reset=1)
NO_LAUNCH = "(false, -1, false)"   # what the primer leaves behind: the step launched no collide_kernel at all


def recipes():
    """[(name, scene key, switches)]: every switch alone on every scene, the IDM controllers crossed with the chaining modes"""
    out = []

    def add(scene, **kw):
        sw = dict(DEFAULT, **kw)
        out.append((scene + "".join(f",{k}={v}" for k, v in sorted(kw.items())), scene, sw))

    for scene in ("highway96", "mixed96", "mixed2200", "parking64", "parking4112"):
        small = scene in ("highway96", "mixed96", "parking64")
        add(scene)
        add(scene, variant="exact")
        for mode in (0, 2, 3, 4):
            add(scene, chaining=mode)
        add(scene, fused=0)
        if small or scene == "parking4112":
            add(scene, ego_kernel=0)
        if small:
            add(scene, split=0)
            add(scene, auto_reset=0)
            add(scene, split=0, chaining=2)
        if not scene.startswith("parking"):   # (controllers drive the vehicles behind slot 0: no such slot in a one-agent env)
            add(scene, idm=True)
            add(scene, idm=True, fused=0)
            for mode in (0, 2, 3, 4) if small else (2,):
                add(scene, idm=True, chaining=mode)
    return out


def scenes():
    from tactics2d_amd import scenarios as S
    return dict(highway96=S.highway(96, 64, seed=5), mixed96=S.mixed(96, 64, seed=5), mixed2200=S.mixed(2200, 64, seed=9),
                parking64=S.parking(64, seed0=2), parking4112=S.parking(4112))


def make_pool(sc, sw):
    from tactics2d_amd import debug as D, layout as L
    from tactics2d_amd.controller import IDMController, install
    p = D.pool(sc.n_env, sc.A)
    sc.load(p)
    p.set_integrator_variant(sw["variant"])
    p.set_auto_reset(bool(sw["auto_reset"]))
    p.set_ego_kernel(bool(sw["ego_kernel"]))
    p.set_fused_step(bool(sw["fused"]))
    p.set_split_step(bool(sw["split"]))
    p.set_step_chaining(sw["chaining"])
    if sw["idm"]:   # (as tests/test_gpu_forms.py installs them)
        veh = (sc.rows[sc.type_id, L.P_MODEL] != L.MODEL_POINTMASS).reshape(sc.n_env, sc.A)
        cid = np.full((sc.n_env, sc.A), L.IDM_NONE, np.uint8)
        cid[:, 1:] = np.where(veh[:, 1:], 0, L.IDM_NONE)
        install(p, [IDMController(desired_speed=20.0, horizon=100.0)], cid.reshape(-1))
    a0, a1 = sc.sample_actions(np.random.default_rng(0))
    p.set_actions(a0, a1)
    return p


class _Primer:
    """The debug library's note of the last collide_kernel launch is one word for the process, and the single-ego kernel does
    not write it: an events-only launch of a two-env pool ahead of every step makes NO_LAUNCH what such a step leaves there,
    whatever ran earlier in the process."""

    def __init__(self):
        from tactics2d_amd import scenarios as S
        sc = S.highway(2, 2, seed=1)
        self.p = make_pool(sc, DEFAULT)

    def __call__(self):
        from tactics2d_amd import debug as D
        self.p.collide()
        assert D.last_step_kernel() == NO_LAUNCH

    def close(self):
        self.p.close()


def observe(sc, sw, primer):
    from tactics2d_amd import debug as D
    p = make_pool(sc, sw)
    try:
        got = dict(form1=p.step_form(1), form4=p.step_form(4))
        primer()
        p.step(100)
        got["kernel_step"] = D.last_step_kernel()
        primer()
        p.step_n(4, 100)
        got["kernel_step_n"] = D.last_step_kernel()
        p.sync()
    finally:
        p.close()
    return got


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def main(out=OUT):
    sc = scenes()
    primer = _Primer()
    entries = {name: observe(sc[key], sw, primer) for name, key, sw in recipes()}
    primer.close()
    with open(out, "w") as fh:
        json.dump(dict(device_cus=device_cus(), entries=entries), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(entries)} recipes -> {out}")


if __name__ == "__main__":
    main(*sys.argv[1:2])
