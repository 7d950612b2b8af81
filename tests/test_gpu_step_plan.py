"""Every pool of tests/golden/make_step_forms.py takes the launch it took before the form decision moved into
tactics2d_amd/csrc/t2d_step_plan.h -- tests/golden/step_forms.json was recorded by the commit before that one -- and what
t2d_step_form REPORTS is what was LAUNCHED: for every recipe on the general kernel the template arguments the debug library saw
(t2d_debug_last_step_kernel) are among those DESIGN.md 4.2c lists for the reported form.  tests/test_gpu_forms.py checks the
report and the launch sites side by side; this file ties the one to the other."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _maker():
    spec = importlib.util.spec_from_file_location("make_step_forms", os.path.join(HERE, "golden", "make_step_forms.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _args(*tails):
    """the template-argument strings "(true, V, ...)" of both integrator variants"""
    return {f"(true, {v}{t})" for v in (0, 1) for t in tails}


# form -> the instantiations of collide_kernel a call that reports it may launch.  ("unfused" is separate
# integrate + check_status launches, or any one-launch-per-step instantiation with helper launches around it: an idm_kernel
# of its own with t2d_set_step_chaining(0), drift, replay, scene regeneration.)
ONE_LAUNCH_PER_STEP = _args(", false", ", true", ", false, false, false, true")
FORM_KERNELS = {
    "unfused": {"(true, -1, false)", "(true, -1, true)"} | ONE_LAUNCH_PER_STEP,
    "step": _args(", false", ", true", ", false, false, false, false, 0, true"),
    "step_split": _args(", false, false, false, true"),
    "chain": _args(", false, true", ", false, true, false, false, 0, true"),
    "chain_split": _args(", false, true, false, true"),
    "loop": _args(", false, false, true"),
    "loop_pipe": _args(", false, false, true, false, 1", ", false, false, true, false, 2", ", false, false, true, false, 1, true"),
}
EGO_FORMS = ("ego", "ego_loop", "ego_loop_pipe")


def test_every_recipe_takes_the_launch_it_took_and_reports_it():
    m = _maker()
    want = json.load(open(os.path.join(HERE, "golden", "step_forms.json")))
    cus = m.device_cus()
    assert cus == want["device_cus"], (f"this device has {cus} compute units, tests/golden/step_forms.json was recorded on one with "
                                       f"{want['device_cus']}: the forms depend on that number -- nothing was compared")
    recipes = m.recipes()
    assert sorted(name for name, _, _ in recipes) == sorted(want["entries"])
    scenes, primer = m.scenes(), m._Primer()
    differs, unlisted = {}, {}
    for name, key, sw in recipes:
        got = m.observe(scenes[key], sw, primer)
        if got != want["entries"][name]:
            differs[name] = dict(got=got, want=want["entries"][name])
        for form, kernel in ((got["form1"], got["kernel_step"]), (got["form4"], got["kernel_step_n"])):
            if form in EGO_FORMS:   # (a body of its own, t2d_ego.hip: no collide_kernel launch at all)
                ok = kernel == m.NO_LAUNCH
            else:
                ok = kernel in FORM_KERNELS[form]
            if not ok:
                unlisted[name] = dict(form=form, kernel=kernel)
    primer.close()
    assert not differs, differs
    assert not unlisted, unlisted
    # the recipes reach every form and every row of the table
    forms = {e[k] for e in want["entries"].values() for k in ("form1", "form4")}
    assert forms == set(FORM_KERNELS) | set(EGO_FORMS), forms
