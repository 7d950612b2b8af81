"""The form decision of the step entry points (tactics2d_amd/csrc/t2d_step_plan.h: plan_step) never asks for a launch that the
launchers refuse: no GPU, the header alone, compiled with the host compiler into a small shared object that walks a grid of
facts in C++ and reports the number of violations with the first offending tuple.

What is held against every plan is NOT a second copy of the decision tree but the preconditions written where the kernels are
launched and compiled: the hipErrorInvalidValue guards of launch_step_chain / launch_collide (t2d_collide.hip), the
static_asserts at the head of collide_kernel, what SPLIT / LOOP / PIPE need to be resident, and the table of
DESIGN.md 4.2c that names a form for (ego, split, loop, pipe, multi-step, fused).

One statement is narrower here than "an unknown CU count (device_cus == 0) means no loop, pipe or split": the single-ego
kernel's multi-step form (`ego_loop`) is every group of lanes walking through the steps by itself -- it needs no resident
workgroups, has always been taken without a CU count, and the plan marks it `loop` (the launcher's v.loop_steps > 0).  The
statement is therefore made for pipe and split on both kernels and for loop on the general kernel, where LOOP does count on
residency.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tactics2d_amd", "csrc")

SHIM = r"""
#include <thread>

#include "t2d_step_plan.h"
using namespace t2d::host;

namespace {
constexpr int kBlock = 256;   // threads of a workgroup of collide_kernel without extra sets of waves (t2d_collide.hip)

int table(bool ego, bool split, bool loop, int pipe, bool multi, bool fused) {   // DESIGN.md 4.2c
    if (!fused) return T2D_FORM_UNFUSED;
    if (ego) return !multi ? T2D_FORM_EGO : pipe ? T2D_FORM_EGO_LOOP_PIPE : T2D_FORM_EGO_LOOP;
    if (!multi) return split ? T2D_FORM_STEP_SPLIT : T2D_FORM_STEP;
    if (pipe) return T2D_FORM_LOOP_PIPE;
    if (split) return T2D_FORM_CHAIN_SPLIT;
    return loop ? T2D_FORM_LOOP : T2D_FORM_CHAIN;
}

bool same(const StepPlan& a, const StepPlan& b) {
    return a.form == b.form && a.fused == b.fused && a.helpers == b.helpers && a.multi == b.multi && a.ego == b.ego &&
           a.idm_fused == b.idm_fused && a.split == b.split && a.pipe == b.pipe && a.loop == b.loop && a.real_wgs == b.real_wgs &&
           a.chain_k == b.chain_k;
}

// 0: fine; else the number of the first statement the plan breaks
int check(const StepFacts& f, int n_steps, const StepPlan& p, const StepPlan& p2) {
    const int log2A = log2_pad(f.A), cus = f.device_cus;
    const bool general_multi = p.form == T2D_FORM_CHAIN || p.form == T2D_FORM_CHAIN_SPLIT || p.form == T2D_FORM_LOOP ||
                               p.form == T2D_FORM_LOOP_PIPE;
    if (n_steps == 1 && !(p.form == T2D_FORM_UNFUSED || p.form == T2D_FORM_STEP || p.form == T2D_FORM_STEP_SPLIT || p.form == T2D_FORM_EGO))
        return 1;
    if (general_multi && !(!f.iou && f.fused_step && !f.grid_tier && !f.side_models && !f.scene_regen && f.chain_steps && n_steps >= 2))
        return 2;
    if (p.pipe > 0 && !(p.loop && !p.split && log2A <= 6 && p.real_wgs <= cus)) return 3;
    if (p.pipe > 0 && !p.ego && f.iou) return 3;   // (static_assert: PIPE = a LOOP launch without IoU events)
    if (p.pipe == 2 && !(!f.idm_on && !p.idm_fused && f.has_geo && f.has_lanes && 3 * (f.epb << log2A) <= 1024)) return 4;
    if (p.split && !(log2A == 6 && !f.iou && !p.idm_fused && !f.wgmap && f.n_env <= 4 * cus && f.has_geo && f.has_static && f.has_lanes))
        return 5;
    if (p.loop && !p.ego && !(!p.split && p.real_wgs <= 2 * cus)) return 6;
    if (p.idm_fused && !(f.A >= 2 && f.A <= 64 && !f.iou && !p.ego && !f.side_models)) return 7;
    // (static_assert: IDMF = the controller inside a PIPE = 1 launch, or ahead of the integrator of a plain or chained one)
    if (p.idm_fused && !(p.pipe == 1 || (p.pipe == 0 && !p.loop && !p.split))) return 7;
    if (p.ego && !(f.ego_eligible && (p.form == T2D_FORM_EGO || p.form == T2D_FORM_EGO_LOOP || p.form == T2D_FORM_EGO_LOOP_PIPE ||
                                      p.form == T2D_FORM_UNFUSED)))
        return 8;
    if (cus == 0 && (p.pipe || p.split || (p.loop && !p.ego))) return 9;
    if (p.form != table(p.ego, p.split, p.loop, p.pipe, p.multi, p.fused && !p.helpers)) return 10;
    if (!p.multi && (p.loop || p.pipe)) return 10;   // (one launch per step: nothing walks through steps)
    if (p.multi != (general_multi || p.form == T2D_FORM_EGO_LOOP || p.form == T2D_FORM_EGO_LOOP_PIPE)) return 10;
    if (f.chain_depth == 1 && (p.chain_k != 0 || (n_steps >= 2 && !same(p, p2)))) return 11;
    return 0;
}

struct Found {
    long long bad = 0, seen = 0;
    int first[28] = {};
};

void walk_n_env(int n_env, Found* out) {
    const int As[] = {1, 2, 32, 33, 64, 65, 128};
    const int epbs[] = {1, 2, 4, 8, 16, 32};
    const int cuss[] = {0, 256};
    const int lane_per_env[] = {0, 4, 5};
    const int steps[] = {1, 2, 4, 600};
    long long bad = 0, seen = 0;
    for (int A : As) for (int epb : epbs) {
        if ((epb << log2_pad(A)) > kBlock) continue;
        for (int cus : cuss) for (int lanes : lane_per_env) for (unsigned bits = 0; bits < (1u << 17); ++bits) {
            StepFacts f{};
            f.n_env = n_env; f.A = A; f.epb = epb; f.device_cus = cus; f.lane_polys = (long long)lanes * n_env;
            f.chain_depth = 1;
            unsigned b = bits;
            auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
            f.has_geo = next(); f.has_static = next(); f.has_lanes = next(); f.wgmap = next(); f.overlapped = next();
            f.fused_step = next(); f.grid_tier = next(); f.side_models = next(); f.scene_regen = next(); f.ego_eligible = next();
            f.iou = next(); f.idm_on = next(); f.chain_steps = next(); f.chain_loop = next(); f.chain_pipe = next();
            f.chain_pipe2 = next(); f.split_steps = next();
            const StepPlan p2 = plan_step(f, 2);
            for (int n : steps) {
                const StepPlan p = plan_step(f, n);
                const int why = check(f, n, p, p2);
                ++seen;
                if (why && !bad++) {
                    const int t[] = {f.n_env, f.A, f.epb, f.device_cus, (int)f.lane_polys, f.has_geo, f.has_static, f.has_lanes, f.wgmap,
                                     f.overlapped, f.fused_step, f.grid_tier, f.side_models, f.scene_regen, f.ego_eligible, f.iou,
                                     f.idm_on, f.chain_steps, f.chain_loop, f.chain_pipe, f.chain_pipe2, f.split_steps, n, why,
                                     p.form, p.split, p.pipe, p.real_wgs};
                    for (int k = 0; k < 28; ++k) out->first[k] = t[k];
                }
            }
        }
    }
    out->bad = bad;
    out->seen = seen;
}
}  // namespace

// out[0..27]: the first offending facts, n_steps, the statement and the plan; plans[0]: how many plans were looked at
extern "C" long long walk_grid(int* out, long long* plans) {
    const int n_envs[] = {1, 16, 96, 255, 256, 257, 512, 513, 1024, 1025, 2200, 4112};
    constexpr int kN = sizeof n_envs / sizeof *n_envs;
    Found found[kN];
    std::thread workers[kN];   // (a billion plans: one thread per pool size)
    for (int i = 0; i < kN; ++i) workers[i] = std::thread(walk_n_env, n_envs[i], &found[i]);
    long long bad = 0;
    *plans = 0;
    for (int i = 0; i < kN; ++i) {
        workers[i].join();
        if (found[i].bad && !bad)
            for (int k = 0; k < 28; ++k) out[k] = found[i].first[k];
        bad += found[i].bad;
        *plans += found[i].seen;
    }
    return bad;
}

// the plan of one set of facts (tests of single cases): f[0..22] in the order of `names` below, out = the plan's fields
extern "C" void plan_one(const int* f_in, int n_steps, int* out) {
    StepFacts f{};
    f.n_env = f_in[0]; f.A = f_in[1]; f.epb = f_in[2]; f.device_cus = f_in[3]; f.lane_polys = f_in[4];
    f.has_geo = f_in[5]; f.has_static = f_in[6]; f.has_lanes = f_in[7]; f.wgmap = f_in[8]; f.overlapped = f_in[9];
    f.fused_step = f_in[10]; f.grid_tier = f_in[11]; f.side_models = f_in[12]; f.scene_regen = f_in[13]; f.ego_eligible = f_in[14];
    f.iou = f_in[15]; f.idm_on = f_in[16]; f.chain_steps = f_in[17]; f.chain_loop = f_in[18]; f.chain_pipe = f_in[19];
    f.chain_pipe2 = f_in[20]; f.split_steps = f_in[21]; f.chain_depth = f_in[22];
    const StepPlan p = plan_step(f, n_steps);
    const int t[] = {p.form, p.fused, p.helpers, p.multi, p.ego, p.idm_fused, p.split, p.pipe, p.loop, p.real_wgs, p.chain_k};
    for (int k = 0; k < 11; ++k) out[k] = t[k];
}
"""

FACTS = ("n_env", "A", "epb", "device_cus", "lane_polys", "has_geo", "has_static", "has_lanes", "wgmap", "overlapped", "fused_step",
         "grid_tier", "side_models", "scene_regen", "ego_eligible", "iou", "idm_on", "chain_steps", "chain_loop", "chain_pipe",
         "chain_pipe2", "split_steps", "chain_depth")
PLAN = ("form", "fused", "helpers", "multi", "ego", "idm_fused", "split", "pipe", "loop", "real_wgs", "chain_k")
STATEMENTS = {1: "one step: unfused, step, step_split or ego", 2: "a multi-step form of the general kernel and its preconditions",
              3: "pipe > 0", 4: "pipe == 2", 5: "split", 6: "loop on the general kernel", 7: "idm_fused", 8: "ego",
              9: "device_cus == 0", 10: "the form is the table's", 11: "chain_depth == 1: no chain_k, one plan for every n_steps >= 2"}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("step_plan")
    src, lib = os.path.join(d, "shim.cpp"), os.path.join(d, "libstep_plan_shim.so")
    with open(src, "w") as fh:
        fh.write(SHIM)
    # (the header alone: nothing from HIP is on the include path)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-I" + CSRC, src, "-o", lib])
    so = ctypes.CDLL(lib)
    so.walk_grid.restype = ctypes.c_longlong
    so.walk_grid.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]
    so.plan_one.restype = None
    so.plan_one.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return so


def test_no_plan_asks_for_a_launch_the_launchers_refuse(shim):
    out, plans = (ctypes.c_int * 28)(), ctypes.c_longlong(0)
    bad = shim.walk_grid(out, ctypes.byref(plans))
    # 12 n_env x 26 (A, epb) pairs with epb << log2_pad(A) <= 256 x 2 device_cus x 3 lane counts x 2^17 boolean facts x 4 n_steps
    assert plans.value == 12 * 26 * 2 * 3 * 2 ** 17 * 4
    first = dict(zip(FACTS[:22] + ("n_steps", "statement", "form", "split", "pipe", "real_wgs"), list(out)))
    assert bad == 0, (bad, STATEMENTS.get(first["statement"]), first)


def _plan(shim, n_steps, **facts):
    base = dict(n_env=96, A=64, epb=1, device_cus=256, lane_polys=96 * 8, has_geo=1, has_static=1, has_lanes=1, wgmap=0, overlapped=0,
                fused_step=1, grid_tier=0, side_models=0, scene_regen=0, ego_eligible=0, iou=0, idm_on=0, chain_steps=1, chain_loop=1,
                chain_pipe=1, chain_pipe2=1, split_steps=1, chain_depth=1)
    base.update(facts)
    f, out = (ctypes.c_int * 23)(*[int(base[k]) for k in FACTS]), (ctypes.c_int * 11)()
    shim.plan_one(f, n_steps, out)
    return dict(zip(PLAN, list(out)))


def test_the_pools_of_the_form_table(shim):
    """the rows of DESIGN.md 4.2c on the facts of the pools that tests/test_gpu_forms.py drives to them (256 CUs)"""
    from tactics2d_amd.pool import ParticipantPool
    name = lambda p: ParticipantPool.STEP_FORMS[p["form"]]
    mixed = dict()                                       # 96 envs x 64, static + lanes, 8 lane polygons per env
    highway = dict(has_static=0, lane_polys=96 * 4)      # lanes only, 4 per env
    big = dict(n_env=2200, epb=4, lane_polys=2200 * 8)   # 550 workgroups: more than two per CU
    assert name(_plan(shim, 1, **highway)) == "step" and name(_plan(shim, 1, **mixed)) == "step_split"
    assert name(_plan(shim, 1, overlapped=1)) == "step"   # (env groups in flight side by side keep one wave per env)
    p = _plan(shim, 1, idm_on=1, **highway)
    assert name(p) == "step" and p["idm_fused"] and not p["split"]
    assert name(_plan(shim, 4, **big)) == "chain" and _plan(shim, 4, **big)["real_wgs"] == 550
    p = _plan(shim, 4, idm_on=1, **big)
    assert name(p) == "chain" and p["idm_fused"] and not p["loop"]
    p = _plan(shim, 4, chain_loop=0, chain_pipe=0, chain_pipe2=0)   # t2d_set_step_chaining(2)
    assert name(p) == "chain_split" and p["real_wgs"] == 96
    assert _plan(shim, 4)["pipe"] == 2 and name(_plan(shim, 4)) == "loop_pipe"
    assert _plan(shim, 4, **highway)["pipe"] == 1 and _plan(shim, 4, chain_pipe2=0)["pipe"] == 1   # (mode 4: no lane waves)
    p = _plan(shim, 4, idm_on=1)
    assert name(p) == "loop_pipe" and p["pipe"] == 1 and p["idm_fused"]
    p = _plan(shim, 4, chain_pipe=0, chain_pipe2=0, **highway)   # t2d_set_step_chaining(3)
    assert name(p) == "loop" and p["loop"] and not p["pipe"]
    assert name(_plan(shim, 4, chain_steps=0, chain_pipe=0, chain_pipe2=0)) == "step_split"   # t2d_set_step_chaining(0)
    assert name(_plan(shim, 4, iou=1, **highway)) == "step"
    for helper in ("side_models", "scene_regen"):
        assert name(_plan(shim, 4, **{helper: 1})) == "unfused"
    assert name(_plan(shim, 4, fused_step=0)) == "unfused" and name(_plan(shim, 4, grid_tier=1)) == "unfused"
    assert name(_plan(shim, 4, idm_on=1, iou=1)) == "unfused"   # (controllers in a launch of their own)
    ego = dict(A=1, epb=32, ego_eligible=1, has_lanes=0, lane_polys=0, iou=1)
    assert name(_plan(shim, 1, n_env=64, **ego)) == "ego" and name(_plan(shim, 4, n_env=64, **ego)) == "ego_loop_pipe"
    assert name(_plan(shim, 4, n_env=4096, **ego)) == "ego_loop_pipe" and name(_plan(shim, 4, n_env=4112, **ego)) == "ego_loop"
    assert name(_plan(shim, 4, n_env=64, chain_loop=0, **ego)) == "ego"
    assert name(_plan(shim, 4, n_env=64, device_cus=0, **ego)) == "ego_loop"


def test_the_chain_depth_experiment_rides_on_the_plan(shim):
    """-DT2D_EXPERIMENTS builds: chain_k is the depth for pools that may take it (no controllers, envs of at most a wave, not with
    t2d_set_step_chaining(2)) whatever the fragment's length; the product's depth of 1 never sets it"""
    big = dict(n_env=2200, epb=4, lane_polys=2200 * 8)
    assert _plan(shim, 4, chain_depth=4, **big)["chain_k"] == 4 and _plan(shim, 4, chain_depth=1, **big)["chain_k"] == 0
    assert _plan(shim, 4, chain_depth=4, idm_on=1, **big)["chain_k"] == 0
    assert _plan(shim, 4, chain_depth=4, chain_loop=0, **big)["chain_k"] == 0
    assert _plan(shim, 4, chain_depth=4, A=128, **dict(big, epb=1))["chain_k"] == 0
    assert _plan(shim, 1, chain_depth=4, **big)["chain_k"] == 0
