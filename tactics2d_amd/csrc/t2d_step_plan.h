// t2d_step_plan.h -- which form of the step kernel a pool takes: ONE decision, as a pure function of plain facts
// about the pool.  t2d_step / t2d_step_n launch from the plan and t2d_step_form reports the plan's own field (t2d_api.hip:
// step_facts fills the facts).  Host only, nothing from HIP: tests/test_step_plan.py compiles this header alone and holds every
// plan of a grid of facts against what the launchers (t2d_collide.hip, t2d_ego.hip) refuse and the kernel static_asserts.
#pragma once
#include <cstdint>

#include "../../include/t2d.h"

// the LOOP form wants every workgroup of the launch resident from the start: at most this many per CU (its launch bounds)
#ifndef T2D_LOOP_MAX_WGS_PER_CU
#define T2D_LOOP_MAX_WGS_PER_CU 2
#endif

namespace t2d {
namespace host {

inline int log2_pad(int A) {  // lanes per env = 2^l >= A, at least 2: the second lane of a one-agent env evaluates the Arrival IoU
    int l = 1;                // while the first evaluates the NoAction IoU (one SIMT pass instead of two calls in a row)
    while ((1 << l) < A) ++l;
    return l;
}

struct StepFacts {
    int n_env, A;            // envs, participant slots per env
    int epb;                 // envs per workgroup of the general kernel (GeoLayout::epb)
    int device_cus;          // compute units of the pool's device; 0 = unknown: nothing that counts on residency
    long long lane_polys;    // lane polygons of the whole pool
    bool has_geo, has_static, has_lanes;   // a geometry record, and static / lane parts in it
    bool wgmap, overlapped;  // a placement map is set (t2d_debug_set_step_placement); an env group whose launches overlap others'
    bool fused_step, grid_tier, side_models, scene_regen;
    bool ego_eligible;       // one box-shaped participant per env, no lanes, no helper models: the single-ego kernel can step it
    bool iou;                // the status configuration checks NoAction or Arrival: per-env history read by the epilogue
    bool idm_on;             // installed IDM controllers
    bool chain_steps, chain_loop, chain_pipe, chain_pipe2;   // t2d_set_step_chaining
    bool split_steps;        // t2d_set_split_step
    int chain_depth;         // -DT2D_EXPERIMENTS: steps per workgroup of the chained form (the product's is 1)
    bool shape64;            // the plain forms may take their twin compiled for 64-wide envs (a pool's default; the debug library can turn it off)
};

struct StepPlan {
    int form;          // T2D_FORM_*: what t2d_step_form reports
    bool fused;        // integrator, events and status in one launch (false: t2d_integrate + t2d_check_status)
    bool helpers;      // ... with launches of their own around it: controllers, drift, replay, scene regeneration
    bool multi;        // one launch covers the steps of a t2d_step_n fragment (false: one launch per step)
    bool ego;          // the single-ego kernel (t2d_ego.hip), not collide_kernel
    bool idm_fused;    // the step launch runs the IDM controllers itself (IDMF): no idm_kernel launch ahead of it
    bool split;        // one workgroup per env (SPLIT)
    int pipe;          // integrator waves a step ahead of the event waves (PIPE); 2 = lane waves as well
    bool loop;         // the workgroups walk through the steps themselves (LOOP)
    int real_wgs;      // workgroups of the launch that own envs
    int chain_k;       // > 1: fragments are cut to multiples of it, and a plain chained launch takes that many steps per workgroup
    bool w64;          // the launch takes the W64 twin of its form: envs of 64 participants, four per workgroup, compiled in
};

// one workgroup per CU is 64 .. 256 lanes of the general kernel, 16 envs of the single-ego kernel
constexpr int kEgoEnvsPerWorkgroup = 16;

inline StepPlan plan_step(const StepFacts& f, int n_steps) {
    StepPlan pl{};
    const int log2A = log2_pad(f.A);
    const int wgs = (f.n_env + f.epb - 1) / f.epb;
    pl.fused = f.fused_step && !f.grid_tier;
    // single-ego pools (ParkingEnv: one box-shaped participant per env, no lanes) step with one WAVE per env (t2d_ego.hip)
    // instead of one lane per participant; same arithmetic, same results (t2d_set_ego_kernel(pool, 0) keeps such a pool on the
    // general kernel: the two are held against each other in tests/test_gpu_ego.py)
    pl.ego = pl.fused && f.ego_eligible && f.A == 1;
    // a pool with installed IDM controllers whose step launch runs them itself (envs of 2..64 participants: an env's positions
    // then sit in one wave's LDS slots; no IoU events: those pools keep the general instantiations): every workgroup ahead of
    // its integrator (t2d_step, the chained form of t2d_step_n), or the integrator waves of the PIPE form where the pool is
    // small enough for it.  t2d_set_step_chaining(pool, 0, *) keeps idm_kernel a launch of its own (tests hold the two
    // against each other).
    // (not pools with SingleTrackDrift participants: drift_kernel runs between the controllers and the step launch and reads
    // the accelerations the controllers wrote -- t2d_step's order is IDM, drift, step -- so there idm_kernel stays a launch)
    pl.idm_fused = f.idm_on && f.chain_steps && pl.fused && !pl.ego && !f.side_models && f.A >= 2 && f.A <= 64 && !f.iou;
    // Replayed participants and drift rows (side_models) keep helper launches around the step, as regenerated scenes do
    pl.helpers = f.side_models || f.scene_regen || (f.idm_on && !pl.idm_fused);
    // kernels outside the fused step go step by step.  Pools with IoU events keep per-env history -- last pose, counters -- that
    // the general kernel's epilogue reads through plain pointers: one launch at a time as well (the single-ego kernel has a
    // LOOP form of its own, which reads the history with sc1 loads: IoU events are fine there)
    pl.multi = f.chain_steps && n_steps >= 2 && pl.fused && !pl.helpers && (pl.ego ? f.chain_loop : !f.iou);

    // SPLIT (one env per workgroup, its event stages on four waves): envs of 33..64 participants, workgroups of the full
    // 256 threads, no IoU events, and few enough envs for every workgroup of a step to be resident (four per CU)
    // ... and only where there is something to run side by side: envs with static obstacles next to their lanes (measured:
    // roundabout / intersection pools gain 7-10 %; a highway pool -- pairs and a few lane rectangles, nothing else -- loses 9 %
    // to the extra barriers and the poses derived four times)
    const bool split_ok = f.split_steps && !pl.ego && log2A == 6 && !f.iou && f.device_cus > 0 && f.n_env <= 4 * f.device_cus &&
                          !f.wgmap && f.has_geo && f.has_static && f.has_lanes;
    if (pl.ego) {
        pl.real_wgs = (f.n_env + kEgoEnvsPerWorkgroup - 1) / kEgoEnvsPerWorkgroup;
        pl.loop = pl.multi;   // 16 lanes per env, each group of lanes loops over the steps
        // (at most one workgroup of 16 envs per CU: integrator waves a step ahead of the event waves, t2d_ego.hip)
        pl.pipe = pl.multi && f.chain_pipe && f.device_cus > 0 && pl.real_wgs <= f.device_cus;
    } else if (!pl.multi) {
        // (one workgroup per env fills the GPU with a quarter of the envs: for a pool that has the GPU to itself, not for env
        // groups whose launches are meant to overlap -- round 4: a group of 1024 envs took every workgroup slot and the groups
        // ran one after the other, 44 us per step of 4 groups)
        pl.split = pl.fused && !pl.idm_fused && !f.overlapped && split_ok;
        pl.real_wgs = pl.split ? f.n_env : wgs;
    } else {
        // pools whose step launch is at most two workgroups per CU (all resident at once): the workgroups loop over the
        // steps themselves; larger pools chain one workgroup per (env set, step)
        const bool loop_ok = f.chain_loop && f.device_cus > 0 && wgs <= T2D_LOOP_MAX_WGS_PER_CU * f.device_cus;
        // ... and at most one workgroup per CU (envs of up to 64 participants): integrator waves a step ahead (PIPE)
        pl.pipe = loop_ok && f.chain_pipe && wgs <= f.device_cus && f.A <= 64;
        // (pools with lane polygons: the lane stage on a wave of its own -- needs three sets of waves in a workgroup)
        // -- where the lane stage is long enough to pay for the poses derived a second time: five lane polygons per env
        // and more (measured: 4 per env, the highway pool, 8.8 us per step without lane waves and 10.0 with them; 6 per
        // env 8.1 / 7.6; 4..16 per env, the mixed pool, 11.0 / 9.2)
        // (installed IDM controllers: the integrator waves run them, and there is no instantiation with lane waves as well)
        if (pl.pipe && !f.idm_on && f.chain_pipe2 && f.has_geo && f.has_lanes && f.lane_polys >= 5LL * f.n_env &&
            3 * (f.epb << log2A) <= 1024)
            pl.pipe = 2;
        // PIPE is preferred to the one-workgroup-per-env chain: the whole step overlaps, not only its stages.  Controllers
        // outside the integrator waves run in every workgroup of the plain chained form: not SPLIT, not LOOP
        pl.split = split_ok && !pl.pipe && !f.idm_on;
        pl.loop = loop_ok && !pl.split && (pl.pipe || !f.idm_on);
        pl.real_wgs = pl.split ? f.n_env : wgs;
        // the chained form of large pools, chain_depth steps per workgroup (measured in round 6 and not shipped: DESIGN.md 8.23)
        if (f.chain_loop && !f.idm_on && f.chain_depth > 1 && log2A <= 6) pl.chain_k = f.chain_depth;
    }

    pl.form = !pl.fused || pl.helpers ? T2D_FORM_UNFUSED
              : pl.ego                ? (!pl.multi ? T2D_FORM_EGO : pl.pipe ? T2D_FORM_EGO_LOOP_PIPE : T2D_FORM_EGO_LOOP)
              : !pl.multi             ? (pl.split ? T2D_FORM_STEP_SPLIT : T2D_FORM_STEP)
              : pl.pipe               ? T2D_FORM_LOOP_PIPE
              : pl.split              ? T2D_FORM_CHAIN_SPLIT
              : pl.loop               ? T2D_FORM_LOOP
                                      : T2D_FORM_CHAIN;
    // The shape of the launch (not a form of its own: t2d_step_form reports the same name).  The plain step and the plain chained
    // step -- no IoU events, no controllers inside, not SPLIT / LOOP / PIPE, one step per workgroup -- have a twin with the shape of
    // the metric pool compiled in: envs of exactly 64 participants, four of them per workgroup (a geometry record that narrows the
    // workgroup, or envs of another width, keep the generic instantiation).
    const bool plain = pl.form == T2D_FORM_STEP ? !f.iou && !pl.idm_fused : pl.form == T2D_FORM_CHAIN && !pl.idm_fused && pl.chain_k <= 1;
    pl.w64 = f.shape64 && plain && f.A == 64 && f.epb == 4;
    return pl;
}

}  // namespace host
}  // namespace t2d
