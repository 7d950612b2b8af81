// t2d_scripted_dev.h -- what the one-workgroup-per-env kernels of the scripted action sources share (off_route_set_kernel in
// t2d_route.hip, pid_kernel in t2d_pid.hip, pursuit_kernel in t2d_pursuit.hip): the env's route set staged in LDS, the launch
// shape, and what a lane that writes one action row and one record starts and ends with.  The laws stay in their kernels, and
// so does the commit of a finite (steering, accel): pid_kernel commits its controller state under the same condition.
#pragma once
#include <algorithm>

#include "t2d_pool.h"

namespace t2d {

constexpr int kScriptedBlock = 256;

// grid = n_env, block = max_agents rounded up to whole waves; dynamic LDS = RouteView::lds_bytes while route sets are installed
struct ScriptedLaunch {
    int block;
    size_t lds;
};
inline ScriptedLaunch scripted_launch(const PoolView& v, const RouteView& rv) {
    return {std::min(kScriptedBlock, (v.A + 63) & ~63), rv.kind == 1 ? (size_t)rv.lds_bytes : 0};
}

// The route set of env e in the launch's dynamic LDS, every lane of the workgroup taking part:
//   float2 verts[nv] | int32 first_vertex[nr + 1]   (nv <= T2D_MAX_ROUTE_SET_VERTS; fp32 pairs, widened on read)
// Route r of the set is verts[first[r] .. first[r + 1]).  The barrier before the first read stays with the caller.
struct StagedRoutes {
    const float2* verts;
    const int32_t* first;
};
__device__ __forceinline__ StagedRoutes stage_route_set(unsigned char* lds, const RouteView& rv, int e) {
    const int s = rv.set_of_env[e];
    const int r0 = rv.set_route_start[s], nr = rv.set_route_start[s + 1] - r0;
    const int v0 = rv.route_vert_off[r0], nv = rv.route_vert_off[r0 + nr] - v0;
    float2* wv = reinterpret_cast<float2*>(lds);
    int32_t* wo = reinterpret_cast<int32_t*>(lds + (size_t)nv * sizeof(float2));
    const float2* gv = reinterpret_cast<const float2*>(rv.verts) + v0;
    for (int k = threadIdx.x; k < nv; k += blockDim.x) wv[k] = gv[k];
    for (int k = threadIdx.x; k <= nr; k += blockDim.x) wo[k] = rv.route_vert_off[r0 + k] - v0;
    return {wv, wo};
}

// Lane a of env e: its participant (lanes past max_agents read nothing and are nobody's), whether it is active, and its
// controller (255 = T2D_PID_NONE = T2D_PURSUIT_NONE: the caller's row goes through).  ALSO: `also` is one more fp32 field of
// the pool that the kernel reads per participant, loaded with the rest so that all loads of the lane are in flight together.
struct ScriptedLane {
    bool valid, active;
    int i, ctrl;
    uint32_t ids;
    float x, y, heading, speed, also;
};
template <bool ALSO = false>
__device__ __forceinline__ ScriptedLane scripted_lane(const PoolView& pv, const uint8_t* ctrl_id, int e, int a,
                                                      const float* also = nullptr) {
    ScriptedLane l;
    l.valid = a < pv.A;
    l.i = e * pv.A + (l.valid ? a : 0);
    l.ids = 0;
    l.x = l.y = l.heading = l.speed = l.also = 0;
    l.ctrl = 255;
    if (l.valid) {
        l.ids = pv.ids[l.i];
        l.x = pv.x[l.i];
        l.y = pv.y[l.i];
        l.heading = pv.heading[l.i];
        l.speed = pv.speed[l.i];
        if (ALSO) l.also = also[l.i];
        l.ctrl = ctrl_id[l.i];
    }
    l.active = l.valid && ((l.ids >> kIdsActiveShift) & 0xffu);
    return l;
}

// what idm::find_leader reads of a lane: its (x, y) as fp64, NaN = inactive (idm_kernel's scheme)
__device__ __forceinline__ double2 scripted_xy(const ScriptedLane& l) {
    const double qnan = __builtin_nan("");
    return l.active ? make_double2((double)l.x, (double)l.y) : make_double2(qnan, qnan);
}

// the caller's action row of participant i (null: zeros), as bits: what an uncontrolled participant's row stays
struct ActionRow {
    uint32_t w0, w1;
};
__device__ __forceinline__ ActionRow action_row_in(const uint32_t* act_in, int i) {
    return {act_in ? act_in[2 * (size_t)i] : 0u, act_in ? act_in[2 * (size_t)i + 1] : 0u};
}
__device__ __forceinline__ void action_row_out(uint32_t* act_out, int i, ActionRow o) {
    act_out[2 * (size_t)i] = o.w0;
    act_out[2 * (size_t)i + 1] = o.w1;
}

// a parameter row's wheel base; NaN = lf + lr of the participant's type row
__device__ __forceinline__ double wheel_base_or_type(double wb, const PoolView& pv, uint32_t ids) {
    if (wb != wb) {
        const int type = (ids >> kIdsTypeShift) & 0xff;
        wb = pv.params[T2D_P_LF * T2D_MAX_TYPES + type] + pv.params[T2D_P_LR * T2D_MAX_TYPES + type];
    }
    return wb;
}

}  // namespace t2d
