// t2d_route.hip -- the off-route detector for every participant of every env in one launch (t2d_off_route, include/t2d.h).
//
// Replaces (reference, tactics2d v0.1.9rc3):
//   OffRoute.update   traffic/event_detection/off_route.py:24-34   distance = route.distance(location); distance > threshold
//   Trajectory.get_trace   participant/trajectory/trajectory.py:151-168   (trace routes: the route IS a recorded trajectory)
//
// Two access patterns, one arithmetic (t2d_route_dev.h):
//   set routes    few polylines shared by many participants.  One workgroup per env; the vertices of the env's route set are
//                 staged once into LDS as fp32 pairs (widened on read) behind the set's route offsets (stage_route_set,
//                 t2d_scripted_dev.h: pid_kernel and pursuit_kernel stage the same way); lane a sweeps the route
//                 of participant a.  Lanes on the same route read the same LDS address in the same iteration (one broadcast
//                 8-byte read); lanes on routes of different lengths diverge in the loop's trip count only.
//   trace routes  one polyline per participant: the (x, y) of a source participant in slots first..last of a recorded
//                 trajectory.  No staging and no copy: lane i walks rows first..last of the trajectory's own x and y columns
//                 ([capacity][N_src]); with route_of = the own agent index consecutive lanes read consecutive words of a row.
//                 Small pools with long traces: G lanes per participant (off_route_trace_group_kernel).
// Both write f32 distance and u8 verdict per participant with vector stores and change no pool field.
#include "t2d_pool.h"
#include "t2d_route_dev.h"
#include "t2d_scripted_dev.h"

namespace t2d {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ bool route_live(uint32_t ids, int r, float x, float y) {
    return ((ids >> kIdsActiveShift) & 0xffu) && r >= 0 && __builtin_isfinite(x) && __builtin_isfinite(y);
}

// grid = n_env, block = max_agents rounded up to whole waves; dynamic LDS = RouteView::lds_bytes:
//   float2 verts[nv] | int32 first_vertex[nr + 1]   of the env's set (nv <= T2D_MAX_ROUTE_SET_VERTS)
__global__ __launch_bounds__(kBlock) void off_route_set_kernel(PoolView pv, RouteView rv, float* dist, uint8_t* off) {
    extern __shared__ __attribute__((aligned(16))) unsigned char route_lds[];
    const int e = blockIdx.x;
    const StagedRoutes routes = stage_route_set(route_lds, rv, e);
    const float2* lv = routes.verts;
    const int32_t* lo = routes.first;
    __syncthreads();
    const int a = threadIdx.x;
    if (a >= pv.A) return;
    const int i = e * pv.A + a;
    const uint32_t ids = pv.ids[i];
    const int r = rv.route_of[i];
    const float xf = pv.x[i], yf = pv.y[i], thr = rv.threshold[i];
    float d_out = __builtin_nanf("");
    uint8_t o = 0;
    if (route_live(ids, r, xf, yf)) {
        const double px = xf, py = yf;
        int k = lo[r];
        const int k1 = lo[r + 1];
        float2 A = lv[k];
        double d2min = __builtin_inf();
        for (++k; k < k1; ++k) {
            const float2 B = lv[k];
            const double d2 = route_seg_d2(A.x, A.y, B.x, B.y, px, py);
            if (d2 < d2min) d2min = d2;
            A = B;
        }
        route_verdict(d2min, thr, &d_out, &o);
    }
    dist[i] = d_out;
    off[i] = o;
}

// one lane per participant; rows of the trajectory's x and y columns are N_src words apart
__global__ __launch_bounds__(kBlock) void off_route_trace_kernel(PoolView pv, RouteView rv, float* dist, uint8_t* off) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= pv.N) return;
    const int e = i / pv.A;
    const uint32_t ids = pv.ids[i];
    const int r = rv.route_of[i];
    const float xf = pv.x[i], yf = pv.y[i], thr = rv.threshold[i];
    float d_out = __builtin_nanf("");
    uint8_t o = 0;
    if (route_live(ids, r, xf, yf)) {
        const int j = rv.src_env[e] * pv.A + r;
        const int first = rv.first_slot[j], last = rv.last_slot[j];
        if (last > first) {   // (a window of fewer than two slots is no polyline)
            const double px = xf, py = yf;
            const size_t N = (size_t)rv.N_src;
            const float* tx = rv.tx + (size_t)first * N + j;
            const float* ty = rv.ty + (size_t)first * N + j;
            double ax = *tx, ay = *ty;
            double d2min = __builtin_inf();
#pragma unroll 4
            for (int k = first + 1; k <= last; ++k) {
                tx += N;
                ty += N;
                const double bx = *tx, by = *ty;
                const double d2 = route_seg_d2(ax, ay, bx, by, px, py);
                if (d2 < d2min) d2min = d2;
                ax = bx;
                ay = by;
            }
            route_verdict(d2min, thr, &d_out, &o);
        }
    }
    dist[i] = d_out;
    off[i] = o;
}

// small pools with long traces (verify_states_kernel's scheme): G = 1 << log2_group consecutive lanes share one participant
// (G <= 64: a group never leaves its wave), lane r of the group takes segments r, r + G, ... of the window, and the group's
// minimum is taken over (d2, segment index) -- the smaller d2, and of equal ones the earlier segment -- which is the first
// minimum in vertex order, bit for bit what the one-lane sweep keeps.  Every lane of a wave reaches the shuffles.
__global__ __launch_bounds__(kBlock) void off_route_trace_group_kernel(PoolView pv, RouteView rv, float* dist, uint8_t* off) {
    const int lg = rv.log2_group, G = 1 << lg;
    const int r = threadIdx.x & (G - 1);
    const int i = blockIdx.x * (kBlock >> lg) + (threadIdx.x >> lg);
    const bool in = i < pv.N;
    double d2min = __builtin_inf();
    int seg = 0x7fffffff;
    bool routed = false;
    float thr = 0.f;
    if (in) {
        const int e = i / pv.A;
        const uint32_t ids = pv.ids[i];
        const int ro = rv.route_of[i];
        const float xf = pv.x[i], yf = pv.y[i];
        thr = rv.threshold[i];
        if (route_live(ids, ro, xf, yf)) {
            const int j = rv.src_env[e] * pv.A + ro;
            const int first = rv.first_slot[j], last = rv.last_slot[j];
            routed = last > first;
            const double px = xf, py = yf;
            const size_t N = (size_t)rv.N_src;
            for (int k = first + r; k < last; k += G) {   // segment k: slot k -> slot k + 1
                const float* tx = rv.tx + (size_t)k * N + j;
                const float* ty = rv.ty + (size_t)k * N + j;
                const double d2 = route_seg_d2(tx[0], ty[0], tx[N], ty[N], px, py);
                if (d2 < d2min) {
                    d2min = d2;
                    seg = k;
                }
            }
        }
    }
    for (int m = G >> 1; m > 0; m >>= 1) {
        const double od = __shfl_xor(d2min, m);
        const int os = __shfl_xor(seg, m);
        if (od < d2min || (od == d2min && os < seg)) {
            d2min = od;
            seg = os;
        }
    }
    if (in && r == 0) {
        float d_out = __builtin_nanf("");
        uint8_t o = 0;
        if (routed) route_verdict(d2min, thr, &d_out, &o);
        dist[i] = d_out;
        off[i] = o;
    }
}

}  // namespace

hipError_t launch_off_route(const PoolView& v, const RouteView& rv, float* dist, uint8_t* off, hipStream_t s) {
    if (rv.kind == 1) {
        const ScriptedLaunch l = scripted_launch(v, rv);
        hipLaunchKernelGGL(off_route_set_kernel, dim3(v.n_env), dim3(l.block), l.lds, s, v, rv, dist, off);
    } else if (rv.log2_group > 0) {
        const int per_block = kBlock >> rv.log2_group;
        hipLaunchKernelGGL(off_route_trace_group_kernel, dim3((v.N + per_block - 1) / per_block), dim3(kBlock), 0, s, v, rv, dist, off);
    } else {
        hipLaunchKernelGGL(off_route_trace_kernel, dim3((v.N + kBlock - 1) / kBlock), dim3(kBlock), 0, s, v, rv, dist, off);
    }
    return hipGetLastError();
}

}  // namespace t2d
